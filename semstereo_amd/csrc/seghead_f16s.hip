// The segmentation head of the reference -- segmenthead (models/submodule.py:31-52): BasicConv(Cin -> 32, 3x3, BatchNorm, ReLU) ->
// Conv2d(32 -> K, 1x1, bias) -> bilinear x2; `head_l` / `head_r`, models/SemStereo.py:200-201, 254-255 -- without its 32-channel map.
//
// Launch 1 (seghead_logits): the 3x3 conv on the two-term block-floating fp16 form of the matrix-core engine (split_f16.h:
// v_mfma_f32_32x32x16_f16, hi*lo + lo*hi + hi*hi, fp32 accumulate) with M = the 32 intermediate channels, so a workgroup's
// accumulators hold ALL channels of its positions; the folded BatchNorm, the ReLU and the 32 -> K contraction with its bias are
// applied to them in fp32 (16 channels in a lane, the other 16 in the lane 32 further on: one cross-lane add per class), and only
// the K logit planes are written, at the input's resolution.
//
// Tile: 8 rows x 32 columns of one batch element, fixed (it depends on nothing but the position, so a batch element has the same bits
// alone and in a batch); wave w owns rows 2 w, 2 w + 1.  Per 8-channel chunk the 10 x 34 halo tile is staged in LDS channel-innermost,
// split once ([term][position][8 ch] fp16) and serves all nine taps; a K-step of 16 is (2 taps = lane half, 8 channels), five
// K-steps per chunk, the tenth tap's weights being zero (its activations are read from the ninth tap's slot: inside the receptive
// field).  The chunk's weight fragments (5 K-steps x 2 terms x 64 lanes x 16 B = 10 KB) go through LDS once per workgroup.  The
// next chunk's activations and fragments are fetched into registers before the current chunk's MFMAs are issued.
//
// Launch 2 (bilinear_up2): F.interpolate(size = (2H, 2W), mode = "bilinear", align_corners = False) of the logits: weights 0.25 / 0.75
// with the source index clamped at the borders, the horizontal pair first, then the vertical one; each pair is one fused
// multiply-add on an exact product, so a constant map comes back unchanged.  A thread owns two input columns = four adjacent
// output pixels of two output rows: 16-byte stores (even W; odd W stores scalars, its rows are not 16-byte aligned).
#include <stdlib.h>

#include "common.h"
#include "split_f16.h"

namespace {

constexpr int H_NT = 2, H_TH = 4 * H_NT, H_IH = H_TH + 2, H_IW = 34;
constexpr int H_CS = H_IH * H_IW;                              // halo positions
constexpr int H_NPOS = (H_CS + 255) / 256;                     // positions per thread
constexpr int H_WSL = 5 * 2 * 64;                              // 16-byte slots of a chunk's weight fragments
constexpr int H_WPT = (H_WSL + 255) / 256;                     // ... per thread
constexpr int H_SLOTS = 2 * H_CS + H_WSL + 1;                  // two operand terms + weights + the four waves' maxima
constexpr int H_KMAX = 8;                                      // classes

__global__ __launch_bounds__(256, 2) void seghead_logits_f16s(const float* __restrict__ in, const uint4* __restrict__ wsplit,
                                                              const float* __restrict__ wunscale, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, const float* __restrict__ w2,
                                                              const float* __restrict__ bias, float* __restrict__ out, int Cin, int H,
                                                              int W, int K, int tiles_w) {
    constexpr int WL = 2 * H_CS, MSLOT = 2 * H_CS + H_WSL;
    __shared__ __attribute__((aligned(16))) uint4 lds[H_SLOTS];
    __shared__ float w2s[H_KMAX * 32];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int x0 = ((int)blockIdx.x % tiles_w) * 32, y0 = ((int)blockIdx.x / tiles_w) * H_TH;
    const int b = blockIdx.y;
    const int plane = H * W;
    const float* inb = in + (size_t)b * Cin * plane;

    w2s[tid] = tid < K * 32 ? w2[tid] : 0.f;                   // (read after the K loop's barriers)

    // staging plan: this thread owns halo positions p = tid + 256 i (row p / 34, column p % 34), all 8 channels of a chunk
    int poff[H_NPOS];
#pragma unroll
    for (int i = 0; i < H_NPOS; ++i) {
        const int p = tid + 256 * i;
        const int gy = y0 - 1 + p / H_IW, gx = x0 - 1 + p % H_IW;
        poff[i] = (p < H_CS && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) ? gy * W + gx : -1;
    }
    const int nchunks = Cin / 8;
    float rin[8 * H_NPOS];
    u32x4 wpre[H_WPT];
    auto fetch = [&](int chunk) {
        const u32x4* wc = reinterpret_cast<const u32x4*>(wsplit) + (size_t)chunk * H_WSL;
#pragma unroll
        for (int i = 0; i < H_WPT; ++i) wpre[i] = wc[min(tid + 256 * i, H_WSL - 1)];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int ch = chunk * 8 + c;
#pragma unroll
            for (int i = 0; i < H_NPOS; ++i) rin[c * H_NPOS + i] = poff[i] >= 0 ? inb[(size_t)ch * plane + poff[i]] : 0.f;
        }
    };
    auto publish_max = [&]() {                                 // this wave's max |rin| -> LDS (an infinity poisons its own receptive field only)
        const unsigned wm = wave_max_bits(__float_as_uint(abs_max<true>(rin, 0.f)));
        if (lane == 0) reinterpret_cast<unsigned*>(&lds[MSLOT])[wave] = wm;
    };

    // K-step ks, lane half -> tap 2 ks + half (the tenth: the ninth's slot, zero weights): its offset in the halo tile
    int tapoff[5];
#pragma unroll
    for (int ks = 0; ks < 5; ++ks) {
        const int t = min(2 * ks + half, 8);
        tapoff[ks] = (t / 3) * H_IW + t % 3;
    }

    f32x16 acc[H_NT];
#pragma unroll
    for (int i = 0; i < H_NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    fetch(0);
    publish_max();
    __syncthreads();
    BlockExp bexp;                                             // block-floating scale of the staged chunk (split_f16.h)
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        if (bexp.advance(lds[MSLOT])) {
            const float ratio = bexp.rescale();
#pragma unroll
            for (int i = 0; i < H_NT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][r] *= ratio;
        }
        const float in_scale = bexp.in_scale();
        // ---- split + transpose: registers -> [term][position][8 ch] ----
#pragma unroll
        for (int i = 0; i < H_NPOS; ++i) {
            const int p = tid + 256 * i;
            if (p >= H_CS) continue;
            unsigned hh[4], ll[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                split2_pk_f16(rin[(2 * c) * H_NPOS + i] * in_scale, rin[(2 * c + 1) * H_NPOS + i] * in_scale, hh[c], ll[c]);
            lds[p] = make_uint4(hh[0], hh[1], hh[2], hh[3]);
            lds[H_CS + p] = make_uint4(ll[0], ll[1], ll[2], ll[3]);
        }
#pragma unroll
        for (int i = 0; i < H_WPT; ++i)
            if (tid + 256 * i < H_WSL) lds[WL + tid + 256 * i] = make_uint4(wpre[i][0], wpre[i][1], wpre[i][2], wpre[i][3]);
        __syncthreads();
        const bool more = chunk + 1 < nchunks;
        fetch(more ? chunk + 1 : chunk);                       // (unconditional: no vector-memory instruction under a branch)
        // ---- 5 K-steps (two taps each) x 2 rows x 3 products ----
#pragma unroll
        for (int ks = 0; ks < 5; ++ks) {
            const f16x8 a0 = __builtin_bit_cast(f16x8, lds[WL + (ks * 2 + 0) * 64 + lane]);
            const f16x8 a1 = __builtin_bit_cast(f16x8, lds[WL + (ks * 2 + 1) * 64 + lane]);
#pragma unroll
            for (int i = 0; i < H_NT; ++i) {
                const int slot = (wave * H_NT + i) * H_IW + l31 + tapoff[ks];
                const f16x8 b0 = __builtin_bit_cast(f16x8, lds[slot]);
                const f16x8 b1 = __builtin_bit_cast(f16x8, lds[H_CS + slot]);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[i], 0, 0, 0);      // smallest cross terms first
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[i], 0, 0, 0);
            }
        }
        if (more) publish_max();
        __syncthreads();
    }

    // ---- epilogue: 32x32 D layout (column = lane & 31 = input column, register r = channel (r & 3) + 8 (r >> 2) + 4 half) ----
    const float acc_unscale = bexp.acc_unscale();
    const int x = x0 + l31;
    float part[H_NT][H_KMAX];
#pragma unroll
    for (int i = 0; i < H_NT; ++i)
#pragma unroll
        for (int k = 0; k < H_KMAX; ++k) part[i][k] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int c = (r & 3) + 8 * (r >> 2) + 4 * half;
        const float un = wunscale[c] * acc_unscale;            // powers of two: acc * un is exact
        const float sc = scale ? scale[c] : 1.0f, sh = shift ? shift[c] : 0.0f;
#pragma unroll
        for (int i = 0; i < H_NT; ++i) {
            float v = ss::add_rn(ss::mul_rn(acc[i][r] * un, sc), sh);
            v = v < 0.f ? 0.f : v;                             // (a NaN stays a NaN, as in F.relu)
#pragma unroll
            for (int k = 0; k < H_KMAX; ++k) part[i][k] = fmaf(w2s[k * 32 + c], v, part[i][k]);
        }
    }
#pragma unroll
    for (int i = 0; i < H_NT; ++i) {
        const int y = y0 + wave * H_NT + i;
#pragma unroll
        for (int k = 0; k < H_KMAX; ++k) {
            const float other = __shfl_xor(part[i][k], 32);   // the other 16 channels
            if (k < K && (k & 1) == half && y < H && x < W)
                out[(((size_t)b * K + k) * H + y) * W + x] = (part[i][k] + other) + bias[k];
        }
    }
}

// Conv2d weight [32,Cin,3,3] fp32 -> [Cin/8][5 K-steps][2 terms][2 taps][32 channels][8] fp16 of w / wunscale[co] (tap 2 ks + lane
// half; the tenth tap zero), wunscale[co] = the power of two that brings max |w[co]| into [2^14, 2^15), stored behind the terms as
// float[32].  One workgroup per intermediate channel.
__global__ __launch_bounds__(256) void pack_seghead_f16s_kernel(const float* __restrict__ w, unsigned short* __restrict__ wsplit,
                                                                 float* __restrict__ wunscale, int Cin) {
    __shared__ unsigned wmax[4];
    const int co = blockIdx.x;
    float m = 0.f;
    for (int i = threadIdx.x; i < Cin * 9; i += 256) m = fmaxf(m, fabsf(w[(size_t)co * Cin * 9 + i]));
    const float u = weight_unscale(m, wmax);
    if (threadIdx.x == 0) wunscale[co] = u;
    const int n = (Cin / 8) * 5 * 2 * 2 * 8;                   // this channel's elements: (chunk, K-step, term, tap half, j)
    for (int e = threadIdx.x; e < n; e += 256) {
        const int j = e % 8;
        int r = e / 8;
        const int hf = r % 2; r /= 2;
        const int term = r % 2; r /= 2;
        const int ks = r % 5;
        const int chunk = r / 5;
        const int tap = 2 * ks + hf, ci = chunk * 8 + j;
        float x = 0.f;
        if (tap < 9) x = w[((size_t)co * Cin + ci) * 9 + tap] / u;             // exact: a power of two
        const size_t i = ((((size_t)chunk * 5 + ks) * 2 + term) * 64 + hf * 32 + co) * 8 + j;
        wsplit[i] = split_weight_f16(x, term);
    }
}

// one thread: input columns 2 j, 2 j + 1 of row y -> output columns 4 j .. 4 j + 3 of rows 2 y, 2 y + 1
template <bool VEC>
__global__ __launch_bounds__(256) void bilinear_up2_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                            int pairs, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx % pairs);
    const long long t = idx / pairs;
    const int y = (int)(t % H);
    const long long bc = t / H;
    const float* ip = in + (size_t)bc * H * W;
    float* op = out + (size_t)bc * 4 * H * W;
    const int xa = 2 * j, xb = min(2 * j + 1, W - 1);
    const int xl = max(xa - 1, 0), xr = min(xb + 1, W - 1);
    const int ys[3] = {max(y - 1, 0), y, min(y + 1, H - 1)};
    float h[3][4];                                             // the horizontal pair of rows y - 1, y, y + 1
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float* row = ip + (size_t)ys[q] * W;
        const float vl = row[xl], va = row[xa], vb = row[xb], vr = row[xr];
        h[q][0] = fmaf(va, 0.75f, vl * 0.25f);
        h[q][1] = fmaf(va, 0.75f, vb * 0.25f);
        h[q][2] = fmaf(vb, 0.75f, va * 0.25f);
        h[q][3] = fmaf(vb, 0.75f, vr * 0.25f);
    }
    float o[2][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        o[0][c] = fmaf(h[1][c], 0.75f, h[0][c] * 0.25f);
        o[1][c] = fmaf(h[1][c], 0.75f, h[2][c] * 0.25f);
    }
    const int Wo = 2 * W;
#pragma unroll
    for (int py = 0; py < 2; ++py) {
        float* orow = op + (size_t)(2 * y + py) * Wo + 4 * j;
        if (VEC) {
            *reinterpret_cast<float4*>(orow) = make_float4(o[py][0], o[py][1], o[py][2], o[py][3]);
        } else {
            orow[0] = o[py][0];
            orow[1] = o[py][1];
            if (2 * j + 1 < W) {
                orow[2] = o[py][2];
                orow[3] = o[py][3];
            }
        }
    }
}

}  // namespace

// the one statement of the packed conv1 weights' size: H_WSL 16-byte slots per chunk of 8 input channels, then float[32]
static ss::Packed seghead_packed(int Cin) {
    const long long terms = (long long)(Cin / 8) * H_WSL * 16;
    return {terms, terms + 4 * 32};
}

extern "C" int ss_pack_seghead_weights_f16s(const float* w, void* wsplit, int Cin, ss_stream_t stream) {
    SS_REQUIRE(w && wsplit && Cin > 0 && Cin % 8 == 0);
    SS_REQUIRE((reinterpret_cast<uintptr_t>(wsplit) & 15) == 0);
    hipLaunchKernelGGL(pack_seghead_f16s_kernel, dim3(32), dim3(256), 0, ss::as_stream(stream), w,
                       reinterpret_cast<unsigned short*>(wsplit), ss::scales_of(wsplit, seghead_packed(Cin)), Cin);
    return ss::check_launch();
}

extern "C" int ss_pack_seghead_weights_f16s_bytes(int Cin, long long* bytes) {
    SS_REQUIRE(bytes && Cin > 0 && Cin % 8 == 0);
    *bytes = seghead_packed(Cin).total;
    return SS_OK;
}

extern "C" int ss_seghead_logits_fwd(const float* in, const void* wsplit, const float* scale, const float* shift, const float* w2,
                                     const float* bias, float* out, int B, int Cin, int H, int W, int K, ss_stream_t stream) {
    SS_REQUIRE(in && wsplit && w2 && bias && out);
    SS_REQUIRE(B > 0 && Cin > 0 && H > 0 && W > 0 && K > 0);
    SS_REQUIRE((reinterpret_cast<uintptr_t>(wsplit) & 15) == 0);
    if (Cin % 8 != 0 || K > H_KMAX) return SS_ERR_UNSUPPORTED;
    // positions are addressed through 32-bit offsets: one batch element's input must stay below 2 GiB
    if ((long long)Cin * H * W * 4 >= 0x7fffffffLL) return SS_ERR_UNSUPPORTED;
    const int tiles_w = ss::ceil_div(W, 32);
    const long long tiles = (long long)tiles_w * ss::ceil_div(H, H_TH);
    if (tiles > 0x7fffffffLL || B > 65535) return SS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(seghead_logits_f16s, dim3((unsigned)tiles, B), dim3(256), 0, ss::as_stream(stream), in,
                       reinterpret_cast<const uint4*>(wsplit), ss::scales_of(wsplit, seghead_packed(Cin)), scale, shift, w2, bias, out, Cin, H,
                       W, K, tiles_w);
    return ss::check_launch();
}

extern "C" int ss_bilinear_up2_fwd(const float* in, float* out, int B, int C, int H, int W, ss_stream_t stream) {
    SS_REQUIRE(in && out);
    SS_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0);
    const int pairs = ss::ceil_div(W, 2);
    const long long total = (long long)B * C * H * pairs;
    const long long blocks = ss::ceil_div_ll(total, 256);
    if (blocks > 0x7fffffffLL) return SS_ERR_UNSUPPORTED;
    const bool vec = W % 2 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(bilinear_up2_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, ss::as_stream(stream), in, out, H, W, pairs, total);
    else
        hipLaunchKernelGGL(bilinear_up2_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, ss::as_stream(stream), in, out, H, W, pairs, total);
    return ss::check_launch();
}
