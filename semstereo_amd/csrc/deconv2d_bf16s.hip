// ConvTranspose2d(Cin, Cout, 4, stride=2, padding=1) + per-channel affine (folded eval BatchNorm, or a bias as the shift) +
// optional ReLU on [B,Cin,H,W] fp32 maps -> [B,Cout,2H,2W]: the first half of every Conv2x of the reference's 2-D decoder
// (models/submodule.py:119-161: FeatUp's deconv32_16 .. deconv4_2, spx32_16 .. spx4_2) and `spx2` (models/SemStereo.py:207), on the
// two-term block-floating fp16 form of the matrix-core engine (split_f16.h: v_mfma_f32_32x32x16_f16, hi*lo + lo*hi + hi*hi, fp32
// accumulate).
//
// out[co, 2y + py, 2x + px] = sum_ci sum_{dy,dx in {0,1}} in[ci, y - 1 + py + dy, x - 1 + px + dx] * w[ci, co, 3 - py - 2 dy, 3 - px - 2 dx]:
// four output-parity classes (py, px), each a 2x2 convolution of the input with its own 4 of the 16 taps -- one GEMM per class with
// M = Cout, N = input positions, K = 4 Cin.
//
// Tile: a workgroup owns 32 output channels x (TH = 4 NT input rows) x 32 input columns of one batch element; wave w owns rows
// w NT .. w NT + NT - 1 and keeps the four classes' accumulators of each (4 NT x 16 registers).  Per 8-channel chunk the
// (TH + 2) x 34 halo tile is staged in LDS channel-innermost, split once ([term][position][8 ch] fp16: one 16-byte slot per term
// and position) and serves all four classes; a K-step of 16 is (dy, dx = lane half, 8 channels), so a class takes two K-steps = six
// MFMAs per row and chunk.  The chunk's weight fragments (4 classes x 2 steps x 2 terms x 64 lanes x 16 B = 16 KB, packed in that order
// by ss_pack_deconv2d_weights_f16s) go through LDS once per workgroup instead of once per wave.  The next chunk's activations and
// fragments are fetched into registers before the current chunk's MFMAs are issued.
//
// Stores: a lane holds both column parities of its input column, i.e. two ADJACENT output pixels of a row: one 8-byte store per lane,
// 256 contiguous bytes per 32 lanes.
#include <stdlib.h>

#include "common.h"
#include "split_f16.h"

namespace {

template <int NT>
struct DCfg {
    static constexpr int TH = 4 * NT, IH = TH + 2, IW = 34;
    static constexpr int CS = IH * IW;                         // halo positions
    static constexpr int NPOS = (CS + 255) / 256;              // positions per thread
    static constexpr int WSL = 16 * 64;                        // 16-byte slots of a chunk's weight fragments
    static constexpr int SLOTS = 2 * CS + WSL + 1;             // two operand terms + weights + the four waves' maxima
};

template <int NT>
__global__ __launch_bounds__(256, 2) void deconv2d_f16s(const float* __restrict__ in, const float* __restrict__ in2, int bsplit,
                                                        const uint4* __restrict__ wsplit, const float* __restrict__ wunscale,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        float* __restrict__ out, int Cin, int H, int W, int Cout, int tiles_w, int relu) {
    using C = DCfg<NT>;
    constexpr int WL = 2 * C::CS, MSLOT = 2 * C::CS + C::WSL;
    __shared__ __attribute__((aligned(16))) uint4 lds[C::SLOTS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int x0 = ((int)blockIdx.x % tiles_w) * 32, y0 = ((int)blockIdx.x / tiles_w) * C::TH;
    const int ct = blockIdx.y, nct = gridDim.y, b = blockIdx.z;
    const int plane = H * W;
    // (in2: batch elements bsplit, bsplit + 1, ... come from a second tensor -- the two views of FeatUp in one launch)
    const float* inb = (in2 != nullptr && b >= bsplit) ? in2 + (size_t)(b - bsplit) * Cin * plane : in + (size_t)b * Cin * plane;

    // staging plan: this thread owns halo positions p = tid + 256 i (row p / 34, column p % 34), all 8 channels of a chunk
    int poff[C::NPOS];
#pragma unroll
    for (int i = 0; i < C::NPOS; ++i) {
        const int p = tid + 256 * i;
        const int gy = y0 - 1 + p / C::IW, gx = x0 - 1 + p % C::IW;
        poff[i] = (p < C::CS && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) ? gy * W + gx : -1;
    }
    const int nchunks = (Cin + 7) / 8;
    float rin[8 * C::NPOS];
    u32x4 wpre[4];
    auto fetch = [&](int chunk) {
        const u32x4* wc = reinterpret_cast<const u32x4*>(wsplit) + ((size_t)chunk * nct + ct) * C::WSL;
#pragma unroll
        for (int i = 0; i < 4; ++i) wpre[i] = wc[tid + 256 * i];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int ch = chunk * 8 + c;
#pragma unroll
            for (int i = 0; i < C::NPOS; ++i)
                rin[c * C::NPOS + i] = (ch < Cin && poff[i] >= 0) ? inb[(size_t)ch * plane + poff[i]] : 0.f;
        }
    };
    auto publish_max = [&]() {                                 // this wave's max |rin| -> LDS (an infinity poisons its own receptive field only)
        const unsigned wm = wave_max_bits(__float_as_uint(abs_max<true>(rin, 0.f)));
        if (lane == 0) reinterpret_cast<unsigned*>(&lds[MSLOT])[wave] = wm;
    };

    f32x16 acc[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][k][r] = 0.f;

    fetch(0);
    publish_max();
    __syncthreads();
    BlockExp bexp;                                             // block-floating scale of the staged chunk (split_f16.h)
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        if (bexp.advance(lds[MSLOT])) {
            const float ratio = bexp.rescale();
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][k][r] *= ratio;
        }
        const float in_scale = bexp.in_scale();
        // ---- split + transpose: registers -> [term][position][8 ch] ----
#pragma unroll
        for (int i = 0; i < C::NPOS; ++i) {
            const int p = tid + 256 * i;
            if (p >= C::CS) continue;
            unsigned hh[4], ll[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                split2_pk_f16(rin[(2 * c) * C::NPOS + i] * in_scale, rin[(2 * c + 1) * C::NPOS + i] * in_scale, hh[c], ll[c]);
            lds[p] = make_uint4(hh[0], hh[1], hh[2], hh[3]);
            lds[C::CS + p] = make_uint4(ll[0], ll[1], ll[2], ll[3]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) lds[WL + tid + 256 * i] = make_uint4(wpre[i][0], wpre[i][1], wpre[i][2], wpre[i][3]);
        __syncthreads();
        const bool more = chunk + 1 < nchunks;
        fetch(more ? chunk + 1 : chunk);                       // (unconditional: no vector-memory instruction under a branch)
        // ---- 8 (class, dy) K-steps x NT rows x 3 products ----
#pragma unroll
        for (int cls = 0; cls < 4; ++cls) {
            const int py = cls >> 1, px = cls & 1;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const f16x8 a0 = __builtin_bit_cast(f16x8, lds[WL + ((cls * 2 + dy) * 2 + 0) * 64 + lane]);
                const f16x8 a1 = __builtin_bit_cast(f16x8, lds[WL + ((cls * 2 + dy) * 2 + 1) * 64 + lane]);
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    const int slot = (wave * NT + i + py + dy) * C::IW + l31 + px + half;      // dx = lane half
                    const f16x8 b0 = __builtin_bit_cast(f16x8, lds[slot]);
                    const f16x8 b1 = __builtin_bit_cast(f16x8, lds[C::CS + slot]);
                    acc[i][cls] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[i][cls], 0, 0, 0);      // smallest cross terms first
                    acc[i][cls] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc[i][cls], 0, 0, 0);
                    acc[i][cls] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[i][cls], 0, 0, 0);
                }
            }
        }
        if (more) publish_max();
        __syncthreads();
    }

    // ---- epilogue: 32x32 D layout (column = lane & 31 = input column, register r = channel (r & 3) + 8 (r >> 2) + 4 half) ----
    const float acc_unscale = bexp.acc_unscale();
    const int x = x0 + l31;
    const int Ho = 2 * H, Wo = 2 * W;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (co >= Cout || x >= W) continue;
        const float un = wunscale[co] * acc_unscale;           // powers of two: acc * un is exact
        const float sc = scale ? scale[co] : 1.0f, sh = shift ? shift[co] : 0.0f;
        float* oc = out + ((size_t)b * Cout + co) * Ho * Wo;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int y = y0 + wave * NT + i;
            if (y >= H) continue;
#pragma unroll
            for (int py = 0; py < 2; ++py) {
                float v0 = ss::add_rn(ss::mul_rn(acc[i][py * 2 + 0][r] * un, sc), sh);
                float v1 = ss::add_rn(ss::mul_rn(acc[i][py * 2 + 1][r] * un, sc), sh);
                if (relu) {                                    // (a NaN stays a NaN, as in F.relu)
                    v0 = v0 < 0.f ? 0.f : v0;
                    v1 = v1 < 0.f ? 0.f : v1;
                }
                *reinterpret_cast<float2*>(oc + (size_t)(2 * y + py) * Wo + 2 * x) = make_float2(v0, v1);
            }
        }
    }
}

// ConvTranspose2d weight [Cin,Cout,4,4] fp32 -> [ceil(Cin/8)][ceil(Cout/32)][4 classes][2 dy][2 terms][2 dx][32 channels][8] fp16 of
// w / wunscale[co] (zero padded), wunscale[co] = the power of two that brings max |w[:, co]| into [2^14, 2^15), stored behind the terms
// as float[32 ceil(Cout/32)].  One workgroup per (padded) output channel.
__global__ __launch_bounds__(256) void pack_deconv2d_f16s_kernel(const float* __restrict__ w, unsigned short* __restrict__ wsplit,
                                                                  float* __restrict__ wunscale, int Cin, int Cout) {
    __shared__ unsigned wmax[4];
    const int co = blockIdx.x, nct = gridDim.x / 32;
    const bool live = co < Cout;
    float m = 0.f;
    if (live)
        for (int i = threadIdx.x; i < Cin * 16; i += 256) m = fmaxf(m, fabsf(w[((size_t)(i / 16) * Cout + co) * 16 + i % 16]));
    const float u = weight_unscale(m, wmax);
    if (threadIdx.x == 0) wunscale[co] = u;
    const int nchunks = (Cin + 7) / 8, ct = co / 32, cl = co % 32;
    const int n = nchunks * 32 * 8;                            // this channel's elements: (chunk, class, dy, term, dx, j)
    for (int e = threadIdx.x; e < n; e += 256) {
        const int j = e % 8;
        int r = e / 8;
        const int dx = r % 2; r /= 2;
        const int term = r % 2; r /= 2;
        const int dy = r % 2; r /= 2;
        const int cls = r % 4;
        const int chunk = r / 4;
        const int py = cls >> 1, px = cls & 1, ci = chunk * 8 + j;
        float x = 0.f;
        if (live && ci < Cin) x = w[((size_t)ci * Cout + co) * 16 + (3 - py - 2 * dy) * 4 + (3 - px - 2 * dx)] / u;      // exact: a power of two
        const size_t i = ((((size_t)chunk * nct + ct) * 16 + (cls * 2 + dy) * 2 + term) * 64 + dx * 32 + cl) * 8 + j;
        wsplit[i] = split_weight_f16(x, term);
    }
}

// the one statement of that layout's size: DCfg::WSL 16-byte slots per (chunk, channel tile), then float[32 ceil(Cout/32)]
ss::Packed deconv2d_packed(int Cin, int Cout) {
    const long long nct = ss::ceil_div(Cout, 32), terms = ss::ceil_div(Cin, 8) * nct * DCfg<1>::WSL * 16;
    return {terms, terms + 4 * 32 * nct};
}

template <int NT>
int launch_deconv2d(const float* in, const float* in2, int bsplit, const void* wsplit, const float* scale, const float* shift, float* out,
                    int B, int Cin, int H, int W, int Cout, int relu, hipStream_t st) {
    using C = DCfg<NT>;
    const int tiles_w = ss::ceil_div(W, 32), nct = ss::ceil_div(Cout, 32);
    const long long tiles = (long long)tiles_w * ss::ceil_div(H, C::TH);
    if (tiles > 0x7fffffffLL || nct > 65535 || B > 65535) return SS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(deconv2d_f16s<NT>, dim3((unsigned)tiles, nct, B), dim3(256), 0, st, in, in2, bsplit,
                       reinterpret_cast<const uint4*>(wsplit), ss::scales_of(wsplit, deconv2d_packed(Cin, Cout)), scale, shift, out, Cin, H, W,
                       Cout, tiles_w, relu ? 1 : 0);
    return ss::check_launch();
}

int deconv2d_impl(const float* in, const float* in2, int bsplit, const void* wsplit, const float* scale, const float* shift, float* out,
                  int B, int Cin, int H, int W, int Cout, int relu, int nterms, ss_stream_t stream) {
    SS_REQUIRE(in && wsplit && out);
    SS_REQUIRE(B > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0);
    SS_REQUIRE((reinterpret_cast<uintptr_t>(wsplit) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0);
    if (nterms != F16X3) return SS_ERR_UNSUPPORTED;            // (the three-term bf16 forms of this layer are not built)
    // positions are addressed through 32-bit offsets: one batch element's input and output must stay below 2 GiB
    if ((long long)Cin * H * W * 4 >= 0x7fffffffLL || (long long)Cout * H * W * 16 >= 0x7fffffffLL) return SS_ERR_UNSUPPORTED;
    // the tile is a property of the LAYER (what one sample of it offers the chip), never of the launch's batch: the block-floating
    // scale is the tile's, so a sample gets the same bits alone, in a batch and in a pair launch
    const long long wgs8 = (long long)ss::ceil_div(W, 32) * ss::ceil_div(H, 8) * ss::ceil_div(Cout, 32);
    if (wgs8 >= 256) return launch_deconv2d<2>(in, in2, bsplit, wsplit, scale, shift, out, B, Cin, H, W, Cout, relu, ss::as_stream(stream));
    return launch_deconv2d<1>(in, in2, bsplit, wsplit, scale, shift, out, B, Cin, H, W, Cout, relu, ss::as_stream(stream));
}

}  // namespace

extern "C" int ss_deconv2d_bf16s_fwd(const float* in, const void* wsplit, const float* scale, const float* shift, float* out, int B,
                                     int Cin, int H, int W, int Cout, int relu, int nterms, ss_stream_t stream) {
    return deconv2d_impl(in, nullptr, 0, wsplit, scale, shift, out, B, Cin, H, W, Cout, relu, nterms, stream);
}

extern "C" int ss_deconv2d_bf16s_pair_fwd(const float* in_a, const float* in_b, const void* wsplit, const float* scale,
                                          const float* shift, float* out, int B, int Cin, int H, int W, int Cout, int relu, int nterms,
                                          ss_stream_t stream) {
    SS_REQUIRE(in_a && in_b && B > 0 && B <= 32767);
    return deconv2d_impl(in_a, in_b, B, wsplit, scale, shift, out, 2 * B, Cin, H, W, Cout, relu, nterms, stream);
}

extern "C" int ss_pack_deconv2d_weights_f16s(const float* w, void* wsplit, int Cin, int Cout, ss_stream_t stream) {
    SS_REQUIRE(w && wsplit && Cout > 0 && Cin > 0);
    SS_REQUIRE((reinterpret_cast<uintptr_t>(wsplit) & 15) == 0);
    hipLaunchKernelGGL(pack_deconv2d_f16s_kernel, dim3(ss::ceil_div(Cout, 32) * 32), dim3(256), 0, ss::as_stream(stream), w,
                       reinterpret_cast<unsigned short*>(wsplit), ss::scales_of(wsplit, deconv2d_packed(Cin, Cout)), Cin, Cout);
    return ss::check_launch();
}

extern "C" int ss_pack_deconv2d_weights_f16s_bytes(int Cin, int Cout, long long* bytes) {
    SS_REQUIRE(bytes && Cout > 0 && Cin > 0);
    *bytes = deconv2d_packed(Cin, Cout).total;
    return SS_OK;
}
