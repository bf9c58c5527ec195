// Conv2d(Cin, Cout, 1) + per-channel affine (the layer's bias and the eval BatchNorm folded into scale / shift) + optional ReLU on
// [B,Cin,npos] fp32 maps -> [B,Cout,npos]: the `chal_0 .. chal_4` projections of the reference (nn.Sequential(Conv2d 1x1, BatchNorm2d),
// models/SemStereo.py:213-217, called at :258-265), on the two-term block-floating fp16 form of the matrix-core engine (split_f16.h:
// v_mfma_f32_32x32x16_f16, hi*lo + lo*hi + hi*hi, fp32 accumulate).  A GEMM with M = Cout, N = positions, K = Cin.
//
// Tile: a workgroup owns 64 CONSECUTIVE positions of one batch element and 128 MT output channels (MT = 1, 2, 3: all 384 channels of
// the widest projection in one pass, so every input element comes from HBM once); wave w owns the 32-channel tiles w, w + 4, w + 8 of
// that group and both 32-position halves (2 MT accumulators of 16 registers).  The 64-position tile is fixed: it depends neither on
// the batch nor on a second input, and with it every block exponent -- a batch element has the same bits alone, in a batch and in
// the pair form.  MT is chosen from the LAYER (positions and channels of one element), see proj2d_impl.
//
// K loop: a chunk is 32 channels x 64 positions (8 KB of fp32).  Thread (position = tid & 63, octet = wave) loads 8 channels of its
// position (a wave reads 256 contiguous bytes per channel), the workgroup agrees on the chunk's block exponent, each thread splits
// its 8 values once and writes one 16-byte slot per term: LDS [term][octet][position][8 ch] fp16, 8 KB, read by all four waves --
// the waves own different output channels and share the split activations.  The weights (at most 1.2 MB for 768 -> 384) do not fit
// in registers: each wave streams the fragments of ITS channel tiles for the current chunk from L2 (4 MT 16-byte loads per lane), in
// the order ss_pack_conv2d_k1_weights_f16s wrote them.  The next chunk's activations are fetched before the MFMAs are issued.
#include <stdlib.h>

#include "common.h"
#include "split_f16.h"

namespace {

constexpr int P_TILE = 64;                                     // positions per workgroup
constexpr int P_CHUNK = 32;                                    // channels per staged chunk (two K-steps)
constexpr int P_ACT = 2 * 4 * P_TILE;                          // 16-byte slots: two terms x four octets x positions

template <int MT>
__global__ __launch_bounds__(256, 2) void proj2d_f16s(const float* __restrict__ in, const float* __restrict__ in2, int bsplit,
                                                      const uint4* __restrict__ wsplit, const float* __restrict__ wunscale,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      float* __restrict__ out, int Cin, int npos, int Cout, int nmt, int relu) {
    __shared__ __attribute__((aligned(16))) uint4 lds[P_ACT + 1];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const long long p0 = (long long)blockIdx.x * P_TILE;
    const int cg = blockIdx.y, b = blockIdx.z;
    // (in2: batch elements bsplit, bsplit + 1, ... come from a second tensor -- the two views of chal_1 / chal_2 in one launch)
    const float* inb = (in2 != nullptr && b >= bsplit) ? in2 + (size_t)(b - bsplit) * Cin * npos : in + (size_t)b * Cin * npos;

    const long long pmine = p0 + lane;                         // staging: this thread's position, octet `wave` of every chunk
    const bool pvalid = pmine < npos;
    const int nchunks = (Cin + P_CHUNK - 1) / P_CHUNK;
    float rin[8];
    auto fetch = [&](int chunk) {
        const int ch0 = chunk * P_CHUNK + wave * 8;
#pragma unroll
        for (int c = 0; c < 8; ++c) rin[c] = (pvalid && ch0 + c < Cin) ? inb[(size_t)(ch0 + c) * npos + pmine] : 0.f;
    };
    auto publish_max = [&]() {                                 // this wave's max |rin| -> LDS (an infinity poisons its own position only)
        const unsigned wm = wave_max_bits(__float_as_uint(abs_max<true>(rin, 0.f)));
        if (lane == 0) reinterpret_cast<unsigned*>(&lds[P_ACT])[wave] = wm;
    };

    // this wave's channel tiles (wave-uniform): tile index, clamped for the loads of a tile past the last one
    int mt[MT];
    bool live[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int t = cg * 4 * MT + wave + 4 * m;
        live[m] = t < nmt;
        mt[m] = live[m] ? t : nmt - 1;
    }

    f32x16 acc[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    fetch(0);
    publish_max();
    __syncthreads();
    BlockExp bexp;                                             // block-floating scale of the staged chunk (split_f16.h)
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        // this chunk's weight fragments of this wave's tiles: [chunk][tile][K-step][term][lane]
        u32x4 wf[MT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const u32x4* wc = reinterpret_cast<const u32x4*>(wsplit) + ((size_t)chunk * nmt + mt[m]) * 256 + lane;
#pragma unroll
            for (int q = 0; q < 4; ++q) wf[m][q] = wc[q * 64];
        }
        if (bexp.advance(lds[P_ACT])) {
            const float ratio = bexp.rescale();
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[m][n][r] *= ratio;
        }
        const float in_scale = bexp.in_scale();
        // ---- split: registers -> [term][octet][position][8 ch] ----
        {
            unsigned hh[4], ll[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) split2_pk_f16(rin[2 * c] * in_scale, rin[2 * c + 1] * in_scale, hh[c], ll[c]);
            lds[wave * P_TILE + lane] = make_uint4(hh[0], hh[1], hh[2], hh[3]);
            lds[4 * P_TILE + wave * P_TILE + lane] = make_uint4(ll[0], ll[1], ll[2], ll[3]);
        }
        __syncthreads();
        const bool more = chunk + 1 < nchunks;
        fetch(more ? chunk + 1 : chunk);                       // (unconditional: no vector-memory instruction under a branch)
        // ---- 2 K-steps x MT channel tiles x 2 position halves x 3 products ----
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            f16x8 b0[2], b1[2];
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int slot = (ks * 2 + half) * P_TILE + n * 32 + l31;
                b0[n] = __builtin_bit_cast(f16x8, lds[slot]);
                b1[n] = __builtin_bit_cast(f16x8, lds[4 * P_TILE + slot]);
            }
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                if (!live[m]) continue;                        // (wave-uniform)
                const f16x8 a0 = __builtin_bit_cast(f16x8, wf[m][ks * 2 + 0]);
                const f16x8 a1 = __builtin_bit_cast(f16x8, wf[m][ks * 2 + 1]);
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1[n], acc[m][n], 0, 0, 0);      // smallest cross terms first
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0[n], acc[m][n], 0, 0, 0);
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0[n], acc[m][n], 0, 0, 0);
            }
        }
        if (more) publish_max();
        __syncthreads();
    }

    // ---- epilogue: 32x32 D layout (column = lane & 31 = position, register r = channel (r & 3) + 8 (r >> 2) + 4 half) ----
    const float acc_unscale = bexp.acc_unscale();
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if (!live[m]) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = mt[m] * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (co >= Cout) continue;
            const float un = wunscale[co] * acc_unscale;       // powers of two: acc * un is exact
            const float sc = scale ? scale[co] : 1.0f, sh = shift ? shift[co] : 0.0f;
            float* oc = out + ((size_t)b * Cout + co) * npos;
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const long long p = p0 + n * 32 + l31;
                if (p >= npos) continue;
                float v = ss::add_rn(ss::mul_rn(acc[m][n][r] * un, sc), sh);
                if (relu) v = v < 0.f ? 0.f : v;               // (a NaN stays a NaN, as in F.relu)
                oc[p] = v;
            }
        }
    }
}

// Conv2d weight [Cout,Cin] fp32 -> [ceil(Cin/32)][ceil(Cout/32)][2 K-steps][2 terms][2 channel octets][32 output channels][8] fp16 of
// w / wunscale[co] (zero padded), wunscale[co] = the power of two that brings max |w[co, :]| into [2^14, 2^15), stored behind the terms
// as float[32 ceil(Cout/32)].  One workgroup per (padded) output channel.
__global__ __launch_bounds__(256) void pack_proj2d_f16s_kernel(const float* __restrict__ w, unsigned short* __restrict__ wsplit,
                                                                float* __restrict__ wunscale, int Cout, int Cin) {
    __shared__ unsigned wmax[4];
    const int co = blockIdx.x, nmt = gridDim.x / 32;
    const bool live = co < Cout;
    float m = 0.f;
    if (live)
        for (int i = threadIdx.x; i < Cin; i += 256) m = fmaxf(m, fabsf(w[(size_t)co * Cin + i]));
    const float u = weight_unscale(m, wmax);
    if (threadIdx.x == 0) wunscale[co] = u;
    const int nchunks = (Cin + P_CHUNK - 1) / P_CHUNK, t = co / 32, cl = co % 32;
    const int n = nchunks * 2 * 2 * 2 * 8;                     // this channel's elements: (chunk, K-step, term, octet, j)
    for (int e = threadIdx.x; e < n; e += 256) {
        const int j = e % 8;
        int r = e / 8;
        const int oct = r % 2; r /= 2;
        const int term = r % 2; r /= 2;
        const int ks = r % 2;
        const int chunk = r / 2;
        const int ci = chunk * P_CHUNK + ks * 16 + oct * 8 + j;
        float x = 0.f;
        if (live && ci < Cin) x = w[(size_t)co * Cin + ci] / u;                 // exact: a power of two
        const size_t i = ((((size_t)chunk * nmt + t) * 4 + ks * 2 + term) * 64 + oct * 32 + cl) * 8 + j;
        wsplit[i] = split_weight_f16(x, term);
    }
}

// the one statement of that layout's size: 256 16-byte slots per (chunk, channel tile), then float[32 ceil(Cout/32)]
ss::Packed proj2d_packed(int Cout, int Cin) {
    const long long nmt = ss::ceil_div(Cout, 32), terms = ss::ceil_div(Cin, P_CHUNK) * nmt * 256 * 16;
    return {terms, terms + 4 * 32 * nmt};
}

template <int MT>
int launch_proj2d(const float* in, const float* in2, int bsplit, const void* wsplit, const float* scale, const float* shift, float* out,
                  int B, int Cin, long long npos, int Cout, int relu, hipStream_t st) {
    const int nmt = ss::ceil_div(Cout, 32), groups = ss::ceil_div(nmt, 4 * MT);
    const long long tiles = ss::ceil_div_ll(npos, P_TILE);
    if (tiles > 0x7fffffffLL || groups > 65535 || B > 65535) return SS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(proj2d_f16s<MT>, dim3((unsigned)tiles, groups, B), dim3(256), 0, st, in, in2, bsplit,
                       reinterpret_cast<const uint4*>(wsplit), ss::scales_of(wsplit, proj2d_packed(Cout, Cin)), scale, shift, out, Cin,
                       (int)npos, Cout, nmt, relu ? 1 : 0);
    return ss::check_launch();
}

int proj2d_impl(const float* in, const float* in2, int bsplit, const void* wsplit, const float* scale, const float* shift, float* out,
                int B, int Cin, long long npos, int Cout, int relu, ss_stream_t stream) {
    SS_REQUIRE(in && wsplit && out);
    SS_REQUIRE(B > 0 && Cin > 0 && npos > 0 && Cout > 0);
    SS_REQUIRE((reinterpret_cast<uintptr_t>(wsplit) & 15) == 0);
    if (Cin % 8 != 0) return SS_ERR_UNSUPPORTED;               // (a thread stages whole channel octets)
    // positions are addressed through 32-bit offsets: one batch element's input and output must stay below 2 GiB
    if ((long long)Cin * npos * 4 >= 0x7fffffffLL || (long long)Cout * npos * 4 >= 0x7fffffffLL) return SS_ERR_UNSUPPORTED;
    // Channel tiles per wave: a property of the LAYER (what one element of it offers the chip), never of the launch's batch.  A map
    // with at least 256 position tiles keeps all its channels (up to 384) in one workgroup, so each input element is read once; a
    // smaller one (the 1/16 and 1/32 levels, L2-resident) spreads its channel groups of 128 over more workgroups instead.
    const int nmt = ss::ceil_div(Cout, 32);
    const int want = ss::ceil_div_ll(npos, P_TILE) >= 256 ? (nmt > 8 ? 3 : (nmt > 4 ? 2 : 1)) : 1;
    hipStream_t st = ss::as_stream(stream);
    if (want == 3) return launch_proj2d<3>(in, in2, bsplit, wsplit, scale, shift, out, B, Cin, npos, Cout, relu, st);
    if (want == 2) return launch_proj2d<2>(in, in2, bsplit, wsplit, scale, shift, out, B, Cin, npos, Cout, relu, st);
    return launch_proj2d<1>(in, in2, bsplit, wsplit, scale, shift, out, B, Cin, npos, Cout, relu, st);
}

}  // namespace

extern "C" int ss_conv2d_k1_f16s_fwd(const float* in, const void* wsplit, const float* scale, const float* shift, float* out, int B,
                                     int Cin, long long npos, int Cout, int relu, ss_stream_t stream) {
    return proj2d_impl(in, nullptr, 0, wsplit, scale, shift, out, B, Cin, npos, Cout, relu, stream);
}

extern "C" int ss_conv2d_k1_f16s_pair_fwd(const float* in_a, const float* in_b, const void* wsplit, const float* scale,
                                          const float* shift, float* out, int B, int Cin, long long npos, int Cout, int relu,
                                          ss_stream_t stream) {
    SS_REQUIRE(in_a && in_b && B > 0 && B <= 32767);
    return proj2d_impl(in_a, in_b, B, wsplit, scale, shift, out, 2 * B, Cin, npos, Cout, relu, stream);
}

extern "C" int ss_pack_conv2d_k1_weights_f16s(const float* w, void* wsplit, int Cout, int Cin, ss_stream_t stream) {
    SS_REQUIRE(w && wsplit && Cout > 0 && Cin > 0);
    SS_REQUIRE((reinterpret_cast<uintptr_t>(wsplit) & 15) == 0);
    hipLaunchKernelGGL(pack_proj2d_f16s_kernel, dim3(ss::ceil_div(Cout, 32) * 32), dim3(256), 0, ss::as_stream(stream), w,
                       reinterpret_cast<unsigned short*>(wsplit), ss::scales_of(wsplit, proj2d_packed(Cout, Cin)), Cout, Cin);
    return ss::check_launch();
}

extern "C" int ss_pack_conv2d_k1_weights_f16s_bytes(int Cout, int Cin, long long* bytes) {
    SS_REQUIRE(bytes && Cout > 0 && Cin > 0);
    *bytes = proj2d_packed(Cout, Cin).total;
    return SS_OK;
}
