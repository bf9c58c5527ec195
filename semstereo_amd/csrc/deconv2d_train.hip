// The two adjoints of ConvTranspose2d(Cin, Cout, 4, stride=2, padding=1) -- conv1 of every 2-D Conv2x (models/submodule.py:104,
// 136-138, 150) and `spx2` (models/SemStereo.py:207) -- for training the 2-D decoder.  The forward (deconv2d_bf16s.hip) is
// out[co, 2y-1+kh, 2x-1+kw] += in[ci, y, x] * w[ci, co, kh, kw]; with g = the gradient of `out`:
//
//   data gradient     gin[ci, y, x] = sum_co sum_{kh,kw} g[co, 2y-1+kh, 2x-1+kw] * w[ci, co, kh, kw]
//   weight gradient   gw[ci, co, kh, kw] = sum_{b,y,x} in[b, ci, y, x] * g[b, co, 2y-1+kh, 2x-1+kw]
//
// ---- data gradient: a 4x4 stride-2 pad-1 CONVOLUTION of g, the same weight tensor read as [out = Cin, in = Cout, 4, 4], no flip ----
// (ss_conv2d_k4s2_f16s_fwd; below "in" is the conv's input, i.e. g, and Cin / Cout are the conv's.)  Two-term block-floating fp16
// form (split_f16.h: v_mfma_f32_32x32x16_f16, hi*lo + lo*hi + hi*hi), in the style of deconv2d_f16s.  A workgroup owns 32 output
// channels x (TH = 4 NT output rows) x 32 output columns of one batch element; wave w owns rows w NT .. w NT + NT - 1.  Per 8-channel
// chunk of the input the (2 TH + 2) x 66 halo tile is staged and split ONCE and serves all sixteen taps.  A K-step of 16 is two taps
// (kw = par + 2 * lane half) x 8 channels: eight K-steps (kh, par) per chunk.  The B operand is read at column stride 2, so even and odd
// halo columns are staged into separate planes ([term][halo row][column parity][33] 16-byte slots): the 32 lanes of a half read 32
// consecutive slots, and the two taps of a K-step are the same plane one slot apart.  The tile is a property of the layer, never of
// the launch's batch, so an element has the same bits alone and in a batch.  An infinity is left out of the block maximum (DROP_INF)
// and poisons its own receptive field only.  No affine, no ReLU.
//
// ---- weight gradient: a GEMM with M = 32 input channels, N = 32 output channels x 16 taps, K = positions ----
// (ss_deconv2d_k4s2_wgrad_fwd.)  Both operands are activations, so this is the three-term bf16 form (split_bf16.h, six products,
// v_mfma_f32_32x32x16_bf16) as in conv3d_wgrad_bf16s.hip.  The four waves of a workgroup own one kh each and its four kw (4 x 16
// accumulator registers); a K-step is 16 consecutive positions of a low-resolution row (8 per lane half).  A lane's operands are
// contiguous in memory -- 8 floats of its `in` channel's row, and the 18 floats 2x-1 .. 2x+16 of its g channel's row 2y-1+kh, of which
// tap kw takes every second one from kw on -- so they are loaded straight into registers (16-byte loads on aligned whole steps, masked
// scalar loads on ragged ones), split there and never staged: no LDS and no barrier.  A workgroup covers a range of rows (b, y) and
// writes ONE partial [16 taps][32][32] block into the workspace; a second, small launch adds a tile's partials in a fixed order in
// double.  No floating-point atomics: two calls give the same bits.  The number of partials is a function of the geometry alone
// (wgrad_plan), capped so that the workspace is at most max(64 MiB, 64 KiB per weight tile).
#include <stdlib.h>

#include "common.h"
#include "split_f16.h"

namespace {

// =====================================================================================================================================
// data gradient
// =====================================================================================================================================

template <int NT>
struct GCfg {
    static constexpr int TH = 4 * NT, IH = 2 * TH + 2, IW = 66, PW = 33;
    static constexpr int CS = IH * IW;                         // halo positions (= slots of one term: IH x 2 parities x 33)
    static constexpr int NPOS = (CS + 255) / 256;              // positions per thread
    static constexpr int WSL = 16 * 64;                        // 16-byte slots of a chunk's weight fragments
    static constexpr int SLOTS = 2 * CS + WSL + 1;             // two operand terms + weights + the four waves' maxima
};

template <int NT>
__global__ __launch_bounds__(256, 2) void conv2d_k4s2_f16s(const float* __restrict__ in, const uint4* __restrict__ wsplit,
                                                           const float* __restrict__ wunscale, float* __restrict__ out, int Cin, int H,
                                                           int W, int Cout, int tiles_w) {
    using C = GCfg<NT>;
    constexpr int WL = 2 * C::CS, MSLOT = 2 * C::CS + C::WSL;
    __shared__ __attribute__((aligned(16))) uint4 lds[C::SLOTS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int x0 = ((int)blockIdx.x % tiles_w) * 32, y0 = ((int)blockIdx.x / tiles_w) * C::TH;      // output tile origin
    const int ct = blockIdx.y, nct = gridDim.y, b = blockIdx.z;
    const int plane = H * W, Ho = H / 2, Wo = W / 2;
    const float* inb = in + (size_t)b * Cin * plane;

    // staging plan: this thread owns halo positions p = tid + 256 i (row p / 66, column p % 66), all 8 channels of a chunk
    int poff[C::NPOS], psl[C::NPOS];
#pragma unroll
    for (int i = 0; i < C::NPOS; ++i) {
        const int p = tid + 256 * i;
        const int row = p / C::IW, col = p % C::IW;
        const int gy = 2 * y0 - 1 + row, gx = 2 * x0 - 1 + col;
        poff[i] = (p < C::CS && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) ? gy * W + gx : -1;
        psl[i] = (row * 2 + (col & 1)) * C::PW + (col >> 1);   // parity-separated: column 2 q + par -> plane par, slot q
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

    f32x16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
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
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][r] *= ratio;
        }
        const float in_scale = bexp.in_scale();
        // ---- split + transpose: registers -> [term][row][parity][33][8 ch] ----
#pragma unroll
        for (int i = 0; i < C::NPOS; ++i) {
            const int p = tid + 256 * i;
            if (p >= C::CS) continue;
            unsigned hh[4], ll[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                split2_pk_f16(rin[(2 * c) * C::NPOS + i] * in_scale, rin[(2 * c + 1) * C::NPOS + i] * in_scale, hh[c], ll[c]);
            lds[psl[i]] = make_uint4(hh[0], hh[1], hh[2], hh[3]);
            lds[C::CS + psl[i]] = make_uint4(ll[0], ll[1], ll[2], ll[3]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) lds[WL + tid + 256 * i] = make_uint4(wpre[i][0], wpre[i][1], wpre[i][2], wpre[i][3]);
        __syncthreads();
        const bool more = chunk + 1 < nchunks;
        fetch(more ? chunk + 1 : chunk);                       // (unconditional: no vector-memory instruction under a branch)
        // ---- 8 (kh, par) K-steps x NT rows x 3 products ----
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int kh = s >> 1, par = s & 1;
            const f16x8 a0 = __builtin_bit_cast(f16x8, lds[WL + (s * 2 + 0) * 64 + lane]);
            const f16x8 a1 = __builtin_bit_cast(f16x8, lds[WL + (s * 2 + 1) * 64 + lane]);
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int slot = ((2 * (wave * NT + i) + kh) * 2 + par) * C::PW + l31 + half;      // kw = par + 2 * lane half
                const f16x8 b0 = __builtin_bit_cast(f16x8, lds[slot]);
                const f16x8 b1 = __builtin_bit_cast(f16x8, lds[C::CS + slot]);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[i], 0, 0, 0);          // smallest cross terms first
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[i], 0, 0, 0);
            }
        }
        if (more) publish_max();
        __syncthreads();
    }

    // ---- epilogue: 32x32 D layout (column = lane & 31 = output column, register r = channel (r & 3) + 8 (r >> 2) + 4 half) ----
    const float acc_unscale = bexp.acc_unscale();
    const int x = x0 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (co >= Cout || x >= Wo) continue;
        const float un = wunscale[co] * acc_unscale;           // powers of two: acc * un is exact
        float* oc = out + ((size_t)b * Cout + co) * Ho * Wo;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int y = y0 + wave * NT + i;
            if (y < Ho) oc[(size_t)y * Wo + x] = acc[i][r] * un;
        }
    }
}

// Conv2d weight [Cout,Cin,4,4] fp32 (= a ConvTranspose2d's [its Cin, its Cout, 4, 4]) -> [ceil(Cin/8)][ceil(Cout/32)][8 steps (kh, par)]
// [2 terms][2 lane halves (kw = par + 2 half)][32 channels][8] fp16 of w / wunscale[co] (zero padded), wunscale[co] = the power of two
// that brings max |w[co]| into [2^14, 2^15), stored behind the terms as float[32 ceil(Cout/32)].  One workgroup per (padded) output channel.
__global__ __launch_bounds__(256) void pack_conv2d_k4s2_f16s_kernel(const float* __restrict__ w, unsigned short* __restrict__ wsplit,
                                                                     float* __restrict__ wunscale, int Cout, int Cin) {
    __shared__ unsigned wmax[4];
    const int co = blockIdx.x, nct = gridDim.x / 32;
    const bool live = co < Cout;
    float m = 0.f;
    if (live)
        for (int i = threadIdx.x; i < Cin * 16; i += 256) m = fmaxf(m, fabsf(w[(size_t)co * Cin * 16 + i]));
    const float u = weight_unscale(m, wmax);
    if (threadIdx.x == 0) wunscale[co] = u;
    const int nchunks = (Cin + 7) / 8, ct = co / 32, cl = co % 32;
    const int n = nchunks * 32 * 8;                            // this channel's elements: (chunk, step, term, half, j)
    for (int e = threadIdx.x; e < n; e += 256) {
        const int j = e % 8;
        int r = e / 8;
        const int hf = r % 2; r /= 2;
        const int term = r % 2; r /= 2;
        const int step = r % 8;
        const int chunk = r / 8;
        const int kh = step >> 1, kw = (step & 1) + 2 * hf, ci = chunk * 8 + j;
        float x = 0.f;
        if (live && ci < Cin) x = w[((size_t)co * Cin + ci) * 16 + kh * 4 + kw] / u;      // exact: a power of two
        const size_t i = ((((size_t)chunk * nct + ct) * 16 + step * 2 + term) * 64 + hf * 32 + cl) * 8 + j;
        wsplit[i] = split_weight_f16(x, term);
    }
}

// the one statement of that layout's size: GCfg::WSL 16-byte slots per (chunk, channel tile), then float[32 ceil(Cout/32)]
ss::Packed conv2d_k4s2_packed(int Cout, int Cin) {
    const long long nct = ss::ceil_div(Cout, 32), terms = ss::ceil_div(Cin, 8) * nct * GCfg<1>::WSL * 16;
    return {terms, terms + 4 * 32 * nct};
}

template <int NT>
int launch_conv2d_k4s2(const float* in, const void* wsplit, float* out, int B, int Cin, int H, int W, int Cout, hipStream_t st) {
    using C = GCfg<NT>;
    const int tiles_w = ss::ceil_div(W / 2, 32), nct = ss::ceil_div(Cout, 32);
    const long long tiles = (long long)tiles_w * ss::ceil_div(H / 2, C::TH);
    if (tiles > 0x7fffffffLL || nct > 65535 || B > 65535) return SS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(conv2d_k4s2_f16s<NT>, dim3((unsigned)tiles, nct, B), dim3(256), 0, st, in, reinterpret_cast<const uint4*>(wsplit),
                       ss::scales_of(wsplit, conv2d_k4s2_packed(Cout, Cin)), out, Cin, H, W, Cout, tiles_w);
    return ss::check_launch();
}

// =====================================================================================================================================
// weight gradient
// =====================================================================================================================================

// How the rows (b, y) of a launch are cut into partials: rows per partial and the number of partials per weight tile.  A partial
// covers at least 2048 positions, and there are at most min(256, 1024 / tiles) of them (64 KiB each: at most 64 MiB of workspace up to
// 1024 weight tiles; beyond that one partial per tile, i.e. tiles * 64 KiB).
struct WgradPlan {
    int rpp, nparts, nci, nco;
};
inline WgradPlan wgrad_plan(int B, int Cin, int H, int W, int Cout) {
    WgradPlan p;
    p.nci = ss::ceil_div(Cin, 32);
    p.nco = ss::ceil_div(Cout, 32);
    const long long rows = (long long)B * H, tiles = (long long)p.nci * p.nco;
    long long cap = 1024 / tiles;
    cap = cap < 1 ? 1 : (cap > 256 ? 256 : cap);
    long long rpp = ss::ceil_div_ll(rows, cap);
    const long long floor_rows = ss::ceil_div_ll(2048, W);
    if (rpp < floor_rows) rpp = floor_rows;
    if (rpp > rows) rpp = rows;
    p.rpp = (int)rpp;
    p.nparts = (int)ss::ceil_div_ll(rows, rpp);
    return p;
}

// six cross products, smallest first: (m,m) (h,l) (l,h) (h,m) (m,h) (h,h)
__device__ __forceinline__ void mfma6(f32x16& acc, const uint4 (&a)[3], const uint4 (&b)[3]) {
    constexpr int pa[6] = {1, 0, 2, 0, 1, 0}, pb[6] = {1, 2, 0, 1, 0, 0};
#pragma unroll
    for (int p = 0; p < 6; ++p)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[pa[p]]), __builtin_bit_cast(bf16x8, b[pb[p]]), acc, 0, 0, 0);
}

// grid (nparts, nci * nco); wave = kh.  VEC: `in` and `g` are 16-byte aligned and W % 4 == 0, so whole K-steps take 16-byte loads.
template <bool VEC>
__global__ __launch_bounds__(256) void deconv2d_k4s2_wgrad_bf16s(const float* __restrict__ in, const float* __restrict__ g,
                                                                  float* __restrict__ ws, int Cin, int H, int W, int Cout, long long rows,
                                                                  int rpp, int nco) {
    const int lane = threadIdx.x & 63, kh = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
    const int part = blockIdx.x, tile = blockIdx.y;
    const int ci = (tile / nco) * 32 + l31, co = (tile % nco) * 32 + l31;
    const bool a_ok = ci < Cin, b_ok = co < Cout;
    const int cia = a_ok ? ci : Cin - 1, cob = b_ok ? co : Cout - 1;      // (masked lanes read a valid channel and drop the value)
    const int Wg = 2 * W, Hg = 2 * H;

    f32x16 acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

    const long long r0 = (long long)part * rpp, r1 = (r0 + rpp < rows) ? r0 + rpp : rows;
    for (long long row = r0; row < r1; ++row) {
        const int b = (int)(row / H), y = (int)(row % H);
        const int gy = 2 * y - 1 + kh;
        if ((unsigned)gy >= (unsigned)Hg) continue;            // (wave-uniform: this tap row lies in the padding)
        const float* arow = in + (((size_t)b * Cin + cia) * H + y) * W;
        const float* grow = g + (((size_t)b * Cout + cob) * Hg + gy) * Wg;
        for (int xs = 0; xs < W; xs += 16) {
            const int x8 = xs + 8 * half;
            float a[8], v[18];                                 // v[k] = g at column 2 x8 - 1 + k; tap kw of position x8 + j is v[kw + 2 j]
            if (VEC && xs + 16 <= W) {
                const float4 a0 = *reinterpret_cast<const float4*>(arow + x8), a1 = *reinterpret_cast<const float4*>(arow + x8 + 4);
                a[0] = a0.x; a[1] = a0.y; a[2] = a0.z; a[3] = a0.w; a[4] = a1.x; a[5] = a1.y; a[6] = a1.z; a[7] = a1.w;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 t = *reinterpret_cast<const float4*>(grow + 2 * x8 + 4 * q);
                    v[1 + 4 * q] = t.x; v[2 + 4 * q] = t.y; v[3 + 4 * q] = t.z; v[4 + 4 * q] = t.w;
                }
                v[0] = x8 > 0 ? grow[2 * x8 - 1] : 0.f;
                v[17] = 2 * x8 + 16 < Wg ? grow[2 * x8 + 16] : 0.f;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) a[j] = x8 + j < W ? arow[x8 + j] : 0.f;
#pragma unroll
                for (int k = 0; k < 18; ++k) {
                    const int gx = 2 * x8 - 1 + k;
                    v[k] = (unsigned)gx < (unsigned)Wg ? grow[gx] : 0.f;
                }
            }
            // masks at load time: a channel beyond the layer's, and g where the position itself is beyond the row (its `in` is 0)
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = a_ok ? a[j] : 0.f;
#pragma unroll
            for (int k = 0; k < 18; ++k) v[k] = b_ok ? v[k] : 0.f;
            auto tap = [&](int kw, int j) { return x8 + j < W ? v[kw + 2 * j] : 0.f; };
            uint4 af[3];
            {
                unsigned h[4], m[4], l[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) split3_pk(a[2 * e], a[2 * e + 1], h[e], m[e], l[e]);
                af[0] = make_uint4(h[0], h[1], h[2], h[3]);
                af[1] = make_uint4(m[0], m[1], m[2], m[3]);
                af[2] = make_uint4(l[0], l[1], l[2], l[3]);
            }
#pragma unroll
            for (int kw = 0; kw < 4; ++kw) {
                unsigned h[4], m[4], l[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) split3_pk(tap(kw, 2 * e), tap(kw, 2 * e + 1), h[e], m[e], l[e]);
                const uint4 bf[3] = {make_uint4(h[0], h[1], h[2], h[3]), make_uint4(m[0], m[1], m[2], m[3]), make_uint4(l[0], l[1], l[2], l[3])};
                mfma6(acc[kw], af, bf);
            }
        }
    }
    // ---- the wave's four tiles -> this workgroup's partial [tap][input channel][output channel] ----
    float* wp = ws + (((size_t)part * gridDim.y + tile) * 16 + kh * 4) * 1024 + l31;
#pragma unroll
    for (int kw = 0; kw < 4; ++kw)
#pragma unroll
        for (int r = 0; r < 16; ++r) wp[kw * 1024 + ((r & 3) + 8 * (r >> 2) + 4 * half) * 32] = acc[kw][r];
}

// gw[ci, co, tap] = sum over the partials, in their order, in double.  One thread per element of a (padded) tile.
__global__ __launch_bounds__(256) void deconv2d_k4s2_wgrad_sum(const float* __restrict__ ws, float* __restrict__ gw, int Cin, int Cout,
                                                               int nco, int nparts, long long per_part) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= per_part) return;
    const int n = (int)(t & 31), m = (int)((t >> 5) & 31), tap = (int)((t >> 10) & 15);
    const int tile = (int)(t >> 14);
    const int ci = (tile / nco) * 32 + m, co = (tile % nco) * 32 + n;
    if (ci >= Cin || co >= Cout) return;
    double s = 0.0;
    for (int p = 0; p < nparts; ++p) s += (double)ws[(size_t)p * per_part + t];
    gw[((size_t)ci * Cout + co) * 16 + tap] = (float)s;
}

int wgrad_check(int B, int Cin, int H, int W, int Cout) {
    SS_REQUIRE(B > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0);
    // one element's tensors are addressed through 32-bit offsets: they must stay below 2 GiB
    if ((long long)Cin * H * W * 4 >= 0x7fffffffLL || (long long)Cout * H * W * 16 >= 0x7fffffffLL) return SS_ERR_UNSUPPORTED;
    if ((long long)B * H > 0x7fffffffLL || (long long)ss::ceil_div(Cin, 32) * ss::ceil_div(Cout, 32) > 65535) return SS_ERR_UNSUPPORTED;
    return SS_OK;
}

}  // namespace

extern "C" int ss_conv2d_k4s2_f16s_fwd(const float* in, const void* wsplit, float* out, int B, int Cin, int H, int W, int Cout,
                                       ss_stream_t stream) {
    SS_REQUIRE(in && wsplit && out);
    SS_REQUIRE(B > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0);
    SS_REQUIRE((reinterpret_cast<uintptr_t>(wsplit) & 15) == 0);
    if ((H & 1) || (W & 1)) return SS_ERR_UNSUPPORTED;        // (the adjoint of a stride-2 transposed conv: even sizes only)
    // positions are addressed through 32-bit offsets: one batch element's input and output must stay below 2 GiB
    if ((long long)Cin * H * W * 4 >= 0x7fffffffLL || (long long)Cout * H * W >= 0x7fffffffLL) return SS_ERR_UNSUPPORTED;
    // the tile is a property of the LAYER, never of the launch's batch: an element gets the same bits alone and in a batch
    const long long wgs8 = (long long)ss::ceil_div(W / 2, 32) * ss::ceil_div(H / 2, 8) * ss::ceil_div(Cout, 32);
    if (wgs8 >= 256) return launch_conv2d_k4s2<2>(in, wsplit, out, B, Cin, H, W, Cout, ss::as_stream(stream));
    return launch_conv2d_k4s2<1>(in, wsplit, out, B, Cin, H, W, Cout, ss::as_stream(stream));
}

extern "C" int ss_pack_conv2d_k4s2_weights_f16s(const float* w, void* wsplit, int Cout, int Cin, ss_stream_t stream) {
    SS_REQUIRE(w && wsplit && Cout > 0 && Cin > 0);
    SS_REQUIRE((reinterpret_cast<uintptr_t>(wsplit) & 15) == 0);
    hipLaunchKernelGGL(pack_conv2d_k4s2_f16s_kernel, dim3(ss::ceil_div(Cout, 32) * 32), dim3(256), 0, ss::as_stream(stream), w,
                       reinterpret_cast<unsigned short*>(wsplit), ss::scales_of(wsplit, conv2d_k4s2_packed(Cout, Cin)), Cout, Cin);
    return ss::check_launch();
}

extern "C" int ss_pack_conv2d_k4s2_weights_f16s_bytes(int Cout, int Cin, long long* bytes) {
    SS_REQUIRE(bytes && Cout > 0 && Cin > 0);
    *bytes = conv2d_k4s2_packed(Cout, Cin).total;
    return SS_OK;
}

extern "C" int ss_deconv2d_k4s2_wgrad_workspace_bytes(int B, int Cin, int H, int W, int Cout, long long* bytes) {
    SS_REQUIRE(bytes);
    const int status = wgrad_check(B, Cin, H, W, Cout);
    if (status != SS_OK) return status;
    const WgradPlan p = wgrad_plan(B, Cin, H, W, Cout);
    *bytes = (long long)p.nparts * p.nci * p.nco * 16 * 1024 * 4;
    return SS_OK;
}

extern "C" int ss_deconv2d_k4s2_wgrad_fwd(const float* in, const float* grad_out, float* grad_w, float* workspace, int B, int Cin, int H,
                                          int W, int Cout, ss_stream_t stream) {
    SS_REQUIRE(in && grad_out && grad_w && workspace);
    const int status = wgrad_check(B, Cin, H, W, Cout);
    if (status != SS_OK) return status;
    const WgradPlan p = wgrad_plan(B, Cin, H, W, Cout);
    const int tiles = p.nci * p.nco;
    const long long rows = (long long)B * H, per_part = (long long)tiles * 16 * 1024;
    const bool vec = W % 4 == 0 && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(grad_out)) & 15) == 0;
    hipStream_t st = ss::as_stream(stream);
    if (vec)
        hipLaunchKernelGGL(deconv2d_k4s2_wgrad_bf16s<true>, dim3(p.nparts, tiles), dim3(256), 0, st, in, grad_out, workspace, Cin, H, W,
                           Cout, rows, p.rpp, p.nco);
    else
        hipLaunchKernelGGL(deconv2d_k4s2_wgrad_bf16s<false>, dim3(p.nparts, tiles), dim3(256), 0, st, in, grad_out, workspace, Cin, H, W,
                           Cout, rows, p.rpp, p.nco);
    int rc = ss::check_launch();
    if (rc != SS_OK) return rc;
    hipLaunchKernelGGL(deconv2d_k4s2_wgrad_sum, dim3((unsigned)ss::ceil_div_ll(per_part, 256)), dim3(256), 0, st, workspace, grad_w, Cin,
                       Cout, p.nco, p.nparts, per_part);
    return ss::check_launch();
}
