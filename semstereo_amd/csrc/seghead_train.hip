// The tail of the segmentation head under autograd -- segmenthead.forward (models/submodule.py:44-51) behind its BasicConv:
// Conv2d(32 -> C, 1x1, bias) -> bilinear x2 (F.interpolate, align_corners=False) -- forward and backward, each in one pass.
//
// Tile: 8 rows x 32 columns of low-resolution positions of ONE batch element, whatever the batch (the tile of seghead_f16s.hip): an
// element of `out` / `grad_a` has the same bits alone and in a batch.
//
// Forward (seghead_tail_fwd): the C logits of the tile's 10 x 34 halo positions (source index clamped at the borders, as
// F.interpolate does) are formed in fp32 from `a` and kept in LDS; a thread then owns two low-resolution columns = four adjacent output
// pixels of two output rows per class, with the arithmetic of bilinear_up2_kernel (seghead_f16s.hip): the horizontal pair first, each
// pair one fused multiply-add on an exact product.  The low-resolution logits never reach memory.
// (`a` is requested 340 / 256 = 1.33 times: the halo positions of a tile are its neighbours' own positions, and those re-reads are left to
// the caches; the compulsory traffic is one read of `a` and one write of `out`.)
//
// Backward (seghead_tail_bwd): the adjoint of the up-sampling is separable, per axis
//   g[i] = 0.75 (G[2i] + G[2i+1]) + 0.25 (G[2i-1] + G[2i+2]),
// the 0.25 tap of an output whose source index was clamped folded onto the border position, i.e. G read at the clamped index.  The
// horizontal half is applied while the 18 grad_out rows of the tile are staged (a thread holds four adjacent columns and their two
// neighbours), the vertical half from LDS; the C values g of a position stay in registers.  From them, in the same launch:
//   grad_a[k]    = sum_c w2[c,k] g[c]                        (thread = 4 adjacent positions x 8 channels)
//   grad_w2[c,k] = sum_{b,pos} g[c] a[k],  grad_bias[c] = sum_{b,pos} g[c]
// the last two as in loss.hip: g and a of the tile staged in LDS, thread (c,k) sums the tile's 256 positions in a fixed order (the
// bias: wave shuffles -> LDS), one partial per workgroup in `workspace`, and a second small launch adds the partials in double in a
// fixed order.  No floating-point atomics: two calls give the same bits.
#include "common.h"
#include "stream.h"

namespace {

constexpr int T_TH = 8, T_TW = 32, T_K = 32, T_CMAX = 8;
constexpr int F_IH = T_TH + 2, F_IW = T_TW + 2;                // the forward's halo tile of logits
constexpr int B_GH = 2 * T_TH + 2;                             // grad_out rows a tile reads (with the one-pixel halo)
constexpr int B_AS = T_TH * T_TW + 4;                          // row stride of the staged `a` tile: 16-byte reads of 16 lanes on 16 slots
constexpr int B_PART = 33;                                      // partials per class and workgroup: 32 weight columns + the bias

template <bool UP, bool VEC>
__global__ __launch_bounds__(256) void seghead_tail_fwd_kernel(const float* __restrict__ a, const float* __restrict__ w2,
                                                                const float* __restrict__ bias, float* __restrict__ out, int C, int H,
                                                                int W, int tiles_w) {
    __shared__ __attribute__((aligned(16))) float w2s[T_K * T_CMAX];           // [k][class], zero beyond C
    __shared__ float bs[T_CMAX];
    __shared__ __attribute__((aligned(16))) float ls[UP ? T_CMAX * F_IH * F_IW : 4];
    const int tid = threadIdx.x;
    const int x0 = ((int)blockIdx.x % tiles_w) * T_TW, y0 = ((int)blockIdx.x / tiles_w) * T_TH;
    const int b = blockIdx.y;
    const int plane = H * W;
    const float* ab = a + (size_t)b * T_K * plane;
    {
        const int k = tid >> 3, c = tid & 7;
        w2s[tid] = c < C ? w2[c * T_K + k] : 0.f;
        if (tid < T_CMAX) bs[tid] = tid < C ? bias[tid] : 0.f;
    }
    __syncthreads();

    if (!UP) {
        const int y = y0 + (tid >> 5), x = x0 + (tid & 31);
        const int off = min(y, H - 1) * W + min(x, W - 1);
        float acc[T_CMAX];
#pragma unroll
        for (int c = 0; c < T_CMAX; ++c) acc[c] = 0.f;
#pragma unroll 8
        for (int k = 0; k < T_K; ++k) {
            const float v = ab[(size_t)k * plane + off];
#pragma unroll
            for (int c = 0; c < T_CMAX; ++c) acc[c] = fmaf(w2s[k * T_CMAX + c], v, acc[c]);
        }
        if (y < H && x < W) {
#pragma unroll
            for (int c = 0; c < T_CMAX; ++c)
                if (c < C) out[((size_t)b * C + c) * plane + (size_t)y * W + x] = acc[c] + bs[c];
        }
        return;
    }

    // ---- the logits of the halo tile (clamped source positions: every address is inside the map) ----
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int p = tid + 256 * i;
        const int pp = min(p, F_IH * F_IW - 1);
        const int gy = min(max(y0 - 1 + pp / F_IW, 0), H - 1), gx = min(max(x0 - 1 + pp % F_IW, 0), W - 1);
        const int off = gy * W + gx;
        float acc[T_CMAX];
#pragma unroll
        for (int c = 0; c < T_CMAX; ++c) acc[c] = 0.f;
#pragma unroll 8
        for (int k = 0; k < T_K; ++k) {
            const float v = ab[(size_t)k * plane + off];
#pragma unroll
            for (int c = 0; c < T_CMAX; ++c) acc[c] = fmaf(w2s[k * T_CMAX + c], v, acc[c]);
        }
        if (p < F_IH * F_IW) {
#pragma unroll
            for (int c = 0; c < T_CMAX; ++c) ls[c * (F_IH * F_IW) + p] = acc[c] + bs[c];
        }
    }
    __syncthreads();

    // ---- one thread: input columns 2 j, 2 j + 1 of row r -> output columns 4 j .. 4 j + 3 of rows 2 r, 2 r + 1, every second class ----
    const int j = tid & 15, r = (tid >> 4) & 7;
    const int y = y0 + r, xa = x0 + 2 * j;
    if (y >= H || xa >= W) return;
    const int Ho = 2 * H, Wo = 2 * W;
    for (int c = tid >> 7; c < C; c += 2) {
        const float* lc = ls + c * (F_IH * F_IW) + r * F_IW + 2 * j;           // halo row r = map row y - 1, halo column 2 j = column xa - 1
        float h[3][4];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float vl = lc[q * F_IW], va = lc[q * F_IW + 1], vb = lc[q * F_IW + 2], vr = lc[q * F_IW + 3];
            h[q][0] = fmaf(va, 0.75f, vl * 0.25f);
            h[q][1] = fmaf(va, 0.75f, vb * 0.25f);
            h[q][2] = fmaf(vb, 0.75f, va * 0.25f);
            h[q][3] = fmaf(vb, 0.75f, vr * 0.25f);
        }
        float o[2][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[0][e] = fmaf(h[1][e], 0.75f, h[0][e] * 0.25f);
            o[1][e] = fmaf(h[1][e], 0.75f, h[2][e] * 0.25f);
        }
        float* op = out + ((size_t)b * C + c) * Ho * Wo;
#pragma unroll
        for (int py = 0; py < 2; ++py) {
            float* orow = op + (size_t)(2 * y + py) * Wo + 2 * xa;
            if (VEC) {
                *reinterpret_cast<float4*>(orow) = make_float4(o[py][0], o[py][1], o[py][2], o[py][3]);
            } else {
                orow[0] = o[py][0];
                orow[1] = o[py][1];
                if (xa + 1 < W) {
                    orow[2] = o[py][2];
                    orow[3] = o[py][3];
                }
            }
        }
    }
}

// workspace: [B * tiles][C][33] floats (32 weight-gradient columns, then the bias gradient)
template <bool UP, bool VEC>
__global__ __launch_bounds__(256) void seghead_tail_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ a,
                                                                const float* __restrict__ w2, float* __restrict__ grad_a,
                                                                float* __restrict__ work, int C, int H, int W, int tiles_w,
                                                                int need_w, int need_b) {
    constexpr int HS = UP ? T_CMAX * B_GH * T_TW : 4;          // the horizontally reduced grad_out rows ...
    constexpr int AS = T_K * B_AS;                             // ... share their LDS with the staged `a` tile
    __shared__ __attribute__((aligned(16))) float un[HS > AS ? HS : AS];
    __shared__ __attribute__((aligned(16))) float gs[T_CMAX * T_TH * T_TW];   // [class][position]
    __shared__ float w2s[T_CMAX * T_K];                        // [class][k], zero beyond C
    __shared__ float bsum[4][T_CMAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = ((int)blockIdx.x % tiles_w) * T_TW, y0 = ((int)blockIdx.x / tiles_w) * T_TH;
    const int b = blockIdx.y;
    const int plane = H * W;
    const int s = UP ? 2 : 1;
    const int Ho = s * H, Wo = s * W;
    const float* gb = gout + (size_t)b * C * Ho * Wo;
    const float* ab = a + (size_t)b * T_K * plane;
    w2s[tid] = tid < C * T_K ? w2[tid] : 0.f;

    // ---- this thread's part of the `a` tile: 4 adjacent positions (row ar, columns 4 aq ..) of channels 8 wave .. 8 wave + 7 ----
    const int ar = (tid >> 3) & 7, aq = tid & 7;
    const int ay = y0 + ar, ax = x0 + 4 * aq;
    float4 av[8];
    if (need_w) {
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const float* row = ab + (size_t)(wave * 8 + kk) * plane + (size_t)min(ay, H - 1) * W;
            if (VEC) {
                av[kk] = *reinterpret_cast<const float4*>(row + min(ax, W - 4));
                if (ay >= H || ax >= W) av[kk] = make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                const bool in = ay < H;
                av[kk].x = (in && ax < W) ? row[min(ax, W - 1)] : 0.f;
                av[kk].y = (in && ax + 1 < W) ? row[min(ax + 1, W - 1)] : 0.f;
                av[kk].z = (in && ax + 2 < W) ? row[min(ax + 2, W - 1)] : 0.f;
                av[kk].w = (in && ax + 3 < W) ? row[min(ax + 3, W - 1)] : 0.f;
            }
        }
    }

    // ---- g of this thread's position (ly, lx) ----
    const int ly = tid >> 5, lx = tid & 31;
    const bool valid = y0 + ly < H && x0 + lx < W;
    float g[T_CMAX];
    if (UP) {
        // items (class, grad_out row of the tile, 4 adjacent columns): the horizontal half of the adjoint -> un[class][row][32]
        const int items = C * B_GH * 16;
        for (int it = tid; it < items; it += 256) {
            const int q = it & 15, gr = (it >> 4) % B_GH, c = (it >> 4) / B_GH;
            const int row = min(max(2 * y0 - 1 + gr, 0), Ho - 1);
            const float* rp = gb + ((size_t)c * Ho + row) * Wo;
            const int c0 = 2 * x0 + 4 * q;
            float l, r, v0, v1, v2, v3;
            if (VEC) {
                const int cq = min(c0, Wo - 4);
                const float4 v = *reinterpret_cast<const float4*>(rp + cq);
                l = rp[max(cq - 1, 0)];
                r = rp[min(cq + 4, Wo - 1)];
                v0 = v.x; v1 = v.y; v2 = v.z; v3 = v.w;
            } else {
                l = rp[min(max(c0 - 1, 0), Wo - 1)];
                v0 = rp[min(c0, Wo - 1)];
                v1 = rp[min(c0 + 1, Wo - 1)];
                v2 = rp[min(c0 + 2, Wo - 1)];
                v3 = rp[min(c0 + 3, Wo - 1)];
                r = rp[min(c0 + 4, Wo - 1)];
            }
            const float h0 = fmaf(0.75f, v0 + v1, 0.25f * (l + v2));
            const float h1 = fmaf(0.75f, v2 + v3, 0.25f * (v1 + r));
            *reinterpret_cast<float2*>(&un[(c * B_GH + gr) * T_TW + 2 * q]) = make_float2(h0, h1);
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < T_CMAX; ++c) {
            g[c] = 0.f;
            if (c < C) {
                const float* hp = un + (c * B_GH + 2 * ly) * T_TW + lx;
                const float v = fmaf(0.75f, hp[T_TW] + hp[2 * T_TW], 0.25f * (hp[0] + hp[3 * T_TW]));
                g[c] = valid ? v : 0.f;
            }
        }
    } else {
        const int off = min(y0 + ly, H - 1) * W + min(x0 + lx, W - 1);
#pragma unroll
        for (int c = 0; c < T_CMAX; ++c) {
            g[c] = 0.f;
            if (c < C) {
                const float v = gb[(size_t)c * plane + off];
                g[c] = valid ? v : 0.f;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < T_CMAX; ++c) gs[c * (T_TH * T_TW) + tid] = g[c];
    if (need_b) {                                              // wave -> LDS; the four waves' sums are added below
#pragma unroll
        for (int c = 0; c < T_CMAX; ++c) {
            float v = g[c];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
            if (lane == 0) bsum[wave][c] = v;
        }
    }
    __syncthreads();                                           // (also: every read of the horizontally reduced rows is done)
    if (need_w) {
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
            *reinterpret_cast<float4*>(&un[(wave * 8 + kk) * B_AS + ar * T_TW + 4 * aq]) = av[kk];
    }

    // ---- grad_a: 4 adjacent positions x 8 channels per thread ----
    if (grad_a != nullptr && ay < H && ax < W) {
        float gv[T_CMAX][4];
#pragma unroll
        for (int c = 0; c < T_CMAX; ++c) ss::lds_read16(&gs[c * (T_TH * T_TW) + ar * T_TW + 4 * aq], gv[c]);
        float* gab = grad_a + (size_t)b * T_K * plane;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const int k = wave * 8 + kk;
            float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < T_CMAX; ++c) {
                const float w = w2s[c * T_K + k];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = fmaf(w, gv[c][e], o[e]);
            }
            float* row = gab + (size_t)k * plane + (size_t)ay * W + ax;
            if (VEC) {
                *reinterpret_cast<float4*>(row) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (ax + e < W) row[e] = o[e];
            }
        }
    }
    if (!need_w && !need_b) return;
    float* wp = work + ((size_t)b * gridDim.x + blockIdx.x) * (size_t)(C * B_PART);
    if (need_b && tid < C) wp[tid * B_PART + 32] = (bsum[0][tid] + bsum[1][tid]) + (bsum[2][tid] + bsum[3][tid]);
    if (!need_w) return;
    __syncthreads();
    // ---- thread (c, k): sum over the tile's positions of g[c] a[k], four interleaved chains ----
    if (tid < C * T_K) {
        const int c = tid >> 5, k = tid & 31;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int p = 0; p < T_TH * T_TW; p += 4) {
            float gq[4], aq4[4];
            ss::lds_read16(&gs[c * (T_TH * T_TW) + p], gq);
            ss::lds_read16(&un[k * B_AS + p], aq4);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(gq[e], aq4[e], acc[e]);
        }
        wp[c * B_PART + k] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    }
}

// one workgroup per output (class c, column j; j = 32: the bias): the partials of all workgroups, in double, in a fixed order
__global__ __launch_bounds__(256) void seghead_tail_sum_kernel(const float* __restrict__ work, float* __restrict__ grad_w2,
                                                                float* __restrict__ grad_bias, int C, long long ntiles) {
    __shared__ double red[256];
    const int c = blockIdx.x / B_PART, j = blockIdx.x % B_PART;
    float* dst = j < 32 ? (grad_w2 ? grad_w2 + c * T_K + j : nullptr) : (grad_bias ? grad_bias + c : nullptr);
    if (dst == nullptr) return;
    double sum = 0.0;
    for (long long t = threadIdx.x; t < ntiles; t += 256) sum += (double)work[(size_t)t * (C * B_PART) + blockIdx.x];
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) *dst = (float)red[0];
}

// 0 when the shape is one the kernels are built for
int tail_check(int B, int K, int C, int H, int W, int up2, long long* tiles) {
    if (K != T_K || C > T_CMAX) return SS_ERR_UNSUPPORTED;
    // positions are addressed through 32-bit offsets: one batch element's `a` and `out` must stay below 2 GiB
    const long long s = up2 ? 2 : 1;
    if ((long long)K * H * W * 4 >= 0x7fffffffLL || (long long)C * s * H * s * W * 4 >= 0x7fffffffLL) return SS_ERR_UNSUPPORTED;
    *tiles = (long long)ss::ceil_div(W, T_TW) * ss::ceil_div(H, T_TH);
    if (B > 65535) return SS_ERR_UNSUPPORTED;
    return SS_OK;
}

using ss::stream::aligned16;

}  // namespace

extern "C" int ss_seghead_tail_workspace_bytes(int B, int K, int C, int H, int W, long long* bytes) {
    SS_REQUIRE(bytes != nullptr);
    SS_REQUIRE(B > 0 && K > 0 && C > 0 && H > 0 && W > 0);
    long long tiles = 0;
    const int st = tail_check(B, K, C, H, W, 0, &tiles);
    if (st != SS_OK) return st;
    *bytes = (long long)B * tiles * C * B_PART * (long long)sizeof(float);
    return SS_OK;
}

extern "C" int ss_seghead_tail_fwd(const float* a, const float* w2, const float* bias, float* out, int B, int K, int C, int H, int W,
                                   int up2, ss_stream_t stream) {
    SS_REQUIRE(a && w2 && bias && out);
    SS_REQUIRE(B > 0 && K > 0 && C > 0 && H > 0 && W > 0);
    long long tiles = 0;
    const int st = tail_check(B, K, C, H, W, up2, &tiles);
    if (st != SS_OK) return st;
    const int tiles_w = ss::ceil_div(W, T_TW);
    const dim3 grid((unsigned)tiles, B), block(256);
    hipStream_t hs = ss::as_stream(stream);
    if (!up2)
        hipLaunchKernelGGL((seghead_tail_fwd_kernel<false, false>), grid, block, 0, hs, a, w2, bias, out, C, H, W, tiles_w);
    else if (W % 2 == 0 && aligned16(out))
        hipLaunchKernelGGL((seghead_tail_fwd_kernel<true, true>), grid, block, 0, hs, a, w2, bias, out, C, H, W, tiles_w);
    else
        hipLaunchKernelGGL((seghead_tail_fwd_kernel<true, false>), grid, block, 0, hs, a, w2, bias, out, C, H, W, tiles_w);
    return ss::check_launch();
}

extern "C" int ss_seghead_tail_bwd(const float* grad_out, const float* a, const float* w2, float* grad_a, float* grad_w2,
                                   float* grad_bias, float* workspace, int B, int K, int C, int H, int W, int up2,
                                   ss_stream_t stream) {
    SS_REQUIRE(grad_out && a && w2);
    SS_REQUIRE(grad_a || grad_w2 || grad_bias);
    SS_REQUIRE(workspace || !(grad_w2 || grad_bias));
    SS_REQUIRE(B > 0 && K > 0 && C > 0 && H > 0 && W > 0);
    long long tiles = 0;
    const int st = tail_check(B, K, C, H, W, up2, &tiles);
    if (st != SS_OK) return st;
    const int tiles_w = ss::ceil_div(W, T_TW);
    const dim3 grid((unsigned)tiles, B), block(256);
    hipStream_t hs = ss::as_stream(stream);
    const int need_w = grad_w2 != nullptr, need_b = grad_bias != nullptr;
    const bool vec = W % 4 == 0 && aligned16(grad_out) && aligned16(a) && (grad_a == nullptr || aligned16(grad_a));
#define SS_TAIL_BWD(UP, VEC)                                                                                                       \
    hipLaunchKernelGGL((seghead_tail_bwd_kernel<UP, VEC>), grid, block, 0, hs, grad_out, a, w2, grad_a, workspace, C, H, W, tiles_w, \
                       need_w, need_b)
    if (up2) {
        if (vec) SS_TAIL_BWD(true, true); else SS_TAIL_BWD(true, false);
    } else {
        if (vec) SS_TAIL_BWD(false, true); else SS_TAIL_BWD(false, false);
    }
#undef SS_TAIL_BWD
    int status = ss::check_launch();
    if (status != SS_OK || !(need_w || need_b)) return status;
    hipLaunchKernelGGL(seghead_tail_sum_kernel, dim3(C * B_PART), dim3(256), 0, hs, workspace, grad_w2, grad_bias, C,
                       (long long)B * tiles);
    return ss::check_launch();
}
