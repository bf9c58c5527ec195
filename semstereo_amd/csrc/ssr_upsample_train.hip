// Training form of the semantic-guided refinement head (SSR_upsample, reference models/submodule.py:412-431; call sites
// models/SemStereo.py:311, 324), forward and backward, BatchNorm on batch statistics (train()) or on the running statistics
// (eval() under autograd).  For n = 6 classes and N = B*H*W full-resolution positions:
//
//   L  = softmax_c(pred_label)            U = bilinear x4 (align_corners=False) of depth_low
//   A  = BN0(U), zero padding AFTER BN0   C = conv3x3_{1->n}(A) + bc          D = BNa(C)
//   P1 = sigmoid(BN1(W1 (L*weights) + b1))        P = sigmoid(BN2(W2 (P1*weights) + b2))
//   out = U + W3 (D*P) + b3
//
// Nothing of full resolution is stored between the passes: every pass recomputes per pixel what it needs from the 1/4-scale map
// (L2-resident; the 3x3 taps are re-interpolated) and the two [B,n,H,W] inputs, and reduces per-workgroup partial sums into a
// float64 slab [G][KS] that a one-workgroup finishing kernel sums in a fixed order (no atomics: bitwise reproducible).  The
// finishing kernels fold the statistics into the convolutions on the device and write the running statistics / parameter
// gradients themselves.
//
//   forward (batch statistics): F1 BN0 sums (reads the 1/4-scale map only) -> F2 BNa + BN1 sums (inputs) -> F3 BN2 sums (inputs)
//                               -> F4 out.  On running statistics: one fold kernel, then F4.
//   backward: B1 BNa / BN2 backward sums, conv3 gradients -> B2 3x3-conv bias, BN0 sums (re-indexed onto the conv output, so no
//             halo), W2 / b2 gradients, BN1 sums; writes gC when grad_depth_low is wanted -> B3 3x3-conv / W1 / b1 gradients,
//             grad_weights, grad_pred_label, the full-resolution gradient of U (gC of the 3x3 neighbours read back) -> B4 the
//             adjoint of the x4 bilinear as a deterministic gather over the full-resolution window of each 1/4-scale pixel.
#include <type_traits>

#include "common.h"

namespace {

constexpr int NC = 6;

// packed raw parameters: the head's 16 parameter tensors flattened in module.parameters() order (grad_params uses the same layout)
constexpr int O_G0 = 0, O_BE0 = 1, O_WC = 2, O_BC = O_WC + NC * 9, O_GA = O_BC + NC, O_BEA = O_GA + NC, O_W1 = O_BEA + NC,
              O_B1 = O_W1 + NC * NC, O_G1 = O_B1 + NC, O_BE1 = O_G1 + NC, O_W2 = O_BE1 + NC, O_B2 = O_W2 + NC * NC,
              O_G2 = O_B2 + NC, O_BE2 = O_G2 + NC, O_W3 = O_BE2 + NC, O_B3 = O_W3 + NC, NPRM = O_B3 + 1;
static_assert(NPRM == 189, "packed parameter count");

// `saved` (floats, written by the forward, read by the backward): float64 mean / invstd of the four BatchNorms first, then the
// float coefficients the per-pixel passes read (every statistic folded into the convolution it follows)
constexpr int S_MU0 = 0, S_IS0 = 1, S_MUA = 2, S_ISA = 8, S_MU1 = 14, S_IS1 = 20, S_MU2 = 26, S_IS2 = 32;   // doubles
constexpr int CO = 80;                                                   // float offset of the coefficients
constexpr int C_MU0 = 0, C_IS0 = 1, C_WA = 2, C_BA = C_WA + NC * 9, C_W1 = C_BA + NC, C_B1 = C_W1 + NC * NC, C_W2 = C_B1 + NC,
              C_B2 = C_W2 + NC * NC, C_N = C_B2 + NC;                    // x^a = WA A + BA, x^1 = W1' z1 + B1', x^2 = W2' z2 + B2'
constexpr int SAVED_FLOATS = 256;
static_assert(CO + C_N <= SAVED_FLOATS, "saved layout");

// backward coefficients (floats, in the workspace right after the slab): dX = k1 (dQ - k2 - x^ k3) per BatchNorm channel
constexpr int K_A1 = 0, K_A2 = 6, K_A3 = 12, K_21 = 18, K_22 = 24, K_23 = 30, K_01 = 36, K_02 = 37, K_03 = 38, K_11 = 39, K_12 = 45,
              K_13 = 51, K_N = 64;

constexpr int KS = 128;        // slab row (doubles) per workgroup
constexpr int GMAX = 1024;     // workgroups of a reduction pass

enum Stage { F1, F2, F3, F4, B1, B2, B3 };
template <int ST> struct NSums { static constexpr int K = ST == F1 ? 2 : ST == F2 ? 24 : ST == F3 ? 12 : ST == F4 ? 0 : ST == B1 ? 31 : ST == B2 ? 62 : 96; };

struct PassArgs {
    const float* low;
    const float* wt;
    const float* lg;
    const float* prm;
    const float* co;
    const float* bk;
    const float* gout;
    float* out;
    float* gc;
    float* gu;
    float* gwt;
    float* glg;
    double* slab;
    int h, w, H, W, N;
};

// ATen upsample_bilinear2d, align_corners=False, scale = in/out = 0.25 (as ssr_upsample.hip)
__device__ __forceinline__ void src_index(int dst, int in_size, int& i0, int& i1, float& l0, float& l1) {
    float s = 0.25f * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = min((int)s, in_size - 1);
    i1 = min(i0 + 1, in_size - 1);
    l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
    l0 = 1.0f - l1;
}

// the 3x3 neighbourhood of (Y, X) in the up-sampled map: u[k] (0 outside) and m[k] = 1 inside the map, 0 on the conv's padding
__device__ __forceinline__ void taps(const float* __restrict__ low, int h, int w, int H, int W, int Y, int X, float (&u)[9],
                                     float (&m)[9]) {
    int r0[3], r1[3], c0[3], c1[3];
    float ly0[3], ly1[3], lx0[3], lx1[3];
    bool iny[3], inx[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int yy = Y + j - 1, xx = X + j - 1;
        iny[j] = (unsigned)yy < (unsigned)H;
        inx[j] = (unsigned)xx < (unsigned)W;
        src_index(min(max(yy, 0), H - 1), h, r0[j], r1[j], ly0[j], ly1[j]);
        src_index(min(max(xx, 0), W - 1), w, c0[j], c1[j], lx0[j], lx1[j]);
    }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const float* a = low + r0[ky] * w;
            const float* b = low + r1[ky] * w;
            const float t0 = ss::add_rn(ss::mul_rn(lx0[kx], a[c0[kx]]), ss::mul_rn(lx1[kx], a[c1[kx]]));
            const float t1 = ss::add_rn(ss::mul_rn(lx0[kx], b[c0[kx]]), ss::mul_rn(lx1[kx], b[c1[kx]]));
            const float v = ss::add_rn(ss::mul_rn(ly0[ky], t0), ss::mul_rn(ly1[ky], t1));
            const bool in = iny[ky] && inx[kx];
            u[ky * 3 + kx] = in ? v : 0.f;
            m[ky * 3 + kx] = in ? 1.f : 0.f;
        }
}

__device__ __forceinline__ float upsampled(const float* __restrict__ low, int h, int w, int Y, int X) {
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    src_index(Y, h, y0, y1, ly0, ly1);
    src_index(X, w, x0, x1, lx0, lx1);
    const float t0 = ss::add_rn(ss::mul_rn(lx0, low[y0 * w + x0]), ss::mul_rn(lx1, low[y0 * w + x1]));
    const float t1 = ss::add_rn(ss::mul_rn(lx0, low[y1 * w + x0]), ss::mul_rn(lx1, low[y1 * w + x1]));
    return ss::add_rn(ss::mul_rn(ly0, t0), ss::mul_rn(ly1, t1));
}

__device__ __forceinline__ float sigm(float q) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896340736f * q));
}

__device__ __forceinline__ void softmax6(const float (&lg)[NC], float (&L)[NC]) {
    float mx = lg[0];
#pragma unroll
    for (int c = 1; c < NC; ++c) mx = fmaxf(mx, lg[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        L[c] = __builtin_amdgcn_exp2f((lg[c] - mx) * 1.44269504088896340736f);
        s += L[c];
    }
    const float r = __builtin_amdgcn_rcpf(s);      // s in [1, 6]
#pragma unroll
    for (int c = 0; c < NC; ++c) L[c] *= r;
}

// x^0 and A = BN0(U) (0 on the padding) at the nine taps
__device__ __forceinline__ void bn0_taps(const float* __restrict__ prm, const float* __restrict__ co, const float (&u)[9],
                                         const float (&m)[9], float (&xh0)[9], float (&A)[9]) {
    const float mu0 = co[C_MU0], is0 = co[C_IS0], g0 = prm[O_G0], be0 = prm[O_BE0];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        xh0[k] = m[k] * ((u[k] - mu0) * is0);
        A[k] = m[k] * fmaf(g0, xh0[k], be0);
    }
}

// the conv branch after its BatchNorm: x^a = (C - mua) * isa through the folded weights, D = ga x^a + bea
__device__ __forceinline__ void conv_branch(const float* __restrict__ prm, const float* __restrict__ co, const float (&A)[9],
                                            float (&xa)[NC], float (&d)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        float a = co[C_BA + c];
#pragma unroll
        for (int k = 0; k < 9; ++k) a = fmaf(co[C_WA + c * 9 + k], A[k], a);
        xa[c] = a;
        d[c] = fmaf(prm[O_GA + c], a, prm[O_BEA + c]);
    }
}

// y[o] = b[o] + sum_c W[o][c] z[c]
__device__ __forceinline__ void mat6(const float* __restrict__ Wm, const float* __restrict__ bv, const float (&z)[NC], float (&y)[NC]) {
#pragma unroll
    for (int o = 0; o < NC; ++o) {
        float a = bv[o];
#pragma unroll
        for (int c = 0; c < NC; ++c) a = fmaf(Wm[o * NC + c], z[c], a);
        y[o] = a;
    }
}

// the class gate: L, z1 = L * wt, x^1, P1, z2 = P1 * wt, x^2, P
struct Gate {
    float L[NC], z1[NC], x1[NC], p1[NC], z2[NC], x2[NC], p[NC];
};

__device__ __forceinline__ void gate(const float* __restrict__ prm, const float* __restrict__ co, const float (&lg)[NC],
                                     const float (&wt)[NC], Gate& q) {
    softmax6(lg, q.L);
#pragma unroll
    for (int c = 0; c < NC; ++c) q.z1[c] = q.L[c] * wt[c];
    mat6(co + C_W1, co + C_B1, q.z1, q.x1);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        q.p1[c] = sigm(fmaf(prm[O_G1 + c], q.x1[c], prm[O_BE1 + c]));
        q.z2[c] = q.p1[c] * wt[c];
    }
    mat6(co + C_W2, co + C_B2, q.z2, q.x2);
#pragma unroll
    for (int c = 0; c < NC; ++c) q.p[c] = sigm(fmaf(prm[O_G2 + c], q.x2[c], prm[O_BE2 + c]));
}

// the workgroup's sums -> slab row (float64; wave butterflies and the four waves in a fixed order)
template <int K, typename T>
__device__ __forceinline__ void block_store(const T (&acc)[K], double* __restrict__ row) {
    __shared__ double part[4][K];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double v = (double)acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) part[wv][k] = v;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) row[k] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
}

template <int ST>
__global__ __launch_bounds__(256) void ssr_train_pass(PassArgs a) {
    constexpr int K = NSums<ST>::K;
    using Acc = typename std::conditional<(ST == F1 || ST == F2 || ST == F3), double, float>::type;
    Acc acc[K > 0 ? K : 1];
#pragma unroll
    for (int k = 0; k < (K > 0 ? K : 1); ++k) acc[k] = 0;
    const float* __restrict__ prm = a.prm;
    const float* __restrict__ co = a.co;
    const float* __restrict__ bk = a.bk;
    const int HW = a.H * a.W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.N; i += gridDim.x * 256) {
        const int b = i / HW, r = i - b * HW, Y = r / a.W, X = r - Y * a.W;
        const float* low = a.low + (long long)b * a.h * a.w;
        if constexpr (ST == F1) {
            const double u = upsampled(low, a.h, a.w, Y, X);
            acc[0] += u;
            acc[1] += u * u;
            continue;
        } else {
            const long long base = (long long)b * NC * HW + r;
            float lg[NC], wt[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                lg[c] = a.lg[base + (long long)c * HW];
                wt[c] = a.wt[base + (long long)c * HW];
            }
            if constexpr (ST == F2) {
                float u[9], m[9], xh0[9], A[9];
                taps(low, a.h, a.w, a.H, a.W, Y, X, u, m);
                bn0_taps(prm, co, u, m, xh0, A);
                float L[NC], z1[NC], y1[NC];
                softmax6(lg, L);
#pragma unroll
                for (int c = 0; c < NC; ++c) z1[c] = L[c] * wt[c];
                mat6(prm + O_W1, prm + O_B1, z1, y1);
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    float cc = prm[O_BC + c];
#pragma unroll
                    for (int k = 0; k < 9; ++k) cc = fmaf(prm[O_WC + c * 9 + k], A[k], cc);
                    acc[c] += (double)cc;
                    acc[6 + c] += (double)cc * cc;
                    acc[12 + c] += (double)y1[c];
                    acc[18 + c] += (double)y1[c] * y1[c];
                }
            } else if constexpr (ST == F3) {
                float L[NC], z1[NC], x1[NC], z2[NC], y2[NC];
                softmax6(lg, L);
#pragma unroll
                for (int c = 0; c < NC; ++c) z1[c] = L[c] * wt[c];
                mat6(co + C_W1, co + C_B1, z1, x1);
#pragma unroll
                for (int c = 0; c < NC; ++c) z2[c] = sigm(fmaf(prm[O_G1 + c], x1[c], prm[O_BE1 + c])) * wt[c];
                mat6(prm + O_W2, prm + O_B2, z2, y2);
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    acc[c] += (double)y2[c];
                    acc[6 + c] += (double)y2[c] * y2[c];
                }
            } else {
                float u[9], m[9], xh0[9], A[9], xa[NC], d[NC];
                taps(low, a.h, a.w, a.H, a.W, Y, X, u, m);
                bn0_taps(prm, co, u, m, xh0, A);
                conv_branch(prm, co, A, xa, d);
                Gate q;
                gate(prm, co, lg, wt, q);
                if constexpr (ST == F4) {
                    float res = prm[O_B3];
#pragma unroll
                    for (int c = 0; c < NC; ++c) res = fmaf(prm[O_W3 + c] * d[c], q.p[c], res);
                    a.out[i] = u[4] + res;
                } else {
                    const float g = a.gout[i];
                    float gD[NC], gQ2[NC];
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        const float gw = g * prm[O_W3 + c];
                        gD[c] = gw * q.p[c];
                        gQ2[c] = gw * d[c] * (q.p[c] * (1.0f - q.p[c]));
                    }
                    if constexpr (ST == B1) {
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            acc[c] += gD[c];
                            acc[6 + c] += gD[c] * xa[c];
                            acc[12 + c] += gQ2[c];
                            acc[18 + c] += gQ2[c] * q.x2[c];
                            acc[24 + c] += g * d[c] * q.p[c];
                        }
                        acc[30] += g;
                    } else {
                        float gC[NC], gY2[NC], gZ2[NC], gQ1[NC];
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            gC[c] = bk[K_A1 + c] * (gD[c] - bk[K_A2 + c] - xa[c] * bk[K_A3 + c]);
                            gY2[c] = bk[K_21 + c] * (gQ2[c] - bk[K_22 + c] - q.x2[c] * bk[K_23 + c]);
                        }
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            float s = 0.f;
#pragma unroll
                            for (int o = 0; o < NC; ++o) s = fmaf(prm[O_W2 + o * NC + c], gY2[o], s);
                            gZ2[c] = s;
                            gQ1[c] = s * wt[c] * (q.p1[c] * (1.0f - q.p1[c]));
                        }
                        if constexpr (ST == B2) {
                            if (a.gc) {
#pragma unroll
                                for (int c = 0; c < NC; ++c) a.gc[(long long)c * a.N + i] = gC[c];
                            }
#pragma unroll
                            for (int c = 0; c < NC; ++c) {
                                float mc = 0.f, xc = 0.f;
#pragma unroll
                                for (int k = 0; k < 9; ++k) {
                                    mc = fmaf(prm[O_WC + c * 9 + k], m[k], mc);
                                    xc = fmaf(prm[O_WC + c * 9 + k], xh0[k], xc);
                                }
                                acc[c] += gC[c];
                                acc[6] += gC[c] * mc;           // sum over the map of dL/dA   (BN0's bias gradient)
                                acc[7] += gC[c] * xc;           // ... of dL/dA * x^0          (BN0's weight gradient)
                            }
#pragma unroll
                            for (int o = 0; o < NC; ++o) {
#pragma unroll
                                for (int c = 0; c < NC; ++c) acc[8 + o * NC + c] += gY2[o] * q.z2[c];
                                acc[44 + o] += gY2[o];
                                acc[50 + o] += gQ1[o];
                                acc[56 + o] += gQ1[o] * q.x1[o];
                            }
                        } else {   // B3
                            float gY1[NC], gZ1[NC];
#pragma unroll
                            for (int c = 0; c < NC; ++c) {
#pragma unroll
                                for (int k = 0; k < 9; ++k) acc[c * 9 + k] += gC[c] * A[k];
                                gY1[c] = bk[K_11 + c] * (gQ1[c] - bk[K_12 + c] - q.x1[c] * bk[K_13 + c]);
                            }
#pragma unroll
                            for (int o = 0; o < NC; ++o) {
#pragma unroll
                                for (int c = 0; c < NC; ++c) acc[54 + o * NC + c] += gY1[o] * q.z1[c];
                                acc[90 + o] += gY1[o];
                            }
#pragma unroll
                            for (int c = 0; c < NC; ++c) {
                                float s = 0.f;
#pragma unroll
                                for (int o = 0; o < NC; ++o) s = fmaf(prm[O_W1 + o * NC + c], gY1[o], s);
                                gZ1[c] = s;
                            }
                            if (a.gwt) {
#pragma unroll
                                for (int c = 0; c < NC; ++c) a.gwt[base + (long long)c * HW] = fmaf(gZ2[c], q.p1[c], gZ1[c] * q.L[c]);
                            }
                            if (a.glg) {
                                float gL[NC], s = 0.f;
#pragma unroll
                                for (int c = 0; c < NC; ++c) {
                                    gL[c] = gZ1[c] * wt[c];
                                    s = fmaf(q.L[c], gL[c], s);
                                }
#pragma unroll
                                for (int c = 0; c < NC; ++c) a.glg[base + (long long)c * HW] = q.L[c] * (gL[c] - s);
                            }
                            if (a.gu) {
                                // dL/dA here = sum over the conv outputs q whose 3x3 window holds this pixel: (Y, X) - (ky - 1, kx - 1)
                                float gA = 0.f;
#pragma unroll
                                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                                    for (int kx = 0; kx < 3; ++kx) {
                                        const int yy = Y + 1 - ky, xx = X + 1 - kx;
                                        if ((unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W) {
                                            const int j = i + (1 - ky) * a.W + (1 - kx);
#pragma unroll
                                            for (int c = 0; c < NC; ++c) gA = fmaf(prm[O_WC + c * 9 + ky * 3 + kx], a.gc[(long long)c * a.N + j], gA);
                                        }
                                    }
                                a.gu[i] = g + bk[K_01] * (gA - bk[K_02] - xh0[4] * bk[K_03]);
                            }
                        }
                    }
                }
            }
        }
    }
    if constexpr (K > 0) block_store<K>(acc, a.slab + (long long)blockIdx.x * KS);
}

// grad_depth_low: the adjoint of the x4 bilinear up-sampling, gathered over the full-resolution window [4y-2, 4y+5] x [4x-2, 4x+5]
// of each 1/4-scale pixel with the forward's clamped source indices and fp32 weights (no atomics)
__global__ __launch_bounds__(256) void ssr_train_grad_low(const float* __restrict__ gu, float* __restrict__ glow, int h, int w, int total) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int H = 4 * h, W = 4 * w;
    const int x = idx % w, y = (idx / w) % h, b = idx / (h * w);
    float wy[8], wx[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        int i0, i1;
        float l0, l1;
        const int Y = 4 * y - 2 + j, X = 4 * x - 2 + j;
        float vy = 0.f, vx = 0.f;
        if ((unsigned)Y < (unsigned)H) {
            src_index(Y, h, i0, i1, l0, l1);
            vy = (i0 == y ? l0 : 0.f) + (i1 == y ? l1 : 0.f);
        }
        if ((unsigned)X < (unsigned)W) {
            src_index(X, w, i0, i1, l0, l1);
            vx = (i0 == x ? l0 : 0.f) + (i1 == x ? l1 : 0.f);
        }
        wy[j] = vy;
        wx[j] = vx;
    }
    const float* g = gu + (long long)b * H * W;
    float acc = 0.f;
#pragma unroll
    for (int jy = 0; jy < 8; ++jy) {
        if (wy[jy] == 0.f) continue;
        const float* row = g + (long long)(4 * y - 2 + jy) * W;
        float s = 0.f;
#pragma unroll
        for (int jx = 0; jx < 8; ++jx)
            if (wx[jx] != 0.f) s = fmaf(wx[jx], row[4 * x - 2 + jx], s);
        acc = fmaf(wy[jy], s, acc);
    }
    glow[idx] = acc;
}

struct BnRun {
    float* rm;
    float* rv;
    long long* nbt;
    float eps;
    double mom;
};

struct FinArgs {
    const double* slab;
    const float* prm;
    float* saved;
    float* bk;
    float* grad;
    BnRun bn[4];      // BN0, BNa, BN1, BN2
    int G, K, stage, batch;
    double n;
};

enum FinStage { FIN_F1, FIN_F2, FIN_F3, FIN_EVAL, FIN_B1, FIN_B2, FIN_B3 };

// BatchNorm `j` (0: BN0, 1: BNa, 2: BN1, 3: BN2), channel c: mean / invstd into `saved`, folded into the convolution it follows
__device__ void fold_bn(const float* __restrict__ prm, float* __restrict__ saved, int j, int c, double mu, double istd) {
    double* sd = reinterpret_cast<double*>(saved);
    float* co = saved + CO;
    if (j == 0) {
        sd[S_MU0] = mu;
        sd[S_IS0] = istd;
        co[C_MU0] = (float)mu;
        co[C_IS0] = (float)istd;
    } else if (j == 1) {
        sd[S_MUA + c] = mu;
        sd[S_ISA + c] = istd;
        for (int k = 0; k < 9; ++k) co[C_WA + c * 9 + k] = (float)(istd * prm[O_WC + c * 9 + k]);
        co[C_BA + c] = (float)((prm[O_BC + c] - mu) * istd);
    } else {
        const int ow = j == 2 ? O_W1 : O_W2, ob = j == 2 ? O_B1 : O_B2, cw = j == 2 ? C_W1 : C_W2, cb = j == 2 ? C_B1 : C_B2;
        sd[(j == 2 ? S_MU1 : S_MU2) + c] = mu;
        sd[(j == 2 ? S_IS1 : S_IS2) + c] = istd;
        for (int k = 0; k < NC; ++k) co[cw + c * NC + k] = (float)(istd * prm[ow + c * NC + k]);
        co[cb + c] = (float)((prm[ob + c] - mu) * istd);
    }
}

// batch statistics of channel c of BatchNorm j from its sums; running statistics moved as F.batch_norm moves them
__device__ void batch_bn(const FinArgs& f, const double* tot, int j, int c, int isum, int isq) {
    const double mu = tot[isum] / f.n;
    const double var = fmax(tot[isq] / f.n - mu * mu, 0.0);
    fold_bn(f.prm, f.saved, j, c, mu, 1.0 / sqrt(var + (double)f.bn[j].eps));
    const BnRun& r = f.bn[j];
    if (r.rm) r.rm[c] = (float)((1.0 - r.mom) * (double)r.rm[c] + r.mom * mu);
    if (r.rv) r.rv[c] = (float)((1.0 - r.mom) * (double)r.rv[c] + r.mom * var * f.n / (f.n - 1.0));
    if (c == 0 && r.nbt) *r.nbt = *r.nbt + 1;
}

__global__ __launch_bounds__(1024) void ssr_train_finish(FinArgs f) {
    __shared__ double tot[KS];
    const int t = threadIdx.x, k = t >> 3, j = t & 7;
    double s = 0.0;
    if (k < f.K)
        for (int b = j; b < f.G; b += 8) s += f.slab[(long long)b * KS + k];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (j == 0) tot[k] = s;
    __syncthreads();
    if (t != 0) return;
    const float* prm = f.prm;
    const double* sd = reinterpret_cast<const double*>(f.saved);
    const double inv_n = f.batch ? 1.0 / f.n : 0.0;      // running statistics: the two mean terms of each BatchNorm backward vanish
    float* g = f.grad;
    float* bk = f.bk;
    switch (f.stage) {
    case FIN_F1:
        batch_bn(f, tot, 0, 0, 0, 1);
        break;
    case FIN_F2:
        for (int c = 0; c < NC; ++c) {
            batch_bn(f, tot, 1, c, c, 6 + c);
            batch_bn(f, tot, 2, c, 12 + c, 18 + c);
        }
        break;
    case FIN_F3:
        for (int c = 0; c < NC; ++c) batch_bn(f, tot, 3, c, c, 6 + c);
        break;
    case FIN_EVAL:
        for (int jj = 0; jj < 4; ++jj)
            for (int c = 0; c < (jj == 0 ? 1 : NC); ++c)
                fold_bn(prm, f.saved, jj, c, (double)f.bn[jj].rm[c], 1.0 / sqrt((double)f.bn[jj].rv[c] + (double)f.bn[jj].eps));
        break;
    case FIN_B1:
        for (int c = 0; c < NC; ++c) {
            g[O_BEA + c] = (float)tot[c];
            g[O_GA + c] = (float)tot[6 + c];
            g[O_BE2 + c] = (float)tot[12 + c];
            g[O_G2 + c] = (float)tot[18 + c];
            g[O_W3 + c] = (float)tot[24 + c];
            bk[K_A1 + c] = (float)(prm[O_GA + c] * sd[S_ISA + c]);
            bk[K_A2 + c] = (float)(tot[c] * inv_n);
            bk[K_A3 + c] = (float)(tot[6 + c] * inv_n);
            bk[K_21 + c] = (float)(prm[O_G2 + c] * sd[S_IS2 + c]);
            bk[K_22 + c] = (float)(tot[12 + c] * inv_n);
            bk[K_23 + c] = (float)(tot[18 + c] * inv_n);
        }
        g[O_B3] = (float)tot[30];
        break;
    case FIN_B2:
        for (int c = 0; c < NC; ++c) {
            g[O_BC + c] = (float)tot[c];
            g[O_B2 + c] = (float)tot[44 + c];
            g[O_BE1 + c] = (float)tot[50 + c];
            g[O_G1 + c] = (float)tot[56 + c];
            bk[K_11 + c] = (float)(prm[O_G1 + c] * sd[S_IS1 + c]);
            bk[K_12 + c] = (float)(tot[50 + c] * inv_n);
            bk[K_13 + c] = (float)(tot[56 + c] * inv_n);
        }
        for (int q = 0; q < NC * NC; ++q) g[O_W2 + q] = (float)tot[8 + q];
        g[O_BE0] = (float)tot[6];
        g[O_G0] = (float)tot[7];
        bk[K_01] = (float)(prm[O_G0] * sd[S_IS0]);
        bk[K_02] = (float)(tot[6] * inv_n);
        bk[K_03] = (float)(tot[7] * inv_n);
        break;
    case FIN_B3:
        for (int q = 0; q < NC * 9; ++q) g[O_WC + q] = (float)tot[q];
        for (int q = 0; q < NC * NC; ++q) g[O_W1 + q] = (float)tot[54 + q];
        for (int c = 0; c < NC; ++c) g[O_B1 + c] = (float)tot[90 + c];
        break;
    default:
        break;
    }
}

int grid_of(int N) { return ss::ceil_div(N, 256) < GMAX ? ss::ceil_div(N, 256) : GMAX; }

template <int ST>
int launch_pass(const PassArgs& a, int G, hipStream_t st) {
    hipLaunchKernelGGL(ssr_train_pass<ST>, dim3(G), dim3(256), 0, st, a);
    return ss::check_launch();
}

int finish(FinArgs f, int stage, int K, hipStream_t st) {
    f.stage = stage;
    f.K = K;
    hipLaunchKernelGGL(ssr_train_finish, dim3(1), dim3(1024), 0, st, f);
    return ss::check_launch();
}

bool shape_ok(int B, int h, int w) {
    const long long n = (long long)B * 16 * h * w;
    return n * NC < 0x7fffffffLL - (long long)GMAX * 256;
}

}  // namespace

extern "C" int ss_ssr_upsample_train_fwd(const float* depth_low, const float* weights, const float* pred_label, const float* params,
                                         float* out, float* saved, float* rm0, float* rv0, long long* nbt0, float* rma, float* rva,
                                         long long* nbta, float* rm1, float* rv1, long long* nbt1, float* rm2, float* rv2,
                                         long long* nbt2, float eps0, float epsa, float eps1, float eps2, double mom0, double moma,
                                         double mom1, double mom2, int batch_stats, int B, int h, int w, int num_classes,
                                         double* workspace, long long workspace_bytes, ss_stream_t stream) {
    SS_REQUIRE(depth_low && weights && pred_label && params && out && saved && workspace);
    SS_REQUIRE(B > 0 && h > 0 && w > 0 && (reinterpret_cast<uintptr_t>(saved) & 7) == 0);
    SS_REQUIRE(batch_stats || (rm0 && rv0 && rma && rva && rm1 && rv1 && rm2 && rv2));
    const double moms[4] = {mom0, moma, mom1, mom2};
    for (double m : moms) SS_REQUIRE(m >= 0.0 && m <= 1.0);
    if (num_classes != NC || !shape_ok(B, h, w)) return SS_ERR_UNSUPPORTED;
    const int N = B * 16 * h * w, G = grid_of(N);
    SS_REQUIRE(workspace_bytes >= (long long)G * KS * 8);
    hipStream_t st = ss::as_stream(stream);
    PassArgs a{depth_low, weights, pred_label, params, saved + CO, nullptr, nullptr, out, nullptr, nullptr, nullptr, nullptr, workspace,
               h, w, 4 * h, 4 * w, N};
    FinArgs f{workspace, params, saved, nullptr, nullptr,
              {{rm0, rv0, nbt0, eps0, mom0}, {rma, rva, nbta, epsa, moma}, {rm1, rv1, nbt1, eps1, mom1}, {rm2, rv2, nbt2, eps2, mom2}},
              G, 0, 0, batch_stats ? 1 : 0, (double)N};
    int s;
    if (batch_stats) {
        if ((s = launch_pass<F1>(a, G, st)) || (s = finish(f, FIN_F1, NSums<F1>::K, st)) || (s = launch_pass<F2>(a, G, st)) ||
            (s = finish(f, FIN_F2, NSums<F2>::K, st)) || (s = launch_pass<F3>(a, G, st)) || (s = finish(f, FIN_F3, NSums<F3>::K, st)))
            return s;
    } else if ((s = finish(f, FIN_EVAL, 0, st))) {
        return s;
    }
    return launch_pass<F4>(a, G, st);
}

extern "C" int ss_ssr_upsample_train_bwd(const float* depth_low, const float* weights, const float* pred_label, const float* params,
                                         const float* saved, const float* grad_out, float* grad_depth_low, float* grad_weights,
                                         float* grad_pred_label, float* grad_params, int batch_stats, int B, int h, int w,
                                         int num_classes, double* workspace, long long workspace_bytes, ss_stream_t stream) {
    SS_REQUIRE(depth_low && weights && pred_label && params && saved && grad_out && grad_params && workspace);
    SS_REQUIRE(B > 0 && h > 0 && w > 0 && (reinterpret_cast<uintptr_t>(saved) & 7) == 0);
    if (num_classes != NC || !shape_ok(B, h, w)) return SS_ERR_UNSUPPORTED;
    const int N = B * 16 * h * w, G = grid_of(N);
    const long long slab_bytes = (long long)G * KS * 8;
    SS_REQUIRE(workspace_bytes >= slab_bytes + K_N * 4 + (grad_depth_low ? 28LL * N : 0));
    float* bk = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + slab_bytes);
    float* gc = grad_depth_low ? bk + K_N : nullptr;
    float* gu = grad_depth_low ? gc + 6LL * N : nullptr;
    hipStream_t st = ss::as_stream(stream);
    PassArgs a{depth_low, weights, pred_label, params, saved + CO, bk, grad_out, nullptr, gc, gu, grad_weights, grad_pred_label,
               workspace, h, w, 4 * h, 4 * w, N};
    FinArgs f{workspace, params, const_cast<float*>(saved), bk, grad_params, {}, G, 0, 0, batch_stats ? 1 : 0, (double)N};
    int s;
    if ((s = launch_pass<B1>(a, G, st)) || (s = finish(f, FIN_B1, NSums<B1>::K, st)) || (s = launch_pass<B2>(a, G, st)) ||
        (s = finish(f, FIN_B2, NSums<B2>::K, st)) || (s = launch_pass<B3>(a, G, st)) || (s = finish(f, FIN_B3, NSums<B3>::K, st)))
        return s;
    if (grad_depth_low) {
        const int total = B * h * w;
        hipLaunchKernelGGL(ssr_train_grad_low, dim3(ss::ceil_div(total, 256)), dim3(256), 0, st, gu, grad_depth_low, h, w, total);
        return ss::check_launch();
    }
    return SS_OK;
}
