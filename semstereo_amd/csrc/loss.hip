// The training objective (main_us3d.py:199-208, models/loss.py): the masked disparity loss, the label loss (cross-entropy with an ignored
// class + multi-class Dice) and the left-right semantic consistency loss (the same cross-entropy with the label gathered along the row).
// All three are streaming reductions in the form of stream.h: a thread's sums are fp32 (a few dozen terms), doubles from the wave on,
// and the finish is a one-workgroup launch that writes the record of sums and the scalar loss.  The backward launches recompute what
// they need from the inputs and read only the record of sums and the incoming gradient from the device; nothing here allocates, copies
// or synchronises.
#include "common.h"
#include "metrics_decode.h"
#include "stream.h"

namespace {

using namespace ss::stream;    // BLOCK, grid_for, aligned_to, aligned16, block_sum
using ss::metrics::NC;         // (label_class is this file's own below, so no using-directive for ss::metrics)
using ss::metrics::LT_I64;
using ss::metrics::LT_U8;
using ss::metrics::LT_F32;

constexpr int GD = 512;       // workgroups per term of the disparity loss (x up to 4 terms)
constexpr int GL = 2048;      // workgroups of the label loss
constexpr int TERMS = 4;
constexpr double DICE_EPS = 1e-6;     // models/loss.py:33

// ---------------------------------------------------------------- disparity loss (models/loss.py:19-31)
struct DispTerm {
    const float* est;
    const float* gt;
    const unsigned char* mask;     // bool tensor, or NULL: lo <= gt < hi
    float* grad;                   // backward only (NULL: this term asks for no gradient)
    long long n;
    float w;
};
struct DispArgs {
    DispTerm t[TERMS];
    float lo, hi;
    int l1, nterms;
    double* ws;                    // [nterms][gridDim.x][2]
    double* rec;                   // [TERMS][2]: masked sum, masked count
    const float* gout;
    float* loss;
};

__device__ __forceinline__ bool disp_keep(const DispTerm& t, float g, unsigned char m, float lo, float hi) {
    return t.mask ? m != 0 : (g >= lo && g < hi);
}
__device__ __forceinline__ float disp_point(float d, int l1) {
    const float ad = fabsf(d);
    return l1 ? ad : (ad < 1.f ? 0.5f * d * d : ad - 0.5f);
}
__device__ __forceinline__ float disp_slope(float d, int l1) {
    return l1 ? (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : fminf(fmaxf(d, -1.f), 1.f);
}

__global__ __launch_bounds__(BLOCK) void disp_loss_fwd_k(DispArgs a) {
    __shared__ double lds[4 * 2];
    const DispTerm t = a.t[blockIdx.y];
    const long long stride = (long long)gridDim.x * BLOCK, first = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool vec = aligned16(t.est) && aligned16(t.gt) && aligned_to(t.mask, 4);
    const long long n4 = vec ? t.n / 4 : 0;
    float s = 0.f;
    int c = 0;
    for (long long i = first; i < n4; i += stride) {
        const float4 e = reinterpret_cast<const float4*>(t.est)[i], g = reinterpret_cast<const float4*>(t.gt)[i];
        uchar4 m = make_uchar4(0, 0, 0, 0);
        if (t.mask) m = reinterpret_cast<const uchar4*>(t.mask)[i];
        if (disp_keep(t, g.x, m.x, a.lo, a.hi)) { s += disp_point(e.x - g.x, a.l1); ++c; }
        if (disp_keep(t, g.y, m.y, a.lo, a.hi)) { s += disp_point(e.y - g.y, a.l1); ++c; }
        if (disp_keep(t, g.z, m.z, a.lo, a.hi)) { s += disp_point(e.z - g.z, a.l1); ++c; }
        if (disp_keep(t, g.w, m.w, a.lo, a.hi)) { s += disp_point(e.w - g.w, a.l1); ++c; }
    }
    for (long long i = n4 * 4 + first; i < t.n; i += stride) {
        const float g = t.gt[i];
        if (disp_keep(t, g, t.mask ? t.mask[i] : 0, a.lo, a.hi)) { s += disp_point(t.est[i] - g, a.l1); ++c; }
    }
    double v[2] = {(double)s, (double)c};
    block_sum<2>(v, lds);
    if (threadIdx.x == 0) {
        double* p = a.ws + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        p[0] = v[0];
        p[1] = v[1];
    }
}

// one workgroup: the partials of each term in a fixed order, the record, and loss = sum_i w_i * sum_i / count_i (0 / 0 = NaN, as the
// mean of an empty selection is in PyTorch)
__global__ __launch_bounds__(BLOCK) void disp_loss_finish_k(DispArgs a, int G) {
    __shared__ double lds[4 * 2];
    double loss = 0.0;
    for (int i = 0; i < a.nterms; ++i) {
        double v[2] = {0.0, 0.0};
        for (int g = threadIdx.x; g < G; g += BLOCK) {
            v[0] += a.ws[((long long)i * G + g) * 2];
            v[1] += a.ws[((long long)i * G + g) * 2 + 1];
        }
        block_sum<2>(v, lds);
        if (threadIdx.x == 0) {
            a.rec[2 * i] = v[0];
            a.rec[2 * i + 1] = v[1];
            loss += (double)a.t[i].w * (v[0] / v[1]);
        }
    }
    if (threadIdx.x == 0) *a.loss = (float)loss;
}

__global__ __launch_bounds__(BLOCK) void disp_loss_bwd_k(DispArgs a) {
    const DispTerm t = a.t[blockIdx.y];
    if (!t.grad) return;
    const float k = (float)((double)a.gout[0] * (double)t.w / a.rec[2 * blockIdx.y + 1]);
    const long long stride = (long long)gridDim.x * BLOCK, first = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool vec = aligned16(t.est) && aligned16(t.gt) && aligned16(t.grad) && aligned_to(t.mask, 4);
    const long long n4 = vec ? t.n / 4 : 0;
    for (long long i = first; i < n4; i += stride) {
        const float4 e = reinterpret_cast<const float4*>(t.est)[i], g = reinterpret_cast<const float4*>(t.gt)[i];
        uchar4 m = make_uchar4(0, 0, 0, 0);
        if (t.mask) m = reinterpret_cast<const uchar4*>(t.mask)[i];
        float4 r;
        r.x = disp_keep(t, g.x, m.x, a.lo, a.hi) ? k * disp_slope(e.x - g.x, a.l1) : 0.f;
        r.y = disp_keep(t, g.y, m.y, a.lo, a.hi) ? k * disp_slope(e.y - g.y, a.l1) : 0.f;
        r.z = disp_keep(t, g.z, m.z, a.lo, a.hi) ? k * disp_slope(e.z - g.z, a.l1) : 0.f;
        r.w = disp_keep(t, g.w, m.w, a.lo, a.hi) ? k * disp_slope(e.w - g.w, a.l1) : 0.f;
        reinterpret_cast<float4*>(t.grad)[i] = r;
    }
    for (long long i = n4 * 4 + first; i < t.n; i += stride) {
        const float g = t.gt[i];
        t.grad[i] = disp_keep(t, g, t.mask ? t.mask[i] : 0, a.lo, a.hi) ? k * disp_slope(t.est[i] - g, a.l1) : 0.f;
    }
}

// ---------------------------------------------------------------- label loss and LRSC loss (models/loss.py:106-135)
struct LabelArgs {
    const float* z;            // logits [B,NC,H,W]
    const void* y;             // labels [B,H,W], dtype by the kernel's template argument
    const float* disp;         // NULL: the label of the pixel itself; else [B,H,W]: the label at column clamp(x - disp, 0, W - 1)
    float* gz;                 // backward: grad of the logits
    long long* warped;         // forward, optional: the gathered label map [B,H,W] (as the reference's .long() leaves it)
    double* ws;                // [gridDim.x][5]
    double* rec;               // [5] + the loss as a double
    const float* gout;
    float* loss;
    int B, H, W;
    int ignore, dice;
    float scale;
};

template <int LT>
__device__ __forceinline__ long long label_raw(const void* y, long long i) {
    if (LT == LT_I64) return reinterpret_cast<const long long*>(y)[i];
    if (LT == LT_U8) return reinterpret_cast<const unsigned char*>(y)[i];
    const float f = reinterpret_cast<const float*>(y)[i];
    return (f > -9.0e18f && f < 9.0e18f) ? (long long)f : -1;       // .long() truncates; NaN and the out-of-range values are nobody's class
}
// a class in [0, NC), or -1: never an index out of bounds.  (Not metrics_decode.h's label_class on purpose: the raw value goes to `warped`.)
__device__ __forceinline__ int label_class(long long v) { return (v < 0 || v >= NC) ? -1 : (int)v; }

// the label of pixel p = (b, r) with r = h * W + x: its own, or (LRSC, models/loss.py:129-131) the one at xs = (long) clamp((float) x -
// disp, 0, W - 1) of the same row, the subtraction and the clamp in fp32 as the reference's int64 - fp32 tensor expression evaluates them
template <int LT>
__device__ __forceinline__ int pixel_label(const LabelArgs& a, long long p, int r, float d) {
    long long v;
    if (a.disp) {
        const int x = r % a.W;
        float t = ss::sub_rn((float)x, d);
        t = fminf(fmaxf(t, 0.f), (float)(a.W - 1));         // (a NaN disparity lands on column 0 here; the reference's gather raises)
        v = label_raw<LT>(a.y, p - x + (int)t);
        if (a.warped) a.warped[p] = v;
    } else {
        v = label_raw<LT>(a.y, p);
    }
    return label_class(v);
}

struct Soft {
    float p[NC];
    float lse;
};
__device__ __forceinline__ Soft softmax6(const float (&z)[NC]) {
    Soft s;
    float m = z[0];
#pragma unroll
    for (int k = 1; k < NC; ++k) m = fmaxf(m, z[k]);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        s.p[k] = expf(z[k] - m);
        sum += s.p[k];
    }
    const float inv = 1.f / sum;
#pragma unroll
    for (int k = 0; k < NC; ++k) s.p[k] *= inv;
    s.lse = m + logf(sum);
    return s;
}
// v[y] by selects.  (Each element passes through an empty asm: left alone, the optimiser turns the select chain back into an indexed
// load of a copy of v[] in scratch memory.)
__device__ __forceinline__ float pick(const float (&v)[NC], int y) {
    float r = v[0];
#pragma unroll
    for (int k = 1; k < NC; ++k) {
        float c = v[k];
        asm("" : "+v"(c));
        r = (k == y) ? c : r;
    }
    return r;
}

struct LabelAcc {
    float ce, py, pfg;      // sum (lse - z_y) over counted pixels; sum p_y over y < NC-1; sum (1 - p_{NC-1})
    int n, nfg;             // counted pixels; pixels with y < NC-1
};
__device__ __forceinline__ void label_point(const float (&z)[NC], int y, const LabelArgs& a, LabelAcc& acc) {
    const Soft s = softmax6(z);
    const bool counted = y >= 0 && y != a.ignore;
    if (counted) {
        acc.ce += s.lse - pick(z, y);
        ++acc.n;
    }
    if (a.dice) {
        const bool fg = y >= 0 && y < NC - 1;
        if (fg) {
            acc.py += pick(s.p, y);
            ++acc.nfg;
        }
        acc.pfg += ((s.p[0] + s.p[1]) + (s.p[2] + s.p[3])) + s.p[4];
    }
}

template <int LT>
__global__ __launch_bounds__(BLOCK) void label_loss_fwd_k(LabelArgs a) {
    __shared__ double lds[4 * 5];
    const long long HW = (long long)a.H * a.W, npix = HW * a.B;
    const long long stride = (long long)gridDim.x * BLOCK, first = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool vec = (HW & 3) == 0 && aligned16(a.z) && (!a.disp || aligned16(a.disp));
    const long long nq = vec ? npix / 4 : 0;
    LabelAcc acc = {0.f, 0.f, 0.f, 0, 0};
    for (long long q = first; q < nq; q += stride) {
        const long long p0 = q * 4, b = p0 / HW;
        const int r0 = (int)(p0 - b * HW);
        const float* zb = a.z + b * NC * HW + r0;
        float4 zv[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) zv[k] = *reinterpret_cast<const float4*>(zb + k * HW);
        float4 dv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.disp) dv = reinterpret_cast<const float4*>(a.disp)[q];
        const float d[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float z[NC];
#pragma unroll
            for (int k = 0; k < NC; ++k) z[k] = j == 0 ? zv[k].x : j == 1 ? zv[k].y : j == 2 ? zv[k].z : zv[k].w;
            label_point(z, pixel_label<LT>(a, p0 + j, r0 + j, d[j]), a, acc);
        }
    }
    for (long long p = nq * 4 + first; p < npix; p += stride) {
        const long long b = p / HW;
        const int r = (int)(p - b * HW);
        const float* zb = a.z + b * NC * HW + r;
        float z[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) z[k] = zb[k * HW];
        label_point(z, pixel_label<LT>(a, p, r, a.disp ? a.disp[p] : 0.f), a, acc);
    }
    double v[5] = {(double)acc.ce, (double)acc.n, (double)acc.py, (double)acc.pfg, (double)acc.nfg};
    block_sum<5>(v, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) a.ws[(long long)blockIdx.x * 5 + k] = v[k];
    }
}

// one workgroup: rec = the five sums; loss = scale * (ce + 1 - dice) with ce = rec0 / rec1, I = 2 rec2, S = rec3 + rec4,
// dice = (I + eps) / (S + eps), and dice = 1 where S == 0 (the torch.where of models/loss.py:42)
__global__ __launch_bounds__(BLOCK) void label_loss_finish_k(LabelArgs a, int G) {
    __shared__ double lds[4 * 5];
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int g = threadIdx.x; g < G; g += BLOCK) {
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] += a.ws[(long long)g * 5 + k];
    }
    block_sum<5>(v, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) a.rec[k] = v[k];
        double loss = v[0] / v[1];
        if (a.dice) {
            const double I = 2.0 * v[2], S = v[3] + v[4];
            loss += 1.0 - (S == 0.0 ? 1.0 : (I + DICE_EPS) / (S + DICE_EPS));
        }
        *a.loss = (float)((double)a.scale * loss);
    }
}

struct LabelCoef {
    float cn, cd, a_hit, a_miss;     // g * scale / N;  g * scale;  the Dice slope of a pixel's own class / of the other foreground classes
};
__device__ __forceinline__ LabelCoef label_coef(const LabelArgs& a) {
    const double gs = (double)a.gout[0] * (double)a.scale;
    LabelCoef c = {(float)(gs / a.rec[1]), (float)gs, 0.f, 0.f};
    if (a.dice) {
        const double I = 2.0 * a.rec[2] + DICE_EPS, S0 = a.rec[3] + a.rec[4], S = S0 + DICE_EPS;
        if (S0 != 0.0) {
            c.a_hit = (float)((2.0 * S - I) / (S * S));
            c.a_miss = (float)(-I / (S * S));
        }
    }
    return c;
}
// grad z_k = g * scale * ( [counted] (p_k - [k == y]) / N  -  p_k (a_k - sum_c a_c p_c) ),  a_{NC-1} = 0
__device__ __forceinline__ void label_point_bwd(const float (&z)[NC], int y, const LabelArgs& a, const LabelCoef& c, float (&g)[NC]) {
    const Soft s = softmax6(z);
    const bool counted = y >= 0 && y != a.ignore, fg = y >= 0 && y < NC - 1;
    float A = 0.f;
    if (a.dice) {
        A = c.a_miss * (((s.p[0] + s.p[1]) + (s.p[2] + s.p[3])) + s.p[4]);
        if (fg) A += (c.a_hit - c.a_miss) * pick(s.p, y);
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const float ak = (!a.dice || k == NC - 1) ? 0.f : ((fg && k == y) ? c.a_hit : c.a_miss);
        const float ce = counted ? c.cn * (s.p[k] - (k == y ? 1.f : 0.f)) : 0.f;
        g[k] = ce - c.cd * s.p[k] * (ak - A);
    }
}

template <int LT>
__global__ __launch_bounds__(BLOCK) void label_loss_bwd_k(LabelArgs a) {
    const long long HW = (long long)a.H * a.W, npix = HW * a.B;
    const long long stride = (long long)gridDim.x * BLOCK, first = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool vec = (HW & 3) == 0 && aligned16(a.z) && aligned16(a.gz) && (!a.disp || aligned16(a.disp));
    const long long nq = vec ? npix / 4 : 0;
    const LabelCoef c = label_coef(a);
    for (long long q = first; q < nq; q += stride) {
        const long long p0 = q * 4, b = p0 / HW;
        const int r0 = (int)(p0 - b * HW);
        const long long off = b * NC * HW + r0;
        float4 zv[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) zv[k] = *reinterpret_cast<const float4*>(a.z + off + k * HW);
        float4 dv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.disp) dv = reinterpret_cast<const float4*>(a.disp)[q];
        const float d[4] = {dv.x, dv.y, dv.z, dv.w};
        float g[4][NC];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float z[NC];
#pragma unroll
            for (int k = 0; k < NC; ++k) z[k] = j == 0 ? zv[k].x : j == 1 ? zv[k].y : j == 2 ? zv[k].z : zv[k].w;
            label_point_bwd(z, pixel_label<LT>(a, p0 + j, r0 + j, d[j]), a, c, g[j]);
        }
#pragma unroll
        for (int k = 0; k < NC; ++k) *reinterpret_cast<float4*>(a.gz + off + k * HW) = make_float4(g[0][k], g[1][k], g[2][k], g[3][k]);
    }
    for (long long p = nq * 4 + first; p < npix; p += stride) {
        const long long b = p / HW;
        const int r = (int)(p - b * HW);
        const long long off = b * NC * HW + r;
        float z[NC], g[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) z[k] = a.z[off + k * HW];
        label_point_bwd(z, pixel_label<LT>(a, p, r, a.disp ? a.disp[p] : 0.f), a, c, g);
#pragma unroll
        for (int k = 0; k < NC; ++k) a.gz[off + k * HW] = g[k];
    }
}

template <int LT>
int label_launch(const LabelArgs& a, bool backward, hipStream_t st) {
    const long long npix = (long long)a.B * a.H * a.W;
    const int G = grid_for(ss::ceil_div_ll(npix, 4), GL);
    if (backward) {
        hipLaunchKernelGGL(label_loss_bwd_k<LT>, dim3(G), dim3(BLOCK), 0, st, a);
        return ss::check_launch();
    }
    hipLaunchKernelGGL(label_loss_fwd_k<LT>, dim3(G), dim3(BLOCK), 0, st, a);
    if (int s = ss::check_launch()) return s;
    hipLaunchKernelGGL(label_loss_finish_k, dim3(1), dim3(BLOCK), 0, st, a, G);
    return ss::check_launch();
}

int label_entry(LabelArgs a, int label_dtype, int num_classes, bool backward, long long workspace_bytes, ss_stream_t stream) {
    SS_REQUIRE(a.z && a.y && a.rec && a.B > 0 && a.H > 0 && a.W > 0);
    SS_REQUIRE(backward ? (a.gout && a.gz) : (a.loss && a.ws && workspace_bytes >= (long long)GL * 5 * 8));
    SS_REQUIRE(label_dtype >= LT_I64 && label_dtype <= LT_F32);
    if (num_classes != NC || (long long)a.B * a.H * a.W * NC >= 0x7fffffffLL) return SS_ERR_UNSUPPORTED;
    hipStream_t st = ss::as_stream(stream);
    switch (label_dtype) {
    case LT_I64:
        return label_launch<LT_I64>(a, backward, st);
    case LT_U8:
        return label_launch<LT_U8>(a, backward, st);
    default:
        return label_launch<LT_F32>(a, backward, st);
    }
}

int disp_entry(DispArgs& a, bool backward, long long workspace_bytes, ss_stream_t stream) {
    SS_REQUIRE(a.nterms >= 1 && a.nterms <= TERMS && a.rec);
    SS_REQUIRE(backward ? a.gout != nullptr : (a.loss && a.ws && workspace_bytes >= (long long)TERMS * GD * 2 * 8));
    long long nmax = 0;
    for (int i = 0; i < a.nterms; ++i) {
        SS_REQUIRE(a.t[i].est && a.t[i].gt && a.t[i].n > 0);
        if (a.t[i].n >= 0x7fffffffLL) return SS_ERR_UNSUPPORTED;
        nmax = a.t[i].n > nmax ? a.t[i].n : nmax;
    }
    hipStream_t st = ss::as_stream(stream);
    const int G = grid_for(ss::ceil_div_ll(nmax, 4), GD);
    if (backward) {
        hipLaunchKernelGGL(disp_loss_bwd_k, dim3(G, a.nterms), dim3(BLOCK), 0, st, a);
        return ss::check_launch();
    }
    hipLaunchKernelGGL(disp_loss_fwd_k, dim3(G, a.nterms), dim3(BLOCK), 0, st, a);
    if (int s = ss::check_launch()) return s;
    hipLaunchKernelGGL(disp_loss_finish_k, dim3(1), dim3(BLOCK), 0, st, a, G);
    return ss::check_launch();
}

}  // namespace

extern "C" int ss_loss_workspace_bytes(int kind, long long* bytes) {
    SS_REQUIRE(bytes && (kind == 0 || kind == 1));
    *bytes = kind == 0 ? (long long)TERMS * GD * 2 * 8 : (long long)GL * 5 * 8;
    return SS_OK;
}

extern "C" int ss_disparity_loss_fwd(const float* est0, const float* gt0, const unsigned char* mask0, long long n0, const float* est1,
                                     const float* gt1, const unsigned char* mask1, long long n1, const float* est2, const float* gt2,
                                     const unsigned char* mask2, long long n2, const float* est3, const float* gt3,
                                     const unsigned char* mask3, long long n3, float w0, float w1, float w2, float w3, float lo, float hi,
                                     int nterms, int l1, double* record, float* loss, double* workspace, long long workspace_bytes,
                                     ss_stream_t stream) {
    DispArgs a{{{est0, gt0, mask0, nullptr, n0, w0}, {est1, gt1, mask1, nullptr, n1, w1}, {est2, gt2, mask2, nullptr, n2, w2},
                {est3, gt3, mask3, nullptr, n3, w3}},
               lo, hi, l1 ? 1 : 0, nterms, workspace, record, nullptr, loss};
    return disp_entry(a, false, workspace_bytes, stream);
}

extern "C" int ss_disparity_loss_bwd(const float* est0, const float* gt0, const unsigned char* mask0, float* grad0, long long n0,
                                     const float* est1, const float* gt1, const unsigned char* mask1, float* grad1, long long n1,
                                     const float* est2, const float* gt2, const unsigned char* mask2, float* grad2, long long n2,
                                     const float* est3, const float* gt3, const unsigned char* mask3, float* grad3, long long n3, float w0,
                                     float w1, float w2, float w3, float lo, float hi, int nterms, int l1, const double* record,
                                     const float* grad_loss, ss_stream_t stream) {
    DispArgs a{{{est0, gt0, mask0, grad0, n0, w0}, {est1, gt1, mask1, grad1, n1, w1}, {est2, gt2, mask2, grad2, n2, w2},
                {est3, gt3, mask3, grad3, n3, w3}},
               lo, hi, l1 ? 1 : 0, nterms, nullptr, const_cast<double*>(record), grad_loss, nullptr};
    return disp_entry(a, true, 0, stream);
}

extern "C" int ss_label_loss_fwd(const float* logits, const void* labels, int label_dtype, int B, int num_classes, int H, int W, int ignore,
                                 float scale, double* record, float* loss, double* workspace, long long workspace_bytes,
                                 ss_stream_t stream) {
    LabelArgs a{logits, labels, nullptr, nullptr, nullptr, workspace, record, nullptr, loss, B, H, W, ignore, 1, scale};
    return label_entry(a, label_dtype, num_classes, false, workspace_bytes, stream);
}

extern "C" int ss_label_loss_bwd(const float* logits, const void* labels, int label_dtype, int B, int num_classes, int H, int W, int ignore,
                                 float scale, const double* record, const float* grad_loss, float* grad_logits, ss_stream_t stream) {
    LabelArgs a{logits, labels, nullptr, grad_logits, nullptr, nullptr, const_cast<double*>(record), grad_loss, nullptr, B, H, W, ignore, 1,
                scale};
    return label_entry(a, label_dtype, num_classes, true, 0, stream);
}

extern "C" int ss_lrsc_loss_fwd(const float* logits_right, const float* disp, const void* labels, int label_dtype, int B, int num_classes,
                                int H, int W, double* record, float* loss, long long* warped, double* workspace, long long workspace_bytes,
                                ss_stream_t stream) {
    SS_REQUIRE(disp);
    LabelArgs a{logits_right, labels, disp, nullptr, warped, workspace, record, nullptr, loss, B, H, W, -1, 0, 1.f};
    return label_entry(a, label_dtype, num_classes, false, workspace_bytes, stream);
}

extern "C" int ss_lrsc_loss_bwd(const float* logits_right, const float* disp, const void* labels, int label_dtype, int B, int num_classes,
                                int H, int W, const double* record, const float* grad_loss, float* grad_logits, ss_stream_t stream) {
    SS_REQUIRE(disp);
    LabelArgs a{logits_right, labels, disp, grad_logits, nullptr, nullptr, const_cast<double*>(record), grad_loss, nullptr, B, H, W, -1, 0,
                1.f};
    return label_entry(a, label_dtype, num_classes, true, 0, stream);
}
