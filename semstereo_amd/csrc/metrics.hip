// The evaluation step's metrics (main_us3d.py:225-263; utils/metrics.py): EPE / D1 / Thres of up to four estimates against one ground
// truth in one pass, and the joint histogram of (label, argmax of the logits) behind the confusion matrix.  Both are streaming
// reductions in the form of stream.h.  Counts are integers from the thread up; the error sum is fp32 per thread (a few dozen terms) and
// a double from the wave reduction on.  Nothing here allocates, copies or synchronises, and nothing comes back to the host.
#include "common.h"
#include "metrics_decode.h"
#include "stream.h"

namespace {

using namespace ss::metrics;   // NC, NBIN, LT_*, label_row, argmax6
using namespace ss::stream;    // BLOCK, grid_for, aligned_to, aligned16, wave_sum, block_sum

constexpr int GM = 1024;       // workgroups of the disparity metrics, all images together
constexpr int GC = 1024;       // workgroups of the confusion matrix
constexpr int NEST = 4, NTHR = 4;
constexpr int NCNT = 8;        // record of counts per (estimate, image): n_sel, n_mask, n_pos, n_d1, n_thr[4]

// ---------------------------------------------------------------- EPE / D1 / Thres (utils/metrics.py:16-59, :63-89)
struct MetricArgs {
    const float* est[NEST];
    const float* gt;
    const unsigned char* mask;         // bool tensor, or NULL: lo <= gt < hi
    const unsigned char* mask_img;     // bool tensor: the selection of the *_mask variants, or NULL: the selection is the mask
    float lo, hi;
    float thr[NTHR];                   // unused ones are +inf
    int nest, nthr, B;
    long long n;                       // pixels per image
    double* ws;                        // [B][gridDim.x][3 + 6 * nest]
    long long* counts;                 // [nest][B][NCNT]
    double* sums;                      // [nest][B]
    float* out;                        // [nest][2 + nthr]: EPE, D1, Thres...
};

template <int NE>
struct MetricAcc {
    float s[NE];
    int t[NE][NTHR], d1[NE];
    int sel, msk, pos;
};

// E / |gt| is the correctly rounded quotient and the test stays in this form: the counts are compared with the reference's as integers
template <int NE>
__device__ __forceinline__ void metric_point(const MetricArgs& a, float g, const float (&e)[NE], unsigned char m, unsigned char mi,
                                             MetricAcc<NE>& acc) {
    const bool inmask = a.mask ? m != 0 : (g >= a.lo && g < a.hi);
    const bool sel = a.mask_img ? mi != 0 : inmask;
    acc.msk += inmask;
    acc.pos += g > 0.f;
    acc.sel += sel;
    const float ag = fabsf(g);
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        const float E = fabsf(g - e[k]);
        if (sel) acc.s[k] += E;
#pragma unroll
        for (int t = 0; t < NTHR; ++t) acc.t[k][t] += sel && E > a.thr[t];
        acc.d1[k] += sel && E > 3.f && E / ag > 0.05f;
    }
}

// grid (G, B): image blockIdx.y.  Partial of a workgroup, as doubles: n_sel, n_mask, n_pos, then per estimate sum E, n_d1, n_thr[4].
template <int NE>
__global__ __launch_bounds__(BLOCK) void disp_metrics_k(MetricArgs a) {
    constexpr int NI = 3 + 5 * NE;
    __shared__ double lds_d[4 * NE];
    __shared__ int lds_i[4 * NI];
    const long long base = (long long)blockIdx.y * a.n;
    const float* gt = a.gt + base;
    const unsigned char* mask = a.mask ? a.mask + base : nullptr;
    const unsigned char* mimg = a.mask_img ? a.mask_img + base : nullptr;
    const float* est[NE];
    bool vec = aligned16(gt) && aligned_to(mask, 4) && aligned_to(mimg, 4);        // (a null mask passes)
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        est[k] = a.est[k] + base;
        vec = vec && aligned16(est[k]);
    }
    const long long stride = (long long)gridDim.x * BLOCK, first = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const long long n4 = vec ? a.n / 4 : 0;
    MetricAcc<NE> acc = {};
    for (long long i = first; i < n4; i += stride) {
        const float4 g = reinterpret_cast<const float4*>(gt)[i];
        float4 ev[NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) ev[k] = reinterpret_cast<const float4*>(est[k])[i];
        uchar4 m = make_uchar4(0, 0, 0, 0), mi = make_uchar4(0, 0, 0, 0);
        if (mask) m = reinterpret_cast<const uchar4*>(mask)[i];
        if (mimg) mi = reinterpret_cast<const uchar4*>(mimg)[i];
        float e[NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) e[k] = ev[k].x;
        metric_point<NE>(a, g.x, e, m.x, mi.x, acc);
#pragma unroll
        for (int k = 0; k < NE; ++k) e[k] = ev[k].y;
        metric_point<NE>(a, g.y, e, m.y, mi.y, acc);
#pragma unroll
        for (int k = 0; k < NE; ++k) e[k] = ev[k].z;
        metric_point<NE>(a, g.z, e, m.z, mi.z, acc);
#pragma unroll
        for (int k = 0; k < NE; ++k) e[k] = ev[k].w;
        metric_point<NE>(a, g.w, e, m.w, mi.w, acc);
    }
    for (long long i = n4 * 4 + first; i < a.n; i += stride) {
        float e[NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) e[k] = est[k][i];
        metric_point<NE>(a, gt[i], e, mask ? mask[i] : 0, mimg ? mimg[i] : 0, acc);
    }
    // the counts stay integers
    int ci[NI];
    double cd[NE];
    ci[0] = acc.sel;
    ci[1] = acc.msk;
    ci[2] = acc.pos;
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        cd[k] = (double)acc.s[k];
        ci[3 + 5 * k] = acc.d1[k];
#pragma unroll
        for (int t = 0; t < NTHR; ++t) ci[4 + 5 * k + t] = acc.t[k][t];
    }
    block_sum<NE>(cd, lds_d);
    block_sum<NI>(ci, lds_i);
    if (threadIdx.x == 0) {
        double* p = a.ws + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * (3 + 6 * NE);
        p[0] = (double)ci[0];
        p[1] = (double)ci[1];
        p[2] = (double)ci[2];
#pragma unroll
        for (int k = 0; k < NE; ++k) {
            p[3 + 6 * k] = cd[k];
#pragma unroll
            for (int t = 0; t < 5; ++t) p[4 + 6 * k + t] = (double)ci[3 + 5 * k + t];
        }
    }
}

// One workgroup.  Per image: the partials in a fixed order (thread = slot x one of 8 interleaved runs of workgroups), the record.
// Then per (estimate, value): the skip rule of utils/metrics.py:25 from the integer counts (n_mask / n_pos < 0.1 in double; the image
// size cancels; x / 0 = inf and 0 / 0 = NaN keep the image), the per-image values in double, their mean over the kept images in
// image order; 0 where no image is kept, NaN where a kept image has an empty selection.
__global__ __launch_bounds__(BLOCK) void disp_metrics_finish_k(MetricArgs a, int G) {
    __shared__ double lds[8][32];
    const int S = 3 + 6 * a.nest, slot = threadIdx.x & 31, run = threadIdx.x >> 5;
    for (int b = 0; b < a.B; ++b) {
        double v = 0.0;
        if (slot < S)
            for (int g = run; g < G; g += 8) v += a.ws[((long long)b * G + g) * S + slot];
        __syncthreads();
        lds[run][slot] = v;
        __syncthreads();
        if (threadIdx.x < S) {
            const int s = threadIdx.x;
            const double tot = ((lds[0][s] + lds[1][s]) + (lds[2][s] + lds[3][s])) + ((lds[4][s] + lds[5][s]) + (lds[6][s] + lds[7][s]));
            if (s < 3) {
                for (int e = 0; e < a.nest; ++e) a.counts[((long long)e * a.B + b) * NCNT + s] = (long long)tot;
            } else {
                const int e = (s - 3) / 6, q = (s - 3) % 6;
                if (q == 0)
                    a.sums[(long long)e * a.B + b] = tot;
                else
                    a.counts[((long long)e * a.B + b) * NCNT + 2 + q] = (long long)tot;
            }
        }
    }
    __syncthreads();
    const int nv = 2 + a.nthr;
    if ((int)threadIdx.x < a.nest * nv) {
        const int e = threadIdx.x / nv, q = threadIdx.x % nv;
        double acc = 0.0;
        int kept = 0;
        for (int b = 0; b < a.B; ++b) {
            const long long* c = a.counts + ((long long)e * a.B + b) * NCNT;
            if ((double)c[1] / (double)c[2] < 0.1) continue;
            const double num = q == 0 ? a.sums[(long long)e * a.B + b] : (double)c[2 + q];
            acc += num / (double)c[0];
            ++kept;
        }
        a.out[threadIdx.x] = kept ? (float)(acc / (double)kept) : 0.f;
    }
}

// ---------------------------------------------------------------- confusion matrix (utils/metrics.py:143-168)
struct ConfArgs {
    const float* z;            // logits [B,NC,H,W]
    const void* y;             // labels, at least [B,H,W]: pixel (b, h, x) at b * y_img + h * y_row + x
    long long y_row, y_img;
    int B, H, W;
    int* ws;                   // [gridDim.x][NBIN]
    long long* out;            // [NC + 1][NC]
    int accumulate;
};

// How a wave counts 42 bins: every lane owns a column of the workgroup's histogram in LDS, hist[bin][lane], and adds 1 to it with a
// ds_add_u32 that returns nothing.  The 64 lanes of one instruction hit 64 different banks whatever their bins are, so the cost does not
// depend on the data (a label map is mostly flat: with one shared row of 42 counters all lanes would queue on one address); the lanes of
// the other three waves that share a column are what the atomic is for.  At the end each bin's 64 columns are added by shuffles.
template <int LT>
__global__ __launch_bounds__(BLOCK) void seg_confusion_k(ConfArgs a) {
    __shared__ unsigned hist[NBIN * 64];
    for (int i = threadIdx.x; i < NBIN * 64; i += BLOCK) hist[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long HW = (long long)a.H * a.W, npix = HW * a.B;
    const long long stride = (long long)gridDim.x * BLOCK, first = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool flat = a.y_row == a.W && a.y_img == HW;
    const bool vec = (a.W & 3) == 0 && aligned16(a.z);          // (four pixels of a load share a row)
    const long long nq = vec ? npix / 4 : 0;
    for (long long q = first; q < nq; q += stride) {
        const long long p0 = q * 4, b = p0 / HW;
        const int r0 = (int)(p0 - b * HW);
        const float* zb = a.z + b * NC * HW + r0;
        float4 zv[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) zv[k] = *reinterpret_cast<const float4*>(zb + k * HW);
        long long yo = p0;
        if (!flat) {
            const int h = r0 / a.W;
            yo = b * a.y_img + h * a.y_row + (r0 - h * a.W);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float z[NC];
#pragma unroll
            for (int k = 0; k < NC; ++k) z[k] = j == 0 ? zv[k].x : j == 1 ? zv[k].y : j == 2 ? zv[k].z : zv[k].w;
            const int bin = label_row<LT>(a.y, yo + j) * NC + argmax6(z);
            atomicAdd(&hist[bin * 64 + lane], 1u);
        }
    }
    for (long long p = nq * 4 + first; p < npix; p += stride) {
        const long long b = p / HW;
        const int r = (int)(p - b * HW), h = r / a.W;
        const float* zb = a.z + b * NC * HW + r;
        float z[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) z[k] = zb[k * HW];
        const int bin = label_row<LT>(a.y, b * a.y_img + h * a.y_row + (r - h * a.W)) * NC + argmax6(z);
        atomicAdd(&hist[bin * 64 + lane], 1u);
    }
    __syncthreads();
    for (int k = wave; k < NBIN; k += 4) {
        const int v = wave_sum((int)hist[k * 64 + lane]);
        if (lane == 0) a.ws[(long long)blockIdx.x * NBIN + k] = v;
    }
}

// grid NBIN: workgroup k adds the partials of bin k and writes the sum to the caller's matrix, or adds it (integers: any order gives
// the same bits)
__global__ __launch_bounds__(BLOCK) void seg_confusion_finish_k(ConfArgs a, int G) {
    __shared__ long long lds[4];
    const int k = blockIdx.x;
    long long v[1] = {0};
    for (int g = threadIdx.x; g < G; g += BLOCK) v[0] += a.ws[(long long)g * NBIN + k];
    block_sum<1>(v, lds);
    if (threadIdx.x == 0) a.out[k] = a.accumulate ? a.out[k] + v[0] : v[0];
}

template <int NE>
int metrics_launch(const MetricArgs& a, int G, hipStream_t st) {
    hipLaunchKernelGGL(disp_metrics_k<NE>, dim3(G, a.B), dim3(BLOCK), 0, st, a);
    if (int s = ss::check_launch()) return s;
    hipLaunchKernelGGL(disp_metrics_finish_k, dim3(1), dim3(BLOCK), 0, st, a, G);
    return ss::check_launch();
}

template <int LT>
int confusion_launch(const ConfArgs& a, hipStream_t st) {
    const int G = grid_for(ss::ceil_div_ll((long long)a.B * a.H * a.W, 4), GC);
    hipLaunchKernelGGL(seg_confusion_k<LT>, dim3(G), dim3(BLOCK), 0, st, a);
    if (int s = ss::check_launch()) return s;
    hipLaunchKernelGGL(seg_confusion_finish_k, dim3(NBIN), dim3(BLOCK), 0, st, a, G);
    return ss::check_launch();
}

}  // namespace

extern "C" int ss_metrics_workspace_bytes(int kind, long long* bytes) {
    SS_REQUIRE(bytes && (kind == 0 || kind == 1));
    *bytes = kind == 0 ? (long long)GM * (3 + 6 * NEST) * 8 : (long long)GC * NBIN * 4;
    return SS_OK;
}

extern "C" int ss_disparity_metrics_fwd(const float* est0, const float* est1, const float* est2, const float* est3, const float* gt,
                                        const unsigned char* mask, const unsigned char* mask_img, int n_est, int B,
                                        long long pixels_per_image, float lo, float hi, float t0, float t1, float t2, float t3, int n_thr,
                                        float* out, long long* counts, double* sums, void* workspace, long long workspace_bytes,
                                        ss_stream_t stream) {
    const float inf = __builtin_huge_valf();
    MetricArgs a{{est0, est1, est2, est3}, gt, mask, mask_img, lo, hi, {t0, t1, t2, t3}, n_est, n_thr, B, pixels_per_image,
                 static_cast<double*>(workspace), counts, sums, out};
    SS_REQUIRE(n_est >= 1 && n_est <= NEST && n_thr >= 0 && n_thr <= NTHR && B > 0 && pixels_per_image > 0);
    SS_REQUIRE(gt && out && counts && sums && workspace && workspace_bytes >= (long long)GM * (3 + 6 * NEST) * 8);
    for (int i = 0; i < NEST; ++i) {
        if (i < n_est) SS_REQUIRE(a.est[i] != nullptr);
        if (i >= n_thr) a.thr[i] = inf;
    }
    if (B > GM || pixels_per_image >= 0x7fffffffLL) return SS_ERR_UNSUPPORTED;
    const int G = grid_for(ss::ceil_div_ll(pixels_per_image, 4), GM / B);
    hipStream_t st = ss::as_stream(stream);
    switch (n_est) {
    case 1:
        return metrics_launch<1>(a, G, st);
    case 2:
        return metrics_launch<2>(a, G, st);
    case 3:
        return metrics_launch<3>(a, G, st);
    default:
        return metrics_launch<4>(a, G, st);
    }
}

extern "C" int ss_seg_confusion_fwd(const float* logits, const void* labels, int label_dtype, int B, int num_classes, int H, int W,
                                    long long label_row_stride, long long label_image_stride, long long* joint, int accumulate,
                                    void* workspace, long long workspace_bytes, ss_stream_t stream) {
    SS_REQUIRE(logits && labels && joint && workspace && B > 0 && H > 0 && W > 0);
    SS_REQUIRE(label_dtype >= LT_I64 && label_dtype <= LT_F32 && workspace_bytes >= (long long)GC * NBIN * 4);
    SS_REQUIRE(label_row_stride >= W && label_image_stride >= (long long)(H - 1) * label_row_stride + W);
    if (num_classes != NC || (long long)B * H * W * NC >= 0x7fffffffLL) return SS_ERR_UNSUPPORTED;
    ConfArgs a{logits, labels, label_row_stride, label_image_stride, B, H, W, static_cast<int*>(workspace), joint, accumulate ? 1 : 0};
    hipStream_t st = ss::as_stream(stream);
    switch (label_dtype) {
    case LT_I64:
        return confusion_launch<LT_I64>(a, st);
    case LT_U8:
        return confusion_launch<LT_U8>(a, st);
    default:
        return confusion_launch<LT_F32>(a, st);
    }
}
