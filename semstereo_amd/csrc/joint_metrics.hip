// The joint stereo-semantic record of one batch: disparity error per semantic class and the confusion matrix gated by the disparity
// error (mIoU-3), from ONE pass over the tensors eval_metrics reads -- up to four estimates, the ground truth, the mask (or its range),
// the six logits and the label map.  A streaming reduction of the stream.h family on a grid (G, B), image blockIdx.y, which keeps
// summation orders of its own: the histogram columns and the per-class sums below are not the shape of stream.h's block_sum, and
// their order is part of the recorded bits.
//
// Where the numbers live (profiles/EXPERIMENTS.md section U):
//   every integer count   a histogram in LDS, hist[bin][column], column = lane & 31, added to with a ds_add_u32 that returns nothing.
//                         Lanes l and l + 32 of a 4-byte LDS instruction are served in different cycles, so 32 columns cost what 64
//                         do and the cost does not depend on the data; 128 B per bin keeps four estimates at 401 bins = 50 KB.
//   the error sums        doubles in registers from the thread on, one per (estimate, class), chosen by a compile-time class loop: a
//                         sum of fp32 values in double is the only form whose error stays at the 2^-53 per term that the record's
//                         consumers are checked against.  7 x n_est doubles: 56 VGPRs at four estimates, no scratch.
// Each workgroup leaves one partial (doubles, then 32-bit counts) in the caller's workspace; a second launch adds the partials in a fixed
// order.  Nothing allocates, copies, synchronises or returns to the host.
#include "common.h"
#include "metrics_decode.h"
#include "stream.h"

namespace {

using namespace ss::metrics;
using namespace ss::stream;    // BLOCK, grid_for, aligned_to, aligned16, wave_sum

constexpr int COLS = 32;       // columns of a histogram bin
constexpr int GJ = 1024;       // workgroups of the reduction, all images together: image b gets GJ / B of them at most ...
constexpr int GI = 512;        // ... and never more than this: two per CU, and half the partials for the finish to read (section U)
constexpr int NEST = 4, NTHR = 4;
constexpr int NCLS = NC + 1;   // label classes and "outside"
constexpr int NFLAG = 1 + NTHR;            // n_d1, n_thr[4]
// bins of an image's histogram
constexpr int B_SEL = 0;                   // [NCLS]           pixels in the mask, per class
constexpr int B_ALL = B_SEL + NCLS;        // [NCLS][NC]       every pixel
constexpr int B_OUT = B_ALL + NBIN;        // [NCLS][NC]       pixels outside the mask
constexpr int B_EST = B_OUT + NBIN;        // per estimate: [NCLS][NC] good pixels, then [NCLS][NFLAG] flags of the pixels in the mask
constexpr int EST_BINS = NBIN + NCLS * NFLAG;
__host__ __device__ constexpr int bins_of(int ne) { return B_EST + ne * EST_BINS + 2; }       // ..., n_mask, n_pos
__host__ __device__ constexpr int ints_of(int ne) { return (bins_of(ne) + 1) & ~1; }          // (the doubles of the next partial stay aligned)
__host__ __device__ constexpr long long partial_bytes(int ne) { return (long long)ne * NCLS * 8 + (long long)ints_of(ne) * 4; }

struct JointArgs {
    const float* est[NEST];
    const float* gt;
    const unsigned char* mask;         // bool tensor, or NULL: lo <= gt < hi
    const float* z;                    // logits [B,NC,H,W], or NULL: no joint tables
    const void* y;                     // labels: pixel (b, h, x) at b * y_img + h * y_row + x
    long long y_row, y_img;
    float lo, hi, tau;
    float thr[NTHR];                   // unused ones are +inf
    int nest, B, H, W;
    char* ws;                          // [B][gridDim.x] partials: doubles [nest][NCLS], then ints [ints_of(nest)]
    long long *image, *cls_sel, *cls_counts;
    double* cls_sums;
    long long *joint_all, *joint_out, *joint_good;
};

// four labels of one row, as classes: wide loads where the caller found every group of four aligned
template <int LT>
__device__ __forceinline__ void label4(const void* y, long long o, bool wide, int (&g)[4]) {
    if (wide) {
        if (LT == LT_I64) {
            const longlong2 u = *reinterpret_cast<const longlong2*>(reinterpret_cast<const long long*>(y) + o);
            const longlong2 v = *reinterpret_cast<const longlong2*>(reinterpret_cast<const long long*>(y) + o + 2);
            g[0] = label_class((long long)u.x), g[1] = label_class((long long)u.y);
            g[2] = label_class((long long)v.x), g[3] = label_class((long long)v.y);
        } else if (LT == LT_U8) {
            const uchar4 v = *reinterpret_cast<const uchar4*>(reinterpret_cast<const unsigned char*>(y) + o);
            g[0] = label_class(v.x), g[1] = label_class(v.y), g[2] = label_class(v.z), g[3] = label_class(v.w);
        } else {
            const float4 v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(y) + o);
            g[0] = label_class(v.x), g[1] = label_class(v.y), g[2] = label_class(v.z), g[3] = label_class(v.w);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = label_row<LT>(y, o + j);
    }
}

template <int NE>
struct JointAcc {
    double sum[NE][NCLS];
    int msk, pos;
};

// One pixel.  E / |gt| is the correctly rounded quotient and the test stays in this form, as in disp_metrics_k.  `good` is E < tau:
// a NaN E and E == tau are not good.  A pixel outside the mask adds +0.0 to its class's sums, whatever its E is.
template <int NE>
__device__ __forceinline__ void joint_point(const JointArgs& a, unsigned* col, float g, const float (&e)[NE], unsigned char m, int cls,
                                            int p, JointAcc<NE>& acc) {
    const bool in = a.mask ? m != 0 : (g >= a.lo && g < a.hi);
    const bool joint = a.z != nullptr;
    const int bin = cls * NC + p;
    acc.msk += in;
    acc.pos += g > 0.f;
    if (joint) atomicAdd(col + (B_ALL + bin) * COLS, 1u);
    if (in)
        atomicAdd(col + (B_SEL + cls) * COLS, 1u);
    else if (joint)
        atomicAdd(col + (B_OUT + bin) * COLS, 1u);
    const float ag = fabsf(g);
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        const float E = fabsf(g - e[k]);
        if (in) {
            unsigned* ck = col + (B_EST + k * EST_BINS) * COLS;
            if (joint && E < a.tau) atomicAdd(ck + bin * COLS, 1u);
            unsigned* cf = ck + (NBIN + cls * NFLAG) * COLS;
            if (E > 3.f && E / ag > 0.05f) atomicAdd(cf, 1u);
#pragma unroll
            for (int t = 0; t < NTHR; ++t)
                if (E > a.thr[t]) atomicAdd(cf + (1 + t) * COLS, 1u);
        }
        const double Ed = in ? (double)E : 0.0;
#pragma unroll
        for (int c = 0; c < NCLS; ++c) acc.sum[k][c] += cls == c ? Ed : 0.0;
    }
}

// grid (G, B): image blockIdx.y
template <int NE, int LT>
__global__ __launch_bounds__(BLOCK) void joint_metrics_k(JointArgs a) {
    constexpr int NB = bins_of(NE);
    __shared__ unsigned hist[NB * COLS];
    __shared__ double lds_d[NCLS * BLOCK];
    for (int i = threadIdx.x; i < NB * COLS; i += BLOCK) hist[i] = 0u;
    __syncthreads();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    unsigned* col = hist + (lane & (COLS - 1));
    const int n = a.H * a.W;                                   // (< 2^31: checked by the caller)
    const long long base = (long long)b * n;
    const float* gt = a.gt + base;
    const unsigned char* mask = a.mask ? a.mask + base : nullptr;
    const float* z = a.z ? a.z + base * NC : nullptr;
    const float* est[NE];
    bool vec = (a.W & 3) == 0 && aligned16(gt) && aligned_to(mask, 4) && (!z || aligned16(z));
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        est[k] = a.est[k] + base;
        vec = vec && aligned16(est[k]);
    }
    const bool ywide = ((a.y_row | a.y_img) & 3) == 0 && aligned_to(a.y, LT == LT_U8 ? 4 : 16);
    const long long ybase = (long long)b * a.y_img;
    const int stride = gridDim.x * BLOCK, first = blockIdx.x * BLOCK + tid;
    const int n4 = vec ? n / 4 : 0;                            // (W % 4 == 0: four pixels of a load share a row, and n4 * 4 == n)
    JointAcc<NE> acc = {};
    for (long long q = first; q < n4; q += stride) {
        const int r0 = (int)q * 4, h = r0 / a.W;
        const float4 gv = reinterpret_cast<const float4*>(gt)[q];
        float4 ev[NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) ev[k] = reinterpret_cast<const float4*>(est[k])[q];
        uchar4 mv = make_uchar4(0, 0, 0, 0);
        if (mask) mv = reinterpret_cast<const uchar4*>(mask)[q];
        float4 zv[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) zv[k] = z ? *reinterpret_cast<const float4*>(z + (long long)k * n + r0) : make_float4(0.f, 0.f, 0.f, 0.f);
        int cls[4];
        label4<LT>(a.y, ybase + (long long)h * a.y_row + (r0 - h * a.W), ywide, cls);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float e[NE], zz[NC];
#pragma unroll
            for (int k = 0; k < NE; ++k) e[k] = j == 0 ? ev[k].x : j == 1 ? ev[k].y : j == 2 ? ev[k].z : ev[k].w;
#pragma unroll
            for (int k = 0; k < NC; ++k) zz[k] = j == 0 ? zv[k].x : j == 1 ? zv[k].y : j == 2 ? zv[k].z : zv[k].w;
            const float g = j == 0 ? gv.x : j == 1 ? gv.y : j == 2 ? gv.z : gv.w;
            const unsigned char m = j == 0 ? mv.x : j == 1 ? mv.y : j == 2 ? mv.z : mv.w;
            joint_point<NE>(a, col, g, e, m, cls[j], z ? argmax6(zz) : 0, acc);
        }
    }
    for (long long r = (long long)n4 * 4 + first; r < n; r += stride) {
        const int h = (int)r / a.W;
        float e[NE], zz[NC];
#pragma unroll
        for (int k = 0; k < NE; ++k) e[k] = est[k][r];
#pragma unroll
        for (int k = 0; k < NC; ++k) zz[k] = z ? z[(long long)k * n + r] : 0.f;
        const int cls = label_row<LT>(a.y, ybase + (long long)h * a.y_row + ((int)r - h * a.W));
        joint_point<NE>(a, col, gt[r], e, mask ? mask[r] : 0, cls, z ? argmax6(zz) : 0, acc);
    }
    // the partial: counts first.  n_mask and n_pos join the histogram through the wave; then thread t adds the 32 columns of bins
    // t, t + 256, ... (rotated by t, so the lanes of a read hit 32 different banks); integers, any order gives the same bits
    const int msk = wave_sum(acc.msk), pos = wave_sum(acc.pos);
    if (lane == 0) {
        atomicAdd(hist + (NB - 2) * COLS, (unsigned)msk);
        atomicAdd(hist + (NB - 1) * COLS, (unsigned)pos);
    }
    __syncthreads();
    char* part = a.ws + ((long long)b * gridDim.x + blockIdx.x) * partial_bytes(NE);
    double* pd = reinterpret_cast<double*>(part);
    unsigned* pi = reinterpret_cast<unsigned*>(part + NE * NCLS * 8);
    for (int k = tid; k < NB; k += BLOCK) {
        unsigned v = 0u;
#pragma unroll 8
        for (int j = 0; j < COLS; ++j) v += hist[k * COLS + ((j + tid) & (COLS - 1))];
        pi[k] = v;
    }
    // ... then the sums, one estimate at a time: thread -> LDS -> wave c adds class c, c + 4 (four values per lane, then shuffles)
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NCLS; ++c) lds_d[c * BLOCK + tid] = acc.sum[k][c];
        __syncthreads();
        for (int c = wave; c < NCLS; c += 4) {
            const double* v = lds_d + c * BLOCK + lane;
            const double s = wave_sum((v[0] + v[64]) + (v[128] + v[192]));
            if (lane == 0) pd[k * NCLS + c] = s;
        }
    }
}

// grid (FD + ceil(bins / 8), B) with FD = 4: workgroups x < FD add the sums, workgroup x >= FD the counts 8 (x - FD) ... of image
// blockIdx.y.  A thread is (slot, one of 32 interleaved runs of partials), sixteen loads in flight -- the partials of one slot lie a
// partial apart, so this launch is bound by the latency of its loads, not their bytes; the runs are combined in a fixed order.
constexpr int FS = 8, FR = BLOCK / FS, FD = (NEST * NCLS + FS - 1) / FS;
__global__ __launch_bounds__(BLOCK) void joint_metrics_finish_k(JointArgs a, int G) {
    __shared__ double lds_d[FR][FS];
    __shared__ long long lds_i[FR][FS];
    const int slot = threadIdx.x & (FS - 1), run = threadIdx.x / FS, b = blockIdx.y, ne = a.nest;
    const long long pb = partial_bytes(ne);
    const char* part = a.ws + (long long)b * G * pb;
    if (blockIdx.x < FD) {
        const int s = blockIdx.x * FS + slot;
        double v = 0.0;
        if (s < ne * NCLS) {
#pragma unroll 16
            for (int g = run; g < G; g += FR) v += reinterpret_cast<const double*>(part + g * pb)[s];
        }
        lds_d[run][slot] = v;
        __syncthreads();
        if (threadIdx.x < FS && s < ne * NCLS) {
            double tot = lds_d[0][slot];
#pragma unroll
            for (int r = 1; r < FR; ++r) tot += lds_d[r][slot];
            a.cls_sums[((long long)(s / NCLS) * a.B + b) * NCLS + s % NCLS] = tot;
        }
        return;
    }
    const int nb = bins_of(ne), s = (blockIdx.x - FD) * FS + slot;
    long long v = 0;
    if (s < nb) {
#pragma unroll 16
        for (int g = run; g < G; g += FR) v += reinterpret_cast<const unsigned*>(part + g * pb + ne * NCLS * 8)[s];
    }
    lds_i[run][slot] = v;
    __syncthreads();
    if (threadIdx.x < FS && s < nb) {
        long long tot = 0;
#pragma unroll
        for (int r = 0; r < FR; ++r) tot += lds_i[r][slot];
        if (s >= nb - 2) {
            a.image[b * 2 + (s - (nb - 2))] = tot;
        } else if (s < B_ALL) {
            a.cls_sel[b * NCLS + s] = tot;
        } else if (s < B_EST) {
            if (a.z) (s < B_OUT ? a.joint_all : a.joint_out)[b * NBIN + (s - B_ALL) % NBIN] = tot;
        } else {
            const int k = (s - B_EST) / EST_BINS, r = (s - B_EST) % EST_BINS;
            const long long kb = (long long)k * a.B + b;
            if (r >= NBIN)
                a.cls_counts[kb * (NCLS * NFLAG) + (r - NBIN)] = tot;
            else if (a.z)
                a.joint_good[kb * NBIN + r] = tot;
        }
    }
}

template <int NE, int LT>
int joint_launch(const JointArgs& a, int G, hipStream_t st) {
    hipLaunchKernelGGL((joint_metrics_k<NE, LT>), dim3(G, a.B), dim3(BLOCK), 0, st, a);
    if (int s = ss::check_launch()) return s;
    hipLaunchKernelGGL(joint_metrics_finish_k, dim3(FD + ss::ceil_div(bins_of(NE), FS), a.B), dim3(BLOCK), 0, st, a, G);
    return ss::check_launch();
}

template <int NE>
int joint_launch_lt(const JointArgs& a, int lt, int G, hipStream_t st) {
    switch (lt) {
    case LT_I64:
        return joint_launch<NE, LT_I64>(a, G, st);
    case LT_U8:
        return joint_launch<NE, LT_U8>(a, G, st);
    default:
        return joint_launch<NE, LT_F32>(a, G, st);
    }
}

}  // namespace

extern "C" int ss_joint_metrics_scratch(int n_est, int B, long long* bytes) {
    SS_REQUIRE(bytes && n_est >= 1 && n_est <= NEST && B > 0);
    if (B > GJ) return SS_ERR_UNSUPPORTED;
    *bytes = (long long)GJ * partial_bytes(n_est);
    return SS_OK;
}

extern "C" int ss_joint_metrics_fwd(const float* est0, const float* est1, const float* est2, const float* est3, const float* gt,
                                    const unsigned char* mask, const float* logits, const void* labels, int label_dtype,
                                    long long label_row_stride, long long label_image_stride, int n_est, int B, int num_classes, int H,
                                    int W, float lo, float hi, float t0, float t1, float t2, float t3, int n_thr, float tau,
                                    long long* image, long long* cls_sel, long long* cls_counts, double* cls_sums, long long* joint_all,
                                    long long* joint_out, long long* joint_good, void* workspace, long long workspace_bytes,
                                    ss_stream_t stream) {
    const float inf = __builtin_huge_valf();
    SS_REQUIRE(n_est >= 1 && n_est <= NEST && n_thr >= 0 && n_thr <= NTHR && B > 0 && H > 0 && W > 0);
    SS_REQUIRE(gt && labels && image && cls_sel && cls_counts && cls_sums && workspace);
    SS_REQUIRE(!logits || (joint_all && joint_out && joint_good));
    SS_REQUIRE(label_dtype >= LT_I64 && label_dtype <= LT_F32);
    SS_REQUIRE(label_row_stride >= W && label_image_stride >= (long long)(H - 1) * label_row_stride + W);
    SS_REQUIRE(workspace_bytes >= (long long)GJ * partial_bytes(n_est));
    JointArgs a{{est0, est1, est2, est3}, gt, mask, logits, labels, label_row_stride, label_image_stride, lo, hi, tau, {t0, t1, t2, t3},
                n_est, B, H, W, static_cast<char*>(workspace), image, cls_sel, cls_counts, cls_sums, joint_all, joint_out, joint_good};
    for (int i = 0; i < NEST; ++i) {
        if (i < n_est) SS_REQUIRE(a.est[i] != nullptr);
        if (i >= n_thr) a.thr[i] = inf;
    }
    if (num_classes != NC || B > GJ || (long long)H * W >= 0x7fffffffLL) return SS_ERR_UNSUPPORTED;
    const int G = grid_for(ss::ceil_div_ll((long long)H * W, 4), GJ / B < GI ? GJ / B : GI);
    hipStream_t st = ss::as_stream(stream);
    switch (n_est) {
    case 1:
        return joint_launch_lt<1>(a, label_dtype, G, st);
    case 2:
        return joint_launch_lt<2>(a, label_dtype, G, st);
    case 3:
        return joint_launch_lt<3>(a, label_dtype, G, st);
    default:
        return joint_launch_lt<4>(a, label_dtype, G, st);
    }
}
