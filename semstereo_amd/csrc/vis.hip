// The evaluation step's image outputs (main_us3d.py:252, :265-268; main_whu.py:242, :250-251): the D1-style error map of
// utils/visualization.py:30-55, the class colours of utils/mask_vis.py:5-31 and the per-image min/max normalisation that
// utils/experiment.py:84-99 asks of make_grid.  All of them are streaming passes of the stream.h family: a lane takes a row quad (4
// consecutive pixels of one row) and writes the planar [B,3,H,W] result; labels and logits are decoded by metrics_decode.h, as the
// confusion matrix decodes them.  Element offsets are 64-bit.  Every division is the IEEE one (no reciprocal, no fast-math): the error
// map is compared with the reference's bit for bit.  Nothing here allocates, copies or synchronises, and nothing comes back to the host.
#include "common.h"
#include "metrics_decode.h"
#include "stream.h"

namespace {

using namespace ss::metrics;   // NC (the palette of utils/mask_vis.py:10-15 has as many colours), LT_*, label_class, argmax_take
using namespace ss::stream;    // BLOCK, grid_for, aligned_to, block_minmax, RowQuad, row_quad, load4, store4

constexpr int GV = 2048;       // workgroups of the per-pixel passes
constexpr int GR = 1024;       // workgroups of the min/max reduction, all images together
constexpr int NBINS = 10;      // rows of the error colour table (utils/visualization.py:11-24)
constexpr int LEGEND_ROWS = 10, LEGEND_STEP = 20;          // utils/visualization.py:51-53

// ---------------------------------------------------------------- error map (utils/visualization.py:30-55)
struct ErrArgs {
    const float* est;          // [B,H,W]
    const float* gt;           // [B,H,W]
    float* out;                // [B,3,H,W]
    int B, H, W;
    float abs_thres, rel_thres;
    int legend, is_signed;
    float lo, hi;              // signed form: valid where lo <= gt < hi and gt != 0
    float bin_lo[NBINS], bin_hi[NBINS], col[NBINS][3];
};

// np.minimum: a NaN in either operand gives NaN
__device__ __forceinline__ float min_nan(float a, float b) { return (a < b || a != a) ? a : b; }

__global__ __launch_bounds__(BLOCK) void error_image_k(ErrArgs a) {
    const unsigned QW = ((unsigned)a.W + 3u) / 4u, total = (unsigned)a.B * (unsigned)a.H * QW;
    const unsigned stride = gridDim.x * BLOCK;
    const long long HW = (long long)a.H * a.W;
    for (unsigned q = blockIdx.x * BLOCK + threadIdx.x; q < total; q += stride) {
        const RowQuad r = row_quad(q, QW, (unsigned)a.H, a.W);
        const long long in = ((long long)r.b * a.H + r.h) * a.W + r.x0;
        float e[4], g[4], c[3][4];
        load4(a.est + in, r.nv, e);
        load4(a.gt + in, r.nv, g);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float gj = g[j];
            const bool valid = a.is_signed ? (gj >= a.lo && gj < a.hi && gj != 0.f) : gj > 0.f;
            const float err = fabsf(gj - e[j]);
            const float v = min_nan(err / a.abs_thres, (err / (a.is_signed ? fabsf(gj) : gj)) / a.rel_thres);
            float cr = 0.f, cg = 0.f, cb = 0.f;
#pragma unroll
            for (int i = 0; i < NBINS; ++i) {
                const bool in_bin = valid && v >= a.bin_lo[i] && v < a.bin_hi[i];
                cr = in_bin ? a.col[i][0] : cr;
                cg = in_bin ? a.col[i][1] : cg;
                cb = in_bin ? a.col[i][2] : cb;
            }
            const int x = r.x0 + j;
            if (a.legend && r.h < (unsigned)LEGEND_ROWS && x < NBINS * LEGEND_STEP) {        // also where the ground truth is invalid
                const int i = x / LEGEND_STEP;
#pragma unroll
                for (int k = 0; k < NBINS; ++k) {
                    cr = i == k ? a.col[k][0] : cr;
                    cg = i == k ? a.col[k][1] : cg;
                    cb = i == k ? a.col[k][2] : cb;
                }
            }
            c[0][j] = cr, c[1][j] = cg, c[2][j] = cb;
        }
        float* o = a.out + ((long long)r.b * 3 * a.H + r.h) * a.W + r.x0;
        store4(o, r.nv, c[0]);
        store4(o + HW, r.nv, c[1]);
        store4(o + 2 * HW, r.nv, c[2]);
    }
}

// ---------------------------------------------------------------- class colours (utils/mask_vis.py:5-31)
constexpr int SRC_LOGITS = -1;         // src_dtype: the logits, or one of LT_*

struct ColorArgs {
    const void* src;           // logits [B,C,H,W] fp32, or labels: pixel (b, h, x) at b * y_img + h * y_row + x
    void* out;                 // [B,3,H,W] float or unsigned char
    long long y_row, y_img;
    int B, C, H, W;
};

// the palette of utils/mask_vis.py:10-15 as three bit sets over the class: black, red, green, blue, yellow, cyan; class 6 = black
__device__ __forceinline__ void palette(int cls, float& r, float& g, float& b) {
    r = ((0x12 >> cls) & 1) ? 255.f : 0.f;         // classes 1, 4
    g = ((0x34 >> cls) & 1) ? 255.f : 0.f;         // classes 2, 4, 5
    b = ((0x28 >> cls) & 1) ? 255.f : 0.f;         // classes 3, 5
}

template <typename T>
__device__ __forceinline__ void label_classes(const void* y, long long off, int nv, int (&cls)[4]) {
    T v[4];
    load4(reinterpret_cast<const T*>(y) + off, nv, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) cls[j] = label_class(v[j]);
}

template <int SRC, typename OutT>
__global__ __launch_bounds__(BLOCK) void class_color_k(ColorArgs a) {
    const unsigned QW = ((unsigned)a.W + 3u) / 4u, total = (unsigned)a.B * (unsigned)a.H * QW;
    const unsigned stride = gridDim.x * BLOCK;
    const long long HW = (long long)a.H * a.W;
    for (unsigned q = blockIdx.x * BLOCK + threadIdx.x; q < total; q += stride) {
        const RowQuad r = row_quad(q, QW, (unsigned)a.H, a.W);
        int cls[4];
        if (SRC == SRC_LOGITS) {
            // argmax6's rule over the a.C <= NC channels, four pixels at a time
            const float* z = reinterpret_cast<const float*>(a.src) + ((long long)r.b * a.C * a.H + r.h) * a.W + r.x0;
            float best[4];
            load4(z, r.nv, best);
#pragma unroll
            for (int j = 0; j < 4; ++j) cls[j] = 0;
#pragma unroll
            for (int k = 1; k < NC; ++k) {
                if (k < a.C) {
                    float zk[4];
                    load4(z + k * HW, r.nv, zk);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool take = argmax_take(best[j], zk[j]);
                        best[j] = take ? zk[j] : best[j];
                        cls[j] = take ? k : cls[j];
                    }
                }
            }
        } else {
            const long long off = (long long)r.b * a.y_img + (long long)r.h * a.y_row + r.x0;
            if (SRC == LT_I64)
                label_classes<long long>(a.src, off, r.nv, cls);
            else if (SRC == LT_U8)
                label_classes<unsigned char>(a.src, off, r.nv, cls);
            else
                label_classes<float>(a.src, off, r.nv, cls);
        }
        float c[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) palette(cls[j], c[0][j], c[1][j], c[2][j]);
        OutT* o = reinterpret_cast<OutT*>(a.out) + ((long long)r.b * 3 * a.H + r.h) * a.W + r.x0;
        store4(o, r.nv, c[0]);
        store4(o + HW, r.nv, c[1]);
        store4(o + 2 * HW, r.nv, c[2]);
    }
}

// ---------------------------------------------------------------- per-image min / max and the normalisation (utils/experiment.py:98)
// grid (G, B): image blockIdx.y of n elements; the workgroup's partial goes to ws[(b * G + g) * 2 + {0, 1}]
__global__ __launch_bounds__(BLOCK) void image_minmax_k(const float* x, long long n, float* ws) {
    __shared__ float lds[8];
    const float* p = x + (long long)blockIdx.y * n;
    const long long stride = (long long)gridDim.x * BLOCK, first = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const long long n4 = aligned_to(p, 16) ? n / 4 : 0;
    const float inf = __builtin_huge_valf();
    float lo = inf, hi = -inf;
    for (long long i = first; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(p)[i];
        lo = fminf(fminf(lo, v.x), fminf(fminf(v.y, v.z), v.w));
        hi = fmaxf(fmaxf(hi, v.x), fmaxf(fmaxf(v.y, v.z), v.w));
    }
    for (long long i = n4 * 4 + first; i < n; i += stride) {
        lo = fminf(lo, p[i]);
        hi = fmaxf(hi, p[i]);
    }
    block_minmax(lo, hi, lds);
    if (threadIdx.x == 0) {
        float* w = ws + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        w[0] = lo, w[1] = hi;
    }
}

// grid B: workgroup b folds the G partials of image b (thread t takes g = t, t + 256, ...) and writes minmax[b] = {min, max}
__global__ __launch_bounds__(BLOCK) void image_minmax_finish_k(const float* ws, int G, float* minmax) {
    __shared__ float lds[8];
    const float inf = __builtin_huge_valf();
    float lo = inf, hi = -inf;
    for (int g = threadIdx.x; g < G; g += BLOCK) {
        const float* w = ws + ((long long)blockIdx.x * G + g) * 2;
        lo = fminf(lo, w[0]);
        hi = fmaxf(hi, w[1]);
    }
    block_minmax(lo, hi, lds);
    if (threadIdx.x == 0) minmax[2 * blockIdx.x] = lo, minmax[2 * blockIdx.x + 1] = hi;
}

// grid (G, B): out[b] = (clamp(x[b], lo, hi) - lo) / max(hi - lo, 1e-5) over the n = C * HW elements of image b; with C == 1 the
// result is written to three equal channels (what make_grid does to a single-channel image)
__global__ __launch_bounds__(BLOCK) void image_normalize_k(const float* x, const float* minmax, float* out, int C, long long HW) {
    const long long n = (long long)C * HW;
    const int rep = C == 1 ? 3 : 1;
    const float* p = x + (long long)blockIdx.y * n;
    float* o = out + (long long)blockIdx.y * n * rep;
    const float lo = minmax[2 * blockIdx.y], hi = minmax[2 * blockIdx.y + 1];
    const float den = fmaxf(hi - lo, 1e-5f);
    const long long stride = (long long)gridDim.x * BLOCK, first = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool vec = aligned_to(p, 16) && aligned_to(o, 16) && (rep == 1 || (HW & 3) == 0);
    const long long n4 = vec ? n / 4 : 0;
    for (long long i = first; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(p)[i];
        float4 w;
        w.x = (fminf(fmaxf(v.x, lo), hi) - lo) / den;
        w.y = (fminf(fmaxf(v.y, lo), hi) - lo) / den;
        w.z = (fminf(fmaxf(v.z, lo), hi) - lo) / den;
        w.w = (fminf(fmaxf(v.w, lo), hi) - lo) / den;
        for (int k = 0; k < rep; ++k) reinterpret_cast<float4*>(o + k * HW)[i] = w;
    }
    for (long long i = n4 * 4 + first; i < n; i += stride) {
        const float w = (fminf(fmaxf(p[i], lo), hi) - lo) / den;
        for (int k = 0; k < rep; ++k) o[k * HW + i] = w;
    }
}

// 4-pixel groups of a [B,H,W] map, or -1 where they do not fit the kernels' 32-bit numbering
long long row_quads(int B, int H, int W) {
    const long long q = (long long)B * H * (((long long)W + 3) / 4);
    return q < 0x7fffffffLL ? q : -1;
}

template <int SRC>
int color_launch(const ColorArgs& a, int out_dtype, int G, hipStream_t st) {
    if (out_dtype == 0)
        hipLaunchKernelGGL((class_color_k<SRC, float>), dim3(G), dim3(BLOCK), 0, st, a);
    else
        hipLaunchKernelGGL((class_color_k<SRC, unsigned char>), dim3(G), dim3(BLOCK), 0, st, a);
    return ss::check_launch();
}

}  // namespace

extern "C" int ss_vis_workspace_bytes(int kind, long long* bytes) {
    SS_REQUIRE(bytes && kind == 0);
    *bytes = (long long)GR * 2 * 4;
    return SS_OK;
}

extern "C" int ss_disp_error_image_fwd(const float* est, const float* gt, const float* table, int B, int H, int W, float abs_thres,
                                       float rel_thres, int legend, int is_signed, float lo, float hi, float* out, ss_stream_t stream) {
    SS_REQUIRE(est && gt && table && out && B > 0 && H > 0 && W > 0);
    const long long quads = row_quads(B, H, W);
    if (quads < 0) return SS_ERR_UNSUPPORTED;
    ErrArgs a{est, gt, out, B, H, W, abs_thres, rel_thres, legend ? 1 : 0, is_signed ? 1 : 0, lo, hi, {}, {}, {}};
    for (int i = 0; i < NBINS; ++i) {          // (host memory: the table travels in the kernel's arguments)
        a.bin_lo[i] = table[5 * i];
        a.bin_hi[i] = table[5 * i + 1];
        for (int k = 0; k < 3; ++k) a.col[i][k] = table[5 * i + 2 + k];
    }
    hipLaunchKernelGGL(error_image_k, dim3(grid_for(quads, GV)), dim3(BLOCK), 0, ss::as_stream(stream), a);
    return ss::check_launch();
}

extern "C" int ss_class_color_fwd(const void* src, int src_dtype, int B, int num_classes, int H, int W, long long label_row_stride,
                                  long long label_image_stride, void* out, int out_dtype, ss_stream_t stream) {
    SS_REQUIRE(src && out && B > 0 && H > 0 && W > 0);
    SS_REQUIRE(src_dtype >= SRC_LOGITS && src_dtype <= LT_F32 && (out_dtype == 0 || out_dtype == 1));
    if (src_dtype == SRC_LOGITS) {
        SS_REQUIRE(num_classes > 0);
        if (num_classes > NC) return SS_ERR_UNSUPPORTED;
    } else {
        SS_REQUIRE(label_row_stride >= W && label_image_stride >= (long long)(H - 1) * label_row_stride + W);
    }
    const long long quads = row_quads(B, H, W);
    if (quads < 0) return SS_ERR_UNSUPPORTED;
    ColorArgs a{src, out, label_row_stride, label_image_stride, B, num_classes, H, W};
    const int G = grid_for(quads, GV);
    hipStream_t st = ss::as_stream(stream);
    switch (src_dtype) {
    case SRC_LOGITS:
        return color_launch<SRC_LOGITS>(a, out_dtype, G, st);
    case LT_I64:
        return color_launch<LT_I64>(a, out_dtype, G, st);
    case LT_U8:
        return color_launch<LT_U8>(a, out_dtype, G, st);
    default:
        return color_launch<LT_F32>(a, out_dtype, G, st);
    }
}

extern "C" int ss_image_minmax_fwd(const float* x, int B, long long elements_per_image, float* minmax, void* workspace,
                                   long long workspace_bytes, ss_stream_t stream) {
    SS_REQUIRE(x && minmax && workspace && B > 0 && elements_per_image > 0 && workspace_bytes >= (long long)GR * 2 * 4);
    if (B > GR) return SS_ERR_UNSUPPORTED;
    const int G = grid_for(ss::ceil_div_ll(elements_per_image, 4), GR / B);
    hipStream_t st = ss::as_stream(stream);
    float* ws = static_cast<float*>(workspace);
    hipLaunchKernelGGL(image_minmax_k, dim3(G, B), dim3(BLOCK), 0, st, x, elements_per_image, ws);
    if (int s = ss::check_launch()) return s;
    hipLaunchKernelGGL(image_minmax_finish_k, dim3(B), dim3(BLOCK), 0, st, ws, G, minmax);
    return ss::check_launch();
}

extern "C" int ss_image_normalize_fwd(const float* x, const float* minmax, float* out, int B, int C, long long pixels_per_channel,
                                      ss_stream_t stream) {
    SS_REQUIRE(x && minmax && out && B > 0 && C > 0 && pixels_per_channel > 0);
    if (B > 65535) return SS_ERR_UNSUPPORTED;
    const int G = grid_for(ss::ceil_div_ll((long long)C * pixels_per_channel, 4), GV);
    hipLaunchKernelGGL(image_normalize_k, dim3(G, B), dim3(BLOCK), 0, ss::as_stream(stream), x, minmax, out, C, pixels_per_channel);
    return ss::check_launch();
}
