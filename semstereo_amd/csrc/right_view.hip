// Right-view ground truth and the left-right consistency check: the forward warp that the reference left as a commented-out per-pixel
// Python loop (datasets/us3d_.py:115-133, the "label_r" entry at :193) and that LRSC_loss (models/loss.py:121-135) stands in for.
// Row-wise, per image b and row y; d is the left-view disparity, a left pixel x matches right column x - d (SpatialTransformer_grid).
//   valid      lo <= d < hi (NaN is not)
//   target     t = rintf(float(x) - d) in fp32, half to even; x LANDS if it is valid and 0 <= t < W (-0.5 rounds to -0: column 0)
//   owner[r]   the LARGEST x that lands on r, -1 if none: the last writer of a raster-order loop, and -- the pixel further right having
//              the larger disparity, up to the rounding step -- the surface nearer the sensor
//   right_disparity[r] = d[owner], right_label[r] = float(label[owner]), the fill values where owner is -1
//   left_visible[x]    = lands(x) and owner[t(x)] == x
//   consistency of two estimates dL, dR (dR[r] the disparity of right pixel r, the form right_disparity has):
//   diff[x] = |dL[x] - dR[t(x)]| in fp32 where x lands and dR[t] is valid, +inf elsewhere; consistent[x] = diff[x] <= threshold
// Nothing is interpolated: every output is a selection, one subtraction or one comparison, so the PyTorch composition of
// semstereo_amd/data.py gives the same bits.  The owners of a row are an LDS INTEGER maximum (order-independent: two calls give the same
// bits); there are no floating-point atomics.  Kernels of the stream.h family: BLOCK threads, a lane takes 4 consecutive pixels of a
// row, 64-bit element offsets.  Nothing here allocates, copies or synchronises, and nothing comes back to the host.
#include "common.h"
#include "metrics_decode.h"
#include "right_view.h"
#include "stream.h"

namespace {

using namespace ss::stream;    // BLOCK, grid_for, RowQuad, row_quad, load4, store4
using ss::metrics::LT_I64;     // label sources: the codes of every label_dtype
using ss::metrics::LT_U8;
using ss::metrics::LT_F32;
using ss::rview::MAX_W;        // owners of a row: 32 KB of LDS
using ss::rview::lr_diff;      // shared with disparity_refine.hip: right_view.h
using ss::rview::map_shape;
using ss::rview::target;

constexpr int GV = 2048;                 // workgroups of a pass

typedef unsigned char u8;

struct ViewArgs {
    const float* disp;         // [B,H,W] contiguous
    const void* label;         // pixel (b, h, x) at b * y_img + h * y_row + x
    float* right_disp;         // [B,H,W], or null
    float* right_label;
    u8* visible;
    long long y_row, y_img;
    float lo, hi, fill_disp, fill_label;
    int label_dtype;
    int B, H, W;
};

__device__ __forceinline__ float label_at(const void* y, int dtype, long long i) {
    if (dtype == LT_I64) return (float)reinterpret_cast<const long long*>(y)[i];
    if (dtype == LT_U8) return (float)reinterpret_cast<const u8*>(y)[i];
    return reinterpret_cast<const float*>(y)[i];
}

// one workgroup per row, grid-stride over the B * H rows; dynamic LDS: W ints
__global__ __launch_bounds__(BLOCK) void right_view_k(ViewArgs a) {
    extern __shared__ __attribute__((aligned(16))) int owner[];
    const int W = a.W;
    const unsigned rows = (unsigned)a.B * (unsigned)a.H;
    for (unsigned row = blockIdx.x; row < rows; row += gridDim.x) {
        const unsigned b = row / (unsigned)a.H, h = row - b * (unsigned)a.H;
        const long long base = (long long)row * W;
        const float* d = a.disp + base;
        for (int i = threadIdx.x; i < W; i += BLOCK) owner[i] = -1;
        __syncthreads();
        for (int x0 = threadIdx.x * 4; x0 < W; x0 += BLOCK * 4) {
            const int left = W - x0, nv = left < 4 ? left : 4;
            float v[4];
            load4(d + x0, nv, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int t = j < nv ? target(x0 + j, v[j], a.lo, a.hi, W) : -1;
                if (t >= 0) atomicMax(&owner[t], x0 + j);
            }
        }
        __syncthreads();
        const long long ybase = (long long)b * a.y_img + (long long)h * a.y_row;
        for (int x0 = threadIdx.x * 4; x0 < W; x0 += BLOCK * 4) {
            const int left = W - x0, nv = left < 4 ? left : 4;
            if (a.right_disp || a.right_label) {
                int o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = j < nv ? owner[x0 + j] : -1;
                if (a.right_disp) {
                    float v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = o[j] >= 0 ? d[o[j]] : a.fill_disp;
                    store4(a.right_disp + base + x0, nv, v);
                }
                if (a.right_label) {
                    float v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = o[j] >= 0 ? label_at(a.label, a.label_dtype, ybase + o[j]) : a.fill_label;
                    store4(a.right_label + base + x0, nv, v);
                }
            }
            if (a.visible) {
                float v[4], vis[4];
                load4(d + x0, nv, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int t = j < nv ? target(x0 + j, v[j], a.lo, a.hi, W) : -1;
                    vis[j] = (t >= 0 && owner[t] == x0 + j) ? 1.f : 0.f;
                }
                store4(a.visible + base + x0, nv, vis);
            }
        }
        __syncthreads();               // (the next row's fill)
    }
}

// a plain row-quad pass: 4 pixels per lane, a scalar gather from the right map's row
__global__ __launch_bounds__(BLOCK) void lr_consistency_k(const float* dl, const float* dr, int B, int H, int W, float lo, float hi,
                                                          float threshold, u8* consistent, float* diff) {
    const unsigned QW = ((unsigned)W + 3u) / 4u, total = (unsigned)B * (unsigned)H * QW;
    const unsigned stride = gridDim.x * BLOCK;
    for (unsigned q = blockIdx.x * BLOCK + threadIdx.x; q < total; q += stride) {
        const RowQuad r = row_quad(q, QW, (unsigned)H, W);
        const long long row = ((long long)r.b * H + r.h) * W;
        float v[4], e[4], c[4];
        load4(dl + row + r.x0, r.nv, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            e[j] = j < r.nv ? lr_diff(r.x0 + j, v[j], dr + row, lo, hi, W) : INFINITY;
            c[j] = e[j] <= threshold ? 1.f : 0.f;
        }
        if (diff) store4(diff + row + r.x0, r.nv, e);
        if (consistent) store4(consistent + row + r.x0, r.nv, c);
    }
}

}  // namespace

extern "C" int ss_right_view_fwd(const float* disparity, const void* label, int label_dtype, long long label_row_stride,
                                 long long label_image_stride, int B, int H, int W, float lo, float hi, float fill_disparity,
                                 float fill_label, float* right_disparity, float* right_label, unsigned char* left_visible,
                                 ss_stream_t stream) {
    SS_REQUIRE(disparity && B > 0 && H > 0 && W > 0);
    SS_REQUIRE(right_disparity || right_label || left_visible);
    SS_REQUIRE((label == nullptr) == (right_label == nullptr));
    if (label) {
        SS_REQUIRE(label_dtype >= LT_I64 && label_dtype <= LT_F32);
        SS_REQUIRE(label_row_stride >= W && label_image_stride >= (long long)(H - 1) * label_row_stride + W);
    }
    SS_REQUIRE(lo < hi);               // (false for a NaN)
    if (W > MAX_W) return SS_ERR_UNSUPPORTED;
    if (int s = map_shape(B, H, W)) return s;
    ViewArgs a{disparity, label, right_disparity, right_label, left_visible, label_row_stride, label_image_stride, lo, hi, fill_disparity,
               fill_label, label_dtype, B, H, W};
    const long long rows = (long long)B * H;
    hipLaunchKernelGGL(right_view_k, dim3((unsigned)(rows < GV ? rows : GV)), dim3(BLOCK), (size_t)W * sizeof(int), ss::as_stream(stream), a);
    return ss::check_launch();
}

extern "C" int ss_lr_consistency_fwd(const float* disp_left, const float* disp_right, int B, int H, int W, float lo, float hi,
                                     float threshold, unsigned char* consistent, float* diff, ss_stream_t stream) {
    SS_REQUIRE(disp_left && disp_right && B > 0 && H > 0 && W > 0);
    SS_REQUIRE(consistent || diff);
    SS_REQUIRE(lo < hi);               // (false for a NaN)
    SS_REQUIRE(threshold >= 0.f);      // (false for a NaN)
    if (int s = map_shape(B, H, W)) return s;
    const long long quads = (long long)B * H * ((W + 3) / 4);
    hipLaunchKernelGGL(lr_consistency_k, dim3(grid_for(quads, GV)), dim3(BLOCK), 0, ss::as_stream(stream), disp_left, disp_right, B, H, W,
                       lo, hi, threshold, consistent, diff);
    return ss::check_launch();
}
