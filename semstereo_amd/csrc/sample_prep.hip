// Sample preparation (datasets/us3d_.py:70-215, datasets/whu_dataset.py:42-92, datasets/data_io.py:6-13 of the reference): what
// __getitem__ computes on the host for every item, from the raw arrays on the device.
//   views      ToTensor + Normalize of both views: uint8 [B,H,W,3] -> float32 [B,3,H,W] through a 3 x 256 table that the caller built with
//              the reference's own fp32 operations -- no division runs here
//   pyramid    cv2.resize(..., INTER_NEAREST) to (w // k, h // k) for H and W divisible by 16, where the source pixel is (y k, x k):
//              disparity_4/8/16, label_2/4 and the float32 label (and disparity, for an integer source) in one launch
//   luma       PIL's convert("L"), (19595 R + 38470 G + 7471 B + 0x8000) >> 16, with the per-image integer sums S1 and S2
//   gradients  z = (L - mean) / std in double from the exact sums, gx = z(y, x-1) - z(y, x+1), gy = z(y-1, x) - z(y+1, x), zero outside
// All of them are streaming passes of the stream.h family, a lane taking a row quad (4 consecutive pixels of one row).  Element offsets
// are 64-bit.  The luma pass leaves one pair of 64-bit integer partial sums per workgroup, which the gradient pass adds; integer sums
// are exact in any order.  Nothing here allocates, copies or synchronises, and nothing comes back to the host.
#include "common.h"
#include "metrics_decode.h"
#include "stream.h"

namespace {

using namespace ss::stream;    // BLOCK, grid_for, aligned_to, block_sum, RowQuad, row_quad, load_rgb4, rgb_byte, store4
using ss::metrics::LT_I64;     // label sources: the codes of every label_dtype
using ss::metrics::LT_U8;
using ss::metrics::LT_F32;

constexpr int GV = 2048;                 // workgroups of a pass, all images together
constexpr long long MAX_STAT_PIXELS = 1ll << 23;      // N S2 - S1^2 is formed in 64 unsigned bits: N <= 2^23 keeps N S2 below 2^62
constexpr long long SUMS_ALIGN = 256;    // the luma plane starts at a multiple of this behind the partial sums
constexpr int MAX_STAT_GROUPS = 1024;    // workgroups (and partial sums) per image of the luma pass

typedef unsigned long long u64;
typedef unsigned char u8;

// ---------------------------------------------------------------- views (datasets/data_io.py:6-13)
struct ViewArgs {
    const u8* src[2];          // [B,H,W,3]
    float* out[2];             // [B,3,H,W]
    const float* table;        // [3][256], device memory
    int B, H, W;
};

// grid (G, views)
__global__ __launch_bounds__(BLOCK) void views_k(ViewArgs a) {
    __shared__ float tab[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += BLOCK) tab[i] = a.table[i];
    __syncthreads();
    const u8* src = blockIdx.y ? a.src[1] : a.src[0];
    float* out = blockIdx.y ? a.out[1] : a.out[0];
    const unsigned QW = ((unsigned)a.W + 3u) / 4u, total = (unsigned)a.B * (unsigned)a.H * QW;
    const unsigned stride = gridDim.x * BLOCK;
    const long long HW = (long long)a.H * a.W;
    for (unsigned q = blockIdx.x * BLOCK + threadIdx.x; q < total; q += stride) {
        const RowQuad r = row_quad(q, QW, (unsigned)a.H, a.W);
        const long long px = ((long long)r.b * a.H + r.h) * a.W + r.x0;
        unsigned w[3];
        load_rgb4(src + px * 3, r.nv, w);
        float c[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch][j] = tab[ch * 256 + rgb_byte(w, 3 * j + ch)];
        float* o = out + ((long long)r.b * 3 * a.H + r.h) * a.W + r.x0;
        store4(o, r.nv, c[0]);
        store4(o + HW, r.nv, c[1]);
        store4(o + 2 * HW, r.nv, c[2]);
    }
}

// ---------------------------------------------------------------- pyramids (cv2.resize INTER_NEAREST, H and W divisible by k)
enum { DT_F32 = 0, DT_I32 = 1 };                 // disparity sources
constexpr int NJOBS = 7;                         // disparity, disparity_4/8/16, label, label_2/4

struct PyrArgs {
    const void* disp;          // [B,H,W] contiguous
    const void* label;         // pixel (b, h, x) at b * y_img + h * y_row + x
    float* out[NJOBS];
    long long y_row, y_img;
    float scale;
    int disp_dtype, label_dtype;
    int B, H, W;
};

// element i * k of p for i < nv, widened to float: one wide load for k == 1 where the address allows
__device__ __forceinline__ void gather4(const float* p, int k, int nv, float (&v)[4]) {
    if (k == 1 && nv == 4 && aligned_to(p, 16)) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[(long long)j * k] : 0.f;
    }
}
__device__ __forceinline__ void gather4(const int* p, int k, int nv, float (&v)[4]) {
    if (k == 1 && nv == 4 && aligned_to(p, 16)) {
        const int4 q = *reinterpret_cast<const int4*>(p);
        v[0] = (float)q.x, v[1] = (float)q.y, v[2] = (float)q.z, v[3] = (float)q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < nv ? (float)p[(long long)j * k] : 0.f;
    }
}
__device__ __forceinline__ void gather4(const u8* p, int k, int nv, float (&v)[4]) {
    if (k == 1 && nv == 4 && aligned_to(p, 4)) {
        const uchar4 q = *reinterpret_cast<const uchar4*>(p);
        v[0] = (float)q.x, v[1] = (float)q.y, v[2] = (float)q.z, v[3] = (float)q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < nv ? (float)p[(long long)j * k] : 0.f;
    }
}
__device__ __forceinline__ void gather4(const long long* p, int k, int nv, float (&v)[4]) {
    if (k == 1 && nv == 4 && aligned_to(p, 16)) {
        const longlong2 a = reinterpret_cast<const longlong2*>(p)[0], b = reinterpret_cast<const longlong2*>(p)[1];
        v[0] = (float)a.x, v[1] = (float)a.y, v[2] = (float)b.x, v[3] = (float)b.y;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < nv ? (float)p[(long long)j * k] : 0.f;
    }
}

// grid (G, NJOBS): job blockIdx.y writes one output; a null output has no work
__global__ __launch_bounds__(BLOCK) void pyramid_k(PyrArgs a) {
    const int job = blockIdx.y;
    float* out = nullptr;
#pragma unroll
    for (int i = 0; i < NJOBS; ++i) out = job == i ? a.out[i] : out;
    if (!out) return;
    const bool is_label = job >= 4;
    const int k = job == 0 || job == 4 ? 1 : job == 1 || job == 6 ? 4 : job == 2 ? 8 : job == 3 ? 16 : 2;
    const int Ho = a.H / k, Wo = a.W / k;
    const unsigned QW = ((unsigned)Wo + 3u) / 4u, total = (unsigned)a.B * (unsigned)Ho * QW;
    const unsigned stride = gridDim.x * BLOCK;
    const long long row = is_label ? a.y_row : (long long)a.W, img = is_label ? a.y_img : (long long)a.H * a.W;
    for (unsigned q = blockIdx.x * BLOCK + threadIdx.x; q < total; q += stride) {
        const RowQuad r = row_quad(q, QW, (unsigned)Ho, Wo);
        const long long off = (long long)r.b * img + (long long)r.h * k * row + (long long)r.x0 * k;
        float v[4];
        if (is_label) {
            if (a.label_dtype == LT_I64)
                gather4(reinterpret_cast<const long long*>(a.label) + off, k, r.nv, v);
            else if (a.label_dtype == LT_U8)
                gather4(reinterpret_cast<const u8*>(a.label) + off, k, r.nv, v);
            else
                gather4(reinterpret_cast<const float*>(a.label) + off, k, r.nv, v);
        } else {
            if (a.disp_dtype == DT_I32)
                gather4(reinterpret_cast<const int*>(a.disp) + off, k, r.nv, v);
            else
                gather4(reinterpret_cast<const float*>(a.disp) + off, k, r.nv, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ss::mul_rn(v[j], a.scale);
        }
        store4(out + ((long long)r.b * Ho + r.h) * Wo + r.x0, r.nv, v);
    }
}

// ---------------------------------------------------------------- luma and the per-image sums
__device__ __forceinline__ unsigned luma_of(unsigned r, unsigned g, unsigned b) { return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16; }

// grid (G, B): image blockIdx.y of n pixels, 4 consecutive ones per lane and trip; the workgroup's partial S1, S2 go to
// sums[(b * G + g) * 2 + {0, 1}]
__global__ __launch_bounds__(BLOCK) void luma_stats_k(const u8* src, long long n, u8* luma, u64* sums) {
    __shared__ u64 lds[4 * 2];
    const u8* p = src + (long long)blockIdx.y * n * 3;
    u8* o = luma + (long long)blockIdx.y * n;
    const long long nq = (n + 3) / 4, stride = (long long)gridDim.x * BLOCK;
    u64 s[2] = {0ull, 0ull};           // S1, S2
    for (long long q = (long long)blockIdx.x * BLOCK + threadIdx.x; q < nq; q += stride) {
        const long long left = n - 4 * q;
        const int nv = left < 4 ? (int)left : 4;
        unsigned w[3];
        load_rgb4(p + 12 * q, nv, w);
        unsigned L[4], packed = 0u, t1 = 0u, t2 = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            L[j] = j < nv ? luma_of(rgb_byte(w, 3 * j), rgb_byte(w, 3 * j + 1), rgb_byte(w, 3 * j + 2)) : 0u;
            packed |= L[j] << (8 * j);
            t1 += L[j];
            t2 += L[j] * L[j];
        }
        s[0] += t1;
        s[1] += t2;
        u8* d = o + 4 * q;
        if (nv == 4 && aligned_to(d, 4)) {
            *reinterpret_cast<unsigned*>(d) = packed;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nv) d[j] = (u8)L[j];
        }
    }
    block_sum<2>(s, lds);
    if (threadIdx.x == 0) {
        u64* w = sums + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        w[0] = s[0], w[1] = s[1];
    }
}

// ---------------------------------------------------------------- gx / gy
// luma bytes x0 - 1 .. x0 + 4 of a row as indices into the z table, or -1 outside the image (row == nullptr: the whole row is outside)
__device__ __forceinline__ void row_window(const u8* row, int x0, int nv, int W, int (&c)[6]) {
#pragma unroll
    for (int j = 0; j < 6; ++j) c[j] = -1;
    if (!row) return;
    if (nv == 4 && aligned_to(row + x0, 4)) {
        const unsigned w = *reinterpret_cast<const unsigned*>(row + x0);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j + 1] = (int)((w >> (8 * j)) & 255u);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) c[j + 1] = (int)row[x0 + j];
    }
    if (x0 > 0) c[0] = (int)row[x0 - 1];
    if (x0 + 4 < W) c[5] = (int)row[x0 + 4];
}

// grid (G, B).  The GS partial sums of image b are added (integers: any order), then the z table is built by the 256 lanes:
// mean = S1 / N, std = sqrt(N S2 - S1^2) / N,
// z[L] = (L - mean) / std, all in double with IEEE division and square root.  std = 0 (a constant image) gives NaN at the image's own
// luma value; the centre tap of the reference's convolution, 0 z(y, x), is kept so that such a pixel is NaN whatever its neighbours are.
__global__ __launch_bounds__(BLOCK) void gradients_k(const u8* luma, const u64* sums, int GS, float* gx, float* gy, int H, int W) {
    __shared__ double z[256];
    __shared__ u64 lds[4 * 2];
    const u64 N = (u64)H * (u64)W;
    u64 s[2] = {0ull, 0ull};
    for (int g = threadIdx.x; g < GS; g += BLOCK) {
        const u64* w = sums + ((long long)blockIdx.y * GS + g) * 2;
        s[0] += w[0], s[1] += w[1];
    }
    block_sum<2>(s, lds);              // (the totals in every thread)
    {
        const u64 S1 = s[0], S2 = s[1];
        const double n = (double)N, mean = (double)S1 / n, sd = sqrt((double)(N * S2 - S1 * S1)) / n;
        z[threadIdx.x] = ((double)(int)threadIdx.x - mean) / sd;
    }
    __syncthreads();
    const u8* img = luma + (long long)blockIdx.y * (long long)N;
    float* ox = gx + (long long)blockIdx.y * (long long)N;
    float* oy = gy + (long long)blockIdx.y * (long long)N;
    const unsigned QW = ((unsigned)W + 3u) / 4u, total = (unsigned)H * QW, stride = gridDim.x * BLOCK;
    for (unsigned q = blockIdx.x * BLOCK + threadIdx.x; q < total; q += stride) {
        const unsigned h = q / QW;
        const int x0 = (int)((q - h * QW) * 4u), left = W - x0, nv = left < 4 ? left : 4;
        const u8* row = img + (long long)h * W;
        int c[6], u[6], d[6];
        row_window(row, x0, nv, W, c);
        row_window(h > 0 ? row - W : nullptr, x0, nv, W, u);
        row_window(h + 1 < (unsigned)H ? row + W : nullptr, x0, nv, W, d);
        double zc[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) zc[j] = c[j] >= 0 ? z[c[j]] : 0.0;
        float vx[4], vy[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double zu = u[j + 1] >= 0 ? z[u[j + 1]] : 0.0, zd = d[j + 1] >= 0 ? z[d[j + 1]] : 0.0;
            const double centre = 0.0 * zc[j + 1];
            vx[j] = (float)((zc[j] - zc[j + 2]) + centre);
            vy[j] = (float)((zu - zd) + centre);
        }
        store4(ox + (long long)h * W + x0, nv, vx);
        store4(oy + (long long)h * W + x0, nv, vy);
    }
}

// 4-pixel groups of a [B,H,W] map, or -1 where the map has 2^31 elements or more
long long row_quads(long long B, long long H, long long W) {
    if (B * H * W >= (1ll << 31)) return -1;
    return B * H * ((W + 3) / 4);
}

// workgroups per image of the luma pass: both statistics entry points and the workspace size derive it from the shape alone
int stat_groups(int B, int H, int W) {
    const int share = GV / B < 1 ? 1 : GV / B;
    return grid_for(((long long)H * W + 3) / 4, share < MAX_STAT_GROUPS ? share : MAX_STAT_GROUPS);
}

long long sums_bytes(int B, int H, int W) {
    return ((long long)B * stat_groups(B, H, W) * 2 * 8 + SUMS_ALIGN - 1) / SUMS_ALIGN * SUMS_ALIGN;
}

// B > 0, H > 0, W > 0 checked by the caller: 0 where the statistics kernels take the shape
int stats_shape(int B, int H, int W) {
    if ((long long)H * W > MAX_STAT_PIXELS || B > 65535 || row_quads(B, H, W) < 0) return SS_ERR_UNSUPPORTED;
    return SS_OK;
}

}  // namespace

extern "C" int ss_prep_workspace_bytes(int B, int H, int W, long long* bytes) {
    SS_REQUIRE(bytes && B > 0 && H > 0 && W > 0);
    if (int s = stats_shape(B, H, W)) return s;
    *bytes = sums_bytes(B, H, W) + ((long long)B * H * W + 15) / 16 * 16;
    return SS_OK;
}

extern "C" int ss_prep_views_fwd(const unsigned char* left, const unsigned char* right, const float* table, int B, int H, int W,
                                 float* out_left, float* out_right, ss_stream_t stream) {
    SS_REQUIRE(left && out_left && table && B > 0 && H > 0 && W > 0);
    SS_REQUIRE((right == nullptr) == (out_right == nullptr));
    if (3ll * B * H * W >= (1ll << 31)) return SS_ERR_UNSUPPORTED;
    const long long quads = row_quads(B, H, W);
    ViewArgs a{{left, right}, {out_left, out_right}, table, B, H, W};
    hipLaunchKernelGGL(views_k, dim3(grid_for(quads, right ? GV / 2 : GV), right ? 2 : 1), dim3(BLOCK), 0, ss::as_stream(stream), a);
    return ss::check_launch();
}

extern "C" int ss_prep_pyramid_fwd(const void* disparity, int disp_dtype, float disp_scale, const void* label, int label_dtype,
                                   long long label_row_stride, long long label_image_stride, int B, int H, int W, float* disparity_out,
                                   float* disparity_4, float* disparity_8, float* disparity_16, float* label_out, float* label_2,
                                   float* label_4, ss_stream_t stream) {
    SS_REQUIRE(B > 0 && H > 0 && W > 0);
    const bool any_disp = disparity_out || disparity_4 || disparity_8 || disparity_16, any_label = label_out || label_2 || label_4;
    SS_REQUIRE(any_disp || any_label);
    if (any_disp) SS_REQUIRE(disparity && (disp_dtype == DT_F32 || disp_dtype == DT_I32));
    if (any_label) {
        SS_REQUIRE(label && label_dtype >= LT_I64 && label_dtype <= LT_F32);
        SS_REQUIRE(label_row_stride >= W && label_image_stride >= (long long)(H - 1) * label_row_stride + W);
    }
    if (H % 16 != 0 || W % 16 != 0) return SS_ERR_UNSUPPORTED;
    const long long quads = row_quads(B, H, W);
    if (quads < 0) return SS_ERR_UNSUPPORTED;
    PyrArgs a{disparity, label, {disparity_out, disparity_4, disparity_8, disparity_16, label_out, label_2, label_4}, label_row_stride,
              label_image_stride, disp_scale, disp_dtype, label_dtype, B, H, W};
    const bool full = disparity_out || label_out;
    const long long most = full ? quads : (label_2 ? quads / 4 : quads / 16);
    hipLaunchKernelGGL(pyramid_k, dim3(grid_for(most, GV / 4), NJOBS), dim3(BLOCK), 0, ss::as_stream(stream), a);
    return ss::check_launch();
}

extern "C" int ss_prep_luma_stats_fwd(const unsigned char* left, int B, int H, int W, void* workspace, long long workspace_bytes,
                                      ss_stream_t stream) {
    SS_REQUIRE(left && workspace && B > 0 && H > 0 && W > 0);
    if (3ll * B * H * W >= (1ll << 31)) return SS_ERR_UNSUPPORTED;
    if (int s = stats_shape(B, H, W)) return s;
    SS_REQUIRE(workspace_bytes >= sums_bytes(B, H, W) + (long long)B * H * W);
    SS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0);
    hipStream_t st = ss::as_stream(stream);
    u64* sums = static_cast<u64*>(workspace);
    u8* luma = static_cast<u8*>(workspace) + sums_bytes(B, H, W);
    hipLaunchKernelGGL(luma_stats_k, dim3(stat_groups(B, H, W), B), dim3(BLOCK), 0, st, left, (long long)H * W, luma, sums);
    return ss::check_launch();
}

extern "C" int ss_prep_gradients_fwd(const void* workspace, long long workspace_bytes, int B, int H, int W, float* gx, float* gy,
                                     ss_stream_t stream) {
    SS_REQUIRE(workspace && gx && gy && B > 0 && H > 0 && W > 0);
    if (int s = stats_shape(B, H, W)) return s;
    SS_REQUIRE(workspace_bytes >= sums_bytes(B, H, W) + (long long)B * H * W);
    SS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0);
    const u64* sums = static_cast<const u64*>(workspace);
    const u8* luma = static_cast<const u8*>(workspace) + sums_bytes(B, H, W);
    const int cap = GV / B < 1 ? 1 : GV / B;
    hipLaunchKernelGGL(gradients_k, dim3(grid_for((long long)H * ((W + 3) / 4), cap), B), dim3(BLOCK), 0, ss::as_stream(stream), luma, sums,
                       stat_groups(B, H, W), gx, gy, H, W);
    return ss::check_launch();
}
