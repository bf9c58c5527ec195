// Training augmentation (datasets/kitti_dataset_15_aug.py:100-156 of the reference, plus the two flips a rectified satellite pair allows):
// per-view brightness, gamma, contrast and saturation as PIL rounds them, a crop shared by both views and the maps, a vertical flip,
// a horizontal flip with the views swapped, and the occluder rectangle of the right view -- from the raw arrays on the device.
//   T1      brightness then gamma, a 256-entry uint8 table per (item, OUTPUT view) that the host builds from the parameters
//   stats   S = the exact integer sum of luma(T1[r], T1[g], T1[b]) over the WHOLE source image; m = int(S / N + 0.5) in double
//   T13     T13[u] = blend(m, T1[u], contrast): brightness, gamma and contrast of a channel value as ONE table, built in LDS
//   pixel   u3 = T13[u] per channel, L3 = luma(u3), u4 = blend(L3, u3, saturation): the only per-pixel fp32 arithmetic
//   blend   trunc(clamp(float(deg) + f * float(x - deg), 0, 255)), the product rounded before the sum (Image.blend)
//   source  row y0 + (vflip ? th - 1 - y : y); column x0 + x, or with the swap W - 1 - (x0 + x) of the OTHER view
//   occluder  crop pixels of the output right view inside [r0, r1) x [c0, c1) take floor(Sc / (th tw)) per channel, Sc the exact sum of u4
//   maps    the selected pixels of the disparity / label (swapped items: of right_view's maps of the full item), and their levels
// Three streaming passes of the stream.h family: the luma sums (one 64-bit partial per workgroup), the occluder's channel sums
// (partials again; launched only when an item has an occluder) and the write.  Partials are added by every workgroup that needs the
// total: integer sums, exact in any order, so two calls give the same bits and no finish launch is needed.  The parameter block is
// device memory that no entry point can check: origins are clamped into the image and rectangles into the crop here, so a wrong block
// gives wrong pixels, never an address outside the tensors.  Element offsets are 64-bit.  Nothing here allocates, copies or waits.
#include "common.h"
#include "metrics_decode.h"
#include "stream.h"

namespace {

using namespace ss::stream;    // BLOCK, grid_for, aligned_to, block_sum, load_rgb4, rgb_byte, store4
using ss::metrics::LT_I64;     // label sources: the codes of every label_dtype
using ss::metrics::LT_U8;
using ss::metrics::LT_F32;

constexpr int GV = 2048;                 // workgroups of a pass, all images together
constexpr int MAX_STAT_GROUPS = 1024;    // partial sums per (item, view) of the luma pass
constexpr int MAX_OCC_GROUPS = 256;      // partial sums per item of the occluder pass
constexpr int MAX_ITEMS = 65535;         // an item per grid.z
constexpr long long PART_ALIGN = 256;    // the occluder partials start at a multiple of this behind the luma partials
constexpr int NMAPS = 7;                 // disparity, disparity_4/8/16, label, label_2/4
constexpr float FILL_DISPARITY = -999.f, FILL_LABEL = 5.f;      // right_view's defaults: what a swapped item without its maps gets

typedef unsigned long long u64;
typedef unsigned char u8;

enum { F_VFLIP = 1, F_SWAP = 2, F_OCCLUDER = 4 };
enum { DT_F32 = 0, DT_I32 = 1 };         // disparity sources

// include/semstereo_hip.h, "training augmentation": the record of one item
struct Item {
    int y0, x0, flags;
    int cy, sy, cx, sx;        // the occluder in crop coordinates, rows first
    int reserved;
    float contrast[2], saturation[2];    // per OUTPUT view
    u8 t1[2][256];
};
static_assert(sizeof(Item) == 560, "the parameter record is 560 bytes");

struct Geometry {
    int y0, x0, flags;
    int r0, r1, c0, c1;        // the occluder clipped to the crop
};

__device__ __forceinline__ int clampi(long long v, int lo, int hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }

__device__ __forceinline__ Geometry geometry(const Item* it, int H, int W, int th, int tw) {
    Geometry g;
    g.y0 = clampi(it->y0, 0, H - th);
    g.x0 = clampi(it->x0, 0, W - tw);
    g.flags = it->flags;
    const long long cy = it->cy, sy = it->sy, cx = it->cx, sx = it->sx;
    g.r0 = clampi(cy - sy, 0, th), g.r1 = clampi(cy + sy, 0, th);
    g.c0 = clampi(cx - sx, 0, tw), g.c1 = clampi(cx + sx, 0, tw);
    return g;
}

__device__ __forceinline__ unsigned luma_of(unsigned r, unsigned g, unsigned b) { return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16; }

// Image.blend as ImageEnhance calls it; a NaN factor (a wrong block) gives 0
__device__ __forceinline__ unsigned blend(unsigned deg, unsigned x, float f) {
    const float t = ss::add_rn((float)deg, ss::mul_rn(f, (float)((int)x - (int)deg)));
    return (unsigned)fminf(fmaxf(t, 0.f), 255.f);
}

// nv pixels of a source row in OUTPUT order: output pixel j is source column s0 + j, or s0 - j when `rev`.  Forward and full reversed
// quads are one load_rgb4 (three dwords where the 12 bytes are dword-aligned, bytes otherwise: an odd x0); a ragged reversed one is bytes.
__device__ __forceinline__ void src_quad(const u8* row, int s0, bool rev, int nv, unsigned (&c)[4][3]) {
    unsigned w[3];
    if (!rev) {
        load_rgb4(row + 3ll * s0, nv, w);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[j][ch] = rgb_byte(w, 3 * j + ch);
    } else if (nv == 4) {
        load_rgb4(row + 3ll * (s0 - 3), 4, w);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[j][ch] = rgb_byte(w, 3 * (3 - j) + ch);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[j][ch] = j < nv ? (unsigned)row[3ll * (s0 - j) + ch] : 0u;
    }
}

// contrast and saturation of one pixel
__device__ __forceinline__ void shade(const unsigned (&c)[3], const u8* t13, float s, unsigned (&o)[3]) {
    const unsigned r = t13[c[0]], g = t13[c[1]], b = t13[c[2]];
    const unsigned L = luma_of(r, g, b);
    o[0] = blend(L, r, s), o[1] = blend(L, g, s), o[2] = blend(L, b, s);
}

// t13 of (item, output view v): the GS partials are added (integers: any order), m = int(S / N + 0.5) in double, and the 256 lanes
// build one entry each.  lds: 4 u64.  Ends with a barrier.
__device__ __forceinline__ void build_table(const Item* it, int v, const u64* sums, int GS, long long bv, double n, u8* t13, u64* lds) {
    u64 s[1] = {0ull};
    for (int g = threadIdx.x; g < GS; g += BLOCK) s[0] += sums[bv * GS + g];
    block_sum<1>(s, lds);              // (the total in every thread)
    const double mean = (double)s[0] / n + 0.5;
    const unsigned m = (unsigned)clampi((long long)mean, 0, 255);
    t13[threadIdx.x] = (u8)blend(m, it->t1[v][threadIdx.x], it->contrast[v]);
    __syncthreads();
}

// ---------------------------------------------------------------- pass 1: the luma sums
// grid (GS, 2, B): output view v = blockIdx.y of item blockIdx.z, over the n pixels of its SOURCE image (a mean is unchanged by a flip);
// the workgroup's partial goes to sums[(b * 2 + v) * GS + g]
__global__ __launch_bounds__(BLOCK) void stats_k(const u8* left, const u8* right, const Item* items, long long n, u64* sums) {
    __shared__ u8 t1[256];
    __shared__ u64 lds[4];
    const int v = blockIdx.y;
    const long long b = blockIdx.z;
    const Item* it = items + b;
    t1[threadIdx.x] = it->t1[v][threadIdx.x];
    __syncthreads();
    const bool swap = (it->flags & F_SWAP) != 0;
    const u8* p = ((v == 1) != swap ? right : left) + b * n * 3;
    const long long nq = (n + 3) / 4, stride = (long long)gridDim.x * BLOCK;
    u64 s[1] = {0ull};
    for (long long q = (long long)blockIdx.x * BLOCK + threadIdx.x; q < nq; q += stride) {
        const long long left_px = n - 4 * q;
        const int nv = left_px < 4 ? (int)left_px : 4;
        unsigned w[3], t = 0u;
        load_rgb4(p + 12 * q, nv, w);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            t += j < nv ? luma_of(t1[rgb_byte(w, 3 * j)], t1[rgb_byte(w, 3 * j + 1)], t1[rgb_byte(w, 3 * j + 2)]) : 0u;
        s[0] += t;
    }
    block_sum<1>(s, lds);
    if (threadIdx.x == 0) sums[(b * 2 + v) * gridDim.x + blockIdx.x] = s[0];
}

// ---------------------------------------------------------------- passes 2 and 3
struct Args {
    const u8* src[2];          // left, right [B,H,W,3]
    const Item* items;
    const float* table;        // [3][256], device memory
    const u64* sums;           // [B][2][GS]
    u64* occ;                  // [B][GO][3]
    int GS, GO, have_occ;
    const void* disp;          // [B,H,W] contiguous
    const void* label;         // pixel (b, h, x) at b * y_img + h * y_row + x
    const float* rdisp;        // right_view's maps of the full items, [B,H,W] contiguous, or null
    const float* rlabel;
    long long y_row, y_img;
    float scale;
    int disp_dtype, label_dtype;
    float* view[2];            // [B,3,th,tw]
    float* map[NMAPS];
    int B, H, W, th, tw;
};

// grid (GO, B): the channel sums of u4 over the crop of the output right view of a flagged item, partials to occ[(b * GO + g) * 3 + ch]
__global__ __launch_bounds__(BLOCK) void occluder_k(Args a) {
    __shared__ u8 t13[256];
    __shared__ u64 lds[4 * 3];
    const long long b = blockIdx.y;
    const Item* it = a.items + b;
    const Geometry g = geometry(it, a.H, a.W, a.th, a.tw);
    if (!(g.flags & F_OCCLUDER)) return;
    build_table(it, 1, a.sums, a.GS, b * 2 + 1, (double)a.H * (double)a.W, t13, lds);
    const bool swap = (g.flags & F_SWAP) != 0, vflip = (g.flags & F_VFLIP) != 0;
    const u8* img = (swap ? a.src[0] : a.src[1]) + b * a.H * a.W * 3;
    const float sat = it->saturation[1];
    const unsigned QW = ((unsigned)a.tw + 3u) / 4u, total = (unsigned)a.th * QW, stride = gridDim.x * BLOCK;
    u64 s[3] = {0ull, 0ull, 0ull};
    for (unsigned q = blockIdx.x * BLOCK + threadIdx.x; q < total; q += stride) {
        const int y = (int)(q / QW), xo = (int)(q - (unsigned)y * QW) * 4, rest = a.tw - xo, nv = rest < 4 ? rest : 4;
        const int row = g.y0 + (vflip ? a.th - 1 - y : y);
        unsigned c[4][3], t[3] = {0u, 0u, 0u};
        src_quad(img + (long long)row * a.W * 3, swap ? a.W - 1 - (g.x0 + xo) : g.x0 + xo, swap, nv, c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned o[3];
            shade(c[j], t13, sat, o);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) t[ch] += j < nv ? o[ch] : 0u;
        }
        s[0] += t[0], s[1] += t[1], s[2] += t[2];
    }
    block_sum<3>(s, lds);
    if (threadIdx.x == 0) {
        u64* w = a.occ + (b * gridDim.x + blockIdx.x) * 3;
        w[0] = s[0], w[1] = s[1], w[2] = s[2];
    }
}

// element i * step of p for i < nv, widened to float: one wide load for step == 1 where the address allows
template <typename T>
__device__ __forceinline__ void fetch4(const T* p, long long step, int nv, float (&v)[4]) {
    struct alignas(4 * sizeof(T)) Quad {
        T e[4];
    };
    if (step == 1 && nv == 4 && aligned_to(p, 4 * (int)sizeof(T))) {
        const Quad q = *reinterpret_cast<const Quad*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (float)q.e[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < nv ? (float)p[j * step] : 0.f;
    }
}

// grid (GW, 2 + NMAPS, B): job blockIdx.y of item blockIdx.z writes one output -- 0, 1 the views, then the maps in Args::map's order;
// a null output has no work
__global__ __launch_bounds__(BLOCK) void write_k(Args a) {
    __shared__ float tab[3 * 256];
    __shared__ u8 t13[256];
    __shared__ u64 lds[4 * 3];
    const int job = blockIdx.y;
    const long long b = blockIdx.z;
    const Item* it = a.items + b;
    const Geometry g = geometry(it, a.H, a.W, a.th, a.tw);
    const bool swap = (g.flags & F_SWAP) != 0, vflip = (g.flags & F_VFLIP) != 0;
    const unsigned stride = gridDim.x * BLOCK;
    if (job < 2) {
        float* out = job ? a.view[1] : a.view[0];
        if (!out) return;
        for (int i = threadIdx.x; i < 3 * 256; i += BLOCK) tab[i] = a.table[i];
        build_table(it, job, a.sums, a.GS, b * 2 + job, (double)a.H * (double)a.W, t13, lds);
        const bool occ = job == 1 && a.have_occ && (g.flags & F_OCCLUDER) != 0;       // (the same for the whole workgroup)
        unsigned colour[3] = {0u, 0u, 0u};
        if (occ) {
            u64 s[3] = {0ull, 0ull, 0ull};
            for (int k = threadIdx.x; k < a.GO; k += BLOCK) {
                const u64* w = a.occ + (b * a.GO + k) * 3;
                s[0] += w[0], s[1] += w[1], s[2] += w[2];
            }
            block_sum<3>(s, lds);
            const u64 n = (u64)a.th * (u64)a.tw;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) colour[ch] = (unsigned)(s[ch] / n) & 255u;
        }
        const u8* img = ((job == 1) != swap ? a.src[1] : a.src[0]) + b * a.H * a.W * 3;
        const float sat = it->saturation[job];
        const long long plane = (long long)a.th * a.tw;
        const unsigned QW = ((unsigned)a.tw + 3u) / 4u, total = (unsigned)a.th * QW;
        for (unsigned q = blockIdx.x * BLOCK + threadIdx.x; q < total; q += stride) {
            const int y = (int)(q / QW), xo = (int)(q - (unsigned)y * QW) * 4, rest = a.tw - xo, nv = rest < 4 ? rest : 4;
            const int row = g.y0 + (vflip ? a.th - 1 - y : y);
            unsigned c[4][3];
            src_quad(img + (long long)row * a.W * 3, swap ? a.W - 1 - (g.x0 + xo) : g.x0 + xo, swap, nv, c);
            const bool in_rows = occ && y >= g.r0 && y < g.r1;
            float f[3][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned o[3];
                shade(c[j], t13, sat, o);
                const bool paint = in_rows && xo + j >= g.c0 && xo + j < g.c1;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) f[ch][j] = tab[ch * 256 + (paint ? colour[ch] : o[ch])];
            }
            float* o = out + (b * 3 * a.th + y) * a.tw + xo;
            store4(o, nv, f[0]);
            store4(o + plane, nv, f[1]);
            store4(o + 2 * plane, nv, f[2]);
        }
        return;
    }
    const int mj = job - 2;
    float* out = nullptr;
#pragma unroll
    for (int i = 0; i < NMAPS; ++i) out = mj == i ? a.map[i] : out;
    if (!out) return;
    const bool is_label = mj >= 4;
    const int k = mj == 0 || mj == 4 ? 1 : mj == 1 || mj == 6 ? 4 : mj == 2 ? 8 : mj == 3 ? 16 : 2;
    const int Ho = a.th / k, Wo = a.tw / k;
    const float* warped = is_label ? a.rlabel : a.rdisp;      // a swapped item reads right_view's maps
    const long long srow = swap || !is_label ? (long long)a.W : a.y_row, simg = swap || !is_label ? (long long)a.H * a.W : a.y_img;
    const long long step = swap ? -(long long)k : (long long)k;
    const float scale = swap ? 1.f : a.scale;
    const unsigned QW = ((unsigned)Wo + 3u) / 4u, total = (unsigned)Ho * QW;
    for (unsigned q = blockIdx.x * BLOCK + threadIdx.x; q < total; q += stride) {
        const int y = (int)(q / QW), xo = (int)(q - (unsigned)y * QW) * 4, rest = Wo - xo, nv = rest < 4 ? rest : 4;
        const int row = g.y0 + (vflip ? a.th - 1 - y * k : y * k);
        const int col = swap ? a.W - 1 - (g.x0 + xo * k) : g.x0 + xo * k;
        const long long off = b * simg + (long long)row * srow + col;
        float v[4];
        if (swap) {
            if (warped) {
                fetch4(warped + off, step, nv, v);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = is_label ? FILL_LABEL : FILL_DISPARITY;
            }
        } else if (is_label) {
            if (a.label_dtype == LT_I64)
                fetch4(reinterpret_cast<const long long*>(a.label) + off, step, nv, v);
            else if (a.label_dtype == LT_U8)
                fetch4(reinterpret_cast<const u8*>(a.label) + off, step, nv, v);
            else
                fetch4(reinterpret_cast<const float*>(a.label) + off, step, nv, v);
        } else {
            if (a.disp_dtype == DT_I32)
                fetch4(reinterpret_cast<const int*>(a.disp) + off, step, nv, v);
            else
                fetch4(reinterpret_cast<const float*>(a.disp) + off, step, nv, v);
        }
        if (!is_label) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ss::mul_rn(v[j], scale);
        }
        store4(out + (b * Ho + y) * Wo + xo, nv, v);
    }
}

// ---------------------------------------------------------------- the host side
// B, H, W, th, tw > 0 and th <= H, tw <= W checked by the caller: 0 where the kernels take the shape
int shape_status(int B, int H, int W, int th, int tw) {
    if (3ll * B * H * W >= (1ll << 31) || B > MAX_ITEMS) return SS_ERR_UNSUPPORTED;
    return SS_OK;
}

int cap_for(int B, int share, int most) {
    const int c = GV / (share * B) < 1 ? 1 : GV / (share * B);
    return c < most ? c : most;
}

// workgroups per (item, view) of the luma pass and per item of the occluder pass: every entry point derives them from the shape alone
int stat_groups(int B, int H, int W) { return grid_for(((long long)H * W + 3) / 4, cap_for(B, 2, MAX_STAT_GROUPS)); }
int occ_groups(int B, int th, int tw) { return grid_for((long long)th * ((tw + 3) / 4), cap_for(B, 1, MAX_OCC_GROUPS)); }

long long sums_bytes(int B, int H, int W) { return ((long long)B * 2 * stat_groups(B, H, W) * 8 + PART_ALIGN - 1) / PART_ALIGN * PART_ALIGN; }
long long total_bytes(int B, int H, int W, int th, int tw) { return sums_bytes(B, H, W) + (long long)B * occ_groups(B, th, tw) * 3 * 8; }

bool sizes_ok(int B, int H, int W, int th, int tw) { return B > 0 && H > 0 && W > 0 && th > 0 && tw > 0 && th <= H && tw <= W; }

}  // namespace

extern "C" int ss_augment_param_bytes(int B, long long* bytes) {
    SS_REQUIRE(bytes && B > 0);
    if (B > MAX_ITEMS) return SS_ERR_UNSUPPORTED;
    *bytes = (long long)B * (long long)sizeof(Item);
    return SS_OK;
}

extern "C" int ss_augment_scratch_bytes(int B, int H, int W, int th, int tw, long long* bytes) {
    SS_REQUIRE(bytes && sizes_ok(B, H, W, th, tw));
    if (int s = shape_status(B, H, W, th, tw)) return s;
    *bytes = total_bytes(B, H, W, th, tw);
    return SS_OK;
}

extern "C" int ss_augment_stats_fwd(const unsigned char* left, const unsigned char* right, const void* params, int B, int H, int W,
                                    int th, int tw, void* workspace, long long workspace_bytes, ss_stream_t stream) {
    SS_REQUIRE(left && right && params && workspace && sizes_ok(B, H, W, th, tw));
    if (int s = shape_status(B, H, W, th, tw)) return s;
    SS_REQUIRE(workspace_bytes >= total_bytes(B, H, W, th, tw));
    SS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(params) & 3u) == 0);
    hipLaunchKernelGGL(stats_k, dim3(stat_groups(B, H, W), 2, B), dim3(BLOCK), 0, ss::as_stream(stream), left, right,
                       static_cast<const Item*>(params), (long long)H * W, static_cast<u64*>(workspace));
    return ss::check_launch();
}

extern "C" int ss_augment_occluder_fwd(const unsigned char* left, const unsigned char* right, const void* params, int B, int H, int W,
                                       int th, int tw, void* workspace, long long workspace_bytes, ss_stream_t stream) {
    SS_REQUIRE(left && right && params && workspace && sizes_ok(B, H, W, th, tw));
    if (int s = shape_status(B, H, W, th, tw)) return s;
    SS_REQUIRE(workspace_bytes >= total_bytes(B, H, W, th, tw));
    SS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(params) & 3u) == 0);
    Args a{};
    a.src[0] = left, a.src[1] = right, a.items = static_cast<const Item*>(params);
    a.sums = static_cast<const u64*>(workspace);
    a.occ = reinterpret_cast<u64*>(static_cast<char*>(workspace) + sums_bytes(B, H, W));
    a.GS = stat_groups(B, H, W), a.GO = occ_groups(B, th, tw), a.have_occ = 1;
    a.B = B, a.H = H, a.W = W, a.th = th, a.tw = tw;
    hipLaunchKernelGGL(occluder_k, dim3(a.GO, B), dim3(BLOCK), 0, ss::as_stream(stream), a);
    return ss::check_launch();
}

extern "C" int ss_augment_write_fwd(const unsigned char* left, const unsigned char* right, const void* params, const float* table,
                                    const void* disparity, int disp_dtype, float disp_scale, const void* label, int label_dtype,
                                    long long label_row_stride, long long label_image_stride, const float* right_disparity,
                                    const float* right_label, int B, int H, int W, int th, int tw, const void* workspace,
                                    long long workspace_bytes, int have_occluder, float* out_left, float* out_right,
                                    float* disparity_out, float* disparity_4, float* disparity_8, float* disparity_16, float* label_out,
                                    float* label_2, float* label_4, ss_stream_t stream) {
    SS_REQUIRE(left && right && params && workspace && sizes_ok(B, H, W, th, tw));
    const bool any_view = out_left || out_right;
    const bool any_disp = disparity_out || disparity_4 || disparity_8 || disparity_16, any_label = label_out || label_2 || label_4;
    SS_REQUIRE(any_view || any_disp || any_label);
    SS_REQUIRE(have_occluder == 0 || have_occluder == 1);
    if (any_view) SS_REQUIRE(table);
    if (any_disp) SS_REQUIRE(disparity && (disp_dtype == DT_F32 || disp_dtype == DT_I32));
    if (any_label) {
        SS_REQUIRE(label && label_dtype >= LT_I64 && label_dtype <= LT_F32);
        SS_REQUIRE(label_row_stride >= W && label_image_stride >= (long long)(H - 1) * label_row_stride + W);
    }
    if (int s = shape_status(B, H, W, th, tw)) return s;
    const bool levels = disparity_4 || disparity_8 || disparity_16 || label_2 || label_4;
    if (levels && (th % 16 != 0 || tw % 16 != 0)) return SS_ERR_UNSUPPORTED;
    SS_REQUIRE(workspace_bytes >= total_bytes(B, H, W, th, tw));
    SS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(params) & 3u) == 0);
    Args a{};
    a.src[0] = left, a.src[1] = right, a.items = static_cast<const Item*>(params), a.table = table;
    a.sums = static_cast<const u64*>(workspace);
    a.occ = reinterpret_cast<u64*>(static_cast<char*>(const_cast<void*>(workspace)) + sums_bytes(B, H, W));
    a.GS = stat_groups(B, H, W), a.GO = occ_groups(B, th, tw), a.have_occ = have_occluder;
    a.disp = disparity, a.label = label, a.rdisp = right_disparity, a.rlabel = right_label;
    a.y_row = label_row_stride, a.y_img = label_image_stride, a.scale = disp_scale;
    a.disp_dtype = disp_dtype, a.label_dtype = label_dtype;
    a.view[0] = out_left, a.view[1] = out_right;
    float* maps[NMAPS] = {disparity_out, disparity_4, disparity_8, disparity_16, label_out, label_2, label_4};
    for (int i = 0; i < NMAPS; ++i) a.map[i] = maps[i];
    a.B = B, a.H = H, a.W = W, a.th = th, a.tw = tw;
    const int gw = grid_for((long long)th * ((tw + 3) / 4), cap_for(B, 2, GV));
    hipLaunchKernelGGL(write_k, dim3(gw, 2 + NMAPS, B), dim3(BLOCK), 0, ss::as_stream(stream), a);
    return ss::check_launch();
}
