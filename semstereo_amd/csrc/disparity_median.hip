// Disparity refinement, the step after the row fill: a 2-D median in which a pixel is smoothed only with pixels of its own predicted
// class.  The definitions (valid, class, window, members, order, pick, target, outputs) are written once, in
// include/semstereo_hip.h, section "disparity refinement: class-aware median".  Nothing is interpolated and no floating-point
// arithmetic touches a value: a disparity is compared with the range, turned into its monotone integer key, selected, and turned
// back, so the PyTorch composition of semstereo_amd/refine.py gives the same bits.
//
// A kernel of the stream.h family (BLOCK threads, a capped grid with a stride loop, a lane owns 4 consecutive columns, 64-bit element
// offsets) with the one shape that family did not have: a 2-D tile with a halo in LDS.  Per tile of TH x TW = 16 x 64 output pixels:
//   1. the tile and its halo, (TH + 2r) x (TW + 2r) pixels, are staged: one 32-bit key per pixel and one byte holding the class
//      (0 .. 7, 8 for none) and the valid bit.  The global reads are the ALIGNED quads that cover the staged columns (TW / 4 + 2 per
//      row); the address is per (b, y, x) and the bounds are per image, so a halo never reads the neighbouring row or image, and a
//      pixel off the image is staged as not valid.  The label is decoded once per staged pixel (refine_class.h).
//   2. lane (ty, tx) owns the row-quad (ty, 4 tx .. 4 tx + 3).  Its four windows share 2r + 1 rows of 2r + 4 staged columns, each read
//      once (16-byte reads: the row stride KS is a multiple of 4 words).  Per pixel the N = (2r + 1)^2 slots go through a fixed
//      compare-exchange network on the integer keys (min / max, every index a compile-time constant: nothing is indexed at run time,
//      so nothing goes to scratch).  A slot that is no member holds a sentinel -- the 0th, 2nd, 4th ... non-member in scan order
//      INT32_MIN, the 1st, 3rd ... INT32_MAX -- so that the element at the FIXED position (N - 1) / 2 of all N is the lower median of
//      the n members: with m = N - n non-members ceil(m / 2) sentinels lie below, and (N - 1) / 2 - ceil(m / 2) = (n - 1) / 2 for
//      both parities of m (N is odd).  19 exchanges for N = 9 and 99 for N = 25 -- rank counting would take N^2 = 81 / 625
//      comparisons and as many additions.
//   3. `where`, the centre's validity, fill_holes and min_count decide at the write only.
// LDS: (TH + 2r) x KS x 5 bytes, 6.8 KB at r = 2.  Every LDS cell is written by one thread per tile and the selection is integer
// minima and maxima: two calls give the same bits.  Nothing here allocates, copies or synchronises, and nothing comes back to the host.
#include "common.h"
#include "refine_class.h"
#include "stream.h"

namespace {

using namespace ss::stream;    // BLOCK, load4, store4
using ss::metrics::LT_F32;     // label sources: the codes of every label_dtype
using ss::metrics::LT_I64;
using ss::refine::NCLS;
using ss::refine::classes4;

constexpr int TH = 16, TW = 64;          // output pixels of a tile: one row-quad per lane (semstereo_amd/refine.py: MEDIAN_TILE)
constexpr int MAX_R = 2;                 // the largest radius with a network here
constexpr int KS = TW + 2 * MAX_R;       // staged row stride, in keys and in bytes: a multiple of 4
constexpr int QS = TW / 4 + 2;           // aligned global quads that cover a staged row
constexpr int GV = 2048;                 // workgroups of a pass
constexpr int VALID = 16;                // the valid bit of a pixel's byte; bits 0-3 the class
constexpr int KEY_MIN = (int)0x80000000, KEY_MAX = 0x7fffffff;      // the sentinels: no valid value has these keys
// (TH * TW / 4 == BLOCK: one row-quad per lane; KS % 4 == 0: 16-byte reads of the staged rows)

typedef unsigned char u8;

struct MedianArgs {
    const float* disp;         // [B,H,W] contiguous
    const void* label;         // pixel (b, y, x) at b * y_img + y * y_row + x, or null
    const u8* where;           // [B,H,W], or null
    float* out;                // [B,H,W]
    u8* count;                 // [B,H,W], or null
    long long y_row, y_img;
    float lo, hi;
    int label_dtype;
    int B, H, W;
    unsigned tiles_y, tiles_x; // per image
    int same_class, fill_holes, min_count;
};

// the order: k = b ^ ((b >> 31) & 0x7fffffff) of the value's bits b, compared as signed integers; its own inverse
__device__ __forceinline__ int key_of(int b) { return b ^ ((b >> 31) & 0x7fffffff); }

__device__ __forceinline__ void cx(int& a, int& b) {
    const int lo = min(a, b), hi = max(a, b);
    a = lo, b = hi;
}

// the element at position (N - 1) / 2 of the ascending order of p[0 .. N - 1]; p is destroyed
__device__ __forceinline__ int middle(int (&p)[9]) {
    cx(p[1], p[2]); cx(p[4], p[5]); cx(p[7], p[8]); cx(p[0], p[1]); cx(p[3], p[4]); cx(p[6], p[7]); cx(p[1], p[2]);
    cx(p[4], p[5]); cx(p[7], p[8]); cx(p[0], p[3]); cx(p[5], p[8]); cx(p[4], p[7]); cx(p[3], p[6]); cx(p[1], p[4]);
    cx(p[2], p[5]); cx(p[4], p[7]); cx(p[4], p[2]); cx(p[6], p[4]); cx(p[4], p[2]);
    return p[4];
}
__device__ __forceinline__ int middle(int (&p)[25]) {
    cx(p[0], p[1]); cx(p[3], p[4]); cx(p[2], p[4]); cx(p[2], p[3]); cx(p[6], p[7]); cx(p[5], p[7]); cx(p[5], p[6]);
    cx(p[9], p[10]); cx(p[8], p[10]); cx(p[8], p[9]); cx(p[12], p[13]); cx(p[11], p[13]); cx(p[11], p[12]); cx(p[15], p[16]);
    cx(p[14], p[16]); cx(p[14], p[15]); cx(p[18], p[19]); cx(p[17], p[19]); cx(p[17], p[18]); cx(p[21], p[22]); cx(p[20], p[22]);
    cx(p[20], p[21]); cx(p[23], p[24]); cx(p[2], p[5]); cx(p[3], p[6]); cx(p[0], p[6]); cx(p[0], p[3]); cx(p[4], p[7]);
    cx(p[1], p[7]); cx(p[1], p[4]); cx(p[11], p[14]); cx(p[8], p[14]); cx(p[8], p[11]); cx(p[12], p[15]); cx(p[9], p[15]);
    cx(p[9], p[12]); cx(p[13], p[16]); cx(p[10], p[16]); cx(p[10], p[13]); cx(p[20], p[23]); cx(p[17], p[23]); cx(p[17], p[20]);
    cx(p[21], p[24]); cx(p[18], p[24]); cx(p[18], p[21]); cx(p[19], p[22]); cx(p[8], p[17]); cx(p[9], p[18]); cx(p[0], p[18]);
    cx(p[0], p[9]); cx(p[10], p[19]); cx(p[1], p[19]); cx(p[1], p[10]); cx(p[11], p[20]); cx(p[2], p[20]); cx(p[2], p[11]);
    cx(p[12], p[21]); cx(p[3], p[21]); cx(p[3], p[12]); cx(p[13], p[22]); cx(p[4], p[22]); cx(p[4], p[13]); cx(p[14], p[23]);
    cx(p[5], p[23]); cx(p[5], p[14]); cx(p[15], p[24]); cx(p[6], p[24]); cx(p[6], p[15]); cx(p[7], p[16]); cx(p[7], p[19]);
    cx(p[13], p[21]); cx(p[15], p[23]); cx(p[7], p[13]); cx(p[7], p[15]); cx(p[1], p[9]); cx(p[3], p[11]); cx(p[5], p[17]);
    cx(p[11], p[17]); cx(p[9], p[17]); cx(p[4], p[10]); cx(p[6], p[12]); cx(p[7], p[14]); cx(p[4], p[6]); cx(p[4], p[7]);
    cx(p[12], p[14]); cx(p[10], p[14]); cx(p[6], p[7]); cx(p[10], p[12]); cx(p[6], p[10]); cx(p[6], p[17]); cx(p[12], p[17]);
    cx(p[7], p[17]); cx(p[7], p[10]); cx(p[12], p[18]); cx(p[7], p[12]); cx(p[10], p[18]); cx(p[12], p[20]); cx(p[10], p[20]);
    cx(p[10], p[12]);
    return p[12];
}

// 4 count bytes: one wide store, or nv bytes
__device__ __forceinline__ void store_counts(u8* p, int nv, const int (&v)[4]) {
    if (nv == 4 && aligned_to(p, 4)) {
        *reinterpret_cast<unsigned*>(p) = (unsigned)v[0] | (unsigned)v[1] << 8 | (unsigned)v[2] << 16 | (unsigned)v[3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) p[j] = (u8)v[j];
    }
}

template <int R>
__global__ __launch_bounds__(BLOCK) void disparity_median_k(MedianArgs a) {
    constexpr int D = 2 * R + 1, N = D * D;          // the window
    constexpr int SH = TH + 2 * R, SW = TW + 2 * R;  // the staged tile
    constexpr int C = 2 * R + 4;                     // staged columns under a lane's four windows
    __shared__ __attribute__((aligned(16))) int key[SH * KS];
    __shared__ __attribute__((aligned(16))) u8 flag[SH * KS];
    const int H = a.H, W = a.W;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const unsigned per_image = a.tiles_y * a.tiles_x, tiles = (unsigned)a.B * per_image;
    for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
        const unsigned b = t / per_image, in_image = t - b * per_image, tile_y = in_image / a.tiles_x;
        const int y0 = (int)tile_y * TH, x0 = (int)(in_image - tile_y * a.tiles_x) * TW;
        const long long base = (long long)b * H * W, ybase = (long long)b * a.y_img;
        // 1 ---- the tile and its halo: staged column s is image column x0 - R + s, staged row sy image row y0 - R + sy
        for (int q = threadIdx.x; q < SH * QS; q += BLOCK) {
            const int sy = q / QS, qx = q - sy * QS;
            const int y = y0 - R + sy, xq = x0 - 4 + 4 * qx;          // the quad's first image column: a multiple of 4
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            int cls[4] = {NCLS, NCLS, NCLS, NCLS};
            int nv = 0;
            if (y >= 0 && y < H && xq >= 0 && xq < W) {
                const int left = W - xq;
                nv = left < 4 ? left : 4;
                load4(a.disp + base + (long long)y * W + xq, nv, v);
                if (a.label) classes4(a.label, a.label_dtype, ybase + (long long)y * a.y_row + xq, nv, cls);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int s = 4 * qx - 4 + R + j;
                if (s >= 0 && s < SW) {
                    const bool valid = (j < nv) & (v[j] >= a.lo) & (v[j] < a.hi);                    // (a NaN fails both)
                    key[sy * KS + s] = key_of(__float_as_int(v[j]));
                    flag[sy * KS + s] = (u8)((j < nv ? cls[j] : NCLS) | (valid ? VALID : 0));
                }
            }
        }
        __syncthreads();
        // 2 ---- the four windows of the lane's row-quad
        const int y = y0 + ty, x = x0 + 4 * tx;
        if (y < H && x < W) {
            const int left = W - x, nv = left < 4 ? left : 4;
            int k[D][C], f[D][C];
#pragma unroll
            for (int dy = 0; dy < D; ++dy) {
                const int row = (ty + dy) * KS + 4 * tx;
                const int4 k0 = *reinterpret_cast<const int4*>(key + row);
                k[dy][0] = k0.x, k[dy][1] = k0.y, k[dy][2] = k0.z, k[dy][3] = k0.w;
                if (R == 2) {
                    const int4 k1 = *reinterpret_cast<const int4*>(key + row + 4);
                    k[dy][C - 4] = k1.x, k[dy][C - 3] = k1.y, k[dy][C - 2] = k1.z, k[dy][C - 1] = k1.w;
                } else {
                    const int2 k1 = *reinterpret_cast<const int2*>(key + row + 4);
                    k[dy][C - 2] = k1.x, k[dy][C - 1] = k1.y;
                }
                const unsigned f0 = *reinterpret_cast<const unsigned*>(flag + row), f1 = *reinterpret_cast<const unsigned*>(flag + row + 4);
#pragma unroll
                for (int c = 0; c < C; ++c) f[dy][c] = (int)(((c < 4 ? f0 : f1) >> (8 * (c & 3))) & 255u);
            }
            u8 on[4] = {1, 1, 1, 1};
            if (a.where) load4(a.where + base + (long long)y * W + x, nv, on);
            float res[4];
            int cnt[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int centre = f[R][R + p], cc = centre & 15;
                const bool own = a.same_class && cc != NCLS;                   // members: valid, and of the centre's class
                const int mask = own ? (VALID | 15) : VALID, wanted = own ? (VALID | cc) : VALID;
                int slot[N];
                int n = 0;
                bool high = false;                                              // the next non-member's sentinel
#pragma unroll
                for (int dy = 0; dy < D; ++dy) {
#pragma unroll
                    for (int dx = 0; dx < D; ++dx) {
                        const bool member = (f[dy][p + dx] & mask) == wanted;
                        slot[dy * D + dx] = member ? k[dy][p + dx] : (high ? KEY_MAX : KEY_MIN);
                        high = member ? high : !high;
                        n += member ? 1 : 0;
                    }
                }
                const int pick = middle(slot);
                const bool target = (on[p] != 0) & (((centre & VALID) != 0) | (a.fill_holes != 0)) & (n >= a.min_count);
                res[p] = __int_as_float(key_of(target ? pick : k[R][R + p]));
                cnt[p] = target ? n : 0;
            }
            const long long o = base + (long long)y * W + x;
            store4(a.out + o, nv, res);
            if (a.count) store_counts(a.count + o, nv, cnt);
        }
        __syncthreads();               // (the next tile's staging)
    }
}

}  // namespace

extern "C" int ss_disparity_median_fwd(const float* disparity, const void* label, int label_dtype, long long label_row_stride,
                                       long long label_image_stride, const unsigned char* where, int B, int H, int W, float lo, float hi,
                                       int radius, int same_class, int fill_holes, int min_count, float* out_disparity,
                                       unsigned char* count, ss_stream_t stream) {
    SS_REQUIRE(disparity && out_disparity && out_disparity != disparity);          // (neighbours are read after a pixel could be written)
    SS_REQUIRE(B > 0 && H > 0 && W > 0);
    if (label) {
        SS_REQUIRE(label_dtype >= LT_I64 && label_dtype <= LT_F32);
        SS_REQUIRE(label_row_stride >= W && label_image_stride >= (long long)(H - 1) * label_row_stride + W);
    }
    SS_REQUIRE(lo < hi);                                   // (false for a NaN)
    SS_REQUIRE(radius >= 1 && (same_class == 0 || same_class == 1) && (fill_holes == 0 || fill_holes == 1));
    SS_REQUIRE(min_count >= 1 && min_count <= (2ll * radius + 1) * (2ll * radius + 1));
    if (radius > MAX_R) return SS_ERR_UNSUPPORTED;
    if ((long long)B * H * W >= (1ll << 31)) return SS_ERR_UNSUPPORTED;
    const unsigned tiles_y = (unsigned)ss::ceil_div(H, TH), tiles_x = (unsigned)ss::ceil_div(W, TW);
    MedianArgs a{disparity, label, where, out_disparity, count, label_row_stride, label_image_stride, lo, hi, label_dtype, B, H, W,
                 tiles_y, tiles_x, same_class, fill_holes, min_count};
    const long long tiles = (long long)B * tiles_y * tiles_x;
    const dim3 grid((unsigned)(tiles < GV ? tiles : GV));
    if (radius == 1)
        hipLaunchKernelGGL(disparity_median_k<1>, grid, dim3(BLOCK), 0, ss::as_stream(stream), a);
    else
        hipLaunchKernelGGL(disparity_median_k<2>, grid, dim3(BLOCK), 0, ss::as_stream(stream), a);
    return ss::check_launch();
}
