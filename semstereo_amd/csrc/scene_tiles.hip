// Scene inference around the model call: the windows of a scene pair cut and normalised in one pass, and the finished tiles gathered
// into the mosaic.  The reference has nothing of the kind (its evaluation loader carries top_pad / right_pad keys that are always 0).
//   window   tile i of size th x tw at origin (oy, ox) = origins[i], anywhere: it may overhang the scene on any side
//   views    out[i][c][y][x] = table[c][scene[oy + y][ox + x][c]] inside the scene, 0.0f off it (the mean colour in normalised space)
//   weights  per axis w(i) = min(i + 1, T - i, R) for window-local index i, tile size T, ramp R: integers >= 1; a tile pixel weighs
//            float(wy) * float(wx)
//   blend    per mosaic pixel, over the covering RESIDENT tiles in ascending (ty, tx): num = num + w * v, den = den + w, each product
//            and each sum rounded to fp32 (nothing contracted into an fma), out = num / den, one IEEE division -- and under ONE
//            tile out = v, the tile's own value, not (w * v) / w, which rounds twice.  The same per logit channel; label = the lowest index of the largest blended logit (np.argmax's rule, metrics_decode.h); spread = max - min
//            of the covering tiles' disparities (0 under one tile); count = their number
// The tiles are read IN PLACE through tables of addresses (entry 0: not resident): the model's own output tensors, a batch of tiles
// being data_ptr() + b * stride.  Every tile pixel maps to one mosaic pixel and is read once.  The order is fixed and nothing is
// atomic: two calls give the same bits.  Kernels of the stream.h family: BLOCK threads, a capped grid-stride loop, a lane takes 4
// consecutive pixels of a row, 64-bit element offsets.  Nothing here allocates, copies or synchronises, and nothing comes back to the host.
#include "common.h"
#include "metrics_decode.h"
#include "stream.h"

namespace {

using namespace ss::stream;    // BLOCK, grid_for, RowQuad, row_quad, load4, load_rgb4, rgb_byte, store4
using ss::metrics::argmax_take;

constexpr int GV = 2048;                 // workgroups of a pass
constexpr int MAX_C = 8;                 // logit channels: 4 accumulators each per lane
constexpr int MAX_WINDOWS = 256;         // windows per axis: the origins of both axes are 2 KB of LDS
constexpr long long MAX_ELEMENTS = 1ll << 31;

typedef unsigned char u8;

// ---------------------------------------------------------------- views
struct ViewArgs {
    const u8* src[2];          // [H,W,3]
    float* out[2];             // [n,3,th,tw]
    const int* origins;        // [n][2]: (y, x)
    const float* table;        // [3][256], device memory
    int n, th, tw, H, W;
};

// grid (G, views)
__global__ __launch_bounds__(BLOCK) void tile_views_k(ViewArgs a) {
    __shared__ float tab[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += BLOCK) tab[i] = a.table[i];
    __syncthreads();
    const u8* src = blockIdx.y ? a.src[1] : a.src[0];
    float* out = blockIdx.y ? a.out[1] : a.out[0];
    const unsigned QW = ((unsigned)a.tw + 3u) / 4u, total = (unsigned)a.n * (unsigned)a.th * QW;
    const unsigned stride = gridDim.x * BLOCK;
    const long long plane = (long long)a.th * a.tw;
    for (unsigned q = blockIdx.x * BLOCK + threadIdx.x; q < total; q += stride) {
        const RowQuad r = row_quad(q, QW, (unsigned)a.th, a.tw);         // r.b: the window, r.h: its row
        const long long gy = (long long)a.origins[2 * r.b] + r.h, gx = (long long)a.origins[2 * r.b + 1] + r.x0;
        const bool row_in = gy >= 0 && gy < a.H;
        float c[3][4];
        if (row_in && gx >= 0 && gx + r.nv <= a.W) {
            unsigned w[3];
            load_rgb4(src + (gy * a.W + gx) * 3, r.nv, w);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) c[ch][j] = tab[ch * 256 + rgb_byte(w, 3 * j + ch)];
        } else {                                                         // the group straddles the scene's edge, or lies off it
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c[0][j] = c[1][j] = c[2][j] = 0.f;
                if (row_in && j < r.nv && gx + j >= 0 && gx + j < a.W) {
                    const u8* p = src + (gy * a.W + gx + j) * 3;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) c[ch][j] = tab[ch * 256 + p[ch]];
                }
            }
        }
        float* o = out + ((long long)r.b * 3 * a.th + r.h) * a.tw + r.x0;
        store4(o, r.nv, c[0]);
        store4(o + plane, r.nv, c[1]);
        store4(o + 2 * plane, r.nv, c[2]);
    }
}

// ---------------------------------------------------------------- blend
struct BlendArgs {
    const long long* dtab;     // [nty * ntx] addresses of float [th,tw]; 0: not resident
    const long long* ltab;     // ... of float [C,th,tw]; null without logits
    const int* oy;             // [nty] ascending
    const int* ox;             // [ntx] ascending
    float* disparity;          // [H,W]
    float* logits;             // [C,H,W]
    u8* label;
    float* spread;
    u8* count;
    int nty, ntx, th, tw, C, ry, rx, H, W, y0, y1;
};

// o[0 .. n) ascending.  The windows that can hold v are [first_reaching, end_starting): the first k with o[k] + t > v, and one past
// the last k with o[k] <= v.  (Whether a window holds a pixel is tested again per pixel: a table that is not ascending gives a wrong
// mosaic, never an address outside a tile.)
__device__ __forceinline__ int first_reaching(const int* o, int n, int t, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (o[m] > v - t) hi = m; else lo = m + 1;
    }
    return lo;
}
__device__ __forceinline__ int end_starting(const int* o, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (o[m] <= v) lo = m + 1; else hi = m;
    }
    return lo;
}
__device__ __forceinline__ int feather(int i, int T, int R) {
    const int e = i + 1 < T - i ? i + 1 : T - i;
    return e < R ? e : R;
}
// One more tile's value v of weight w into the numerator of a pixel that `seen` tiles of total weight `den` cover so far.  The first
// tile's value is kept as it is -- under ONE tile the mosaic is the tile's own value, nothing multiplied or divided -- and is
// weighted when the second arrives (den is then the first tile's weight): the products and sums of 0 + w0 v0 + w1 v1 + ..., in that order.
__device__ __forceinline__ float blend_in(float num, float den, float seen, float w, float v) {
    if (seen == 0.f) return v;
    if (seen == 1.f) num = ss::mul_rn(den, num);
    return ss::add_rn(num, ss::mul_rn(w, v));
}
// 4 tile pixels at p: one wide access or four scalars where the whole group lies in the window, else the pixels that do
__device__ __forceinline__ void load_covered(const float* p, bool whole, const bool (&in)[4], float (&v)[4]) {
    if (whole) {
        load4(p, 4, v);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = 0.f;
            if (in[j]) v[j] = p[j];
        }
    }
}

__global__ __launch_bounds__(BLOCK) void tile_blend_k(BlendArgs a) {
    __shared__ int s_oy[MAX_WINDOWS], s_ox[MAX_WINDOWS];
    for (int i = threadIdx.x; i < a.nty; i += BLOCK) s_oy[i] = a.oy[i];
    for (int i = threadIdx.x; i < a.ntx; i += BLOCK) s_ox[i] = a.ox[i];
    __syncthreads();
    const int W = a.W, th = a.th, tw = a.tw;
    const int C = (a.logits || a.label) ? a.C : 0;                       // (the logits are not read for the other outputs)
    const unsigned QW = ((unsigned)W + 3u) / 4u, total = (unsigned)(a.y1 - a.y0) * QW;
    const unsigned stride = gridDim.x * BLOCK;
    const long long plane = (long long)th * tw, HW = (long long)a.H * W;
    for (unsigned q = blockIdx.x * BLOCK + threadIdx.x; q < total; q += stride) {
        const unsigned row = q / QW;
        const int y = a.y0 + (int)row, x0 = (int)((q - row * QW) * 4u);
        const int nv = W - x0 < 4 ? W - x0 : 4;
        const int ty0 = first_reaching(s_oy, a.nty, th, y), ty1 = end_starting(s_oy, a.nty, y);
        const int tx0 = first_reaching(s_ox, a.ntx, tw, x0), tx1 = end_starting(s_ox, a.ntx, x0 + nv - 1);
        float num[4], den[4], hi[4], lo[4], cnt[4], nl[MAX_C][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            num[j] = den[j] = cnt[j] = 0.f;
            hi[j] = -INFINITY, lo[j] = INFINITY;
#pragma unroll
            for (int c = 0; c < MAX_C; ++c) nl[c][j] = 0.f;
        }
        for (int ty = ty0; ty < ty1; ++ty) {
            const int iy = y - s_oy[ty];
            if (iy < 0 || iy >= th) continue;
            const float wy = (float)feather(iy, th, a.ry);
            for (int tx = tx0; tx < tx1; ++tx) {
                const long long da = a.dtab[ty * a.ntx + tx];
                if (!da) continue;                                       // not resident
                const int ix0 = x0 - s_ox[tx];
                bool in[4];
                float w[4], v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ix = ix0 + j;
                    in[j] = j < nv && ix >= 0 && ix < tw;
                    w[j] = ss::mul_rn(wy, (float)feather(ix, tw, a.rx));
                }
                const bool whole = nv == 4 && ix0 >= 0 && ix0 + 4 <= tw;
                const long long at = (long long)iy * tw + ix0;
                load_covered(reinterpret_cast<const float*>(da) + at, whole, in, v);
                float seen[4], den0[4];                                  // tiles over the pixel and their weight before this one
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    seen[j] = cnt[j], den0[j] = den[j];
                    if (in[j]) {
                        num[j] = blend_in(num[j], den0[j], seen[j], w[j], v[j]);
                        den[j] = ss::add_rn(den[j], w[j]);
                        hi[j] = ((v[j] > hi[j]) | (v[j] != v[j])) ? v[j] : hi[j];      // (a NaN stays, as torch.maximum keeps it)
                        lo[j] = ((v[j] < lo[j]) | (v[j] != v[j])) ? v[j] : lo[j];
                        cnt[j] += 1.f;
                    }
                }
                const long long la = C > 0 ? a.ltab[ty * a.ntx + tx] : 0ll;
                if (!la) continue;
#pragma unroll
                for (int c = 0; c < MAX_C; ++c) {
                    if (c < C) {
                        load_covered(reinterpret_cast<const float*>(la) + c * plane + at, whole, in, v);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (in[j]) nl[c][j] = blend_in(nl[c][j], den0[j], seen[j], w[j], v[j]);
                    }
                }
            }
        }
        const long long px = (long long)y * W + x0;
        float v[4];
        if (a.disparity) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = cnt[j] == 1.f ? num[j] : num[j] / den[j];
            store4(a.disparity + px, nv, v);
        }
        if (a.spread) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ss::sub_rn(hi[j], lo[j]);
            store4(a.spread + px, nv, v);
        }
        if (a.count) store4(a.count + px, nv, cnt);
        if (C > 0) {
            float best[4] = {0.f, 0.f, 0.f, 0.f}, idx[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < MAX_C; ++c) {
                if (c < C) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        v[j] = cnt[j] == 1.f ? nl[c][j] : nl[c][j] / den[j];
                        const bool take = c == 0 || argmax_take(best[j], v[j]);
                        best[j] = take ? v[j] : best[j];
                        idx[j] = take ? (float)c : idx[j];
                    }
                    if (a.logits) store4(a.logits + c * HW + px, nv, v);
                }
            }
            if (a.label) store4(a.label + px, nv, idx);
        }
    }
}

}  // namespace

extern "C" int ss_tile_views_fwd(const unsigned char* left, const unsigned char* right, const int* origins, const float* table, int n,
                                 int th, int tw, int H, int W, float* out_left, float* out_right, ss_stream_t stream) {
    SS_REQUIRE(left && origins && table && out_left);
    SS_REQUIRE((right == nullptr) == (out_right == nullptr));
    SS_REQUIRE(n > 0 && th > 0 && tw > 0 && H > 0 && W > 0);
    if ((long long)H * W * 3 >= MAX_ELEMENTS || (long long)n * 3 * th * tw >= MAX_ELEMENTS) return SS_ERR_UNSUPPORTED;
    ViewArgs a{{left, right}, {out_left, out_right}, origins, table, n, th, tw, H, W};
    const long long quads = (long long)n * th * ((tw + 3) / 4);
    hipLaunchKernelGGL(tile_views_k, dim3(grid_for(quads, GV), right ? 2 : 1), dim3(BLOCK), 0, ss::as_stream(stream), a);
    return ss::check_launch();
}

extern "C" int ss_tile_blend_fwd(const long long* disp_tiles, const long long* logit_tiles, const int* origin_y, const int* origin_x,
                                 int nty, int ntx, int th, int tw, int C, int ry, int rx, int H, int W, int y0, int y1,
                                 float* disparity, float* logits, unsigned char* label, float* spread, unsigned char* count,
                                 ss_stream_t stream) {
    SS_REQUIRE(disp_tiles && origin_y && origin_x);
    SS_REQUIRE(disparity || logits || label || spread || count);
    SS_REQUIRE(nty > 0 && ntx > 0 && th > 0 && tw > 0 && H > 0 && W > 0 && C >= 0);
    SS_REQUIRE((logit_tiles != nullptr) == (C > 0));
    SS_REQUIRE(logit_tiles || !(logits || label));
    SS_REQUIRE(ry >= 1 && rx >= 1);
    SS_REQUIRE(0 <= y0 && y0 <= y1 && y1 <= H);
    if (C > MAX_C || nty > MAX_WINDOWS || ntx > MAX_WINDOWS) return SS_ERR_UNSUPPORTED;
    if ((long long)H * W * (C > 0 ? C : 1) >= MAX_ELEMENTS || (long long)th * tw * (C > 0 ? C : 1) >= MAX_ELEMENTS) return SS_ERR_UNSUPPORTED;
    if (y0 == y1) return SS_OK;
    BlendArgs a{disp_tiles, logit_tiles, origin_y, origin_x, disparity, logits, label, spread, count, nty, ntx, th, tw, C, ry, rx, H, W, y0, y1};
    const long long quads = (long long)(y1 - y0) * ((W + 3) / 4);
    hipLaunchKernelGGL(tile_blend_k, dim3(grid_for(quads, GV)), dim3(BLOCK), 0, ss::as_stream(stream), a);
    return ss::check_launch();
}
