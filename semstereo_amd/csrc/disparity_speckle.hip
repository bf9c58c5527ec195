// Disparity refinement, the step before the row fill: small connected blobs of wrong disparity are found and removed, so that the
// fill does not take them for sources.  The definitions (valid, class, link, component, size, speckle, outputs) are written once,
// in include/semstereo_hip.h, section "disparity refinement: speckle removal".  The only floating-point operation is the ONE fp32
// subtraction of a link test; components, sizes and the speckle decision are integers fixed by the definitions, whatever order the
// unions ran in, so the PyTorch composition of semstereo_amd/refine.py gives the same bits and so do two calls.
//
// Connected-component labelling by union-find with the SMALLEST index as the root (speckle_union.h), in four launches on the caller's
// stream.  No launch waits on another workgroup: no cooperative launch, no grid barrier, no flag, no spin loop; every loop is a
// find or a unite of speckle_union.h, whose descent is argued there.  All atomics are integer minima and integer additions.
//   1. local   one workgroup per tile of TH x TW = 32 x 64 pixels.  Values and a byte (class, valid bit) are staged in LDS -- no
//              halo: a link that leaves the tile is the merge pass's.  A tile row is one wave wide: ONE ballot of "links to its left
//              neighbour" gives every pixel the first pixel of its row run as its parent, without an atomic; then every link down
//              that the links beside it do not imply is one unite on the LDS parent array (ds_min_rtn): one per pair of overlapping
//              runs, not one per pixel.  After a barrier every pixel's root is found into REGISTERS, after another it is
//              written back and counted (ds_add) -- nobody walks the array while it is plainly stored.  To scratch: parent[p] = the
//              image-linear index of p's local root (local row-major order and image order agree inside a tile), -1 on a pixel that
//              is not valid; counts[p] = the local count on a local root, 0 elsewhere -- every element of both is written.
//   2. merge   one thread per pixel pair across a tile boundary (bottom row / right column of a tile and its neighbour in the next
//              tile): if the pair links, the two are united in the global parent array.  The loads of its find loops are relaxed
//              agent-scope atomic loads (they bypass L1 and cannot be hoisted), the link is an agent-scope atomicMin whose returned
//              value decides everything: a stale ancestor is still an ancestor, so no hand-off inside the launch is needed.
//   3. fold    every local root p with counts[p] > 0 whose final root r is another pixel adds counts[p] to counts[r]: one add per
//              local root and tile, not one per pixel.  Only final roots receive adds and no thread uses a final root's count in
//              this launch, so every value that is used is final.  The same thread puts p directly under r (atomicMin again).
//   4. apply   per row-quad, coalesced: r = find(parent[p]) -- parent is read-only by now: plain loads, two steps -- and size =
//              counts[r]; writes the outputs that were asked for into their own buffers.  It reads nothing of the disparity but
//              d[p] for p: out_disparity may be the input.
// LDS of the local pass: 2048 x (4 + 4 + 4 + 1) bytes + 32 row masks = 26.3 KB.  Nothing here allocates, copies or synchronises, and
// nothing comes back to the host.
#include "common.h"
#include "refine_class.h"
#include "speckle_union.h"
#include "stream.h"

namespace {

using namespace ss::stream;    // BLOCK, load4, store4, row_quad
using ss::metrics::LT_F32;     // label sources: the codes of every label_dtype
using ss::metrics::LT_I64;
using ss::refine::NCLS;
using ss::refine::classes4;
using ss::speckle::find;
using ss::speckle::unite;

constexpr int TH = 32, TW = 64;          // pixels of a tile (semstereo_amd/refine.py: SPECKLE_TILE)
constexpr int TP = TH * TW;              // ... 2048: two row-quads per lane
constexpr int QPT = TP / 4 / BLOCK;      // row-quads of a lane
constexpr int QX = TW / 4;               // row-quads of a tile row
constexpr int RPW = TH / 4;              // tile rows of a wave in the union passes: a wave holds a row, lane = column
constexpr int GV = 2048;                 // workgroups of a pass
constexpr int VALID = 16;                // the valid bit of a pixel's byte; bits 0-3 the class
static_assert(QPT * 4 * BLOCK == TP && TW == ss::kWave && RPW * 4 == TH, "a lane owns whole row-quads; a wave holds a tile row");

typedef unsigned char u8;

struct SpeckleArgs {
    const float* disp;         // [B,H,W] contiguous
    const void* label;         // pixel (b, y, x) at b * y_img + y * y_row + x, or null
    const u8* where;           // [B,H,W], or null
    int* parent;               // scratch [B,H,W]: image-linear index of an ancestor, -1 on a pixel that is not valid
    int* counts;               // scratch [B,H,W]
    float* out;                // [B,H,W], or null
    u8* speckle;               // [B,H,W], or null
    int* size;                 // [B,H,W], or null
    int* component;            // [B,H,W], or null
    long long y_row, y_img;
    float lo, hi, max_diff, fill;
    int label_dtype;
    int B, H, W;
    unsigned tiles_y, tiles_x; // per image
    int class_mask;            // 15 with same_class, 0 without: the bits of a pixel's byte two linked pixels agree in
    int max_size;
};

// the parents of a tile, in LDS: workgroup scope
struct TileParents {
    typedef int __attribute__((address_space(3))) * lds_int;
    lds_int p;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ int fetch_min(int i, int v) const {
        return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};
// the parents of an image while other workgroups unite in it: agent scope, never from L1
struct ImageParents {
    int* p;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int fetch_min(int i, int v) const {
        return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
// ... and once the merge launch has ended: read-only (a view without fetch_min cannot be handed to unite)
struct FinalParents {
    const int* p;
    __device__ __forceinline__ int load(int i) const { return p[i]; }
};

// link(p, q) of two 4-neighbours, from their values and bytes: both valid, the same class (or none asked), |d[p] - d[q]| <= max_diff
// with the difference rounded once (a NaN difference, inf - inf, links nothing)
__device__ __forceinline__ bool links(float va, int fa, float vb, int fb, int class_mask, float max_diff) {
    return ((fa & fb & VALID) != 0) & (((fa ^ fb) & class_mask) == 0) & (fabsf(ss::sub_rn(va, vb)) <= max_diff);
}

__device__ __forceinline__ void load_ints(const int* p, int nv, int (&v)[4]) {
    if (nv == 4 && aligned_to(p, 16)) {
        const int4 q = *reinterpret_cast<const int4*>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[j] : 0;
    }
}
__device__ __forceinline__ void store_bytes(u8* p, int nv, const int (&v)[4]) {
    if (nv == 4 && aligned_to(p, 4)) {
        *reinterpret_cast<unsigned*>(p) = (unsigned)v[0] | (unsigned)v[1] << 8 | (unsigned)v[2] << 16 | (unsigned)v[3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) p[j] = (u8)v[j];
    }
}

// the byte of ONE pixel of value v, its label at element offset o of the label map
__device__ __forceinline__ int byte_of(const SpeckleArgs& a, float v, long long o) {
    int cls[4] = {NCLS, NCLS, NCLS, NCLS};
    if (a.label) classes4(a.label, a.label_dtype, o, 1, cls);
    const bool valid = (v >= a.lo) & (v < a.hi);                                                    // (a NaN fails both)
    return cls[0] | (valid ? VALID : 0);
}

// 1 ---- the components of every tile
__global__ __launch_bounds__(BLOCK) void speckle_local_k(SpeckleArgs a) {
    __shared__ __attribute__((aligned(16))) float val[TP];
    __shared__ __attribute__((aligned(16))) int par[TP];
    __shared__ __attribute__((aligned(16))) int cnt[TP];
    __shared__ __attribute__((aligned(16))) u8 flag[TP];
    __shared__ unsigned long long run[TH];             // per tile row: bit x set = pixel x links to pixel x - 1
    const TileParents tile{(TileParents::lds_int)par};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = a.H, W = a.W;
    const unsigned per_image = a.tiles_y * a.tiles_x, tiles = (unsigned)a.B * per_image;
    for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
        const unsigned b = t / per_image, in_image = t - b * per_image, tile_y = in_image / a.tiles_x;
        const int y0 = (int)tile_y * TH, x0 = (int)(in_image - tile_y * a.tiles_x) * TW;
        const long long base = (long long)b * H * W, ybase = (long long)b * a.y_img;
        // the tile: a pixel off the image is staged as not valid and links nothing
#pragma unroll
        for (int k = 0; k < QPT; ++k) {
            const int q = (int)threadIdx.x + k * BLOCK, ly = q / QX, lx = 4 * (q - ly * QX);
            const int y = y0 + ly, x = x0 + lx;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            int cls[4] = {NCLS, NCLS, NCLS, NCLS};
            int nv = 0;
            if (y < H && x < W) {
                const int left = W - x;
                nv = left < 4 ? left : 4;
                load4(a.disp + base + (long long)y * W + x, nv, v);
                if (a.label) classes4(a.label, a.label_dtype, ybase + (long long)y * a.y_row + x, nv, cls);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int l = ly * TW + lx + j;
                const bool valid = (j < nv) & (v[j] >= a.lo) & (v[j] < a.hi);
                val[l] = v[j];
                flag[l] = (u8)((j < nv ? cls[j] : NCLS) | (valid ? VALID : 0));
            }
        }
        __syncthreads();
        // the runs of every row, without an atomic: a wave holds a tile row, lane = column.  One ballot of "links to its left
        // neighbour" names every run, and a pixel starts under the first pixel of its run: the highest clear bit at or below its own.
#pragma unroll
        for (int k = 0; k < RPW; ++k) {
            const int row = wave + 4 * k, l = row * TW + lane, lp = lane > 0 ? l - 1 : l;
            const bool left = lane > 0 && links(val[l], flag[l], val[lp], flag[lp], a.class_mask, a.max_diff);
            const unsigned long long m = __ballot(left);
            const unsigned long long starts = ~m & ((2ull << lane) - 1ull);          // (lane 63: 2 << 63 is 0, all bits; bit 0 is always set)
            par[l] = row * TW + 63 - __builtin_clzll(starts);
            cnt[l] = 0;
            if (lane == 0) run[row] = m;
        }
        __syncthreads();
        // one unite per link down that no link beside it implies: where (x - 1) links down too and both rows run on from x - 1 to x,
        // the two runs are already one through that link.  The leftmost link of such a stretch is never skipped.
#pragma unroll
        for (int k = 0; k < RPW; ++k) {
            const int row = wave + 4 * k, l = row * TW + lane;
            if (row < TH - 1) {                                                       // (the same for a whole wave)
                const bool down = links(val[l], flag[l], val[l + TW], flag[l + TW], a.class_mask, a.max_diff);
                const unsigned long long dm = __ballot(down), implied = run[row] & run[row + 1] & (dm << 1);
                if (((dm & ~implied) >> lane) & 1ull) unite(tile, l, l + TW);
            }
        }
        __syncthreads();
        // every pixel's root, into registers: the array is only read here ...
        int root[RPW];
#pragma unroll
        for (int k = 0; k < RPW; ++k) root[k] = find(tile, (wave + 4 * k) * TW + lane);
        __syncthreads();
        // ... and only written here, with the count of every root
#pragma unroll
        for (int k = 0; k < RPW; ++k) {
            const int l = (wave + 4 * k) * TW + lane;
            par[l] = root[k];
            if (flag[l] & VALID) atomicAdd(&cnt[root[k]], 1);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < QPT; ++k) {
            const int q = (int)threadIdx.x + k * BLOCK, ly = q / QX, lx = 4 * (q - ly * QX);
            const int y = y0 + ly, x = x0 + lx;
            if (y < H && x < W) {
                const int left = W - x, nv = left < 4 ? left : 4;
                int up[4], n[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int l = ly * TW + lx + j, r = par[l];
                    const bool valid = (flag[l] & VALID) != 0;
                    up[j] = valid ? (y0 + r / TW) * W + x0 + (r & (TW - 1)) : -1;
                    n[j] = (valid && r == l) ? cnt[l] : 0;
                }
                const long long o = base + (long long)y * W + x;
                store4(a.parent + o, nv, up);
                store4(a.counts + o, nv, n);
            }
        }
        __syncthreads();               // (the next tile's staging)
    }
}

// 2 ---- the links across tile boundaries.  Per image (tiles_y - 1) * W pairs (y, x) - (y + 1, x) under a tile's bottom row, then
// (tiles_x - 1) * H pairs (y, x) - (y, x + 1) beside a tile's right column.  A link is skipped where the pair before it along the
// boundary (one column to the left; one row up) links too, lies in the SAME two tiles and is linked to this pair on both sides: those
// two side links are inside a tile and the local pass has united them, so this link adds nothing.  The first pair of a tile edge has
// no such pair before it and is never skipped (around a tile corner each of the four pairs is the first of its edge, or follows one
// of its own edge only), so every stretch of links along an edge is united through its first pair.
__global__ __launch_bounds__(BLOCK) void speckle_merge_k(SpeckleArgs a, unsigned below, unsigned per_image, unsigned items) {
    const int H = a.H, W = a.W;
    for (unsigned i = blockIdx.x * BLOCK + threadIdx.x; i < items; i += gridDim.x * BLOCK) {
        const unsigned b = i / per_image, r = i - b * per_image;
        int y, x, y2, x2, back_y, back_x;                     // the pair, and the step to the pair before it along the boundary
        bool has_before;
        if (r < below) {
            const unsigned k = r / (unsigned)W;
            x = x2 = (int)(r - k * (unsigned)W), y = (int)(k + 1) * TH - 1, y2 = y + 1;
            back_y = 0, back_x = 1, has_before = (x & (TW - 1)) != 0;
        } else {
            const unsigned s = r - below, k = s / (unsigned)H;
            y = y2 = (int)(s - k * (unsigned)H), x = (int)(k + 1) * TW - 1, x2 = x + 1;
            back_y = 1, back_x = 0, has_before = (y & (TH - 1)) != 0;
        }
        const long long base = (long long)b * H * W, ybase = (long long)b * a.y_img;
        const int p = y * W + x, q = y2 * W + x2;
        const float vp = a.disp[base + p], vq = a.disp[base + q];
        const int fp = byte_of(a, vp, ybase + (long long)y * a.y_row + x), fq = byte_of(a, vq, ybase + (long long)y2 * a.y_row + x2);
        if (!links(vp, fp, vq, fq, a.class_mask, a.max_diff)) continue;
        if (has_before) {
            const int pb = p - back_y * W - back_x, qb = q - back_y * W - back_x;
            const float vpb = a.disp[base + pb], vqb = a.disp[base + qb];
            const int fpb = byte_of(a, vpb, ybase + (long long)(y - back_y) * a.y_row + x - back_x);
            const int fqb = byte_of(a, vqb, ybase + (long long)(y2 - back_y) * a.y_row + x2 - back_x);
            if (links(vpb, fpb, vqb, fqb, a.class_mask, a.max_diff) && links(vpb, fpb, vp, fp, a.class_mask, a.max_diff) &&
                links(vqb, fqb, vq, fq, a.class_mask, a.max_diff))
                continue;
        }
        unite(ImageParents{a.parent + base}, p, q);
    }
}

// 3 ---- the counts of the local roots, added up on the final roots; and a local root is put directly under its final root (an
// atomicMin with an element of its own set, as everywhere: other threads of this launch walk the array, so its loads are the merge
// pass's), which leaves the last pass two steps to any root instead of a chain of tile roots
__global__ __launch_bounds__(BLOCK) void speckle_fold_k(SpeckleArgs a, unsigned quads, long long n) {
    const long long HW = (long long)a.H * a.W;
    for (unsigned q = blockIdx.x * BLOCK + threadIdx.x; q < quads; q += gridDim.x * BLOCK) {
        const long long i0 = 4ll * q, left = n - i0;
        int c[4];
        load_ints(a.counts + i0, left < 4 ? (int)left : 4, c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (c[j] > 0) {                                  // a local root (never a pixel past the end: those read as 0)
                const long long b = (i0 + j) / HW;
                const ImageParents image{a.parent + b * HW};
                const int p = (int)(i0 + j - b * HW), r = find(image, p);
                if (r != p) {
                    __hip_atomic_fetch_add(a.counts + b * HW + r, c[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    image.fetch_min(p, r);
                }
            }
        }
    }
}

// 4 ---- the outputs
__global__ __launch_bounds__(BLOCK) void speckle_apply_k(SpeckleArgs a, unsigned quads, unsigned QW) {
    const int H = a.H, W = a.W;
    for (unsigned q = blockIdx.x * BLOCK + threadIdx.x; q < quads; q += gridDim.x * BLOCK) {
        const RowQuad rq = row_quad(q, QW, (unsigned)H, W);
        const long long base = (long long)rq.b * H * W, o = base + (long long)rq.h * W + rq.x0;
        int up[4];
        load_ints(a.parent + o, rq.nv, up);
        u8 on[4] = {1, 1, 1, 1};
        if (a.where) load4(a.where + o, rq.nv, on);
        int comp[4], size[4], gone[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool valid = j < rq.nv && up[j] >= 0;
            comp[j] = valid ? find(FinalParents{a.parent + base}, up[j]) : -1;
            size[j] = valid ? a.counts[base + comp[j]] : 0;
            gone[j] = (valid && size[j] <= a.max_size && on[j] != 0) ? 1 : 0;
        }
        if (a.out) {
            float v[4];
            load4(a.disp + o, rq.nv, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = gone[j] ? a.fill : v[j];
            store4(a.out + o, rq.nv, v);
        }
        if (a.speckle) store_bytes(a.speckle + o, rq.nv, gone);
        if (a.size) store4(a.size + o, rq.nv, size);
        if (a.component) store4(a.component + o, rq.nv, comp);
    }
}

// bytes of one scratch plane of n ints, a multiple of 16
inline long long plane_bytes(long long n) { return (4 * n + 15) / 16 * 16; }

}  // namespace

extern "C" int ss_disparity_speckle_scratch(int B, int H, int W, long long* bytes) {
    SS_REQUIRE(bytes && B > 0 && H > 0 && W > 0);
    const long long n = (long long)B * H * W;
    if (n >= (1ll << 31)) return SS_ERR_UNSUPPORTED;
    *bytes = 2 * plane_bytes(n);
    return SS_OK;
}

extern "C" int ss_disparity_speckle_fwd(const float* disparity, const void* label, int label_dtype, long long label_row_stride,
                                        long long label_image_stride, const unsigned char* where, int B, int H, int W, float lo, float hi,
                                        float max_diff, int max_size, int same_class, float fill_value, void* scratch,
                                        long long scratch_bytes, float* out_disparity, unsigned char* out_speckle, int* out_size,
                                        int* out_component, ss_stream_t stream) {
    SS_REQUIRE(disparity && scratch && (out_disparity || out_speckle || out_size || out_component));
    SS_REQUIRE(B > 0 && H > 0 && W > 0);
    if (label) {
        SS_REQUIRE(label_dtype >= LT_I64 && label_dtype <= LT_F32);
        SS_REQUIRE(label_row_stride >= W && label_image_stride >= (long long)(H - 1) * label_row_stride + W);
    }
    SS_REQUIRE(lo < hi);                                   // (false for a NaN)
    SS_REQUIRE(max_diff >= 0.f && max_size >= 0 && (same_class == 0 || same_class == 1));
    const long long n = (long long)B * H * W;
    if (n >= (1ll << 31)) return SS_ERR_UNSUPPORTED;
    SS_REQUIRE(aligned16(scratch) && scratch_bytes >= 2 * plane_bytes(n));
    const unsigned tiles_y = (unsigned)ss::ceil_div(H, TH), tiles_x = (unsigned)ss::ceil_div(W, TW);
    int* parent = static_cast<int*>(scratch);
    int* counts = reinterpret_cast<int*>(static_cast<char*>(scratch) + plane_bytes(n));
    const SpeckleArgs a{disparity, label, where, parent, counts, out_disparity, out_speckle, out_size, out_component, label_row_stride,
                        label_image_stride, lo, hi, max_diff, fill_value, label_dtype, B, H, W, tiles_y, tiles_x, same_class ? 15 : 0,
                        max_size};
    hipStream_t st = ss::as_stream(stream);
    const long long tiles = (long long)B * tiles_y * tiles_x;
    hipLaunchKernelGGL(speckle_local_k, dim3((unsigned)(tiles < GV ? tiles : GV)), dim3(BLOCK), 0, st, a);
    const long long below = (long long)(tiles_y - 1) * W, per_image = below + (long long)(tiles_x - 1) * H, items = per_image * B;
    if (items > 0)                                         // (below 2 n: both fit 32 bits)
        hipLaunchKernelGGL(speckle_merge_k, dim3(grid_for(items, GV)), dim3(BLOCK), 0, st, a, (unsigned)below, (unsigned)per_image,
                           (unsigned)items);
    const long long flat = ss::ceil_div_ll(n, 4);
    if (items > 0) hipLaunchKernelGGL(speckle_fold_k, dim3(grid_for(flat, GV)), dim3(BLOCK), 0, st, a, (unsigned)flat, n);
    const unsigned QW = (unsigned)ss::ceil_div(W, 4);
    const long long quads = (long long)B * H * QW;
    hipLaunchKernelGGL(speckle_apply_k, dim3(grid_for(quads, GV)), dim3(BLOCK), 0, st, a, (unsigned)quads, QW);
    return ss::check_launch();
}
