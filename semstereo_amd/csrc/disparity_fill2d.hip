// Disparity refinement, the fill along rows AND columns: a hole takes its value from the nearest source of its own class to its left,
// to its right, above or below it, and only then from any class.  The definitions (candidates L, R, U, D, the two gaps, the tiers, the
// four-way choice, the outputs) are written once, in include/semstereo_hip.h, section "disparity refinement: fill along rows and
// columns"; source, class and the consistency term are the row fill's (disparity_refine.hip, right_view.h's lr_diff).  Nothing is
// interpolated: every output is a selection or a comparison, so the PyTorch composition of semstereo_amd/refine.py gives the same bits.
//
// The first scan of this family that runs ACROSS rows.  One workgroup per column would leave the chip idle (1024 columns are 16
// waves), so the column scan is decomposed: reduce per segment, scan the segments' summaries, sweep per segment -- four launches on
// the caller's stream, none waiting on another workgroup: no cooperative launch, no flag, no spin loop.
// A tile is TR x TC = 64 rows x 256 columns (semstereo_amd/refine.py: FILL2D_TILE): a thread owns 4 adjacent columns -- one 32-bit
// word of the pixels' bytes, a wave 256 bytes of a row -- and each of the 4 waves 16 rows, whose 16 words it keeps in registers.
//   1. classify   per tile: the row kernel's byte of every pixel (bits 0-3 the class, 8 for none; bit 4 source) to the flag plane, and
//                 `consistent`; per column the last and the first source row of each class and of any class in the tile's 64 rows
//                 (9 + 9 values as 16-bit rows, 0xFFFF for none), the four waves' combined through LDS, to the summaries.
//   2. scan       one thread per (image, direction, class, 4 columns) walks the at most 128 segments down (up) and replaces every
//                 summary by the exclusive carry: the nearest source row in the segments above (below).  Tiny; it exists so that
//                 launch 3 reads ONE carry per column and direction.
//   3. sweep      per tile again: the flag words back into registers, the per-wave reduction again, the carry of a wave = the scan's
//                 carry overridden by the waves above (below) it, through LDS; then 16 rows down and 16 rows up, writing per pixel
//                 the candidate rows U and D of its own class and of any class.
//   4. rows       one workgroup per row, as disparity_refine_k: the row's bytes from the flag plane into LDS, steps 2 and 3 of the
//                 row kernel (refine_rows_steps.inc: the very text), then per pixel both gaps, the tiers and the choice: the winner of (L, R)
//                 and the winner of (U, D) by refine_rows.h's choose, then the winner of those two by the same comparison -- the
//                 least of a total order, found as a tournament.  d is gathered at the winner.
// Departures from the shape the design note recommends: launch 3 stages nothing in LDS -- a thread reads exactly the 16 words it
// would have staged, so they stay in registers and LDS holds only the 36 KB of the waves' hand-off; and the candidates are TWO planes
// of 4 bytes per pixel (U: own | any << 16; D likewise), not one of 8, because the down sweep has written U before the up sweep
// starts: a thread-row is one 16-byte store per plane, a wave 1 KB, and nothing is held back for 16 rows.  Launch 1 restates the
// byte of the row kernel's step 1 (that step stays where it is: disparity_refine.hip keeps its own text of the check).
// Scratch: ss_disparity_fill2d_scratch is the one place that knows its size; every byte read is written by the same call first
// (rows are padded to Wp = W rounded up to 4 columns, and all Wp are written).  Selections of integers only, no floating-point
// atomics, no atomics at all: two calls give the same bits.  Nothing here allocates, copies or synchronises, and nothing comes back
// to the host.
#include "common.h"
#include "metrics_decode.h"
#include "refine_class.h"
#include "refine_rows.h"
#include "right_view.h"
#include "stream.h"

namespace {

using namespace ss::stream;    // BLOCK, load4, store4
using ss::metrics::LT_F32;     // label sources: the codes of every label_dtype
using ss::metrics::LT_I64;
using ss::refine::NCLS;
using ss::refine::NOCOL;
using ss::refine::SCRATCH;
using ss::refine::SRC;
using ss::refine::choose;
using ss::refine::classes4;
using ss::refine::halves4;
using ss::refine::later_wins;
using ss::rview::MAX_W;
using ss::rview::lr_diff;
using ss::rview::map_shape;

constexpr int TR = 64, TC = 256;         // rows and columns of a tile (semstereo_amd/refine.py: FILL2D_TILE)
constexpr int RPW = TR / 4;              // rows of a wave
constexpr int MAX_H = 8192;              // rows travel as 16-bit values too
constexpr int GV = 2048;                 // workgroups of the row pass
constexpr int NK = NCLS + 1;             // carried values per column and direction: classes 0 .. 7, any class
constexpr unsigned NONE4 = NCLS * 0x01010101u;       // four pixels of no class that are no sources
static_assert(TC == 4 * ss::kWave && BLOCK == 4 * ss::kWave && RPW * 4 == TR, "a lane owns 4 columns, a wave 16 rows");

typedef unsigned char u8;
typedef unsigned short u16;

struct Fill2dArgs {
    const float* disp;         // [B,H,W] contiguous
    const float* disp_right;   // [B,H,W], or null
    const u8* keep;            // [B,H,W], or null
    const void* label;         // pixel (b, h, x) at b * y_img + h * y_row + x, or null
    u8* flag;                  // scratch [B,H,Wp]: the byte of every pixel
    unsigned* up;              // scratch [B,H,Wp]: U of the own class | U of any class << 16
    unsigned* down;            // scratch [B,H,Wp]: D likewise
    u16* summ;                 // scratch [B,nseg,2,NK,Wp]: last (0) and first (1) source row per segment; after launch 2 the carries
    float* out;                // [B,H,W] each, or null
    u8* kind;
    int* source;
    int* source_row;
    u8* consistent;
    long long y_row, y_img;
    float lo, hi, threshold, fill;
    int label_dtype;
    int B, H, W, Wp, nseg, nstrip, chunk;
    int gap_x, gap_y, prefer, fallback;
};

struct Tile {
    unsigned b, seg, strip;
};
__device__ __forceinline__ Tile tile_of(const Fill2dArgs& a, unsigned t) {
    const unsigned per_image = (unsigned)a.nseg * (unsigned)a.nstrip, b = t / per_image, r = t - b * per_image;
    const unsigned seg = r / (unsigned)a.nstrip;
    return Tile{b, seg, r - seg * (unsigned)a.nstrip};
}

// of two 16-bit halves each: the new value where it is one, the current elsewhere
__device__ __forceinline__ unsigned over16(unsigned cur, unsigned nw) {
    const unsigned lo = (nw & 0xFFFFu) != 0xFFFFu ? (nw & 0xFFFFu) : (cur & 0xFFFFu);
    const unsigned hi = (nw >> 16) != 0xFFFFu ? (nw & 0xFFFF0000u) : (cur & 0xFFFF0000u);
    return lo | hi;
}
__device__ __forceinline__ uint2 over16(uint2 cur, uint2 nw) { return make_uint2(over16(cur.x, nw.x), over16(cur.y, nw.y)); }

// The 16 rows of a wave reduced: v[j][k] = the last (UP: the first) row y0 + r with a source of class k (k = NCLS: of any class) in
// column j of the thread's four, `none` where there is none.
// The passes over a wave's 16 words each decode them anew: without this the compiler keeps every "class == k" mask of one pass
// alive for the next ones, 8 x 4 x 16 wave masks, and spills them.  It emits no instruction.
__device__ __forceinline__ void decode_anew(unsigned (&f)[RPW]) {
#pragma unroll
    for (int r = 0; r < RPW; ++r) asm volatile("" : "+v"(f[r]));
}

template <bool UP>
__device__ __forceinline__ void reduce_rows(const unsigned (&f)[RPW], int y0, int none, int (&v)[4][NK]) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < NK; ++k) v[j][k] = none;
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const int r = UP ? RPW - 1 - i : i, y = y0 + r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int fb = (int)((f[r] >> (8 * j)) & 255u);
            const int c = (fb & SRC) ? (fb & 15) : 15;              // the class a source row is recorded under; 15: no source
            v[j][NCLS] = (fb & SRC) ? y : v[j][NCLS];
#pragma unroll
            for (int k = 0; k < NK - 1; ++k) v[j][k] = c == k ? y : v[j][k];
        }
    }
}

// ... and handed to the other waves: ex[k][lane] = the four columns' values as 16-bit rows (-1 becomes 0xFFFF)
__device__ __forceinline__ void hand_off(const int (&v)[4][NK], uint2 (*ex)[ss::kWave], int lane) {
#pragma unroll
    for (int k = 0; k < NK; ++k)
        ex[k][lane] = make_uint2(((unsigned)v[0][k] & 0xFFFFu) | (unsigned)v[1][k] << 16, ((unsigned)v[2][k] & 0xFFFFu) | (unsigned)v[3][k] << 16);
}

// 1 ---- the byte of every pixel, `consistent`, and the summaries of every tile
__global__ __launch_bounds__(BLOCK) void fill2d_classify_k(Fill2dArgs a) {
    __shared__ uint2 ex[2][4][NK][ss::kWave];            // [direction][wave][value][lane]: 36 KB
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = a.H, W = a.W, Wp = a.Wp;
    const Tile t = tile_of(a, blockIdx.x);
    const int x0 = (int)t.strip * TC + lane * 4, y0 = (int)t.seg * TR + wave * RPW;
    unsigned f[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const int y = y0 + r;
        f[r] = NONE4;
        if (y < H && x0 < W) {
            const long long row = (long long)t.b * H + y, base = row * W;
            const long long ybase = (long long)t.b * a.y_img + (long long)y * a.y_row;
            const int left = W - x0, nv = left < 4 ? left : 4;
            float v[4], ok[4];
            int cls[4] = {NCLS, NCLS, NCLS, NCLS};
            u8 kp[4] = {1, 1, 1, 1};
            load4(a.disp + base + x0, nv, v);
            if (a.keep) load4(a.keep + base + x0, nv, kp);
            if (a.label) classes4(a.label, a.label_dtype, ybase + x0, nv, cls);
            unsigned packed = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bool src = (j < nv) & (v[j] >= a.lo) & (v[j] < a.hi) & (kp[j] != 0);
                ok[j] = 0.f;
                if (a.disp_right && j < nv) {
                    const bool c = lr_diff(x0 + j, v[j], a.disp_right + base, a.lo, a.hi, W) <= a.threshold;
                    ok[j] = c ? 1.f : 0.f;
                    src &= c;
                }
                const unsigned byte = (j < nv ? (unsigned)cls[j] : (unsigned)NCLS) | (src ? (unsigned)SRC : 0u);
                packed |= byte << (8 * j);
            }
            if (a.consistent) store4(a.consistent + base + x0, nv, ok);
            f[r] = packed;
            *reinterpret_cast<unsigned*>(a.flag + row * Wp + x0) = packed;
        }
    }
    if (!a.summ) return;                                 // (only `consistent` was asked for)
    int v[4][NK];
    reduce_rows<false>(f, y0, -1, v);
    hand_off(v, ex[0][wave], lane);
    decode_anew(f);
    reduce_rows<true>(f, y0, NOCOL, v);
    hand_off(v, ex[1][wave], lane);
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * NK * ss::kWave; i += BLOCK) {
        const int dir = i / (NK * ss::kWave), k = (i >> 6) % NK, l = i & 63;
        const int x = (int)t.strip * TC + l * 4;
        if (x >= Wp) continue;
        uint2 s = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
#pragma unroll
        for (int w = 0; w < 4; ++w) s = over16(s, ex[dir][dir ? 3 - w : w][k][l]);        // the last: the lowest wave's; the first: the highest's
        const long long o = ((((long long)t.b * a.nseg + t.seg) * 2 + dir) * NK + k) * Wp + x;
        *reinterpret_cast<uint2*>(a.summ + o) = s;
    }
}

// 2 ---- the summaries of every column turned into exclusive carries, in place
__global__ __launch_bounds__(BLOCK) void fill2d_scan_k(Fill2dArgs a, long long items, unsigned QW) {
    const long long plane = (long long)2 * NK * a.Wp;                                       // u16 elements of a segment
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < items; i += (long long)gridDim.x * BLOCK) {       // (B = 2^30: above 2^32)
        const long long line = i / QW, q = i - line * QW, b = line / (2 * NK), dk = line - b * (2 * NK);        // dk = dir * NK + k
        const bool upward = dk >= NK;
        u16* p = a.summ + b * a.nseg * plane + dk * a.Wp + 4 * q;
        uint2 carry = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        for (int n = 0; n < a.nseg; ++n) {
            uint2* at = reinterpret_cast<uint2*>(p + (long long)(upward ? a.nseg - 1 - n : n) * plane);
            const uint2 own = *at;
            *at = carry;
            carry = over16(carry, own);
        }
    }
}

// 3 ---- the candidate rows of every pixel
__global__ __launch_bounds__(BLOCK) void fill2d_sweep_k(Fill2dArgs a) {
    __shared__ uint2 ex[2][4][NK][ss::kWave];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int H = a.H, Wp = a.Wp;
    const Tile t = tile_of(a, blockIdx.x);
    const int x0 = (int)t.strip * TC + lane * 4, y0 = (int)t.seg * TR + wave * RPW;
    const bool inside = x0 < Wp;
    const long long row0 = (long long)t.b * H + y0;
    unsigned f[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) f[r] = (inside && y0 + r < H) ? *reinterpret_cast<const unsigned*>(a.flag + (row0 + r) * Wp + x0) : NONE4;
    int v[4][NK];
    reduce_rows<false>(f, y0, -1, v);
    hand_off(v, ex[0][wave], lane);
    decode_anew(f);
    reduce_rows<true>(f, y0, NOCOL, v);
    hand_off(v, ex[1][wave], lane);
    __syncthreads();
    const long long carries = (((long long)t.b * a.nseg + t.seg) * 2) * NK * Wp + x0;
    // down: U, the last source row above
    decode_anew(f);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        uint2 c = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        if (inside) c = *reinterpret_cast<const uint2*>(a.summ + carries + (long long)k * Wp);
#pragma unroll
        for (int w = 0; w < 3; ++w)
            if (w < wave) c = over16(c, ex[0][w][k][lane]);
        v[0][k] = (int)(short)(c.x & 0xFFFFu), v[1][k] = (int)(short)(c.x >> 16);           // (0xFFFF becomes -1)
        v[2][k] = (int)(short)(c.y & 0xFFFFu), v[3][k] = (int)(short)(c.y >> 16);
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const int y = y0 + r;
        unsigned word[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int fb = (int)((f[r] >> (8 * j)) & 255u);
            int mine = -1;
#pragma unroll
            for (int k = 0; k < NK - 1; ++k) mine = (fb & 15) == k ? v[j][k] : mine;
            word[j] = ((unsigned)mine & 0xFFFFu) | (unsigned)v[j][NCLS] << 16;
            const int c = (fb & SRC) ? (fb & 15) : 15;              // the class a source row is recorded under; 15: no source
            v[j][NCLS] = (fb & SRC) ? y : v[j][NCLS];
#pragma unroll
            for (int k = 0; k < NK - 1; ++k) v[j][k] = c == k ? y : v[j][k];
        }
        if (inside && y < H) *reinterpret_cast<uint4*>(a.up + (row0 + r) * Wp + x0) = make_uint4(word[0], word[1], word[2], word[3]);
    }
    // up: D, the first source row below
    decode_anew(f);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        uint2 c = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        if (inside) c = *reinterpret_cast<const uint2*>(a.summ + carries + (long long)(NK + k) * Wp);
#pragma unroll
        for (int w = 3; w > 0; --w)
            if (w > wave) c = over16(c, ex[1][w][k][lane]);
        v[0][k] = (int)(c.x & 0xFFFFu), v[1][k] = (int)(c.x >> 16), v[2][k] = (int)(c.y & 0xFFFFu), v[3][k] = (int)(c.y >> 16);
    }
#pragma unroll
    for (int r = RPW - 1; r >= 0; --r) {
        const int y = y0 + r;
        unsigned word[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int fb = (int)((f[r] >> (8 * j)) & 255u);
            int mine = NOCOL;
#pragma unroll
            for (int k = 0; k < NK - 1; ++k) mine = (fb & 15) == k ? v[j][k] : mine;
            word[j] = (unsigned)mine | (unsigned)v[j][NCLS] << 16;
            const int c = (fb & SRC) ? (fb & 15) : 15;              // the class a source row is recorded under; 15: no source
            v[j][NCLS] = (fb & SRC) ? y : v[j][NCLS];
#pragma unroll
            for (int k = 0; k < NK - 1; ++k) v[j][k] = c == k ? y : v[j][k];
        }
        if (inside && y < H) *reinterpret_cast<uint4*>(a.down + (row0 + r) * Wp + x0) = make_uint4(word[0], word[1], word[2], word[3]);
    }
}

// The winner of a tier at pixel (x, y) as its index y* * W + x* in the image, -1 for none.  L, R: columns, U, D: rows, NOCOL for
// none; row: element 0 of the pixel's row, col: element 0 of its column.  (L, R) and (U, D) are each refine_rows.h's choice; the
// two winners meet in the same comparison, the horizontal one being the earlier in the order L, R, U, D.
__device__ __forceinline__ int choose4(int x, int y, int L, int R, int U, int D, const float* row, const float* col, int W, int gap_x,
                                       int gap_y, int prefer) {
    const int hx = choose(x, L, R, row, gap_x, prefer), vy = choose(y, U, D, col, gap_y, prefer, W);
    if (hx < 0 || vy < 0) return hx >= 0 ? y * W + hx : (vy >= 0 ? vy * W + x : -1);
    const int gh = hx < x ? x - hx : hx - x, gv = vy < y ? y - vy : vy - y;
    return later_wins(row[hx], gh, col[vy * W], gv, prefer) ? vy * W + x : y * W + hx;
}

// 4 ---- the row candidates and the choice.  Dynamic LDS as disparity_refine_k's: SCRATCH ints, 2 x Wr / 4 candidate words, Wr bytes,
// with Wr = chunk * BLOCK columns.
__global__ __launch_bounds__(BLOCK) void fill2d_rows_k(Fill2dArgs a) {
    extern __shared__ __attribute__((aligned(16))) int smem[];
    const int W = a.W, H = a.H, Wp = a.Wp, chunk = a.chunk, Wr = chunk * BLOCK, QR = Wr / 4;
    int* scratch = smem;
    uint4* cand = reinterpret_cast<uint4*>(smem + SCRATCH);
    u8* flag = reinterpret_cast<u8*>(cand + 2 * QR);
    const unsigned rows = (unsigned)a.B * (unsigned)H;
    const int c0 = threadIdx.x * chunk;            // the chunk of steps 2 and 3
    for (unsigned row = blockIdx.x; row < rows; row += gridDim.x) {
        const unsigned b = row / (unsigned)H;
        const int h = (int)(row - b * (unsigned)H);
        const long long base = (long long)row * W, pbase = (long long)row * Wp;
        const float* img = a.disp + (long long)b * H * W;
        const float* d = a.disp + base;
        // 1 ---- the row's bytes, as launch 1 wrote them
        for (int x0 = threadIdx.x * 4; x0 < Wr; x0 += BLOCK * 4)
            *reinterpret_cast<unsigned*>(flag + x0) = x0 < W ? *reinterpret_cast<const unsigned*>(a.flag + pbase + x0) : NONE4;
        __syncthreads();
#include "refine_rows_steps.inc"       // 2, 3 ---- the left and the right candidates
        __syncthreads();
        // 4 ---- both gaps, the tiers, the choice; the outputs
        for (int x0 = threadIdx.x * 4; x0 < W; x0 += BLOCK * 4) {
            const int left = W - x0, nv = left < 4 ? left : 4;
            const unsigned f4 = *reinterpret_cast<const unsigned*>(flag + x0);
            const uint4 l4 = cand[x0 >> 2], r4 = cand[QR + (x0 >> 2)];
            const uint4 u4 = *reinterpret_cast<const uint4*>(a.up + pbase + x0), d4 = *reinterpret_cast<const uint4*>(a.down + pbase + x0);
            const unsigned uw[4] = {u4.x, u4.y, u4.z, u4.w}, dw[4] = {d4.x, d4.y, d4.z, d4.w};
            int lown[4], lany[4], rown[4], rany[4];
            halves4(l4.x, l4.y, lown), halves4(l4.z, l4.w, lany), halves4(r4.x, r4.y, rown), halves4(r4.z, r4.w, rany);
            float v[4], kd[4];
            int sx[4], sy[4];
            load4(d + x0, nv, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = (int)((f4 >> (8 * j)) & 255u), x = x0 + j;
                sx[j] = x, sy[j] = h, kd[j] = 0.f;
                if (!(f & SRC) && j < nv) {
                    int s = -1;
                    kd[j] = 1.f;
                    if ((f & 15) < NCLS)
                        s = choose4(x, h, lown[j], rown[j], (int)(uw[j] & 0xFFFFu), (int)(dw[j] & 0xFFFFu), d, img + x, W, a.gap_x, a.gap_y, a.prefer);
                    if (s < 0 && a.fallback)
                        s = choose4(x, h, lany[j], rany[j], (int)(uw[j] >> 16), (int)(dw[j] >> 16), d, img + x, W, a.gap_x, a.gap_y, a.prefer), kd[j] = 2.f;
                    if (s < 0) kd[j] = 3.f;
                    v[j] = s >= 0 ? img[s] : a.fill;
                    sy[j] = s >= 0 ? s / W : -1;
                    sx[j] = s >= 0 ? s - sy[j] * W : -1;
                }
            }
            if (a.out) store4(a.out + base + x0, nv, v);
            if (a.kind) store4(a.kind + base + x0, nv, kd);
            if (a.source) store4(a.source + base + x0, nv, sx);
            if (a.source_row) store4(a.source_row + base + x0, nv, sy);
        }
        __syncthreads();               // (the next row's bytes)
    }
}

inline long long round16(long long bytes) { return (bytes + 15) / 16 * 16; }

// the scratch: the flag plane, the two candidate planes, the summaries
struct Layout {
    int Wp, nseg, nstrip;
    long long flag, plane, summ, total;
};
inline Layout layout(int B, int H, int W) {
    Layout l;
    l.Wp = (W + 3) / 4 * 4, l.nseg = ss::ceil_div(H, TR), l.nstrip = ss::ceil_div(W, TC);
    const long long px = (long long)B * H * l.Wp;
    l.flag = round16(px), l.plane = 4 * px, l.summ = round16((long long)B * l.nseg * 2 * NK * l.Wp * (long long)sizeof(u16));
    l.total = l.flag + 2 * l.plane + l.summ;
    return l;
}

inline int shape(int B, int H, int W) {
    if (W > MAX_W || H > MAX_H) return SS_ERR_UNSUPPORTED;
    return map_shape(B, H, W);
}

}  // namespace

extern "C" int ss_disparity_fill2d_scratch(int B, int H, int W, long long* bytes) {
    SS_REQUIRE(bytes && B > 0 && H > 0 && W > 0);
    if (int s = shape(B, H, W)) return s;
    *bytes = layout(B, H, W).total;
    return SS_OK;
}

extern "C" int ss_disparity_fill2d_fwd(const float* disparity, const float* disparity_right, const unsigned char* keep, const void* label,
                                       int label_dtype, long long label_row_stride, long long label_image_stride, int B, int H, int W,
                                       float lo, float hi, float threshold, int max_gap_x, int max_gap_y, int prefer, int fallback,
                                       float fill_value, void* scratch, long long scratch_bytes, float* out_disparity,
                                       unsigned char* kind, int* source, int* source_row, unsigned char* consistent,
                                       ss_stream_t stream) {
    SS_REQUIRE(disparity && scratch && B > 0 && H > 0 && W > 0);
    SS_REQUIRE(out_disparity || kind || source || source_row || consistent);
    SS_REQUIRE(disparity_right || !consistent);
    if (label) {
        SS_REQUIRE(label_dtype >= LT_I64 && label_dtype <= LT_F32);
        SS_REQUIRE(label_row_stride >= W && label_image_stride >= (long long)(H - 1) * label_row_stride + W);
    }
    SS_REQUIRE(lo < hi);                                   // (false for a NaN)
    SS_REQUIRE(!disparity_right || threshold >= 0.f);      // (false for a NaN)
    SS_REQUIRE(max_gap_x >= 1 && max_gap_y >= 1 && (prefer == 0 || prefer == 1) && (fallback == 0 || fallback == 1));
    if (int s = shape(B, H, W)) return s;
    const Layout l = layout(B, H, W);
    SS_REQUIRE(aligned16(scratch) && scratch_bytes >= l.total);
    const bool fills = out_disparity || kind || source || source_row;
    char* at = static_cast<char*>(scratch);
    const int chunk = (ss::ceil_div(W, BLOCK) + 3) / 4 * 4;
    Fill2dArgs a{disparity, disparity_right, keep, label, reinterpret_cast<u8*>(at), reinterpret_cast<unsigned*>(at + l.flag),
                 reinterpret_cast<unsigned*>(at + l.flag + l.plane), fills ? reinterpret_cast<u16*>(at + l.flag + 2 * l.plane) : nullptr,
                 out_disparity, kind, source, source_row, consistent, label_row_stride, label_image_stride, lo, hi, threshold,
                 fill_value, label_dtype, B, H, W, l.Wp, l.nseg, l.nstrip, chunk, max_gap_x, max_gap_y, prefer, fallback};
    const size_t lds = SCRATCH * sizeof(int) + (size_t)chunk * BLOCK * 9;
    if (fills && ss::ensure_dynamic_lds(reinterpret_cast<const void*>(fill2d_rows_k), (int)lds) != SS_OK) return SS_ERR_LAUNCH;
    hipStream_t st = ss::as_stream(stream);
    const unsigned tiles = (unsigned)((long long)B * l.nseg * l.nstrip);                   // (at most one per pixel: below 2^31)
    hipLaunchKernelGGL(fill2d_classify_k, dim3(tiles), dim3(BLOCK), 0, st, a);
    if (!fills) return ss::check_launch();
    const unsigned QW = (unsigned)(l.Wp / 4);
    const long long items = (long long)B * 2 * NK * QW;
    hipLaunchKernelGGL(fill2d_scan_k, dim3(grid_for(items, GV)), dim3(BLOCK), 0, st, a, items, QW);
    hipLaunchKernelGGL(fill2d_sweep_k, dim3(tiles), dim3(BLOCK), 0, st, a);
    const long long rows = (long long)B * H;
    hipLaunchKernelGGL(fill2d_rows_k, dim3((unsigned)(rows < GV ? rows : GV)), dim3(BLOCK), lds, st, a);
    return ss::check_launch();
}
