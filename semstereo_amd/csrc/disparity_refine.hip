// Disparity refinement: the left-right check followed by a hole fill that takes a hole's value from the surface it belongs to -- the
// nearest kept pixel of the SAME predicted class in its row, left or right -- and only then from any class.  The definitions (source,
// class, candidates, tiers, choice, outputs) are written once, in include/semstereo_hip.h, section "disparity refinement"; the
// consistency term is right_view.h's lr_diff, the function ss_lr_consistency_fwd runs.  Nothing is interpolated: every output is a
// selection, one subtraction or a comparison, so the PyTorch composition of semstereo_amd/refine.py gives the same bits.
//
// One workgroup per row, grid-stride over the B * H rows; a kernel of the stream.h family (BLOCK threads, 64-bit element offsets).  With
// chunk = ceil(W / BLOCK) rounded up to 4 and Wp = chunk * BLOCK >= W columns:
//   1. a coalesced row-quad pass computes source and class of every pixel (the right map's value is a scalar gather) and packs them
//      into one byte per pixel: bits 0-3 the class, 8 for none; bit 4 source.  Columns W .. Wp - 1 are "none, no source".
//   2. (steps 2 and 3 are refine_rows_steps.inc and the choice is refine_rows.h's: disparity_fill2d.hip runs the same text)
//      thread t owns columns [t * chunk, (t + 1) * chunk).  It reduces them to the last source column per class and of any class
//      (9 registers), an exclusive maximum scan over the threads (stream.h: block_scan_exclusive) carries those across the row, and a
//      sweep over the chunk writes, per pixel, the left candidate of its own class and of any class as 16-bit columns (0xFFFF: none):
//      one 16-byte word per 4 pixels.
//   3. the mirror image: a minimum scan from the right gives the right candidates.
//   4. a coalesced row-quad pass applies max_gap, the tiers and the choice, gathers d[x*] from the row just read and stores.
// LDS: 192 bytes of scan scratch + 9 bytes per column, 73.9 KB at W = 8192: two workgroups per CU.  In steps 2 and 3 a thread's
// accesses are a chunk apart from its neighbour's: conflict-free at chunk 4, several lanes on a bank from chunk 8 on.  Storing the
// chunks 4 columns apart removed most of those conflicts at W = 4096 and made the kernel SLOWER (the larger row costs a resident
// workgroup, and the kernel waits on memory, not on the LDS: profiles/EXPERIMENTS.md part AC), so the rows are stored plainly.
// Every LDS word is written by one thread per step and the scans are integer maxima and minima: two calls give the same bits.
// Nothing here allocates, copies or synchronises, and nothing comes back to the host.
#include "common.h"
#include "metrics_decode.h"
#include "refine_class.h"
#include "refine_rows.h"
#include "right_view.h"
#include "stream.h"

namespace {

using namespace ss::stream;    // BLOCK, RowQuad, load4, store4, block_scan_exclusive
using ss::metrics::LT_I64;     // label sources: the codes of every label_dtype
using ss::metrics::LT_F32;
using ss::refine::NCLS;        // classes 0 .. 7; NCLS itself stands for "none" (refine_class.h: class_of, classes4)
using ss::refine::classes4;
using ss::refine::NOCOL;        // refine_rows.h: the byte of a pixel, the choice
using ss::refine::SCRATCH;
using ss::refine::SRC;
using ss::refine::choose;
using ss::rview::MAX_W;
using ss::rview::lr_diff;
using ss::rview::map_shape;

constexpr int GV = 2048;                 // workgroups of a pass

typedef unsigned char u8;

struct RefineArgs {
    const float* disp;         // [B,H,W] contiguous
    const float* disp_right;   // [B,H,W], or null
    const u8* keep;            // [B,H,W], or null
    const void* label;         // pixel (b, h, x) at b * y_img + h * y_row + x, or null
    float* out;                // [B,H,W] each, or null
    u8* kind;
    int* source;
    u8* consistent;
    long long y_row, y_img;
    float lo, hi, threshold, fill;
    int label_dtype;
    int B, H, W, chunk;        // chunk: the columns of a thread in steps 2 and 3
    int max_gap, prefer, fallback;
};

// dynamic LDS: SCRATCH ints; the candidates, left then right, one 16-byte word per 4 columns (own-class x 4, any-class x 4 as 16-bit
// columns): 2 x Wp / 4 words; Wp bytes
__global__ __launch_bounds__(BLOCK) void disparity_refine_k(RefineArgs a) {
    extern __shared__ __attribute__((aligned(16))) int smem[];
    const int W = a.W, chunk = a.chunk, Wp = chunk * BLOCK, QR = Wp / 4;
    int* scratch = smem;
    uint4* cand = reinterpret_cast<uint4*>(smem + SCRATCH);
    u8* flag = reinterpret_cast<u8*>(cand + 2 * QR);
    const unsigned rows = (unsigned)a.B * (unsigned)a.H;
    const int c0 = threadIdx.x * chunk;            // the chunk of steps 2 and 3
    for (unsigned row = blockIdx.x; row < rows; row += gridDim.x) {
        const unsigned b = row / (unsigned)a.H, h = row - b * (unsigned)a.H;
        const long long base = (long long)row * W;
        const long long ybase = (long long)b * a.y_img + (long long)h * a.y_row;
        const float* d = a.disp + base;
        // 1 ---- source and class, one byte per pixel
        for (int x0 = threadIdx.x * 4; x0 < Wp; x0 += BLOCK * 4) {
            unsigned packed = NCLS * 0x01010101u;
            if (x0 < W) {
                const int left = W - x0, nv = left < 4 ? left : 4;
                float v[4], ok[4];
                int cls[4] = {NCLS, NCLS, NCLS, NCLS};
                u8 kp[4] = {1, 1, 1, 1};
                load4(d + x0, nv, v);
                if (a.keep) load4(a.keep + base + x0, nv, kp);
                if (a.label) classes4(a.label, a.label_dtype, ybase + x0, nv, cls);
                packed = 0u;
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
            }
            *reinterpret_cast<unsigned*>(flag + x0) = packed;
        }
        __syncthreads();
#include "refine_rows_steps.inc"       // 2, 3 ---- the left and the right candidates
        __syncthreads();
        // 4 ---- max_gap, the tiers, the choice; the outputs
        if (a.out || a.kind || a.source) {
            for (int x0 = threadIdx.x * 4; x0 < W; x0 += BLOCK * 4) {
                const int left = W - x0, nv = left < 4 ? left : 4;
                const unsigned f4 = *reinterpret_cast<const unsigned*>(flag + x0);
                const uint4 l4 = cand[x0 >> 2], r4 = cand[QR + (x0 >> 2)];
                const int lown[4] = {(int)(l4.x & 0xFFFFu), (int)(l4.x >> 16), (int)(l4.y & 0xFFFFu), (int)(l4.y >> 16)};
                const int lany[4] = {(int)(l4.z & 0xFFFFu), (int)(l4.z >> 16), (int)(l4.w & 0xFFFFu), (int)(l4.w >> 16)};
                const int rown[4] = {(int)(r4.x & 0xFFFFu), (int)(r4.x >> 16), (int)(r4.y & 0xFFFFu), (int)(r4.y >> 16)};
                const int rany[4] = {(int)(r4.z & 0xFFFFu), (int)(r4.z >> 16), (int)(r4.w & 0xFFFFu), (int)(r4.w >> 16)};
                float v[4], kd[4];
                int s[4];
                load4(d + x0, nv, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int f = (int)((f4 >> (8 * j)) & 255u), x = x0 + j;
                    s[j] = x, kd[j] = 0.f;
                    if (!(f & SRC) && j < nv) {
                        s[j] = (f & 15) < NCLS ? choose(x, lown[j], rown[j], d, a.max_gap, a.prefer) : -1;
                        kd[j] = 1.f;
                        if (s[j] < 0 && a.fallback) s[j] = choose(x, lany[j], rany[j], d, a.max_gap, a.prefer), kd[j] = 2.f;
                        if (s[j] < 0) kd[j] = 3.f;
                        v[j] = s[j] >= 0 ? d[s[j]] : a.fill;
                    }
                }
                if (a.out) store4(a.out + base + x0, nv, v);
                if (a.kind) store4(a.kind + base + x0, nv, kd);
                if (a.source) store4(a.source + base + x0, nv, s);
            }
        }
        __syncthreads();               // (the next row's bytes)
    }
}

}  // namespace

extern "C" int ss_disparity_refine_fwd(const float* disparity, const float* disparity_right, const unsigned char* keep, const void* label,
                                       int label_dtype, long long label_row_stride, long long label_image_stride, int B, int H, int W,
                                       float lo, float hi, float threshold, int max_gap, int prefer, int fallback, float fill_value,
                                       float* out_disparity, unsigned char* kind, int* source, unsigned char* consistent,
                                       ss_stream_t stream) {
    SS_REQUIRE(disparity && B > 0 && H > 0 && W > 0);
    SS_REQUIRE(out_disparity || kind || source || consistent);
    SS_REQUIRE(disparity_right || !consistent);
    if (label) {
        SS_REQUIRE(label_dtype >= LT_I64 && label_dtype <= LT_F32);
        SS_REQUIRE(label_row_stride >= W && label_image_stride >= (long long)(H - 1) * label_row_stride + W);
    }
    SS_REQUIRE(lo < hi);                                   // (false for a NaN)
    SS_REQUIRE(!disparity_right || threshold >= 0.f);      // (false for a NaN)
    SS_REQUIRE(max_gap >= 1 && (prefer == 0 || prefer == 1) && (fallback == 0 || fallback == 1));
    if (W > MAX_W) return SS_ERR_UNSUPPORTED;
    if (int s = map_shape(B, H, W)) return s;
    const int chunk = (ss::ceil_div(W, BLOCK) + 3) / 4 * 4;
    RefineArgs a{disparity, disparity_right, keep, label, out_disparity, kind, source, consistent, label_row_stride, label_image_stride,
                 lo, hi, threshold, fill_value, label_dtype, B, H, W, chunk, max_gap, prefer, fallback};
    const size_t lds = SCRATCH * sizeof(int) + (size_t)chunk * BLOCK * 9;
    if (ss::ensure_dynamic_lds(reinterpret_cast<const void*>(disparity_refine_k), (int)lds) != SS_OK) return SS_ERR_LAUNCH;
    const long long rows = (long long)B * H;
    hipLaunchKernelGGL(disparity_refine_k, dim3((unsigned)(rows < GV ? rows : GV)), dim3(BLOCK), lds, ss::as_stream(stream), a);
    return ss::check_launch();
}
