// What the two fill kernels share (disparity_refine.hip: along rows; disparity_fill2d.hip: along rows and columns): the byte of a
// pixel and the choice between two candidates -- ONE definition each (include/semstereo_hip.h, "disparity refinement": candidates,
// choice), so the two-axis fill can never differ from the row fill in what it finds along a row.  Steps 2 and 3, the candidates of a
// row, are refine_rows_steps.inc: program text that both kernels include.
#pragma once
#include "common.h"
#include "refine_class.h"
#include "stream.h"

namespace ss {
namespace refine {

constexpr int SRC = 16;                  // the source bit of a pixel's byte; bits 0-3 the class, NCLS for none
constexpr int NOCOL = 0xFFFF;            // no candidate (W, H <= 8192 < 0xFFFF): columns and rows travel as 16-bit values
constexpr int SCRATCH = 48;              // ints of scan scratch: 4 waves x 9 values, each wave's rounded up to 12

// of two candidates a (earlier in the order L, R, U, D) and b with values va, vb and distances ga, gb: b wins
__device__ __forceinline__ bool later_wins(float va, int ga, float vb, int gb, int prefer) {
    return prefer == 0 ? (vb < va) | ((vb == va) & (gb < ga))        // background: the smaller disparity
                       : (gb < ga) | ((gb == ga) & (vb < va));       // nearest
}

// the candidate of a tier that wins at position x of a line (a row: stride 1; a column: stride W): L, R positions or NOCOL; -1 if
// neither lies within max_gap.  d: element 0 of the line.
__device__ __forceinline__ int choose(int x, int L, int R, const float* d, int max_gap, int prefer, int stride = 1) {
    const bool hasL = L != NOCOL && x - L <= max_gap, hasR = R != NOCOL && R - x <= max_gap;
    if (!(hasL && hasR)) return hasL ? L : (hasR ? R : -1);
    return later_wins(d[L * stride], x - L, d[R * stride], R - x, prefer) ? R : L;
}

// the four 16-bit values of two words
__device__ __forceinline__ void halves4(unsigned a, unsigned b, int (&v)[4]) {
    v[0] = (int)(a & 0xFFFFu), v[1] = (int)(a >> 16), v[2] = (int)(b & 0xFFFFu), v[3] = (int)(b >> 16);
}

}  // namespace refine
}  // namespace ss
