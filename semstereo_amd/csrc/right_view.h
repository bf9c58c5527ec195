// What right_view.hip, disparity_refine.hip and disparity_fill2d.hip share: where a left pixel lands in the right view and the left-right difference of two
// estimates -- ONE definition each (include/semstereo_hip.h, "right-view ground truth"), so the check inside the refinement can never
// differ from ss_lr_consistency_fwd's -- and the limits of the row kernels.
#pragma once
#include "common.h"

namespace ss {
namespace rview {

constexpr int MAX_W = 8192;              // widest row of the one-workgroup-per-row kernels

// the right column a left pixel x with disparity d lands on, or -1
__device__ __forceinline__ int target(int x, float d, float lo, float hi, int W) {
    const float t = rintf(ss::sub_rn((float)x, d));
    const bool lands = (d >= lo) & (d < hi) & (t >= 0.f) & (t < (float)W);       // (NaN fails the first two; -0 passes the third)
    return lands ? (int)t : -1;
}

// diff[x] of the consistency check: |v - dr[t(x)]| in fp32 where x lands and dr[t] is valid, +inf elsewhere.  dr: the right map's row,
// a scalar gather.
__device__ __forceinline__ float lr_diff(int x, float v, const float* dr, float lo, float hi, int W) {
    const int t = target(x, v, lo, hi, W);
    float e = INFINITY;
    if (t >= 0) {
        const float m = dr[t];
        if ((m >= lo) & (m < hi)) e = fabsf(ss::sub_rn(v, m));
    }
    return e;
}

// B > 0, H > 0, W > 0 checked by the caller: 0 where the kernels take the shape
inline int map_shape(int B, int H, int W) {
    if ((long long)B * H * W >= (1ll << 31) || (long long)B * H >= (1ll << 31)) return SS_ERR_UNSUPPORTED;
    return SS_OK;
}

}  // namespace rview
}  // namespace ss
