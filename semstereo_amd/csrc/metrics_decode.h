// How a pixel is decoded, for every kernel that reads a label map or takes the prediction of the logits (metrics.hip,
// joint_metrics.hip, vis.hip; loss.hip and sample_prep.hip share the dtype codes): the class of a label, np.argmax's rule.  One
// definition, so the joint record, the confusion matrix and the colours of one pixel can never differ.
#pragma once
#include "common.h"

namespace ss {
namespace metrics {

constexpr int NC = 6;          // channels of the logits (the reference's US3D setting, main_us3d.py: nums = 6)
constexpr int NBIN = (NC + 1) * NC;      // joint histogram: label 0..5 and "outside" x prediction 0..5

enum { LT_I64 = 0, LT_U8 = 1, LT_F32 = 2 };      // include/semstereo_hip.h: label_dtype

// the class of a label in [0, NC), or NC for "outside": never an index out of bounds.  Float labels truncate toward zero as the
// reference's np.asarray(..., dtype=int) and label.to(torch.int64) do; NaN is outside.
__device__ __forceinline__ int label_class(long long v) { return (v < 0 || v >= NC) ? NC : (int)v; }
__device__ __forceinline__ int label_class(unsigned char v) { return v >= NC ? NC : (int)v; }
__device__ __forceinline__ int label_class(float f) { return (f > -1.f && f < (float)NC) ? (int)f : NC; }

template <int LT>
__device__ __forceinline__ int label_row(const void* y, long long i) {
    if (LT == LT_I64) return label_class(reinterpret_cast<const long long*>(y)[i]);
    if (LT == LT_U8) return label_class(reinterpret_cast<const unsigned char*>(y)[i]);
    return label_class(reinterpret_cast<const float*>(y)[i]);
}

// np.argmax: the lowest index among equal maxima, and a NaN counts as the maximum (the first one wins).  Whether a later channel's z
// replaces the best so far (three compares and no branch: & and | on purpose):
__device__ __forceinline__ bool argmax_take(float best, float z) { return (best == best) & ((z > best) | (z != z)); }

__device__ __forceinline__ int argmax6(const float (&z)[NC]) {
    float best = z[0];
    int idx = 0;
#pragma unroll
    for (int k = 1; k < NC; ++k) {
        const bool take = argmax_take(best, z[k]);
        best = take ? z[k] : best;
        idx = take ? k : idx;
    }
    return idx;
}

}  // namespace metrics
}  // namespace ss
