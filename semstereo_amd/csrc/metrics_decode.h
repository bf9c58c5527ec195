// What the evaluation kernels share (metrics.hip, joint_metrics.hip): the class of a label, the prediction of six logits, the
// reductions of a wave.  One definition, so the joint record and the confusion matrix can never decode a pixel differently.
#pragma once
#include "common.h"

namespace ss {
namespace metrics {

constexpr int NC = 6;          // channels of the logits (the reference's US3D setting, main_us3d.py: nums = 6)
constexpr int NBIN = (NC + 1) * NC;      // joint histogram: label 0..5 and "outside" x prediction 0..5

enum { LT_I64 = 0, LT_U8 = 1, LT_F32 = 2 };      // include/semstereo_hip.h: label_dtype

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// the class of a label in [0, NC), or NC for "outside": never an index out of bounds.  Float labels truncate toward zero as the
// reference's np.asarray(..., dtype=int) does; NaN is outside.
__device__ __forceinline__ int label_class(long long v) { return (v < 0 || v >= NC) ? NC : (int)v; }
__device__ __forceinline__ int label_class(unsigned char v) { return v >= NC ? NC : (int)v; }
__device__ __forceinline__ int label_class(float f) { return (f > -1.f && f < (float)NC) ? (int)f : NC; }

template <int LT>
__device__ __forceinline__ int label_row(const void* y, long long i) {
    if (LT == LT_I64) return label_class(reinterpret_cast<const long long*>(y)[i]);
    if (LT == LT_U8) return label_class(reinterpret_cast<const unsigned char*>(y)[i]);
    return label_class(reinterpret_cast<const float*>(y)[i]);
}

// np.argmax: the lowest index among equal maxima, and a NaN counts as the maximum (the first one wins)
__device__ __forceinline__ int argmax6(const float (&z)[NC]) {
    float best = z[0];
    int idx = 0;
#pragma unroll
    for (int k = 1; k < NC; ++k) {
        const bool take = best == best && (z[k] > best || z[k] != z[k]);
        best = take ? z[k] : best;
        idx = take ? k : idx;
    }
    return idx;
}

}  // namespace metrics
}  // namespace ss
