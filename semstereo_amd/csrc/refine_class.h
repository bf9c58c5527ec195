// What the refinement kernels share (disparity_refine.hip, disparity_fill2d.hip, disparity_median.hip, disparity_speckle.hip): the class of a pixel -- ONE definition
// (include/semstereo_hip.h, "disparity refinement": class[x]), so the fill, the median and the speckle filter can never disagree on which surface a
// pixel belongs to.
#pragma once
#include "common.h"
#include "metrics_decode.h"
#include "stream.h"

namespace ss {
namespace refine {

constexpr int NCLS = 8;                  // classes 0 .. 7; NCLS itself stands for "none"

// class[x]: int(v) for an integer-valued 0 <= v < 8, NCLS for every other value (negative, 8 or more, a fraction, NaN)
__device__ __forceinline__ int class_of(long long v) { return (v < 0 || v >= NCLS) ? NCLS : (int)v; }
__device__ __forceinline__ int class_of(unsigned char v) { return v >= NCLS ? NCLS : (int)v; }
__device__ __forceinline__ int class_of(float f) { return (f >= 0.f && f < (float)NCLS && f == truncf(f)) ? (int)f : NCLS; }

// the classes of 4 consecutive pixels at element offset i of the label map
__device__ __forceinline__ void classes4(const void* y, int dtype, long long i, int nv, int (&c)[4]) {
    using ss::stream::load4;
    if (dtype == ss::metrics::LT_I64) {
        long long v[4];
        load4(reinterpret_cast<const long long*>(y) + i, nv, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = class_of(v[j]);
    } else if (dtype == ss::metrics::LT_U8) {
        unsigned char v[4];
        load4(reinterpret_cast<const unsigned char*>(y) + i, nv, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = class_of(v[j]);
    } else {
        float v[4];
        load4(reinterpret_cast<const float*>(y) + i, nv, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = class_of(v[j]);
    }
}

}  // namespace refine
}  // namespace ss
