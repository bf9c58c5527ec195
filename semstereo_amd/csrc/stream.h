// What the streaming kernels share (loss.hip, metrics.hip, joint_metrics.hip, vis.hip, sample_prep.hip, right_view.hip, disparity_refine.hip, disparity_fill2d.hip, disparity_median.hip, disparity_speckle.hip, scene_tiles.hip).  They are all one kind of
// kernel: BLOCK threads, a capped grid with a grid-stride loop, a lane takes 4 consecutive elements (one wide access where the address
// allows, scalars otherwise), and a reduction goes thread -> wave (shuffles) -> LDS -> one partial per workgroup in the caller's
// workspace -> a small finish launch that adds the partials in a fixed order.  No floating-point atomics anywhere: two calls on the
// same inputs return the same bits.  The order of that sum is written down here, once.
#pragma once
#include "common.h"

namespace ss {
namespace stream {

constexpr int BLOCK = 256;     // threads of every streaming kernel: four waves

// workgroups for `work` lane-trips: one trip per lane where that fits under `cap`, never fewer than one
inline int grid_for(long long work, int cap) {
    const long long g = ceil_div_ll(work, BLOCK);
    return (int)(g < 1 ? 1 : (g < cap ? g : cap));
}

// a: a power of two.  A null pointer is aligned, so an optional tensor needs no test of its own.
__host__ __device__ __forceinline__ bool aligned_to(const void* p, int a) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(a - 1)) == 0; }
__host__ __device__ __forceinline__ bool aligned16(const void* p) { return aligned_to(p, 16); }

// ---------------------------------------------------------------- reductions
// The shuffle-down tree 32, 16, ..., 1: the total is valid in lane 0.  T: double, int, long long, unsigned long long.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_down(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, 64));
    return v;
}

// v[k] summed over the workgroup, every k; lds holds 4 * K elements.  The order is fixed and is part of the recorded bits: in a wave
// the shuffle-down tree of wave_sum, then the four waves' totals as (w0 + w1) + (w2 + w3).
//   - The totals land in EVERY thread (gradients_k builds its table from them in all 256; a kernel that writes a partial uses thread 0's).
//   - The helper owns the leading barrier: no lane writes lds before every thread is done with what it held, so calls may follow each
//     other on the same lds (disp_loss_finish_k calls it in a loop) and the caller adds no barrier of its own.
template <int K, typename T>
__device__ __forceinline__ void block_sum(T (&v)[K], T* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) lds[wave * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (lds[k] + lds[K + k]) + (lds[2 * K + k] + lds[3 * K + k]);
}

// the same for a minimum and a maximum (lds: 8 floats); both decisions above hold
__device__ __forceinline__ void block_minmax(float& lo, float& hi, float* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    lo = wave_min(lo);
    hi = wave_max(hi);
    __syncthreads();
    if (lane == 0) lds[wave] = lo, lds[4 + wave] = hi;
    __syncthreads();
    lo = fminf(fminf(lds[0], lds[1]), fminf(lds[2], lds[3]));
    hi = fmaxf(fmaxf(lds[4], lds[5]), fmaxf(lds[6], lds[7]));
}

// An EXCLUSIVE scan of v[k] over the workgroup's 256 threads, every k, for values that are MONOTONE in the thread: a thread holds
// `identity` (nothing) or a value that is not below (DOWN: not above) any value an earlier thread holds -- a column of the thread's own
// chunk of a row, as in disparity_refine.hip.  lds: 16-byte aligned, 4 * K ints with K rounded up to 4.
//   DOWN = false: thread t receives the MAXIMUM of v[k] over threads 0 .. t - 1, thread 0 `identity`: a prefix, carried left to right
//   DOWN = true:  thread t receives the MINIMUM of v[k] over threads t + 1 .. 255, thread 255 `identity`: a suffix, carried right to left
// For monotone values that extreme is the value of the NEAREST thread on that side that holds one, so the scan is a selection.  Order:
// in a wave one ballot of "holds a value" names that lane (the highest set bit below the lane's own; DOWN: the lowest above) and one
// shuffle fetches its value -- a doubling scan (steps 1 .. 32) was measured first: its 7 shuffles per value, 126 per thread and row,
// are LDS-pipe instructions and were most of the kernel's LDS time (profiles/EXPERIMENTS.md, part AC).  The wave's total, its last
// (first) lane's own value or else what that lane received, goes to lds; the totals of the waves before (after) this one fill in,
// nearest wave first, where the own wave had nothing.  Selections of integers: no order matters for the bits.  The helper owns the
// leading barrier, as block_sum does.
template <int K, bool DOWN>
__device__ __forceinline__ void block_scan_exclusive(int (&v)[K], int identity, int* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull, above = ~((2ull << lane) - 1ull);      // (lane 63: 2 << 63 is 0, above is 0)
    int own[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        own[k] = v[k];
        const unsigned long long side = __ballot(v[k] != identity) & (DOWN ? above : below);
        const int from = side == 0ull ? lane : (DOWN ? __builtin_ctzll(side) : 63 - __builtin_clzll(side));
        const int got = __shfl(v[k], from, 64);
        v[k] = side == 0ull ? identity : got;
    }
    constexpr int Q = (K + 3) / 4;                 // a wave's totals as Q 16-byte words
    int4* totals = reinterpret_cast<int4*>(lds);
    __syncthreads();
    if (lane == (DOWN ? 0 : 63)) {
        int t[4 * Q];
#pragma unroll
        for (int k = 0; k < 4 * Q; ++k) t[k] = k >= K ? identity : (own[k < K ? k : 0] != identity ? own[k < K ? k : 0] : v[k < K ? k : 0]);
#pragma unroll
        for (int q = 0; q < Q; ++q) totals[wave * Q + q] = make_int4(t[4 * q], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]);
    }
    __syncthreads();
#pragma unroll
    for (int s = 1; s < 4; ++s) {                  // the waves on that side, nearest first (w is the same for a whole wave)
        const int w = DOWN ? wave + s : wave - s;
        if (w < 0 || w >= 4) continue;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int4 t4 = totals[w * Q + q];
            const int t[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * q + j < K && v[4 * q + j] == identity) v[4 * q + j] = t[j];
        }
    }
}

// ---------------------------------------------------------------- 4 consecutive elements of a row
// The 4-pixel groups of all rows of a [B,H,W] map are numbered row by row (QW = ceil(W / 4) per row); the launchers keep their number
// below 2^31, so the group's row and column come from 32-bit divisions and only the element offsets are 64-bit.
struct RowQuad {
    unsigned b, h;
    int x0, nv;                // first column, and how many of the 4 lie inside the row
};
__device__ __forceinline__ RowQuad row_quad(unsigned q, unsigned QW, unsigned H, int W) {
    const unsigned row = q / QW, qx = q - row * QW, b = row / H;
    const int x0 = (int)(qx * 4u), left = W - x0;
    return RowQuad{b, row - b * H, x0, left < 4 ? left : 4};
}

// one wide access, or nv scalars (a load leaves the rest zero)
__device__ __forceinline__ void load4(const float* p, int nv, float (&v)[4]) {
    if (nv == 4 && aligned_to(p, 16)) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[j] : 0.f;
    }
}
__device__ __forceinline__ void load4(const unsigned char* p, int nv, unsigned char (&v)[4]) {
    if (nv == 4 && aligned_to(p, 4)) {
        const uchar4 q = *reinterpret_cast<const uchar4*>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[j] : (unsigned char)0;
    }
}
__device__ __forceinline__ void load4(const long long* p, int nv, long long (&v)[4]) {
    if (nv == 4 && aligned_to(p, 16)) {
        const longlong2 a = reinterpret_cast<const longlong2*>(p)[0], b = reinterpret_cast<const longlong2*>(p)[1];
        v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[j] : 0ll;
    }
}
// 4 interleaved RGB pixels (12 bytes) at p as three little-endian words: three dword loads, or 3 nv byte loads (the rest zero)
__device__ __forceinline__ void load_rgb4(const unsigned char* p, int nv, unsigned (&w)[3]) {
    if (nv == 4 && aligned_to(p, 4)) {
        const unsigned* q = reinterpret_cast<const unsigned*>(p);
        w[0] = q[0], w[1] = q[1], w[2] = q[2];
    } else {
        w[0] = w[1] = w[2] = 0u;
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < 3 * nv) w[k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
    }
}
__device__ __forceinline__ unsigned rgb_byte(const unsigned (&w)[3], int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }
__device__ __forceinline__ void store4(float* p, int nv, const float (&v)[4]) {
    if (nv == 4 && aligned_to(p, 16)) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) p[j] = v[j];
    }
}
__device__ __forceinline__ void store4(int* p, int nv, const int (&v)[4]) {
    if (nv == 4 && aligned_to(p, 16)) {
        *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) p[j] = v[j];
    }
}
__device__ __forceinline__ void store4(unsigned char* p, int nv, const float (&v)[4]) {
    if (nv == 4 && aligned_to(p, 4)) {
        *reinterpret_cast<uchar4*>(p) = make_uchar4((unsigned char)v[0], (unsigned char)v[1], (unsigned char)v[2], (unsigned char)v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) p[j] = (unsigned char)v[j];
    }
}

}  // namespace stream
}  // namespace ss
