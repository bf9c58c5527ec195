// The two-term fp16 operand form of the matrix-core kernels, stated once: the split, the block exponent of the activations
// (BlockExp) and the per-channel scale of the packed weights.  Used by conv3d_bf16s.hip, deconv3d_bf16s.hip, deconv2d_bf16s.hip,
// proj2d_f16s.hip and seghead_f16s.hip, in parts by conv3d_head.hip, conv3d_pre.hip and window_attention.hip.  Device code
// only; everything lives in the including file's anonymous namespace.
#pragma once
#include "common.h"
#include "split_bf16.h"

namespace {

// ---- the two-term fp16 form ("f16x3", NTERMS = 19) ----
// fp16 carries 11 significand bits, so x = hi + lo leaves |x - hi - lo| <= 2^-23 |x| (one fp32 ulp) and THREE
// products (hh, hl, lh; ll <= 2^-22 is dropped) reach the accuracy of the six bf16 ones at half the matrix-core
// time -- provided both terms stay NORMAL fp16 numbers (5 exponent bits).  Weights are pre-scaled per output
// channel by a power of two at pack time (undone in the epilogue); activations are block floating point: each
// staged chunk (8 channels x halo tile) is multiplied by 2^k with k from the running |max| of the tile, and the
// fp32 accumulators are re-scaled (exactly: a power of two) whenever k changes.  Everything within 2^-17 of the
// tile's maximum keeps full precision; below that the absolute error is <= 2^-39 of that maximum.
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f16x2_t = __attribute__((ext_vector_type(2))) _Float16;
__device__ __forceinline__ void split2_pk_f16(float x0, float x1, unsigned& h, unsigned& l) {
    const f32x2_t v = {x0, x1};
    const f16x2_t hv = __builtin_convertvector(v, f16x2_t);
    const f32x2_t r = {x0 - (float)hv[0], x1 - (float)hv[1]};
    h = __builtin_bit_cast(unsigned, hv);
    l = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2_t));
}
// max over the wave of non-negative floats (as their bit patterns), wave-uniform result
__device__ __forceinline__ unsigned wave_max_bits(unsigned x) {
    x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true));      // row_shr:1, 0 shifted in
    x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true));      // row_shr:2
    x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true));      // row_shr:4
    x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true));      // row_shr:8 -> lane 15 of each row
    return max(max((unsigned)__builtin_amdgcn_readlane((int)x, 15), (unsigned)__builtin_amdgcn_readlane((int)x, 31)),
               max((unsigned)__builtin_amdgcn_readlane((int)x, 47), (unsigned)__builtin_amdgcn_readlane((int)x, 63)));
}
// One wave-wide LDS-DMA load (buffer_load_dwordx4 ... lds): 64 lanes x 16 bytes from (voffset per lane, soffset) to 1 KB of
// LDS at `dst`, no registers.  (Kept in a helper: called directly inside some __global__ templates the builtin makes
// hipcc 7.2 drop the kernel's host stub without a diagnostic.)
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t res, uint4* dst, int voffset, int soffset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(res, (__attribute__((address_space(3))) void*)dst, 16, voffset, soffset, 0, 0);
}
// ... and 4 bytes per lane (buffer_load_dword ... lds): 64 lanes -> 256 bytes of LDS at `dst`
__device__ __forceinline__ void lds_dma4(__amdgpu_buffer_rsrc_t res, float* dst, int voffset, int soffset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(res, (__attribute__((address_space(3))) void*)dst, 4, voffset, soffset, 0, 0);
}
// a 4-byte LDS read that stays a ds_read_b32 on data the compiler cannot see being written (LDS-DMA); `p` points into LDS
__device__ __forceinline__ float lds_read4(const float* p) {
    return *(const volatile float __attribute__((address_space(3)))*)(p);
}
constexpr int F16X3 = 19;                                       // the ABI's `nterms` code of this form
// biased fp32 exponents.  A maximum with exponent e is scaled by 2^(E_ONE - e) into [2^14, 2^15); E_MIN floors e so that
// every scale and its inverse stay normal fp32 numbers (values below 2^-111 are flushed).  Both operands being normalised,
// an accumulator never exceeds K * 2^30 whatever the scales.  A value that INITIALISES an accumulator (a partial sum, the
// skip projection) enters the running maximum 2^-E_INIT_SHIFT-fold: it then sits below 2^100 in the scaled domain, and
// whenever that bound is what sets the scale, the products it pushes out of fp16's range lie below the value's own ulp.
constexpr int E_MIN = 16, E_ONE = 141, E_INIT_SHIFT = 85;

// 2^(e - 127) from its biased exponent e, 0 < e < 255 (e = 0 gives 0, e = 255 gives inf)
__device__ __forceinline__ float pow2_biased(int e) { return __uint_as_float((unsigned)e << 23); }
// the power of two that brings a maximum of biased exponent e into [2^14, 2^15), and its inverse
__device__ __forceinline__ float scale_for(int e) { return pow2_biased(127 + E_ONE - e); }
__device__ __forceinline__ float unscale_for(int e) { return pow2_biased(127 - E_ONE + e); }

// max(m0, |v[0]|, ..., |v[N-1]|): a thread's share of a staged chunk's maximum.  fmaxf drops a NaN in every kernel.  DROP_INF says
// what an infinity does:
//   false (conv3d_bf16s, deconv3d_bf16s): it enters the maximum and the block exponent is 255 for the rest of the tile, whose
//         other values are then scaled far below fp16's range: the whole tile is affected, not only the infinity's receptive field.
//   true  (deconv2d_bf16s, proj2d_f16s, seghead_f16s): it is left out of the maximum, stays an infinity after scaling and poisons
//         its own receptive field only; every other output keeps the bits it has without the infinity (their tests assert it).
// The 3-D kernels are older and were specified tile-wide ("two-term fp16"); the 2-D kernels, written later, confine it.  The
// two rules are kept as each kernel had them; they are not unified here.
template <bool DROP_INF, int N>
__device__ __forceinline__ float abs_max(const float (&v)[N], float m0) {
    float m = m0;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const float ax = fabsf(v[q]);
        m = fmaxf(m, DROP_INF && ax == __builtin_inff() ? 0.f : ax);
    }
    return m;
}

// the biased exponent of a workgroup's maximum from its four waves' wave_max_bits, floored at E_MIN
__device__ __forceinline__ int workgroup_exponent(const unsigned (&wmax)[4]) {
    return max((int)(max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3])) >> 23), E_MIN);
}

// Block-floating scale of the staged chunks of one output tile.  e_cur: the biased exponent the accumulators are scaled for;
// e_run: that of the tile's running maximum (monotone: the accumulators only scale down after the first chunk).
struct BlockExp {
    int e_cur = E_ONE, e_run = E_MIN;
    __device__ __forceinline__ void reset() { e_cur = E_ONE; e_run = E_MIN; }
    // Takes in the four waves' maxima of the chunk staged next; true when the scale has to change (workgroup-uniform).  The caller
    // then multiplies every accumulator by rescale(), an exact power of two.  (Two calls with the branch between them in the
    // kernel: with the branch inside one helper the compiler lays the blocks of the 3-D kernels out differently.)
    __device__ __forceinline__ bool advance(uint4 wm) {
        e_run = max(e_run, (int)(max(max(wm.x, wm.y), max(wm.z, wm.w)) >> 23));      // inf / NaN: 255
        return e_run != e_cur;
    }
    __device__ __forceinline__ float rescale() {
        const float ratio = pow2_biased(max(127 + e_cur - e_run, 0));
        e_cur = e_run;
        return ratio;
    }
    __device__ __forceinline__ float in_scale() const { return scale_for(e_cur); }        // activations -> [2^14, 2^15)
    __device__ __forceinline__ float acc_unscale() const { return unscale_for(e_cur); }   // ... and back, in the epilogue
};

// Packed weights: a channel's values are divided by u, the power of two that brings the channel's max |w| into [2^14, 2^15).
// weight_unscale: `m` = this thread's max |w| over its share of the channel, `wmax` = the workgroup's LDS array -> u, the same
// value in every thread.  Synchronisation: called by ALL 256 threads of the workgroup, outside divergent code; it holds one
// __syncthreads() (between the four waves' writes of `wmax` and everybody's read).  `wmax` is not read before that barrier and
// not written after it, so a kernel that calls this once needs no barrier of its own; a second call needs one in between.
__device__ __forceinline__ float weight_unscale(float m, unsigned (&wmax)[4]) {
    const unsigned wm = wave_max_bits(__float_as_uint(m));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = wm;
    __syncthreads();
    return unscale_for(workgroup_exponent(wmax));
}
// term 0 / 1 of x = w / u as an fp16 bit pattern
__device__ __forceinline__ unsigned short split_weight_f16(float x, int term) {
    const _Float16 h = (_Float16)x;
    const _Float16 l = (_Float16)(x - (float)h);
    return __builtin_bit_cast(unsigned short, term == 0 ? h : l);
}

}  // namespace
