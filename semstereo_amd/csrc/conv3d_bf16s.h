// 3x3x3 Conv3d (+ folded BatchNorm, residual, ReLU) with fp32 operands emulated on the bf16 matrix
// core: "split-bf16" engine for the same layers as conv3d.hip (gfx950 v_mfma_f32_32x32x16_bf16).
//
// Every fp32 value is split exactly into three bf16 terms x = hi + mid + lo (24+ significand bits);
// a product a*b is the sum of its cross terms.  Keeping the six terms down to 2^-24 relative
// (hh, hm, mh, mm, hl, lh) on bf16 MFMAs with fp32 accumulation gives a GEMM whose measured error
// (tools/exp_split_bf16.hip on MI355X: 1.1e-7 of sum|a*b| at K = 864..3456) is BELOW that of the exact
// fp32 MFMA (1.8e-7), at 6/16 of its matrix-core time; the three-term form (hh, hm, mh: 3/16 of the
// time) measures 3-6e-7.  NTERMS selects the form; products of bf16 are exact in fp32, so the only
// rounding is the accumulation, as in any fp32 GEMM.
//
// GEMM mapping: M = 32 output channels, N = 32 consecutive output columns of one row (lanes),
// K-step of 16 = lanes 0-31: 8 input channels of tap 2s, lanes 32-63: the same 8 channels of tap
// 2s+1 (27 taps -> 14 steps, the 28th half is zero).  The bf16 B operand wants 8 consecutive k per
// lane, so the LDS halo tile is CHANNEL-INNERMOST: [term][position][8 channels] bf16 = one 16-byte
// slot per (term, position); a wave's fragment read is 64 consecutive slots (conflict-free
// ds_read_b128).  The NCDHW fp32 input is transposed/split while it is staged: each thread owns
// whole positions, loads their 8 channels (coalesced along W per channel, register-prefetched one
// chunk ahead), splits them and writes three 16-byte slots.  Weights are pre-split and pre-packed in
// fragment order by ss_pack_conv3d_weights_bf16s and streamed from L2 (every wave of a workgroup
// reads the same 16 B per lane per term and step; LDS is left to the activations).
//
// This header is what the translation units that instantiate the kernel share -- conv3d_bf16s.hip (the plain, stride-2 and 2-D forms),
// conv3d_gather.hip (GATHER) and conv3d_classifier.hip (HEAD): the tuning constants, the kernel template and the launch helpers.
#pragma once
#include <algorithm>
#include <stdlib.h>

#include "common.h"
#include "conv_plan.h"
#include "split_f16.h"

// Phase stamps of a workgroup: no-ops here.  tools/conv_timing.hip defines SS_STAMP / SS_STAMP_STEPS_* before including
// conv3d_bf16s.hip (and with it this header) to build the instrumented library tools/wg_phases.py reads (tools/build_timing.sh);
// the product build has no instrumentation in it.
#ifndef SS_STAMP
#define SS_STAMP(k) do {} while (0)
#define SS_STAMP_STEPS_BEGIN() do {} while (0)
#define SS_STAMP_STEPS_END() do {} while (0)
#define SS_STAMP_FINISH() do {} while (0)
#endif

namespace {

// measured-best settings (each was swept on the bench shapes)
#ifndef SS_IN_STEPS
#define SS_IN_STEPS 10            // K-steps over which the next chunk's input loads are issued
#endif
#ifndef SS_IN_STEPS_S2
#define SS_IN_STEPS_S2 10         // ... in the stride-2 form (tools/build_variant.sh sweeps: 5: 94.0, 7: 89.1, 10: 87.9, 14: 86.5 us)
#endif
#ifndef SS_A_AHEAD_S2
#define SS_A_AHEAD_S2 2           // SS_A_AHEAD / SS_ROW_PAIR of the stride-2 form (3, 4 steps ahead / row pairs: all within +-1.5 us of 90)
#endif
#ifndef SS_ROW_PAIR_S2
#define SS_ROW_PAIR_S2 1
#endif
constexpr int SS_ROW_PAIR = 1;    // rows whose MFMAs alternate; 2 measured 1 % slower: the other wave of the SIMD already fills the gaps
#ifndef SS_A_AHEAD
#define SS_A_AHEAD 2              // K-steps between the load of a weight fragment and its MFMAs
#endif
#ifndef SS_F16_WGS
#define SS_F16_WGS 2              // workgroups per CU the fp16 form is compiled for (3 = 168 VGPRs: spills, +29 %)
#endif

// KD: kernel depth, 3 (3x3x3) or 1 (3x3 over [B,C,H,W] maps seen as depth-1 volumes: 9 taps, 5 K-steps)
// WSL: 16-byte LDS slots of a chunk's weight fragments (0: every wave fetches its own)
// MS: waves that share a row group and split the workgroup's output channels (1: every wave owns NT rows of all of them)
// XSL: further 16-byte slots behind everything else (the gather form's candidate / weight words)
template <int S, int NT, int TD, int TH, int KD = 3, int LT = 3, int WSL = 0, int MS = 1, int XSL = 0>      // LT: operand terms kept in LDS
struct BCfg {
    static constexpr int KT = KD * 9, KSTEPS = (KT + 1) / 2;
    static constexpr int ID = (TD - 1) * S + KD, IH = (TH - 1) * S + 3, IW = 31 * S + 3;
    static_assert(KD == 3 || (KD == 1 && TD == 1), "2-D form: depth-1 tiles");
    static constexpr int CS = ID * IH * IW;                    // positions in the halo tile
    static constexpr int NPOS = (CS + 255) / 256;              // positions per thread
    // + one all-zero slot (the 28th half-step) + the waves' maxima (f16 form) + the affine of the workgroup's (<= 64) channels
    static constexpr int SLOTS = LT * CS + 2 + 48 + WSL + XSL;
    static constexpr int XS0 = LT * CS + 2 + 48 + WSL;         // first extra slot
    static constexpr size_t LDS_BYTES = (size_t)SLOTS * 16;
    static_assert(TD * TH * MS == 4 * NT && TH % NT == 0 && (MS == 1 || MS == 2), "4 / MS wave groups x NT rows tile TD x TH");
};

#ifndef SS_ACCB_PASSES_44
#define SS_ACCB_PASSES_44 2       // passes over a chunk's K-steps of the chunk-blocked 4 x 4 x 32 form (acc_passes below); 1: one pass with the rest of the two-pass form's register diet: 235 VGPRs, no scratch; built, never timed (profiles/EXPERIMENTS.md I.6)
#endif
// (accb: the chunk-blocked 4-row tile walks its rows in two passes per chunk and reads the fragments of every pass from the LDS copy;
// the plain 4-row tile fetches its fragments per wave: through LDS it measured 250.7 / 250.0 -> 255.4 / 253.5 us on classif,
// profiles/r05_ad_wlds_nt4.txt)
constexpr bool wlds_form(int S, int NT, int NTERMS, int MT, int KD, bool gather = false, bool accb = false) {
    // (the gather form's tile has no LDS left for the 28 KB slab at two workgroups per CU)
    return NTERMS == F16X3 && S == 1 && (NT == 1 || (accb && NT == 4 && !gather)) && MT == 1 && KD == 3;       // (NT = 2: 43 B/clk, measured +3 %: left alone)
}
// Chunk-blocked accumulation on the 4-row tile: a second accumulator set for all four rows does not fit beside the first (64 + 64 of
// 256 registers: 15 / 46 spilled on the 4 x 4 / 2 x 8 tile).  The chunk's K-steps are therefore walked TWICE, each pass over two of
// the wave's rows with a 32-register second set that is folded into `acc` at the end of the pass.  A row's products are still summed
// from zero in K order and added to `acc` once per chunk: the same bits.  What a second pass re-reads are the weight fragments, which
// this form keeps in LDS (wlds_form).  Against the single pass that spills, alone at batch 4 / 8 (profiles/fill_hint_ab.txt): the 2 x 8
// form -9.6 / -5.7 %, the 4 x 4 form +0.8 / +3.1 %; the pipelined step 606 -> 615 pairs/s.
constexpr int acc_passes(int S, int NT, int NTERMS, int MT, int KD, bool accb, bool gather) {
    return (accb && NT == 4 && wlds_form(S, NT, NTERMS, MT, KD, gather, accb)) ? 2 : 1;
}
// gather form: per halo position one candidate word and two attention words (this tile's, the next tile's), each thread's
// own positions p = tid + 256 i -> 3 x NPOS x 256 floats
constexpr int gather_slots(bool gather, int S, int TD, int TH, int KD) {
    return gather ? 3 * ((((TD - 1) * S + KD) * ((TH - 1) * S + 3) * (31 * S + 3) + 255) / 256) * 64 : 0;
}
// head form (HEAD of the kernel): the 32 -> 1 head's weight fragments, [3 bf16 terms][2 K-steps][64 lanes] 16-byte slots
constexpr int HEAD_WSLOTS = 3 * 2 * 64;
constexpr int HEAD_PATCH = 6 * 6 * 34;        // a 4 x 4 x 32 tile's contributions to the head's output: its positions and one ring around them
// the bits of the kernel's `relu` word (launch_conv packs them from ConvArgs' three booleans)
constexpr int RELU_BIT = 1, RES_PRE_BIT = 2, OUT_CL_BIT = 4;

// (ACCB of the kernel, chunk-blocked accumulation, is a property of the LAYER: conv_plan.h decides it)

// GATED: the channelAtt gate is fused into the epilogue (only concat_stem has one, so its launches also carry
// their own kernel symbol in a profile: conv3d_bf16s<..., true>)
// MT: 32-channel output tiles per wave (the activation fragments of a row then feed MT x 6 MFMAs: used by the stride-2
// layers, whose staging is 8x dearer per MFMA and whose 2-4 output tiles would otherwise each stage the same input)
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

// MS = 2 (stride-2 layers): the four waves are 2 row groups x 2 halves of the workgroup's 64 * MT output channels.  A wave then
// fetches the weight fragments of ITS channels only (the vector L1 carried every fragment four times per workgroup: 32 KB
// per K-step and CU beside 8 KB of activations, 640 clocks at its 64 B/clk for 384 clocks of MFMA issue -- tools/wg_phases_s2.py)
// and reads the activation fragments of two rows from LDS instead of one.
//
// GATHER (r05; SURVEY.md section 8 f1, second half: sparse concat -> x att -> concat_stem in ONE launch): `in` is the 2-D right
// feature map [B,Cin,H,W]; the operand of the convolution, x[c, j, h, w] = att[j,h,w] * in[c, h, w - cand[j,h,w]] (zero where
// the column leaves the image) -- the warped half of the reference's sparse concat volume times the attention weights
// (models/SemStereo.py:241-244, 316-318; models/submodule.py:265-288 for INTEGER candidates, which is what :299-305 produce) --
// is formed while the halo tile is staged: no [B,Cin,nd,H,W] volume exists.  Per halo position the candidate and the weight
// are fetched once per TILE by LDS-DMA (no registers: each thread's own positions, parked in LDS) a chunk ahead of their
// first use; the gathered loads take the place of the volume loads one for one (same prefetch registers, same slices).
// D = the number of candidates.  Cin % 8 == 0 and Cin >= 16 (the look-ahead needs two chunks per tile).
//
// HEAD (r05, late): nn.Sequential(convbn_3d(32,32,3,1,1), ReLU, Conv3d(32,1,3,p1)) -- `classif` / `classif_att_`, models/SemStereo.py:228-234 -- in
// ONE pass over the volume: the 32-channel intermediate never leaves the CU.  After a tile's K loop its y = ReLU(BN(conv)) sits in the
// accumulators in exactly the B-operand layout of the next contraction (lane = position, 8 consecutive registers = 8 channels of a
// K-step), so t[tap][position] = sum_c w2[c][tap] y[c][position] is 12 more MFMAs per row (27 taps as matrix rows, three bf16 terms, six
// products); the 27 shifted sums out[q] = sum_tap t[tap][q + tap - 1] are done in three deterministic stages: over kh in registers
// (a wave owns 4 rows of one plane, a lane half whole kh-triples), over (kd, kw) through a 30 KB LDS buffer that reuses the dead
// activation tile -- giving the tile's contribution to the 6 x 6 x 34 output positions it touches, written to `out` as a PATCH
// [B][tiles][6][6][34] -- and over the <= 8 tiles that touch an output position in classifier_patch_sum_kernel.  201 MB written +
// 288 MB read per classifier become 15 + 15 MB; the head's own launch disappears.  `cand` carries the head's fragments
// (ss_pack_classifier_head_weights), `out` the patch buffer.
//
// CAT (the 2-D form only): the input's channels [0, csplit) come from `in` (`in2` for batch elements >= bsplit) and [csplit, Cin) from
// `cand` (`catt` for batch elements >= bsplit), each a contiguous [B,.,H,W] tensor -- Conv2x's torch.cat((x, rem), 1) in front of its
// 3x3 conv (models/submodule.py:156-160) without the copy.  csplit % 8 == 0, so a staged 8-channel chunk never straddles the two: the
// chunk loop changes the buffer descriptor at csplit and nothing else; the weights, the K order and therefore the bits are those of
// the plain form on the materialised concatenation.
template <int S, int NT, int TD, int TH, int NTERMS, bool GATED, int MT, int KD = 3, int MS = 1, bool ACCB = false, bool GATHER = false, bool HEAD = false, bool CAT = false>
__global__ __launch_bounds__(256, (NTERMS == F16X3) ? SS_F16_WGS : 2) void conv3d_bf16s(const float* __restrict__ in, const uint4* __restrict__ wsplit,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        const float* __restrict__ residual, const float* __restrict__ gate,
                                                        float* __restrict__ out,
                                                        int Cin, int D, int H, int W, int Cout, int Do, int Ho, int Wo,
                                                        int tiles_w, int tiles_h, int ntiles, int relu,
                                                        const float* __restrict__ cand, const float* __restrict__ catt,
                                                        const float* __restrict__ in2, int bsplit, int csplit) {
    static_assert(!CAT || (KD == 1 && S == 1 && !GATED && !GATHER && !HEAD), "concat-free form: the plain 2-D tiles");
    static_assert(!GATHER || (S == 1 && MT == 1 && KD == 3 && MS == 1), "gather form: plain stride-1 3-D tiles");
    static_assert(!HEAD || (S == 1 && NT == 4 && TD == 4 && TH == 4 && MT == 1 && KD == 3 && MS == 1 && !GATED && !GATHER && NTERMS == F16X3),
                  "head form: the 4 x 4 x 32 tile of the fp16 engine, one wave per plane");
    constexpr bool F16 = (NTERMS == F16X3);
    constexpr int NC = (NTERMS == 6) ? 3 : 2;                  // operand terms actually read
    constexpr int NCW = F16 ? 2 : 3;                           // terms in the packed weights
    // Small tiles in the fp16 form: a K-step has only 3 MFMAs per row and wave, and eight waves per CU each re-reading the
    // step's 2 KB of weight fragments every 96-192 cycles ask the vector L1 for 43-85 B/clk of its 64.  The chunk's fragments
    // (14 steps x 2 terms, 28 KB) are then brought into LDS once per workgroup by LDS-DMA loads (no registers) and read
    // from there by the four waves (deconv3d_bf16s.hip has the measurement: -11 %).
    constexpr bool WLDS = wlds_form(S, NT, NTERMS, MT, KD, GATHER, ACCB);
    // LOCAL: the register diet that goes with it (fragment addresses per K-step, halo index arithmetic per tile; see read_b, make_poff)
    constexpr bool LOCAL = acc_passes(S, NT, NTERMS, MT, KD, ACCB, GATHER) > 1;
    constexpr int PASSES = !LOCAL ? 1 : (TD == 4 ? SS_ACCB_PASSES_44 : 2), NR = NT / PASSES;       // rows of a pass over the chunk's K-steps
    static_assert(!ACCB || NTERMS == F16X3, "chunk-blocked accumulation: fp16 form only");
    static_assert(!WLDS || MS == 1, "the LDS copy of the weights is one channel tile's");
    using C = BCfg<S, NT, TD, TH, KD, NC, WLDS ? ((KD * 9 + 1) / 2) * 2 * 64 : 0, MS, gather_slots(GATHER, S, TD, TH, KD) + (HEAD ? HEAD_WSLOTS : 0)>;
    constexpr int WL = NC * C::CS + 2 + 48;                    // first slot of the weight fragments
    constexpr int KSTEPS = C::KSTEPS;                          // 14 (3x3x3: ceil(27 taps / 2)) or 5 (3x3)
    constexpr int ZSLOT = NC * C::CS;                          // the all-zero slot; ZSLOT + 1: the four waves' maxima
    extern __shared__ __attribute__((aligned(16))) uint4 lds[];   // [NC][CS] slots + zero slot + maxima

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    SS_STAMP(0);
    const int l31 = lane & 31, half = lane >> 5;
    // PERSISTENT workgroups: a workgroup walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of its (channel tile, batch
    // element).  While the LAST chunk of a tile is multiplied, the prefetch registers -- idle there until now -- fetch the
    // FIRST chunk of the next tile, so only the very first tile of a workgroup pays the exposed round trip to HBM that used
    // to open every workgroup's life (12 k of ~100 k cycles, tools/wg_phases.py); the epilogue's stores then drain under the
    // next tile's first K-steps.
    const int co0 = blockIdx.y * 32 * MT * MS;                  // the workgroup's first channel
    const int wrow = wave / MS;                                 // row group of this wave
    const int cow = co0 + (wave % MS) * 32 * MT;                // this wave's first channel
    const int b = blockIdx.z;
    const int dzw = (wrow * NT) / TH, hy0 = (wrow * NT) % TH;
    // Stride 2: with a row's columns in their natural order the 32 lanes of a fragment read are 32 bytes apart, a 2-way bank conflict
    // per ds_read_b128 lane group (r05: SQ_LDS_BANK_CONFLICT 5.3 M cycles on the largest layer, the only conv family with any).  The
    // natural order stays: rows de-interleaved by column parity measured 5.3 M -> 0 conflicts but the largest layer 88.0 -> 94.8 us
    // (slot-owned loads) and 85.4 -> 87.7 (write-permuted), profiles/r06_e_ab_conv_s2_deint.txt, r06_e_ab_conv_s2_deint_w.txt.
    const int lane_pos = (dzw * S * C::IH + hy0 * S) * C::IW + l31 * S;     // slot of this lane's first row, tap (0,0,0)
    auto tile_origin = [&](int tile, int& ow0, int& oh0, int& od0) {
        int t = tile;
        const int tw = t % tiles_w; t /= tiles_w;
        const int th = t % tiles_h; t /= tiles_h;
        ow0 = tw * 32; oh0 = th * TH; od0 = t * TD;
    };
    // relu bit 0: ReLU; bit 1: `residual` is added BEFORE the affine: a partial sum of the same convolution computed
    // elsewhere (stem_left.hip).  It joins the accumulator in the epilogue, fetched together with the gate (as initial
    // accumulators its 64 loads per lane were 14 k cycles of every workgroup's prologue: tools/wg_phases.py).
    const bool res_pre = (relu & RES_PRE_BIT) != 0 && residual != nullptr;
    // bit 2: CHANNELS-LAST output [Do][Ho][Wo][Cout] (the hand-off to the 32 -> 1 head of the same classifier, conv3d_head.hip,
    // which wants 8 consecutive channels of a position per lane): a lane's 4 consecutive channels of a fragment register
    // group go out as one 16-byte store instead of four 4-byte ones.  Plain stride-1 form only, Cout % 8 == 0.
    constexpr bool CAN_CL = !GATED && MT == 1 && S == 1 && KD == 3;
    const bool out_cl = CAN_CL && (relu & OUT_CL_BIT) != 0;
    // f16 form: float[Cout] of 2^-(weight scale of the channel), stored behind the packed terms (must agree with conv_packed().terms)
    const float* wunscale = reinterpret_cast<const float*>(
        reinterpret_cast<const char*>(wsplit) + (size_t)((Cin + 7) / 8) * C::KSTEPS * ((NTERMS == F16X3 ? 2 : 3) * 2 * Cout * 16));
    // Output-side addressing (partial sum in, result out, gate, residual): buffer descriptors per batch element with a
    // 32-bit per-lane offset per row and a scalar offset per channel, positions outside the volume parked beyond the
    // buffer (loads give 0, stores are dropped): no 64-bit per-lane arithmetic and no branches around the 64 stores of a
    // lane (they were ~35 instructions and 3.5 branches per store).
    const size_t out_plane = (size_t)Ho * Wo;
    const unsigned ochan_b = (unsigned)((size_t)Do * out_plane * 4), gchan_b = (unsigned)(out_plane * 4);
    const int obytes = (int)min((long long)Cout * (long long)ochan_b, 0x7fffffffLL);
    unsigned vout[NT], vgate[NT];
    auto set_outputs = [&](int tile) {
        int ow0, oh0, od0;
        tile_origin(tile, ow0, oh0, od0);
        const int ow_ = ow0 + l31, od_ = od0 + dzw;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int oh_ = oh0 + hy0 + i;
            const bool ok = ow_ < Wo && od_ < Do && oh_ < Ho;
            vout[i] = ok ? (unsigned)((((size_t)od_ * Ho + oh_) * Wo + ow_) * 4) + 4u * half * ochan_b : 0x80000000u;
            if (CAN_CL && out_cl) vout[i] = ok ? (unsigned)((((size_t)od_ * Ho + oh_) * Wo + ow_) * Cout * 4) + 16u * half : 0x80000000u;
            vgate[i] = ok ? (unsigned)(((size_t)oh_ * Wo + ow_) * 4) + 4u * half * gchan_b : 0x80000000u;
        }
    };
    // this lane's channel of fragment register r of output tile mt: cbase(mt, r) + 4 * half
    auto cbase = [&](int mt, int r) { return cow + mt * 32 + (r & 3) + 8 * (r >> 2); };
    f32x16 acc[MT * NT];                  // index mt * NT + row

    const size_t in_plane = (size_t)H * W, chan = GATHER ? in_plane : (size_t)D * in_plane;     // (gather: channels of a 2-D map)
    // (in2: batch elements bsplit, bsplit + 1, ... of the launch come from a SECOND input tensor -- the left and right views of
    // concat_feature in one launch without a torch.cat in front, ss_conv2d_bf16s_pair_fwd)
    const int Cin1 = CAT ? csplit : Cin;                        // channels of the (first) input tensor
    const float* inb = (in2 != nullptr && b >= bsplit) ? in2 + (size_t)(b - bsplit) * Cin1 * chan : in + (size_t)b * Cin1 * chan;

    // staging plan of a tile: this thread owns positions p = tid + 256*i of the halo tile, all 8 channels
    auto make_poff = [&](int tile, unsigned (&po)[C::NPOS]) {
        int ow0, oh0, od0;
        tile_origin(tile, ow0, oh0, od0);
        const int iw0 = ow0 * S - 1, ih0 = oh0 * S - 1, id0 = od0 * S - KD / 2;
        int ptid = tid;                // (LOCAL: opaque, so that the positions' index arithmetic is redone per tile instead of living in registers -- or scratch -- through the K loop)
        if constexpr (LOCAL) asm volatile("" : "+v"(ptid));
#pragma unroll
        for (int i = 0; i < C::NPOS; ++i) {
            const int p = ptid + 256 * i;
            const int wx = p % C::IW;
            int r = p / C::IW;
            const int hy = r % C::IH;
            const int dz = r / C::IH;
            const int gw = iw0 + wx, gh = ih0 + hy, gd = id0 + dz;
            const bool ok = (p < C::CS) && (unsigned)gd < (unsigned)D && (unsigned)gh < (unsigned)H && (unsigned)gw < (unsigned)W;
            // halo positions outside the volume get an offset beyond the buffer's num_records: the buffer
            // load returns 0 for them, no select needed
            po[i] = ok ? (unsigned)(((size_t)gd * in_plane + (size_t)gh * W + gw) * 4) : 0x80000000u;
        }
    };
    unsigned poff[C::NPOS];
    if constexpr (!GATHER) make_poff(blockIdx.x, poff);
    // ---- gather form: candidates and attention weights of a tile's halo positions, parked in LDS ----
    float* gcand = reinterpret_cast<float*>(&lds[C::XS0]);                       // [NPOS * 256]: candidates of the tile set up next
    float* gatt = gcand + C::NPOS * 256;                                        // [2][NPOS * 256]: weights of this tile / the next
    const __amdgpu_buffer_rsrc_t cres = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(GATHER ? cand + (size_t)b * D * in_plane : in), 0, GATHER ? (int)min((long long)D * (long long)in_plane * 4, 0x7fffffffLL) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t tres = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(GATHER ? catt + (size_t)b * D * in_plane : in), 0, GATHER ? (int)min((long long)D * (long long)in_plane * 4, 0x7fffffffLL) : 0, 0x00020000);
    // request (LDS-DMA, 4 bytes per lane, no registers) the candidate and weight words of `tile`'s halo positions; positions
    // outside the volume -- and every position of a tile that does not exist -- read beyond the buffers and get zeros
    auto gather_request = [&](int tile, int buf) {
        unsigned po[C::NPOS];
        make_poff(tile, po);                                   // offsets into [D][H][W]: the candidates' and the weights' own layout
        const unsigned dead = tile < ntiles ? 0u : 0x80000000u;
        const int wbase = __builtin_amdgcn_readfirstlane(wave * 64);
#pragma unroll
        for (int i = 0; i < C::NPOS; ++i) {
            lds_dma4(cres, gcand + 256 * i + wbase, (int)(po[i] | dead), 0);
            lds_dma4(tres, gatt + buf * (C::NPOS * 256) + 256 * i + wbase, (int)(po[i] | dead), 0);
        }
    };
    // offsets of the gathered elements of `tile` (its candidates have landed in gcand): row h, column w - candidate of the 2-D map
    auto gather_offsets = [&](int tile, unsigned (&po)[C::NPOS]) {
        __builtin_amdgcn_s_waitcnt(0x0F70);                    // vmcnt(0): the LDS-DMA words have landed
        int ow0, oh0, od0;
        tile_origin(tile, ow0, oh0, od0);
        const int iw0 = ow0 - 1, ih0 = oh0 - 1, id0 = od0 - 1;
#pragma unroll
        for (int i = 0; i < C::NPOS; ++i) {
            const int p = tid + 256 * i;
            const int wx = p % C::IW;
            int r = p / C::IW;
            const int hy = r % C::IH;
            const int dz = r / C::IH;
            const int gw = iw0 + wx, gh = ih0 + hy, gd = id0 + dz;
            const int col = gw - (int)lds_read4(gcand + p);      // integer candidates (the ABI's contract)
            const bool ok = (p < C::CS) && (unsigned)gd < (unsigned)D && (unsigned)gh < (unsigned)H && (unsigned)gw < (unsigned)W &&
                            (unsigned)col < (unsigned)W && tile < ntiles;
            po[i] = ok ? (unsigned)(((size_t)gh * W + col) * 4) : 0x80000000u;
        }
    };
    if constexpr (GATHER) {
        gather_request(blockIdx.x, 0);
        gather_offsets(blockIdx.x, poff);
    }
    // input prefetch registers, flattened q = c * NPOS + i, loaded in KSTEPS slices spread over the
    // K-steps of the previous chunk so that a wait for a weight fragment never drains them all
    constexpr int NQ = 8 * C::NPOS;
    // ... all of them within the first SS_IN_STEPS steps: the split phase at the end of the chunk waits
    // for the youngest slice, which needs a few K-steps (HBM latency) to land
    constexpr int IN_STEPS = ((S == 2 ? SS_IN_STEPS_S2 : SS_IN_STEPS) < KSTEPS) ? (S == 2 ? SS_IN_STEPS_S2 : SS_IN_STEPS) : KSTEPS;
    constexpr int QS = (NQ + IN_STEPS - 1) / IN_STEPS;
    float rin[NQ];
    int nlive = min(8, Cin), nlive_next = 8;                 // channels that exist in the staged / prefetched chunk
    if (tid == 0) lds[ZSLOT] = make_uint4(0u, 0u, 0u, 0u);
    // per-channel epilogue constants, fetched now and parked in LDS: read after the K loop they cost two exposed round
    // trips to L2/HBM per workgroup (tools/wg_phases.py).  aff[c] = scale, aff[64 + c] = shift, aff[128 + c] = 2^-(weight scale)
    float* aff = reinterpret_cast<float*>(&lds[ZSLOT + 2]);
    if constexpr (HEAD) {             // the head's weight fragments: parked in LDS once per workgroup
        const uint4* hw = reinterpret_cast<const uint4*>(cand);
        for (int i = tid; i < HEAD_WSLOTS; i += 256) lds[C::XS0 + i] = hw[i];
    }
    if (tid < 32 * MT * MS) {
        const int co = min(co0 + tid, Cout - 1);
        aff[tid] = scale ? scale[co] : 1.0f;
        aff[64 + tid] = shift ? shift[co] : 0.0f;
        aff[128 + tid] = F16 ? wunscale[co] : 1.0f;            // 2^-(weight scale of the channel)
    }

    // weight fragments: [global K-step g = blk*14 + s][term][half][Cout][8 bf16] as uint4 slots; lanes of
    // output channels beyond Cout read a clamped (valid) column and are dropped in the epilogue
    // Both operands are fetched with buffer loads: wave-uniform base (SGPR descriptor) + uniform
    // scalar offset + one 32-bit per-lane offset, so no 64-bit per-lane addresses are kept live.
    int wlane[MT];                                                            // byte offset of this lane's column, per output tile
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) wlane[mt] = (half * Cout + min(cow + mt * 32 + l31, Cout - 1)) * 16;
    const int wstep = NCW * 2 * Cout * 16;                                    // bytes per K-step
    const __amdgpu_buffer_rsrc_t wres = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint4*>(wsplit), 0, (int)min((long long)((Cin + 7) / 8) * KSTEPS * wstep, 0x7fffffffLL), 0x00020000);
    const __amdgpu_buffer_rsrc_t ires = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(inb), 0, (int)min((long long)Cin1 * (long long)chan * 4, 0x7fffffffLL), 0x00020000);
    // (CAT: the second tensor's channels, addressed from its own channel 0)
    const float* inc = !CAT ? inb : ((in2 != nullptr && b >= bsplit) ? catt + (size_t)(b - bsplit) * (Cin - csplit) * chan : cand + (size_t)b * (Cin - csplit) * chan);
    const __amdgpu_buffer_rsrc_t ires2 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(inc), 0, CAT ? (int)min((long long)(Cin - csplit) * (long long)chan * 4, 0x7fffffffLL) : 0, 0x00020000);
    const int chan_b = (int)(chan * 4);                                       // bytes per input channel
    auto load_a = [&](int g, int c, int mt) {
        return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(wres, wlane[mt], g * wstep + c * 2 * Cout * 16, 0));
    };
    // (plain cache policy, also for the gated launch -- concat_stem -- whose inputs are dead after it: nt / sc0+nt measured
    // 479.5 / 476 against 489.6 pairs/s on the whole step, the launch itself 284 -> 334 / 344 us)
    auto load_in = [&](int ch, int i) {                                       // channel ch (absolute), position slot i
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ires, (int)poff[i], ch * chan_b, 0));
    };
    const int G = ((Cin + 7) / 8) * KSTEPS;
    // Ring of weight fragments, AP steps ahead: vmcnt retires in order, so a wait for a fragment also
    // waits for every input (HBM) load issued before it -- the distance must cover HBM latency, not L2's.
    constexpr int AP = (S == 2) ? SS_A_AHEAD_S2 : SS_A_AHEAD, AR = AP + 1;
    uint4 aq[AR][MT][NC];                                      // aq[s % AR] = fragments of step s of the chunk
    if (!WLDS) {
#pragma unroll
        for (int k = 0; k < AP; ++k)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int c = 0; c < NC; ++c) aq[k][mt][c] = load_a(min(k, G - 1), c, mt);
    }
    {   // first chunk: plain load of every slice
#pragma unroll
        for (int q = 0; q < NQ; ++q) rin[q] = load_in(min(q / C::NPOS, nlive - 1), q % C::NPOS);
    }
    BlockExp bexp;                                              // f16 form: block-floating scale of the staged chunk (split_f16.h)
    // gather form: the prefetched chunk times the attention weights of its positions (models/SemStereo.py:318), rounded to fp32 as
    // the reference's materialised product is
    auto apply_att = [&](int buf) {
#pragma unroll
        for (int i = 0; i < C::NPOS; ++i) {
            const float a = lds_read4(gatt + buf * (C::NPOS * 256) + tid + 256 * i);
#pragma unroll
            for (int c = 0; c < 8; ++c) rin[c * C::NPOS + i] = ss::mul_rn(rin[c * C::NPOS + i], a);
        }
    };
    if constexpr (GATHER) apply_att(0);
    auto publish_max = [&](float m) {                                         // this wave's max(m, |rin|) -> LDS (an infinity counts)
        const unsigned wm = wave_max_bits(__float_as_uint(abs_max<false>(rin, m)));
        if (lane == 0) reinterpret_cast<unsigned*>(&lds[ZSLOT + 1])[wave] = wm;
    };
    if (F16) {
        publish_max(0.f);
        __syncthreads();
    }
    SS_STAMP(1);

    int gbuf = 0;                                               // gather form: which half of gatt holds this tile's weights
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x, gbuf ^= 1) {
    const bool has_next = tile + (int)gridDim.x < ntiles;
#pragma unroll
    for (int i = 0; i < MT * NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    bexp.reset();
    nlive = min(8, Cin);
    for (int ci0 = 0, g0 = 0; ci0 < Cin; ci0 += 8, g0 += KSTEPS) {
        // ---- split + transpose: registers -> [term][position][8 ch] ----
        if constexpr (WLDS) {         // this chunk's weights: wave w issues the (K-step, term) pairs i = w, w + 4, ...; lane -> (half, channel)
            // (the wave index as a scalar, opaque once per chunk: the entries' LDS addresses and source offsets are scalar arithmetic
            // done here instead of per-lane loop invariants hoisted out of the chunk loop -- deconv3d_bf16s.hip, r05)
            int wv = __builtin_amdgcn_readfirstlane(wave);
            asm volatile("" : "+s"(wv));
#pragma unroll
            for (int k = 0; k < (KSTEPS * 2 + 3) / 4; ++k) {
                const int i = wv + 4 * k;                      // wave-uniform
                if (i < KSTEPS * 2)
                    lds_dma16(wres, &lds[WL + i * 64], wlane[0], (g0 + i / 2) * wstep + (i & 1) * 2 * Cout * 16);
            }
        }
        float in_scale = 1.f;
        if (F16) {
            if (bexp.advance(lds[ZSLOT + 1])) {
                const float ratio = bexp.rescale();
#pragma unroll
                for (int i = 0; i < MT * NT; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][r] *= ratio;
            }
            in_scale = bexp.in_scale();
        }
        // (a chunk of 8 live channels -- every chunk when Cin % 8 == 0 -- takes the copy of this loop without the
        // per-channel selects: 7 of its 32 VALU instructions per position, ISA count r03)
        auto stage = [&](auto whole_chunk) {
            constexpr bool WHOLE = decltype(whole_chunk)::value;
#pragma unroll
            for (int i = 0; i < C::NPOS; ++i) {
                const int p = tid + 256 * i;
                if (p >= C::CS) continue;
                unsigned hh[4], mm[4], ll[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float x0 = (WHOLE || 2 * c < nlive) ? rin[(2 * c) * C::NPOS + i] : 0.f;
                    const float x1 = (WHOLE || 2 * c + 1 < nlive) ? rin[(2 * c + 1) * C::NPOS + i] : 0.f;
                    if (F16) split2_pk_f16(x0 * in_scale, x1 * in_scale, hh[c], mm[c]);
                    else split3_pk(x0, x1, hh[c], mm[c], ll[c]);
                }
                lds[0 * C::CS + p] = make_uint4(hh[0], hh[1], hh[2], hh[3]);
                lds[1 * C::CS + p] = make_uint4(mm[0], mm[1], mm[2], mm[3]);
                if (NC == 3) lds[2 * C::CS + p] = make_uint4(ll[0], ll[1], ll[2], ll[3]);
            }
        };
        if (nlive == 8) stage(std::true_type{});
        else stage(std::false_type{});
        if (WLDS) __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0): the LDS-DMA weight loads have landed
        __syncthreads();
        const bool more = ci0 + 8 < Cin;                       // another chunk of THIS tile follows
        // what the K-steps prefetch: the next chunk of this tile, or (last chunk) the first chunk of the workgroup's next tile
        // (this tile's own offsets are not needed past this point: its last chunk is already staged)
        if constexpr (GATHER) {
            // second-to-last chunk: request the next tile's candidates / weights; last chunk: they have landed (every load of the
            // chunk in between was issued behind them) -- the prefetch below then gathers the next tile's first chunk
            if (more && ci0 + 16 >= Cin) gather_request(tile + (int)gridDim.x, gbuf ^ 1);
            if (!more) gather_offsets(tile + (int)gridDim.x, poff);
        } else if (!more) make_poff(tile + (int)gridDim.x, poff);          // pure index arithmetic under a wave-uniform branch
        nlive_next = more ? min(8, Cin - ci0 - 8) : min(8, Cin);
        int ch_next = more ? ci0 + 8 : 0;
        const bool second = CAT && ch_next >= csplit;          // workgroup-uniform: the prefetched chunk lies in the second tensor
        if (CAT && second) ch_next -= csplit;
        const unsigned nomore = (more || has_next) ? 0u : 0x80000000u;
        SS_STAMP_STEPS_BEGIN();
        // ACCB: the chunk's 14 x 3 MFMAs accumulate from ZERO in a second register set that is added to `acc` once per chunk
        // (two-level blocked summation).  One chain over all of K = Cin x 27 products rounds a growing partial sum 3 K / 16
        // times: measured 3.3e-7 ... 6.2e-7 of the output's rms for K = 864 ... 3456 against float64 (tools/err_stages.py),
        // 1.2 - 3.5x the fp32 CPU convolution of the reference, which sums in blocks too; chunk-blocked it is 1.9e-7 ... 2.3e-7
        // whatever K, at or below the CPU's.  Where the second set fits the register budget it costs no time (stride-2
        // forms 85.0 vs 85.5 us, the 1 x 4 tile 68.8 vs 68.2); the big 4-row layers would spill (+7 %) and keep the single chain.
        // (the 4-row tile: in PASSES passes of NR rows each, see acc_passes)
        static_assert(PASSES == 1 || (WLDS && MT == 1), "a second pass re-reads the weight fragments from LDS");
        f32x16 tacc[ACCB ? MT * NR : 1];

        // B fragments are read one row GROUP ahead of their MFMAs.  With RP = 2 the MFMAs of two rows
        // alternate so that no two consecutive ones share an accumulator (SS_ROW_PAIR; no gain measured).
        constexpr int RP = (NT >= 2) ? ((S == 2) ? SS_ROW_PAIR_S2 : SS_ROW_PAIR) : 1;
        static_assert(NR % RP == 0, "rows are processed in whole groups");
        uint4 bcur[RP][NC], bnxt[RP][NC];
        int hv = half;
        auto read_b = [&](uint4 (&dst)[NC], int s, int i) {
            const int ta = 2 * s, tb = 2 * s + 1;
            const int offa = ((ta / 9) * C::IH + (ta / 3) % 3) * C::IW + ta % 3;
            const int offb = (tb < C::KT) ? ((tb / 9) * C::IH + (tb / 3) % 3) * C::IW + tb % 3 : 0;
            // (LOCAL: the two-pass form derives the lane half's slot from `hv`, opaque once per K-step: as invariants of the chunk loop the 14
            // steps' fragment addresses were hoisted out of it, one register each, and then spilled)
            const int hf = LOCAL ? hv : half;
            const int slot = lane_pos + i * S * C::IW + (LOCAL ? offa + hf * (offb - offa) : (hf ? offb : offa));
#pragma unroll
            for (int c = 0; c < NC; ++c) dst[c] = lds[(tb >= C::KT && hf) ? ZSLOT : c * C::CS + slot];
        };
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
        const int rb = ps * NR;                                // first row of this pass
        if constexpr (LOCAL) asm volatile("" : "+v"(hv));
        if constexpr (ACCB) {
#pragma unroll
            for (int i = 0; i < MT * NR; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) tacc[i][r] = 0.f;
        }
#pragma unroll
        for (int r = 0; r < RP; ++r) read_b(bcur[r], 0, rb + r);
        if (WLDS) {
#pragma unroll
            for (int c = 0; c < NC; ++c) aq[0][0][c] = lds[WL + c * 64 + lane];
        }
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            // weight fragments two steps ahead, then this step's slice of the next chunk's input
            // No vector-memory instruction of the K loop sits under a branch: where control flow merges, the compiler's
            // wait-count pass cannot tell how many loads are younger than the one it waits for and falls back to
            // vmcnt(0/1) -- every K-step then waited for the input loads it had just issued (seen in the ISA).  Past the
            // end, the last fragment is requested again and the input loads get an offset beyond the buffer (no access).
            if constexpr (LOCAL) asm volatile("" : "+v"(hv));
            if (!WLDS) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int c = 0; c < NC; ++c) {              // (past the tile's last step: steps 0, 1, .. of the next tile)
                        const int gw_ = g0 + s + AP;
                        aq[(s + AP) % AR][mt][c] = load_a(gw_ < G ? gw_ : gw_ - G, c, mt);
                    }
            } else if (s + 1 < KSTEPS) {                       // next step's fragments from the LDS copy
#pragma unroll
                for (int c = 0; c < NC; ++c) aq[(s + 1) % AR][0][c] = lds[WL + ((s + 1) * 2 + c) * 64 + lane];
            }
            if (ps == 0)
#pragma unroll
            for (int q = s * QS; q < (s + 1) * QS && q < NQ; ++q)
                rin[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                       (CAT && second) ? ires2 : ires, (int)(poff[q % C::NPOS] | nomore), (ch_next + min(q / C::NPOS, max(nlive_next, 1) - 1)) * chan_b, 0));
            uint4 a[MT][NC];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int c = 0; c < NC; ++c) a[mt][c] = aq[s % AR][mt][c];
#pragma unroll
            for (int i0 = 0; i0 < NR; i0 += RP) {
#pragma unroll
                for (int r = 0; r < RP; ++r) {
                    if (i0 + RP < NR) read_b(bnxt[r], s, rb + i0 + RP + r);
                    else if (s + 1 < KSTEPS) read_b(bnxt[r], s + 1, rb + r);
                }
                // cross terms (a term, b term), smallest first; rows of the group alternate
                constexpr int NP = (NTERMS == 6) ? 6 : 3;
                constexpr int pa[6] = {1, 0, NC - 1, 0, 1, 0}, pb[6] = {1, NC - 1, 0, 1, 0, 0};
#pragma unroll
                for (int p = 6 - NP; p < 6; ++p)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int r = 0; r < RP; ++r) {
                            f32x16& dst = ACCB ? tacc[ACCB ? mt * NR + i0 + r : 0] : acc[mt * NT + rb + i0 + r];
                            if (F16)
                                dst = __builtin_amdgcn_mfma_f32_32x32x16_f16(
                                    __builtin_bit_cast(f16x8, a[mt][pa[p]]), __builtin_bit_cast(f16x8, bcur[r][pb[p]]), dst, 0, 0, 0);
                            else
                                dst = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                                    __builtin_bit_cast(bf16x8, a[mt][pa[p]]), __builtin_bit_cast(bf16x8, bcur[r][pb[p]]), dst, 0, 0, 0);
                        }
#pragma unroll
                for (int r = 0; r < RP; ++r)
#pragma unroll
                    for (int c = 0; c < NC; ++c) bcur[r][c] = bnxt[r][c];
                // pin the software pipeline: the next group's fragment reads are issued BEFORE this
                // group's MFMAs (the scheduler otherwise sinks them next to their use and every row
                // starts with an exposed LDS latency)
                __builtin_amdgcn_sched_group_barrier(0x100, NC * RP, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, NP * RP * MT, 0);
            }
            __builtin_amdgcn_sched_barrier(0);     // keep each step's loads inside the step
        }
        if constexpr (ACCB && PASSES > 1) {
#pragma unroll
            for (int i = 0; i < NR; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[rb + i][r] += tacc[i][r];
            // (the fold is pinned here: sunk towards the next use of `acc`, it kept this pass's second set alive through the next pass)
#pragma unroll
            for (int i = 0; i < NR; ++i) asm volatile("" : "+v"(acc[rb + i]));
        }
        }       // passes
        // steps 14 .. 14+AP-1 of this chunk are steps 0 .. AP-1 of the next: re-base the fragment ring
        if (!WLDS) {
            uint4 tq[AP][MT][NC];
#pragma unroll
            for (int k = 0; k < AP; ++k)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int c = 0; c < NC; ++c) tq[k][mt][c] = aq[(KSTEPS + k) % AR][mt][c];
#pragma unroll
            for (int k = 0; k < AP; ++k)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int c = 0; c < NC; ++c) aq[k][mt][c] = tq[k][mt][c];
        }
        if constexpr (ACCB && PASSES == 1) {
#pragma unroll
            for (int i = 0; i < MT * NT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][r] += tacc[i][r];
        }
        nlive = nlive_next;
        SS_STAMP_STEPS_END();
        if (GATHER && (more || has_next)) apply_att(more ? gbuf : gbuf ^ 1);
        if (F16 && (more || has_next)) publish_max(0.f);       // of the chunk staged next (its loads were issued >= 4 K-steps ago)
        __syncthreads();
    }

    SS_STAMP(2);
    if constexpr (HEAD) {
        int ow0, oh0, od0;
        tile_origin(tile, ow0, oh0, od0);
        const float hunscale = bexp.acc_unscale();
        const float hfloor = (relu & RELU_BIT) ? 0.f : -__builtin_inff();
        const bool colok = ow0 + l31 < Wo && od0 + dzw < Do;
        // ---- t[tap row][position] of this wave's rows: the accumulators become the B operand as they are ----
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const bool ok = colok && oh0 + hy0 + i < Ho;
            float y[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cl = (r & 3) + 8 * (r >> 2) + 4 * half;
                const float v = fmaxf(ss::add_rn(ss::mul_rn(acc[i][r] * (aff[128 + cl] * hunscale), aff[cl]), aff[64 + cl]), hfloor);
                y[r] = ok ? v : 0.f;            // positions outside the volume: the head's zero padding
            }
            f32x16 tt = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                unsigned bh[4], bm[4], bl[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) split3_pk(y[8 * ks + 2 * c], y[8 * ks + 2 * c + 1], bh[c], bm[c], bl[c]);
                const bf16x8 h8 = __builtin_bit_cast(bf16x8, make_uint4(bh[0], bh[1], bh[2], bh[3]));
                const bf16x8 m8 = __builtin_bit_cast(bf16x8, make_uint4(bm[0], bm[1], bm[2], bm[3]));
                const bf16x8 l8 = __builtin_bit_cast(bf16x8, make_uint4(bl[0], bl[1], bl[2], bl[3]));
                const bf16x8 ah = __builtin_bit_cast(bf16x8, lds[C::XS0 + (0 * 2 + ks) * 64 + lane]);
                const bf16x8 am = __builtin_bit_cast(bf16x8, lds[C::XS0 + (1 * 2 + ks) * 64 + lane]);
                const bf16x8 al = __builtin_bit_cast(bf16x8, lds[C::XS0 + (2 * 2 + ks) * 64 + lane]);
                tt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, m8, tt, 0, 0, 0);      // smallest cross terms first
                tt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, l8, tt, 0, 0, 0);
                tt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, h8, tt, 0, 0, 0);
                tt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, m8, tt, 0, 0, 0);
                tt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, h8, tt, 0, 0, 0);
                tt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, h8, tt, 0, 0, 0);
            }
            acc[i] = tt;                        // register 3 * ps + kh of this lane half: (kd, kw) pair ps + 5 * half, tap row kh
            __builtin_amdgcn_sched_barrier(0);  // one row at a time (all four interleaved: 43 spilled registers)
        }
        // ---- over kh, in registers: U[ps][ph] = sum_row t[row][3 ps + (row + 2 - ph)], ph = 0..5 the patch row (fixed order) ----
        float* ubuf = reinterpret_cast<float*>(lds);      // [10 pairs][6 patch rows][4 planes][32 columns], over the dead activation tile
        float* ub = ubuf + (5 * half * 6 * 4 + wave) * 32 + l31;      // (one per-lane address, the rest immediate offsets)
#pragma unroll
        for (int ps = 0; ps < 5; ++ps) {
#pragma unroll
            for (int ph = 0; ph < 6; ++ph) {
                float u = 0.f;
#pragma unroll
                for (int row = 0; row < 4; ++row) {
                    const int kh = row + 2 - ph;
                    if (kh >= 0 && kh < 3) u = ss::add_rn(u, acc[row][3 * ps + kh]);
                }
                ub[(ps * 6 + ph) * 4 * 32] = u;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        // ---- over (kd, kw): each thread owns patch positions q = tid + 256 i ----
        float* pout = out + ((size_t)b * ntiles + tile) * HEAD_PATCH;
        int ptid = tid;                // (opaque: the positions' index arithmetic is redone here per tile instead of living in registers -- or scratch -- through the K loop)
        asm volatile("" : "+v"(ptid));
#pragma unroll
        for (int i = 0; i < (HEAD_PATCH + 255) / 256; ++i) {
            const int q = ptid + 256 * i;
            if (q < HEAD_PATCH) {
                const int pw = q % 34, ph = (q / 34) % 6, pd = q / (34 * 6);
                // (all nine reads issued before the first add, from clamped -- always valid -- addresses: under a branch each the reads
                // were 37 dependent LDS round trips per thread)
                float uv[9];
#pragma unroll
                for (int kd = 0; kd < 3; ++kd)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const int pl = min(max(pd - 2 + kd, 0), 3), n = min(max(pw - 2 + kw, 0), 31);
                        uv[kd * 3 + kw] = ubuf[(((kd * 3 + kw) * 6 + ph) * 4 + pl) * 32 + n];
                    }
                float pv = 0.f;
#pragma unroll
                for (int kd = 0; kd < 3; ++kd)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const bool in = (unsigned)(pd - 2 + kd) < 4u && (unsigned)(pw - 2 + kw) < 32u;
                        pv = ss::add_rn(pv, in ? uv[kd * 3 + kw] : 0.f);
                    }
                pout[q] = pv;
            }
        }
        __syncthreads();               // the next tile's first chunk is staged over ubuf
    } else {
    set_outputs(tile);                 // (output addressing is derived here, not kept live through the K loop)
    // ---- epilogue: 32x32 D layout (col = lane & 31 = output column, row = channel, see cbase) ----
    // f16 form: 2^-(activation scale); the per-channel 2^-(weight scale) is stored behind the packed weights
    const float acc_unscale = bexp.acc_unscale();
    const float* obase = out + (size_t)b * Cout * Do * out_plane;
    const __amdgpu_buffer_rsrc_t ores = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(obase), 0, obytes, 0x00020000);
    // the residual: added after the affine, or (res_pre) a partial sum added before it
    const bool res_epi = residual != nullptr && !res_pre;
    const __amdgpu_buffer_rsrc_t rres = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(residual ? residual + (size_t)b * Cout * Do * out_plane : obase), 0, residual ? obytes : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t gres = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(GATED ? gate + (size_t)b * Cout * out_plane : obase), 0,
        GATED ? (int)min((long long)Cout * (long long)gchan_b, 0x7fffffffLL) : 0, 0x00020000);
    const float floor_v = (relu & RELU_BIT) ? 0.f : -__builtin_inff();
    // the side inputs (affine, gate, residual) of a group of EG fragment rows are fetched first so that their latencies
    // overlap instead of chaining; every group costs one exposed round trip (load -> store -> the next group's loads)
    // (the next tile's first chunk occupies the prefetch registers during the epilogue: with both a gate and a residual to
    // fetch, groups of 4 rows keep the kernel out of scratch)
    constexpr int EG = (GATED || NT * MT >= 4) ? 4 : 8;
    // (a workgroup whose 32 * MT channels all exist -- every one when Cout % 32 == 0 -- takes the copy of the epilogue without
    // the per-element "channel exists" selects on the load / store offsets: 4 of ~11 VALU instructions per element, ISA count r03)
    auto epilogue = [&](auto all_channels) {
    constexpr bool ALLC = decltype(all_channels)::value;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r0 = 0; r0 < 16; r0 += EG) {
        float sc[EG], sh[EG], un[EG], gv[EG][NT], rv[EG][NT];
#pragma unroll
        for (int q = 0; q < EG; ++q) {
            const int cb = cbase(mt, r0 + q);
            const bool cok = ALLC || cb + 4 * half < Cout;
            sc[q] = aff[cb - co0 + 4 * half];
            sh[q] = aff[64 + cb - co0 + 4 * half];
            un[q] = F16 ? aff[128 + cb - co0 + 4 * half] * acc_unscale : 1.0f;      // powers of two: acc * un is exact
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                if (GATED) gv[q][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                                      gres, (int)(cok ? vgate[i] : 0x80000000u), cb * (int)gchan_b, 0));
            }
        }
        if (residual != nullptr) {                             // one uniform branch per group, none per element
#pragma unroll
            for (int q = 0; q < EG; ++q) {
                const int cb = cbase(mt, r0 + q);
                const bool cok = ALLC || cb + 4 * half < Cout;
#pragma unroll
                for (int i = 0; i < NT; ++i)
                    rv[q][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                             rres, (int)(cok ? vout[i] : 0x80000000u), cb * (int)ochan_b, 0));
            }
        } else {
#pragma unroll
            for (int q = 0; q < EG; ++q)
#pragma unroll
                for (int i = 0; i < NT; ++i) rv[q][i] = 0.f;
        }
        float vv[EG][NT];
#pragma unroll
        for (int q = 0; q < EG; ++q) {
            const int r = r0 + q;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                float a0 = F16 ? acc[mt * NT + i][r] * un[q] : acc[mt * NT + i][r];
                if (res_pre) a0 = ss::add_rn(a0, rv[q][i]);                 // the partial sum of the same convolution
                float v = ss::add_rn(ss::mul_rn(a0, sc[q]), sh[q]);
                if (res_epi) v = ss::add_rn(v, rv[q][i]);
                v = fmaxf(v, floor_v);
                if (GATED) v = ss::mul_rn(gv[q][i], v);     // channelAtt gate, broadcast over D
                vv[q][i] = v;
            }
        }
        if (CAN_CL && out_cl) {
#pragma unroll
            for (int g4 = 0; g4 < EG; g4 += 4) {
                const int cb = cbase(mt, r0 + g4);           // channels cb + 4 * half .. + 3 sit in registers r0 + g4 .. + 3
                const bool cok = ALLC || cb + 4 * half < Cout;
#pragma unroll
                for (int i = 0; i < NT; ++i)
                    __builtin_amdgcn_raw_buffer_store_b128(
                        __builtin_bit_cast(u32x4_t, make_float4(vv[g4][i], vv[g4 + 1][i], vv[g4 + 2][i], vv[g4 + 3][i])), ores,
                        (int)(cok ? vout[i] : 0x80000000u), cb * 4, 0);
            }
        } else {
#pragma unroll
            for (int q = 0; q < EG; ++q) {
                const int cb = cbase(mt, r0 + q);
                const bool cok = ALLC || cb + 4 * half < Cout;
#pragma unroll
                for (int i = 0; i < NT; ++i)
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vv[q][i]), ores,
                                                          (int)(cok ? vout[i] : 0x80000000u), cb * (int)ochan_b, 0);
            }
        }
    }
    };
    if (co0 + 32 * MT * MS <= Cout) epilogue(std::true_type{});
    else epilogue(std::false_type{});
    }       // !HEAD
    SS_STAMP(3);
    }       // tiles of this workgroup (the next one's first chunk is already in the prefetch registers)
    SS_STAMP_FINISH();
}


// ---- host side: a launch's arguments by NAME (the entry points fill them), an instantiation by what it SETS ----
static_assert(ss::kNtermsF16 == F16X3, "conv_plan.h and split_f16.h name the same engine");
struct ConvArgs {
    const float* in = nullptr;                                  // [B,Cin,D,H,W]; gather form: the 2-D right feature map [B,Cin,H,W]; concat-free form: channels [0, csplit)
    const float* in_second_view = nullptr; int bsplit = 0;      // batch elements >= bsplit come from this tensor instead (ss_conv2d_bf16s_pair_fwd)
    const void* wsplit = nullptr;                               // ss_pack_conv{3d,2d}_weights_*
    const float *scale = nullptr, *shift = nullptr;             // the folded BatchNorm (null: 1 / 0)
    const float* residual = nullptr;                            // added after the affine, or (residual_is_partial_sum) before it
    const float* gate = nullptr;                                // channelAtt gate [B,Cout,H,W]
    float* out = nullptr;                                       // head form: the patch buffer
    const float *candidates = nullptr, *attention = nullptr;    // gather form: [B,D,H,W] each
    const void* head_weights = nullptr;                         // head form: ss_pack_classifier_head_weights
    const float *rem = nullptr, *rem_second_view = nullptr; int csplit = 0;      // concat-free form: channels [csplit, Cin)
    int B = 0, Cin = 0, D = 1, H = 0, W = 0, Cout = 0;          // the INPUT's extents (gather form: D = the number of candidates)
    hipStream_t stream = nullptr;  bool relu = false, residual_is_partial_sum = false, channels_last = false;
};

// One instantiation of conv3d_bf16s, named by what it sets: ConvForm<S, NT, TD, TH, NTERMS> is the plain form of a tile and each member
// returns the form with one thing changed -- ConvForm<1, 4, 4, 4, F16X3>{}.head().  Nobody else spells the thirteen positions.  The kernel's
// and BCfg's static_asserts are reached through launch_conv; the assert here holds the launchers' own rules.
template <int S_, int NT_, int TD_, int TH_, int NTERMS_, bool GATED_, int MT_, int KD_, int MS_, bool ACCB_, bool GATHER_, bool HEAD_, bool CAT_>
struct ConvFormT {
    static constexpr int S = S_, NT = NT_, TD = TD_, TH = TH_, NTERMS = NTERMS_, MT = MT_, KD = KD_, MS = MS_;
    static constexpr bool GATED = GATED_, ACCB = ACCB_, GATHER = GATHER_, HEAD = HEAD_, CAT = CAT_;
    static_assert((MT == 1 || S == 2) && (MS == 1 || (S == 2 && !GATED)), "two channel tiles per wave, split channels: stride 2 only; no gated split form (it would spill)");
    template <bool V = true> constexpr auto gated(ss::bool_c<V> = {}) const { return ConvFormT<S, NT, TD, TH, NTERMS, V, MT, KD, MS, ACCB, GATHER, HEAD, CAT>{}; }
    template <bool V = true> constexpr auto accb(ss::bool_c<V> = {}) const { return ConvFormT<S, NT, TD, TH, NTERMS, GATED, MT, KD, MS, V, GATHER, HEAD, CAT>{}; }
    template <bool V = true> constexpr auto cat(ss::bool_c<V> = {}) const { return ConvFormT<S, NT, TD, TH, NTERMS, GATED, MT, KD, MS, ACCB, GATHER, HEAD, V>{}; }
    constexpr auto gather() const { return ConvFormT<S, NT, TD, TH, NTERMS, GATED, MT, KD, MS, ACCB, true, HEAD, CAT>{}; }
    constexpr auto head() const { return ConvFormT<S, NT, TD, TH, NTERMS, GATED, MT, KD, MS, ACCB, GATHER, true, CAT>{}; }
    constexpr auto conv2d() const { return ConvFormT<S, NT, TD, TH, NTERMS, GATED, MT, 1, MS, ACCB, GATHER, HEAD, CAT>{}; }          // 3x3 over depth-1 volumes
    constexpr auto two_channel_tiles() const { return ConvFormT<S, NT, TD, TH, NTERMS, GATED, 2, KD, MS, ACCB, GATHER, HEAD, CAT>{}; }   // per wave (MT)
    // the waves split the workgroup's 64 channels (MS = 2): a wave is (row pair, 32 channels) and owns twice the rows
    constexpr auto split_channels() const { return ConvFormT<S, 2 * NT, TD, TH, NTERMS, GATED, MT, KD, 2, ACCB, GATHER, HEAD, CAT>{}; }
};
template <int S, int NT, int TD, int TH, int NTERMS>
using ConvForm = ConvFormT<S, NT, TD, TH, NTERMS, false, 1, 3, 1, false, false, false, false>;

// The ONE function that knows how the kernel's trailing parameters alias: `cand` carries the candidates (gather form), the packed
// head weights (head form) or rem (concat-free form), `catt` the attention weights or rem_second_view, `relu` the three booleans.
template <class F>
int launch_conv(F, const ConvArgs& a) {
    constexpr int S = F::S, TD = F::TD, TH = F::TH, KD = F::KD, MT = F::MT, MS = F::MS;
    // (fields the form cannot use stay null; channels-last output: the plain stride-1 3-D forms)
    SS_REQUIRE(F::GATED == (a.gate != nullptr) && (F::GATHER || (!a.candidates && !a.attention)) && (F::HEAD || !a.head_weights));
    SS_REQUIRE((F::CAT || (!a.rem && !a.rem_second_view && a.csplit == 0)) && (!F::HEAD || !a.residual));
    SS_REQUIRE(!a.channels_last || (!F::GATED && !F::HEAD && MT == 1 && S == 1 && KD == 3));
    const float* cand = F::GATHER ? a.candidates : (F::HEAD ? reinterpret_cast<const float*>(a.head_weights) : a.rem);
    const float* catt = F::GATHER ? a.attention : a.rem_second_view;
    const int relu = (a.relu ? RELU_BIT : 0) | (a.residual_is_partial_sum ? RES_PRE_BIT : 0) | (a.channels_last ? OUT_CL_BIT : 0);
    using C = BCfg<S, F::NT, TD, TH, KD, (F::NTERMS == 6) ? 3 : 2, wlds_form(S, F::NT, F::NTERMS, MT, KD, F::GATHER, F::ACCB) ? ((KD * 9 + 1) / 2) * 2 * 64 : 0, MS,
                   gather_slots(F::GATHER, S, TD, TH, KD) + (F::HEAD ? HEAD_WSLOTS : 0)>;
    const int Do = (a.D + 2 * (KD / 2) - KD) / S + 1, Ho = (a.H - 1) / S + 1, Wo = (a.W - 1) / S + 1;
    const int tiles_w = ss::ceil_div(Wo, 32), tiles_h = ss::ceil_div(Ho, TH), tiles_d = ss::ceil_div(Do, TD);
    const long long nt = (long long)tiles_w * tiles_h * tiles_d;
    if (nt > 0x7fffffffLL || a.B > 65535) return SS_ERR_UNSUPPORTED;
    auto kern = conv3d_bf16s<S, F::NT, TD, TH, F::NTERMS, F::GATED, MT, KD, MS, F::ACCB, F::GATHER, F::HEAD, F::CAT>;
    if (C::LDS_BYTES > 64 * 1024) {
        if (ss::ensure_dynamic_lds(reinterpret_cast<const void*>(kern), (int)C::LDS_BYTES) != SS_OK) return SS_ERR_LAUNCH;
    }
    // persistent workgroups: as many as the chip holds at once (2 - 4 per CU depending on the tile), each walking an equal
    // share of the tiles
    const int groups = ss::ceil_div(a.Cout, 32 * MT * MS) * a.B;
    const long long cap = std::max<long long>(1, ss::resident_workgroups(reinterpret_cast<const void*>(kern), 256, (int)C::LDS_BYTES) / groups);
    const long long rounds = ss::ceil_div_ll(nt, cap);
    const long long gx = ss::ceil_div_ll(nt, rounds);
    dim3 grid((unsigned)gx, ss::ceil_div(a.Cout, 32 * MT * MS), a.B);
    // (Workgroups of equal duration that all start together stay in lock-step -- every CU stages, multiplies and stores at
    // the same time.  Starting the first round's workgroups spread over 0.5-1.5 estimated lifetimes, in 2-16 groups, was
    // measured: no gain, -0 .. -8 %.)
    hipLaunchKernelGGL(kern, grid, dim3(256), C::LDS_BYTES, a.stream, a.in, reinterpret_cast<const uint4*>(a.wsplit), a.scale, a.shift,
                       a.residual, a.gate, a.out, a.Cin, a.D, a.H, a.W, a.Cout, Do, Ho, Wo, tiles_w, tiles_h, (int)nt, relu, cand, catt,
                       a.in_second_view, a.bsplit, a.csplit);
    return ss::check_launch();
}

// ---- runtime -> compile time (ss::with_bool / ss::with_int): exactly the instantiations that are built -- chunk-blocked accumulation
// in the fp16 form only, two channel tiles per wave at stride 2 only, no gated split-channel form ----
// the stride-1 tile candidates of ss::plan_conv3d as forms (a new candidate: one row there, one arm here)
template <int NTERMS, class Fn>
int with_stride1_tile(ss::Tile3 tile, Fn&& fn) {
    switch (tile) {
        case ss::Tile3::t4x4x32: return fn(ConvForm<1, 4, 4, 4, NTERMS>{});
        case ss::Tile3::t2x8x32: return fn(ConvForm<1, 4, 2, 8, NTERMS>{});
        case ss::Tile3::t1x8x32: return fn(ConvForm<1, 2, 1, 8, NTERMS>{});
        default: return fn(ConvForm<1, 1, 1, 4, NTERMS>{});
    }
}
// a 3-D tile with the layer's gate and accumulation
template <class Tile, class Fn>
int with_gate_and_accb(Tile tile, bool gated, bool accb, Fn&& fn) {
    return ss::with_bool(gated, [&](auto g) {
        if constexpr (Tile::NTERMS != F16X3) return fn(tile.gated(g));
        else return ss::with_bool(accb, [&](auto b) { return fn(tile.gated(g).accb(b)); });
    });
}

}  // namespace
