// The ONE statement of the conv launchers' tile and accumulation rule (conv3d_bf16s.hip, conv3d_gather.hip, conv3d_classifier.hip),
// of the transposed convs' form rule (deconv3d_bf16s.hip) and of the 3x3x3 weight gradients' kernel and partition rule (conv3d_wgrad_bf16s.hip):
// pure functions of integers, host-only, nothing from HIP.  Callers pass ss::fill_hint() and ss::tuning() in.
#pragma once
#ifndef SS_S2_MS_MIN_WGS
#define SS_S2_MS_MIN_WGS 256      // stride 2: fewest 64-channel workgroups for which the waves split the channels (below: one 32-channel tile per workgroup; 128 on the 128-workgroup layer: 29.5 vs 26.4 us)
#endif
// Chunk-blocked accumulation (ACCB of the kernel) is a property of the LAYER, never of the tile a launch happens to get: the
// tile candidates depend on the batch size, and a pair must get the same bits alone and in a batch
// (test_hot_segment_batch_invariance_at_the_sharded_batch_sizes).  fp16 form only.  It is on for every stride-2 layer, every
// 2-D layer, and the stride-1 3-D layers that at batch 1 are too small for the 4-row tile -- the deep, narrow layers with the
// longest K (conv2 / conv4 of the hourglasses: K = 1728 / 3456): there the second accumulator set fits the registers of the 1- and
// 2-row tiles they run on at small batch; when a larger batch -- or the fill hint of a pipelined call -- moves them onto the 4-row
// tile, that variant walks the chunk in two passes of two rows (acc_passes of conv3d_bf16s.h; one pass with a second set for all
// four rows spilled 15 - 46 registers).  The big 4-row layers (concat_stem, classif.0, hourglass2.conv2) keep the single chain.
#ifndef SS_ACC_BLOCKED
#define SS_ACC_BLOCKED 1                  // 0: single chains everywhere (tools/build_variant.sh, for A/B measurements)
#endif

namespace ss {
constexpr int kNtermsF16 = 19;            // the ABI's `nterms` code of the two-term fp16 form (F16X3 of split_f16.h)
constexpr long long kFillWgs = 512;       // workgroups of 32 channels x one tile that fill the chip (two on each of 256 CUs)
constexpr long long kFillWgsS2 = 256;     // ... of 64 channels x one 2 x 2 x 32 tile (stride 2, two channel tiles per wave)

// the stride-1 3-D tile candidates, planes x rows x columns (4, 4, 2, 1 rows per wave); stride 2 has one tile, 2 x 2 x 32, in three
// forms: the waves split the workgroup's 64 channels / two 32-channel tiles per wave / one
enum class Tile3 { t4x4x32, t2x8x32, t1x8x32, t1x4x32 };
enum class S2Form { split_channels, two_channel_tiles, one_channel_tile };
struct ConvPlan { Tile3 tile; bool accb; S2Form s2; };      // accb: chunk-blocked accumulation

// workgroups of a launch: td x th x 32 output tiles x tiles of `cpw` channels x batch elements -- what every threshold counts
constexpr long long blocks(int Do, int Ho, int Wo, int Cout, int B, int td, int th, int cpw = 32) {
    return (long long)((Wo + 31) / 32) * ((Ho + th - 1) / th) * ((Do + td - 1) / td) * ((Cout + cpw - 1) / cpw) * B;
}
// a layer too small for the 4-row tile at batch 1: decided by what ONE pair of it offers the chip, not by a launch's batch or tile
constexpr bool small_layer(int Do, int Ho, int Wo, int Cout) { return blocks(Do, Ho, Wo, Cout, 1, 2, 8) < kFillWgs; }

// (Do, Ho, Wo): the OUTPUT's extents; hint: pairs in flight on the chip beside this launch's own (ss::fill_hint()) -- the fill
// thresholds count their workgroups too; forced_tile: ss::tuning().conv_tile; s2_mt1: ss::tuning().conv_s2_mt1
constexpr ConvPlan plan_conv3d(int Do, int Ho, int Wo, int Cout, int B, int stride, int nterms, bool gated, int hint, int forced_tile, int s2_mt1) {
    // The tile is chosen for FILL: the largest whose workgroups still cover the chip.  A launch that shares the chip with other pairs'
    // launches (PairPipeline's lanes) is not alone in filling it: the hint scales the count by the pairs in flight.  Every tile
    // gives the same bits (the summation order is the layer's, see SS_ACC_BLOCKED), so the hint -- and a race on it -- changes speed only.
    int tile = (blocks(Do, Ho, Wo, Cout, B, 2, 8) * hint >= kFillWgs) ? 0 : ((blocks(Do, Ho, Wo, Cout, B, 1, 8) * hint >= kFillWgs) ? 1 : 2);
    if (forced_tile >= 0 && forced_tile <= 2) tile = forced_tile;
    // 4 planes x 4 rows: the most compact halo (6 x 6 x 34 = 1224 positions against 1360 for 2 x 8: -3 % time, 8 fewer
    // prefetch registers); 2 x 8 when the depth is not a multiple of 4
    const Tile3 t = tile == 0 ? (Do % 4 == 0 ? Tile3::t4x4x32 : Tile3::t2x8x32) : (tile == 1 ? Tile3::t1x8x32 : Tile3::t1x4x32);
    const bool accb = SS_ACC_BLOCKED && nterms == kNtermsF16 && (stride == 2 || small_layer(Do, Ho, Wo, Cout));
    // stride 2: two output tiles per wave (the activation staging is then shared: 154 vs 191 us on the largest layer)
    // unless that leaves fewer workgroups than CUs (57 vs 41 us on the smallest)
    // ... and, since r03, the 64 channels split over the waves (wave = (row pair, 32 channels)) instead of two channel
    // tiles per wave: the same MFMAs and staging with half the weight-fragment fetches (SS_CONV_S2_MT1=0: the r02 form)
    // (no layer gates a stride-2 conv; its split form would spill)
    const long long wg2 = blocks(Do, Ho, Wo, Cout, B, 2, 2, 64) * hint;
    const S2Form s2 = (Cout > 32 && wg2 >= SS_S2_MS_MIN_WGS && s2_mt1 < 0 && !gated) ? S2Form::split_channels
                    : (Cout > 32 && wg2 >= kFillWgsS2 && s2_mt1 <= 0)               ? S2Form::two_channel_tiles
                                                                                    : S2Form::one_channel_tile;
    return {t, accb, s2};
}

// the 2-D form (3x3 over [B,C,H,W] maps): rows of the 1 x rows x 32 tile (16, 8 or 4: 4, 2, 1 per wave), the first candidate that
// fills the chip; chunk-blocked accumulation on every 2-D layer of the fp16 form
constexpr int plan_conv2d_rows(int H, int W, int Cout, int B) {
    return blocks(1, H, W, Cout, B, 1, 16) >= kFillWgs ? 16 : (blocks(1, H, W, Cout, B, 1, 8) >= kFillWgs ? 8 : 4);
}
constexpr bool kConv2dAccb = SS_ACC_BLOCKED != 0;

// ---- the transposed 3-D convs (deconv3d_bf16s.hip): ConvTranspose3d(k3, s2, p1, op1) over an INPUT of (D, H, W) ----
// The tile is an input-space tile of planes x rows x 32 columns, one row per wave: 2 x 2 where the volume has two planes and
// fewer than four rows, 1 x 4 otherwise.
enum class DeconvTile { t2x2x32, t1x4x32 };
// groups (fp16 form only; the bf16 forms have one form, reported as groups 0 without streaming):
//   0: a workgroup computes all 8 output parity classes of its tile; 1: two workgroups per tile, one per class group
//   ({0, 1, 6, 7} and {2, 3, 4, 5}); 2: two class groups + chunk-blocked accumulation.
// stream: nontemporal stores of the output -- an instantiation of the groups-0 form only.
struct DeconvPlan { DeconvTile tile; int groups; bool stream; };
constexpr long long kDeconvFillUnits = 256;               // tiles x channel tiles of ONE pair from which all 8 classes share a workgroup
constexpr long long kDeconvStreamBytes = 192LL << 20;     // output bytes of a launch from which it is streamed

// forced_groups: ss::tuning().deconv_groups (SS_DECONV_GROUPS = 0 / 1 / 2, anything else: by layer size);
// forced_stream: ss::tuning().deconv_stream (SS_DECONV_STREAM = 0 / 1, negative: by output size)
constexpr DeconvPlan plan_deconv3d(int D, int H, int W, int Cout, int B, int nterms, int forced_groups, int forced_stream) {
    const DeconvTile tile = (D >= 2 && H < 4) ? DeconvTile::t2x2x32 : DeconvTile::t1x4x32;
    if (nterms != kNtermsF16) return {tile, 0, false};
    // Parity-class groups (r05, Grp<> of the kernel), measured alone on the four transposed convs of the 1024^2 pair (hourglass2.conv6 /
    // .conv5, hourglass_att.conv6 / .conv5; profiles/r05_f_deconv_forms.txt): all 8 classes per workgroup 128 / 55 / 38 / 39 us;
    // two class groups at three workgroups per CU 148 / 56 / 55 / 36; two groups + chunk-blocked accumulation 163 / 75 / 55 / 36.
    // The second staging of the input tile costs more than the third workgroup per CU returns wherever the layer fills the
    // chip; it pays -- and brings the blocked sum's accuracy -- on a layer whose tiles number fewer than the chip's CUs.
    // That is a property of the LAYER (tiles x channel tiles of ONE pair), so a pair gets the same bits at every batch size.
    // SS_DECONV_GROUPS=0 / 1 / 2 forces the form (2 = groups + chunk-blocked accumulation).
    const int td = tile == DeconvTile::t2x2x32 ? 2 : 1, th = tile == DeconvTile::t2x2x32 ? 2 : 4;
    const long long per_pair = blocks(D, H, W, Cout, 1, td, th);
    const int groups = (forced_groups >= 0 && forced_groups <= 2) ? forced_groups : (per_pair < kDeconvFillUnits ? 2 : 0);
    // Nontemporal stores (STREAM of the kernel), measured r05 on hourglass2.conv6 (201 MB written, alone): 128 -> 108 us
    // (profiles/r05_f_deconv_forms.txt).  Outputs of >= 192 MB per launch are streamed (the rule of the gwc volume kernel: smaller
    // outputs are handed to the next kernel by the 256 MB Infinity Cache); SS_DECONV_STREAM=0/1 forces it.
    const bool stream = forced_stream >= 0 ? forced_stream != 0 : (long long)B * Cout * 8 * D * H * W * 4 >= kDeconvStreamBytes;
    return {tile, groups, groups == 0 && stream};
}

// ---- the weight gradients of the 3x3x3 convs (conv3d_wgrad_bf16s.hip): which kernel, and how its K range (every output position, walked
// in chunks of kWgradChunk positions of one output row) is cut over the grid ----
#ifndef SS_COOP_WGS
#define SS_COOP_WGS 768           // cooperative stride-1 form: workgroups aimed at (~3 per CU) when a column of chunks is cut into segments
#endif
#ifndef SS_S2A_WGS
#define SS_S2A_WGS 256            // shared-gout stride-2 form: ONE workgroup per CU's worth of chunk ranges
#endif
constexpr int kWgradChunk = 32;           // output positions per chunk (two K-steps of 16)
enum class WgradKernel { coop, per_wave_s1, s2a, per_wave_s2, head };
// The fields a kernel does not launch by are 0.
//   every kernel: chunks_per_row, total_chunks (Do x Ho rows of chunks_per_row);  ci_tiles x co_tiles = tiles of 32 x 32 channels
//   per_wave_s1 / per_wave_s2: nsplit chunk ranges of per_unit chunks; the grid has ceil(nsplit / 8) * 24 blocks (split, kd) -> block
//                              ((split / 8) * 3 + kd) * 8 + split % 8, those with split >= nsplit leave
//   coop: a column (od, w0) of chunks is cut into nseg segments of seg_len output rows
//   s2a:  ns chunk ranges of pu chunks
//   head: nwaves waves of per_wave chunks, four to a workgroup
struct WgradPlan {
    WgradKernel kernel;
    int ci_tiles, tiles, chunks_per_row, total_chunks, per_unit, nsplit, nseg, seg_len, ns, pu, per_wave, nwaves;
};

constexpr long long cdiv(long long a, long long b) { return (a + b - 1) / b; }
constexpr long long imax(long long a, long long b) { return a > b ? a : b; }
constexpr long long imin(long long a, long long b) { return a < b ? a : b; }

// (D, H, W): the INPUT's extents (the output's are (N - 1) / stride + 1); coop: ss::tuning().wgrad_coop != 0.  The caller has checked
// that the chunk count fits an int.
constexpr WgradPlan plan_wgrad3d(int B, int Cin, int Cout, int D, int H, int W, int stride, bool coop) {
    const int Do = (D - 1) / stride + 1, Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    WgradPlan p{};
    p.ci_tiles = (int)cdiv(Cin, 32);
    p.tiles = p.ci_tiles * (int)cdiv(Cout, 32);
    p.chunks_per_row = (int)cdiv(Wo, kWgradChunk);
    const long long total = (long long)Do * Ho * p.chunks_per_row;
    p.total_chunks = (int)total;
    if (Cout == 1 && stride == 1 && coop) {
        // a single output channel: the taps as the matrix columns, ~2048 waves
        p.kernel = WgradKernel::head;
        const long long waves = imax(4, 2048 / ((long long)p.ci_tiles * B));
        p.per_wave = (int)imax(1, cdiv(total, waves));
        p.nwaves = (int)cdiv(total, p.per_wave);
        return p;
    }
    const int floor_chunks = p.chunks_per_row >= 4 ? 4 : 1;
    if (stride == 1 && coop) {
        // the cooperative form: a workgroup walks down a column (od, w0) of chunks, the columns cut into segments so that ~3 workgroups
        // per CU exist
        p.kernel = WgradKernel::coop;
        const long long cols = (long long)Do * p.chunks_per_row;
        const long long nseg = imin(imax(1, SS_COOP_WGS / imax(1, cols * p.tiles * B)), imax(1, Ho / 8));
        p.seg_len = (int)cdiv(Ho, nseg);
        p.nseg = (int)cdiv(Ho, p.seg_len);
    } else if (stride == 2 && coop) {
        // stride 2 with the gout chunk shared: a workgroup = the nine kernel rows of a chunk range; ONE workgroup per CU's worth of ranges (each
        // ends with 27 648 atomics into the workspace: 768 ranges 234 us, 256 ranges 203, 3072 ranges 368 on hourglass.conv1's layer)
        p.kernel = WgradKernel::s2a;
        const long long ns = imax(1, SS_S2A_WGS / ((long long)p.tiles * B));
        p.pu = (int)imax(floor_chunks, cdiv(total, ns));
        p.ns = (int)cdiv(total, p.pu);
    } else {
        // one wave = one unit (kernel-depth plane, kernel row, tile pair, batch element, chunk range): ~12 waves per CU on 256 CUs
        p.kernel = stride == 1 ? WgradKernel::per_wave_s1 : WgradKernel::per_wave_s2;
        const long long nsplit = imax(1, 3072 / (9LL * p.tiles * B));
        p.per_unit = (int)imax(floor_chunks, cdiv(total, nsplit));
        p.nsplit = (int)cdiv(total, p.per_unit);
    }
    return p;
}
}  // namespace ss
