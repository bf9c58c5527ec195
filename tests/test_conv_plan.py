"""The conv launchers' tile and accumulation rule (semstereo_amd/csrc/conv_plan.h), checked on the CPU: a probe of a few lines around the
header is compiled with the system c++ and called through ctypes.

  * chunk-blocked accumulation (what decides the summation order, hence the bits) depends on the LAYER alone: not on the batch, the
    fill hint or a forced tile;
  * the Python restatements of the rule in the GPU tests (_rule of tests/test_fill_hint_gpu.py; _s1_form, _s2_form, _stem_form,
    _conv2d_tile of tests/test_f16_ranges_gpu.py) and engine.classifier_fused_applies give the header's answers;
  * both sides of every threshold, the forced tile, the depth rule of the 4-row tile, one plan for the plain and the gather entry;
  * the transposed convs' form rule (ss::plan_deconv3d, what deconv3d_bf16s.hip launches by): its restatement _deconv_form of
    tests/test_f16_ranges_gpu.py on a grid across every threshold and every value of SS_DECONV_GROUPS and SS_DECONV_STREAM, and the
    forms of the four transposed convs of the 1024^2 pair;
  * the weight gradients' kernel and partition rule (ss::plan_wgrad3d, what conv3d_wgrad_bf16s.hip launches by): its restatement
    _wgrad_form of tests/test_wgrad_forms_gpu.py on a grid across every threshold, on every case of that file and on the
    CONV_TRAIN_CASES of tests/test_parity_gpu.py.
"""
import ctypes
import itertools
import os
import subprocess

import pytest
import torch

import test_f16_ranges_gpu as fr
import test_fill_hint_gpu as fh
import test_parity_gpu as tp
import test_wgrad_forms_gpu as wf

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "semstereo_amd", "csrc")
PROBE = """
#include "conv_plan.h"
extern "C" {
long long probe_blocks(int Do, int Ho, int Wo, int Cout, int B, int td, int th) { return ss::blocks(Do, Ho, Wo, Cout, B, td, th); }
void probe_plan3d(int Do, int Ho, int Wo, int Cout, int B, int stride, int nterms, int gated, int hint, int forced, int mt1, int* out) {
    const ss::ConvPlan p = ss::plan_conv3d(Do, Ho, Wo, Cout, B, stride, nterms, gated != 0, hint, forced, mt1);
    out[0] = (int)p.tile; out[1] = p.accb; out[2] = (int)p.s2;
}
int probe_rows2d(int H, int W, int Cout, int B) { return ss::plan_conv2d_rows(H, W, Cout, B); }
int probe_small_layer(int D, int H, int W, int Cout) { return ss::small_layer(D, H, W, Cout); }
int probe_s2_min_wgs() { return SS_S2_MS_MIN_WGS; }
void probe_deconv3d(int D, int H, int W, int Cout, int B, int nterms, int forced_groups, int forced_stream, int* out) {
    const ss::DeconvPlan p = ss::plan_deconv3d(D, H, W, Cout, B, nterms, forced_groups, forced_stream);
    out[0] = p.tile == ss::DeconvTile::t2x2x32 ? 2 : 1; out[1] = p.tile == ss::DeconvTile::t2x2x32 ? 2 : 4; out[2] = p.groups; out[3] = p.stream;
}
long long probe_deconv_stream_bytes() { return ss::kDeconvStreamBytes; }
void probe_wgrad3d(int B, int Cin, int Cout, int D, int H, int W, int stride, int coop, int* out) {
    const ss::WgradPlan p = ss::plan_wgrad3d(B, Cin, Cout, D, H, W, stride, coop != 0);
    const int v[13] = {(int)p.kernel, p.ci_tiles, p.tiles, p.chunks_per_row, p.total_chunks, p.per_unit, p.nsplit, p.nseg, p.seg_len, p.ns, p.pu,
                       p.per_wave, p.nwaves};
    for (int i = 0; i < 13; ++i) out[i] = v[i];
}
int probe_wgrad_constant(int which) { return which == 0 ? SS_COOP_WGS : (which == 1 ? SS_S2A_WGS : ss::kWgradChunk); }
}
"""
TILES = ("4x4x32", "2x8x32", "1x8x32", "1x4x32")          # enum Tile3
S2FORMS = ("split", "two_tiles", "one_tile")              # enum S2Form, under the names the GPU tests use
CANDIDATE = {"4x4x32": 0, "2x8x32": 0, "1x8x32": 1, "1x4x32": 2}      # SS_CONV_TILE's number of a tile
BATCHES, HINTS, FORCED = (1, 2, 4, 8), (1, 3, 6, 64), (-1, 0, 1, 2)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("conv_plan")
    src, so = d / "probe.cpp", d / "probe.so"
    src.write_text(PROBE)
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    lib.probe_blocks.restype = ctypes.c_longlong
    lib.probe_deconv_stream_bytes.restype = ctypes.c_longlong
    return lib


def _out(dhw, stride):
    return tuple((n - 1) // stride + 1 for n in dhw)


def plan(lib, out_dhw, cout, B=1, stride=1, nterms=19, gated=False, hint=1, forced=-1, mt1=-1):
    """-> (tile name, accb, stride-2 form name)"""
    r = (ctypes.c_int * 3)()
    lib.probe_plan3d(*out_dhw, cout, B, stride, nterms, int(gated), hint, forced, mt1, r)
    return TILES[r[0]], bool(r[1]), S2FORMS[r[2]]


def _layers():
    """(Cout, input (D, H, W), stride) of every stride-1 and stride-2 shape the GPU tests of the rule run"""
    cases = [(c[1], c[2], c[3]) for c in fh.CASES.values()] + [(c[1], c[2], 1) for c in fr.S1_SHAPES.values()]
    return cases + [(fr.S2_SHAPE[1], fr.S2_SHAPE[2], 2), (fr.LARGE_S1[1], fr.LARGE_S1[2], 1)]


def test_accumulation_is_the_layers_not_the_launchs(probe):
    for cout, dhw, stride in _layers():
        got = {plan(probe, _out(dhw, stride), cout, B, stride, hint=h, forced=f, mt1=m)[1]
               for B, h, f, m in itertools.product(BATCHES, HINTS, FORCED, (-1, 0, 1))}
        want = stride == 2 or fr._s1_form(cout, dhw, 0)[2]
        assert got == {want}, (cout, dhw, stride, got)
        for nterms in (3, 6):                   # the bf16 engines have no chunk-blocked form
            assert not plan(probe, _out(dhw, stride), cout, 1, stride, nterms=nterms)[1]


def test_python_restatements_give_the_headers_answers(probe):
    for case in fh.CASES.values():
        _cin, cout, dhw, stride = case
        for hint, B in itertools.product(sorted(set(fh.HINTS + HINTS)), (1, 2)):
            tile, _accb, s2 = plan(probe, _out(dhw, stride), cout, B, stride, hint=hint)
            assert fh._rule(case, hint, B) == (CANDIDATE[tile] if stride == 1 else s2), (case, hint, B)
    for (_cin, cout, dhw), B, forced in itertools.product(list(fr.S1_SHAPES.values()) + [fr.LARGE_S1], (1, 4), (0, 1, 2)):
        tile, accb, _ = plan(probe, dhw, cout, B, forced=forced)
        rows, (td, th), want_accb = fr._s1_form(cout, dhw, forced, B)
        assert (tile, accb) == (f"{td}x{th}x32", want_accb) and rows == {0: 4, 1: 2, 2: 1}[forced]
    for hint, mt1, B in itertools.product(HINTS, (-1, 0, 1), (1, 2)):
        _cin, cout, dhw = fr.S2_SHAPE
        assert plan(probe, _out(dhw, 2), cout, B, 2, hint=hint, mt1=mt1)[2] == fr._s2_form(cout, dhw, hint, mt1, B)
    for B, C, nd, H, W, forced in fr.STEM:
        tile, accb, _ = plan(probe, (nd, H, W), C, B, forced=-1 if forced is None else forced)
        (td, th), want_accb = fr._stem_form(B, C, nd, H, W, forced)
        assert (tile, accb) == (f"{td}x{th}x32", want_accb)
    for B, _cs, _cin, cout, H, W in fr.CAT_SHAPES:
        assert probe.probe_rows2d(H, W, cout, B) == (16, 8, 4)[fr._conv2d_tile(B, cout, H, W)]


def test_both_sides_of_every_threshold(probe):
    # blocks(2, 8) x hint = 511 | 512: 7 x 73 x 1 tiles | 8 x 64 x 1, and 73 tiles x 7 pairs in flight | 64 x 8
    below, at = (2, 8 * 73, 32 * 7), (2, 8 * 64, 32 * 8)
    assert probe.probe_blocks(*below, 32, 1, 2, 8) == 511 and probe.probe_blocks(*at, 32, 1, 2, 8) == 512
    assert plan(probe, below, 32) == ("1x8x32", True, "one_tile") and plan(probe, at, 32)[:2] == ("2x8x32", False)
    assert plan(probe, (2, 8 * 73, 32), 32, hint=7)[0] == "1x8x32" and plan(probe, (2, 8 * 64, 32), 32, hint=8)[0] == "2x8x32"
    assert plan(probe, (2, 8 * 73, 32), 32, B=7)[:2] == ("1x8x32", True) and plan(probe, (2, 8 * 64, 32), 32, B=8)[:2] == ("2x8x32", True)
    assert bool(probe.probe_small_layer(*below, 32)) and not probe.probe_small_layer(*at, 32)
    # blocks(1, 8) x hint = 511 | 512 with blocks(2, 8) below 512
    below, at = (1, 8 * 73, 32 * 7), (2, 8 * 32, 32 * 8)
    assert probe.probe_blocks(*below, 32, 1, 1, 8) == 511 and probe.probe_blocks(*at, 32, 1, 1, 8) == 512
    assert probe.probe_blocks(*at, 32, 1, 2, 8) == 256
    assert plan(probe, below, 32)[0] == "1x4x32" and plan(probe, at, 32)[0] == "1x8x32"
    # stride 2, OUTPUT extents: 17 x 5 x 3 = 255 workgroups of 64 channels | 8 x 8 x 4 = 256
    assert probe.probe_s2_min_wgs() == 256
    below, at = (34, 10, 96), (16, 16, 128)
    for mt1 in (-1, 0, 1):
        assert plan(probe, below, 64, stride=2, mt1=mt1)[2] == "one_tile"
    assert [plan(probe, at, 64, stride=2, mt1=m)[2] for m in (-1, 0, 1)] == ["split", "two_tiles", "one_tile"]
    assert plan(probe, (34, 10, 32), 64, stride=2, hint=3)[2] == "one_tile" and plan(probe, (16, 16, 32), 64, stride=2, hint=4)[2] == "split"
    assert plan(probe, at, 32, stride=2)[2] == "one_tile"                     # one channel tile: nothing to split or pair
    assert plan(probe, at, 64, stride=2, gated=True)[2] == "two_tiles"        # no gated split-channel form
    # the 2-D form: 16, 8 or 4 rows, no hint
    assert probe.probe_rows2d(16 * 64, 32 * 8, 32, 1) == 16 and probe.probe_rows2d(16 * 73, 32 * 7, 32, 1) == 8
    assert probe.probe_rows2d(8 * 73, 32 * 7, 32, 1) == 4 and probe.probe_rows2d(8 * 64, 32 * 8, 32, 1) == 8


def test_forced_tile_overrides_the_count_and_depth_picks_the_four_row_tile(probe):
    big, small = (8, 512, 512), (4, 16, 64)
    assert plan(probe, big, 32)[0] == "4x4x32" and plan(probe, small, 32)[0] == "1x4x32"
    assert [plan(probe, big, 32, forced=f)[0] for f in (0, 1, 2, 3, -1)] == ["4x4x32", "1x8x32", "1x4x32", "4x4x32", "4x4x32"]
    assert [plan(probe, small, 32, forced=f)[0] for f in (0, 1, 2, 3)] == ["4x4x32", "1x8x32", "1x4x32", "1x4x32"]
    for depth, tile in ((4, "4x4x32"), (6, "2x8x32"), (7, "2x8x32"), (24, "4x4x32")):
        assert plan(probe, (depth, 512, 512), 32)[0] == tile and plan(probe, (depth, 16, 64), 32, forced=0)[0] == tile


def test_plain_and_gather_entry_get_one_plan(probe):
    """ss_conv3d_bf16s_fwd passes the output extents of its stride-1 input, ss_conv3d_gather_fwd (candidates, H, W): the same numbers"""
    stems = [(B, 32, 24, 256, 256) for B in (1, 4)] + [s[:5] for s in fr.STEM]       # concat_stem at quarter resolution of 1024^2
    for (B, C, nd, H, W), hint, forced, gated in itertools.product(stems, HINTS, FORCED, (False, True)):
        assert plan(probe, _out((nd, H, W), 1), C, B, hint=hint, forced=forced, gated=gated) == \
            plan(probe, (nd, H, W), C, B, hint=hint, forced=forced, gated=gated)
    for B in (1, 4):
        assert plan(probe, (24, 256, 256), 32, B)[:2] == ("4x4x32", False)


class _Volume:
    """what engine.classifier_fused_applies reads of a tensor"""
    is_cuda, dtype = True, torch.float32

    def __init__(self, *shape):
        self.shape = shape

    def dim(self):
        return len(self.shape)


def test_classifier_rule_is_the_engines_arithmetic(probe):
    from semstereo_amd import engine
    # (B, D, H, W) of tests/test_parity_gpu.py and tests/test_f16_ranges_gpu.py, the layer below 512 of the former, 510 | 512 tiles (4 planes: an even count),
    # and the small maps of the heads' HEAD_SHAPES as 4-, 12- and 24-plane volumes
    shapes = [(1, 12, 134, 200), (2, 8, 140, 250), (1, 4, 300, 260), (1, 32, 128, 128), (1, 24, 256, 256), (2, 36, 128, 160),
              (8, 8, 64, 64), (1, 4, 8 * 17, 32 * 15), (1, 4, 8 * 16, 32 * 16), (3, 12, 134, 200)]
    shapes += [(1, D, H, W) for (_c, H, W), D in itertools.product(fr.HEAD_SHAPES, (4, 12, 24))]
    served = []
    for B, D, H, W in shapes:
        assert D % 4 == 0
        want = engine.classifier_fused_applies(_Volume(B, 32, D, H, W), 19)
        assert want == (not probe.probe_small_layer(D, H, W, 32)), (B, D, H, W)
        served.append(want)
    assert served[:10] == [True] * 6 + [False, False, True, True] and not any(served[10:])


# --------------------------------------------------------------------------------------------------------------------
# the transposed convs: ss::plan_deconv3d
# --------------------------------------------------------------------------------------------------------------------

def deconv_plan(lib, D, H, W, cout, B=1, nterms=19, groups=-1, stream=-1):
    """-> ((planes, rows) of the tile, groups, stream), the form of fr._deconv_form's answer"""
    r = (ctypes.c_int * 4)()
    lib.probe_deconv3d(D, H, W, cout, B, nterms, groups, stream, r)
    return (r[0], r[1]), r[2], bool(r[3])


def _per_pair(D, H, W, cout):
    (td, th), _, _ = fr._deconv_form(D, H, W, cout)
    return fr._cdiv(W, 32) * fr._cdiv(H, th) * fr._cdiv(D, td) * fr._cdiv(cout, 32)


# (D, H, W, Cout, B) either side of each threshold.  per_pair = 255 | 256: 1 x 4 tile 5 x 17 x 3 tiles x 1 | 4 x 16 x 4 x 1 (and by the
# channel tiles: 1 x 5 x 17 x 3 | 2 x 16 x 4 x 2), 2 x 2 tile (H < 4, D >= 2) 17 x 1 x 15 x 1 | 16 x 2 x 8 x 1 (and 17 x 1 x 3 x 5 | 16 x 1 x 16 x 1); H = 3 | 4 and D = 1 | 2 move the tile;
# the output, B Cout 8 D H W 4 bytes: 192 MB = 2^21 x 96, so Cout 32 x D 12 x H 128 x W 128 is AT it, W = 127 below, and B counts
DECONV_EDGES = [(5, 68, 96, 32, 1), (4, 64, 128, 32, 1), (17, 20, 32, 96, 1), (4, 64, 64, 64, 1), (4, 64, 64, 33, 1),
                (30, 2, 17 * 32, 32, 1), (16, 3, 16 * 32, 32, 1), (32, 2, 16 * 32 - 31, 32, 1), (6, 2, 17 * 32, 160, 1),
                (2, 3, 64, 32, 1), (2, 4, 64, 32, 1), (1, 3, 64, 32, 1), (1, 4, 64, 32, 1), (3, 1, 5, 8, 2), (1, 1, 1, 1, 1),
                (12, 128, 128, 32, 1), (12, 128, 127, 32, 1), (6, 128, 128, 32, 2), (6, 128, 127, 32, 2), (12, 128, 128, 31, 1),
                (6, 128, 128, 32, 1), (3, 128, 128, 32, 4), (3, 128, 128, 32, 3), (8, 32, 32, 64, 12), (8, 32, 32, 64, 11)]


def test_deconv_restatement_gives_the_headers_answers(probe):
    shapes = list(DECONV_EDGES)
    shapes += [(D, H, W, cout, B) for D, H, W, cout, B in itertools.product((1, 2, 3, 16), (1, 3, 4, 9, 64), (1, 33, 64, 512), (1, 32, 33, 64, 128), (1, 2))]
    for (D, H, W, cout, B), nterms, groups, stream in itertools.product(shapes, (19, 6, 3), (-1, 0, 1, 2, 3), (-1, 0, 1)):
        assert deconv_plan(probe, D, H, W, cout, B, nterms, groups, stream) == fr._deconv_form(D, H, W, cout, B, nterms, groups, stream), \
            (D, H, W, cout, B, nterms, groups, stream)


def test_deconv_both_sides_of_every_threshold(probe):
    # per_pair 255 | 256, each tile: groups 2 | 0, at every batch size (the LAYER's property) and whatever the stream switch says
    for below, at, tile in (((5, 68, 96, 32), (4, 64, 128, 32), (1, 4)), ((17, 20, 32, 96), (4, 64, 64, 64), (1, 4)),
                            ((30, 2, 17 * 32, 32), (16, 3, 16 * 32, 32), (2, 2)), ((6, 2, 17 * 32, 160), (32, 2, 16 * 32 - 31, 32), (2, 2))):
        assert (_per_pair(*below), _per_pair(*at)) == (255, 256)
        for B, stream in ((1, -1), (2, -1), (1, 0), (2, 0), (8, 0)):         # (at B = 8 the larger of these would stream by its size)
            assert deconv_plan(probe, *below, B, stream=stream) == (tile, 2, False) and deconv_plan(probe, *at, B, stream=stream) == (tile, 0, False)
        assert deconv_plan(probe, *at, 1, stream=1) == (tile, 0, True) and deconv_plan(probe, *below, 1, stream=1) == (tile, 2, False)
    assert deconv_plan(probe, 4, 64, 64, 33)[1] == 0 and deconv_plan(probe, 4, 64, 64, 32)[1] == 2      # 128 tiles: the 33rd channel opens a second channel tile
    # the tile: 2 x 2 needs two planes AND fewer than four rows
    assert [deconv_plan(probe, D, H, 64, 32)[0] for D, H in ((2, 3), (2, 4), (1, 3), (1, 4), (3, 1), (1, 1))] == [(2, 2), (1, 4), (1, 4), (1, 4), (2, 2), (1, 4)]
    # output bytes, integers only: B x Cout x 8 D H W x 4 at 192 MB | one column less
    edge = probe.probe_deconv_stream_bytes()
    assert edge == 192 << 20
    for (D, H, W, cout, B), streams in (((12, 128, 128, 32, 1), True), ((12, 128, 127, 32, 1), False), ((6, 128, 128, 32, 2), True),
                                        ((6, 128, 127, 32, 2), False), ((6, 128, 128, 32, 1), False), ((3, 128, 128, 32, 4), True),
                                        ((3, 128, 128, 32, 3), False), ((12, 128, 128, 31, 1), False)):
        nbytes = B * cout * 8 * D * H * W * 4
        assert (nbytes >= edge) == streams and (B * cout * D * H * W != 32 * 12 * 128 * 128 or nbytes == edge)
        assert _per_pair(D, H, W, cout) >= 256
        assert deconv_plan(probe, D, H, W, cout, B) == ((1, 4), 0, streams)
        assert deconv_plan(probe, D, H, W, cout, B, stream=0)[2] is False and deconv_plan(probe, D, H, W, cout, B, stream=1)[2] is True
    # a streamed size on the two-group forms: they have no streaming instantiation
    assert _per_pair(8, 32, 32, 64) == 128 and 12 * 64 * 8 * 8 * 32 * 32 * 4 == edge
    assert deconv_plan(probe, 8, 32, 32, 64, 12) == ((1, 4), 2, False) and deconv_plan(probe, 8, 32, 32, 64, 12, groups=1) == ((1, 4), 1, False)
    assert deconv_plan(probe, 8, 32, 32, 64, 12, groups=0) == ((1, 4), 0, True) and deconv_plan(probe, 8, 32, 32, 64, 11, groups=0) == ((1, 4), 0, False)
    # every forced value of both switches, on a layer either side of the count; 3 and beyond: as unset
    for shape, natural in (((2, 3, 5, 64), 2), ((16, 32, 64, 32), 0)):
        assert _per_pair(*shape) < 256 if natural == 2 else _per_pair(*shape) >= 256
        for groups, stream in itertools.product((-1, 0, 1, 2, 3), (-1, 0, 1)):
            want = groups if groups in (0, 1, 2) else natural
            assert deconv_plan(probe, *shape, 1, groups=groups, stream=stream)[1:] == (want, want == 0 and stream == 1)
        for nterms in (6, 3):               # the bf16 forms: one form, no switch
            assert {deconv_plan(probe, *shape, 1, nterms, g, s)[1:] for g, s in itertools.product((-1, 0, 1, 2), (-1, 0, 1))} == {(0, False)}


def test_deconv_forms_of_the_1024_pair(probe):
    """the four transposed convs of the 1024^2 / maxdisp 128 pair (input D, H, W, Cout; tools/run_kernel.py builds the same): all 8
    classes per workgroup wherever the layer fills the chip, hourglass2.conv6 streamed (192 MB written at batch 1), the 128-unit
    hourglass_att.conv5 on two class groups with chunk-blocked accumulation -- at every batch size"""
    layers = {"hourglass2.conv6": ((12, 128, 128, 32), 1536, 0), "hourglass2.conv5": ((6, 64, 64, 64), 384, 0),
              "hourglass_att.conv6": ((16, 64, 64, 32), 512, 0), "hourglass_att.conv5": ((8, 32, 32, 64), 128, 2)}
    for name, (shape, units, groups) in layers.items():
        assert _per_pair(*shape) == units, name
        for B in (1, 2, 4):
            D, H, W, cout = shape
            streams = groups == 0 and B * cout * 8 * D * H * W * 4 >= 192 << 20
            assert deconv_plan(probe, *shape, B) == ((1, 4), groups, streams), (name, B)
    assert deconv_plan(probe, 12, 128, 128, 32, 1)[2] and not deconv_plan(probe, 6, 64, 64, 64, 1)[2]
    assert deconv_plan(probe, 6, 64, 64, 64, 4)[2] and not deconv_plan(probe, 8, 32, 32, 64, 64)[2]


# --------------------------------------------------------------------------------------------------------------------
# the 3x3x3 weight gradients: ss::plan_wgrad3d
# --------------------------------------------------------------------------------------------------------------------

WGRAD_KERNELS = ("coop", "per_wave_s1", "s2a", "per_wave_s2", "head")         # enum WgradKernel, under the names _wgrad_form uses
WGRAD_FIELDS = ("kernel", "ci_tiles", "tiles", "chunks_per_row", "total_chunks", "per_unit", "nsplit", "nseg", "seg_len", "ns", "pu", "per_wave", "nwaves")


def wgrad_plan(lib, B, Cin, Cout, D, H, W, stride, coop=True):
    """-> the dict of wf._wgrad_form"""
    r = (ctypes.c_int * 13)()
    lib.probe_wgrad3d(B, Cin, Cout, D, H, W, stride, int(coop), r)
    return dict(zip(WGRAD_FIELDS, (WGRAD_KERNELS[r[0]],) + tuple(r[1:])))


# (B, Cin, Cout, D, H, W, stride) either side of each threshold of the rule:
#   Cout 1 | 2 (the head kernel);  Wo 96 | 97 (three | four chunks per row: the floor of 4 chunks per range), at stride 2 W 192 | 193;
#   per-wave: 3072 / (9 tiles B) = 341 ranges at one tile: 341 | 342 chunks (ranges of 1 | 2), 170 at two tiles, 0 -> 1 from 342 tiles x pairs;
#   cooperative: 768 / (columns x tiles x B) against Ho / 8: 384 | 385 columns (2 | 1 segments), 768 | 769, Ho 15 | 16 | 17 | 24;
#   shared gout: 256 / (tiles B) ranges: 256 | 257 chunks, 128 | 129 at two tiles, 0 -> 1 from 257 tiles x pairs;
#   head: 2048 / (ci_tiles B) waves, at least 4: 2048 | 2049 chunks, B = 512 | 513, two channel tiles
WGRAD_EDGES = [(1, 32, 1, 2, 3, 32, 1), (1, 32, 2, 2, 3, 32, 1), (1, 32, 1, 2, 3, 32, 2), (1, 32, 32, 1, 4, 96, 1), (1, 32, 32, 1, 4, 97, 1),
               (1, 32, 32, 2, 4, 192, 2), (1, 32, 32, 2, 4, 193, 2), (1, 32, 32, 11, 31, 32, 1), (1, 32, 32, 9, 38, 32, 1), (1, 32, 33, 10, 17, 32, 1),
               (1, 32, 33, 9, 19, 32, 1), (342, 32, 32, 2, 2, 32, 1), (341, 32, 32, 2, 2, 32, 1), (1, 32, 32, 12, 16, 32 * 32, 1),
               (1, 32, 32, 11, 16, 32 * 35, 1), (1, 32, 32, 24, 64, 32 * 32, 1), (1, 32, 32, 769, 64, 32, 1), (1, 32, 32, 2, 15, 64, 1),
               (1, 32, 32, 2, 16, 64, 1), (1, 32, 32, 2, 17, 64, 1), (1, 32, 32, 2, 24, 64, 1), (1, 32, 32, 31, 16, 64, 2), (1, 32, 32, 2, 257 * 2, 64, 2),
               (1, 32, 64, 16, 16, 64, 2), (1, 32, 64, 2, 129 * 2, 64, 2), (128, 32, 32, 2, 8, 64, 2), (129, 32, 32, 2, 8, 64, 2), (170, 32, 32, 2, 2, 32, 1), (171, 32, 32, 2, 2, 32, 1),
               (1, 32, 1, 32, 64, 32, 1), (1, 32, 1, 1, 2049, 32, 1), (512, 32, 1, 1, 5, 32, 1), (513, 32, 1, 1, 5, 32, 1), (1, 64, 1, 16, 64, 32, 1),
               (1, 64, 1, 1, 1025, 32, 1), (1, 1, 1, 1, 1, 1, 1), (1, 1, 1, 1, 1, 1, 2), (3, 1, 2, 1, 1, 1, 2)]


def test_wgrad_restatement_gives_the_headers_answers(probe):
    assert [probe.probe_wgrad_constant(i) for i in range(3)] == [768, 256, 32]
    shapes = list(WGRAD_EDGES) + list(wf.ENTRIES) + list(tp.CONV_TRAIN_CASES)
    assert len(tp.CONV_TRAIN_CASES) == 11 and len(wf.ENTRIES) == 7 + 8 + 4 + 2
    shapes += [(B, Cin, Cout, D, H, W, stride) for B, Cin, Cout, D, H, W, stride in itertools.product(
        (1, 2, 3, 513), (1, 32, 33, 96), (1, 2, 32, 33, 64), (1, 2, 3, 12), (1, 7, 8, 15, 16, 17, 64), (1, 31, 32, 33, 96, 97, 129, 193, 257), (1, 2))]
    for shape, coop in itertools.product(shapes, (True, False)):
        assert wgrad_plan(probe, *shape, coop) == wf._wgrad_form(*shape, coop), (shape, coop)


def test_wgrad_both_sides_of_every_threshold(probe):
    live = lambda *a, **k: {n: v for n, v in wgrad_plan(probe, *a, **k).items() if v and n not in ("ci_tiles", "tiles")}      # noqa: E731
    # which kernel: a single output channel at stride 1 is the head's, unless SS_WGRAD_COOP=0; the stride and the switch decide the rest
    assert live(1, 32, 1, 2, 3, 32, 1) == dict(kernel="head", chunks_per_row=1, total_chunks=6, per_wave=1, nwaves=6)
    assert live(1, 32, 1, 2, 3, 32, 1, coop=False)["kernel"] == "per_wave_s1" and live(1, 32, 1, 2, 3, 32, 2)["kernel"] == "s2a"
    assert [live(1, 32, 2, 2, 3, 32, s, coop=c)["kernel"] for s, c in ((1, True), (1, False), (2, True), (2, False))] == list(WGRAD_KERNELS[:4])
    # the floor of 4 chunks per range from four chunks per row: Wo 96 | 97 (per-wave form), W 192 | 193 at stride 2 (both forms)
    assert live(1, 32, 32, 1, 4, 96, 1, coop=False) == dict(kernel="per_wave_s1", chunks_per_row=3, total_chunks=12, per_unit=1, nsplit=12)
    assert live(1, 32, 32, 1, 4, 97, 1, coop=False) == dict(kernel="per_wave_s1", chunks_per_row=4, total_chunks=16, per_unit=4, nsplit=4)
    assert live(1, 32, 32, 2, 4, 192, 2) == dict(kernel="s2a", chunks_per_row=3, total_chunks=6, ns=6, pu=1)
    assert live(1, 32, 32, 2, 4, 193, 2) == dict(kernel="s2a", chunks_per_row=4, total_chunks=8, ns=2, pu=4)
    assert live(1, 32, 32, 2, 4, 193, 2, coop=False) == dict(kernel="per_wave_s2", chunks_per_row=4, total_chunks=8, per_unit=4, nsplit=2)
    # per-wave: 3072 / 9 = 341 ranges of one tile pair: 341 | 342 chunks; two tiles: 170 ranges, 170 | 171 chunks; 170 | 171 pairs: two ranges | one
    assert live(1, 32, 32, 11, 31, 32, 1, coop=False) == dict(kernel="per_wave_s1", chunks_per_row=1, total_chunks=341, per_unit=1, nsplit=341)
    assert live(1, 32, 32, 9, 38, 32, 1, coop=False) == dict(kernel="per_wave_s1", chunks_per_row=1, total_chunks=342, per_unit=2, nsplit=171)
    assert live(1, 32, 33, 10, 17, 32, 1, coop=False)["per_unit"] == 1 and live(1, 32, 33, 9, 19, 32, 1, coop=False)["per_unit"] == 2
    assert live(341, 32, 32, 2, 2, 32, 1, coop=False)["nsplit"] == 1 and live(342, 32, 32, 2, 2, 32, 1, coop=False)["nsplit"] == 1
    assert live(170, 32, 32, 2, 2, 32, 1, coop=False)["nsplit"] == 2 and live(171, 32, 32, 2, 2, 32, 1, coop=False)["nsplit"] == 1
    # cooperative: min(768 / (columns tiles B), Ho / 8) segments, of equal length rounded up
    assert live(1, 32, 32, 12, 16, 32 * 32, 1) == dict(kernel="coop", chunks_per_row=32, total_chunks=12 * 16 * 32, nseg=2, seg_len=8)       # 384 columns
    assert live(1, 32, 32, 11, 16, 32 * 35, 1) == dict(kernel="coop", chunks_per_row=35, total_chunks=11 * 16 * 35, nseg=1, seg_len=16)      # 385
    assert live(1, 32, 32, 24, 64, 32 * 32, 1)["nseg"] == 1 and live(1, 32, 32, 769, 64, 32, 1)["nseg"] == 1                              # 768 | 769
    assert [(lambda f: (f["nseg"], f["seg_len"]))(live(1, 32, 32, 2, H, 64, 1)) for H in (15, 16, 17, 24)] == [(1, 15), (2, 8), (2, 9), (3, 8)]
    assert live(2, 32, 33, 2, 64, 64, 1)["nseg"] == 8 and live(2, 32, 33, 2, 64, 64, 1)["seg_len"] == 8                                    # 16 columns-tiles-pairs: 48, Ho / 8 decides
    # shared gout: 256 / (tiles B) ranges
    assert live(1, 32, 32, 31, 16, 64, 2) == dict(kernel="s2a", chunks_per_row=1, total_chunks=128, ns=128, pu=1)
    assert live(1, 32, 32, 2, 257 * 2, 64, 2) == dict(kernel="s2a", chunks_per_row=1, total_chunks=257, ns=129, pu=2)
    assert live(1, 32, 32, 2, 256 * 2, 64, 2)["pu"] == 1 and live(1, 32, 64, 2, 128 * 2, 64, 2)["pu"] == 1 and live(1, 32, 64, 2, 129 * 2, 64, 2)["pu"] == 2
    assert live(128, 32, 32, 2, 8, 64, 2)["ns"] == 2 and live(129, 32, 32, 2, 8, 64, 2)["ns"] == 1           # four chunks: 256 / B = 2 | 1 ranges
    # head: max(4, 2048 / (ci_tiles B)) waves
    assert live(1, 32, 1, 32, 64, 32, 1) == dict(kernel="head", chunks_per_row=1, total_chunks=2048, per_wave=1, nwaves=2048)
    assert live(1, 32, 1, 1, 2049, 32, 1) == dict(kernel="head", chunks_per_row=1, total_chunks=2049, per_wave=2, nwaves=1025)
    assert live(1, 64, 1, 16, 64, 32, 1)["per_wave"] == 1 and live(1, 64, 1, 1, 1025, 32, 1)["per_wave"] == 2
    assert live(512, 32, 1, 1, 5, 32, 1)["per_wave"] == 2 and live(513, 32, 1, 1, 5, 32, 1)["per_wave"] == 2 and live(513, 32, 1, 1, 4, 32, 1)["per_wave"] == 1
    assert live(1024, 32, 1, 1, 8, 32, 1)["nwaves"] == 4 and live(1024, 32, 1, 1, 9, 32, 1)["nwaves"] == 3


def test_wgrad_forms_of_the_training_cases(probe):
    """which kernel each of the eleven CONV_TRAIN_CASES of tests/test_parity_gpu.py runs, and by what partition: stated here, so that a
    retune that moves them shows"""
    got = [wgrad_plan(probe, *c) for c in tp.CONV_TRAIN_CASES]
    assert [g["kernel"] for g in got] == ["coop", "s2a", "coop", "coop", "s2a", "coop", "s2a", "head", "coop", "coop", "s2a"]
    assert [(g["nseg"], g["seg_len"]) for g in got if g["kernel"] == "coop"] == [(1, 10), (1, 7), (1, 6), (2, 11), (8, 8), (4, 8)]
    assert [(g["ns"], g["pu"]) for g in got if g["kernel"] == "s2a"] == [(12, 1), (6, 1), (50, 2), (64, 4)]
    assert (got[7]["per_wave"], got[7]["nwaves"]) == (1, 81)
    for c in tp.CONV_TRAIN_CASES:
        assert wgrad_plan(probe, *c, coop=False) == wf._wgrad_form(*c, False)
