"""Every launch form of the transposed 3-D convs (semstereo_amd/csrc/deconv3d_bf16s.hip) at small ragged shapes, against float64.

The launcher decides by ss::plan_deconv3d (csrc/conv_plan.h; restated as _deconv_form of tests/test_f16_ranges_gpu.py, held to the
header by tests/test_conv_plan.py): the 2 x 2 or the 1 x 4 tile, and for the fp16 form all 8 output parity classes in one workgroup
(groups 0: what the large layers of a real pair run, with nontemporal stores from 192 MB of output), two class groups (groups 1) or
two groups + chunk-blocked accumulation (groups 2: what every small shape gets by itself).  SS_DECONV_GROUPS / SS_DECONV_STREAM force
each form onto nine shapes that are ragged in every extent; two shapes either side of the 256-unit threshold run with no switch set.

  * Reference: F.conv_transpose3d in float64 + the float64 1x1x1 skip projection + shift, ReLU -- as test_deconv3d_split_bf16_engine
    (tests/test_parity_gpu.py) builds it, whose bound is the one used: e <= 1.5 e_f32 + 1e-6 (nterms 19 and 6), 4e-5 (nterms 3), e the
    largest absolute error and e_f32 that of the exact-fp32 kernel (deconv3d_hip) on the same input OVER THE SAME REGION: the whole
    tensor, each of the 8 output parity classes (the class groups are {0, 1, 6, 7} and {2, 3, 4, 5}: a mistake in one group's step
    table shows in its classes alone), the columns / rows / planes / channels of a partial tile, the border positions 2N - 1.
    (Cout = 33 is no shape of the exact-fp32 kernel, which needs Cout % 4 == 0: it gets that layer with three zero channels appended.)
  * Bit relations, each read from the kernel's order of summation (the docstrings of the tests say how).
Which instantiation a case reaches is asserted from the restated rule, never by looking at a kernel.  Every figure is printed; set
SS_DECONV_FORMS_ERR_OUT=<file> to keep the table (profiles/deconv_forms_err.txt is a copy of one run).
Run on the MI355X box: pytest -m gpu."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import test_f16_ranges_gpu as fr
from oracle import detdata as dd

pytestmark = pytest.mark.gpu

# (Cin, Cout, D, H, W, Cs), B = 2: the five of test_deconv3d_split_bf16_engine, then
#   ragged in W, H, Cout and Cin at once / one column, two of the tile's four rows, a channel tile of a single channel /
#   the 2 x 2 tile with an odd depth and a 1-column last tile / D = 1 with H < 4: the 1 x 4 tile at H = 3
SHAPES = [(128, 64, 2, 3, 5, 64), (64, 32, 3, 9, 33, 32), (32, 32, 2, 4, 40, 0), (8, 24, 2, 3, 6, 6), (20, 40, 1, 5, 34, 10),
          (48, 40, 3, 9, 35, 16), (16, 33, 1, 2, 1, 0), (16, 32, 5, 3, 33, 8), (64, 64, 1, 3, 70, 32)]
BOTH_SKIP_ORDERS = [SHAPES[0], SHAPES[1], SHAPES[5], SHAPES[8]]
LONG_K = SHAPES[0]
# name -> (SS_DECONV_GROUPS, SS_DECONV_STREAM); "natural": no switch set
FORMS = {"groups0": ("0", "0"), "groups0_stream": ("0", "1"), "groups1": ("1", "-1"), "groups2": ("2", "-1")}
# natural dispatch either side of per_pair = 256, B = 1: 2 x 8 x 16 tiles of 1 x 4 x 32 x one channel tile | 2 x 8 x 15 = 240
THRESHOLD = [(64, 32, 16, 32, 64, 0), (64, 32, 15, 32, 64, 0)]

_ids = lambda cases: ["x".join(map(str, c)) for c in cases]      # noqa: E731
_TABLE = []


@pytest.fixture(scope="module", autouse=True)
def _dump_table():
    yield
    path = os.environ.get("SS_DECONV_FORMS_ERR_OUT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(_TABLE) + "\n")
    _case.cache_clear()


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    return semstereo_amd


def _force(tuning_env, form):
    if form != "natural":
        groups, stream = FORMS[form]
        tuning_env("SS_DECONV_GROUPS", groups)
        tuning_env("SS_DECONV_STREAM", stream)


class _Case:
    """the seeded inputs of test_deconv3d_split_bf16_engine at one shape, their float64 result, the exact-fp32 kernel's, and the packed
    weights: built once per shape and shared, never written to"""

    def __init__(self, sa, shape, B):
        M = sa.modules
        Cin, Cout, D, H, W, Cs = shape
        self.shape, self.B, self.M = shape, B, M
        x = dd.t_normalish((B, Cin, D, H, W), 391)
        w = dd.t_uniform((Cin, Cout, 3, 3, 3), 392, -1, 1) * (3.0 / (Cin * 27 / 8)) ** 0.5
        shift = dd.t_uniform((Cout,), 393, -0.2, 0.2)
        main = F.conv_transpose3d(x.double(), w.double(), None, stride=2, padding=1, output_padding=1) + shift.double().reshape(1, -1, 1, 1, 1)
        self.ref_noskip = F.relu(main)
        self.lin = main - shift.double().reshape(1, -1, 1, 1, 1)           # before shift and ReLU (+ the skip projection below)
        self.x, self.shift = x.cuda(), shift.cuda()
        self.wp = M.pack_conv_weight(w.cuda(), transposed=True)
        self.skip = self.wsp = None
        self.ref = self.ref_noskip
        if Cs:
            skip = dd.t_normalish((B, Cs, 2 * D, 2 * H, 2 * W), 394)
            ws = dd.t_uniform((Cout, Cs, 1, 1, 1), 395, -1, 1) * (3.0 / Cs) ** 0.5
            self.ref = F.relu(main + F.conv3d(skip.double(), ws.double()))
            self.lin = self.lin + F.conv3d(skip.double(), ws.double())
            self.skip = skip.cuda()
            self.wsp = M.pack_conv_weight(ws.cuda()).reshape(Cs, Cout).contiguous()
        self.packed = {n: M.pack_deconv_weight_bf16s(self.wp, n) for n in (19, 6, 3)}
        self.skip_packed = None if self.wsp is None else M.pack_deconv_weight_bf16s(self.wsp)
        # the yardstick: the exact-fp32 kernel moves its weights as float4 and takes no Cout that is not a multiple of 4; such a
        # layer is given to it with zero output channels appended (an output channel's sum does not involve the others)
        pad = -Cout % 4
        wp32 = self.wp if not pad else M.pack_conv_weight(F.pad(w, (0, 0, 0, 0, 0, 0, 0, pad)).cuda(), transposed=True)
        wsp32 = self.wsp if not (pad and Cs) else M.pack_conv_weight(F.pad(ws, (0, 0, 0, 0, 0, 0, 0, 0, 0, pad)).cuda()).reshape(Cs, Cout + pad).contiguous()
        shift32 = F.pad(self.shift, (0, pad))
        self.y32 = M.deconv3d_hip(self.x, wp32, shift32, True, self.skip, wsp32)[:, :Cout].double().cpu()
        self.y32_noskip = self.y32 if not Cs else M.deconv3d_hip(self.x, wp32, shift32, True, None, None)[:, :Cout].double().cpu()
        self.y32_lin = M.deconv3d_hip(self.x, wp32, torch.zeros_like(shift32), False, self.skip, wsp32)[:, :Cout]      # fp32, on the device

    def run(self, nterms=19, skip=True, x=None, skip_t=None):
        """the kernel under test, under whatever switches are set; x / skip_t: other batch elements of the same layer"""
        use = skip and self.skip is not None
        x = self.x if x is None else x
        skip_t = (self.skip if skip_t is None else skip_t) if use else None
        return self.M.deconv3d_bf16s_hip(x, self.packed[nterms], self.shape[1], self.shift, True, nterms, skip_t, self.skip_packed if use else None)


@functools.lru_cache(maxsize=None)
def _case(sa, shape, B=2):
    return _Case(sa, shape, B)


def _regions(shape):
    """name -> boolean mask over [Cout, 2D, 2H, 2W] (every batch element)"""
    _cin, Cout, D, H, W, _cs = shape
    (td, th), _, _ = fr._deconv_form(D, H, W, Cout)
    c = torch.arange(Cout).reshape(-1, 1, 1, 1)
    od, oh, ow = torch.arange(2 * D).reshape(1, -1, 1, 1), torch.arange(2 * H).reshape(1, 1, -1, 1), torch.arange(2 * W).reshape(1, 1, 1, -1)
    full = torch.ones(Cout, 2 * D, 2 * H, 2 * W, dtype=torch.bool)
    r = {"whole": full}
    for cls in range(8):                            # the kernel's class index: (od & 1) * 4 + (oh & 1) * 2 + (ow & 1)
        r[f"class{cls}"] = full & ((od & 1) * 4 + (oh & 1) * 2 + (ow & 1) == cls)
    if W % 32:
        r["last_partial_column_tile"] = full & (ow >= 2 * (W // 32 * 32))
    if H % th:
        r["rows_of_partial_tile"] = full & (oh >= 2 * (H // th * th))
    if D % td:
        r["planes_of_partial_tile"] = full & (od >= 2 * (D // td * td))
    if Cout % 32:
        r["partial_channel_tile"] = full & (c >= Cout // 32 * 32)
    r["border_plane"], r["border_row"], r["border_column"] = full & (od == 2 * D - 1), full & (oh == 2 * H - 1), full & (ow == 2 * W - 1)
    return r


def _judge(what, shape, y, y32, ref, nterms=19):
    """the bound over every region; every figure goes into the table BEFORE the first assertion"""
    assert y.shape == ref.shape and bool(torch.isfinite(y).all()), what
    err, err32 = (y.double().cpu() - ref).abs(), (y32 - ref).abs()
    missed = []
    for name, mask in _regions(shape).items():
        assert bool(mask.any()), (what, name)
        e, e32 = float(err[:, mask].max()), float(err32[:, mask].max())
        bound = 4e-5 if nterms == 3 else 1.5 * e32 + 1e-6
        line = f"{what:58s} {name:26s} e {e:.3e}  e_f32 {e32:.3e}  {e / bound:6.3f} of {'4e-5' if nterms == 3 else '1.5 e_f32 + 1e-6'}"
        print(line)
        _TABLE.append(line)
        if not e <= bound:
            missed.append((name, e, e32))
    assert not missed, (what, missed)


def test_shapes_reach_the_forms_and_both_skip_orders():
    tiles = [fr._deconv_form(*s[2:5], s[1])[0] for s in SHAPES]
    assert tiles == [(2, 2), (1, 4), (1, 4), (2, 2), (1, 4), (1, 4), (1, 4), (2, 2), (1, 4)]
    for s in SHAPES:                        # by themselves all of them get groups 2; every switch value moves them
        assert fr._deconv_form(*s[2:5], s[1], 2) == (tiles[SHAPES.index(s)], 2, False)
        for form, (groups, stream) in FORMS.items():
            assert fr._deconv_form(*s[2:5], s[1], 2, 19, int(groups), int(stream))[1:] == (int(groups), form == "groups0_stream")
    # skip first where (unit ^ channel tile) is odd, after the main loop elsewhere (the non-split forms): both populations need two
    # units or two channel tiles
    for s in BOTH_SKIP_ORDERS:
        assert s[5] > 0 and fr._deconv_skip_orders(*s[2:5], s[1]) == {0, 1}, s
    assert [fr._deconv_form(*s[2:5], s[1], 1)[1] for s in THRESHOLD] == [0, 2]
    # what the region masks name exists: a partial column tile, partial row and plane tiles, a partial channel tile
    names = set().union(*(set(_regions(s)) for s in SHAPES))
    assert {"last_partial_column_tile", "rows_of_partial_tile", "planes_of_partial_tile", "partial_channel_tile"} <= names


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_fp16_form_against_float64(sa, shape, form, tuning_env):
    c = _case(sa, shape)
    _force(tuning_env, form)
    _judge(f"{shape} {form}", shape, c.run(19), c.y32, c.ref)
    if shape[5]:                            # ... and the layer without its skip tensor (what training runs)
        _judge(f"{shape} {form} no skip", shape, c.run(19, skip=False), c.y32_noskip, c.ref_noskip)


@pytest.mark.parametrize("nterms", [6, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_bf16_forms_against_float64(sa, shape, nterms):
    """one form each (the switches do not reach them): the baseline of the table.  (This test found the one miss of the file: bf16x6 on
    the long-K shape, parity class 1, 1.142 of the bound while six MFMAs per K-step rounded straight into the accumulator; the kernel
    now sums a step from zero and joins it once -- profiles/EXPERIMENTS.md part X.)"""
    c = _case(sa, shape)
    _judge(f"{shape} bf16x{nterms}", shape, c.run(nterms), c.y32, c.ref, nterms)


def _skip_first_mask(shape):
    """[Cout, 2D, 2H, 2W]: outputs of the workgroups that project the skip tensor BEFORE the main loop in the non-split forms:
    (unit ^ channel tile) & 1, unit = (tile_d * tiles_h + tile_h) * tiles_w + tile_w"""
    _cin, Cout, D, H, W, _cs = shape
    (td, th), _, _ = fr._deconv_form(D, H, W, Cout)
    tiles_w, tiles_h = fr._cdiv(W, 32), fr._cdiv(H, th)
    c = torch.arange(Cout).reshape(-1, 1, 1, 1) // 32
    d = torch.arange(2 * D).reshape(1, -1, 1, 1) // (2 * td)
    h = torch.arange(2 * H).reshape(1, 1, -1, 1) // (2 * th)
    w = torch.arange(2 * W).reshape(1, 1, 1, -1) // 64
    return ((((d * tiles_h + h) * tiles_w + w) ^ c) & 1).bool()


@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_bit_relations_between_the_forms(sa, shape, tuning_env):
    """Read from the kernel (deconv3d_bf16s.hip):
      * STREAM changes the aux bits of the store instruction and nothing else: stream 1 == stream 0, with and without skip tensor.
      * Without a skip tensor groups 1 == groups 0: a class group's step list is the full list filtered (make_grp_table), so the
        K-steps feeding one class keep their order, each is the same three MFMAs, and the block exponent comes from the same staged
        input tile; the epilogue is the same arithmetic per class.
      * With a skip tensor, groups 0 projects it BEFORE the main loop in the workgroups with (unit ^ channel tile) odd and after it in
        the others; groups 1 always after.  So the two agree bit for bit on the outputs of the skip-after workgroups only; on the
        skip-first ones the sum is taken in another order (there: float64 alone, test_fp16_form_against_float64).  That they DO
        differ somewhere there is asserted on the shapes with both populations: it shows the skip-first path ran.
      * groups 2 (chunk-blocked: a chunk's 27 steps summed from zero, then joined) is another order than groups 1 wherever there is
        more than one 16-channel chunk; asserted to differ on the long-K shape (Cin = 128), with and without the skip tensor."""
    c = _case(sa, shape)
    out = {}
    for form in sorted(FORMS):
        _force(tuning_env, form)
        out[form] = c.run(19)
        out[form, "noskip"] = c.run(19, skip=False) if shape[5] else out[form]
    assert torch.equal(out["groups0_stream"], out["groups0"]) and torch.equal(out["groups0_stream", "noskip"], out["groups0", "noskip"])
    assert torch.equal(out["groups1", "noskip"], out["groups0", "noskip"])
    if shape[5]:
        first = _skip_first_mask(shape)
        g0, g1 = out["groups0"].cpu(), out["groups1"].cpu()
        assert torch.equal(g0[:, ~first], g1[:, ~first])
        if shape in BOTH_SKIP_ORDERS:
            assert bool(first.any()) and bool((~first).any()) and not torch.equal(g0[:, first], g1[:, first])
    if shape == LONG_K:
        assert not torch.equal(out["groups2"], out["groups0"]) and not torch.equal(out["groups2", "noskip"], out["groups1", "noskip"])


# the folded form (SHIFT27: the shift is a table over the 27 border cases of an output position) exists with the skip projection only
SHIFT27_SHAPES = [SHAPES[1], SHAPES[5], SHAPES[7]]


def _border_case_rows(D, H, W):
    """[2D, 2H, 2W] rows of the table: (cd * 3 + ch) * 3 + cw, per axis 0 = even index, 1 = odd interior, 2 = the last odd index 2N - 1"""
    def axis(N):
        n = torch.arange(2 * N)
        return torch.where(n % 2 == 0, 0, torch.where(n == 2 * N - 1, 2, 1))
    return (axis(D).reshape(-1, 1, 1) * 3 + axis(H).reshape(1, -1, 1)) * 3 + axis(W).reshape(1, 1, -1)


@pytest.mark.parametrize("shape", SHIFT27_SHAPES, ids=_ids(SHIFT27_SHAPES))
def test_shift_table_form_against_float64(sa, shape, tuning_env):
    """ss_deconv3d_bf16s_shift27_fwd under every form, with a seeded table [27, Cout]: float64 reference relu(conv + skip + table
    [case of the position]); the yardstick is the exact-fp32 kernel without shift and ReLU, the table added and the ReLU taken in
    fp32 on the device (one more rounding than the kernel under test makes).  Stream 1 == stream 0 here too."""
    _cin, Cout, D, H, W, _cs = shape
    c = _case(sa, shape)
    t27 = dd.t_uniform((27, Cout), 396, -0.2, 0.2)
    rows = _border_case_rows(D, H, W)
    assert sorted(set(rows.flatten().tolist())) == list(range(27))
    ref = F.relu(c.lin + t27.double()[rows].permute(3, 0, 1, 2).unsqueeze(0))
    y32 = F.relu(c.y32_lin + t27.cuda()[rows.cuda()].permute(3, 0, 1, 2).unsqueeze(0)).double().cpu()
    out = {}
    for form, nterms in [(f, 19) for f in sorted(FORMS)] + [("natural", 6)]:
        _force(tuning_env, form)
        out[form] = sa.engine.deconv3d_bf16s_shift27_hip(c.x, c.packed[nterms], Cout, t27.cuda(), True, nterms, c.skip, c.skip_packed)
        _judge(f"{shape} table {form if nterms == 19 else 'bf16x6'}", shape, out[form], y32, ref, nterms)
        tuning_env("SS_DECONV_GROUPS", "-1")
        tuning_env("SS_DECONV_STREAM", "-1")
    assert torch.equal(out["groups0_stream"], out["groups0"])


@pytest.mark.parametrize("form", ["natural"] + sorted(FORMS))
def test_a_pair_gets_the_same_bits_at_every_batch_size(sa, form, tuning_env):
    """the launcher's claim (the form is the LAYER's: tiles x channel tiles of ONE pair): batch element 1 alone (B = 1) and as the
    first of two gives the bits it has as the second of two -- under each forced form and the natural dispatch, every shape"""
    _force(tuning_env, form)
    for shape in SHAPES:
        c = _case(sa, shape)
        both = c.run(19)
        x1 = c.x[1:2].contiguous()
        s1 = None if c.skip is None else c.skip[1:2].contiguous()
        alone = c.run(19, x=x1, skip_t=s1)
        swapped = c.run(19, x=c.x.flip(0).contiguous(), skip_t=None if c.skip is None else c.skip.flip(0).contiguous())
        assert torch.equal(alone[0], both[1]) and torch.equal(swapped[0], both[1]) and torch.equal(swapped[1], both[0]), (shape, form)


def test_natural_dispatch_across_the_threshold(sa, tuning_env):
    """no switch set: 256 units of one pair -> all 8 classes per workgroup (groups 0), 240 -> two groups + chunk-blocked accumulation
    (groups 2); the result is the bits of the predicted form forced and not those of the other (Cin = 64: four chunks, so the
    chunk-blocked sum is another order), and meets the float64 bound"""
    for shape, want, other in ((THRESHOLD[0], "groups0", "groups2"), (THRESHOLD[1], "groups2", "groups0")):
        _cin, Cout, D, H, W, _cs = shape
        assert fr._deconv_form(D, H, W, Cout, 1) == ((1, 4), int(FORMS[want][0]), False)
        c = _case(sa, shape, 1)
        natural = c.run(19)
        _judge(f"{shape} B=1 natural ({want})", shape, natural, c.y32, c.ref)
        _force(tuning_env, want)
        assert torch.equal(c.run(19), natural), (shape, want)
        _force(tuning_env, other)
        forced_other = c.run(19)
        assert not torch.equal(forced_other, natural), (shape, other)
        _judge(f"{shape} B=1 forced {other}", shape, forced_other, c.y32, c.ref)
        tuning_env("SS_DECONV_GROUPS", "-1")
        tuning_env("SS_DECONV_STREAM", "-1")
