"""Every kernel and K-range partition of the 3x3x3 weight gradients (semstereo_amd/csrc/conv3d_wgrad_bf16s.hip) at small shapes, against
float64 autograd on the CPU.

ss_conv3d_wgrad_bf16s_fwd launches by ss::plan_wgrad3d (csrc/conv_plan.h; restated here as _wgrad_form, held to the header by
tests/test_conv_plan.py): the cooperative form (stride 1), the shared-gout form (stride 2, and every transposed conv's weights with the
roles swapped), the per-wave form of either stride under SS_WGRAD_COOP=0, the single-output-channel kernel; then wgrad_reorder_kernel.
The exact-fp32 kernel of conv3d_wgrad.hip (ss_conv3d_wgrad_fwd) is the yardstick and is itself held to bounds (1) and (2).
The C entries are called directly: the test owns grad_w and the workspace.

  * Reference: float64 autograd of F.conv3d(x, w, None, stride, 1) seeded with the same grad_out (the roles-swapped cases:
    F.conv_transpose3d(..., stride=2, padding=1, output_padding=1)).
  * Regions of dW [Cout, Cin, 27]: the whole tensor, each of the 27 taps, each (output-channel tile, input-channel tile) pair, the rows
    and columns of partial channel tiles.  Per region, e the largest absolute error and s the region's largest |reference|:
      (1) a tap whose float64 gradient is identically zero (no input position contributes: kd != 1 at D = 1, ...) is exactly 0.0;
      (2) e <= 5e-6 s: the figure of tests/test_parity_gpu.py on the region's OWN scale (three bf16 terms carry 24 bits, the three
          dropped cross products are below 2^-23 of a product);
      (3) e <= 1.5 e_f32 + 1e-6 s, e_f32 the exact-fp32 kernel's error over the same region: what the kernel file says of its
          error, with the factor and floor of tests/test_deconv_forms_gpu.py.  (Measured: e / e_f32 between 0.2 and 2.5 over the
          regions, (3) at most 0.40 of its bound -- the file's header said "below the exact-fp32 MFMA's" until this test; it now
          states these figures, profiles/EXPERIMENTS.md part AA.)
Which kernel and which partition branch a case reaches is asserted from _wgrad_form, never by looking at a kernel.  Every figure is
printed and appended to a table before the first assertion; set SS_WGRAD_FORMS_ERR_OUT=<file> to keep the table
(profiles/wgrad_forms_err.txt is a copy of one run).
Run on the MI355X box: pytest -m gpu."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import detdata as dd

pytestmark = pytest.mark.gpu


def _cdiv(a, b):
    return -(-a // b)


def _wgrad_form(B, Cin, Cout, D, H, W, stride, coop=True):
    """ss::plan_wgrad3d (csrc/conv_plan.h) over an INPUT of (D, H, W): the kernel and the numbers it is launched by (those of the other
    kernels are 0).  coop: SS_WGRAD_COOP != 0."""
    Do, Ho, Wo = ((n - 1) // stride + 1 for n in (D, H, W))
    ci_tiles = _cdiv(Cin, 32)
    tiles = ci_tiles * _cdiv(Cout, 32)
    cpr = _cdiv(Wo, 32)
    total = Do * Ho * cpr
    f = dict(kernel=None, ci_tiles=ci_tiles, tiles=tiles, chunks_per_row=cpr, total_chunks=total, per_unit=0, nsplit=0, nseg=0, seg_len=0,
             ns=0, pu=0, per_wave=0, nwaves=0)
    if Cout == 1 and stride == 1 and coop:
        f["kernel"] = "head"
        f["per_wave"] = max(1, _cdiv(total, max(4, 2048 // (ci_tiles * B))))
        f["nwaves"] = _cdiv(total, f["per_wave"])
        return f
    floor = 4 if cpr >= 4 else 1
    if stride == 1 and coop:
        f["kernel"] = "coop"
        nseg = min(max(1, 768 // max(1, Do * cpr * tiles * B)), max(1, Ho // 8))
        f["seg_len"] = _cdiv(Ho, nseg)
        f["nseg"] = _cdiv(Ho, f["seg_len"])
    elif stride == 2 and coop:
        f["kernel"] = "s2a"
        f["pu"] = max(floor, _cdiv(total, max(1, 256 // (tiles * B))))
        f["ns"] = _cdiv(total, f["pu"])
    else:
        f["kernel"] = "per_wave_s1" if stride == 1 else "per_wave_s2"
        f["per_unit"] = max(floor, _cdiv(total, max(1, 3072 // (9 * tiles * B))))
        f["nsplit"] = _cdiv(total, f["per_unit"])
    return f


# (B, Cin, Cout, D, H, W), input extents; what each reaches is asserted in test_shapes_reach_the_kernels_and_partition_branches.
# (The last stride-2 shape, W = 63, is the only one at which the second half of the stride-2 kernels' `whole` predicate decides.)
S1_SHAPES = [(1, 32, 32, 1, 1, 1), (1, 16, 33, 2, 3, 31), (2, 40, 48, 3, 17, 33), (1, 64, 32, 5, 9, 64), (1, 32, 64, 2, 20, 100),
             (1, 8, 24, 1, 8, 97), (2, 96, 32, 4, 5, 40)]
S2_SHAPES = [(1, 32, 32, 1, 1, 1), (1, 16, 33, 3, 5, 31), (2, 64, 64, 5, 7, 139), (1, 40, 48, 2, 5, 259), (1, 32, 64, 4, 6, 16),
             (1, 32, 32, 6, 3, 66), (2, 8, 40, 3, 9, 72), (1, 16, 32, 3, 4, 63)]
HEAD_SHAPES = [(1, 8, 1, 3, 9, 70), (2, 64, 1, 4, 33, 130), (1, 33, 1, 1, 1, 5), (1, 32, 1, 2, 3, 32)]
# (B, Cin, Cout, D, H, W) of a ConvTranspose3d(k3, s2, p1, op1): _Deconv3dK3.backward hands its INPUT over as grad_out and the
# gradient of its output (twice the extents) as the input of a stride-2 layer Cout -> Cin
SWAPPED_SHAPES = [(1, 48, 40, 2, 5, 33), (2, 16, 33, 1, 3, 17)]


def _entry(kind, shape):
    """-> (B, Cin, Cout, D, H, W, stride) as ss_conv3d_wgrad_bf16s_fwd is called"""
    B, Cin, Cout, D, H, W = shape
    if kind == "swapped":
        return (B, Cout, Cin, 2 * D, 2 * H, 2 * W, 2)
    return (B, Cin, Cout, D, H, W, 2 if kind == "s2" else 1)


CASES = [("s1", s) for s in S1_SHAPES] + [("s2", s) for s in S2_SHAPES] + [("head", s) for s in HEAD_SHAPES] + [("swapped", s) for s in SWAPPED_SHAPES]
ENTRIES = [_entry(*c) for c in CASES]              # what tests/test_conv_plan.py runs through the header
_ids = lambda cases: [k + "-" + "x".join(map(str, s)) for k, s in cases]      # noqa: E731
_TABLE = ["per call (== kind, shape, kernel, what is special) and region: s the largest |float64 reference| of the region, e the largest "
          "absolute error, (2) e / (5e-6 s), e_f32 the exact-fp32 kernel's error, (3) e / (1.5 e_f32 + 1e-6 s); both ratios must be <= 1"]
BOUND2, FACTOR3, FLOOR3 = 5e-6, 1.5, 1e-6


@pytest.fixture(scope="module", autouse=True)
def _dump_table():
    yield
    path = os.environ.get("SS_WGRAD_FORMS_ERR_OUT")
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


def _ws_floats(Cin, Cout):
    return _cdiv(Cout, 32) * _cdiv(Cin, 32) * 27 * 1024


def _run_bf16s(gout, x, Cout, stride, gw=None, ws=None):
    """ss_conv3d_wgrad_bf16s_fwd under whatever SS_WGRAD_COOP says -> dW [Cout, Cin, 27] (the caller's gw and ws, if given)"""
    from semstereo_amd._lib import call, ptr
    B, Cin, D, H, W = x.shape
    gw = torch.empty(Cout * Cin * 27, dtype=torch.float32, device=x.device) if gw is None else gw
    ws = torch.empty(_ws_floats(Cin, Cout), dtype=torch.float32, device=x.device) if ws is None else ws
    assert gout.is_contiguous() and x.is_contiguous() and gw.is_contiguous() and ws.is_contiguous()
    assert gw.numel() == Cout * Cin * 27 and ws.numel() == _ws_floats(Cin, Cout)
    call("ss_conv3d_wgrad_bf16s_fwd", ptr(gout), ptr(x), ptr(gw), ptr(ws), B, Cin, D, H, W, Cout, stride)
    return gw.reshape(Cout, Cin, 27)


def _run_f32(gout, x, Cout, stride, gw=None):
    """ss_conv3d_wgrad_fwd, the exact-fp32 kernel"""
    from semstereo_amd._lib import call, ptr
    B, Cin, D, H, W = x.shape
    gw = torch.empty(Cout * Cin * 27, dtype=torch.float32, device=x.device) if gw is None else gw
    assert gout.is_contiguous() and x.is_contiguous() and gw.is_contiguous() and gw.numel() == Cout * Cin * 27
    call("ss_conv3d_wgrad_fwd", ptr(gout), ptr(x), ptr(gw), B, Cin, D, H, W, Cout, stride)
    return gw.reshape(Cout, Cin, 27)


def _reference(kind, gout, x, stride):
    """float64 autograd on the CPU -> dW [Cout, Cin, 27] in the entry's roles"""
    Cout, Cin = gout.shape[1], x.shape[1]
    if kind == "swapped":                       # gout: the transposed conv's input [B, Cout, D, H, W]; x: the gradient of its output
        w = torch.zeros(Cout, Cin, 3, 3, 3, dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose3d(gout.double(), w, None, stride=2, padding=1, output_padding=1)
        assert y.shape == x.shape
        (g,) = torch.autograd.grad(y, w, x.double())
    else:
        w = torch.zeros(Cout, Cin, 3, 3, 3, dtype=torch.float64, requires_grad=True)
        y = F.conv3d(x.double(), w, None, stride, 1)
        assert y.shape == gout.shape
        (g,) = torch.autograd.grad(y, w, gout.double())
    return g.reshape(Cout, Cin, 27)


class _Case:
    """seeded inputs of one shape, their float64 weight gradient and the exact-fp32 kernel's: built once per shape and shared, never written to"""

    def __init__(self, sa, kind, shape):
        self.kind, self.shape = kind, shape
        self.entry = B, Cin, Cout, D, H, W, stride = _entry(kind, shape)
        Do, Ho, Wo = ((n - 1) // stride + 1 for n in (D, H, W))
        self.x_cpu = dd.t_normalish((B, Cin, D, H, W), 861)
        self.g_cpu = dd.t_normalish((B, Cout, Do, Ho, Wo), 862)
        self.ref = _reference(kind, self.g_cpu, self.x_cpu, stride)
        self.x, self.g = self.x_cpu.cuda(), self.g_cpu.cuda()
        self.y32 = _run_f32(self.g, self.x, Cout, stride).double().cpu()
        self.K = B * Do * Ho * Wo

    def form(self, coop=True):
        return _wgrad_form(*self.entry, coop)

    def run(self, g=None, x=None):
        g, x = self.g if g is None else g, self.x if x is None else x
        return _run_bf16s(g, x, self.entry[2], self.entry[6])


@functools.lru_cache(maxsize=None)
def _case(sa, kind, shape):
    return _Case(sa, kind, shape)


def _regions(Cout, Cin):
    """name -> boolean mask over [Cout, Cin, 27]"""
    co = torch.arange(Cout).reshape(-1, 1, 1)
    ci = torch.arange(Cin).reshape(1, -1, 1)
    tap = torch.arange(27).reshape(1, 1, -1)
    full = torch.ones(Cout, Cin, 27, dtype=torch.bool)
    r = {"whole": full}
    for t in range(27):
        r[f"tap{t // 9}{t // 3 % 3}{t % 3}"] = full & (tap == t)
    for i in range(_cdiv(Cout, 32)):
        for j in range(_cdiv(Cin, 32)):
            r[f"tile_co{i}_ci{j}"] = full & (co // 32 == i) & (ci // 32 == j)
    if Cout % 32:
        r["co_partial_tile"] = full & (co >= Cout // 32 * 32)
    if Cin % 32:
        r["ci_partial_tile"] = full & (ci >= Cin // 32 * 32)
    return r


def _judge(what, y, ref, y32=None):
    """(1), (2) and -- given the exact-fp32 kernel's result -- (3) over every region; every figure goes into the table BEFORE the first
    assertion"""
    y = y.detach().double().cpu()
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    finite = bool(torch.isfinite(y).all())
    err = (y - ref).abs()
    err32 = None if y32 is None else (y32 - ref).abs()
    missed = []
    _TABLE.append(f"== {what}")
    print(_TABLE[-1])
    for name, mask in _regions(*ref.shape[:2]).items():
        assert bool(mask.any()), (what, name)
        s, e = float(ref[mask].abs().max()), float(err[mask].max())
        if s == 0.0:                             # (1): no position contributes (decided from the reference)
            nonzero = int((y[mask] != 0).sum())
            line = f"{name:14s} identically zero; values of the kernel that are not 0.0: {nonzero}"
            ok = nonzero == 0
        else:
            line = f"{name:14s} s {s:.3e}  e {e:.3e}  (2) {e / (BOUND2 * s):5.3f}"
            ok = e <= BOUND2 * s
            if err32 is not None:
                e32 = float(err32[mask].max())
                bound3 = FACTOR3 * e32 + FLOOR3 * s
                line += f"  e_f32 {e32:.3e}  e/e_f32 {e / e32 if e32 else float('inf'):6.3f}  (3) {e / bound3:5.3f}"
                ok = ok and e <= bound3
        print(line)
        _TABLE.append(line)
        if not ok:
            missed.append((name, e, s))
    assert finite, what
    assert not missed, (what, missed)


def _live(form):
    return {k: v for k, v in form.items() if v}


def test_shapes_reach_the_kernels_and_partition_branches():
    """what the shape tables of this file promise, from the restated rule -- a retune of a threshold moves a case HERE, not silently"""
    f = lambda kind, shape, coop=True: _wgrad_form(*_entry(kind, shape), coop)      # noqa: E731
    for kind, shapes, kern, other in (("s1", S1_SHAPES, "coop", "per_wave_s1"), ("s2", S2_SHAPES, "s2a", "per_wave_s2"),
                                      ("head", HEAD_SHAPES, "head", "per_wave_s1"), ("swapped", SWAPPED_SHAPES, "s2a", "per_wave_s2")):
        for s in shapes:
            assert (f(kind, s)["kernel"], f(kind, s, False)["kernel"]) == (kern, other), (kind, s)
    # ---- stride 1: the cooperative form (nseg, seg_len) | the per-wave form (per_unit, nsplit) ----
    s1 = {s: (f("s1", s), f("s1", s, False)) for s in S1_SHAPES}
    coop = {s: (c["chunks_per_row"], c["total_chunks"], c["nseg"], c["seg_len"]) for s, (c, _) in s1.items()}
    wave = {s: (w["per_unit"], w["nsplit"]) for s, (_, w) in s1.items()}
    assert coop[S1_SHAPES[0]] == (1, 1, 1, 1) and wave[S1_SHAPES[0]] == (1, 1)            # every extent 1; one live split of the 8 of a group
    assert coop[S1_SHAPES[1]] == (1, 6, 1, 3) and wave[S1_SHAPES[1]] == (1, 6)            # one partial chunk; 6 of 8 splits live
    assert S1_SHAPES[1][2] == 33 and S1_SHAPES[1][5] % 4                                  # Cout one past a tile, narrow gout loads
    assert coop[S1_SHAPES[2]] == (2, 102, 2, 9) and S1_SHAPES[2][4] - 9 == 8              # two segments, of 9 and 8 rows
    assert S1_SHAPES[2][5] - 32 == 1                                                      # the last chunk one column wide
    assert wave[S1_SHAPES[2]] == (3, 34) and _cdiv(34, 8) == 5                            # five groups of 8 splits; a range of 3 chunks crosses
    assert 2 % 3 and (2 * 17) % 3                                                         # ... rows (2 chunks each) and planes (34 chunks each)
    assert s1[S1_SHAPES[2]][0]["tiles"] == 4 and S1_SHAPES[2][1] % 32 and S1_SHAPES[2][2] % 32
    assert coop[S1_SHAPES[3]] == (2, 90, 1, 9) and S1_SHAPES[3][5] % 32 == 0 and s1[S1_SHAPES[3]][0]["ci_tiles"] == 2
    assert coop[S1_SHAPES[4]] == (4, 160, 2, 10) and wave[S1_SHAPES[4]] == (4, 40)        # two equal segments; the floor of 4 decides:
    assert _cdiv(160, 3072 // (9 * 2)) == 1                                               # ... by the wave count a range would be one chunk
    assert coop[S1_SHAPES[5]] == (4, 32, 1, 8) and wave[S1_SHAPES[5]] == (4, 8)           # D = 1, the floor of 4 with exactly 8 splits
    assert coop[S1_SHAPES[6]] == (2, 40, 1, 5) and s1[S1_SHAPES[6]][0]["ci_tiles"] == 3   # three input-channel tiles, H < 8
    # ---- stride 2: the shared-gout form (pu, ns) | the per-wave form (per_unit, nsplit) ----
    s2 = {s: (f("s2", s), f("s2", s, False)) for s in S2_SHAPES}
    sh = {s: (c["chunks_per_row"], c["total_chunks"], c["pu"], c["ns"]) for s, (c, _) in s2.items()}
    wave = {s: (w["per_unit"], w["nsplit"]) for s, (_, w) in s2.items()}
    assert sh[S2_SHAPES[0]] == (1, 1, 1, 1) and wave[S2_SHAPES[0]] == (1, 1)
    assert sh[S2_SHAPES[1]] == (1, 6, 1, 6) and all(n % 2 for n in S2_SHAPES[1][3:]) and (S2_SHAPES[1][5] + 1) // 2 == 16      # wide gout loads
    assert sh[S2_SHAPES[2]] == (3, 36, 2, 18) and wave[S2_SHAPES[2]] == (1, 36) and all(n % 2 for n in S2_SHAPES[2][3:])
    assert (S2_SHAPES[2][5] + 1) // 2 == 70 and 70 % 4 and s2[S2_SHAPES[2]][0]["tiles"] == 4                                   # narrow loads, four tile pairs
    assert sh[S2_SHAPES[3]] == (5, 15, 4, 4) and wave[S2_SHAPES[3]] == (4, 4) and 15 - 3 * 4 == 3                              # the floor of 4; the last range holds 3
    assert _cdiv(15, 256 // 4) == 1
    assert sh[S2_SHAPES[4]] == (1, 6, 1, 6) and not any(n % 2 for n in S2_SHAPES[4][3:])
    assert sh[S2_SHAPES[5]] == (2, 12, 1, 12) and (S2_SHAPES[5][5] - 1) // 2 + 1 == 33                                         # the second chunk holds one position
    assert sh[S2_SHAPES[6]] == (2, 20, 1, 20) and [n % 2 for n in S2_SHAPES[6][3:]] == [1, 1, 0]
    # Wo = 32 is a whole chunk of gout, yet its last position's kw = 2 column 2 * 31 + 1 = W lies outside the row: the second half of
    # the kernels' `whole` predicate, (w0 + 32) * 2 + 1 <= W, is what keeps the next row's first value out
    assert sh[S2_SHAPES[7]] == (1, 4, 1, 4) and (S2_SHAPES[7][5] - 1) // 2 + 1 == 32 and 2 * 31 + 1 == S2_SHAPES[7][5]
    # ---- a single output channel: the head kernel (per_wave, nwaves) | the per-wave tile kernel ----
    hd = {s: (f("head", s), f("head", s, False)) for s in HEAD_SHAPES}
    head = {s: (h["chunks_per_row"], h["total_chunks"], h["per_wave"], h["nwaves"]) for s, (h, _) in hd.items()}
    assert head[HEAD_SHAPES[0]] == (3, 81, 1, 81)
    assert head[HEAD_SHAPES[1]] == (5, 660, 2, 330) and _cdiv(330, 4) == 83 and 83 * 4 - 330 == 2 and hd[HEAD_SHAPES[1]][0]["ci_tiles"] == 2
    assert (hd[HEAD_SHAPES[1]][1]["per_unit"], hd[HEAD_SHAPES[1]][1]["nsplit"]) == (8, 83) and 660 - 82 * 8 == 4
    assert head[HEAD_SHAPES[2]] == (1, 1, 1, 1) and hd[HEAD_SHAPES[2]][0]["ci_tiles"] == 2                                     # one chunk, three idle waves
    assert head[HEAD_SHAPES[3]] == (1, 6, 1, 6)
    # ---- roles swapped ----
    assert _live(f("swapped", SWAPPED_SHAPES[0])) == dict(kernel="s2a", ci_tiles=2, tiles=4, chunks_per_row=2, total_chunks=20, ns=20, pu=1)
    assert _live(f("swapped", SWAPPED_SHAPES[1])) == dict(kernel="s2a", ci_tiles=2, tiles=2, chunks_per_row=1, total_chunks=3, ns=3, pu=1)
    # what the region masks name exists
    names = set().union(*(set(_regions(e[2], e[1])) for e in ENTRIES))
    assert {"co_partial_tile", "ci_partial_tile", "tile_co1_ci1", "tile_co0_ci2", "tap000", "tap222"} <= names


@pytest.mark.parametrize("coop", ["1", "0"])
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_bf16_kernels_against_float64_and_the_exact_fp32_kernel(sa, case, coop, tuning_env):
    c = _case(sa, *case)
    tuning_env("SS_WGRAD_COOP", coop)
    _judge(f"{case[0]} {case[1]} {c.form(coop == '1')['kernel']}", c.run(), c.ref, c.y32)


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_exact_fp32_kernel_against_float64(sa, case):
    """the yardstick itself: (1) and (2) on every shape"""
    c = _case(sa, *case)
    _judge(f"{case[0]} {case[1]} f32", c.y32, c.ref)


# one case of each kernel: (kind, shape, SS_WGRAD_COOP, the kernel)
ONE_PER_KERNEL = [("s1", S1_SHAPES[2], "1", "coop"), ("s1", S1_SHAPES[2], "0", "per_wave_s1"), ("s2", S2_SHAPES[2], "1", "s2a"),
                  ("s2", S2_SHAPES[2], "0", "per_wave_s2"), ("head", HEAD_SHAPES[1], "1", "head"), ("s1", S1_SHAPES[2], "1", "f32")]
SENTINEL, MARGIN, OFFSET = -12345.678, 4096, 260       # guard bands of MARGIN floats; the slices start OFFSET floats (a multiple of 4) into the payload area


@pytest.mark.parametrize("kind,shape,coop,kernel", ONE_PER_KERNEL, ids=[k[3] for k in ONE_PER_KERNEL])
def test_dirty_buffers_and_guard_bands(sa, kind, shape, coop, kernel, tuning_env):
    """grad_w and the workspace as slices out of the middle of larger buffers, pre-filled with NaN, sentinels before and after: the
    entry's zero-fills are what makes the atomics' sums right, nothing is written outside tiles * 27 * 1024 floats of workspace and
    Cout * Cin * 27 of grad_w, and the head kernel leaves the workspace alone"""
    c = _case(sa, kind, shape)
    tuning_env("SS_WGRAD_COOP", coop)
    B, Cin, Cout, D, H, W, stride = c.entry
    assert kernel == "f32" or c.form(coop == "1")["kernel"] == kernel

    def guarded(n):
        buf = torch.full((MARGIN + OFFSET + n + MARGIN,), SENTINEL, dtype=torch.float32, device="cuda")
        sl = buf[MARGIN + OFFSET:MARGIN + OFFSET + n]
        sl.fill_(float("nan"))
        assert sl.data_ptr() % 16 == 0
        return buf, sl

    gbuf, gw = guarded(Cout * Cin * 27)
    wbuf, ws = guarded(_ws_floats(Cin, Cout))
    y = _run_f32(c.g, c.x, Cout, stride, gw) if kernel == "f32" else _run_bf16s(c.g, c.x, Cout, stride, gw, ws)
    torch.cuda.synchronize()
    for buf, n in ((gbuf, gw.numel()), (wbuf, ws.numel())):
        lo, hi = buf[:MARGIN + OFFSET], buf[MARGIN + OFFSET + n:]
        assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()) and hi.numel() == MARGIN, kernel
    if kernel in ("head", "f32"):
        assert bool(torch.isnan(ws).all()), "the workspace was written"
    else:
        assert bool(torch.isfinite(ws).all())
    assert bool(torch.isfinite(y).all())
    _judge(f"{kind} {shape} {kernel} dirty buffers", y, c.ref)


# the longest K of each kernel's shapes (test_magnitude_shapes_have_the_longest_k)
LONGEST_K = [("s1", S1_SHAPES[4], "1", "coop"), ("s1", S1_SHAPES[4], "0", "per_wave_s1"), ("s2", S2_SHAPES[2], "1", "s2a"),
             ("s2", S2_SHAPES[2], "0", "per_wave_s2"), ("head", HEAD_SHAPES[1], "1", "head"), ("s1", S1_SHAPES[4], "1", "f32")]


@pytest.mark.parametrize("exp", [-100, -40, 40])
@pytest.mark.parametrize("kind,shape,coop,kernel", LONGEST_K, ids=[k[3] for k in LONGEST_K])
def test_gradients_of_any_magnitude(sa, kind, shape, coop, kernel, exp, tuning_env):
    """the kernel file's "gradients of any magnitude need no scaling": grad_out times 2^-100, 2^-40, 2^40 on the longest K of each
    kernel's shapes; (1) and (2) against the reference times the same power of two (exact in float64), nothing non-finite"""
    c = _case(sa, kind, shape)
    tuning_env("SS_WGRAD_COOP", coop)
    assert kernel == "f32" or c.form(coop == "1")["kernel"] == kernel
    g = c.g * 2.0 ** exp
    assert torch.equal(g.double().cpu(), c.g_cpu.double() * 2.0 ** exp), "the scaled seed is not exact in fp32"
    Cout, stride = c.entry[2], c.entry[6]
    y = _run_f32(g, c.x, Cout, stride) if kernel == "f32" else _run_bf16s(g, c.x, Cout, stride)
    _judge(f"{kind} {shape} {kernel} grad_out x 2^{exp}", y, c.ref * 2.0 ** exp)


def test_magnitude_shapes_have_the_longest_k():
    def K(kind, s):
        B, _cin, _cout, D, H, W, stride = _entry(kind, s)
        return B * ((D - 1) // stride + 1) * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
    assert max(S1_SHAPES, key=lambda s: K("s1", s)) == S1_SHAPES[4] and K("s1", S1_SHAPES[4]) == 4000
    assert max(S2_SHAPES, key=lambda s: K("s2", s)) == S2_SHAPES[2] and K("s2", S2_SHAPES[2]) == 1680
    assert max(HEAD_SHAPES, key=lambda s: K("head", s)) == HEAD_SHAPES[1] and K("head", HEAD_SHAPES[1]) == 34320


BATCH_CASES = [c for c in CASES if c[1][0] == 2]


@pytest.mark.parametrize("coop", ["1", "0"])
@pytest.mark.parametrize("case", BATCH_CASES, ids=_ids(BATCH_CASES))
def test_batch_of_two_is_the_sum_of_its_pairs(sa, case, coop, tuning_env):
    """dW(B = 2) against dW(pair 0) + dW(pair 1): each of the three by (2) against its own float64 reference, the sum against the
    B = 2 reference as well.  (The kernels add with atomics: no two runs are asserted to agree bit for bit.)"""
    c = _case(sa, *case)
    tuning_env("SS_WGRAD_COOP", coop)
    stride = c.entry[6]
    kern = c.form(coop == "1")["kernel"]
    _judge(f"{case[0]} {case[1]} {kern} B=2", c.run(), c.ref)
    total = torch.zeros_like(c.ref)
    ref_total = torch.zeros_like(c.ref)
    for b in range(2):
        g, x = c.g[b:b + 1].contiguous(), c.x[b:b + 1].contiguous()
        ref_b = _reference(case[0], c.g_cpu[b:b + 1], c.x_cpu[b:b + 1], stride)
        y = c.run(g, x)
        _judge(f"{case[0]} {case[1]} {kern} pair {b} alone", y, ref_b)
        total += y.double().cpu()
        ref_total += ref_b
    assert float((ref_total - c.ref).abs().max()) <= 1e-12 * float(c.ref.abs().max())          # the reference is additive to float64 rounding
    _judge(f"{case[0]} {case[1]} {kern} pair 0 + pair 1", total, c.ref)


def test_conv3d_train_sends_odd_extents_at_stride_2_to_the_stock_layer(sa):
    """the C entry takes odd extents at stride 2 (above); conv3d_train does not -- the data gradient of a stride-2 layer is the k3-s2-p1-op1
    transposed conv, which needs even sizes -- and must take the stock layer, with the bounds of
    test_conv3d_training_forward_dgrad_wgrad_in_hip (tests/test_parity_gpu.py)"""
    B, Cin, Cout, D, H, W = 1, 16, 32, 3, 5, 31
    x = dd.t_normalish((B, Cin, D, H, W), 830)
    w = dd.t_uniform((Cout, Cin, 3, 3, 3), 831, -1, 1) * (3.0 / (Cin * 27)) ** 0.5
    conv = torch.nn.Conv3d(Cin, Cout, 3, 2, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(w)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = F.conv3d(x64, w64, None, 2, 1)
    seed = dd.t_normalish(tuple(y64.shape), 832)
    y64.backward(seed.double())
    conv = conv.cuda()
    xg = x.cuda().requires_grad_(True)
    counts = sa.modules.PATH_COUNTS
    before = (counts["torch"], counts.get("hip_train", 0))
    y = sa.modules.conv3d_train(conv, xg)
    assert (counts["torch"], counts.get("hip_train", 0)) == (before[0] + 1, before[1]), "an odd extent at stride 2 went to the HIP function"
    y.backward(seed.cuda())
    scale = lambda t: float(t.detach().abs().max())                        # noqa: E731
    e_y = float((y.detach().double().cpu() - y64.detach()).abs().max()) / scale(y64)
    e_x = float((xg.grad.double().cpu() - x64.grad).abs().max()) / scale(x64.grad)
    e_w = float((conv.weight.grad.double().cpu() - w64.grad).abs().max()) / scale(w64.grad)
    line = f"conv3d_train stride 2 {(B, Cin, Cout, D, H, W)} stock layer: e_y {e_y:.3e} e_x {e_x:.3e} e_w {e_w:.3e} (of the largest |reference|)"
    print(line)
    _TABLE.append(line)
    assert e_y <= 2e-6 and e_x <= 2e-6 and e_w <= 5e-6, (e_y, e_x, e_w)
