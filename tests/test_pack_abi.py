"""CPU: every `ss_pack_*` entry point that fills a buffer of split fragments has a `_bytes` twin, and the twin's answer is the size
the Python side allocated before the library stated it -- the expressions below, in int16 elements as `torch.empty` took them, kept
here as the independent statement.  No device call is made."""
import ctypes

import pytest

from abi import declared, library

LL = ctypes.c_longlong


def cdiv(a, b):
    return -(-a // b)


#: pack -> (names of its scalar arguments in call order, int16 elements of its buffer)
PACKS = {
    "ss_pack_conv3d_weights_bf16s": (("Cout", "Cin"), lambda Cout, Cin: cdiv(Cin, 8) * 14 * 3 * 2 * Cout * 8),
    "ss_pack_conv3d_weights_f16s": (("Cout", "Cin"), lambda Cout, Cin: cdiv(Cin, 8) * 14 * 2 * 2 * Cout * 8 + 2 * Cout),
    "ss_pack_conv2d_weights_bf16s": (("Cout", "Cin"), lambda Cout, Cin: cdiv(Cin, 8) * 5 * 3 * 2 * Cout * 8),
    "ss_pack_conv2d_weights_f16s": (("Cout", "Cin"), lambda Cout, Cin: cdiv(Cin, 8) * 5 * 2 * 2 * Cout * 8 + 2 * Cout),
    "ss_pack_deconv3d_weights_bf16s": (("Cin", "Cout", "ntaps"), lambda Cin, Cout, ntaps: cdiv(Cin, 16) * ntaps * 3 * 2 * Cout * 8),
    "ss_pack_deconv3d_weights_f16s": (("Cin", "Cout"), lambda Cin, Cout: cdiv(Cin, 16) * 27 * 2 * 2 * Cout * 8 + 2 * Cout),
    "ss_pack_deconv2d_weights_f16s": (("Cin", "Cout"),
                                      lambda Cin, Cout: cdiv(Cin, 8) * cdiv(Cout, 32) * 16 * 64 * 8 + 2 * 32 * cdiv(Cout, 32)),
    "ss_pack_conv2d_k4s2_weights_f16s": (("Cout", "Cin"),
                                         lambda Cout, Cin: cdiv(Cin, 8) * cdiv(Cout, 32) * 16 * 64 * 8 + 2 * 32 * cdiv(Cout, 32)),
    "ss_pack_conv2d_k1_weights_f16s": (("Cout", "Cin"),
                                       lambda Cout, Cin: cdiv(Cin, 32) * cdiv(Cout, 32) * 256 * 8 + 2 * 32 * cdiv(Cout, 32)),
    "ss_pack_seghead_weights_f16s": (("Cin",), lambda Cin: (Cin // 8) * 640 * 8 + 2 * 32),
    "ss_pack_conv3d_head_weights_bf16s": (("Cin",), lambda Cin: (Cin // 16) * 3 * 2 * 32 * 8),
    "ss_pack_conv3d_head_weights_f16s": (("Cin",), lambda Cin: (Cin // 16) * 2 * 2 * 32 * 8 + 8),
    "ss_pack_pointwise_weights_bf16s": (("Cout", "Cin"), lambda Cout, Cin: cdiv(Cout, 32) * (Cin // 16) * 3 * 2 * 32 * 8),
    "ss_pack_stem_left_weights_f16s": (("Cout", "C"), lambda Cout, C: 4 * 9 * 2 * 2 * 64 * 8 + 2 * 4 * 9 * 24),
    "ss_pack_classifier_head_weights": ((), lambda: 3 * 2 * 64 * 8),
}
#: (Cout, Cin): a channel count below one tile, one that is no multiple of the tile (32), an input count that is no multiple of the
#: chunk (8, 16 or 32), and the largest layer of the model
GENERAL = ((1, 1), (6, 8), (32, 16), (33, 17), (40, 70), (384, 768))


def cases(name):
    """The argument tuples (in the pack's own order) a pack is checked at."""
    names = PACKS[name][0]
    if name == "ss_pack_pointwise_weights_bf16s":
        return [(33, 16), (40, 48), (384, 128)]
    if name == "ss_pack_stem_left_weights_f16s":
        return [(32, 32)]
    if names == ("Cin",):
        return [(c,) for c in ((8, 24, 136) if "seghead" in name else (16, 32, 64))]
    if names == ():
        return [()]
    out = [tuple({"Cout": Cout, "Cin": Cin}[n] for n in names[:2]) for Cout, Cin in GENERAL]
    return [c + (t,) for c in out for t in (1, 27)] if "ntaps" in names else out


def test_there_are_fifteen_and_each_has_a_twin_with_the_packs_scalar_parameters():
    decl = declared()
    packs = sorted(n for n in decl if n.startswith("ss_pack_") and not n.endswith("_bytes") and n != "ss_pack_conv3d_weights")
    assert packs == sorted(PACKS) and len(packs) == 15
    assert sorted(n for n in decl if n.startswith("ss_pack_") and n.endswith("_bytes")) == sorted(p + "_bytes" for p in packs)
    for p in packs:
        scalars = [t for t in decl[p][1] if not t.endswith("*") and t != "ss_stream_t"]
        assert decl[p][0] == "int" and decl[p][1][-1] == "ss_stream_t" and len(scalars) == len(PACKS[p][0]), p
        assert decl[p + "_bytes"] == ("int", scalars + ["long long*"]), (p, decl[p + "_bytes"])


@pytest.mark.parametrize("name", sorted(PACKS))
def test_the_query_is_the_expression_python_allocated(name):
    _l, lib = library()
    query, formula = getattr(lib, name + "_bytes"), PACKS[name][1]
    for args in cases(name):
        n = LL(-1)
        assert query(*args, ctypes.byref(n)) == 0 and n.value == 2 * formula(*args) > 0, (name, args, n.value)
        for _ in range(2):                                      # the second answer comes from the memo
            got = _l.query_bytes(name + "_bytes", *args)
            assert type(got) is int and got == n.value, (name, args, got)


def test_the_documented_sizes():
    _l, lib = library()
    n = LL(-1)
    assert lib.ss_pack_classifier_head_weights_bytes(ctypes.byref(n)) == 0 and n.value == 6144
    assert lib.ss_pack_stem_left_weights_f16s_bytes(32, 32, ctypes.byref(n)) == 0 and n.value == 150912
    assert lib.ss_pack_conv3d_head_weights_f16s_bytes(32, ctypes.byref(n)) == 0 and n.value == 2 * 2 * 2 * 32 * 16 + 16   # one float in a 16-byte tail
    assert lib.ss_abi_version() == _l.ABI_VERSION == 20


@pytest.mark.parametrize("name", sorted(PACKS))
def test_refusals_return_their_status_and_write_nothing(name):
    _l, lib = library()
    query, good = getattr(lib, name + "_bytes"), cases(name)[-1]
    n = LL(-7)
    assert query(*good, None) == -1                             # NULL `bytes`
    for i in range(len(good)):                                  # each dimension zero and negative
        for bad in (0, -good[i]):
            assert query(*good[:i], bad, *good[i + 1:], ctypes.byref(n)) == -1, (name, i, bad)
    own = {"ss_pack_seghead_weights_f16s": (((12,), -1), ((7,), -1)),
           "ss_pack_conv3d_head_weights_bf16s": (((24,), -1),), "ss_pack_conv3d_head_weights_f16s": (((8,), -1),),
           "ss_pack_pointwise_weights_bf16s": (((32, 24), -1),),
           "ss_pack_stem_left_weights_f16s": (((32, 64), -2), ((16, 32), -2), ((64, 64), -2)),
           "ss_pack_deconv3d_weights_bf16s": (((16, 16, 3), -1), ((16, 16, 9), -1), ((16, 16, 26), -1))}
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                       # 16-byte aligned host memory that is never followed
    for args, status in own.get(name, ()):                      # what the pack itself refuses, with the pack's status
        assert query(*args, ctypes.byref(n)) == status, (name, args)
        assert getattr(lib, name)(p, p, *args, None) == status, (name, args)
    assert n.value == -7
    if good:
        with pytest.raises(_l.SemStereoHipError, match=name + r"_bytes failed \(-1\)"):
            _l.query_bytes(name + "_bytes", *good[:-1], 0)
