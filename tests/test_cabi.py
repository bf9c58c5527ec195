"""CPU: the C-ABI shared library loads (no GPU needed for dlopen) and exports exactly the entry
points include/semstereo_hip.h declares, bound with the types the header gives them.
No compute call is made here."""
import ctypes

import pytest

from abi import declared, library

#: the parameter kinds of the header, as the tests read them (anything with a `*` is a pointer)
CTYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double,
          "ss_stream_t": ctypes.c_void_p}
RESTYPES = {"int": ctypes.c_int, "const char*": ctypes.c_char_p}


@pytest.fixture(scope="module")
def lib():
    return library()[1]


def test_header_declares_something():
    d = declared()
    assert len(d) >= 20 and "ss_gwc_volume_fwd" in d and "ss_conv3d_fwd" in d


def test_every_declared_symbol_is_exported(lib):
    for name in declared():
        assert hasattr(lib, name), f"{name} is declared in include/semstereo_hip.h but not exported"


def test_binding_matches_header(lib):
    """Type by type: a `long long` bound as an int, or a `double` as a float, has the right count and truncates on the device."""
    from semstereo_amd import _lib
    decl = declared()
    assert _lib.EXPORTS == sorted(decl) and set(_lib._SIGNATURES) == set(decl)
    kinds = set()
    for name, (ret, params) in decl.items():
        expected = [ctypes.c_void_p if p.endswith("*") else CTYPES[p] for p in params]
        fn = getattr(lib, name)
        assert list(fn.argtypes) == expected == list(_lib._SIGNATURES[name]), (name, params, fn.argtypes)
        assert fn.restype is RESTYPES[ret], (name, ret, fn.restype)
        kinds.update("*" if p.endswith("*") else p for p in params)
    assert kinds == set(CTYPES) | {"*"}                        # every kind is met, so every row of the mapping is checked
    assert decl["ss_tool_copy_fwd"] == ("int", ["const void*", "void*", "long long", "ss_stream_t"])
    assert lib.ss_batchnorm_train_fwd_rs.argtypes[12] is ctypes.c_double and lib.ss_conv_k1_wgrad_fwd.argtypes[6] is ctypes.c_longlong


def test_the_parser_refuses_a_type_it_does_not_know():
    from semstereo_amd import _lib
    ok = "/* a comment, int ss_not_this(short x); */\nint ss_a(const float* x, long long n, ss_stream_t stream);\nconst char* ss_b(void);\n"
    parsed = _lib.parse_header(ok)
    assert parsed == {"ss_a": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]), "ss_b": (ctypes.c_char_p, [])}
    for bad in ("int ss_c(const float* x, unsigned n);", "int ss_c(size_t n, ss_stream_t stream);", "int ss_c(long n);",
                "float ss_c(int n);", "int ss_c(hipStream_t stream);"):
        with pytest.raises(_lib.SemStereoHipError, match="ss_c"):
            _lib.parse_header(ok + bad)


def test_query_bytes_is_the_raw_query(lib):
    """Each workspace query through _lib.query_bytes and through the module that owns it gives what a raw byref call gives.  (The
    eighth scratch size, train_ssr.workspace_bytes, is a formula in Python: the header has no entry point for it.)"""
    import torch
    from semstereo_amd import _lib, data, losses, metrics, train, train_decoder, train_heads, visualization
    queries = (("ss_loss_workspace_bytes", (1,), lambda: losses.workspace_bytes(1)),
               ("ss_metrics_workspace_bytes", (0,), lambda: metrics.workspace_bytes(0)),
               ("ss_vis_workspace_bytes", (0,), visualization.workspace_bytes),
               ("ss_prep_workspace_bytes", (2, 37, 53), lambda: data.workspace_bytes(2, 37, 53)),
               ("ss_seghead_tail_workspace_bytes", (3, 32, 6, 9, 33), lambda: train_heads.tail_workspace(3, 6, 9, 33, "cpu").numel() * 4),
               ("ss_deconv2d_k4s2_wgrad_workspace_bytes", (7, 70, 23, 37, 40), lambda: train_decoder.wgrad_workspace_bytes(7, 70, 23, 37, 40)),
               ("ss_conv2d_k3_wgrad_workspace_bytes", (2, 16, 0, 40, 70, 16), lambda: train.conv2d_k3_wgrad_workspace_bytes(2, 16, 0, 40, 70, 16)))
    assert sorted(q[0] for q in queries) == [n for n in _lib.EXPORTS if n.endswith("_workspace_bytes")]
    for name, args, owner in queries:
        n = ctypes.c_longlong(-1)
        assert getattr(lib, name)(*args, ctypes.byref(n)) == 0 and n.value > 0, name
        for _ in range(2):                                      # the second answer comes from the memo
            got = _lib.query_bytes(name, *args)
            assert type(got) is int and got == n.value == owner(), (name, got, n.value)
    with pytest.raises(_lib.SemStereoHipError, match=r"ss_loss_workspace_bytes failed \(-1\)"):
        _lib.query_bytes("ss_loss_workspace_bytes", 7)
    assert isinstance(train_heads.tail_workspace(3, 6, 9, 33, "cpu"), torch.Tensor)


def test_abi_version_and_status_strings(lib):
    from semstereo_amd import _lib
    assert lib.ss_abi_version() == _lib.ABI_VERSION
    assert lib.ss_status_string(0) == b"ok"
    assert b"invalid" in lib.ss_status_string(-1)
    assert b"not supported" in lib.ss_status_string(-2)


def test_invalid_arguments_are_rejected_before_any_launch(lib):
    """NULL pointers / bad sizes return SS_ERR_INVALID without touching a device."""
    assert lib.ss_gwc_volume_fwd(None, None, None, 1, 8, 4, 4, -2, 4, 2, 0, None) == -1
    assert lib.ss_conv3d_fwd(None, None, None, None, None, None, None, 1, 1, 1, 1, 1, 1, 3, 1, 0, None) == -1
    assert lib.ss_regression_topk_fwd(None, None, None, 1, 4, 2, 2, 2, None) == -1
