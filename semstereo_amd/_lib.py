"""ctypes binding of libsemstereo_hip.so (the C ABI declared in include/semstereo_hip.h).

There is deliberately NO fallback: if the shared library is missing or a kernel
returns an error, the caller gets an exception.  PyTorch is used only for
device memory and streams; the signatures carry raw pointers and sizes.

The header is the one definition of the boundary: load() reads every declaration of it and binds it.  A parameter is an int,
a long long, a float, a double, an ss_stream_t or (anything with a `*`) a pointer; any other type is an error, never a guess.
"""
import ctypes
import os
import re

import torch  # noqa: F401  (must be imported first: it loads the HIP runtime the library binds to)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsemstereo_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "semstereo_hip.h")
ABI_VERSION = 20

_SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double,
            "ss_stream_t": ctypes.c_void_p}
_RETURNS = {"int": ctypes.c_int, "const char*": ctypes.c_char_p}
_DECLARATION = re.compile(r"([\w \t*]+?)\s*\b(ss_\w+)\s*\(([^()]*)\)\s*;")

_SIGNATURES = {}      # name -> argument types of every declared function (filled by load())
EXPORTS = []          # every declared name, sorted (filled by load())
_lib = None
_BYTES = {}           # (query, args) -> bytes: the size queries are pure functions of their arguments


class SemStereoHipError(RuntimeError):
    pass


def _ctype(param, decl):
    if "*" in param:
        return ctypes.c_void_p
    words = [w for w in param.split() if w != "const"]
    for kind in (" ".join(words), " ".join(words[:-1])):       # without and with a parameter name
        if kind in _SCALARS:
            return _SCALARS[kind]
    raise SemStereoHipError(f"include/semstereo_hip.h: `{decl}`: parameter `{param}` is none of int, long long, float, double, "
                            f"ss_stream_t or a pointer")


def parse_header(text):
    """C declarations `(int|const char*) ss_name(params);` -> {name: (restype, [argtypes])} in ctypes classes."""
    out = {}
    for m in _DECLARATION.finditer(re.sub(r"/\*.*?\*/", "", text, flags=re.S)):
        decl = " ".join(m.group(0).split())
        ret = re.sub(r"\s*\*", "*", " ".join(m.group(1).split()))
        if ret not in _RETURNS:
            raise SemStereoHipError(f"include/semstereo_hip.h: `{decl}`: return type `{ret}` is neither int nor const char*")
        params = [p.strip() for p in m.group(3).split(",")]
        if params in ([""], ["void"]):
            params = []
        out[m.group(2)] = (_RETURNS[ret], [_ctype(p, decl) for p in params])
    return out


def load():
    """Load the shared library once and bind every declaration of the header; raise (never fall back) if that is impossible."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SemStereoHipError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C semstereo_amd/csrc`. There is no CPU or PyTorch fallback for the HIP path.")
    lib = ctypes.CDLL(LIB_PATH)
    with open(HEADER_PATH) as f:
        declared = parse_header(f.read())
    for name, (restype, argtypes) in declared.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.ss_abi_version() != ABI_VERSION:
        raise SemStereoHipError(f"ABI mismatch: library {lib.ss_abi_version()} != binding {ABI_VERSION}; rebuild")
    _SIGNATURES.update((name, argtypes) for name, (_, argtypes) in declared.items())
    EXPORTS[:] = sorted(declared)
    _lib = lib
    return lib


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def call(name, *args):
    """Invoke an entry point on the current stream; raise on a non-zero status."""
    lib = load()
    status = getattr(lib, name)(*args, stream())
    if status != 0:
        msg = lib.ss_status_string(status).decode()
        if status == -3:
            msg += ": " + lib.ss_last_hip_error().decode()
        raise SemStereoHipError(f"{name} failed ({status}): {msg}")


def query_bytes(name, *args):
    """The answer of a `*_bytes` query -- a `*_workspace_bytes` scratch size or an `ss_pack_*_bytes` packed-weight size (no stream,
    no device: asked once per argument list)."""
    if (name, args) not in _BYTES:
        n = ctypes.c_longlong(0)
        status = getattr(load(), name)(*args, ctypes.byref(n))
        if status != 0:
            raise SemStereoHipError(f"{name} failed ({status})")
        _BYTES[(name, args)] = int(n.value)
    return _BYTES[(name, args)]


def require_device(*tensors):
    """Every tensor must be fp32 on a HIP device; anything else is an error (no fallback)."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise SemStereoHipError("semstereo_amd ops run on MI355X only: got a CPU tensor (no CPU fallback exists)")
        if t.dtype != torch.float32:
            raise TypeError(f"semstereo_amd ops are fp32 like the reference, got {t.dtype}")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise SemStereoHipError("all tensors of one call must live on the same device")
    return dev
