"""What the ABI tests share (test infrastructure, like strict.py): the tests' OWN reading of include/semstereo_hip.h -- written
apart from the parser of semstereo_amd/_lib.py, which it checks -- and the loaded library."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "semstereo_hip.h")


def declared(text=None):
    """name -> (return C type, [parameter C types, the names dropped]) of every `ss_*` declaration, e.g.
    "ss_tool_copy_fwd": ("int", ["const void*", "void*", "long long", "ss_stream_t"])."""
    if text is None:
        text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"^[ \t]*(int|const\s+char\s*\*)\s*(ss_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S | re.M):
        params = []
        for arg in m.group(3).split(","):
            arg = " ".join(arg.split())
            if arg in ("", "void"):
                continue
            kind = re.fullmatch(r"(.*?[\s*])\w+", arg)            # everything before the parameter's name; a `*` belongs to the type
            assert kind, (m.group(2), arg)
            params.append(re.sub(r"\s*\*", "*", kind.group(1)).strip())
        out[m.group(2)] = ("int" if m.group(1) == "int" else "const char*", params)
    return out


def library():
    """(semstereo_amd._lib, the loaded library), built first if it is missing."""
    import __graft_entry__ as ge
    from semstereo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib, _lib.load()
