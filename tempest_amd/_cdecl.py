"""The ctypes tables of the package, read from the C declarations they bind: include/tempest_hip.h for libtempest_hip.so (_lib.py),
the extern "C" block of a rendered plugin text for a HipCallbacks plugin (hipcallbacks.py).  Not a C parser: a closed rule over the
flat declarations those texts hold, which raises on anything else instead of skipping it."""
import ctypes as C
import re


class TempestHipError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double}


def constants(text: str) -> dict:
    """{name: value} of the lines `#define TPH_NAME <integer>`."""
    return {name: int(value) for name, value in re.findall(r"^#define (TPH_\w+) (-?\d+)\s*$", text, re.M)}


def prototypes(text: str, prefix: str) -> dict:
    """{name: (restype, [argtypes])} of every function `prefix*` declared (`;`) or defined (`{`) at the top level of `text` -- of its
    last extern "C" block where it has one.  Comments and preprocessor lines are dropped, bodies skipped, line breaks are blanks."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*|^[ \t]*#[^\n]*", " ", text, flags=re.S | re.M)
    flat, depth = [], 0
    for piece in re.split(r"([{}])", re.split(r'extern\s+"C"\s*\{', text)[-1]):
        depth += (piece == "{") - (piece == "}")
        if depth < 0:                        # the brace that closes the extern "C" block
            break
        if depth == 0:
            flat.append(";" if piece == "}" else piece)
    flat = "".join(flat)
    fn_types = re.findall(r"typedef[^;(]*\(\s*\*\s*(\w+)\s*\)", flat)       # function-pointer typedefs: passed as addresses
    out = {}

    def ctype(decl, name, ret=False):
        words = re.sub(r"\bconst\b", " ", decl).replace("*", " * ").split()
        first = words[0] if words else ""
        if ret and words == ["char", "*"]:
            return C.c_char_p
        if not ret and ("*" in words or first in fn_types):
            return C.c_void_p
        if first in _SCALARS and len(words) <= (1 if ret else 2):        # the type [and the parameter's name]
            return _SCALARS[first]
        raise TempestHipError(f"{name}: {' '.join(decl.split())!r} is outside the binding rule")

    for ret, name, params in re.findall(rf"(?:^|;)\s*([\w\s*]+?)\s*\b({prefix}\w*)\s*\(([^();]*)\)\s*(?=;)", flat):
        row = (ctype(ret, name, True), [ctype(p, name) for p in params.split(",")] if params.strip() not in ("", "void") else [])
        if out.setdefault(name, row) != row:
            raise TempestHipError(f"{name}: declared twice, differently")
    seen = set(re.findall(rf"\b({prefix}\w*)\s*\(", flat))
    if not out or seen != set(out):
        raise TempestHipError(f"declarations of {prefix}* not understood: {sorted(seen ^ set(out)) or 'none found'}")
    return out
