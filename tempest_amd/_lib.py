"""ctypes binding of libtempest_hip.so (C ABI: include/tempest_hip.h).

The product path has no CPU fallback: if the shared library is missing or a call fails this
module raises.  Build with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C tempest_amd/csrc``.
"""
import ctypes as C
import os

from ._cdecl import TempestHipError, constants, prototypes

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libtempest_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "tempest_hip.h")
with open(HEADER_PATH) as _f:
    _header = _f.read()
# name -> (restype, argtypes) of every function the header declares, and its #define TPH_* integers: read from the declarations
# (_cdecl.py: pointers of any kind are c_void_p, which takes an int, None, a ctypes pointer or byref(...))
SIGNATURES = prototypes(_header, "tph_")
CONSTANTS = constants(_header)

# host collectives handed to tph_comm_attach (see include/tempest_hip.h): written out, because callers construct them
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int)

_lib = None


def load(path=None):
    """Load the shared library and attach prototypes.  Raises if it is missing or incomplete."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    # torch bundles its own HIP/HSA runtime; it must be in the process BEFORE our library is loaded so that both
    # resolve to the same libamdhip64 (loading ROCm's copy first leaves the process with two HSA runtimes and
    # "no ROCm-capable device is detected")
    import torch  # noqa: F401
    if not os.path.exists(p):
        raise TempestHipError(
            f"{p} not found: the HIP extension is not built (run `make -C tempest_amd/csrc`). "
            "tempest_amd has no CPU fallback.")
    lib = C.CDLL(p)
    missing = []
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    if missing:
        raise TempestHipError(f"{p} lacks symbols declared in include/tempest_hip.h: {missing}")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().tph_last_error()
        raise TempestHipError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")
