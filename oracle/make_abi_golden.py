"""Record the HAND-WRITTEN ctypes tables of the host layer (tests/golden/abi_tables.json; tests/test_abi_tables.py compares what the
declaration reader derives from include/tempest_hip.h and from the plugin texts against it).

    python -m oracle.make_abi_golden          # on the last commit that still has the hand tables

It was run once, on the commit before the tables were replaced by tempest_amd/_cdecl.py, and is kept as the record of how the golden
came about: it reads _lib.SIGNATURES as a literal, the constants device.py spelled out, and what _Parts.bind(lib, n_dim, path) set on
a plugin from its `fns` dict and the argtypes column of _PARTS -- none of which exist afterwards.  It does not import the reader.

  prototypes  {name: [restype, [argtypes]]} by ctypes type name, POINTER(...) written as c_void_p
  constants   every upper-case int of device.py, KERNEL_ID and HipContext.P2P_HANDLE_BYTES
  plugin      rows: {"entry|0" or "entry|1" (data-carrying): its argtypes by name}, once each; cases: {id: [0 | 1, [entries bound]]}
              over the combinations of oracle/make_plugin_texts.cases(); every bound entry returned c_int
"""
import ctypes as C
import json
import os

from oracle import make_plugin_texts as texts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_tables.json")

NAMES = {C.c_int: "c_int", C.c_int64: "c_int64", C.c_uint64: "c_uint64", C.c_uint32: "c_uint32", C.c_double: "c_double",
         C.c_void_p: "c_void_p", C.c_char_p: "c_char_p"}


def type_name(t):
    return "c_void_p" if issubclass(t, C._Pointer) else NAMES[t]


class _Fn:
    """Stands in for a function of a loaded plugin: keeps what bind assigns, answers the handshakes bind makes before it assigns."""
    argtypes = restype = None

    def __init__(self, value):
        self.value = value

    def __call__(self, *a):
        return self.value


class _Lib:
    def __init__(self, answers):
        self.fns, self.answers = {}, answers

    def __getattr__(self, name):
        return self.fns.setdefault(name, _Fn(self.answers.get(name, 0)))


def plugin_tables():
    from tempest_amd import hipcallbacks as H
    rows, cases = {}, {}
    for cid, ((source, tables, term), kw), (_, kkw) in texts.cases():
        parts = H._Parts.of(source, tables, term, kkw["n_derived"], kw["predict"], kw["pointwise"], kw["replicate"], kkw["discrepancy"])
        words = 0 if parts.tables is None else sum(1 + rank for _, rank in parts.tables) + 1
        lib = _Lib({"tphu_data_abi": 1, "tphu_data_size": 8 * words, "tphu_n_dim": texts.N_DIM})
        try:
            parts.bind(lib, texts.N_DIM, "golden")
        except H.TempestHipError:            # a layout handshake the stand-in does not answer: the prototypes are set before it
            pass
        on = int(parts.tables is not None)
        bound = sorted(name for name, fn in lib.fns.items() if fn.argtypes is not None)
        for name in bound:
            fn = lib.fns[name]
            assert fn.restype is C.c_int, name
            args = [type_name(t) for t in fn.argtypes]
            assert rows.setdefault(f"{name}|{on}", args) == args, name
        cases[cid] = [on, bound]
    return {"rows": rows, "cases": cases}


def record():
    from tempest_amd import _lib, device
    protos = {name: [type_name(res), [type_name(t) for t in args]] for name, (res, args) in _lib.SIGNATURES.items()}
    consts = {k: v for k, v in vars(device).items() if k.isupper() and isinstance(v, int) and not isinstance(v, bool)}
    consts["P2P_HANDLE_BYTES"] = device.HipContext.P2P_HANDLE_BYTES
    return {"prototypes": protos, "constants": consts, "kernel_id": dict(device.KERNEL_ID), "plugin": plugin_tables()}


if __name__ == "__main__":
    rec = record()
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec['prototypes'])} prototypes, {len(rec['constants'])} constants, {len(rec['plugin']['cases'])} plugin cases, "
          f"{len(rec['plugin']['rows'])} distinct rows -> {GOLDEN}")
