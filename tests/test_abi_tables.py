"""The ctypes tables are READ from the C declarations (tempest_amd/_cdecl.py).  CPU only, no compiler: what the reader derives from
include/tempest_hip.h and from every plugin text equals the hand-written tables of the commit before (tests/golden/abi_tables.json,
oracle/make_abi_golden.py), and it raises on a declaration it cannot classify instead of skipping it."""
import ctypes as C
import json
import os
import re

import pytest

from oracle import make_plugin_texts as M
from tempest_amd import _lib, cluster, device, hipcallbacks as H, marginals
from tempest_amd._cdecl import constants, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_tables.json")))
HEADER = open(_lib.HEADER_PATH).read()


def types(names):
    return [getattr(C, name) for name in names]


def test_library_prototypes_equal_the_hand_table():
    got = prototypes(HEADER, "tph_")
    assert len(got) == 79 and got == _lib.SIGNATURES
    assert got == {name: (getattr(C, res), types(args)) for name, (res, args) in GOLD["prototypes"].items()}


def test_constants_cover_the_hand_block_and_the_names_it_lacked():
    assert _lib.CONSTANTS == constants(HEADER)
    for name, value in GOLD["constants"].items():            # the tags are not in the header: test_rng_tags_are_one_number_space
        assert getattr(device, name) == value and (name.startswith("TAG_") or _lib.CONSTANTS["TPH_" + name] == value), name
    assert device.KERNEL_ID == GOLD["kernel_id"] and device.HipContext.P2P_HANDLE_BYTES == GOLD["constants"]["P2P_HANDLE_BYTES"]
    for name, value in (("OPT_PROPOSE_VARIANT", 0), ("OPT_REDUCE_GRID", 1), ("OPT_REDRAW_LANES", 2), ("MARGINALS_TILES", 7), ("VERSION", 100)):
        assert name not in GOLD["constants"] and f"\n#define TPH_{name} {value}\n" in HEADER and getattr(device, name) == value
    assert len(marginals.MARGINAL_TILE_KEYS) == device.MARGINALS_TILES


def test_plugin_prototypes_equal_the_hand_tables_for_every_combination():
    rows, cases = GOLD["plugin"]["rows"], dict(GOLD["plugin"]["cases"])
    for cid, ((source, tables, term), kw), (_, kkw) in M.cases():
        parts = H._Parts.of(source, tables, term, kkw["n_derived"], kw["predict"], kw["pointwise"], kw["replicate"], kkw["discrepancy"])
        got, (on, bound) = prototypes(parts.text(source), "tphu_"), cases.pop(cid)
        # bind declares what the hand tables declared, and tphu_last_error (which had its restype alone)
        assert sorted(H._ENTRIES + tuple(p.entry for p in parts.present() if p.entry)) == sorted(bound + ["tphu_last_error"]), cid
        assert {name: got[name] for name in bound} == {name: (C.c_int, types(rows[f"{name}|{on}"])) for name in bound}, cid
        assert got["tphu_last_error"] == (C.c_char_p, []) and on == (parts.tables is not None)
    assert cases == {} and len(GOLD["plugin"]["cases"]) == 216


@pytest.mark.parametrize("text, word", [
    ("int tph_f(tph_ctx* ctx, float x);", "tph_f"),                              # scalar types outside the rule
    ("float tph_f(tph_ctx* ctx);", "tph_f"),
    ("typedef struct { int a; } tph_pair;\nint tph_g(tph_pair p);", "tph_g"),    # a struct by value
    ("int tph_ok(int a);\nint tph_h(int a) __attribute__((unused));", "tph_h"),  # found by the loose scan, missed by the strict pattern
    ("int tph_ok(int a);\nint tph_h(int (*cb)(int), int a);", "tph_h"),
    ("int tph_ok(int a);\nint tph_ok(int64_t a);", "tph_ok"),                    # two declarations that disagree
    ("", "none found"),
    ("/* int tph_f(int a); */\n#define TPH_X 1\n", "none found"),
])
def test_the_reader_raises_on_what_it_cannot_classify(text, word):
    with pytest.raises(_lib.TempestHipError, match=word):
        prototypes(text, "tph_")


def test_comments_line_breaks_bodies_and_earlier_extern_blocks():
    text = """extern "C" { int tph_user(float x) { return 0; } }
    static int tph_helper(float x) { return tph_user(x); }
    extern "C" {
    typedef int (*tph_cb_fn)(void* user, int64_t n);
    int tph_f(tph_ctx* ctx, int kernel, double* u_dev /* in; with pending_dev
                                                         also out */,
              int64_t n,   // rows
              uint64_t seed, uint32_t tick,
              double beta, tph_cb_fn cb /* or NULL */, const uint8_t* pending_dev /* NULL, or the mask (written, by the
                                                                                     previous step); particles */);
    int64_t tph_g(void);
    const char* tph_h(void) { if (tph_g()) { tph_helper(1.0f); } return "x"; }
    }  // extern "C"
    int tph_after(float x);"""
    want = (C.c_int, types("c_void_p c_int c_void_p c_int64 c_uint64 c_uint32 c_double c_void_p c_void_p".split()))
    assert prototypes(text, "tph_") == {"tph_f": want, "tph_g": (C.c_int64, []), "tph_h": (C.c_char_p, [])}
    got = prototypes(HEADER, "tph_")           # the header's own: pending_dev's comment runs over three lines, tph_adapt over fifteen
    assert [len(got[name][1]) for name in ("tph_propose", "tph_accept", "tph_marginals", "tph_adapt")] == [21, 23, 23, 15]


def test_a_derived_pointer_parameter_takes_byref():
    args = _lib.SIGNATURES["tph_history_ptr"][1]
    assert args == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    args[2].from_param(C.byref(C.c_void_p())), args[3].from_param(C.byref(C.c_int64()))
    for value in (None, 0, 1 << 40, C.create_string_buffer(8), _lib.ALLREDUCE_FN(lambda *a: 0)):
        C.c_void_p.from_param(value)
    with pytest.raises(TypeError):                      # a number that is no address is still refused
        args[3].from_param(1.5)


def test_rng_tags_are_one_number_space():
    tags = {name: value for name, value in vars(device).items() if name.startswith("TAG_")}
    assert sorted(tags.values()) == list(range(1, 12))                 # pairwise distinct, no gap
    assert cluster.TAG_CLUSTER == device.TAG_CLUSTER == 9 and H.REPLICATE_TAGS == (device.TAG_REP_NORMAL, device.TAG_REP_UNIFORM) == (10, 11)
    text = open(os.path.join(ROOT, "tempest_amd", "csrc", "common.h")).read()
    lines = "".join(re.findall(r"^constexpr uint32_t TPH_TAG_[^;]*;", text, re.M))
    library = {name: int(value) for name, value in re.findall(r"TPH_(TAG_\w+) = (\d+)", lines)}
    assert sorted(library.values()) == list(range(1, 8)) and {name: tags[name] for name in library} == library
