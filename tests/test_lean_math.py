"""The host side of the lean-math and Philox tests (tests/test_lean_math_gpu.py is the device side): the two host transcriptions of
Philox4x32-10 against Random123's published vectors and against each other, how far the oracle's own normals and Gamma candidates are
from the truth, and that the probe plugins of tests/lean_math_cases.py compile."""
import os
import shutil

import numpy as np
import pytest

from oracle import philox as px
from tempest_amd import _philox_host as ph
from tests import lean_math_cases as L


# ------------------------------------------------------------------------------------------------------------- known-answer vectors
@pytest.mark.parametrize("counter, key, want", L.KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    got = px.philox4x32(*counter, *key)
    assert tuple(int(np.asarray(w).reshape(-1)[0]) for w in got) == want, "oracle/philox.py"
    assert tuple(int(w) for w in ph.philox4x32(*counter, *key)) == want, "tempest_amd/_philox_host.py"
    vec = ph.philox4x32(*(np.array([c, c], dtype=np.uint64) for c in counter), *key)
    assert all(int(w[0]) == int(w[1]) == v for w, v in zip(vec, want)), "tempest_amd/_philox_host.py over arrays"


# -------------------------------------------------------------------------------------------------------- host twin against oracle
def test_host_twin_equals_oracle_bit_for_bit():
    c = L.corner_counters()
    assert c.item.size == 3 + 560 + 4096
    for name in ("uniform_pair", "normal_pair"):
        want = L.by_seed(c, getattr(px, name), 2)
        got = L.by_seed(c, getattr(ph, name), 2)
        for k in range(2):
            np.testing.assert_array_equal(L.bits(got[k]), L.bits(want[k]), err_msg=f"{name}[{k}]")
    want = L.by_seed(c, px.uniform_pair, 2)[0]
    got = np.array([ph.uniform_scalar(int(s), int(t), int(g), int(i), int(d)) for i, d, t, g, s in zip(*c)])
    np.testing.assert_array_equal(L.bits(got), L.bits(want), err_msg="uniform_scalar")
    # item 2^32 is item 0 in both, and the uniforms are k 2^-53 with k < 2^53
    first = L.by_seed(c, px.uniform_pair, 2)
    per_item = 560 // len(L.CORNER_ITEMS)                 # the corners are item-major behind the three known-answer vectors
    lo, hi = 3 + L.CORNER_ITEMS.index(0) * per_item, 3 + L.CORNER_ITEMS.index(2 ** 32) * per_item
    assert np.all(c.item[lo:lo + per_item] == 0) and np.all(c.item[hi:hi + per_item] == 2 ** 32)
    for u in first:
        np.testing.assert_array_equal(u[lo:lo + per_item], u[hi:hi + per_item])
    assert all(np.all((u >= 0.0) & (u < 1.0) & (u * 2.0 ** 53 == np.floor(u * 2.0 ** 53))) for u in first)


# ------------------------------------------------------------------------------------------------------------------ oracle accuracy
def test_oracle_normals_and_candidates_against_mpmath():
    """oracle/philox.py forms its normals with np.log, np.sqrt and np.cos / np.sin of the ROUNDED angle 2 pi u2: every value must lie
    within L.bound_oracle_normal (derived there) of the truth, and its log of the acceptance uniform within one ulp.  The kernels'
    parity tests allow rtol = 1e-11 against this oracle; printed: how much of that the oracle itself uses."""
    c, t = L.normal_counters(), L.truth_normals()
    assert c.item.size == 20000 + 11 * 32
    z0, z1 = L.by_seed(c, px.normal_pair, 2)
    u2 = L.by_seed(c, px.uniform_pair, 2)[1]
    x, logu = L.by_seed(c, lambda s, i, d, tk, g: px.gamma_candidate(s, i, d, tk, g), 2)
    turn32 = L.oracle_words(c)[2].astype(np.float64) * 2.0 ** -32
    for name, got, truth, turn in (("normal_pair[0]", z0, t.z0, u2), ("normal_pair[1]", z1, t.z1, u2),
                                   ("gamma_candidate x", x, t.x, turn32)):
        err, bound = L.abs_error(got, truth), L.bound_oracle_normal(t.rad, turn)
        worst = int(np.argmax(err / np.maximum(bound, 1e-300)))
        rel = err / np.maximum(np.abs(truth.near), 1e-300)
        print(f"{name}: largest error / bound {float(err[worst] / bound[worst]):.3f} (error {err[worst]:.3e} at radius {t.rad[worst]:.4g}); "
              f"largest relative error {rel.max():.3e} (next to a zero of the cosine or sine), median {np.median(rel):.3e}, "
              "beside the parity tests' rtol of 1e-11")
        assert np.all(err <= bound), (name, worst, float(err[worst]), float(bound[worst]))
    err = L.ulp_error(logu, t.logu)
    print(f"gamma_candidate logu: largest error {err.max():.3f} ulp")
    assert err.max() <= 1.0


# -------------------------------------------------------------------------------------------------------------- the probes compile
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
@pytest.mark.parametrize("name", sorted(L.PROBES))
def test_probe_sources_compile(name):
    from tempest_amd.hipcallbacks import MAX_DERIVED, build_plugin
    source, n_dim, n_derived = L.PROBES[name]
    assert len(L.PROBES) <= 3 and n_derived <= MAX_DERIVED
    path = build_plugin(source, n_dim, n_derived=n_derived)
    assert path.exists() and path.stat().st_size > 0
