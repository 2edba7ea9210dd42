"""Pareto-smoothed importance-sampling LOO on the device (HipCallbacks(pointwise="psis").psis_loo, Sampler.pointwise(); DESIGN.md
section 11) against the NumPy oracle of tests/psis_cases.py (checked on the CPU by tests/test_psis.py).

The term of psis_cases.SOURCE is a table lookup, so the device and the oracle see the same a_ir to the bit and differ only through
the device's libm and the order of its sums: every finite output within psis_cases.PSIS_RTOL x max(1, |value|) -- 8 x the figure the
perturbed oracle gave --, every special value, pareto_k = +inf (nothing smoothed) and tail_len exactly.  Values at both sides of a
wave, the 256-lane sweep, the 64 x 16 row block and the powers of two of the sort; ties as a systematic resample makes them; NaN and
infinite terms; every tile and several batches to the bit; the tail clamp; the traced route; Sampler.pointwise()."""
import os
import shutil

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import psis_cases as pc  # noqa: E402

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")]


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def tp():
    """The package, with the one plugin of psis_cases.SOURCE compiled (every object below finds it in the cache)."""
    need_gpu()
    import tempest_amd
    tempest_amd.HipCallbacks(pc.SOURCE, pc.N_DIM, data={"A": np.zeros((1, 1))}, n_terms=1, pointwise="psis")
    return tempest_amd


def device_psis(tp, A, tile=0, cap=0):
    cb = tp.HipCallbacks(pc.SOURCE, pc.N_DIM, data={"A": A}, n_terms=A.shape[0], pointwise="psis")
    cb.pointwise_tile, cb.psis_scratch_cap = tile, cap
    return cb.psis_loo(pc.rows(A.shape[1]))


def check(got, A, name):
    S = A.shape[1]
    want = pc.psis_oracle(A)
    assert got["tail_len"] == pc.tail_len(S) and got["n_rows"] == S and got["k_threshold"] == pc.k_threshold(S)
    for k in pc.KEYS:
        assert got[k].shape == (A.shape[0],) and got[k].dtype == np.float64
        print(f"{name} {k}: {pc.close(got[k], want[k], k) / pc.PSIS_RTOL[k]:.3f} of the bound")
    return want


def same_bits(a, b, msg=""):
    for k in pc.KEYS:
        np.testing.assert_array_equal(a[k].view(np.int64), b[k].view(np.int64), err_msg=f"{msg} {k}")
    assert a["totals"].keys() == b["totals"].keys()
    for k in a["totals"]:
        np.testing.assert_array_equal(a["totals"][k], b["totals"][k], err_msg=f"{msg} totals {k}")


@pytest.mark.parametrize("S", pc.GAUSS_SIZES)
def test_values_against_the_oracle(tp, S):
    for T in pc.GAUSS_TERMS:
        A = pc.gauss_case(S, T)
        got = device_psis(tp, A)
        want = check(got, A, f"S={S} T={T}")
        assert np.all(np.isinf(want["pareto_k"])) == (S <= 20)          # a tail below 5 is not smoothed; every other one here is
        hk = int(np.sum(~(want["pareto_k"] <= pc.k_threshold(S))))
        assert got["totals"]["n_high_k"] == hk
        assert got["totals"]["elpd_psis_se"] == float(np.sqrt(T * np.var(got["elpd_psis"])))
    if S == 4096:                                                        # s_r from 0.3 to 2.5: k-hat from about 0.1 to about 5
        assert want["pareto_k"][0] < 0.3 and want["pareto_k"][-1] > 3.0


def test_ties(tp):
    for name, A in pc.tie_cases().items():
        want = check(device_psis(tp, A), A, name)
        assert np.all(np.isfinite(want["pareto_k"])) if name == "runs_of_8" else np.all(want["pareto_k"] == np.inf), name


def test_special_values(tp):
    A = pc.special_case()
    got = device_psis(tp, A)
    check(got, A, "special")
    nan, inf = np.array(np.nan).view(np.int64), np.array(np.inf).view(np.int64)
    for k in pc.KEYS:
        assert got[k][1].view(np.int64) == nan, k                                   # a NaN term: all three NaN
    for col, sign in ((2, -1.0), (4, 1.0)):                                         # min a = -inf; every a = +inf
        assert got["elpd_psis"][col] == sign * np.inf
        assert got["pareto_k"][col].view(np.int64) == nan and got["ess_psis"][col].view(np.int64) == nan
    assert all(np.isfinite(got[k][3]) for k in pc.KEYS)                             # a single +inf row carries ratio 0
    assert got["pareto_k"][0].view(np.int64) != inf
    assert got["totals"]["n_high_k"] >= 3 and np.isnan(got["totals"]["elpd_psis_se"])


def test_no_tile_and_no_batch_changes_a_bit(tp):
    from tempest_amd import hipcallbacks as H
    S, T = 1025, 65
    A = pc.gauss_case(S, T, seed=2)
    A[3, 100] = np.nan
    A[9, 7] = -np.inf
    ref = device_psis(tp, A)
    check(ref, A, "launch shape")
    for tile in (1, 8, 64):
        same_bits(device_psis(tp, A, tile=tile), ref, f"tile {tile}")
    per_r = 3 * 2 + 264 + pc.tail_len(S)
    assert H.psis_scratch_words(S, T) == 1 + 2 + per_r * T
    for batch in (1, 7, 64):
        same_bits(device_psis(tp, A, tile=8, cap=1 + 2 + per_r * batch + 5), ref, f"batches of {batch}")
    with pytest.raises(H.TempestHipError, match="scratch too small"):
        device_psis(tp, A, cap=per_r)


def test_the_tail_clamp(tp):
    A = pc.clamp_case()
    S = A.shape[1]
    assert int(np.ceil(3.0 * np.sqrt(S))) > pc.MAX_TAIL == pc.tail_len(S)
    got = device_psis(tp, A)
    assert got["tail_len"] == pc.MAX_TAIL
    check(got, A, "clamp")
    assert np.all(np.isfinite(got["pareto_k"]))


def test_the_traced_route_gives_the_bits_of_the_hand_written_source(tp):
    from tests.test_hipcallbacks_data import particles, reg_data
    from tests.test_hipcallbacks_predict import QUAD
    from tests.test_trace_data import prior, quad_term
    D = {k: v for k, v in reg_data(50).items() if k != "c"}
    traced = tp.trace_callbacks(prior, quad_term, 3, data=D, n_terms="t", pointwise="psis")
    hand = tp.HipCallbacks(QUAD, 3, data=D, n_terms="t", pointwise="psis")
    assert traced.path != hand.path and traced.psis_enabled
    x = torch.from_numpy(particles(1000, seed=3) * 0.2 + np.array([0.7, 1.9, -1.1])).cuda()
    a, b = traced.psis_loo(x), hand.psis_loo(x)
    same_bits(a, b, "traced")
    assert a["tail_len"] == b["tail_len"] == 95 and a["pareto_k"].shape == (50,) and np.all(np.isfinite(a["elpd_psis"]))
    w = torch.ones(1000, dtype=torch.float64, device="cuda")
    pa, pb = traced.pointwise(x, w), hand.pointwise(x, w)                           # pointwise() itself: the six keys of before
    assert set(pa) == {"lppd", "mean", "p_waic", "elpd_waic", "elpd_loo", "ess_loo", "n_rows", "ess", "totals"}
    for k in ("lppd", "elpd_loo", "ess_loo"):
        np.testing.assert_array_equal(pa[k], pb[k])


def test_sampler_pointwise_adds_the_smoothed_values(tp):
    from tests.test_hipcallbacks_predict import QUAD, quad_data
    cb = tp.HipCallbacks(QUAD, 3, data=quad_data(), n_terms="t", pointwise="psis")
    s = tp.Sampler(cb.prior_transform, cb.log_likelihood, 3, n_particles=128, vectorize=True, clustering=False, random_state=11)
    s.run(n_total=512, progress=False)
    pw = s.pointwise()
    x, w, _ = s.posterior()
    plain = cb.pointwise(x, w)
    assert set(pw) == set(plain) | set(pc.KEYS)
    assert set(pw["totals"]) == set(plain["totals"]) | {"elpd_psis", "elpd_psis_se", "p_psis", "n_high_k", "k_threshold"}
    for k in plain:                                                                  # what pointwise() gave before is untouched
        if k != "totals":
            np.testing.assert_array_equal(pw[k], plain[k])
    assert all(pw["totals"][k] == v for k, v in plain["totals"].items())
    rows = s._core._psis_rows
    assert rows.is_cuda and tuple(rows.shape) == (len(x), 3)
    assert set(map(tuple, rows.cpu().numpy())) <= set(map(tuple, x))                # drawn from the weighted rows
    direct = cb.psis_loo(rows)
    for k in pc.KEYS:
        np.testing.assert_array_equal(pw[k].view(np.int64), direct[k].view(np.int64))
        assert pw[k].shape == (200,)
    assert pw["totals"]["elpd_psis"] == direct["totals"]["elpd_psis"] and pw["totals"]["n_high_k"] == direct["totals"]["n_high_k"]
    assert pw["totals"]["p_psis"] == pw["totals"]["lppd"] - pw["totals"]["elpd_psis"]
    assert pw["totals"]["k_threshold"] == pc.k_threshold(len(x))
    again = s.pointwise()
    for k in pc.KEYS:
        np.testing.assert_array_equal(pw[k].view(np.int64), again[k].view(np.int64))
    other = s.pointwise(psis_draws=300, seed=5)
    assert tuple(s._core._psis_rows.shape) == (300, 3) and other["totals"]["k_threshold"] == pc.k_threshold(300)
    same = s.pointwise(psis_draws=300, seed=5)
    for k in pc.KEYS:
        np.testing.assert_array_equal(other[k].view(np.int64), same[k].view(np.int64))
    d = tp.compare_pointwise(pw, other, key="elpd_psis")
    assert d["n"] == 200 and np.isfinite(d["diff"]) and d["se"] >= 0.0
    with pytest.raises(ValueError, match="psis_draws must be a positive int"):
        s.pointwise(psis_draws=0)
