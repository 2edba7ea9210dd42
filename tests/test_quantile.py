"""The inverse normal CDF of the fused path on the host: csrc/quantile.h built as a stand-alone program (plain and under the address
and undefined-behaviour sanitizers) against mpmath at 40 digits on a fixed sample; the tracer's NumPy restatement against that
program; special values, odd symmetry, monotonicity across the region edges; the traced ops; tempest_amd.priors.  CPU only."""
import inspect
import math
import shutil

import numpy as np
import pytest
import torch

from tests import quantile_cases as Q

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The program's values over the samples and the special arguments."""
    d = tmp_path_factory.mktemp("quantile")
    exe = Q.build_host(d)
    return {"dir": d, "exe": exe, "ndtri": Q.run_host(exe, Q.sample_p(), d)[0], "erfinv": Q.run_host(exe, Q.sample_y(), d)[1],
            "special_ndtri": Q.run_host(exe, Q.SPECIAL_P, d)[0], "special_erfinv": Q.run_host(exe, Q.SPECIAL_Y, d)[1]}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b, msg=""):
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=msg)


# ------------------------------------------------------------------------------------------------------------ the device functions
def test_the_sample_covers_every_region():
    p, y = Q.sample_p(), Q.sample_y()
    assert 19000 < p.size < 21000 and p.min() == 5e-324 and p.max() == 1.0 - 2.0 ** -53
    q, t = p - 0.5, np.minimum(p, 1.0 - p)
    central, far = np.abs(q) <= 0.425, np.sqrt(-np.log(t)) > 5.0
    assert central.sum() > 8000 and (~central & ~far).sum() > 3000 and far.sum() > 2500
    assert np.abs(y).min() < 1e-290 and np.abs(y).max() < 1.0


def test_host_build_against_mpmath(host):
    for name, got, truth, bound in (("tphu_ndtri", host["ndtri"], Q.truth_ndtri(), Q.NDTRI_HOST_ULP),
                                    ("tphu_erfinv", host["erfinv"], Q.truth_erfinv(), Q.ERFINV_HOST_ULP)):
        assert np.all(np.isfinite(got)), name
        err = Q.ulp_error(got, truth)
        print(f"{name}: largest error {err.max():.3f} ulp, mean {err.mean():.3f} ulp over {err.size} points")
        assert err.max() <= bound, (name, float(err.max()))


def test_finite_and_signed_down_to_the_smallest_subnormal(host):
    p = Q.sample_p()
    assert np.all(np.sign(host["ndtri"]) == np.sign(p - 0.5))
    assert np.all(np.isfinite(host["ndtri"])) and np.all(np.isfinite(host["erfinv"]))
    assert -38.5 < host["ndtri"][p == 5e-324][0] < -38.4 and 8.2 < host["ndtri"][p == 1.0 - 2.0 ** -53][0] < 8.3


def test_sanitized_build_gives_the_same_values(host):
    """-fsanitize=address,undefined on the stand-alone program: a plain executable, nothing preloaded."""
    exe = Q.build_host(host["dir"], "quantile_host_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    same_bits(Q.run_host(exe, Q.sample_p(), host["dir"])[0], host["ndtri"])
    same_bits(Q.run_host(exe, Q.sample_y(), host["dir"])[1], host["erfinv"])
    got = Q.run_host(exe, np.concatenate([Q.SPECIAL_P, Q.SPECIAL_Y]), host["dir"])
    same_bits(np.isnan(got[0][:Q.SPECIAL_P.size]), np.isnan(host["special_ndtri"]))
    same_bits(np.isnan(got[1][Q.SPECIAL_P.size:]), np.isnan(host["special_erfinv"]))


def test_special_values(host):
    inf, nan = np.inf, np.nan
    # SPECIAL_P: 0, 1, 0.5, tiny, -tiny, -0.0, -0.25, 1 + eps, 2, -inf, inf, NaN
    want = np.array([-inf, inf, 0.0, host["special_ndtri"][3], nan, -inf, nan, nan, nan, nan, nan, nan])
    np.testing.assert_array_equal(host["special_ndtri"], want)
    assert bits(host["special_ndtri"][2:3])[0] == 0                                   # exactly +0 at 0.5
    assert -38.5 < host["special_ndtri"][3] < -38.4
    # SPECIAL_Y: -1, 1, 0, -0.0, tiny, -tiny, 1 + eps, -1 - eps, 3, -inf, inf, NaN
    want = np.array([-inf, inf, 0.0, -0.0, 0.0, -0.0, nan, nan, nan, nan, nan, nan])
    np.testing.assert_array_equal(host["special_erfinv"], want)
    np.testing.assert_array_equal(np.signbit(host["special_erfinv"][:6]), [True, False, False, True, False, True])
    # torch's conventions, where torch defines them
    t = torch.special.ndtri(torch.from_numpy(Q.SPECIAL_P)).numpy()
    np.testing.assert_array_equal(np.isnan(t), np.isnan(host["special_ndtri"]))
    np.testing.assert_array_equal(t[:3], host["special_ndtri"][:3])
    t = torch.erfinv(torch.from_numpy(Q.SPECIAL_Y)).numpy()
    np.testing.assert_array_equal(np.isnan(t), np.isnan(host["special_erfinv"]))
    np.testing.assert_array_equal(t[:4], host["special_erfinv"][:4])


def test_a_tiny_argument_of_erfinv_keeps_its_relative_accuracy(host):
    y = Q.sample_y()
    tiny = np.abs(y) < 1e-100
    assert tiny.sum() > 500
    np.testing.assert_allclose(host["erfinv"][tiny], y[tiny] * (math.sqrt(math.pi) / 2.0), rtol=8 * 2.0 ** -53)


def test_odd_symmetry_to_the_bit(host):
    p = Q.sample_p()
    lower = (p <= 0.5) & (1.0 - (1.0 - p) == p)
    assert lower.sum() > 5000
    mirrored = Q.run_host(host["exe"], 1.0 - p[lower], host["dir"])[0]
    half = p[lower] == 0.5                                    # its own mirror image: +0, not -0
    same_bits(mirrored[~half], -host["ndtri"][lower][~half])
    assert half.any() and np.all(bits(mirrored[half]) == 0)
    y = Q.sample_y()
    same_bits(Q.run_host(host["exe"], -y, host["dir"])[1], -host["erfinv"])


def test_monotone_across_the_region_edges(host):
    for run in Q.edge_runs():
        x = Q.run_host(host["exe"], run, host["dir"])[0]
        ulp = np.array([math.ulp(v) for v in x[:-1]])
        drop = (x[:-1] - x[1:]) / ulp
        assert np.all(drop <= Q.NDTRI_HOST_ULP), (run, drop)


def test_the_replay_restates_the_header(host):
    from tempest_amd.trace import _ulps, erfinv_host, ndtri_host
    p, y = Q.sample_p(), Q.sample_y()
    for arg, got, want, central in ((p, ndtri_host(p), host["ndtri"], np.abs(p - 0.5) <= 0.425),
                                    (y, erfinv_host(y), host["erfinv"], np.abs(0.5 * y) <= 0.425)):
        same_bits(got[central], want[central], "central region: exact operations only")
        assert _ulps(got[~central], want[~central]).max() <= 2.0             # the two logs may differ in the last place
    same_bits(np.isnan(ndtri_host(Q.SPECIAL_P)), np.isnan(host["special_ndtri"]))
    np.testing.assert_array_equal(ndtri_host(Q.SPECIAL_P), host["special_ndtri"])
    np.testing.assert_array_equal(erfinv_host(Q.SPECIAL_Y), host["special_erfinv"])
    np.testing.assert_array_equal(np.signbit(erfinv_host(Q.SPECIAL_Y)), np.signbit(host["special_erfinv"]))


# ------------------------------------------------------------------------------------------------------------------- the tracer
def prior_quantiles(u):
    return torch.stack([2.0 * torch.special.ndtri(u[:, 0]) + 1.0, torch.erfinv(2.0 * u[:, 1] - 1.0), torch.special.ndtri(0.5 * u[:, 2] + 0.25),
                        (u[:, 2] - 0.5).erfinv()], dim=1)


def prior_plain(u):
    return 20.0 * u - 10.0


def like_plain(x):
    return -0.5 * (x * x).sum(dim=1)


def test_ndtri_and_erfinv_trace_emit_and_replay():
    from tempest_amd import trace as T
    header = T.quantile_header()
    g = T.trace_function(prior_quantiles, 4, 4, "prior_transform")
    assert sorted(g.nodes[i][0] for i in g.live() if g.nodes[i][0] in ("ndtri", "erfinv")) == ["erfinv", "erfinv", "ndtri", "ndtri"]
    gl = T.trace_function(like_plain, 4, (), "log_likelihood")
    src = T.emit_source({"prior_transform": g, "log_likelihood": gl})
    assert src.startswith(header) and src.count(header) == 1 and src.count("#ifndef TPHU_QUANTILE_H") == 1
    assert src.count("= tphu_ndtri(t") == 2 and src.count("= tphu_erfinv(t") == 2
    # a likelihood that uses them brings the text too, once
    both = T.emit_source({"prior_transform": g, "log_likelihood": T.trace_function(lambda x: torch.erfinv(x[:, 0]), 4, (), "log_likelihood")})
    assert both.count(header) == 1
    # without these ops the emitted source is what it was: no helper text
    plain = T.emit_source({"prior_transform": T.trace_function(prior_plain, 4, 4, "prior_transform"), "log_likelihood": gl})
    assert "TPHU_QUANTILE_H" not in plain and "tphu_ndtri" not in plain and plain.startswith("// emitted by tempest_amd.trace_callbacks")
    # the replay against eager torch on the CPU, by the probe's rule
    u = T.probe_batch(4)
    eager = prior_quantiles(torch.from_numpy(u)).numpy()
    mx, ulps, same, ok = T.compare(eager, T.replay(g, u))
    print(f"replay against eager torch: {mx:.3g} absolute, {ulps:.3g} ulp")
    assert same and ok
    # the method of a traced value that a tensor does not have: the same node
    gm = T.trace_function(lambda u: torch.stack([u[:, 0].ndtri(), torch.special.erfinv(u[:, 1])], dim=1), 2, 2, "prior_transform")
    assert sorted(gm.nodes[i][0] for i in gm.live() if gm.nodes[i][0] != "in") == ["erfinv", "ndtri"]
    # the replay IS the restatement
    np.testing.assert_array_equal(T.replay(g, u)[:, 1], T.erfinv_host(2.0 * u[:, 1] - 1.0))
    np.testing.assert_array_equal(T.replay(g, u)[:, 0], 2.0 * T.ndtri_host(u[:, 0]) + 1.0)


def test_trace_callbacks_hands_the_helper_text_to_the_compiler(monkeypatch):
    import tempest_amd as tp
    from tempest_amd import hipcallbacks as H
    from tempest_amd import trace as T

    class Captured(Exception):
        pass

    def capture(source, *a, **k):
        raise Captured(source)
    monkeypatch.setattr(H, "build_plugin", capture)
    with pytest.raises(Captured) as e:
        tp.trace_callbacks(prior_quantiles, like_plain, 4)
    assert e.value.args[0].count(T.quantile_header()) == 1
    with pytest.raises(Captured) as e:
        tp.trace_callbacks(prior_plain, like_plain, 4)
    assert "TPHU_QUANTILE_H" not in e.value.args[0]


@pytest.mark.parametrize("name, fn, instead", [
    ("ndtr", lambda x: torch.special.ndtr(x[:, 0]), "erfc"),
    ("log_ndtr", lambda x: torch.special.log_ndtr(x[:, 0]), "erfc"),
    ("erfcinv", lambda x: x[:, 0].erfcinv(), "ndtri"),
    ("distributions", lambda x: torch.distributions.Normal(0.0, 1.0, validate_args=False).icdf(x[:, 0]), "tempest_amd.priors.Normal"),
])
def test_the_neighbouring_functions_stay_refused(name, fn, instead):
    from tempest_amd import trace as T
    with pytest.raises(T.TraceError) as e:
        T.trace_function(fn, 2, (), "log_likelihood")
    assert "instead:" in str(e.value) and instead in str(e.value).split("instead:")[1]


# --------------------------------------------------------------------------------------------------------------- tempest_amd.priors
def seven():
    import tempest_amd as tp
    P = tp.priors
    return tp.Prior([P.Uniform(-5, 5), P.Normal(0.0, 2.0), P.LogNormal(0.0, 0.5), P.HalfNormal(1.0),
                     P.TruncatedNormal(0.0, 1.0, lo=-1.0, hi=3.0), P.LogUniform(1e-3, 1e2), P.Exponential(2.0)])


def scipy_laws():
    """(tempest_amd.priors distribution, the frozen scipy.stats law) pairs: the seven columns, and truncated normals on either side
    of the mean, one of them three standard deviations above it (the mirrored form).  The added ones are wide enough that their
    log density stays away from zero, where an error relative to it says nothing."""
    import scipy.stats as st
    import tempest_amd as tp
    P = tp.priors
    return [(P.Uniform(-5, 5), st.uniform(-5, 10)), (P.Normal(0.0, 2.0), st.norm(0.0, 2.0)), (P.LogNormal(0.0, 0.5), st.lognorm(0.5, scale=1.0)),
            (P.HalfNormal(1.0), st.halfnorm(scale=1.0)), (P.TruncatedNormal(0.0, 1.0, lo=-1.0, hi=3.0), st.truncnorm(-1.0, 3.0)),
            (P.LogUniform(1e-3, 1e2), st.loguniform(1e-3, 1e2)), (P.Exponential(2.0), st.expon(scale=0.5)),
            (P.TruncatedNormal(1.5, 10.0, lo=31.5, hi=54.0), st.truncnorm(3.0, 5.25, loc=1.5, scale=10.0)),
            (P.TruncatedNormal(1.5, 10.0, lo=-51.0, hi=-21.0), st.truncnorm(-5.25, -2.25, loc=1.5, scale=10.0)),
            (P.TruncatedNormal(-1.0, 5.0, lo=1.5), st.truncnorm(0.5, np.inf, loc=-1.0, scale=5.0)),
            (P.TruncatedNormal(-1.0, 0.5, hi=0.0), st.truncnorm(-np.inf, 2.0, loc=-1.0, scale=0.5))]


def test_exports():
    import tempest_amd as tp
    from tempest_amd import priors
    from tempest_amd.trace import quantile_header
    assert tp.priors is priors and tp.Prior is priors.Prior and "Prior" in tp.__all__ and "priors" in tp.__all__
    assert priors.DEVICE_HELPERS == quantile_header() and priors.DEVICE_HELPERS.startswith("#pragma clang fp contract(off)\n")
    assert seven().n_dim == 7


@pytest.mark.parametrize("make", [
    lambda P: P.Uniform(1.0, 1.0), lambda P: P.Uniform(2.0, 1.0), lambda P: P.Uniform(0.0, math.inf), lambda P: P.Uniform(math.nan, 1.0),
    lambda P: P.LogUniform(0.0, 1.0), lambda P: P.LogUniform(-1.0, 1.0), lambda P: P.LogUniform(2.0, 1.0), lambda P: P.LogUniform(1.0, 1.0),
    lambda P: P.Normal(0.0, 0.0), lambda P: P.Normal(0.0, -1.0), lambda P: P.Normal(math.inf, 1.0), lambda P: P.Normal("0", 1.0),
    lambda P: P.LogNormal(0.0, 0.0), lambda P: P.LogNormal(0.0, -2.0), lambda P: P.HalfNormal(0.0), lambda P: P.HalfNormal(-1.0),
    lambda P: P.Exponential(0.0), lambda P: P.Exponential(-1.0),
    lambda P: P.TruncatedNormal(0.0, 0.0, lo=-1.0, hi=1.0), lambda P: P.TruncatedNormal(0.0, 1.0, lo=1.0, hi=1.0),
    lambda P: P.TruncatedNormal(0.0, 1.0, lo=2.0, hi=1.0), lambda P: P.TruncatedNormal(0.0, 1.0, lo=40.0, hi=41.0),
    lambda P: P.TruncatedNormal(0.0, 1.0, lo=-41.0, hi=-40.0), lambda P: P.Prior([]), lambda P: P.Prior([P.Uniform(0, 1), "Normal"]),
])
def test_bad_parameters_are_refused_at_construction(make):
    import tempest_amd as tp
    with pytest.raises(ValueError):
        make(tp.priors)


def test_pushforward_is_the_law():
    """The CDF of transform(u) is u: eager torch on the CPU, and the replay of the trace (what the device computes)."""
    import tempest_amd as tp
    from tempest_amd import trace as T
    laws = scipy_laws()
    prior = tp.Prior([d for d, _ in laws])
    u = np.random.RandomState(7).uniform(size=(4000, prior.n_dim))
    g = T.trace_function(prior.transform, prior.n_dim, prior.n_dim, "prior_transform")
    for how, x in (("eager", prior.transform(u)), ("replay", T.replay(g, u))):
        assert isinstance(x, np.ndarray) and x.shape == u.shape
        for j, (d, law) in enumerate(laws):
            err = np.abs(law.cdf(x[:, j]) - u[:, j]).max()
            assert err <= 1e-12, (how, d, err)
    mirrored = laws[7][0]
    assert mirrored._mirrored and not laws[8][0]._mirrored
    x = prior.transform(u)[:, 7]
    assert 31.5 <= x.min() and x.max() <= 54.0 and np.all(np.diff(x[np.argsort(u[:, 7])]) >= 0.0)


def test_log_prob_against_scipy():
    import tempest_amd as tp
    laws = scipy_laws()
    u = np.random.RandomState(8).uniform(size=(2000, len(laws)))
    x = tp.Prior([d for d, _ in laws]).transform(u)
    for j, (d, law) in enumerate(laws):
        np.testing.assert_allclose(tp.Prior([d]).log_prob(x[:, j:j + 1]), law.logpdf(x[:, j]), rtol=1e-12, atol=0.0, err_msg=repr(d))
    prior = seven()
    x7 = x[:, :7]
    np.testing.assert_allclose(prior.log_prob(x7), sum(law.logpdf(x7[:, j]) for j, (_, law) in enumerate(laws[:7])), rtol=1e-12)
    # outside the support: -inf
    out = np.array([[6.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0], [0.0, 0.0, -1.0, 1.0, 0.0, 1.0, 1.0], [0.0, 0.0, 1.0, -1.0, 0.0, 1.0, 1.0],
                    [0.0, 0.0, 1.0, 1.0, 3.5, 1.0, 1.0], [0.0, 0.0, 1.0, 1.0, 0.0, 1e3, 1.0], [0.0, 0.0, 1.0, 1.0, 0.0, 1.0, -0.5]])
    assert np.all(prior.log_prob(out) == -np.inf) and np.isfinite(prior.log_prob(np.array([0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0])))


def test_container_kinds():
    prior = seven()
    u = np.random.RandomState(9).uniform(size=(5, 7))
    xn, xt = prior.transform(u), prior.transform(torch.from_numpy(u))
    assert isinstance(xn, np.ndarray) and isinstance(xt, torch.Tensor) and xt.dtype == torch.float64
    np.testing.assert_array_equal(xn, xt.numpy())
    ln, lt = prior.log_prob(xn), prior.log_prob(xt)
    assert isinstance(ln, np.ndarray) and ln.shape == (5,) and isinstance(lt, torch.Tensor) and lt.shape == (5,)
    np.testing.assert_array_equal(ln, lt.numpy())
    assert prior.transform(u[0]).shape == (7,) and np.array_equal(prior.transform(u[0]), xn[0])
    with pytest.raises(ValueError):
        prior.transform(u[:, :6])


def test_the_ends_of_the_unit_interval():
    """u = 0 or 1 under a column of unbounded support is an infinite parameter, as the quantile function says."""
    x = seven().transform(np.array([[0.5, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0]]))
    assert x[0, 0] == 0.0 and x[0, 1] == -np.inf and x[0, 2] == np.inf and x[0, 3] == 0.0 and x[0, 6] == 0.0
    assert x[0, 4] == pytest.approx(-1.0, abs=1e-15) and x[0, 4] >= -1.0 and x[0, 5] == pytest.approx(1e2, rel=1e-14)
    assert x[1, 0] == -5.0 and x[1, 1] == np.inf and x[1, 2] == 0.0 and x[1, 3] == np.inf and x[1, 6] == np.inf
    assert x[1, 4] == pytest.approx(3.0, abs=1e-13) and x[1, 4] <= 3.0 and x[1, 5] == pytest.approx(1e-3, rel=1e-14)


def test_hip_source_passes_the_constructor_checks(monkeypatch):
    """hip_source() + a hand-written likelihood reaches build_plugin as a plain plugin of x alone."""
    import tempest_amd as tp
    from tempest_amd import hipcallbacks as H
    from tempest_amd import trace as T
    like = "__device__ double log_likelihood(const double* x) { return -x[0] * x[0]; }\n"
    prior = seven()
    src = prior.hip_source()
    assert src.count("void prior_transform(") == 1 and src.count(tp.priors.DEVICE_HELPERS) == 1 and src.startswith(tp.priors.DEVICE_HELPERS)
    assert src.count("tphu_ndtri(t") == 4 and "log_likelihood" not in src
    # the statements are the ones trace_callbacks emits for the same function
    g = T.trace_function(prior.transform, 7, 7, "prior_transform")
    traced = T.emit_source({"prior_transform": g, "log_likelihood": T.trace_function(like_plain, 7, (), "log_likelihood")})
    body = src[len(tp.priors.DEVICE_HELPERS):]
    assert body in traced
    # a prior without the Gaussian family needs no helper text
    assert "TPHU_QUANTILE_H" not in tp.Prior([tp.priors.Uniform(0, 1), tp.priors.Exponential(1.0)]).hip_source()
    signature = inspect.signature(H.build_plugin)

    class Captured(Exception):
        pass

    def capture(*a, **k):
        raise Captured(signature.bind(*a, **k))
    monkeypatch.setattr(H, "build_plugin", capture)
    with pytest.raises(Captured) as e:
        tp.HipCallbacks(src + like, prior.n_dim)
    bound = e.value.args[0]
    bound.apply_defaults()
    assert bound.arguments == dict(source=src + like, n_dim=7, verbose=False, tables=None, term=False, n_derived=0, predict=False,
                                   pointwise=False, replicate=False, discrepancy=False)
    assert H._Parts.of(src + like).traced            # the clamp of the truncated normal calls the traced helpers
