"""HipCallbacks with observed data (tempest_amd/hipcallbacks.py): data tables handed to every kernel as a
kernel argument, and likelihoods given per observation (log_likelihood_term) whose sum the library owns -- one order of additions,
two evaluations (lane per particle, split over the data) that agree bit for bit.

CPU: the generated plugins compile for gfx950, the cache key holds names and ranks but no values, a data-less source generates
the text it always did, and every validation error.  GPU: the sum against a NumPy restatement to the bit, lane == split, two
objects on one plugin, update_data under a captured graph, the fused Metropolis kernel against tph_accept, whole runs, and the
evidence of a regression target against its closed form."""
import ctypes
import hashlib
import shutil

import numpy as np
import pytest

torch = pytest.importorskip("torch")

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not __import__("os").path.exists("/opt/rocm/bin/hipcc"),
                                 reason="hipcc not available")

PRIOR = '''
__device__ void prior_transform(const double* u, double* x, const tphu_data& D) {
#pragma unroll
  for (int j = 0; j < N_DIM; ++j) x[j] = 10.0 * u[j] - 5.0;
}
'''
# quadratic regression with known noise; c = log s + 0.5 log 2 pi is a table, so the term uses + - * / only
REG = PRIOR + '''
__device__ double log_likelihood_term(const double* x, int64_t r, const tphu_data& D) {
  const double m = x[0] + x[1] * D.t[r] + x[2] * D.t[r] * D.t[r];
  const double z = (D.y[r] - m) / D.s[r];
  return -0.5 * z * z - D.c[r];
}
'''
# Poisson counts k with rate exp(x0 + x1 t) + b, b = x2 + 6 > 0 inside the prior box: a term with exp and log
POIS = PRIOR + '''
__device__ double log_likelihood_term(const double* x, int64_t r, const tphu_data& D) {
  const double lam = exp(0.1 * x[0] + 0.1 * x[1] * D.t[r]) + (x[2] + 6.0);
  return D.k[r] * log(lam) - lam - D.c[r];
}
'''
# the same regression with the sum written by the user: data tables without the term form (and a 2-D entry)
WHOLE = PRIOR + '''
__device__ double log_likelihood(const double* x, const tphu_data& D) {
  double s = 0.0;
  for (int64_t r = 0; r < D.obs_rows; ++r) {
    const double t = D.obs[r * D.obs_cols], y = D.obs[r * D.obs_cols + 1], sg = D.obs[r * D.obs_cols + 2];
    const double z = (y - (x[0] + x[1] * t + x[2] * t * t)) / sg;
    s += -0.5 * z * z;
  }
  return s;
}
'''
# tests/test_hipcallbacks.py's SRC and the SHA-256 of the translation unit the parent of this feature generated for it
OLD_SRC = '''
__device__ void prior_transform(const double* u, double* x) {
#pragma unroll
  for (int j = 0; j < N_DIM; ++j) x[j] = 20.0 * u[j] - 10.0;
}
__device__ double log_likelihood(const double* x) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < N_DIM; j += 2) {
    double a = x[j] * x[j] - x[j + 1], b = x[j] - 1.0;
    s += 10.0 * a * a + b * b;
  }
  return -s;
}
'''
OLD_TEXT_SHA256 = "85422a8c6c6b7f15300384fe0cff150dc7d93d0c9030862000df9219ef6bc467"

N_TERMS = (1, 255, 256, 257, 16_384, 16_385, 100_000)
N_PARTICLES = (1, 63, 700, 3001)


def reg_data(n_terms, seed=7):
    rng = np.random.RandomState(seed)
    t = np.linspace(-1, 1, n_terms) if n_terms > 1 else np.array([0.3])
    s = 0.5 + 0.5 * rng.rand(n_terms)
    y = 0.7 + 1.9 * t - 1.1 * t * t + s * rng.randn(n_terms)
    return {"t": t, "y": y, "s": s, "c": np.log(s) + 0.5 * np.log(2.0 * np.pi)}


def pois_data(n_terms, seed=11):
    from math import lgamma
    rng = np.random.RandomState(seed)
    t = np.linspace(-1, 1, n_terms) if n_terms > 1 else np.array([0.3])
    k = rng.poisson(np.exp(0.1 + 0.05 * t) + 5.0).astype(np.float64)
    return {"t": t, "k": k, "c": np.array([lgamma(v + 1.0) for v in k])}


def reg_terms(x, D):
    """The terms of REG for particles x (m, 3): elementwise, operation by operation in the order of the C expression."""
    x0, x1, x2 = x[:, 0:1], x[:, 1:2], x[:, 2:3]
    t, y, s, c = D["t"][None, :], D["y"][None, :], D["s"][None, :], D["c"][None, :]
    m = (x0 + x1 * t) + (x2 * t) * t
    z = (y - m) / s
    return (-0.5 * z) * z - c


def pois_terms(x, D, ft):
    x = x.astype(ft)
    x0, x1, x2 = x[:, 0:1], x[:, 1:2], x[:, 2:3]
    t, k, c = D["t"].astype(ft)[None, :], D["k"].astype(ft)[None, :], D["c"].astype(ft)[None, :]
    lam = np.exp((ft(0.1) * x0) + ((ft(0.1) * x1) * t)) + (x2 + ft(6.0))
    return (k * np.log(lam) - lam) - c


def seq_sum_last(a):
    """Sum along the last axis, sequentially from +0.0 (np.cumsum adds in order)."""
    z = np.zeros(a.shape[:-1] + (1,), dtype=a.dtype)
    return np.cumsum(np.concatenate([z, a], axis=-1), axis=-1)[..., -1]


def layered_sum(terms, chunk, block):
    """The contract of DESIGN.md section 11: chunks of `chunk` consecutive terms added in order, blocks of `block` consecutive chunk
    sums added in order, the block sums added in order; every level starts from +0.0.  (Padding with +0.0 changes no bit: a
    running sum that started from +0.0 is never -0.0.)"""
    m, nt = terms.shape
    nch = -(-nt // chunk)
    pad = np.zeros((m, nch * chunk), dtype=terms.dtype)
    pad[:, :nt] = terms
    cs = seq_sum_last(pad.reshape(m, nch, chunk))
    nb = -(-nch // block)
    pad = np.zeros((m, nb * block), dtype=terms.dtype)
    pad[:, :nch] = cs
    return seq_sum_last(seq_sum_last(pad.reshape(m, nb, block)))


def reference_loglike(x, D, terms_fn, layout, batch=128):
    out = np.empty(len(x), dtype=terms_fn(x[:1], D).dtype)
    for i in range(0, len(x), batch):
        out[i:i + batch] = layered_sum(terms_fn(x[i:i + batch], D), *layout)
    return out


def particles(n, seed=1):
    return np.random.RandomState(seed).uniform(-5.0, 5.0, size=(n, 3))


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------------- CPU
@needs_hipcc
def test_data_plugins_build_and_export_abi():
    from tempest_amd.hipcallbacks import build_plugin
    tabs = (("t", 1), ("y", 1), ("s", 1), ("c", 1))
    for path in (build_plugin(REG, 3, tables=tabs, term=True), build_plugin(WHOLE, 3, tables=(("obs", 2),))):
        lib = ctypes.CDLL(str(path))
        for sym in ("tphu_last_error", "tphu_n_dim", "tphu_abi", "tphu_prior", "tphu_like", "tphu_accept", "tphu_step", "tphu_run",
                    "tphu_data_abi"):
            assert hasattr(lib, sym), sym
        assert lib.tphu_n_dim() == 3 and lib.tphu_abi() == 3 and lib.tphu_data_abi() == 1
    term = ctypes.CDLL(str(build_plugin(REG, 3, tables=tabs, term=True)))
    assert hasattr(term, "tphu_like_split") and (term.tphu_sum_chunk(), term.tphu_sum_block()) == (256, 64)


@needs_hipcc
def test_cache_key_holds_names_and_ranks_not_values():
    import tempest_amd as tp
    a = tp.HipCallbacks(REG, 3, data=reg_data(100), n_terms="t")
    b = tp.HipCallbacks(REG, 3, data=reg_data(777, seed=3), n_terms=777)
    assert a.path == b.path and a.sum_layout == b.sum_layout == (256, 64)
    d = reg_data(100)
    d["extra"] = np.ones(3)
    assert tp.HipCallbacks(REG, 3, data=d, n_terms="t").path != a.path                     # another name
    d = reg_data(100)
    d["w"] = np.ones(4)
    e = tp.HipCallbacks(REG, 3, data=d, n_terms="t")
    d["w"] = np.ones((2, 2))
    assert tp.HipCallbacks(REG, 3, data=d, n_terms="t").path != e.path                     # another rank, same names


def test_dataless_source_generates_the_text_it_always_did():
    from tempest_amd.hipcallbacks import plugin_source
    text = plugin_source(OLD_SRC)
    assert hashlib.sha256(text.encode()).hexdigest() == OLD_TEXT_SHA256
    assert "tphu_data" not in text and "@" not in text.replace(OLD_SRC, "")
    with_data = plugin_source(WHOLE, (("obs", 2),))
    assert "int64_t obs_rows, obs_cols;" in with_data and "tphu_data_abi" in with_data and "k_user_like_split" not in with_data
    assert "k_user_like_split" in plugin_source(REG, (("t", 1),), True)


@pytest.mark.parametrize("data,match", [
    ({"t": np.ones((2, 2, 2))}, "1-D or 2-D"),
    ({"t": np.array(["a", "b"])}, "real numbers"),
    ({"t": np.ones(3) + 1j}, "real numbers"),
    ({"t": np.ones(0)}, "empty"),
    ({"2t": np.ones(3)}, "C identifier"),
    ({"double": np.ones(3)}, "C identifier"),
    ({"a b": np.ones(3)}, "C identifier"),
    ({"n_terms": np.ones(3)}, "collides"),
    ({"t": np.ones(3), "t_len": np.ones(3)}, "collides"),
    ({"a": np.ones((2, 2)), "a_cols": np.ones(3)}, "collides"),
    ([1.0, 2.0], "dict"),
])
def test_data_validation_raises_before_the_compiler_runs(data, match, monkeypatch):
    import tempest_amd as tp
    from tempest_amd import hipcallbacks
    monkeypatch.setattr(hipcallbacks, "build_plugin", lambda *a, **k: pytest.fail("the compiler ran"))
    with pytest.raises(ValueError, match=match):
        tp.HipCallbacks(WHOLE, 3, data=data)


def test_term_form_validation(monkeypatch):
    import tempest_amd as tp
    from tempest_amd import hipcallbacks
    monkeypatch.setattr(hipcallbacks, "build_plugin", lambda *a, **k: pytest.fail("the compiler ran"))
    both = REG + "__device__ double log_likelihood(const double* x, const tphu_data& D) { return 0.0; }\n"
    with pytest.raises(ValueError, match="both"):
        tp.HipCallbacks(both, 3, data=reg_data(10), n_terms=10)
    with pytest.raises(ValueError, match="n_terms"):
        tp.HipCallbacks(REG, 3, data=reg_data(10))
    with pytest.raises(ValueError, match="names no data entry"):
        tp.HipCallbacks(REG, 3, data=reg_data(10), n_terms="nope")
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="n_terms"):
            tp.HipCallbacks(REG, 3, data=reg_data(10), n_terms=bad)
    with pytest.raises(ValueError, match="log_likelihood_term"):
        tp.HipCallbacks(WHOLE, 3, data={"obs": np.ones((4, 3))}, n_terms=4)
    monkeypatch.setenv("TEMPEST_AMD_DATA_LIKE", "sideways")
    with pytest.raises(ValueError, match="TEMPEST_AMD_DATA_LIKE"):
        tp.HipCallbacks(REG, 3, data=reg_data(10), n_terms=10)


@needs_hipcc
def test_non_float64_input_is_converted_and_update_data_checks_the_shape():
    import tempest_amd as tp
    d = {k: v.astype(np.float32) for k, v in reg_data(50).items()}
    d["t"] = torch.from_numpy(d["t"])
    d["y"] = list(range(50))
    cb = tp.HipCallbacks(REG, 3, data=d, n_terms="t")
    assert cb.n_terms == 50 and all(a.dtype == np.float64 for a in cb._host.values())
    with pytest.raises(ValueError, match="shape"):
        cb.update_data("y", np.ones(51))
    with pytest.raises(ValueError, match="no data entry"):
        cb.update_data("w", np.ones(50))
    cb.update_data("y", np.ones(50, dtype=np.float32))


@needs_hipcc
def test_sampler_points_likelihood_args_to_data():
    import tempest_amd as tp
    cb = tp.HipCallbacks(REG, 3, data=reg_data(50), n_terms="t")
    for kw in ({"log_likelihood_args": [1.0]}, {"log_likelihood_kwargs": {"a": 1.0}}):
        with pytest.raises(ValueError, match="data="):
            tp.Sampler(cb.prior_transform, cb.log_likelihood, 3, n_particles=64, vectorize=True, **kw)


def test_sum_layout_is_the_one_design_md_states():
    import re
    from pathlib import Path
    from tempest_amd.hipcallbacks import SUM_LAYOUT
    design = (Path(__file__).resolve().parent.parent / "DESIGN.md").read_text()
    chunk = int(re.search(r"`TPHU_CHUNK = (\d+)`", design).group(1))
    block = int(re.search(r"`TPHU_BLOCK = (\d+)`", design).group(1))
    assert (chunk, block) == tuple(SUM_LAYOUT)


def test_path_rule_is_a_table_with_its_sweep_named():
    from tempest_amd.hipcallbacks import DATA_LIKE_THRESHOLDS, prefer_split
    assert DATA_LIKE_THRESHOLDS["source"].startswith("profiles/")
    assert not prefer_split(256, 1) and not prefer_split(1 << 20, 10 ** 6)
    t_min, n_below = DATA_LIKE_THRESHOLDS["bands"][0]
    assert prefer_split(n_below - 1, t_min) and not prefer_split(n_below, t_min)


# ------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@needs_hipcc
@pytest.mark.parametrize("n_terms", N_TERMS)
def test_sum_matches_numpy_bit_for_bit(n_terms):
    """Arithmetic-only term: both paths == the NumPy restatement (terms elementwise in the C expression's order, added in the
    chunk / block order), assert_array_equal.  Every split tile size gives the same bits too (the geometry is free)."""
    import tempest_amd as tp
    need_gpu()
    D = reg_data(n_terms)
    cb = tp.HipCallbacks(REG, 3, data=D, n_terms="t")
    for n in N_PARTICLES:
        x = particles(n, seed=n)
        want = reference_loglike(x, D, reg_terms, cb.sum_layout)
        xt = torch.from_numpy(x).cuda()
        for path in ("lane", "split"):
            cb.data_like = path
            got = cb.log_likelihood(xt).cpu().numpy()
            np.testing.assert_array_equal(got, want, err_msg=f"{path} n={n} n_terms={n_terms}")
        if n == 63:
            for tile in (64, 16, 4, 1):
                cb.split_tile = tile
                np.testing.assert_array_equal(cb.log_likelihood(xt).cpu().numpy(), want, err_msg=f"tile {tile}")
            cb.split_tile = 0
    cb.data_like = "split"
    np.testing.assert_array_equal(cb.log_likelihood(x), want)                     # NumPy in -> NumPy out
    assert cb.log_likelihood(xt[0]).item() == want[0]


@pytest.mark.gpu
@needs_hipcc
@pytest.mark.parametrize("n_terms", N_TERMS)
def test_lane_path_equals_split_path_with_exp_and_log(n_terms):
    """A Poisson count model (exp and log in the term): lane path == split path bitwise at every size.  Against the same
    restatement in np.longdouble (n = 1 and 63 at every n_terms) only a guard: the device's exp / log are not NumPy's.
    Largest relative difference observed on an MI355X: 1.251e-15 (n_terms = 255; 3.1e-16 ... 1.0e-15 at the other sizes);
    asserted: ten times that."""
    import tempest_amd as tp
    need_gpu()
    D = pois_data(n_terms)
    cb = tp.HipCallbacks(POIS, 3, data=D, n_terms=n_terms)
    worst = 0.0
    for n in N_PARTICLES:
        x = particles(n, seed=100 + n)
        xt = torch.from_numpy(x).cuda()
        cb.data_like = "lane"
        lane = cb.log_likelihood(xt).cpu().numpy()
        cb.data_like = "split"
        np.testing.assert_array_equal(cb.log_likelihood(xt).cpu().numpy(), lane, err_msg=f"n={n} n_terms={n_terms}")
        if n <= 63:
            want = reference_loglike(x, D, lambda xx, DD: pois_terms(xx, DD, np.longdouble), cb.sum_layout)
            worst = max(worst, float(np.max(np.abs((lane - want) / want))))
    print(f"n_terms={n_terms}: largest relative difference to the longdouble restatement {worst:.3e}")
    assert worst < 1.251e-14


@pytest.mark.gpu
@needs_hipcc
def test_two_objects_share_one_plugin_on_two_streams():
    import tempest_amd as tp
    need_gpu()
    Da, Db = reg_data(5000, seed=1), reg_data(3333, seed=2)
    a = tp.HipCallbacks(REG, 3, data=Da, n_terms="t")
    b = tp.HipCallbacks(REG, 3, data=Db, n_terms="t")
    assert a.path == b.path and a.lib._handle == b.lib._handle
    x = particles(700)
    xt = torch.from_numpy(x).cuda()
    wa, wb = (reference_loglike(x, D, reg_terms, a.sum_layout) for D in (Da, Db))
    a.data_like, b.data_like = "lane", "split"
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for rep in range(6):
        with torch.cuda.stream(sa):
            ra = a.log_likelihood(xt)
        with torch.cuda.stream(sb):
            rb = b.log_likelihood(xt)
        outs.append((ra, rb))
        if rep == 2:
            a.data_like, b.data_like = "split", "lane"
    torch.cuda.synchronize()
    for ra, rb in outs:
        np.testing.assert_array_equal(ra.cpu().numpy(), wa)
        np.testing.assert_array_equal(rb.cpu().numpy(), wb)


@pytest.mark.gpu
@needs_hipcc
@pytest.mark.parametrize("path", ["lane", "split"])
def test_update_data_reaches_a_captured_graph(path):
    import tempest_amd as tp
    need_gpu()
    D = reg_data(20_000)
    cb = tp.HipCallbacks(REG, 3, data=D, n_terms="t")
    cb.data_like = path
    x = particles(300)
    xt = torch.from_numpy(x).cuda()
    cb.log_likelihood(xt)                                  # tables uploaded, scratch sized: nothing is allocated by the object below
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = cb.log_likelihood(xt)
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), reference_loglike(x, D, reg_terms, cb.sum_layout))
    D2 = dict(D, y=D["y"] + 0.25)
    cb.update_data("y", D2["y"])
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), reference_loglike(x, D2, reg_terms, cb.sum_layout))


@pytest.mark.gpu
@needs_hipcc
def test_user_written_sum_reads_a_2d_table():
    import tempest_amd as tp
    need_gpu()
    D = reg_data(300)
    cb = tp.HipCallbacks(WHOLE, 3, data={"obs": np.stack([D["t"], D["y"], D["s"]], axis=1)})
    x = particles(500)
    z = (D["y"][None, :] - ((x[:, 0:1] + x[:, 1:2] * D["t"][None, :]) + (x[:, 2:3] * D["t"][None, :]) * D["t"][None, :])) / D["s"][None, :]
    np.testing.assert_array_equal(cb.log_likelihood(x), seq_sum_last((-0.5 * z) * z))
    np.testing.assert_array_equal(cb.prior_transform((x + 5.0) / 10.0), 10.0 * ((x + 5.0) / 10.0) - 5.0)


@pytest.mark.gpu
@needs_hipcc
@pytest.mark.parametrize("kernel", ["tpcn", "rwm"])
def test_fused_accept_with_data_is_bit_identical_to_library_accept(kernel):
    """tphu_accept with the data table == tph_accept fed with cb.prior_transform / cb.log_likelihood values (either path)."""
    import tempest_amd as tp
    from tempest_amd.device import HipContext, KERNEL_ID
    need_gpu()
    d, n, K = 3, 5000, 1
    cb = tp.HipCallbacks(REG, d, data=reg_data(2000), n_terms="t")
    ctx = HipContext(d, device=0)
    g = torch.Generator().manual_seed(3)
    # near the posterior, where the likelihood differences are of order one and both outcomes of the Metropolis test occur
    centre = (torch.tensor([0.7, 1.9, -1.1], dtype=torch.float64) + 5.0) / 10.0
    u = (centre[:, None] + 0.003 * torch.randn(d, n, generator=g, dtype=torch.float64)).cuda()
    up = (u.cpu() + 0.002 * torch.randn(d, n, generator=g, dtype=torch.float64)).clamp(0, 1).cuda()
    cb.data_like = "split"
    x = cb.prior_transform(u.T).T.contiguous()
    logl = cb.log_likelihood(x.T)
    mu, mup = torch.rand(n, generator=g, dtype=torch.float64).cuda() * 8, torch.rand(n, generator=g, dtype=torch.float64).cuda() * 8
    dof = torch.full((K,), 5.0, dtype=torch.float64).cuda()
    beta, seed, tick = 0.31, 99, 17
    a = [t.clone() for t in (u, x, logl)]
    sums_a = ctx.zeros(1 + K)
    xp = cb.prior_transform(up.T).T.contiguous()
    lp = cb.log_likelihood(xp.T)
    mu_a, mu_b = mu.clone(), mu.clone()
    ctx.accept(kernel, beta, a[0], a[1], a[2], up, xp, lp, mu_a, mup, None, K, dof, seed, tick, 0, sums_a)
    b = [t.clone() for t in (u, x, logl)]
    sums_b = ctx.zeros(1 + K)
    part = ctx.empty(((n + 255) // 256) * (1 + K))
    cb.accept(KERNEL_ID[kernel], beta, b[0], b[1], b[2], up, mu_b, mup, None, K, dof, seed, tick, 0, sums_b, partials=part)
    torch.cuda.synchronize()
    assert torch.equal(mu_a, mu_b)
    for ta, tb in zip(a, b):
        assert torch.equal(ta, tb)
    assert torch.equal(sums_a, sums_b)
    assert 0 < sums_a[0].item() < n


def closed_form_logz(D):
    A = np.stack([np.ones_like(D["t"]), D["t"], D["t"] ** 2], axis=1) / D["s"][:, None]
    b = D["y"] / D["s"]
    H = A.T @ A
    r = b - A @ np.linalg.solve(H, A.T @ b)
    return -0.5 * r @ r - D["c"].sum() + 1.5 * np.log(2.0 * np.pi) - 0.5 * np.linalg.slogdet(H)[1] - 3.0 * np.log(10.0)


@pytest.mark.gpu
@needs_hipcc
@pytest.mark.parametrize("graph", [False, True])
def test_whole_runs_with_data(graph, monkeypatch):
    """Fused == unfused, lane pinned == split pinned: equal evidence, step history and posterior arrays; and the evidence is the
    closed form of the Gaussian integral (box prior [-5, 5]^3, posterior many standard deviations inside) within 0.25."""
    import tempest_amd as tp
    need_gpu()
    D = reg_data(2000)
    assert abs(closed_form_logz(D) - (-2232.2646)) < 1e-3
    out = []
    for pin, fused in (("lane", True), ("lane", False), ("split", True), ("split", False)):
        monkeypatch.setenv("TEMPEST_AMD_DATA_LIKE", pin)
        cb = tp.HipCallbacks(REG, 3, data=D, n_terms="t", fused=fused)
        assert cb.use_split(2048) == (pin == "split") and cb.can_fuse_step(1, False, 2048) == (fused and pin == "lane")
        s = tp.Sampler(cb.prior_transform, cb.log_likelihood, 3, n_particles=2048, vectorize=True, clustering=False,
                       random_state=4, graph=graph)
        s.run(n_total=8192, progress=False)
        assert (s._core.callbacks.hip_plugin is cb) == fused
        out.append((s.evidence()[0], np.asarray(s.state.get_history("steps")), s.posterior()[0]))
    for o in out[1:]:
        assert o[0] == out[0][0]
        np.testing.assert_array_equal(o[1], out[0][1])
        np.testing.assert_array_equal(o[2], out[0][2])
    truth = closed_form_logz(D)
    print(f"logZ {out[0][0]:.4f}, closed form {truth:.4f}")
    assert abs(out[0][0] - truth) < 0.25, (out[0][0], truth)
