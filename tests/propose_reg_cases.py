"""Input recipes of tests/test_propose_reg_gpu.py (the d <= 16 proposal kernel against oracle/mcmc.py: propose), kept apart
from it so that tests/test_host_logic.py can check, with the oracle alone, that they put the kernel where the GPU tests
claim: a redraw loop of several rounds (20-70 % of the first attempts out of the cube) in the ordinary ensembles, a real
mix of capped and proposing walkers in the redraw-cap ensembles."""
import numpy as np

from oracle import mcmc as omc
from oracle import philox as px
from oracle import ps

SEED, TICK, ITEM0 = 4242, 11, 100_000
DIMS = tuple(range(1, 17))
CAP_DIMS = (1, 8, 16)


def step_scale(d, kernel, K):
    """Common factor g on the modes' Cholesky factors and on the spread of the walkers of the recipe of
    test_propose_accept_adapt_vs_oracle (A = 0.08 randn, walkers 0.2 randn around their mode's mean).  With g = 1 that recipe
    redraws 1 % of the proposals at d = 1 and 90 % (a tenth of them up to the cap) at d = 16, tpCN; these powers of d keep the
    share of first attempts out of the cube near 40 % at every d and the walkers that reach the redraw cap below 1 %
    (tests/test_host_logic.py: test_propose_reg_recipes_*)."""
    if kernel == "rwm":
        return 2.5 / d ** 0.35
    if d == 1:                                  # one coordinate: the contraction towards the mean keeps most attempts inside
        return 12.0 if K == 1 else 5.0
    return (2.6 if K == 1 else 3.9) / d ** 0.6


def ensemble(d, kernel, K, n, g=None, sigmas=None, dof=None, spread=0.2, seed=0):
    """One ensemble of n walkers over K modes: means 0.5 +- 0.1, random SPD covariances, walkers clipped to [0.01, 0.99] (many
    sit on a wall).  Returns a dict of host arrays; particle arrays are (n, d)."""
    rs = np.random.RandomState(1000 * d + 10 * K + (kernel == "rwm") + 100_000 * seed)
    g = step_scale(d, kernel, K) if g is None else g
    means = 0.5 + 0.1 * rs.randn(K, d)
    covs = np.empty((K, d, d))
    for k in range(K):
        A = rs.randn(d, d) * 0.08 * g
        covs[k] = A @ A.T + 1e-3 * g * g * np.eye(d)
    _, chol, inv = ps.mode_statistics(means, covs)
    if dof is None:
        dof = np.array([1e6, 4.0, 25.0])[:K] if K > 1 else np.array([4.0])
    if sigmas is None:
        sigmas = (np.array([0.9, 0.5, 0.2])[:K] if K > 1 else np.array([0.7])) * (2.38 / np.sqrt(d) if kernel == "rwm" else 1.0)
    assign = rs.randint(K, size=n).astype(np.int32)
    u = np.clip(means[assign] + spread * g * rs.randn(n, d), 0.01, 0.99)
    return dict(d=d, n=n, K=K, kernel=kernel, means=means, chol=chol, inv=inv, dof=np.asarray(dof, dtype=np.float64),
                sigmas=np.asarray(sigmas, dtype=np.float64), assign=assign, u=u)


# (g, sigma) of the redraw-cap ensembles (one mode, dof 4, the walkers spread 0.2 as in the ordinary ones): a step so large that
# 10-90 % of the walkers fail all 256 attempts while the others win at attempts spread over 1 ... 255.  RWM: sigma does it;
# tpCN has sigma < 1, there the covariance is blown up.
CAP_STEP = {("rwm", 1): (1.0, 600.0), ("rwm", 8): (1.0, 4.0), ("rwm", 16): (1.0, 1.5),
            ("tpcn", 1): (1000.0, 0.95), ("tpcn", 8): (10.0, 0.95), ("tpcn", 16): (1.0, 0.95)}


def cap_ensemble(d, kernel, n=4097):
    g, sigma = CAP_STEP[kernel, d]
    return ensemble(d, kernel, 1, n, g=g, sigmas=[sigma], dof=[4.0], spread=0.2 / g, seed=1)


def runaway_ensemble(d, n=777):
    """RWM with a step so large that all 256 attempts of every walker leave the cube (the runaway of DESIGN section 9, as in
    test_stage_machine_redraw_cap_proposes_the_current_point: covariance 0.08 I, sigma 30).  Per attempt a coordinate stays in
    the cube with probability ~ 1 / (2.5 sigma 0.28), so with one coordinate it takes sigma = 1e9 for 777 x 256 attempts to fail."""
    means = np.full((1, d), 0.5)
    _, chol, inv = ps.mode_statistics(means, (np.eye(d) * 0.08)[None])
    u = np.random.RandomState(4 + d).rand(n, d)
    return dict(d=d, n=n, K=1, kernel="rwm", means=means, chol=chol, inv=inv, dof=np.array([1e6]),
                sigmas=np.array([1e9 if d == 1 else 30.0]), assign=np.zeros(n, dtype=np.int32), u=u)


def flags_for(d, bc, which=0):
    """bc None: every coordinate strict.  "mixed": periodic on coordinate 0 and reflective on coordinate d - 1 (d = 1: `which`
    0 periodic, 1 reflective)."""
    if not bc:
        return omc.bc_flags(d)
    if d == 1:
        return omc.bc_flags(1, [0], None) if which == 0 else omc.bc_flags(1, None, [0])
    return omc.bc_flags(d, [0], [d - 1])


def oracle(e, flags, a=0, b=None, seed=SEED, tick=TICK, item0=ITEM0):
    """omc.propose on the walkers [a, b) of the ensemble (their items are item0 + a ...): (u', form at u, form at u')"""
    b = e["n"] if b is None else b
    return omc.propose(e["kernel"], e["u"][a:b], e["assign"][a:b], e["means"], e["chol"], e["inv"], e["dof"], e["sigmas"], flags,
                       seed, tick, item0 + a)


def first_attempt_out(e, flags, seed=SEED, tick=TICK, item0=ITEM0):
    """Share of the walkers whose attempt 0 leaves the cube, recomputed as omc.propose computes it."""
    n, d, assign = e["n"], e["d"], e["assign"]
    items = np.arange(n, dtype=np.uint64) + np.uint64(item0)
    sig = e["sigmas"][assign]
    z = px.normals(seed, items, d, tick, px.TAG_NORMAL, attempt=0)
    Lz = np.einsum("ijk,ik->ij", e["chol"][assign], z)
    if e["kernel"] == "tpcn":
        mu = e["means"][assign]
        diff = e["u"] - mu
        m_u = np.einsum("ij,ijk,ik->i", diff, e["inv"][assign], diff)
        nu = e["dof"][assign]
        gam = px.gamma_mt(seed, items, 0.5 * (d + nu), tick) * (2.0 / (nu + m_u))
        v = mu + np.sqrt(1.0 - sig * sig)[:, None] * diff + (sig * np.sqrt(1.0 / gam))[:, None] * Lz
    else:
        v = e["u"] + sig[:, None] * Lz
    _, ok = omc._apply_bc(v, flags)
    return 1.0 - ok.mean()


def cap_rows(e, want_up):
    """Walkers for which the oracle proposed the current point: all 256 attempts out of the cube (an in-bounds RWM attempt
    never reproduces u; for tpCN neither, short of mu + a (u - mu) + b L z == u to the last bit)."""
    return np.all(want_up == e["u"], axis=1)


REG_MAX_TILES = 8


def launch_geometry(n, n_simd, redraw_lanes=0):
    """(waves, tiles per wave) of k_propose_reg for n rows, exactly as launch_propose_reg computes them
    (tempest_amd/csrc/mutate.hip:960-969): one wave per workgroup; a wave owns the 64-row tiles w + k * waves, k < tiles."""
    ntiles = (n + 63) // 64
    waves = min(4 * n_simd, ntiles)
    if ntiles > waves * REG_MAX_TILES:
        waves = (ntiles + REG_MAX_TILES - 1) // REG_MAX_TILES
    tiles = (ntiles + waves - 1) // waves
    if redraw_lanes > 0:
        tiles = min(redraw_lanes, REG_MAX_TILES)
    waves = (ntiles + tiles - 1) // tiles
    return waves, tiles


def rolled_form(kernel, d, n, n_simd):
    """Does a one-mode launch without boundary conditions take the rolled instantiation <.., true, 4, false> (tpCN at
    d = 12 ... 16 with more than two waves per SIMD) instead of the interleaved <.., true, 2, false>?  (mutate.hip:977-978)"""
    return kernel == "tpcn" and d > 11 and launch_geometry(n, n_simd)[0] > 2 * n_simd
