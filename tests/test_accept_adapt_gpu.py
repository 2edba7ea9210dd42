"""The three library kernels that end every MCMC step -- k_accept, the canonical column sums of its block partials
(k_accept_sums, or folded into k_adapt) and the scalar adaptation tph_adapt_scalar (csrc/mutate.hip, csrc/common.h) -- against
the references of tests/accept_cases.py, which tests/test_accept_ref.py checks on the CPU.

Tolerances.  Sums, partials, the adaptation, masks and every written array: bit for bit (assert_array_equal).  Per-row alpha:
C_DEVICE * b_i relative with b_i from alpha_ref (accept_cases.py: the bound, the constant and the measured ratios); references
that are exactly 0 or 1 are hit exactly.  Sums against math.fsum: (n - 1) 2^-53 relative (non-negative terms, any order).

What these tests cannot tell apart.  `U <= alpha` for `U < alpha`: the two differ only where U == alpha bit for bit, i.e. at
alpha = 0 with U = 0, one draw in 2^53 (the NaN -> 0 rows of the edge table are there, their uniforms are not 0).  The LDS / global
switch of k_adapt written `<` for `<=`: both paths give the same sums; K = 63 at n = 4096 fills s_vs[1024] to its last entry (an
array one short would lose shard 15's last column and fail test_three_routes_to_the_sums), K = 64 takes the global path."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import accept_cases as ac  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_CTX = {}


def ctx(d):
    from tempest_amd.device import HipContext
    if d not in _CTX:
        _CTX[d] = HipContext(d, 0)
    return _CTX[d]


def T(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype=dtype))
    return torch.from_numpy(a.copy()).cuda()


def H(t):
    return t.cpu().numpy()


def kid(kernel):
    from tempest_amd.device import KERNEL_ID
    return KERNEL_ID[kernel]


def raw_accept(c, kernel, beta, u, x, logl, up, xp, lp, mu, mup, assign, n, ld, K, dof, sums, partials, pending, tick=ac.TICK):
    """tph_accept as the C ABI has it (the Python wrapper always passes ld = n and checks some arguments itself)."""
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    return c.lib.tph_accept(c._ctx, kid(kernel), float(beta), p(u), p(x), p(logl), p(up), p(xp), p(lp), p(mu), p(mup), p(assign),
                            n, ld, K, p(dof), ac.SEED, tick, ac.ITEM0, p(sums), None, p(partials), p(pending))


def last_error(c):
    return c.lib.tph_last_error().decode()


class Call:
    """Device copies of one input set (fresh for every call: tph_accept updates logl, maha_u and the points in place)."""

    def __init__(self, r, assign, K, dof, d=None, with_x=False, seed=0):
        self.r, self.K, self.d = r, K, r.d if d is None else d
        n = r.n
        rs = np.random.RandomState(seed)
        self.u_h, self.up_h = rs.rand(self.d, n), rs.rand(self.d, n)
        self.u, self.up = T(self.u_h), T(self.up_h)
        self.x, self.xp = (T(2.0 * self.u_h - 1.0), T(2.0 * self.up_h - 1.0)) if with_x else (None, None)
        self.logl, self.lp = T(r.logl), T(r.loglp)
        tp = r.kernel == "tpcn"
        self.mu, self.mup = (T(r.maha_u), T(r.maha_up)) if tp else (None, None)
        self.assign = None if assign is None else T(assign, np.int32)
        self.dof = T(dof) if tp else None

    def accept(self, c, beta, sums, partials=None, pending=None):
        r = self.r
        c.accept(r.kernel, beta, self.u, self.x, self.logl, self.up, self.xp, self.lp, self.mu, self.mup, self.assign, self.K,
                 self.dof, ac.SEED, ac.TICK, ac.ITEM0, sums, partials=partials, pending=pending)


def refs(r, beta):
    a, b = ac.alpha_ref(r.kernel, beta, r.logl, r.loglp, r.maha_u, r.maha_up, r.nu, r.d)
    return a, b, ac.uniforms(r.n) < a


def cluster_args(r, K):
    """(assign, dof) of a K = 1 (no assignments) or K = len(dofs) call."""
    return (None if K == 1 else r.cluster), np.asarray(r.dofs)


def per_row_alpha(c, r, beta, d=None):
    """The device's alpha of every row, observed through K = n: with a permutation as assignments column 1 + k of the sums holds
    exactly one alpha (adding zeros is exact).  -> (alpha per row, #accepted)."""
    n = r.n
    assert n <= 4096
    perm = np.random.RandomState(n).permutation(n).astype(np.int32)
    dof = np.empty(n)
    dof[perm] = r.nu
    call = Call(r, perm, n, dof, d=d)
    sums = c.empty(1 + n)
    call.accept(c, beta, sums)
    s = H(sums)
    return s[1:][perm], s[0]


# ------------------------------------------------------------------------------------------------ 1. per-row alpha
@pytest.mark.parametrize("d", ac.ALPHA_DIMS)
@pytest.mark.parametrize("kernel", ac.KERNELS)
def test_alpha_per_row_within_the_bound(kernel, d):
    """tph_tpcn_factor (lean log and division, library log from 1e300) and the exp of k_accept, row by row: random forms over
    seven decades at four dofs, the +-inf / NaN likelihood pairs, forms 0 / inf / NaN, forms around 1e300 nu, beta 0, 0.6, 1."""
    r = ac.alpha_rows(kernel, d)
    c = ctx(d)
    for beta in ac.BETAS:
        a, b, mask = refs(r, beta)
        got, n_acc = per_row_alpha(c, r, beta)
        ratio = ac.alpha_ratio(got, a, b)
        worst = int(np.argmax(ratio))
        print(f"alpha {kernel} d={d} beta={beta}: worst ratio {ratio[worst]:.4f} of {ac.C_DEVICE} at row {worst} "
              f"(ref {a[worst]!r}, device {got[worst]!r}, nu {r.nu[worst]}, forms {r.maha_u[worst]!r} {r.maha_up[worst]!r})")
        bad = np.nonzero(~(ratio <= ac.C_DEVICE))[0]
        assert bad.size == 0, (beta, bad[:8], a[bad[:8]], got[bad[:8]], ratio[bad[:8]])
        exact = (a == 0) | (a == 1)
        np.testing.assert_array_equal(got[exact], a[exact])
        assert n_acc == mask.sum()
        if beta == 0.0:        # 0 * inf: no infinite likelihood difference moves a row
            with np.errstate(invalid="ignore"):
                assert not got[np.isinf(r.loglp - r.logl)].any()


# ------------------------------------------------------------------------------- 2. decisions and writes
@pytest.mark.parametrize("mode", ["in_place_x", "in_place", "deferred"])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096])
@pytest.mark.parametrize("kernel", ac.KERNELS)
def test_decisions_and_writes(kernel, n, K, mode):
    r = ac.decision_rows(kernel, n, K)
    beta = 0.6 if K == 3 else 1.0
    a, b, mask = refs(r, beta)
    c = ctx(r.d)
    assign, dof = cluster_args(r, K)
    call = Call(r, assign, K, dof, with_x=mode == "in_place_x", seed=n)
    pending = torch.full((n,), 7, dtype=torch.uint8, device="cuda") if mode == "deferred" else None
    sums = c.empty(1 + K)
    call.accept(c, beta, sums, pending=pending)
    s = H(sums)
    assert s[0] == mask.sum()
    if mode == "deferred":
        np.testing.assert_array_equal(H(pending), mask.astype(np.uint8))
        np.testing.assert_array_equal(H(call.u), call.u_h)
    else:
        np.testing.assert_array_equal(H(call.u), np.where(mask[None, :], call.up_h, call.u_h))
    if call.x is not None:
        np.testing.assert_array_equal(H(call.x), np.where(mask[None, :], 2.0 * call.up_h - 1.0, 2.0 * call.u_h - 1.0))
    np.testing.assert_array_equal(H(call.logl), np.where(mask, r.loglp, r.logl))
    if kernel == "tpcn":
        np.testing.assert_array_equal(H(call.mu), np.where(mask, r.maha_up, r.maha_u))
        np.testing.assert_array_equal(H(call.mup), r.maha_up)
    np.testing.assert_array_equal(H(call.up), call.up_h)
    np.testing.assert_array_equal(H(call.lp), r.loglp)
    # NaN / -inf proposals never move; +inf against a finite value always does (U < 1)
    assert not mask[np.isnan(r.loglp) | (r.loglp == -np.inf)].any()
    forms_ok = np.isfinite(r.maha_u) & np.isfinite(r.maha_up) if kernel == "tpcn" else np.ones(n, dtype=bool)
    assert mask[(r.loglp == np.inf) & np.isfinite(r.logl) & forms_ok].all()
    # the alpha columns: the sums of the reference alphas, to the per-row bound (bit for bit against the device's own
    # alphas: test_block_partials_bit_for_bit)
    for k in range(K):
        sel = r.cluster == k
        assert abs(s[1 + k] - a[sel].sum()) <= (ac.C_DEVICE * b[sel] * a[sel]).sum() + n * ac.EPS * a[sel].sum()


@pytest.mark.parametrize("kernel", ac.KERNELS)
def test_leading_dimension_larger_than_n(kernel):
    """tph_accept with ld > n (the wrapper always passes ld = n): rows are found at stride ld, padding columns stay untouched."""
    n, ld, K = 257, 320, 3
    r = ac.decision_rows(kernel, n, K)
    a, b, mask = refs(r, 0.6)
    c = ctx(r.d)
    d = r.d
    rs = np.random.RandomState(5)
    pad = lambda v: np.concatenate([v, np.full((d, ld - n), -7.0)], axis=1)  # noqa: E731
    u_h, up_h = rs.rand(d, n), rs.rand(d, n)
    u, up, x, xp = T(pad(u_h)), T(pad(up_h)), T(pad(-u_h)), T(pad(-up_h))
    logl, lp = T(r.logl), T(r.loglp)
    tp = kernel == "tpcn"
    mu, mup = (T(r.maha_u), T(r.maha_up)) if tp else (None, None)
    sums = c.empty(1 + K)
    rc = raw_accept(c, kernel, 0.6, u, x, logl, up, xp, lp, mu, mup, T(r.cluster, np.int32), n, ld, K,
                    T(np.asarray(r.dofs)) if tp else None, sums, None, None)
    assert rc == 0, last_error(c)
    assert H(sums)[0] == mask.sum()
    np.testing.assert_array_equal(H(u), pad(np.where(mask[None, :], up_h, u_h)))
    np.testing.assert_array_equal(H(x), pad(np.where(mask[None, :], -up_h, -u_h)))
    np.testing.assert_array_equal(H(up), pad(up_h))
    np.testing.assert_array_equal(H(xp), pad(-up_h))
    np.testing.assert_array_equal(H(logl), np.where(mask, r.loglp, r.logl))


# ---------------------------------------------------------------------------------- 3. block partials, bit for bit
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n", [4096, 1000])
@pytest.mark.parametrize("kernel", ac.KERNELS)
def test_block_partials_bit_for_bit(kernel, n, K):
    """partials[block][1 + K] is tph_block_sum of the device's OWN per-row alphas (seen through K = n) and decisions: the
    shuffle tree per wave, then (w0 + w2) + (w1 + w3); n = 1000 leaves a ragged last block."""
    r = ac.decision_rows(kernel, n, K)
    beta = 0.6
    c = ctx(r.d)
    alpha, n_acc = per_row_alpha(c, r, beta)
    mask = ac.uniforms(n) < alpha
    assert n_acc == mask.sum()
    assign, dof = cluster_args(r, K)
    call = Call(r, assign, K, dof)
    partials = torch.full((((n + 255) // 256) * (1 + K),), -1.0, dtype=torch.float64, device="cuda")
    call.accept(c, beta, None, partials=partials)
    want = ac.block_partials_ref(alpha, mask, assign, K)
    np.testing.assert_array_equal(H(partials).reshape(want.shape), want)


# ----------------------------------------------------------------------------- 4. the canonical sums, at every V
SUM_CASES = ([(n, 3) for n in (256, 512, 768, 1024, 1536, 2048, 3072, 4096, 12288)]       # V = 1 ... 48, one block per shard
             + [(266240, 3),            # V = 16 with 65 blocks per shard: the second trip of the lane loop
                (266241, 3),            # not canonical: one shard of 1041 blocks
                (5000, 3)]
             + [(4096, K) for K in (1, 63, 64)]    # vl (1 + K) = 16, 1024, 1040: across the LDS / global switch of k_adapt
             + [(256, 1), (512, 1), (768, 1)])     # vl (1 + K) = 2, 4 (256-thread launch), 6


# (the ensembles above 12 288 particles once: the sums do not know the kernel)
@pytest.mark.parametrize("kernel,n,K", [(k, n, K) for k in ac.KERNELS for n, K in SUM_CASES if k == "tpcn" or n <= 12288])
def test_three_routes_to_the_sums(kernel, n, K):
    """The sums of one accept call by (a) tph_accept_sums_global without a communicator, (b) tph_accept(sums_dev), (c) tph_adapt
    folding the partials: one tree -- active_partition, a wave per (shard, column), the fold in shard order -- restated by
    sums_ref on the partials read back."""
    r = ac.sum_rows(kernel, n, K)
    c = ctx(r.d)
    beta = 0.6
    assign = None if K == 1 else r.cluster
    dof = np.asarray(r.dofs)
    nb = (n + 255) // 256
    first = Call(r, assign, K, dof)
    p1 = torch.full((nb * (1 + K),), -1.0, dtype=torch.float64, device="cuda")
    first.accept(c, beta, None, partials=p1)
    P = H(p1).reshape(nb, 1 + K)
    want = ac.sums_ref(P, n, K)
    sa = c.accept_sums_global(p1, n, K, torch.full((1 + K,), -1.0, dtype=torch.float64, device="cuda"))
    second = Call(r, assign, K, dof)
    p2, sb = torch.full_like(p1, -2.0), torch.full((1 + K,), -1.0, dtype=torch.float64, device="cuda")
    second.accept(c, beta, sb, partials=p2)
    third = Call(r, assign, K, dof)                        # (b) with the partials in the library's own scratch
    sb2 = torch.full((1 + K,), -1.0, dtype=torch.float64, device="cuda")
    third.accept(c, beta, sb2)
    counts = c.cluster_counts(first.assign, n, K)
    sc = torch.full((1 + K,), -1.0, dtype=torch.float64, device="cuda")
    sig, state = torch.full((K,), 0.3, dtype=torch.float64, device="cuda"), c.zeros(10)
    c.adapt(kernel, sc, counts, K, n, 2, 40, sig, state, partials=p1, n=n)
    np.testing.assert_array_equal(H(p2), H(p1))
    np.testing.assert_array_equal(H(sa), want)
    np.testing.assert_array_equal(H(sb), want)
    np.testing.assert_array_equal(H(sb2), want)
    np.testing.assert_array_equal(H(sc), want)
    np.testing.assert_array_equal(H(p1).reshape(nb, 1 + K), P)             # tph_adapt reads the partials, nothing else
    assert H(state)[0] == 1.0 and H(state)[2] == want[0] / n
    fs = ac.fsum_columns(P, K)
    assert want[0] == fs[0] == P[:, 0].sum()
    assert (np.abs(want[1:] - fs[1:]) <= (n - 1) * ac.EPS * fs[1:]).all()
    assert 0 < want[0] < n and (want[1:] > 0).all()


# ------------------------------------------------------------------------------------- 5. tph_adapt_scalar
@pytest.mark.parametrize("kernel", ac.KERNELS)
def test_adapt_scalar_on_the_grid(kernel):
    """sigmas, state[0..5] and the stop flag of every case of the grid (empty first / middle / last clusters and the
    sigmas[:n_nonempty] quirk, both clamps of tpCN, the floors of acc and sigma, each of n_min, n_adapt, n_max d winning, the
    int() truncation, n_global = 2 n, 0 / 4 / 999 steps done): exactly adapt_ref."""
    bad = []
    cases = ac.adapt_cases(kernel)
    fused_matters = 0
    for case in cases:
        c = ctx(case.d)
        sums, counts, sig = T(np.array(case.sums)), T(np.array(case.counts)), T(np.array(case.sigmas))
        state = c.zeros(10)
        state[0] = float(case.steps_done)
        c.adapt(kernel, sums, counts, case.K, case.n_global, case.n_steps, case.n_max, sig, state)
        args = (kernel, case.sums, case.counts, case.K, case.sigmas, case.steps_done, case.n_global, case.d, case.n_steps,
                case.n_max)
        ws, wst = ac.adapt_ref(*args)
        ps, pst = ac.adapt_ref(*args, contract=False)
        fused_matters += int(not (np.array_equal(ws, ps) and np.array_equal(wst, pst)))
        gs, gst = H(sig), H(state)
        if not (np.array_equal(gs, ws) and np.array_equal(gst[:6], wst) and not gst[6:].any()):
            bad.append((case.label, gs, ws, gst[:6], wst))
        for k in range(case.K):
            if case.counts[k] == 0:
                assert gs[k] == case.sigmas[k], case.label          # an empty cluster keeps its sigma bit for bit
        np.testing.assert_array_equal(H(sums), np.array(case.sums))
    print(f"adapt {kernel}: {len(cases)} cases, {len(bad)} differ; the fused multiply-adds change {fused_matters} of them")
    assert not bad, bad[:5]


def test_adapt_mailbox_ring_and_stop():
    """Six successive steps into a pinned ring of 4 slots: slot iteration % 4 holds state[0..5], state[8] in field 6 and the
    iteration in field 7, older records are overwritten in ring order; once the stop flag is up a further call changes nothing."""
    kernel, d, K, n = "tpcn", 3, 2, 1000.0
    c = ctx(d)
    sums_h, counts_h = [n, 120.0, 150.0], [400.0, 600.0]       # every move accepted, mean alphas 0.3 and 0.25
    sums, counts = T(np.array(sums_h)), T(np.array(counts_h))
    sig_h = np.array([0.9, 0.95])
    sig = T(sig_h)
    state = c.zeros(10)
    state[8] = 3.25
    mailbox = torch.full((4, 8), -1.0, dtype=torch.float64).pin_memory()
    want_box = np.full((4, 8), -1.0)
    for it in range(1, 7):
        c.adapt(kernel, sums, counts, K, n, 2, 40, sig, state, mailbox=mailbox)
        c.synchronize()
        sig_h, st = ac.adapt_ref(kernel, sums_h, counts_h, K, sig_h, it - 1, n, d, 2, 40)
        want_box[it % 4] = list(st) + [3.25, float(it)]
        np.testing.assert_array_equal(mailbox.numpy(), want_box, err_msg=f"step {it}")
        np.testing.assert_array_equal(H(state)[:6], st)
        np.testing.assert_array_equal(H(sig), sig_h)
        assert st[1] == (1.0 if it == 6 else 0.0)            # n_min = n_steps d = 6 wins: the rule fires at the sixth step
    frozen = (H(state).copy(), H(sig).copy(), mailbox.numpy().copy())
    c.adapt(kernel, sums, counts, K, n, 2, 40, sig, state, mailbox=mailbox)
    c.synchronize()
    np.testing.assert_array_equal(H(state), frozen[0])
    np.testing.assert_array_equal(H(sig), frozen[1])
    np.testing.assert_array_equal(mailbox.numpy(), frozen[2])


# ------------------------------------------------------------------------------------- 6. tph_cluster_counts
@pytest.mark.parametrize("K", [1, 3, 4096])
@pytest.mark.parametrize("n", [1, 257, 100_003])
def test_cluster_counts(n, K):
    c = ctx(3)
    rs = np.random.RandomState(n + K)
    lab = rs.randint(K, size=n).astype(np.int32)
    out = rs.rand(n) < 0.2                                  # labels outside [0, K) are ignored
    lab[out] = rs.choice(np.array([-1, K, 2 ** 31 - 1, -2 ** 31], dtype=np.int64), size=int(out.sum())).astype(np.int32)
    if n > 1:
        lab[:2] = (0, K - 1)
    got = H(c.cluster_counts(T(lab), n, K))
    ok = (lab >= 0) & (lab < K)
    np.testing.assert_array_equal(got, np.bincount(lab[ok], minlength=K).astype(np.float64))
    none = H(c.cluster_counts(None, n, K))
    np.testing.assert_array_equal(none, np.array([float(n)] + [0.0] * (K - 1)))


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_come_before_any_launch():
    from tempest_amd._lib import TempestHipError
    n, K = 300, 3
    r = ac.decision_rows("tpcn", 257, 3)
    c = ctx(r.d)
    d = r.d
    u, up, x, xp = (c.zeros(d, n) for _ in range(4))
    logl, lp, mu, mup = (c.zeros(n) for _ in range(4))
    assign = torch.zeros(n, dtype=torch.int32, device="cuda")
    dof = T(np.asarray(ac.DOFS3))
    sums = torch.full((1 + K,), -5.0, dtype=torch.float64, device="cuda")
    partials = torch.full((2 * (1 + K),), -5.0, dtype=torch.float64, device="cuda")
    pending = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    big = torch.zeros(4098, dtype=torch.float64, device="cuda")

    def refused(text, *a, **kw):
        rc = raw_accept(c, *a, **kw)
        assert rc == -2 and text in last_error(c), (rc, last_error(c))
    refused("deferred mode (pending_dev) does not maintain x", "tpcn", 0.5, u, x, logl, up, xp, lp, mu, mup, assign, n, n, K, dof,
            sums, partials, pending)
    refused("K>1 needs assignments", "tpcn", 0.5, u, x, logl, up, xp, lp, mu, mup, None, n, n, K, dof, sums, partials, None)
    refused("K=4097 too large", "tpcn", 0.5, u, x, logl, up, xp, lp, mu, mup, assign, n, n, 4097, big, big, None, None)
    refused("tpCN needs maha/dof", "tpcn", 0.5, u, x, logl, up, xp, lp, None, mup, assign, n, n, K, dof, sums, partials, None)
    refused("tpCN needs maha/dof", "tpcn", 0.5, u, x, logl, up, xp, lp, mu, mup, assign, n, n, K, None, sums, partials, None)
    refused("without sums_dev the block partials must go to partials_dev", "tpcn", 0.5, u, x, logl, up, xp, lp, mu, mup, assign,
            n, n, K, dof, None, None, None)
    refused("bad sizes", "tpcn", 0.5, u, x, logl, up, xp, lp, mu, mup, assign, n, n - 1, K, dof, sums, partials, None)
    counts, sig, state = c.zeros(K), c.zeros(K), c.zeros(10)
    with pytest.raises(TempestHipError, match="partials need the particle count"):
        c.adapt("tpcn", sums, counts, K, n, 2, 40, sig, state, partials=partials, n=0)
    mailbox = torch.full((4, 8), -1.0, dtype=torch.float64).pin_memory()
    rc = c.lib.tph_adapt(c._ctx, kid("tpcn"), sums.data_ptr(), counts.data_ptr(), K, float(n), d, 2, 40, sig.data_ptr(),
                         state.data_ptr(), mailbox.data_ptr(), 0, None, 0)
    assert rc == -2 and "mailbox needs at least one slot" in last_error(c)
    # nothing ran: every output still holds what it held
    c.synchronize()
    assert (H(sums) == -5.0).all() and (H(partials) == -5.0).all() and (H(pending) == 9).all()
    assert not H(state).any() and not H(u).any() and (mailbox.numpy() == -1.0).all()
