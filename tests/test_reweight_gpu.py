"""The log-mixture (k_logmix_append), the reweighting pass (k_reweight_reduce<NB, U>, k_reweight_vshards, k_reweight_fold) and the
weight kernels (k_weights, k_logw, k_sum_sq_max, k_sum_sq_max_final) through HipContext, against the references and derived bounds
of tests/reweight_cases.py (checked on the CPU by tests/test_reweight_cases.py).

Tolerances: none that is a constant.  A comparison is either assert_array_equal -- the exact counts at every launch geometry, the
gathered merge against the plain fold, one unroll class against itself, the maximum and k_logw against their two correctly rounded
forms, k_sum_sq_max on its lattice -- or a bound the cases module derives from the inputs of the case.  The largest error of each
family as a fraction of its bound is printed when the module finishes (run with -s)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import reweight_cases as rc  # noqa: E402

LD = rc.LD
_CTX = {}
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()
    for family, (frac, where) in sorted(_WORST.items()):
        print(f"\nlargest error / bound  {family}: {frac:.3g}  ({where})", end="")
    print()


def ctx(kind="plain"):
    """One context per kind for the whole module: plain | loop (one-rank loopback communicator) | p2p (with the peer-to-peer layer)."""
    if kind not in _CTX:
        from tempest_amd.comm import attach_loopback
        from tempest_amd.device import HipContext
        c = HipContext(1, 0)
        if kind != "plain":
            attach_loopback(c, p2p=(kind == "p2p"))
            assert c.p2p_active == (kind == "p2p")
        _CTX[kind] = c
    return _CTX[kind]


def load(c, h):
    from tempest_amd.device import KEY_LOGMIX
    c.history_load(None, None, h.logl, h.bt, h.zt, h.nt)
    return c.history_read(KEY_LOGMIX)


def note(family, frac, where):
    if frac > _WORST.get(family, (-1.0, ""))[0]:
        _WORST[family] = (float(frac), where)


def same_bits(got, want, msg=""):
    np.testing.assert_array_equal(rc.bits(got), rc.bits(want), err_msg=msg)


def same_count(got, want, msg=""):
    """Bit for bit, but for the sign of a zero maximum: with one row in one iteration C = log 1 = 0, and v = beta l - C is +0 or -0
    with the sign of beta l."""
    same_bits(np.asarray(got) + 0.0, np.asarray(want) + 0.0, msg)


def check_triple(got, h, C, beta, g, nb, where):
    """One device triple against the long-double reference on the device's own C, every figure within its derived bound."""
    ref = rc.acc_reference(h.logl, C, beta)
    bound = rc.acc_bound(h.logl, beta, ref, g, nb)
    err = rc.acc_errors(got, ref)
    for name, e, b in zip(bound._fields, err, bound):
        print(f"{where} beta={beta} nb={nb} {name}: error {e:.3e} bound {b:.3e}")
        assert e <= b, (where, beta, nb, name, e, b)
        if b > 0:
            note("K2 " + name, e / b, f"{where}, beta {beta}, nb {nb}")
    return ref, bound


# ------------------------------------------------------------------------- 1. every row exactly once, at every launch geometry
@pytest.mark.parametrize("case", rc.COUNT_GEOMS, ids=lambda c: c.name)
def test_every_row_is_counted_exactly_once(case):
    from tempest_amd.device import OPT_REDUCE_GRID
    c = ctx()
    c.set_option(OPT_REDUCE_GRID, case.reduce_grid)
    try:
        for label, on in rc.count_patterns(case):
            C = load(c, rc.History(*rc.count_history(case, on)))
            assert np.all(rc.bits(C) == rc.bits(C)[0]), (case.name, label)
            want = rc.count_expected(C[0], on.size, int(on.sum()), rc.COUNT_BETAS)
            same_count(c.reweight_eval(rc.COUNT_BETAS), want, f"{case.name} {label}: reweight_eval")
            same_count(c.reweight_partials(rc.COUNT_BETAS).cpu().numpy(), want, f"{case.name} {label}: reweight_partials")
    finally:
        c.set_option(OPT_REDUCE_GRID, 0)


@pytest.mark.parametrize("name", rc.COUNT_WIDTH_GEOMS)
def test_every_batch_width_counts_every_row(name):
    case = rc.COUNT_BY_NAME[name]
    c = ctx()
    label, on = next(iter(rc.count_patterns(case)))
    C = load(c, rc.History(*rc.count_history(case, on)))
    want = rc.count_expected(C[0], on.size, int(on.sum()), rc.COUNT_BETAS)
    for nb in range(1, rc.MAX_NB + 1):
        same_count(c.reweight_eval(rc.COUNT_BETAS[:nb]), want[:nb], f"{name} {label} nb = {nb}")


# ------------------------------------------------------------------------------------ 2. the same bits through the gathered merge
def _merge_histories():
    on = np.random.RandomState(3).rand(12288 * 40) < 0.5
    yield "count 12288x40", rc.History(*rc.count_history(rc.COUNT_BY_NAME["12288x40"], on)), rc.COUNT_BETAS
    for rows, T in ((12288, 40), (34304, 3), (777, 9)):
        yield f"realistic {rows}x{T}", rc.realistic(rows, T), rc.ACC_BETAS


@pytest.mark.parametrize("kind", ["loop", "p2p"])
def test_gathered_merge_gives_the_bits_of_the_plain_fold(kind):
    plain, other = ctx(), ctx(kind)
    for where, h, betas in _merge_histories():
        same_bits(load(other, h), load(plain, h), f"{where}: log-mixture")
        for nb in (16, 3, 1):
            want = plain.reweight_eval(betas[:nb])
            same_bits(other.reweight_eval(betas[:nb]), want, f"{where} {kind} nb = {nb}: reweight_eval")
            same_bits(other.reweight_partials(betas[:nb]).cpu().numpy(), want, f"{where} {kind} nb = {nb}: reweight_partials")
            same_bits(plain.reweight_partials(betas[:nb]).cpu().numpy(), want, f"{where} plain nb = {nb}: reweight_partials")


# ---------------------------------------------------------------------------- 3. accuracy over the weight range, derived bounds
@pytest.mark.parametrize("rows,T", rc.ACC_GEOMS)
def test_realistic_histories_within_the_derived_bounds(rows, T):
    h = rc.realistic(rows, T)
    c, g = ctx(), rc.geometry(h.nt)
    C = load(c, h)
    batch = c.reweight_eval(rc.ACC_BETAS)
    # the million-row case: every third beta of the batch (the reference is a long-double pass over the history per beta)
    for i in range(0, rc.MAX_NB, 3 if h.logl.size > 500_000 else 1):
        _, b = check_triple(batch[i], h, C, rc.ACC_BETAS[i], g, rc.MAX_NB, f"{rows}x{T}")
        assert max(b.s1, b.s2, b.logz, b.ess) <= rc.ACC_LIMIT
    for beta in (1.0, 0.37):
        check_triple(c.reweight_eval([beta])[0], h, C, beta, g, 1, f"{rows}x{T}")


def test_the_maximum_is_one_of_its_two_rounded_forms():
    h = rc.exact_case()
    c = ctx()
    C = load(c, h)
    batch = c.reweight_eval(rc.EXACT_BETAS)
    for i, beta in enumerate(rc.EXACT_BETAS):
        fused, unfused = rc.two_forms(beta, h.logl, C)
        one = c.reweight_eval([beta])[0]
        assert one[0] in (fused.max(), unfused.max()), (beta, one[0], fused.max(), unfused.max())
        print(f"4099 beta={beta}: m is the maximum of the {'fused' if one[0] == fused.max() else 'unfused'} form"
              f" (the forms' maxima {'differ' if fused.max() != unfused.max() else 'agree'})")
        assert batch[i][0] == one[0]
        check_triple(one, h, C, beta, rc.geometry(h.nt), 1, "4099")


def test_every_width_gives_the_bits_of_its_unroll_class():
    """Result i of a batch does not depend on the batch's width inside one unroll class (U = 8: nb = 1; 4: 2 .. 4; 2: 5 .. 16) -- the
    same instructions on the same numbers --; across classes the rows meet in another order and the results agree within the sum of
    their bounds."""
    h = rc.realistic(34304, 3)
    c, g = ctx(), rc.geometry(h.nt)
    C = load(c, h)
    by_nb = {nb: c.reweight_eval(rc.ACC_BETAS[:nb]) for nb in range(1, rc.MAX_NB + 1)}
    single = np.array([c.reweight_eval([b])[0] for b in rc.ACC_BETAS])
    same_bits(by_nb[1][0], single[0])
    for u, nbs in rc.U_CLASSES.items():
        widest = by_nb[nbs[-1]]
        for nb in nbs:
            same_bits(by_nb[nb], widest[:nb], f"U = {u}: nb = {nb} against nb = {nbs[-1]}")
    for i in (0, 3, 5):
        check_triple(single[i], h, C, rc.ACC_BETAS[i], g, 1, "34304x3 widths")
        for nb in (4, 16):
            if i < nb:
                check_triple(by_nb[nb][i], h, C, rc.ACC_BETAS[i], g, nb, "34304x3 widths")


@pytest.mark.parametrize("name", sorted(rc.acc_edges()))
def test_edges_of_the_weight_range(name):
    h, betas, _ = rc.acc_edges()[name]
    c, g = ctx(), rc.geometry(h.nt)
    C = load(c, h)
    got = c.reweight_eval(betas)
    same_bits(c.reweight_partials(betas).cpu().numpy(), got)
    for i, beta in enumerate(betas):
        with np.errstate(over="ignore", invalid="ignore"):
            v64 = beta * h.logl - C
        if np.all(v64 == -np.inf):                               # every row v = -inf: what k_reweight_fold documents
            same_bits(got[i], [-np.inf, 0.0, 0.0], f"{name} beta {beta}")
            continue
        ref = rc.acc_reference(h.logl, C, beta)
        if np.isnan(ref.s1):                                     # NaN rows: NaN sums; fmax drops them from the maximum
            assert np.isnan(got[i][1]) and np.isnan(got[i][2]), (name, beta, got[i])
            assert abs(LD(got[i][0]) - ref.m) <= rc.max_bound(h.logl, beta, ref), (name, beta, got[i][0], ref.m)
            continue
        assert np.all(np.isfinite(got[i])), (name, beta, got[i])
        check_triple(got[i], h, C, beta, g, len(betas), name)
        one = c.reweight_eval([beta])[0]
        check_triple(one, h, C, beta, g, 1, name)


# -------------------------------------------------------------------------------------------- 4. K1: the log-mixture, both routes
def _append(c, logl, beta, logz):
    n = logl.size
    z = torch.zeros(1, n, dtype=torch.float64, device="cuda")
    c.history_append(z, z, torch.from_numpy(np.ascontiguousarray(logl)).cuda(), beta, logz)


def check_logmix(got, h, route, where, lo=0, hi=None, entered=None):
    """Rows [lo, hi) of a cached log-mixture against the long-double log-sum-exp, within the per-row bound of the route."""
    hi = h.logl.size if hi is None else hi
    ref = rc.logmix_reference(h.logl[lo:hi], h.bt, h.zt, h.nt)
    part = rc.History(h.logl[lo:hi], h.bt, h.zt, h.nt)
    if entered is None and route == "append":
        entered = np.repeat(np.arange(len(h.bt)), h.nt)[lo:hi]
    bound = rc.logmix_bounds(*part, route, entered=entered)
    got = got[lo:hi]
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=where)
    np.testing.assert_array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)].astype(np.float64), err_msg=where)
    if fin.any():
        frac = (np.abs(got[fin].astype(LD) - ref[fin]) / bound[fin]).astype(np.float64)
        worst = int(np.argmax(frac))
        print(f"{where} {route}: largest error / bound {frac[worst]:.3f} (bound {bound[fin][worst]:.3e})")
        assert frac[worst] <= 1.0, (where, route, np.flatnonzero(fin)[worst] + lo, frac[worst])
        note("K1 " + route, frac[worst], where)


@pytest.mark.parametrize("name", sorted(rc.logmix_cases()))
def test_log_mixture_by_load_and_by_append(name):
    from tempest_amd.device import KEY_LOGMIX
    h = rc.logmix_cases()[name]
    c = ctx()
    check_logmix(load(c, h), h, "load", name)
    c.history_clear()
    off = 0
    for t, n in enumerate(h.nt):
        _append(c, h.logl[off:off + n], h.bt[t], h.zt[t])
        off += n
        if t in (0, len(h.nt) // 2):                            # an early and a middle commit on their own
            upto = rc.History(h.logl[:off], h.bt[:t + 1], h.zt[:t + 1], h.nt[:t + 1])
            check_logmix(c.history_read(KEY_LOGMIX), upto, "append", f"{name} after commit {t}")
    check_logmix(c.history_read(KEY_LOGMIX), h, "append", name)


@pytest.mark.parametrize("size_old,n_new", rc.APPEND_LARGE)
def test_append_at_the_capped_grid(size_old, n_new):
    from tempest_amd.device import KEY_LOGMIX
    h = rc.append_large(size_old, n_new)
    c = ctx()
    first = rc.History(h.logl[:size_old], h.bt[:1], h.zt[:1], h.nt[:1])
    same_bits(load(c, first), np.full(size_old, rc.log_nh(size_old)))        # one term with beta_0 = logZ_0 = 0: C = log n, exactly
    _append(c, h.logl[size_old:], h.bt[1], h.zt[1])
    got = c.history_read(KEY_LOGMIX)
    assert got.size == size_old + n_new
    step = 1 << 20
    for lo in range(0, got.size, step):
        check_logmix(got, h, "append", f"append {size_old} + {n_new}", lo, min(lo + step, got.size))


# -------------------------------------------------------------------------------------------------------------------- 5. K3
@pytest.mark.parametrize("n", rc.SSM_SIZES)
def test_sum_sq_max_is_exact_on_its_lattice(n):
    c = ctx()
    for row in rc.ssm_max_rows(n):
        k, w = rc.ssm_weights(n, row)
        same_bits(c.sum_sq_max(torch.from_numpy(w).cuda()), rc.ssm_expected(k), f"n = {n}, maximum in row {row}")
    same_bits(c.sum_sq_max(torch.zeros(n, dtype=torch.float64, device="cuda")), [0.0, 0.0, 0.0], f"n = {n}, all zero")


def _weights_cases():
    h, _, _ = rc.acc_edges()["spread"]
    return {"spread 777x9": h, "realistic 1064961x1": rc.realistic(1064961, 1)}


@pytest.mark.parametrize("name", sorted(_weights_cases()))
def test_weights_row_by_row_and_their_sum(name):
    h = _weights_cases()[name]
    c, g, beta, n = ctx(), rc.geometry(h.nt), 1.0, h.logl.size
    C = load(c, h)
    m, s1, s2 = c.reweight_eval([beta])[0]
    ref, b = check_triple((m, s1, s2), h, C, beta, g, 1, name)
    w_dev = c.weights(beta, m, s1)
    got = w_dev.cpu().numpy()
    w, v, e = rc.weights_reference(h.logl, C, beta, m, s1)
    rel, ab = rc.weights_bound(h.logl, beta, v, m, w)
    allow = (w * rel + ab).astype(np.float64)
    err = np.abs(got.astype(LD) - w).astype(np.float64)
    worst = int(np.argmax(err / allow))
    print(f"{name}: k_weights largest error / bound {err[worst] / allow[worst]:.3f} in row {worst}")
    assert err[worst] <= allow[worst], (name, worst, got[worst], w[worst])
    note("K3 k_weights", err[worst] / allow[worst], name)
    under = e * (1 + rel) < rc.HALF_STEP                   # the exact quotient rounds to 0
    assert np.all(got[under] == 0.0) and (name != "spread 777x9" or under.any())
    # (sum w, sum w^2, max w): k_sum_sq_max against the device's own weights, then the sum against 1
    s = c.sum_sq_max(w_dev)
    adds = rc.ssm_additions(n) * rc.U / (1 - rc.ssm_additions(n) * rc.U)
    exact1, exact2 = np.sum(got.astype(LD)), np.sum(got.astype(LD) ** 2)
    assert abs(LD(s[0]) - exact1) <= adds * exact1 and abs(LD(s[1]) - exact2) <= (adds + rc.U) * exact2 and s[2] == got.max()
    note("K3 k_sum_sq_max", float(abs(LD(s[0]) - exact1) / (adds * exact1)), name)
    total = b.s1 / (1 - b.s1) + float(np.sum(allow.astype(LD))) + adds * float(exact1)
    print(f"{name}: sum w - 1 = {s[0] - 1.0:.3e}, bound {total:.3e}")
    assert abs(s[0] - 1.0) <= total
    note("K3 sum of weights", abs(s[0] - 1.0) / total, name)


def test_logw_is_one_of_its_two_rounded_forms():
    h = rc.exact_case()
    c = ctx()
    C = load(c, h)
    sub = C - rc.log_nh(h.logl.size)                             # the kernel's cmix - lognh: one rounding
    for beta in rc.EXACT_BETAS:
        got = c.logw(beta).cpu().numpy()
        fused, unfused = rc.two_forms(beta, h.logl, sub)
        assert np.array_equal(rc.bits(got), rc.bits(fused)) or np.array_equal(rc.bits(got), rc.bits(unfused)), \
            (beta, int((got != fused).sum()), int((got != unfused).sum()))
        print(f"k_logw beta={beta}: the {'fused' if np.array_equal(got, fused) else 'unfused'} form; the forms differ in "
              f"{int((fused != unfused).sum())} of {got.size} rows")
        same_bits(c.logw(beta, n_h_global=3 * h.logl.size).cpu().numpy(),
                  rc.two_forms(beta, h.logl, C - rc.log_nh(3 * h.logl.size))[int(not np.array_equal(got, fused))])
