"""k_propose_reg, the proposal kernel of every run with n_dim <= 16 (tempest_amd/csrc/mutate.hip), instantiation by
instantiation and launch shape by launch shape, against oracle/mcmc.py: propose (NumPy FP64 on the shared Philox stream).
Run on the GPU box:  python -m pytest tests/test_propose_reg_gpu.py -m gpu

What launch_propose_reg can launch, and the test that reaches it:
  <KERNEL, D, true, 2, false>   one mode, no boundary conditions, interleaved Box-Muller chains (the benchmark's kernel):
                                 every D in test_every_dimension_vs_oracle[one-none]
  <TPCN, D, true, 4, false>     the rolled one-mode form, D = 12 ... 16 beyond two waves per SIMD: test_rolled_form_* (D = 12, 13,
                                 16), and D = 7, 13 through TPH_OPT_REDRAW_LANES in test_tiles_per_wave_option_*
  <.., true, 4, true>           one mode with periodic / reflective coordinates: test_every_dimension_vs_oracle[one-mixed]
  <.., false, 4, false | true>  several modes: test_every_dimension_vs_oracle[three-*]
  several tiles per wave, the last wave short of one, the ntiles > waves * REG_MAX_TILES branch: test_launch_geometry_*
  the redraw cap: test_redraw_cap_*;  pending moves and the carried form: test_one_mode_*;  ld > n: test_leading_dimension_*

Tolerances are those of test_propose_accept_adapt_vs_oracle: u' rtol 1e-11 / atol 1e-13, form at u rtol 1e-10, form at u' rtol
1e-9 / atol 1e-9.  "Bitwise" is torch.equal.  The input recipes live in tests/propose_reg_cases.py; tests/test_host_logic.py
checks with the oracle alone that they redraw as much as these tests need.

Every call through `propose_padded` gives the kernel buffers of leading dimension n + GUARD: the columns past n hold a
sentinel (NaN in u) and are checked after the call -- the last 64-row tile is where a kernel of this shape writes out of range.
The calls through HipContext.propose (ld = n) carry their guard behind the last coordinate's row."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import propose_reg_cases as pc  # noqa: E402
from tests.test_kernels_gpu import _Modes, aos, soa  # noqa: E402
from tempest_amd.device import OPT_PROPOSE_VARIANT as OPT_VARIANT  # noqa: E402
from tempest_amd.device import OPT_REDRAW_LANES  # noqa: E402

GUARD, SENT = 128, 1e300
SLICE = 2048                                  # rows of one oracle comparison inside a large launch


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctxs(dev):
    """One HipContext per dimension for the whole module."""
    from tempest_amd.device import HipContext
    made = {}

    def get(d):
        if d not in made:
            made[d] = HipContext(d, 0, 0)
        c = made[d]
        c.set_option(OPT_VARIANT, 0)
        c.set_option(OPT_REDRAW_LANES, 0)
        return c
    yield get
    for c in made.values():
        c.close()


def n_simd():
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


class _Inputs:
    """An ensemble of tests/propose_reg_cases.py on the device.  One mode: no assignment array (the ONE_MODE instantiations);
    no boundary conditions: no flag array (the HAS_BC = false instantiations)."""

    def __init__(self, e, flags, dev):
        self.e, self.flags = e, flags
        self.d, self.n, self.K, self.kernel = e["d"], e["n"], e["K"], e["kernel"]
        self.modes = _Modes(e["means"], e["chol"], e["inv"], e["dof"], dev)
        self.u = soa(e["u"], dev)
        self.assign = torch.from_numpy(e["assign"]).to(dev) if self.K > 1 else None
        self.sigmas = torch.from_numpy(e["sigmas"]).to(dev)
        self.bc = torch.from_numpy(flags).to(dev) if flags.any() else None


def propose_padded(c, x, pad=GUARD, variant=0, lanes=0, seed=pc.SEED, tick=pc.TICK, item0=pc.ITEM0):
    """tph_propose through the C ABI with buffers of leading dimension n + pad; checks the guard columns and that u is
    untouched; returns contiguous (u' (d, n), form at u (n), form at u' (n)) on the device."""
    from tempest_amd._lib import check
    from tempest_amd.device import KERNEL_ID
    d, n = x.d, x.n
    ld = n + pad
    dev = x.u.device
    u = torch.full((d, ld), float("nan"), dtype=torch.float64, device=dev)
    u[:, :n] = x.u
    up = torch.full((d, ld), SENT, dtype=torch.float64, device=dev)
    mu_ = torch.full((ld,), SENT, dtype=torch.float64, device=dev)
    mup = torch.full((ld,), SENT, dtype=torch.float64, device=dev)
    c.set_option(OPT_VARIANT, variant)
    c.set_option(OPT_REDRAW_LANES, lanes)
    m = x.modes
    check(c.lib.tph_propose(c._ctx, KERNEL_ID[x.kernel], u.data_ptr(), x.assign.data_ptr() if x.assign is not None else None,
                            n, ld, m.K, m.means_dev.data_ptr(), m.chol_dev.data_ptr(), None, m.dof_dev.data_ptr(),
                            x.sigmas.data_ptr(), x.bc.data_ptr() if x.bc is not None else None, seed, tick, item0,
                            up.data_ptr(), mu_.data_ptr(), mup.data_ptr(), None, None), "tph_propose")
    torch.cuda.synchronize()
    c.set_option(OPT_VARIANT, 0)
    c.set_option(OPT_REDRAW_LANES, 0)
    assert bool((up[:, n:] == SENT).all()), "u' written past n"
    assert bool((mu_[n:] == SENT).all()) and bool((mup[n:] == SENT).all()), "a form written past n"
    assert bool(torch.isnan(u[:, n:]).all()), "u written past n"
    assert torch.equal(u[:, :n], x.u), "u changed without a pending move"
    return up[:, :n].contiguous(), mu_[:n].clone(), mup[:n].clone()


def propose_tight(c, x, a=0, b=None, variant=0, seed=pc.SEED, tick=pc.TICK, item0=pc.ITEM0):
    """HipContext.propose (ld = n) on the rows [a, b) as an ensemble of their own (items item0 + a ...); the guard follows the
    last coordinate's row."""
    d = x.d
    b = x.n if b is None else b
    m = b - a
    dev = x.u.device
    flat = torch.full((d * m + GUARD,), SENT, dtype=torch.float64, device=dev)
    f1 = torch.full((m + GUARD,), SENT, dtype=torch.float64, device=dev)
    f2 = torch.full((m + GUARD,), SENT, dtype=torch.float64, device=dev)
    up, mu_, mup = flat[:d * m].view(d, m), f1[:m], f2[:m]
    u = x.u[:, a:b].contiguous()
    at = x.assign[a:b].contiguous() if x.assign is not None else None
    c.set_option(OPT_VARIANT, variant)
    c.set_option(OPT_REDRAW_LANES, 0)
    c.propose(x.kernel, u, at, x.modes, x.sigmas, x.bc, seed, tick, item0 + a, up, mu_, mup)
    torch.cuda.synchronize()
    c.set_option(OPT_VARIANT, 0)
    assert bool((flat[d * m:] == SENT).all()) and bool((f1[m:] == SENT).all()) and bool((f2[m:] == SENT).all())
    assert torch.equal(u, x.u[:, a:b])
    return up, mu_, mup


def propose_chunks(c, x, **kw):
    """The reference launch shape: the same rows in contiguous chunks of at most 65 536 (one tile per wave, at most two waves
    per SIMD: the interleaved one-mode form where there is a choice)."""
    chunk = min(65536, 128 * n_simd())
    assert pc.launch_geometry(chunk, n_simd())[1] == 1 and not pc.rolled_form(x.kernel, x.d, chunk, n_simd())
    parts = [propose_tight(c, x, a, min(x.n, a + chunk), **kw) for a in range(0, x.n, chunk)]
    return torch.cat([p[0] for p in parts], dim=1), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts])


def assert_bitwise(got, ref, what):
    for name, g, r in zip(("u'", "form at u", "form at u'"), got, ref):
        if not torch.equal(g, r):
            rows = torch.nonzero((g != r).reshape(-1, g.shape[-1]).any(dim=0)).flatten()
            raise AssertionError(f"{what}: {name} differs in {rows.numel()} rows, first {rows[:8].tolist()}")


def assert_vs_oracle(x, got, a=0, b=None):
    """rows [a, b) of a device result against omc.propose at the project's tolerances"""
    b = x.n if b is None else b
    a = max(0, a)
    want_up, want_mu, want_mup = pc.oracle(x.e, x.flags, a, b)
    got_up = aos(got[0][:, a:b])
    np.testing.assert_allclose(got_up, want_up, rtol=1e-11, atol=1e-13)
    strict = np.nonzero(x.flags == 0)[0]
    assert np.all((got_up[:, strict] >= 0) & (got_up[:, strict] <= 1))
    assert np.all((got_up >= 0) & (got_up <= 1))
    mu_, mup = got[1][a:b].cpu().numpy(), got[2][a:b].cpu().numpy()
    if x.kernel == "tpcn":
        np.testing.assert_allclose(mu_, want_mu, rtol=1e-10)
        np.testing.assert_allclose(mup, want_mup, rtol=1e-9, atol=1e-9)
    else:                                                # RWM: both forms are written as zeros
        np.testing.assert_array_equal(mu_, want_mu)
        np.testing.assert_array_equal(mup, want_mup)
    return want_up


# ------------------------------------------------------------- 1. every dimension, every instantiation, small n
_D_BC = [(d, bc) for d in pc.DIMS for bc in ((None, "mixed", "mixed_reflective") if d == 1 else (None, "mixed"))]


@pytest.mark.parametrize("kernel", ["tpcn", "rwm"])
@pytest.mark.parametrize("modes", ["one", "three"])
@pytest.mark.parametrize("d,bc", _D_BC, ids=[f"d{d}-{bc or 'none'}" for d, bc in _D_BC])
def test_every_dimension_vs_oracle(dev, ctxs, kernel, modes, d, bc):
    """64 full tiles and a tile of one row.  TPH_OPT_PROPOSE_VARIANT 0 (leading dimension n + 128) and 2 (ld = n) must both take
    the register kernel: bitwise the same outputs, and those equal to the oracle's."""
    n = 4097
    e = pc.ensemble(d, kernel, 1 if modes == "one" else 3, n)
    x = _Inputs(e, pc.flags_for(d, bc, which=1 if bc == "mixed_reflective" else 0), dev)
    c = ctxs(d)
    got = propose_padded(c, x, variant=0)
    assert_vs_oracle(x, got)
    assert_bitwise(propose_tight(c, x, variant=2), got, "variant 2 against variant 0")


# ------------------------------------------------------------- 2. rolled form == interleaved form
def _large_against_chunks(dev, ctxs, kernel, d, K, bc, n, marks):
    """One launch of n rows (guarded buffers) bitwise equal to the same rows in chunks, then the oracle on SLICE rows around
    each of `marks` (row indices; clipped to [0, n))."""
    x = _Inputs(pc.ensemble(d, kernel, K, n), pc.flags_for(d, bc), dev)
    c = ctxs(d)
    got = propose_padded(c, x)
    assert_bitwise(got, propose_chunks(c, x), f"{kernel} d={d} n={n}: one launch against chunks")
    for m in marks:
        a = min(max(0, m - SLICE // 2), n - SLICE)
        assert_vs_oracle(x, got, a, a + SLICE)


@pytest.mark.parametrize("d", [12, 13, 16])
def test_rolled_form_equals_interleaved_form(dev, ctxs, d):
    """tpCN, one mode, no boundary conditions, just past two waves per SIMD: one launch takes the rolled instantiation
    <TPCN, d, true, 4, false>, chunks of 65 536 rows the interleaved <TPCN, d, true, 2, false>.  A run sharded over G GPUs picks
    the form from its shard's row count, so the world-size invariance promised at d <= 16 needs these to be the same function,
    bit for bit."""
    n = 128 * n_simd() + 64 * 3 + 1
    waves, tiles = pc.launch_geometry(n, n_simd())
    assert tiles == 1 and pc.rolled_form("tpcn", d, n, n_simd())
    _large_against_chunks(dev, ctxs, "tpcn", d, 1, None, n, [0, n // 2, n])


# ------------------------------------------------------------- 3. launch geometry does not change a proposal
@pytest.mark.parametrize("kernel,d,K,bc", [("tpcn", 10, 1, None), ("rwm", 10, 1, None), ("tpcn", 16, 1, None), ("rwm", 5, 3, "mixed")],
                         ids=["tpcn-d10-one", "rwm-d10-one", "tpcn-d16-one-rolled", "rwm-d5-three-mixed"])
def test_launch_geometry_two_tiles_per_wave(dev, ctxs, kernel, d, K, bc):
    """One resident batch and 4 097 rows more: every wave owns the tiles w and w + waves, the last wave a single one."""
    n = 256 * n_simd() + 4097
    waves, tiles = pc.launch_geometry(n, n_simd())
    assert tiles == 2 and waves * tiles == (n + 63) // 64 + 1
    _large_against_chunks(dev, ctxs, kernel, d, K, bc, n, [0, waves * 64, n])


def test_launch_geometry_more_tiles_than_a_resident_batch_holds(dev, ctxs):
    """ntiles > waves * REG_MAX_TILES: eight tiles per wave and more waves than one resident batch."""
    n = 8 * 256 * n_simd() + 64 * 5 + 3
    waves, tiles = pc.launch_geometry(n, n_simd())
    assert tiles == pc.REG_MAX_TILES and waves > 4 * n_simd()
    _large_against_chunks(dev, ctxs, "rwm", 2, 1, None, n, [0, waves * 64, (tiles - 1) * waves * 64, n])


@pytest.mark.parametrize("d", [7, 13])
def test_tiles_per_wave_option_does_not_change_a_proposal(dev, ctxs, d):
    """TPH_OPT_REDRAW_LANES = 1, 3, 8 tiles per wave against the automatic launch.  The option also selects the rolled one-mode
    instantiation, the automatic launch of 20 000 rows the interleaved one: a second check of their equality."""
    x = _Inputs(pc.ensemble(d, "tpcn", 1, 20_000), pc.flags_for(d, None), dev)
    c = ctxs(d)
    auto = propose_padded(c, x)
    assert_vs_oracle(x, auto, x.n - SLICE, x.n)
    for lanes in (1, 3, 8):
        assert_bitwise(propose_padded(c, x, lanes=lanes), auto, f"d={d}: {lanes} tiles per wave against the automatic launch")


# ------------------------------------------------------------- 4. the redraw cap
@pytest.mark.parametrize("d", [1, 7, 16])
def test_redraw_cap_every_attempt_out_proposes_the_current_point(dev, ctxs, d):
    """RWM with a step far too large (as test_stage_machine_redraw_cap_proposes_the_current_point): all 256 attempts leave the
    cube and u' is u, bit for bit."""
    x = _Inputs(pc.runaway_ensemble(d), pc.flags_for(d, None), dev)
    up, mu_, mup = propose_padded(ctxs(d), x)
    assert torch.equal(up, x.u)
    assert not bool(mu_.any()) and not bool(mup.any())


@pytest.mark.parametrize("kernel", ["tpcn", "rwm"])
@pytest.mark.parametrize("d", pc.CAP_DIMS)
def test_redraw_cap_mixed_ensemble(dev, ctxs, kernel, d):
    """10-90 % of the walkers fail all 256 attempts (tests/test_host_logic.py checks that share), the others win at attempts
    spread over 1 ... 255: the rounds with G lanes per walker step over the cap (a0 + G past 256)."""
    e = pc.cap_ensemble(d, kernel)
    x = _Inputs(e, pc.flags_for(d, None), dev)
    got = propose_padded(ctxs(d), x)
    want_up = assert_vs_oracle(x, got)
    capped = pc.cap_rows(e, want_up)
    assert 0.10 <= capped.mean() <= 0.90
    if kernel == "rwm":
        got_capped = (got[0] == x.u).all(dim=0).cpu().numpy()
        np.testing.assert_array_equal(got_capped, capped)
        ct = torch.from_numpy(capped).to(dev)
        assert torch.equal(got[0][:, ct], x.u[:, ct])


# ------------------------------------------------------------- 5. deferred update and carried form, one mode
_CHAIN = [(k, d, 6000) for k in ("tpcn", "rwm") for d in (1, 10, 13, 16)] + [("tpcn", 13, None)]


def _like(up):
    z = 20 * up - 10
    return -0.5 * (z * z).sum(dim=0) * (0.05 if up.shape[0] > 1 else 1.0)    # one coordinate: sharper, or nearly every move is accepted


@pytest.mark.parametrize("kernel,d,n", _CHAIN, ids=[f"{k}-d{d}-{n or 'rolled'}" for k, d, n in _CHAIN])
def test_one_mode_deferred_metropolis_update_equals_in_place(dev, ctxs, kernel, d, n):
    """test_deferred_metropolis_update_equals_in_place on the one-mode instantiation (no assignments, K = 1, variant 0): four
    steps, the chain with pending moves resolved by the next proposal is the in-place chain bit for bit.  n = None: just past
    two waves per SIMD, where tpCN at d = 13 takes the rolled form."""
    if n is None:
        n = 128 * n_simd() + 1000
        assert pc.rolled_form(kernel, d, n, n_simd())
    x = _Inputs(pc.ensemble(d, kernel, 1, n), pc.flags_for(d, None), dev)
    c = ctxs(d)

    def chain(deferred):
        u = x.u.clone()
        logl = _like(u).clone()
        up, mu_, mup = c.empty(d, n), c.empty(n), c.empty(n)
        sums = c.empty(2)
        pend = torch.zeros(n, dtype=torch.uint8, device=dev) if deferred else None
        trace = []
        for step in range(4):
            tick = 50 + 2 * step
            c.propose(kernel, u, None, x.modes, x.sigmas, None, 99, tick, 7, up, mu_, mup, pending=pend)
            lp = _like(up)
            c.accept(kernel, 0.8, u, None, logl, up, None, lp, mu_, mup, None, 1, x.modes.dof_dev, 99, tick + 1, 7, sums, pending=pend)
            trace.append((up.clone(), logl.clone(), mu_.clone(), sums.clone()))
        if deferred:
            assert int(pend.sum().item()) > 0                 # moves are waiting
            c.propose(kernel, u, None, x.modes, x.sigmas, None, 99, 999, 7, up, mu_, mup, pending=pend)
            assert int(pend.sum().item()) == 0
        return u, trace
    ua, ta = chain(False)
    ub, tb = chain(True)
    for a, b in zip(ta, tb):
        for p, q in zip(a, b):
            assert torch.equal(p, q)
    assert torch.equal(ua, ub)
    assert 0.02 < float(ta[-1][3][0]) / n < 0.98            # a real mix: hundreds of rows to move, hundreds to leave alone


@pytest.mark.parametrize("kernel,d,n", _CHAIN, ids=[f"{k}-d{d}-{n or 'rolled'}" for k, d, n in _CHAIN])
def test_one_mode_control_block_and_carried_form(dev, ctxs, kernel, d, n):
    """As test_step_control_block_semantics does at d = 5: with steps done in the control block (ctl[0] > 0) the kernel reads the
    form at u from maha_u and proposes, bit for bit, what recomputing it proposes; tick = tick + ctl[7] + 2 ctl[0]."""
    if n is None:
        n = 128 * n_simd() + 1000
    x = _Inputs(pc.ensemble(d, kernel, 1, n), pc.flags_for(d, None), dev)
    c = ctxs(d)
    seed, base, done_steps = 1234, 100, 3

    def propose(tick, ctl, maha_u=None):
        up, mu_, mup = c.empty(d, n), (c.empty(n) if maha_u is None else maha_u.clone()), c.empty(n)
        c.propose(kernel, x.u, None, x.modes, x.sigmas, None, seed, tick, 0, up, mu_, mup, ctl=ctl)
        return up, mu_, mup
    ctl = torch.tensor([done_steps, 0, 0, 0, 0, 0, 0.37, base, 0, 0], dtype=torch.float64, device=dev)   # TPH_STEP_STATE_LEN
    b = propose(1 + base + 2 * done_steps, None)
    a = propose(1, ctl, maha_u=b[1])
    assert_bitwise(a, b, "carried form against recomputed")
    ctl0 = ctl.clone()
    ctl0[0] = 0.0
    wrong = b[1] * 4.0 + 1.0
    assert_bitwise(propose(1, ctl0, maha_u=wrong), propose(1 + base, None), "step 0 computes the form whatever the buffer holds")
    if kernel == "tpcn":                              # the carried value really is read: a wrong one changes the proposals
        assert not torch.equal(propose(1, ctl, maha_u=wrong)[0], b[0])


# ------------------------------------------------------------- 6. ld > n through the C ABI
@pytest.mark.parametrize("modes", ["one", "three"])
@pytest.mark.parametrize("d", [3, 12])
def test_leading_dimension_larger_than_n(dev, ctxs, d, modes):
    """tph_propose requires ld >= n; HipContext.propose always passes ld = n.  With ld = n + 37 the rows < n are those of the
    ld = n call and the columns >= n of u', of both forms and of u stay untouched (propose_padded checks them)."""
    x = _Inputs(pc.ensemble(d, "tpcn", 1 if modes == "one" else 3, 4097), pc.flags_for(d, None), dev)
    c = ctxs(d)
    assert_bitwise(propose_padded(c, x, pad=37), propose_tight(c, x), f"d={d} {modes}: ld = n + 37 against ld = n")
