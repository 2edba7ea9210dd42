"""Host-side logic that needs neither a GPU nor the HIP library: checkpoint metadata encoding, format selection, the
detection of a fusable HipCallbacks pair, the size buckets of history-sized temporaries."""
import numpy as np
import pytest


def test_checkpoint_scalar_encoding_roundtrip():
    from tempest_amd import checkpoint as ck
    vals = [None, True, 3, np.int64(7), 2.5, np.float64(-1e300), float("inf"), np.array([1.0, 2.0]), np.array([[1, 2], [3, 4]])]
    for v in vals:
        enc = ck._json_scalar(v)
        dec = ck._from_json_scalar(enc)
        if isinstance(v, np.ndarray):
            np.testing.assert_array_equal(dec, v)
            assert dec.dtype == v.dtype
        else:
            assert dec == v or (v is None and dec is None)
    with pytest.raises(TypeError):
        ck._json_scalar(object())


def test_checkpoint_format_selection(tmp_path):
    from tempest_amd import checkpoint as ck
    assert ck.wants_native(tmp_path / "a.ckpt") and not ck.wants_native(tmp_path / "a.state")
    assert ck.wants_native(tmp_path / "a.state", "native") and not ck.wants_native(tmp_path / "a.ckpt", "dill")
    # a checkpoint caught between the two renames of save() exists as `<name>.old` only: still found
    assert not ck.is_native(tmp_path / "run.ckpt")
    (tmp_path / "run.ckpt.old").mkdir()
    (tmp_path / "run.ckpt.old" / "meta.json").write_text("{}")
    assert ck.is_native(tmp_path / "run.ckpt") and ck._resolve(tmp_path / "run.ckpt").name == "run.ckpt.old"
    (tmp_path / "run.ckpt").mkdir()
    (tmp_path / "run.ckpt" / "meta.json").write_text("{}")
    assert ck._resolve(tmp_path / "run.ckpt").name == "run.ckpt"
    with pytest.raises(ValueError):
        ck.wants_native(tmp_path / "a", "hdf5")
    (tmp_path / "d").mkdir()
    assert ck.wants_native(tmp_path / "d") and not ck.is_native(tmp_path / "d")
    (tmp_path / "d" / "meta.json").write_text("{}")
    assert ck.is_native(tmp_path / "d")

    class FakeComm:
        active = True
    assert ck.wants_native(tmp_path / "x.state", None, FakeComm())       # sharded runs never write one pickle per rank


def test_fused_plugin_detection():
    from tempest_amd.hipcallbacks import HipCallbacks, fused_plugin

    def f(x):
        return x
    assert fused_plugin(f, f) is None
    a = HipCallbacks.__new__(HipCallbacks)
    a.fused, a.whole_step, a.n_dim = True, True, 10
    b = HipCallbacks.__new__(HipCallbacks)
    b.fused, b.whole_step, b.n_dim = True, True, 10
    assert fused_plugin(a.prior_transform, a.log_likelihood) is a
    assert fused_plugin(a.prior_transform, b.log_likelihood) is None     # two different plugins: nothing to fuse
    a.fused = False
    assert fused_plugin(a.prior_transform, a.log_likelihood) is None
    a.fused = True
    assert a.can_fuse_step(1, False, 131072) and not a.can_fuse_step(1, False, 1 << 20)
    assert not a.can_fuse_step(3, True, 1000)
    a.whole_step = "always"
    assert a.can_fuse_step(1, False, 1 << 20)
    a.n_dim = 17
    assert not a.can_fuse_step(1, False, 1000)


def test_history_sized_temporaries_come_from_buckets():
    # the rule of HipContext.empty_rows: capacity = the smallest of {2^k, 1.5 * 2^k} >= n (at least 1024)
    def bucket(n):
        p2 = 1 << max(10, (n - 1).bit_length())
        return p2 * 3 // 4 if p2 * 3 // 4 >= n else p2
    for n in (1, 1024, 1025, 1536, 1537, 2048, 3000, 3073, 10 ** 6, 25 * 10 ** 6):
        c = bucket(n)
        assert c >= n and c <= max(1024, int(1.5 * n) + 1)
        assert c & (c - 1) == 0 or (c // 3) & ((c // 3) - 1) == 0
    import inspect
    from tempest_amd.device import HipContext
    src = inspect.getsource(HipContext.empty_rows)
    assert "bit_length" in src and "3 // 4" in src


class _Rule:
    """The regime rule alone: Regime.next over the readings of one engine shape.  `fresh`: every reading as if the last switch were
    long ago (the thresholds without the dwell)."""

    def __init__(self, d, n, K=1, opts=None, fresh=False):
        from tempest_amd.regime import Regime, RegimeOptions
        self.shape = dict(n_dim=d, n=n, K=K, opts=opts or RegimeOptions())
        self.regime, self.fresh = Regime(), fresh

    def read(self, mean_attempts, captured=False):
        if self.fresh:
            self.regime = self.regime._replace(since=1 << 30, dwell=0, quick=0)
        self.regime = self.regime.next(mean_attempts, captured=captured, **self.shape)

    blocked, staged, unstaged = (property(lambda self, f=f: getattr(self.regime, f)) for f in ("blocked", "staged", "unstaged"))


def _engine(d, n, K=1, opts=None, fresh=False):
    """What is the engine's of a reading: the regime's options in the context and the retirement of a captured graph."""
    from tempest_amd import mcmc

    class Ctx:
        n_dim = d

        def __init__(self):
            self.opts = {}

        def set_option(self, k, v):
            self.opts[k] = v

    class Eng(mcmc.StepEngine):
        def __init__(self):
            self.ctx, self.n, self.K, self.graph, self._keep, self._retired_graphs = Ctx(), n, K, None, None, []
            self._opts, self.regime = opts or mcmc.RegimeOptions(), mcmc.Regime()

        def _regime(self, m):
            if fresh:
                self.regime = self.regime._replace(since=1 << 30, dwell=0, quick=0)
            mcmc.StepEngine._regime(self, m)
    return Eng()


def test_proposal_regime_rule_d_gt_16():
    """(With the screen off, TEMPEST_AMD_SCREEN=0: the FP64 row walker's crossovers; the screened rule: second half.)
    Regime.next (regime.py): which d > 16 proposal kernel the NEXT steps get from the redraw probe -- blocked kernel in
    R rounds for a few attempts per particle (R from the expected length of the round's list), row walker when redraws
    dominate, one threshold per direction (the blocked path reports the geometric estimate, the walker the true mean), the
    multi-lane kernel for several modes; StepEngine._regime puts the regime into the context, and a captured graph keeps what it
    was captured with until the rule asks for another kernel.  (Every reading as if the last switch were long ago; the dwell:
    next test.)"""
    from tempest_amd import mcmc
    from tempest_amd.device import OPT_BLOCKED, OPT_ML_UNSTAGED, OPT_SCREEN, OPT_STAGED_REDRAW
    off = mcmc.RegimeOptions.from_env({"TEMPEST_AMD_SCREEN": "0"})
    assert not off.screen and mcmc.RegimeOptions.from_env({}).screen

    e = _engine(50, 65536, opts=off, fresh=True)
    e._regime(60.0)                                   # first steps of a run from the prior: redraws dominate
    assert e.staged and e.blocked == 0 and e.ctx.opts[OPT_STAGED_REDRAW] == 1 and e.ctx.opts.get(OPT_BLOCKED, 0) == 0
    e._regime(6.0)                                    # the walker's probe is the TRUE mean: it keeps the step down to 5
    assert e.staged and e.blocked == 0
    e._regime(4.0)
    assert not e.staged and e.blocked >= 1 and e.ctx.opts[OPT_STAGED_REDRAW] == 0
    assert e.blocked == 4 and e.ctx.opts[OPT_BLOCKED] == 4     # expected lists 49 152, 36 864, 27 648 >= 24 576 > 20 736
    e._regime(3.4)                                    # the blocked path's probe is the geometric estimate: stays up to 3.5
    assert not e.staged and e.blocked >= 1
    e._regime(3.6)
    assert e.staged and e.blocked == 0
    e._regime(1.0)
    assert not e.staged and e.blocked == 1            # (nearly) every first attempt in bounds: one round
    g = e.graph = object()
    e._regime(1.3)                                    # a captured graph keeps its kernel, rounds included ...
    assert e.graph is g and not e.staged and e.blocked == 1 and not e._retired_graphs
    e._regime(90.0)                                   # ... until the rule asks for ANOTHER kernel: retired, captured again later
    assert e.graph is None and e.staged and e.blocked == 0 and e._retired_graphs[0][0] is g
    e.graph = g
    e._regime(60.0)
    assert e.graph is g and len(e._retired_graphs) == 1
    # many particles: rounds while the expected list fills the chip, at most 24
    big = _engine(32, 262144, opts=off, fresh=True)
    big._regime(2.27)
    assert big.blocked == 5 and big.ctx.opts[OPT_BLOCKED] == 5
    big.regime = big.regime._replace(blocked=1)
    big._regime(3.4)
    assert 5 < big.blocked <= 24
    # n_dim >= 64: the crossovers sit higher (estimate 4.5, true mean 8)
    wide = _Rule(100, 131072, opts=off, fresh=True)
    wide.read(7.0)
    assert wide.blocked >= 1 and not wide.staged
    wide.read(4.4)
    assert wide.blocked >= 1
    wide.read(4.6)
    assert wide.staged and wide.blocked == 0
    wide.read(8.5)
    assert wide.staged
    wide.read(7.9)
    assert wide.blocked >= 1 and not wide.staged
    # several modes: neither; the multi-lane kernel, un-staged while redraws dominate (hysteresis 8 / 4)
    k4 = _engine(32, 262144, K=4, opts=off, fresh=True)
    k4._regime(20.0)
    assert k4.blocked == 0 and not k4.staged and k4.unstaged and k4.ctx.opts[OPT_ML_UNSTAGED] == 1
    k4._regime(5.0)
    assert k4.unstaged
    k4._regime(3.0)
    assert not k4.unstaged
    # d <= 16 has one kernel
    small = _engine(10, 1 << 20, opts=off, fresh=True)
    small._regime(3.0)
    assert small.ctx.opts == {}
    # ---- with the screened batches (default): their time is flat in the attempt count, so the crossovers sit lower at high
    # n_dim and higher at 32-D (tools/regime_sweep.py), and the blocked kernel runs more, shorter rounds (the straggler pass is
    # a screened launch over the list)
    s100 = _engine(100, 131072, fresh=True)
    s100._regime(60.0)
    assert s100.staged and s100.blocked == 0 and s100.ctx.opts[OPT_SCREEN] == 1
    s100._regime(5.1)
    assert s100.staged
    s100._regime(4.9)                                 # true mean below 5: blocked rounds
    assert not s100.staged and 1 <= s100.blocked <= 6
    s100._regime(2.9)                                 # now the geometric estimate: stays up to 3
    assert not s100.staged and s100.blocked == 6
    s100._regime(3.1)
    assert s100.staged and s100.blocked == 0
    s50 = _Rule(50, 65536, fresh=True)                # 33..63-D, with the list rounds fanned out: estimate 3.4 / true mean 5.5
    s50.read(30.0)
    assert s50.staged and s50.blocked == 0
    s50.read(5.6)
    assert s50.staged
    s50.read(5.4)
    assert not s50.staged and 2 <= s50.blocked <= 8
    s50.read(3.3)
    assert not s50.staged and s50.blocked >= 2
    s50.read(3.5)
    assert s50.staged and s50.blocked == 0
    s50.read(1.3)                                     # one try per round above 32-D; a fanned-out second round empties the list
    assert not s50.staged and 2 <= s50.blocked <= 4
    s32 = _Rule(32, 262144, fresh=True)
    s32.read(14.0)
    assert s32.staged
    s32.read(12.0)                                    # 32-D: the screened batches only win above ~13 attempts per particle
    assert not s32.staged and s32.blocked == 12
    s32.read(1.05)                                    # two attempts per round in place: lists 594, 1: two rounds
    assert s32.blocked == 2
    s32.read(8.1)
    assert s32.staged
    # several modes: the matrix-core rounds over mode-pure tiles below ~8 estimated attempts, the screened batches mode by mode
    # above (round 5; the multi-lane kernel only with the screen off: first half)
    m4 = _Rule(32, 262144, K=4, fresh=True)
    m4.read(20.0)
    assert m4.blocked == 0 and m4.staged
    m4.read(12.0)
    assert m4.blocked == 12 and not m4.staged
    m4.read(1.2)
    assert 2 <= m4.blocked <= 4 and not m4.staged
    m4.read(8.5)
    assert m4.blocked == 0 and m4.staged
    m80 = _Rule(32, 262144, K=80, fresh=True)          # more modes than the mode tables hold: the multi-lane kernel
    m80.read(20.0)
    assert m80.blocked == 0 and not m80.staged and m80.unstaged


def test_regime_rule_does_not_oscillate(monkeypatch):
    """a redraw probe that sits on a threshold of the regime rule and crosses it at every reading (the blocked
    rounds report the geometric estimate, the screened batches the true mean: 3.1 >= 3.0 sends the step to the batches, whose 4.9 <
    5.0 sends it back) must not retire and re-capture the step's graph at every step: after two free switches the next ones wait
    4, 8, ... 64 readings.  Each threshold crossed ONCE, in either direction, switches at once; the debugging switches are read
    when the engine is built, not per step."""
    from tempest_amd import mcmc
    for var in ("TEMPEST_AMD_SCREEN", "TEMPEST_AMD_STAGED", "TEMPEST_AMD_BLK_MFMA", "TEMPEST_AMD_BLK_FAN", "TEMPEST_AMD_SM_LANES"):
        monkeypatch.delenv(var, raising=False)
    opts = mcmc.RegimeOptions.from_env()

    for d, n in ((100, 131072), (50, 65536), (32, 262144)):
        up, down, _, _ = mcmc.regime_band("screened", d)
        # one crossing each way switches immediately, in both directions, at exactly the tabulated numbers
        r = _Rule(d, n, opts=opts)
        r.read(60.0)
        assert r.staged and not r.blocked
        r.read(down + 0.01)
        assert r.staged
        r.read(down - 0.01)
        assert r.blocked >= 1 and not r.staged
        r.read(up - 0.01)
        assert r.blocked >= 1
        r.read(up + 0.01)
        assert r.staged and not r.blocked
        # the probe flips at every reading: count the kernel switches (= graph retirements) over 400 readings
        e = _engine(d, n, opts=opts)
        e._regime(60.0)
        switches, kinds = 0, []
        for _ in range(400):
            e.graph = object()                     # the step has been captured again since the last reading
            was = (e.blocked > 0, e.staged)
            e._regime(down - 0.01 if e.staged else up + 0.01)
            now = (e.blocked > 0, e.staged)
            if now != was:
                switches += 1
                assert e.graph is None and e._retired_graphs      # a switch retires the graph ...
            else:
                assert e.graph is not None                         # ... and nothing else does
            kinds.append(now)
        assert 4 <= switches <= 12, (d, switches)                  # 2 free + waits of 4, 8, 16, 32, 64, 64, ... readings
        assert len(e._retired_graphs) == switches
        # a run that has settled is free to switch again at once
        for _ in range(200):
            e._regime(1.05 if not e.staged else down - 0.01)
        assert e.blocked >= 1 and not e.staged
        e._regime(90.0)
        assert e.staged and not e.blocked
    # several modes: the same with the two-sided band of the matrix-core rounds
    sm = mcmc.REGIME_THRESHOLDS["several_modes"]
    r = _Rule(32, 262144, K=4, opts=opts)
    r.read(20.0)
    assert not r.blocked
    switches = 0
    for _ in range(400):
        was = r.blocked > 0
        r.read(sm["up"] - 0.01 if not r.blocked else sm["down"] + 0.01)
        switches += (r.blocked > 0) != was
    assert switches <= 12
    # the environment is not consulted per step: a switch flipped AFTER construction changes nothing for this engine
    e = _engine(50, 65536, opts=mcmc.RegimeOptions.from_env())
    monkeypatch.setenv("TEMPEST_AMD_SCREEN", "0")
    e._regime(6.0)                                  # screened band of 50-D: 6.0 >= 5.5 keeps the batches; the walker band (5.0) too
    e._regime(5.2)                                  # screened: 5.2 < 5.5 -> blocked rounds; with the screen off it would have stayed
    assert e.blocked >= 1


def test_regime_module_needs_neither_the_environment_nor_torch():
    """The rule is a function of its arguments: tempest_amd/regime.py imports nothing but typing at module level -- no os, no torch,
    no device.py -- and only RegimeOptions.from_env, called when an engine is built, looks at the environment."""
    import ast
    import inspect
    from tempest_amd import regime
    tree = ast.parse(inspect.getsource(regime))
    imported = {a.name if isinstance(node, ast.Import) else node.module
                for node in tree.body if isinstance(node, (ast.Import, ast.ImportFrom)) for a in node.names}
    assert imported == {"typing"}
    assert not hasattr(regime, "os") and not hasattr(regime, "torch") and not hasattr(regime, "device")
    nested = {node.module for node in ast.walk(tree) if isinstance(node, ast.ImportFrom)} | {
        a.name for node in ast.walk(tree) if isinstance(node, ast.Import) for a in node.names}
    assert nested == {"typing", "os"}
    for fn in (regime.Regime.next, regime.Regime.initial, regime.Regime.options, regime.regime_band):
        assert not {"os", "environ", "getenv"} & set(inspect.unwrap(getattr(fn, "__func__", fn)).__code__.co_names)


@pytest.mark.parametrize("d", [16, 17, 112, 113])
@pytest.mark.parametrize("K", [1, 4, 64, 65])
def test_regime_initial_truth_table(d, K):
    """An engine's first steps run as screened batches exactly where the screened kernel exists for its shape and may be used:
    16 < d <= 112 with the screen and the walker switches on, and one mode without an assignment or 2..64 modes with one."""
    from tempest_amd.regime import Regime, RegimeOptions
    for has_assign in (False, True):
        for screen in (False, True):
            for walker_ok in (False, True):
                r = Regime.initial(d, K, has_assign, RegimeOptions(walker_ok=walker_ok, screen=screen))
                want = (d > 16 and (screen and d <= 112) and walker_ok
                        and ((K == 1 and not has_assign) or (1 < K <= 64 and has_assign)))
                assert r.staged is bool(want), (d, K, has_assign, screen, walker_ok)
                assert r == Regime(staged=bool(want)) and (r.blocked, r.sm_lanes, r.unstaged, r.dwell, r.quick) == (0, 0, False, 0, 0)


def test_virtual_shards_of_the_canonical_partition():
    """csrc/common.h: tph_vshards_for and its Python twin -- V depends on the particle count alone (never on the number of
    ranks): the largest of 48, 16, 12, 8, 6, 4, 3, 2, 1 with n % (256 V) == 0.  The BASELINE ensembles are powers of two (V = 16:
    1, 2, 4, 8 or 16 GPUs give the same bits); 3 * 2^k particles also admit 3, 6, 12, 24, 48."""
    from tempest_amd.device import vshards_for
    assert vshards_for(1048576) == 16 and vshards_for(2097152) == 16 and vshards_for(65536) == 16 and vshards_for(262144) == 16
    assert vshards_for(49152) == 48 and vshards_for(12288) == 48 and vshards_for(3 * 4096) == 48
    assert vshards_for(512) == 2 and vshards_for(1024) == 4 and vshards_for(256) == 1 and vshards_for(768) == 3
    assert vshards_for(1000) == 1 and vshards_for(4096) == 16 and vshards_for(2048) == 8
    for n in (256 * k for k in range(1, 200)):
        v = vshards_for(n)
        assert n % (256 * v) == 0 and v in (48, 16, 12, 8, 6, 4, 3, 2, 1)
        assert all(n % (256 * w) != 0 for w in (48, 16, 12, 8, 6, 4, 3, 2, 1) if w > v)
    # the C side exports the same rule through the bench digest only; the kernels are pinned by tests/test_distributed.py (GPU)


# ------------------------------------------------- the input recipes of tests/test_propose_reg_gpu.py, with the oracle alone
@pytest.mark.parametrize("kernel", ["tpcn", "rwm"])
@pytest.mark.parametrize("d", range(1, 17))
def test_propose_reg_recipes_redraw_20_to_70_percent_of_first_attempts(kernel, d):
    """The ensembles of test_propose_reg_vs_oracle_every_dimension: at every d, for one mode and for three, 20-70 % of the
    walkers leave the cube at attempt 0 (the kernel's redraw rounds run, their list shrinks below half a wave and several lanes
    share a walker), and fewer than 1 % run into the redraw cap (256 oracle sweeps over a handful of rows, not over hundreds)."""
    from tests import propose_reg_cases as pc
    for K in (1, 3):
        e = pc.ensemble(d, kernel, K, 4097)
        flags = pc.flags_for(d, None)
        out0 = pc.first_attempt_out(e, flags)
        assert 0.20 <= out0 <= 0.70, (kernel, d, K, out0)
        capped = pc.cap_rows(e, pc.oracle(e, flags)[0]).mean()
        assert capped < 0.01, (kernel, d, K, capped)


@pytest.mark.parametrize("kernel", ["tpcn", "rwm"])
@pytest.mark.parametrize("d", [1, 8, 16])
def test_propose_reg_recipes_cap_ensembles_mix_capped_and_proposing_walkers(kernel, d):
    """The ensembles of test_propose_reg_redraw_cap_mixed_ensemble: 10-90 % of the walkers fail all 256 attempts."""
    from tests import propose_reg_cases as pc
    e = pc.cap_ensemble(d, kernel)
    capped = pc.cap_rows(e, pc.oracle(e, pc.flags_for(d, None))[0]).mean()
    assert 0.10 <= capped <= 0.90, (kernel, d, capped)


@pytest.mark.parametrize("d", [1, 7, 16])
def test_propose_reg_recipes_runaway_ensemble_fails_every_attempt(d):
    """The ensembles of test_redraw_cap_every_attempt_out_proposes_the_current_point: the oracle proposes u for every walker."""
    from tests import propose_reg_cases as pc
    e = pc.runaway_ensemble(d)
    assert pc.cap_rows(e, pc.oracle(e, pc.flags_for(d, None))[0]).all()


def test_propose_reg_launch_geometry_of_the_large_cases():
    """tests/propose_reg_cases.py: launch_geometry restates launch_propose_reg; on a 256-CU device the large cases of
    tests/test_propose_reg_gpu.py land where their names say."""
    from tests import propose_reg_cases as pc
    n_simd = 1024
    B2, B4 = 128 * n_simd, 256 * n_simd
    assert pc.launch_geometry(4097, n_simd) == (65, 1) and pc.launch_geometry(65536, n_simd) == (1024, 1)
    assert pc.launch_geometry(B2 + 64 * 3 + 1, n_simd) == (2052, 1)
    assert pc.rolled_form("tpcn", 12, B2 + 64 * 3 + 1, n_simd) and not pc.rolled_form("tpcn", 12, B2, n_simd)
    assert not pc.rolled_form("tpcn", 11, B4, n_simd) and not pc.rolled_form("rwm", 16, B4, n_simd)
    assert pc.launch_geometry(B4, n_simd) == (4096, 1)
    waves, tiles = pc.launch_geometry(B4 + 4097, n_simd)          # two tiles per wave, the last wave owns one
    assert (waves, tiles) == (2081, 2) and waves * tiles - (B4 + 4097 + 63) // 64 == 1
    assert pc.launch_geometry(8 * B4, n_simd) == (4096, 8)
    assert pc.launch_geometry(8 * B4 + 64 * 5 + 3, n_simd) == (4097, 8)      # ntiles > waves * REG_MAX_TILES: more waves
    assert pc.launch_geometry(20_000, n_simd, 3) == (105, 3) and pc.launch_geometry(20_000, n_simd, 8) == (40, 8)
