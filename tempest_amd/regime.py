"""Which d > 16 proposal kernel the next steps run: the rule as a value (`Regime`) and a pure function of the redraw probe
(`Regime.next`).  Nothing here touches a context, a graph or the environment of a running step; StepEngine (mcmc.py) applies what
the rule returns."""
from typing import NamedTuple


class RegimeOptions:
    """Debugging switches of the d > 16 proposal regime (TEMPEST_AMD_STAGED / _SCREEN / _BLK_MFMA / _BLK_FAN / _SM_LANES): read from
    the environment ONCE, when an engine is built -- never in the step path."""
    __slots__ = ("walker_ok", "screen", "blk_mfma", "fan", "sm_lanes", "pin")

    def __init__(self, walker_ok=True, screen=True, blk_mfma=True, fan=1, sm_lanes=0, pin=""):
        self.walker_ok, self.screen, self.blk_mfma, self.fan, self.sm_lanes = walker_ok, screen, blk_mfma, int(fan), int(sm_lanes)
        # TEMPEST_AMD_REGIME=screened: every d > 16 step of a one-mode run through the screened batches, whatever the probe says.
        # Their proposals are the FP64 row walker's bit for bit and a particle's arithmetic never depends on its neighbours, so a
        # run pinned there is bitwise the same on any number of GPUs (the adaptive rule sends a step to the matrix-core rounds by
        # the RANK's own list lengths, and those kernels agree with the batches to rounding only)
        self.pin = pin

    @classmethod
    def from_env(cls, env=None):
        if env is None:
            from os import environ as env
        return cls(walker_ok=env.get("TEMPEST_AMD_STAGED", "1") != "0", screen=env.get("TEMPEST_AMD_SCREEN", "1") != "0",
                   blk_mfma=env.get("TEMPEST_AMD_BLK_MFMA", "1") != "0", fan=int(env.get("TEMPEST_AMD_BLK_FAN", "1")),
                   sm_lanes=int(env.get("TEMPEST_AMD_SM_LANES", "0")), pin=env.get("TEMPEST_AMD_REGIME", ""))


# Crossovers of the redraw probe (mean attempts per particle of a step) between the d > 16 proposal kernels.  One row per
# dimension band (the first whose n_dim_min <= n_dim):  (n_dim_min, up, down, cap, floor) --
#   up:    the blocked rounds are left when THEIR probe, the geometric estimate n / (n - first-attempt failures), reaches it;
#   down:  they are taken up again when the TRUE mean reported by the screened batches / the row walker falls below it
#          (the hard particles near a wall pull the true mean above the estimate: hence two numbers);
#   cap, floor: at most `cap` rounds, and only while the expected failure list still holds `floor` particles.
# All fitted on one MI355X with tools/regime_sweep.py; `source` names the sweep a row came from.
REGIME_THRESHOLDS = {
    "screened": {"source": "profiles/r04_regime_sweep.jsonl, profiles/r04_regime_sweep_fan.jsonl (fanned-out list rounds); the crossover "
                           "re-measured with the LDS-staged rounds of round 5: profiles/r05_regime_sweep.jsonl (unchanged)",
                 "bands": ((64, 3.0, 5.0, 6, 64.0), (33, 3.4, 5.5, 8, 64.0), (17, 8.0, 13.0, 12, 64.0))},
    "walker": {"source": "profiles/r03_propose_d50_d100.json (screen off: FP64 row walker, multi-lane straggler pass)",
               "bands": ((64, 4.5, 8.0, 24, 24576.0), (17, 3.5, 5.0, 24, 24576.0))},
    # several modes (matrix-core rounds over mode-pure tiles <-> per-mode screened batches / multi-lane kernel): leave at, return below
    "several_modes": {"source": "profiles/r04_regime_sweep_fan.jsonl", "up": 13.0, "down": 8.0},
    # multi-lane kernel: matrices from global memory (a quarter of the LDS) above, LDS-staged below
    "unstaged": {"source": "profiles/r02_propose_d50_d100.json", "up": 8.0, "down": 4.0},
    # a kernel switch retires the captured graph of the step: from the third switch in a row that comes within `recent` readings of
    # the one before, the next has to wait (4, 8, ... 64 probe readings) -- a probe that sits on a threshold and flips every step
    # costs a bounded number of captures (test_regime_rule_does_not_oscillate)
    "dwell": {"first": 4, "max": 64, "recent": 8},
}


def regime_band(table, n_dim):
    for row in REGIME_THRESHOLDS[table]["bands"]:
        if n_dim >= row[0]:
            return row[1:]
    return REGIME_THRESHOLDS[table]["bands"][-1][1:]


def _screened(n_dim, opts):
    return opts.screen and n_dim <= 112


class Regime(NamedTuple):
    """The d > 16 proposal regime of an engine and the rule's memory of its last switches."""
    blocked: int = 0            # rounds of the blocked kernel (attempts in lockstep) before the straggler pass; 0 = off
    staged: bool = False        # screened batches / row-walker kernel for redraw-dominated steps
    sm_lanes: int = 0           # the row walker's lanes per particle (log2); 0: the library sizes the lane groups (8 or 16)
    unstaged: bool = False      # multi-lane kernel without LDS-staged matrices (redraw-dominated steps)
    since: int = 1 << 30        # readings since the last kernel switch
    dwell: int = 0              # readings the next switch must wait
    quick: int = 0              # quick switches in a row

    @property
    def kernel(self):
        """What a captured graph has baked in: blocked rounds or not (not their number), screened batches / walker or multi-lane."""
        return self.blocked > 0, bool(self.staged)

    @classmethod
    def initial(cls, n_dim, K, has_assign, opts):
        """Nothing is known about the redraw rate before an engine's first steps: they run as screened batches, whose time is
        flat in it (0.4-3 ms), instead of through the multi-lane kernel, whose time is not (30 ms per launch from the prior
        at 131 072 x 100-D: three such launches were 2 % of the config-5 shard's run); the probe of step 2 picks the regime."""
        return cls(staged=bool(n_dim > 16 and _screened(n_dim, opts) and opts.walker_ok
                               and ((K == 1 and not has_assign) or (1 < K <= 64 and has_assign))))

    def options(self, n_dim, opts):
        """The six options of the library (names of device.OPT_*) that hold this regime, with their values."""
        return (("OPT_BLOCKED", int(self.blocked)), ("OPT_BLK_FAN", opts.fan), ("OPT_ML_UNSTAGED", int(self.unstaged)),
                ("OPT_STAGED_REDRAW", int(self.staged)), ("OPT_SM_LANES", self.sm_lanes),
                ("OPT_SCREEN", int(_screened(n_dim, opts))))

    def next(self, mean_attempts, *, n_dim, n, K, opts, captured):
        """The d > 16 proposal kernels report the mean number of attempts per particle of the step, and the host picks the
        kernel for the next steps from it (thresholds: REGIME_THRESHOLDS above).  A captured graph has its kernels baked in: when
        the rule asks for a different KERNEL than the graph holds (blocked <-> screened batches / walker <-> multi-lane; not for a
        different number of rounds), the engine retires the graph and captures the step again at its next launch -- an engine
        captured in a run's redraw-dominated first iterations would otherwise walk rows for the rest of the run.  One mode:
          * a step is a few attempts per particle: the blocked rounds (propose_blkm.hip: attempts in lockstep, 16 particles per
            wave, both triangular products on the FP64 matrix cores) -- attempt 0 of everybody, further rounds over the particles
            still out of bounds (fanned out), the rest finished by a screened launch over the list.  Its probe is the geometric
            estimate n / (n - first-attempt failures);
          * most attempts are redraws: the screened batches (propose_mf.hip; screen off: the FP64 row walker, propose_sm.hip).
            Their probe is the true mean, which the hard particles near a wall pull above the geometric estimate (131 072 x
            100-D: estimate 2.8 / true 4.7; 65 536 x 50-D: 2.1 / 2.7, 4.2 / 7.2) -- hence the two thresholds per band.
        Several modes (K > 1, up to 64): the matrix-core rounds over mode-pure tiles while a step is a few attempts per particle,
        their stragglers and the redraw-dominated steps through the per-mode screened batches (screen off: the multi-lane kernel,
        un-staged while redraws dominate, LDS-staged once a step is about one attempt).
        A switch back within a few readings of the last one makes the NEXT switch wait (REGIME_THRESHOLDS["dwell"]): a probe that
        sits on a threshold and flips every step costs a bounded number of captures, not one per step.
        `captured`: the step is held by a graph -- the same kernel then keeps its rounds and lane groups."""
        if n_dim <= 16 or not mean_attempts > 0.0:
            return self
        if opts.pin == "screened" and self.staged:
            return self                # pinned to the screened batches (RegimeOptions.pin)
        walker_ok = opts.walker_ok
        screened = _screened(n_dim, opts)
        up_est, down_true, cap, floor = regime_band("screened" if screened else "walker", n_dim)
        multi_ok = screened and K <= 64 and opts.blk_mfma
        if K != 1:
            sm_ = REGIME_THRESHOLDS["several_modes"]
            want_blk = multi_ok and mean_attempts < (sm_["down"] if self.blocked else sm_["up"])
        elif self.blocked:             # geometric estimate
            want_blk = mean_attempts < up_est or not walker_ok
        else:                          # true mean (screened batches / row walker, or the multi-lane kernel of a run's first steps)
            want_blk = mean_attempts < down_true and (walker_ok or mean_attempts < 2.0)
        # redraw-dominated steps: the screened batches -- with several modes one mode after the other over the particles of each
        # (propose_mf.hip: tph_propose_mf_modes); the multi-lane kernel only where the screen is off or K > 64
        want_sm = (K == 1 or multi_ok) and not want_blk and walker_ok
        since, dwell, quick = self.since + 1, self.dwell, self.quick
        if (want_blk, want_sm) == self.kernel:
            if captured:
                return self._replace(since=since)      # same kernel: the graph stays (its rounds and lane groups too)
        else:
            dw = REGIME_THRESHOLDS["dwell"]
            if since <= dwell:
                return self._replace(since=since)      # a switch so soon after the last one: wait (the current kernel is correct, only not the fastest)
            # consecutive switches each within a few readings of the one before: the second is still free (a run that crosses a
            # band once each way), from the third on the wait doubles
            quick = quick + 1 if since < max(dw["recent"], 2 * dwell) else 0
            dwell = 0 if quick < 2 else min(dw["max"], dw["first"] << (quick - 2))
            since = 0
        rounds = 0
        if want_blk:
            # A round that still has work costs at least one tile's latency (30-45 us at 100-D) however short its list: rounds
            # pay while the list fills the chip.  Expected list after k rounds: n (1 - 1/m)^k.  Measured against one round +
            # stragglers: 262 144 x 32-D -20 ... -26 %, 131 072 x 100-D -12 ... -17 %, 65 536 x 50-D +-0 (lists too short).
            # (screened: the straggler pass is a screened launch over the list: it settles a short list in one launch's latency, a
            # long one at ~8 us per straggler and wave -- rounds pay while the expected list is more than a few hundred particles)
            f, left = max(0.0, 1.0 - 1.0 / mean_attempts), float(n)
            rounds = 1
            # (a matrix-core round gives its failing columns `tries` attempts in place: TPH_OPT_BLK_TRIES, 2 up to n_dim 32, 1 above)
            f_round = f ** (1 if (n_dim > 32 or not screened) else 2)
            fan, fan_div = screened and opts.fan != 0, {2: 1, 3: 4}.get(opts.fan, 2)
            left *= f_round                         # after round 0
            while rounds < cap and left >= floor:
                # a list round gives every listed particle G attempts side by side (TPH_OPT_BLK_FAN, propose_blkm.hip: the largest
                # power of two <= 16 with G x list <= n / 2), so the list shrinks by f_round ** G
                G = 1
                while fan and G < 16 and 2 * fan_div * G * left <= n:
                    G *= 2
                left *= f_round ** G
                rounds += 1
        un = REGIME_THRESHOLDS["unstaged"]
        unstaged = self.unstaged
        if not captured:
            unstaged = mean_attempts > (un["down"] if unstaged else un["up"])      # hysteresis
        return Regime(rounds, want_sm, opts.sm_lanes, unstaged, since, dwell, quick)
