"""Record what the d > 16 proposal-regime rule decides over a grid of engines, switches and scripted probe readings
(tests/golden/regime_traces.json; tests/test_regime_traces.py regenerates and compares).  The rule is host logic whose every number
was fitted on the hardware: a change of the code around it must move no decision.  Everything here but `drive`, the one adapter onto
the code as it stands, is independent of where the rule lives, so the same script runs before and after such a change.

    python -m oracle.make_regime_traces          # rewrites the golden file

One scripted run is `drive(n_dim, n, K, env, initial_staged, script)`; a script item is (mean_attempts, captured), where
mean_attempts is a number or (attribute, a, b): `a` while the engine's `attribute` is set, else `b` (the flip-flop reads the
threshold that sends the current kernel away).  Per reading the record is
    [blocked, staged, sm_lanes, unstaged, retired a graph, OPT_BLOCKED, OPT_BLK_FAN, OPT_ML_UNSTAGED, OPT_STAGED_REDRAW, OPT_SM_LANES,
     OPT_SCREEN]
with the options' EFFECTIVE values in the context: what the library would read, however many calls set it (an option never set has the
default of include/tempest_hip.h).  Two conventions, both the engine's own:
  * a run starts the way StepEngine.load() starts one, with the engine's regime asserted in the context (an engine never reads a
    probe before load());
  * OPT_BLK_FAN is null while OPT_BLOCKED is 0: the library reads it in the blocked rounds only (mutate.hip, propose_blkm.hip), and
    blocked rounds begin with a change of OPT_BLOCKED.
Stored: per (n_dim, env) group the first 16 hex digits of a SHA-256 over its runs (n, K, initial_staged, script in grid order), and a
dozen runs in full; runs are run-length encoded as [count, record], in the hash too."""
import hashlib
import itertools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "regime_traces.json")
RECORDED_AT = "1e7948d"

OPTIONS = ("OPT_BLOCKED", "OPT_BLK_FAN", "OPT_ML_UNSTAGED", "OPT_STAGED_REDRAW", "OPT_SM_LANES", "OPT_SCREEN")
DEFAULTS = dict(zip(OPTIONS, (0, 1, 0, 0, 0, 1)))          # include/tempest_hip.h

N_DIMS = (10, 17, 32, 33, 50, 63, 64, 100, 112, 113, 128)
# 4096, 65536, 131072, 262144, 1048576 took 18 s to regenerate, a few seconds each; n only enters the number of rounds, so the hashed
# grid keeps one size in the middle, whose lists cross the floors of both tables, and the others are among the runs written out in full
NS = (131072,)
KS = (1, 4, 64, 80)
ENVS = ({}, {"TEMPEST_AMD_SCREEN": "0"}, {"TEMPEST_AMD_STAGED": "0"}, {"TEMPEST_AMD_BLK_MFMA": "0"}, {"TEMPEST_AMD_BLK_FAN": "0"},
        {"TEMPEST_AMD_BLK_FAN": "2"}, {"TEMPEST_AMD_BLK_FAN": "3"}, {"TEMPEST_AMD_SM_LANES": "3"}, {"TEMPEST_AMD_REGIME": "screened"})
SCRIPTS = ("sweep", "sweep_captured", "flipflop", "random", "ignored")

_SWEEP = [round(float(v), 6) for v in np.geomspace(90.0, 1.0, 40)]
_SWEEP = _SWEEP + _SWEEP[::-1]
_RANDOM = [round(float(10.0 ** (2.0 * v)), 6) for v in np.random.RandomState(20240611).uniform(0.0, 1.0, 300)]


def drive(n_dim, n, K, env, initial_staged, script):
    """One scripted run on the code as it stands: the records of its readings."""
    from tempest_amd import device as D
    from tempest_amd import mcmc
    ids = {name: getattr(D, name) for name in OPTIONS}

    class Ctx:
        def __init__(self):
            self.n_dim, self.opts, self.sets = n_dim, {}, 0

        def set_option(self, k, v):
            self.opts[k] = int(v)
            self.sets += 1

    class Eng:
        _regime, _push_options = mcmc.StepEngine._regime, mcmc.StepEngine._push_options
        blocked, staged, sm_lanes, unstaged = (property(lambda self, i=i: self.regime[i]) for i in range(4))

    e = Eng()
    e.ctx, e.n, e.K, e.graph = Ctx(), n, K, None
    e.regime = mcmc.Regime(staged=bool(initial_staged))
    e._retired_graphs, e._keep = [], None
    e._opts = mcmc.RegimeOptions.from_env(env)
    e._push_options()       # the start of a run, as StepEngine.load() asserts the engine's regime
    out, seen = [], {}
    for mean, captured in script:
        if isinstance(mean, tuple):
            mean = mean[1] if getattr(e, mean[0]) else mean[2]
        if captured:
            e.graph = object()
        retired = len(e._retired_graphs)
        e._regime(mean)
        key = e.regime[:4] + (len(e._retired_graphs) > retired, e.ctx.sets)
        rec = seen.get(key)
        if rec is None:
            eff = {name: e.ctx.opts.get(ids[name], DEFAULTS[name]) for name in OPTIONS}
            if not eff["OPT_BLOCKED"]:
                eff["OPT_BLK_FAN"] = None
            rec = seen[key] = [int(v) for v in key[:5]] + [eff[name] for name in OPTIONS]
        out.append(rec)
    return out


def script(name, n_dim, K, env):
    """The readings of one script (the flip-flop's depend on the band in force)."""
    from tempest_amd import mcmc
    if name == "sweep":
        return [(m, False) for m in _SWEEP]
    if name == "sweep_captured":
        return [(m, True) for m in _SWEEP]
    if name == "flipflop":      # test_regime_rule_does_not_oscillate: either kernel is asked for the other at every reading
        if K > 1:
            sm = mcmc.REGIME_THRESHOLDS["several_modes"]
            flip = ("blocked", sm["down"] + 0.01, sm["up"] - 0.01)
        else:
            screened = env.get("TEMPEST_AMD_SCREEN", "1") != "0" and n_dim <= 112
            up, down, _, _ = mcmc.regime_band("screened" if screened else "walker", n_dim)
            flip = ("staged", down - 0.01, up + 0.01)
        return [(60.0, False)] + [(flip, True)] * 400
    if name == "random":
        return [(m, (i // 7) % 2 == 1) for i, m in enumerate(_RANDOM)]
    if name == "ignored":
        return [(0.0, False), (-1.0, False), (float("nan"), False), (0.0, True), (-1.0, True), (float("nan"), True)]
    raise KeyError(name)


def env_id(env):
    return ",".join(f"{k[len('TEMPEST_AMD_'):]}={v}" for k, v in sorted(env.items())) or "default"


# runs written out in full (n_dim, n, K, env, initial_staged, script)
FULL = ((50, 65536, 1, {}, True, "flipflop"), (32, 262144, 4, {}, True, "flipflop"), (100, 131072, 1, {}, True, "flipflop"),
        (32, 262144, 1, {}, False, "flipflop"), (50, 65536, 1, {"TEMPEST_AMD_SCREEN": "0"}, False, "flipflop"),
        (50, 65536, 1, {}, True, "sweep"), (100, 131072, 1, {}, True, "sweep_captured"), (32, 262144, 4, {}, True, "sweep"),
        (32, 262144, 80, {}, False, "sweep"), (113, 131072, 1, {"TEMPEST_AMD_BLK_FAN": "2"}, False, "random"),
        (64, 1048576, 1, {"TEMPEST_AMD_SM_LANES": "3"}, True, "random"), (50, 65536, 1, {"TEMPEST_AMD_REGIME": "screened"}, True, "sweep"),
        (17, 4096, 1, {"TEMPEST_AMD_STAGED": "0"}, False, "sweep"), (50, 65536, 1, {}, True, "ignored"),
        (100, 4096, 1, {}, True, "sweep"), (32, 1048576, 1, {"TEMPEST_AMD_SCREEN": "0"}, False, "sweep"))


def run_length(records):
    out = []
    for r in records:
        if out and out[-1][1] == r:
            out[-1][0] += 1
        else:
            out.append([1, r])
    return out


def record(ns=NS):
    """{"groups": {"d<n_dim>|<env>": hash}, "full": {id: run-length encoded records}} of the code as it stands."""
    groups = {}
    for n_dim, env in itertools.product(N_DIMS, ENVS):
        h = hashlib.sha256()
        for n, K, staged, name in itertools.product(ns, KS, (False, True), SCRIPTS):
            recs = drive(n_dim, n, K, env, staged, script(name, n_dim, K, env))
            h.update(json.dumps([n, K, int(staged), name, run_length(recs)], separators=(",", ":")).encode())
        groups[f"d{n_dim}|{env_id(env)}"] = h.hexdigest()[:16]
    full = {}
    for n_dim, n, K, env, staged, name in FULL:
        full[f"d{n_dim}-n{n}-K{K}-{env_id(env)}-staged{int(staged)}-{name}"] = run_length(
            drive(n_dim, n, K, env, staged, script(name, n_dim, K, env)))
    return {"groups": groups, "full": full}


if __name__ == "__main__":
    rec = record()
    rec.update(recorded_at=RECORDED_AT, n=list(NS), K=list(KS), n_dim=list(N_DIMS), scripts=list(SCRIPTS),
               record=["blocked", "staged", "sm_lanes", "unstaged", "retired"] + list(OPTIONS))
    line = lambda v: json.dumps(v, separators=(",", ":"), sort_keys=True)      # noqa: E731
    with open(GOLDEN, "w") as f:        # one line per group and per run
        f.write("{\n" + ",\n".join(
            f'"{k}": ' + ("{\n" + ",\n".join(f'"{kk}": {line(vv)}' for kk, vv in sorted(v.items())) + "\n}" if isinstance(v, dict) else line(v))
            for k, v in sorted(rec.items())) + "\n}\n")
    print(f"{len(rec['groups'])} groups, {len(rec['full'])} runs in full -> {GOLDEN}")
