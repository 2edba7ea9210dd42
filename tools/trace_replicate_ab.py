#!/usr/bin/env python
"""trace_callbacks(replicate=, discrepancy=) against the hand-written source it restates: time cb.replicated of both (DESIGN.md
section 11t).

    python tools/trace_replicate_ab.py --out profiles/trace_replicate_ab.json

The linear Gaussian model of tools/bench_replicated.py over `--n-obs` observations, `--rows` weighted rows, 3 quantiles, with
observed= and discrepancy (bands, PIT and p-value).  Two legs in one process, alternating inside every round (the order swaps from round to round): the traced
object and the hand-written one.  A round times a window of `--calls` whole calls per leg (weights check, every launch, the results to the host:
the call ends in a synchronisation) with the host clock; per leg the median over `--rounds` rounds of the time per call, the
minimum, the maximum and the spread (max - min) / median.  Before any timing the two legs' outputs are compared at the timed shape,
bit for bit.  --build-only compiles the two plugins into the cache and stops (no GPU needed)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_replicated import DISCREPANCY, MODEL, QS, REPLICATE  # noqa: E402

KEYS = ("mean", "var", "quantiles", "pit", "p_value", "t_obs_mean", "t_rep_mean")


def prior(u):
    return 4.0 * u - 1.0


def term(x, D):
    z = (D["y"] - (x[:, 0:1] + x[:, 1:2] * D["t"])) / D["s"]
    return -0.5 * z * z


def replicate(x, D, g):
    return (x[:, 0:1] + x[:, 1:2] * D["t"]) + D["s"] * g.normal(0)


def discrepancy(x, y, D):
    z = (y - (x[:, 0:1] + x[:, 1:2] * D["t"])) / D["s"]
    return z * z


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/trace_replicate_ab.json")
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--n-obs", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import tempest_amd as tp
    rng = np.random.RandomState(5)
    t = np.linspace(0.0, 1.0, a.n_obs)
    s = 0.1 + 0.2 * rng.rand(a.n_obs)
    data = {"t": t, "s": s, "y": 1.5 + 0.75 * t + s * rng.randn(a.n_obs)}
    kw = dict(data=data, n_terms="t", n_replicate="t", observed="y")
    legs = {"traced": tp.trace_callbacks(prior, term, 2, replicate=replicate, discrepancy=discrepancy, **kw),
            "hand_written": tp.HipCallbacks(MODEL + REPLICATE + DISCREPANCY, 2, **kw)}
    draws = legs["traced"].trace_report["draws"]["replicate"]
    assert legs["traced"].source.count("g.normal(0)") == 1 and draws == {"normal": [0], "uniform": []}, draws
    if a.build_only:
        print("\n".join(str(cb.path) for cb in legs.values()))
        return 0
    if not torch.cuda.is_available():
        print("trace_replicate_ab: no GPU (a timing needs one)", file=sys.stderr)
        return 1
    n = a.rows
    x = torch.from_numpy(np.array([1.5, 0.75]) + 0.05 * rng.randn(n, 2)).cuda()
    w = torch.from_numpy(rng.uniform(0.1, 3.0, n)).cuda()
    outs = {}
    for _ in range(a.warmup):
        for name, cb in legs.items():
            outs[name] = cb.replicated(x, w, quantiles=QS, seed=1)
    for key in KEYS:
        assert np.array_equal(np.asarray(outs["traced"][key]), np.asarray(outs["hand_written"][key])), key
    torch.cuda.synchronize()
    per_call = {name: [] for name in legs}
    for k in range(a.rounds):
        for name, cb in (list(legs.items()) if k % 2 == 0 else list(legs.items())[::-1]):       # neither leg always follows the other
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                cb.replicated(x, w, quantiles=QS, seed=1)
            torch.cuda.synchronize()
            per_call[name].append((time.perf_counter() - t0) / a.calls * 1e3)
    row = {"rows": n, "n_obs": a.n_obs, "quantiles": list(QS), "calls_per_window": a.calls, "rounds": a.rounds,
           "outputs_equal": True, "probe": {k: legs["traced"].trace_report["probe"][k] for k in ("replicate", "discrepancy")}}
    for name, v in per_call.items():
        v.sort()
        med = v[len(v) // 2]
        row[name + "_ms"], row[name + "_min_ms"], row[name + "_max_ms"] = round(med, 4), round(v[0], 4), round(v[-1], 4)
        row[name + "_spread"] = round((v[-1] - v[0]) / med, 4)
    row["traced_over_hand_written"] = round(row["traced_ms"] / row["hand_written_ms"], 4)
    print(json.dumps(row), flush=True)
    doc = {"tool": "tools/trace_replicate_ab.py", "device": torch.cuda.get_device_name(0),
           "method": "milliseconds per whole cb.replicated call: host clock around a window of %d calls between two synchronisations, "
                     "median (minimum, maximum) over %d rounds, the two legs alternating inside every round in an order that swaps from round to round, after %d warm-up calls "
                     "each; one process" % (a.calls, a.rounds, a.warmup), "rows": [row]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
