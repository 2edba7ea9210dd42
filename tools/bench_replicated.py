#!/usr/bin/env python
"""HipCallbacks replicated data: time cb.replicated against cb.predictive of the same model.

    python tools/bench_replicated.py --out profiles/replicated_sweep.json

A linear Gaussian model over `--n-obs` observations (data t, s, y), `--rows` weighted rows, 3 quantiles.  The median over `--reps`
HIP-event timings of one whole call -- weights check, every launch, the copy of the results to the host -- after `--warmup` calls,
the variants alternating inside every repeat, of

  predictive     cb.predictive of predict(x, r) = x[0] + x[1] t[r]                     (the yardstick: no noise),
  replicated     cb.replicated of replicate = predict + s[r] g.normal(0), no observed= (bands alone),
  with_pit       the same with observed="y"                                             (bands + PIT counters),
  with_pvalue    the same with discrepancy() = z^2                                      (bands + PIT + the p-value kernel).

--build-only compiles the four plugins into the cache and stops (no GPU needed).  One process; a failure ends the run."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODEL = '''
__device__ void prior_transform(const double* u, double* x, const tphu_data& D) { x[0] = 4.0 * u[0] - 1.0; x[1] = 4.0 * u[1] - 1.0; }
__device__ double log_likelihood_term(const double* x, int64_t r, const tphu_data& D) {
  const double z = (D.y[r] - (x[0] + x[1] * D.t[r])) / D.s[r];
  return -0.5 * z * z;
}
'''
PREDICT = '''
__device__ double predict(const double* x, int64_t r, const tphu_data& D) { return x[0] + x[1] * D.t[r]; }
'''
REPLICATE = '''
__device__ double replicate(const double* x, int64_t r, const tphu_noise& g, const tphu_data& D) {
  return (x[0] + x[1] * D.t[r]) + D.s[r] * g.normal(0);
}
'''
DISCREPANCY = '''
__device__ double discrepancy(const double* x, int64_t r, double y, const tphu_data& D) {
  const double z = (y - (x[0] + x[1] * D.t[r])) / D.s[r];
  return z * z;
}
'''
QS = (0.025, 0.5, 0.975)


def objects(tp, data):
    kw = dict(data=data, n_terms="t")
    return {"predictive": tp.HipCallbacks(MODEL + PREDICT, 2, n_predict="t", **kw),
            "replicated": tp.HipCallbacks(MODEL + REPLICATE, 2, n_replicate="t", **kw),
            "with_pit": tp.HipCallbacks(MODEL + REPLICATE, 2, n_replicate="t", observed="y", **kw),
            "with_pvalue": tp.HipCallbacks(MODEL + REPLICATE + DISCREPANCY, 2, n_replicate="t", observed="y", **kw)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/replicated_sweep.json")
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--n-obs", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import tempest_amd as tp
    rng = np.random.RandomState(5)
    t = np.linspace(0.0, 1.0, a.n_obs)
    s = 0.1 + 0.2 * rng.rand(a.n_obs)
    data = {"t": t, "s": s, "y": 1.5 + 0.75 * t + s * rng.randn(a.n_obs)}
    cbs = objects(tp, data)
    if a.build_only:
        print("\n".join(str(cb.path) for cb in cbs.values()))
        return 0
    if not torch.cuda.is_available():
        print("bench_replicated: no GPU (a timing needs one)", file=sys.stderr)
        return 1
    n = a.rows
    x = torch.from_numpy(np.array([1.5, 0.75]) + 0.05 * rng.randn(n, 2)).cuda()
    w = torch.from_numpy(rng.uniform(0.1, 3.0, n)).cuda()
    calls = {name: ((lambda cb=cb: cb.predictive(x, w, quantiles=QS)) if name == "predictive" else
                    (lambda cb=cb: cb.replicated(x, w, quantiles=QS, seed=1))) for name, cb in cbs.items()}
    outs = {}
    for _ in range(a.warmup):
        for name, fn in calls.items():
            outs[name] = fn()
    for key in ("mean", "var", "quantiles"):          # one matrix of draws: the three replicated variants agree to the bit
        assert np.array_equal(outs["replicated"][key], outs["with_pit"][key]) and np.array_equal(outs["replicated"][key], outs["with_pvalue"][key])
    assert np.array_equal(outs["with_pit"]["pit"], outs["with_pvalue"]["pit"])
    torch.cuda.synchronize()
    ts = {name: [] for name in calls}
    for _ in range(a.reps):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1))
    row = {"rows": n, "n_obs": a.n_obs, "quantiles": list(QS), "tile_slab": list(tp.hipcallbacks.predict_tiles(n, a.n_obs, len(QS)))}
    for name, v in ts.items():
        v.sort()
        row[name + "_ms"] = round(v[len(v) // 2], 3)
        row[name + "_min_ms"] = round(v[0], 3)
        row[name + "_max_ms"] = round(v[-1], 3)
    for name in ("replicated", "with_pit", "with_pvalue"):
        row[name + "_over_predictive"] = round(row[name + "_ms"] / row["predictive_ms"], 3)
    row["p_value"], row["pit_mean"] = outs["with_pvalue"]["p_value"], float(np.mean(outs["with_pit"]["pit"]))
    print(json.dumps(row), flush=True)
    doc = {"tool": "tools/bench_replicated.py", "device": torch.cuda.get_device_name(0),
           "method": "median (minimum, maximum) of %d HIP-event timings of one whole call after %d warm-up calls, milliseconds; the four "
                     "variants alternate inside every repeat; one process" % (a.reps, a.warmup), "rows": [row]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
