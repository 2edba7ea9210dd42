"""What Pareto smoothing costs beside the plain pointwise pass: cb.psis_loo(x) against cb.pointwise(x, w) on the SAME object, rows and
observations -- the README's quadratic regression built with pointwise="psis" -- `bench_psis.py [--rows 131072] [--terms 1000]
[--calls K] [--rounds R] [--out FILE]`.  One process, the two legs alternating inside a round; a call of each untimed first (code
objects, scratch), then K calls between two device synchronisations (each call ends in the copy of its results to the host).  Prints
seconds per call -- the median over the rounds, their smallest and largest, every round -- and the share of rows x terms term
evaluations per second that is, as one JSON line.  psis_loo sweeps the rows 10 times (range, 8 select passes, collect) and
pointwise twice."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

QUAD = '''
__device__ void prior_transform(const double* u, double* x, const tphu_data& D) {
  for (int j = 0; j < N_DIM; ++j) x[j] = 10.0 * u[j] - 5.0;
}
__device__ double log_likelihood_term(const double* x, int64_t r, const tphu_data& D) {
  const double m = x[0] + x[1] * D.t[r] + x[2] * D.t[r] * D.t[r];
  const double z = (D.y[r] - m) / D.s[r];
  return -0.5 * z * z;
}
'''


def main():
    import torch
    import tempest_amd as tp
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--terms", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(a.seed)
    t = np.linspace(-1.0, 1.0, a.terms)
    s = 0.5 + 0.5 * rng.rand(a.terms)
    D = {"t": t, "y": 0.7 + 1.9 * t - 1.1 * t * t + s * rng.randn(a.terms), "s": s}
    cb = tp.HipCallbacks(QUAD, 3, data=D, n_terms="t", pointwise="psis")
    # rows as a posterior of this regression has them: the truth plus noise of the posterior's scale
    x = torch.from_numpy(np.array([0.7, 1.9, -1.1]) + 0.05 * rng.randn(a.rows, 3)).to(dev)
    w = torch.ones(a.rows, dtype=torch.float64, device=dev)
    legs = (("pointwise", lambda: cb.pointwise(x, w)), ("psis_loo", lambda: cb.psis_loo(x)))
    last = {name: fn() for name, fn in legs}
    runs = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, fn in legs:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            torch.cuda.synchronize(dev)
            runs[name].append((time.perf_counter() - t0) / a.calls)
            print(f"{name}: {runs[name][-1] * 1e3:.3f} ms", file=sys.stderr, flush=True)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    ps = last["psis_loo"]
    out = {"tool": "tools/bench_psis.py", "unit": "seconds per call", "rows": a.rows, "terms": a.terms, "calls": a.calls, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "tail_len": ps["tail_len"], "median": med,
           "min": {k: min(v) for k, v in runs.items()}, "max": {k: max(v) for k, v in runs.items()}, "rounds_s": runs,
           "psis_over_pointwise": med["psis_loo"] / med["pointwise"],
           "term_evaluations_per_s": {"pointwise": 2 * a.rows * a.terms / med["pointwise"], "psis_loo": 10 * a.rows * a.terms / med["psis_loo"]},
           "pareto_k_quartiles": [float(v) for v in np.percentile(ps["pareto_k"], (0, 25, 50, 75, 100))],
           "n_high_k": ps["totals"]["n_high_k"],
           "max_abs_elpd_psis_minus_elpd_loo": float(np.max(np.abs(ps["elpd_psis"] - last["pointwise"]["elpd_loo"])))}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
