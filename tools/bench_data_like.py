#!/usr/bin/env python
"""Term-form likelihoods of HipCallbacks: time the lane-per-particle kernel against the split kernel.

    python tools/bench_data_like.py --out profiles/data_like_sweep.json

For a cheap term (Gaussian residual: + - * /) and a dear one (Poisson rate with exp and log) and every (n, n_terms) of the sweep,
the median over `--reps` timed calls (HIP events around one cb.log_likelihood call on an idle stream, after `--warmup` calls) of
both paths, and of the split kernel with smaller particle tiles where n is small.  The two paths return the same bits (checked
here on every point), so the table decides time only: DATA_LIKE_THRESHOLDS in tempest_amd/hipcallbacks.py is read off it.

Every (term, n) runs in a child process of its own under a time limit; the first child that fails or runs out of time ends the
sweep (nothing more is started on a device that has just misbehaved).  Points with more than --max-work term evaluations per
call are left out and listed as such."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PRIOR = '''
__device__ void prior_transform(const double* u, double* x, const tphu_data& D) {
  for (int j = 0; j < N_DIM; ++j) x[j] = 10.0 * u[j] - 5.0;
}
'''
TERMS = {
    "cheap": PRIOR + '''
__device__ double log_likelihood_term(const double* x, int64_t r, const tphu_data& D) {
  const double m = x[0] + x[1] * D.t[r] + x[2] * D.t[r] * D.t[r];
  const double z = (D.y[r] - m) / D.s[r];
  return -0.5 * z * z - D.c[r];
}
''',
    "dear": PRIOR + '''
__device__ double log_likelihood_term(const double* x, int64_t r, const tphu_data& D) {
  const double lam = exp(0.1 * x[0] + 0.1 * x[1] * D.t[r]) + (x[2] + 6.0);
  return D.y[r] * log(lam) - lam - D.c[r];
}
''',
}
N_PARTICLES = (256, 1024, 4096, 16384, 65536, 262144, 1048576)
N_TERMS = (100, 1000, 10_000, 100_000, 1_000_000)


def child(kind, n, max_work, warmup, reps):
    import numpy as np
    import torch
    import tempest_amd as tp
    rng = np.random.RandomState(5)
    x = torch.from_numpy(rng.uniform(-5.0, 5.0, size=(3, n))).cuda().T         # the sampler's layout: (n, d) view of (d, n)
    rows = []
    for nt in N_TERMS:
        if n * nt > max_work:
            rows.append({"term": kind, "n": n, "n_terms": nt, "skipped": "n * n_terms above --max-work"})
            continue
        t = np.linspace(-1, 1, nt)
        s = 0.5 + 0.5 * rng.rand(nt)
        data = {"t": t, "y": np.floor(5.0 + 2.0 * rng.rand(nt)), "s": s, "c": np.log(s)}
        cb = tp.HipCallbacks(TERMS[kind], 3, data=data, n_terms=nt)
        row = {"term": kind, "n": n, "n_terms": nt}
        ref = None
        variants = [("lane", "lane", 0), ("split", "split", 0)]
        if n <= 1024:
            variants += [("split_tile16", "split", 16), ("split_tile4", "split", 4)]
        for name, path, tile in variants:
            cb.data_like, cb.split_tile = path, tile
            for _ in range(warmup):
                out = cb.log_likelihood(x)
            torch.cuda.synchronize()
            ref = out.clone() if ref is None else ref
            if not torch.equal(out, ref):
                raise SystemExit(f"{name} differs from the lane path at {kind} n={n} n_terms={nt}")
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                cb.log_likelihood(x)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            ts.sort()
            row[name + "_us"] = round(ts[len(ts) // 2], 2)
            row[name + "_min_us"] = round(ts[0], 2)
        row["split_over_lane"] = round(row["split_us"] / row["lane_us"], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/data_like_sweep.json")
    ap.add_argument("--max-work", type=float, default=4e9, help="largest n * n_terms timed")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child-timeout", type=float, default=120.0, help="seconds for one (term, n) child")
    ap.add_argument("--child", nargs=2, metavar=("TERM", "N"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        rows = child(a.child[0], int(a.child[1]), a.max_work, a.warmup, a.reps)
        print("ROWS " + json.dumps(rows), flush=True)
        return 0
    rows, t0 = [], time.time()
    for kind in TERMS:
        for n in N_PARTICLES:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, str(n), "--max-work", str(a.max_work),
                   "--warmup", str(a.warmup), "--reps", str(a.reps)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
            except subprocess.TimeoutExpired:
                print(f"child {kind} n={n} ran out of time: sweep ends here", file=sys.stderr)
                return 1
            got = [ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")]
            if r.returncode != 0 or not got:
                print(f"child {kind} n={n} failed ({r.returncode}): sweep ends here\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", file=sys.stderr)
                return 1
            rows += json.loads(got[-1][5:])
            print(f"{kind} n={n} done ({time.time() - t0:.0f} s)", flush=True)
            # (written after every child: a sweep that ends early leaves what it measured)
            import tempest_amd.hipcallbacks as hc
            doc = {"tool": "tools/bench_data_like.py", "sum_layout": list(hc.SUM_LAYOUT), "method": "median of %d HIP-event timings "
                   "of one cb.log_likelihood call after %d warm-up calls, microseconds; one process per (term, n)" % (a.reps, a.warmup),
                   "rows": rows}
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
