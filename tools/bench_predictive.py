#!/usr/bin/env python
"""HipCallbacks posterior predictive: time cb.predictive over rows x n_predict.

    python tools/bench_predictive.py --out profiles/predictive_sweep.json

The README's quadratic model (3 parameters, predict = x0 + x1 t + x2 t^2), quantiles (0.025, 0.5, 0.975), rows in
{10^3, 2^14, 2^18, 2^22} and n_predict in {10^2, 10^3, 10^4}.  Per point the median over `--reps` wall-clock timings (the call returns
host arrays, so it ends synchronised) after `--warmup` calls of

  predictive   cb.predictive(x, w) at the package's own tile rule,
  torch_slabs  a torch formulation that materialises the (rows, slab) matrix of predictions, at most `--slab-bytes` of it at a
               time: weighted mean and variance by matrix products, quantiles by a sort of every column and a search in the
               cumulative weights (skipped where rows x n_predict exceeds `--torch-limit`).

The two agree to rounding in mean and var, and in the quantiles except at knife edges; the tool prints the largest differences.
One process; a failure ends the sweep."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SOURCE = '''
__device__ void prior_transform(const double* u, double* x, const tphu_data& D) { for (int j = 0; j < N_DIM; ++j) x[j] = 10.0 * u[j] - 5.0; }
__device__ double log_likelihood(const double* x, const tphu_data& D) { double s = 0.0; for (int j = 0; j < N_DIM; ++j) s += x[j] * x[j]; return -0.5 * s; }
__device__ double predict(const double* x, int64_t r, const tphu_data& D) { return x[0] + x[1] * D.t[r] + x[2] * D.t[r] * D.t[r]; }
'''
ROWS = (1000, 1 << 14, 1 << 18, 1 << 22)
N_PREDICT = (100, 1000, 10_000)
QS = (0.025, 0.5, 0.975)


def torch_slabs(torch, x, w, t, qs, slab_bytes):
    n, R = x.shape[0], t.shape[0]
    u = w / w.sum()
    step = max(1, slab_bytes // (8 * n))
    mean, var, quant = [], [], []
    qv = torch.tensor(qs, dtype=torch.float64, device=x.device)
    for r0 in range(0, R, step):
        tt = t[r0:r0 + step]
        p = x[:, 0:1] + x[:, 1:2] * tt + x[:, 2:3] * tt * tt                 # (n, slab)
        m = u @ p
        mean.append(m)
        var.append(u @ (p - m) ** 2)
        ps, order = torch.sort(p, dim=0)
        cw = torch.cumsum(u[order], dim=0)                                     # (n, slab)
        idx = torch.searchsorted(cw.T.contiguous(), (cw[-1][:, None] * qv).contiguous()).clamp_(max=n - 1)
        quant.append(torch.gather(ps.T, 1, idx).T)
    return torch.cat(mean), torch.cat(var), torch.cat(quant, dim=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/predictive_sweep.json")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="*", default=list(ROWS))
    ap.add_argument("--n-predict", type=int, nargs="*", default=list(N_PREDICT))
    ap.add_argument("--slab-bytes", type=int, default=1 << 28)
    ap.add_argument("--torch-limit", type=float, default=5e9, help="rows x n_predict above which the torch formulation is skipped")
    a = ap.parse_args()
    import numpy as np
    import torch
    import tempest_amd as tp
    from tempest_amd.hipcallbacks import predict_tiles
    if not torch.cuda.is_available():
        print("bench_predictive: no GPU (a timing needs one)", file=sys.stderr)
        return 1
    rng = np.random.RandomState(5)
    rows = []

    def timed(fn):
        for _ in range(a.warmup):
            out = fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return out, ts

    for R in a.n_predict:
        tgrid = np.linspace(-1.0, 1.0, R)
        cb = tp.HipCallbacks(SOURCE, 3, data={"t": tgrid}, n_predict="t")
        tt = torch.from_numpy(tgrid).cuda()
        for n in a.rows:
            x = torch.from_numpy(np.array([0.7, 1.9, -1.1]) + 0.1 * rng.randn(n, 3)).cuda()
            w = torch.from_numpy(rng.uniform(0.1, 3.0, n)).cuda()
            pp, ts = timed(lambda: cb.predictive(x, w, quantiles=QS))
            tile, slab = predict_tiles(n, R, len(QS))
            row = {"rows": n, "n_predict": R, "tile": tile, "slab": slab, "predictive_ms": round(ts[len(ts) // 2], 3),
                   "predictive_min_ms": round(ts[0], 3), "evaluations_per_ns": round(n * R * 10 / ts[len(ts) // 2] / 1e6, 3)}
            if n * R <= a.torch_limit:
                (m, v, q), tt_ms = timed(lambda: torch_slabs(torch, x, w, tt, QS, a.slab_bytes))
                torch.cuda.synchronize()
                row.update(torch_slabs_ms=round(tt_ms[len(tt_ms) // 2], 3), torch_slabs_min_ms=round(tt_ms[0], 3),
                           torch_over_predictive=round(tt_ms[len(tt_ms) // 2] / ts[len(ts) // 2], 2),
                           mean_max_rel_diff=float(np.max(np.abs(m.cpu().numpy() - pp["mean"]) / np.abs(pp["mean"]).clip(1e-300))),
                           quantiles_equal_fraction=float(np.mean(q.cpu().numpy() == pp["quantiles"])))
                del m, v, q
            rows.append(row)
            print(json.dumps(row), flush=True)
            del x, w
            torch.cuda.empty_cache()
    doc = {"tool": "tools/bench_predictive.py", "device": torch.cuda.get_device_name(0),
           "method": "median (and minimum) of %d wall-clock timings of one synchronised call after %d warm-up call(s), milliseconds; "
                     "quantiles %s; evaluations_per_ns counts predict() 10 times per (row, index): two moment passes and eight select "
                     "passes; one process" % (a.reps, a.warmup, list(QS)), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
