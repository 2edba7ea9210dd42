#!/usr/bin/env python
"""HipCallbacks derived quantities: time tphu_derived on the posterior layout.

    python tools/bench_derived.py --out profiles/derived_sweep.json

For a cheap function (n_dim 10, n_derived 2: a sum and a product) and a dear one (a loop over a 10 000-entry table) and
2^16, 2^20, 2^24 rows, row-major (n, n_dim) in and (n, n_derived) out, the median over `--reps` HIP-event timings (after `--warmup`
calls; the variants of one point alternate inside every repeat) of

  rowmajor   the LDS-tiled row-major kernel (what posterior(return_blobs=True) runs),
  direct     the same layout read a lane per row straight from memory (the fallback kernel, pinned),
  route_b    the route the row-major kernel replaces: x.T.contiguous(), the dimension-major kernel, out.T.contiguous(),
  copy       a device-to-device copy of the same number of bytes (n x (n_dim + n_derived) doubles): the streaming yardstick.

All three evaluations return the same bits (checked here at every point).  One process; a failure ends the sweep."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_DIM, N_DERIVED, N_TABLE = 10, 2, 10_000
SOURCES = {
    "cheap": ('''
__device__ void prior_transform(const double* u, double* x) { for (int j = 0; j < N_DIM; ++j) x[j] = 10.0 * u[j] - 5.0; }
__device__ double log_likelihood(const double* x) { double s = 0.0; for (int j = 0; j < N_DIM; ++j) s += x[j] * x[j]; return -0.5 * s; }
__device__ void derived(const double* x, double* out) {
  out[0] = x[0] + x[1];
  out[1] = x[0] * x[1];
}
''', False),
    "dear": ('''
__device__ void prior_transform(const double* u, double* x, const tphu_data& D) { for (int j = 0; j < N_DIM; ++j) x[j] = 10.0 * u[j] - 5.0; }
__device__ double log_likelihood(const double* x, const tphu_data& D) { double s = 0.0; for (int j = 0; j < N_DIM; ++j) s += x[j] * x[j]; return -0.5 * s; }
__device__ void derived(const double* x, double* out, const tphu_data& D) {      // chi^2 of a line against the table, and its largest residual
  double chi = 0.0, worst = 0.0;
  for (int64_t r = 0; r < D.t_len; ++r) {
    const double z = D.y[r] - (x[0] + x[1] * D.t[r]);
    chi += z * z;
    worst = fmax(worst, fabs(z));
  }
  out[0] = chi;
  out[1] = worst;
}
''', True),
}
SIZES = (1 << 16, 1 << 20, 1 << 24)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/derived_sweep.json")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    a = ap.parse_args()
    import numpy as np
    import torch
    import tempest_amd as tp
    from tempest_amd.hipcallbacks import derived_tiles
    if not torch.cuda.is_available():
        print("bench_derived: no GPU (a timing needs one)", file=sys.stderr)
        return 1
    rng = np.random.RandomState(5)
    t = np.linspace(-1.0, 1.0, N_TABLE)
    data = {"t": t, "y": 0.3 + 1.7 * t + 0.1 * rng.randn(N_TABLE)}
    rows = []
    for kind, (src, with_data) in SOURCES.items():
        cb = tp.HipCallbacks(src, N_DIM, n_derived=N_DERIVED, **({"data": data} if with_data else {}))
        for n in a.sizes:
            x = torch.from_numpy(rng.uniform(-5.0, 5.0, size=(n, N_DIM))).cuda()
            src_buf = torch.empty(n * (N_DIM + N_DERIVED), dtype=torch.float64, device="cuda").normal_()
            dst_buf = torch.empty_like(src_buf)

            def rowmajor():
                cb.derived_tile = 0
                return cb.derived(x)

            def direct():
                cb.derived_tile = 1
                out = cb.derived(x)
                cb.derived_tile = 0
                return out

            def route_b():
                return cb.derived(x.T.contiguous().T).contiguous()

            def copy():
                dst_buf.copy_(src_buf)
                return None

            variants = (("rowmajor", rowmajor), ("direct", direct), ("route_b", route_b), ("copy", copy))
            ref = None
            for _ in range(a.warmup):
                for name, fn in variants:
                    out = fn()
                    if out is not None:
                        ref = out.clone() if ref is None else ref
                        if not torch.equal(out, ref):
                            raise SystemExit(f"{name} differs from the row-major kernel at {kind} n={n}")
            torch.cuda.synchronize()
            ts = {name: [] for name, _ in variants}
            for _ in range(a.reps):
                for name, fn in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    ts[name].append(e0.elapsed_time(e1) * 1e3)
            row = {"function": kind, "n": n, "n_dim": N_DIM, "n_derived": N_DERIVED, "tile": (derived_tiles(N_DIM, N_DERIVED) or (0,))[0],
                   "bytes": 8 * n * (N_DIM + N_DERIVED)}
            for name, v in ts.items():
                v.sort()
                row[name + "_us"] = round(v[len(v) // 2], 2)
                row[name + "_min_us"] = round(v[0], 2)
            row["rowmajor_over_route_b"] = round(row["rowmajor_us"] / row["route_b_us"], 3)
            row["rowmajor_over_copy"] = round(row["rowmajor_us"] / row["copy_us"], 3)
            row["rowmajor_GBps"] = round(row["bytes"] / row["rowmajor_us"] / 1e3, 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del x, src_buf, dst_buf, ref
            torch.cuda.empty_cache()
    doc = {"tool": "tools/bench_derived.py", "device": torch.cuda.get_device_name(0),
           "method": "median (and minimum) of %d HIP-event timings of one call after %d warm-up calls, microseconds; the four variants "
                     "of a point alternate inside every repeat; one process; bytes = 8 n (n_dim + n_derived), what the row-major "
                     "kernel must move" % (a.reps, a.warmup), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
