#!/usr/bin/env python
"""Posterior marginals: time HipContext.marginals (tph_marginals).

    python tools/bench_marginals.py --out profiles/marginals_sweep.json

For 2^16 .. 2^24 rows, 10 and 100 columns, 64 bins and five quantiles -- at 10 columns also with pairs="all" (45 tables of 32 x 32) --
the median over `--reps` HIP-event timings (after `--warmup` calls; the variants of one point alternate inside every repeat) of

  marginals  one HipContext.marginals call: everything, the copies of the results to the host included,
  torch      the same work as torch ops on the device: sums for the moments, the bin index by arithmetic and integer index_add_ for
             the tables, sort + cumsum + searchsorted for the quantiles (ten columns at a time, to bound its memory),
  copy       a device-to-device copy of the same number of bytes (rows x columns doubles): the streaming yardstick.

The counts and the quantiles of the two evaluations are compared at every point (to the last place of the sum of the weights, which
torch adds in its own order).  One process; a failure ends the sweep."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (1 << 16, 1 << 18, 1 << 20, 1 << 22, 1 << 24)
COLUMNS = (10, 100)
BINS, BINS_2D = 64, 32
QS = (0.025, 0.16, 0.5, 0.84, 0.975)


def torch_marginals(torch, v, w, pairs):
    """The torch formulation: (counts, quantiles, counts_2d) and the moments, all on the device."""
    m, c = v.shape
    W = w.sum()
    u = w / W
    k = torch.round(u * 2.0 ** 52).to(torch.int64)
    mean = (u[:, None] * v).sum(0)
    var = (u[:, None] * (v - mean) ** 2).sum(0)
    lo, hi = v.amin(0), v.amax(0)

    def bins_of(B):
        b = ((v - lo) * (B / (hi - lo))).to(torch.int64)
        return b.clamp_(max=B - 1)
    b1 = bins_of(BINS)
    counts = torch.zeros(c * BINS, dtype=torch.int64, device=v.device)
    counts.index_add_(0, (b1 + torch.arange(c, device=v.device) * BINS).reshape(-1), k[:, None].expand(m, c).reshape(-1))
    counts2 = None
    if len(pairs):
        b2 = bins_of(BINS_2D)
        counts2 = torch.zeros(len(pairs) * BINS_2D * BINS_2D, dtype=torch.int64, device=v.device)
        for p, (a, b) in enumerate(pairs):
            counts2.index_add_(0, p * BINS_2D * BINS_2D + b2[:, a] * BINS_2D + b2[:, b], k)
    targets = torch.tensor([max(1, int(-(-q * 2.0 ** 52 // 1))) for q in QS], dtype=torch.int64, device=v.device)
    quant = torch.empty(len(QS), c, dtype=torch.float64, device=v.device)
    for j0 in range(0, c, 10):
        vs, order = v[:, j0:j0 + 10].sort(dim=0)
        cum = k[order].cumsum(0).T.contiguous()
        at = torch.searchsorted(cum, torch.minimum(targets[None, :], cum[:, -1:]).expand(cum.shape[0], len(QS)).contiguous())
        quant[:, j0:j0 + 10] = vs.T.gather(1, at).T
    return counts.reshape(c, BINS), quant, counts2, mean, var


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/marginals_sweep.json")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--columns", type=int, nargs="*", default=list(COLUMNS))
    a = ap.parse_args()
    import numpy as np
    import torch
    from tempest_amd.device import HipContext
    if not torch.cuda.is_available():
        print("bench_marginals: no GPU (a timing needs one)", file=sys.stderr)
        return 1
    ctx = HipContext(2, 0)

    def save(rows):
        doc = {"tool": "tools/bench_marginals.py", "device": torch.cuda.get_device_name(0),
               "method": "median (and minimum) of %d HIP-event timings of one call after %d warm-up calls, microseconds; the three "
                         "variants of a point alternate inside every repeat; one process; bytes = 8 n c, one reading of the rows (a "
                         "marginals call reads them 12 times: two moment sweeps, eight select passes, the two histograms)"
                         % (a.reps, a.warmup),
               "sizes": a.sizes, "columns": a.columns, "rows": rows}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    gen = torch.Generator(device="cuda").manual_seed(5)
    rows = []
    for c in a.columns:
        for n in a.sizes:
            for with_pairs in ((False, True) if c == 10 else (False,)):
                v = torch.randn(n, c, dtype=torch.float64, device="cuda", generator=gen)
                w = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) + 0.1
                src_buf, dst_buf = v.reshape(-1), torch.empty(n * c, dtype=torch.float64, device="cuda")
                pairs = [(i, j) for i in range(c) for j in range(i + 1, c)] if with_pairs else []

                def marginals():
                    return ctx.marginals(v, w, bins=BINS, quantiles=QS, pairs=pairs or None, bins_2d=BINS_2D)

                def torch_way():
                    return torch_marginals(torch, v, w, pairs)

                def copy():
                    dst_buf.copy_(src_buf)

                variants = (("marginals", marginals), ("torch", torch_way), ("copy", copy))
                got = marginals()
                tc, tq, tc2, _, _ = torch_way()
                # torch sums the weights in its own order: its W, and with it every integer weight, may differ in the last place
                slack = dict(rtol=1e-9, atol=float(n))
                if not (np.allclose(got["counts"], tc.cpu().numpy(), **slack) and np.allclose(got["quantiles"], tq.cpu().numpy(), rtol=0, atol=1e-2)
                        and (not pairs or np.allclose(got["counts_2d"].reshape(-1), tc2.cpu().numpy(), **slack))):
                    raise SystemExit(f"the torch formulation differs from tph_marginals at n={n} c={c} pairs={with_pairs}")
                del tc, tq, tc2
                for _ in range(a.warmup):
                    for _, fn in variants:
                        fn()
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
                row = {"n": n, "c": c, "bins": BINS, "n_q": len(QS), "pairs": len(pairs), "bins_2d": BINS_2D, "bytes": 8 * n * c}
                for name, t in ts.items():
                    t.sort()
                    row[name + "_us"] = round(t[len(t) // 2], 2)
                    row[name + "_min_us"] = round(t[0], 2)
                row["marginals_over_torch"] = round(row["marginals_us"] / row["torch_us"], 3)
                row["marginals_over_copy"] = round(row["marginals_us"] / row["copy_us"], 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
                save(rows)                                    # after every point: an interrupted sweep keeps what it measured
                del v, w, src_buf, dst_buf
                torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
