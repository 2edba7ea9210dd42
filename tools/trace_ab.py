"""The 10-D Rosenbrock of bench.py three ways in one process, interleaved: the torch callbacks as they are, tempest_amd.trace_callbacks
of those same two functions, and the hand-written ROSENBROCK_HIP -- `trace_ab.py [--particles 1048576,131072] [--steps K] [--warmup W]
[--rounds R] [--out FILE]`.  Every round builds a fresh Sampler per leg (same seed, so the same schedule of betas and steps where the
likelihood bits agree), runs the initialisation and W warm-up iterations untimed and times K iterations between two device
synchronisations, bench.py's protocol; the legs alternate inside a round so that clock and temperature drift falls on all three.
Prints particle-mutation-steps/s per leg and size (median and every round) as one JSON line."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import tempest_amd as tp
    from bench import ROSENBROCK_HIP, prior20, rosenbrock_torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", default="1048576,131072")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    traced = tp.trace_callbacks(prior20, rosenbrock_torch, 10)
    hand = tp.HipCallbacks(ROSENBROCK_HIP, 10)
    legs = (("eager_torch", (prior20, rosenbrock_torch)), ("traced", (traced.prior_transform, traced.log_likelihood)),
            ("hand_written_hip", (hand.prior_transform, hand.log_likelihood)))

    def timed(cbs, n):
        s = tp.Sampler(cbs[0], cbs[1], 10, n_particles=n, vectorize=True, clustering=False, random_state=a.seed, backend="torch",
                       batch_prior=True, device=0)
        while True:
            s.sample(return_state=False)
            if s.state.get_current("beta") > 0.0:
                break
        for _ in range(a.warmup):
            s.sample(return_state=False)
        torch.cuda.synchronize(dev)
        it0 = len(s.state._scalars["steps"])
        gc.collect()
        gc.disable()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            s.sample(return_state=False)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        gc.enable()
        steps, beta = np.asarray(s.state._scalars["steps"][it0:]), np.asarray(s.state._scalars["beta"][it0:])
        del s
        torch.cuda.empty_cache()
        return float(np.sum(steps[beta > 0])) * n / dt, [int(v) for v in steps]

    out = {"tool": "tools/trace_ab.py", "unit": "particle-mutation-steps/s", "workload": "10-D Rosenbrock of bench.py, clustering=False",
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "trace_report": {k: v for k, v in traced.trace_report.items() if k != "constants"}, "sizes": {}}
    for n in (int(v) for v in a.particles.split(",")):
        runs, sched = {name: [] for name, _ in legs}, {}
        for _ in range(a.rounds):
            for name, cbs in legs:
                v, st = timed(cbs, n)
                runs[name].append(v)
                sched[name] = st
                print(f"n={n} {name}: {v:.4g}", file=sys.stderr, flush=True)
        med = {k: float(np.median(v)) for k, v in runs.items()}
        out["sizes"][str(n)] = {"median": med, "rounds": runs, "traced_over_eager": med["traced"] / med["eager_torch"],
                                "traced_over_hand_written": med["traced"] / med["hand_written_hip"],
                                "mcmc_steps_per_timed_iteration": sched}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
