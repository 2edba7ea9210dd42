"""What a non-uniform prior costs on the fused path, and what tracing it buys: the 10-D Rosenbrock of bench.py under
Prior([Normal(0, 5)] * 10) with traced callbacks, the same two functions as eager torch callbacks (the baseline: what such a model ran
on before torch.special.ndtri could be traced), and today's traced uniform prior (what the ten tphu_ndtri calls cost) -- `bench_priors.py
[--particles 1048576,131072] [--steps K] [--warmup W] [--rounds R] [--out FILE]`.  One process, the legs alternating inside a round
so that clock and temperature drift falls on all three (tools/trace_ab.py's protocol, which is bench.py's: initialisation and W
warm-up iterations untimed, K iterations between two device synchronisations).  Prints particle-mutation-steps/s per leg and size --
the median over the rounds, their smallest and largest, every round -- as one JSON line.  The legs under the Normal prior sample
another posterior than the uniform one, so their schedules of MCMC steps differ: the unit divides that out."""
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
    from bench import prior20, rosenbrock_torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", default="1048576,131072")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    prior = tp.Prior([tp.priors.Normal(0.0, 5.0)] * 10)
    normal = tp.trace_callbacks(prior.transform, rosenbrock_torch, 10)
    uniform = tp.trace_callbacks(prior20, rosenbrock_torch, 10)
    legs = (("traced_normal", (normal.prior_transform, normal.log_likelihood)), ("eager_normal", (prior.transform, rosenbrock_torch)),
            ("traced_uniform", (uniform.prior_transform, uniform.log_likelihood)))

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

    out = {"tool": "tools/bench_priors.py", "unit": "particle-mutation-steps/s",
           "workload": "10-D Rosenbrock of bench.py, clustering=False; Prior([Normal(0, 5)] * 10) against 20 u - 10",
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "probe": {"traced_normal": normal.trace_report["probe"]["prior_transform"]}, "sizes": {}}
    for n in (int(v) for v in a.particles.split(",")):
        runs, sched = {name: [] for name, _ in legs}, {}
        for _ in range(a.rounds):
            for name, cbs in legs:
                v, st = timed(cbs, n)
                runs[name].append(v)
                sched[name] = st
                print(f"n={n} {name}: {v:.4g}", file=sys.stderr, flush=True)
        med = {k: float(np.median(v)) for k, v in runs.items()}
        out["sizes"][str(n)] = {"median": med, "min": {k: min(v) for k, v in runs.items()}, "max": {k: max(v) for k, v in runs.items()},
                                "rounds": runs, "traced_normal_over_eager_normal": med["traced_normal"] / med["eager_normal"],
                                "traced_normal_over_traced_uniform": med["traced_normal"] / med["traced_uniform"],
                                "mcmc_steps_per_timed_iteration": sched}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
