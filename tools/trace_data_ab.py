"""A likelihood over observed data three ways in one process, interleaved: tempest_amd.trace_callbacks of a torch term function of
(x, D), the hand-written HipCallbacks source it restates (the yardstick), and the eager torch closure (the (n, T) term matrix,
.sum(1)) -- `trace_data_ab.py [--rounds R] [--reps K] [--window SECONDS] [--steps S] [--warmup W] [--out FILE]`.

The model is the quadratic regression of the README (QUAD of tests/test_hipcallbacks_predict.py).  Measured: cb.log_likelihood at
(n, T) = (131 072, 100), the lane-per-particle path, and (4096, 100 000), the split path -- seconds per call: K calls between two
device synchronisations after 3 untimed ones, K raised per leg and shape until the timed window lasts --window seconds (a window of a
millisecond measures the clock and the scheduler) --; and particle-mutation-steps/s of a short Sampler run at 131 072 particles, T = 1000
(bench.py's protocol, as tools/trace_ab.py: initialisation and W warm-up iterations untimed, S iterations timed).  The legs alternate
inside a round, so clock and temperature drift falls on all three; medians over the rounds and the round-to-round spread
((max - min) / median) per leg are printed as one JSON line.  Needs a GPU: there is no fallback."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PRIOR_HIP = '''
__device__ void prior_transform(const double* u, double* x, const tphu_data& D) {
  for (int j = 0; j < N_DIM; ++j) x[j] = 10.0 * u[j] - 5.0;
}
'''
QUAD_HIP = PRIOR_HIP + '''
__device__ double log_likelihood_term(const double* x, int64_t r, const tphu_data& D) {
  const double m = x[0] + x[1] * D.t[r] + x[2] * D.t[r] * D.t[r];
  const double z = (D.y[r] - m) / D.s[r];
  return -0.5 * z * z;
}
'''
LIKE_SHAPES = ((131_072, 100), (4096, 100_000))
RUN_SHAPE = (131_072, 1000)


def prior(u):
    return 10.0 * u - 5.0


def term(x, D):
    m = x[:, 0:1] + x[:, 1:2] * D["t"] + x[:, 2:3] * D["t"] * D["t"]
    z = (D["y"] - m) / D["s"]
    return -0.5 * z * z


def data(n_terms, seed=7):
    rng = np.random.RandomState(seed)
    t = np.linspace(-1, 1, n_terms)
    s = 0.5 + 0.5 * rng.rand(n_terms)
    return {"t": t, "y": 0.7 + 1.9 * t - 1.1 * t * t + s * rng.randn(n_terms), "s": s}


def summary(runs, higher_is_better):
    med = {k: float(np.median(v)) for k, v in runs.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in runs.items()}
    ratio = med["traced"] / med["hand_written_hip"]
    return {"median": med, "spread": spread, "rounds": runs,
            "traced_over_hand_written": ratio if higher_is_better else 1.0 / ratio, "note": "ratios > 1: traced is faster"}


def main():
    import torch
    import tempest_amd as tp
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--window", type=float, default=0.25, help="least timed window of a log_likelihood leg, seconds")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("trace_data_ab.py: no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    out = {"tool": "tools/trace_data_ab.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps,
           "steps": a.steps, "warmup": a.warmup, "log_likelihood": {}, "sampler": {}}

    def objects(n_terms):
        D = data(n_terms)
        Dt = {k: torch.from_numpy(v).to(dev) for k, v in D.items()}
        return (tp.trace_callbacks(prior, term, 3, data=D, n_terms="t"), tp.HipCallbacks(QUAD_HIP, 3, data=D, n_terms="t"),
                lambda x: term(x, Dt).sum(1))

    for n, n_terms in LIKE_SHAPES:
        traced, hand, eager = objects(n_terms)
        legs = (("traced", traced.log_likelihood), ("hand_written_hip", hand.log_likelihood), ("eager_torch", eager))
        x = torch.from_numpy(np.random.RandomState(1).uniform(-5.0, 5.0, size=(n, 3))).to(dev)
        assert torch.equal(traced.log_likelihood(x), hand.log_likelihood(x))
        runs, reps = {name: [] for name, _ in legs}, {}

        def window(fn, k):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(k):
                fn(x)
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0
        for name, fn in legs:                     # untimed: the calls per window of this leg at this shape
            window(fn, 3)
            reps[name] = max(a.reps, int(1.1 * a.window / (window(fn, a.reps) / a.reps)) + 1)
        for _ in range(a.rounds):
            for name, fn in legs:
                window(fn, 3)
                runs[name].append(window(fn, reps[name]) / reps[name])
                print(f"log_likelihood n={n} T={n_terms} {name}: {runs[name][-1]:.4g} s", file=sys.stderr, flush=True)
        out["log_likelihood"][f"{n}x{n_terms}"] = dict(summary(runs, False), unit="seconds per call", calls_per_window=reps,
                                                       path="split" if traced.use_split(n) else "lane")
        del x
        torch.cuda.empty_cache()

    n, n_terms = RUN_SHAPE
    traced, hand, eager = objects(n_terms)
    legs = (("traced", (traced.prior_transform, traced.log_likelihood)), ("hand_written_hip", (hand.prior_transform, hand.log_likelihood)),
            ("eager_torch", (prior, eager)))

    def timed(cbs):
        s = tp.Sampler(cbs[0], cbs[1], 3, n_particles=n, vectorize=True, clustering=False, random_state=a.seed, backend="torch",
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
        return float(np.sum(steps[beta > 0])) * n / dt

    runs = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, cbs in legs:
            runs[name].append(timed(cbs))
            print(f"sampler n={n} T={n_terms} {name}: {runs[name][-1]:.4g}", file=sys.stderr, flush=True)
    out["sampler"][f"{n}x{n_terms}"] = dict(summary(runs, True), unit="particle-mutation-steps/s")
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
