"""The JSON line bench.py prints (driver contract): checked on the line committed under profiles/ by the last GPU run, and on
the static parts of bench.py that do not need a GPU."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_bench_line_has_the_contract_fields():
    d = json.load(open(os.path.join(ROOT, "profiles", "r03_bench_unprofiled.json")))
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["higher_is_better"] is True and d["scaling"] == "strong" and d["vs_baseline"] is None
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and d["n_gpus"] == 1
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - d["timed_mcmc_steps"] * d["config"]["particles_global"] / (d["ms_per_step"] * d["steps"] * 1e-3)) \
        < 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e9) < 1.0
    assert r["traffic"] is None or 0.9 < r["traffic"] / r["algorithmic_bytes_per_launch"] < 1.5
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    assert abs(d["logz"] - d["analytic_logz"]) < 0.5
    # the extras the docs quote: whole-run figures (cold, and repeated in the same process with the same evidence), the
    # mutation-only rate and the HIP-callback leg on the same schedule
    assert d["whole_run"]["value"] > 0 and d["whole_run_warm"]["same_logz_as_first_run"] is True
    assert d["whole_run_warm"]["iterations"] == d["whole_run"]["iterations"] == d["iterations_total"]
    assert d["whole_run_warm"]["seconds"] < d["whole_run"]["seconds"]
    assert d["mutation_only"]["value"] > d["value"] and d["hip_callbacks"]["same_schedule_as_value_run"] is True
    # round 3: the cold whole run is timed from before the Sampler's construction and says what its start-up cost
    sb = d["whole_run"]["startup_breakdown"]
    assert sb["wall_s_from_construction"] > 0 and "user_callbacks" in sb["threads_s"] and "device_context" in sb["threads_s"]


def test_committed_profiles_are_self_consistent():
    """The evidence under profiles/ that the docs quote: rates follow from bytes and durations, counter traffic is the corrected
    FETCH + WRITE, the roofline kernel's counters match its algorithmic bytes, the A/B set carries its medians."""
    t = json.load(open(os.path.join(ROOT, "profiles", "r03_roofline_table.json")))
    assert t["peak_GBs"] == 8000.0 and len(t["kernels"]) >= 18
    names = " ".join(k["kernel"] for k in t["kernels"])
    for needed in ("k_logmix_append", "k_reweight_reduce<1, 8>", "k_weights", "k_gather_rows", "k_rows_pack", "k_propose_reg", "k_accept",
                   "k_wmom_small", "k_cv_sum_small", "k_membw<0>", "k_membw<1>"):
        assert needed in names, needed
    for k in t["kernels"]:
        if k["algorithmic_bytes_per_launch"]:
            rate = k["algorithmic_bytes_per_launch"] / k["mean_duration_us"] / 1e3
            assert abs(rate - k["achieved_GBs_algorithmic"]) <= 0.01 * rate + 0.1, k["kernel"]
            assert abs(k["frac_of_8TBs"] - k["achieved_GBs_algorithmic"] / 8000.0) < 1e-3
        assert abs(k["counter_bytes_per_launch"] - (k["FETCH_SIZE_bytes_x2"] + k["WRITE_SIZE_bytes"])) < 1.0
    k2 = next(k for k in t["kernels"] if k["kernel"].startswith("void k_reweight_reduce<1, 8>"))
    assert 0.99 < k2["traffic_over_algorithmic"] < 1.02
    rw = json.load(open(os.path.join(ROOT, "profiles", "r03_reweight_pmc.json")))
    assert rw["n_rows"] == 67108864 and 0.999 < rw["traffic_over_algorithmic"] < 1.01
    assert abs(rw["hbm_bytes_per_launch"] - (rw["hbm_read_bytes_per_launch"] + rw["hbm_write_bytes_per_launch"])) < 1.0
    ab = json.load(open(os.path.join(ROOT, "profiles", "r03_bench_131k_ab.json")))
    plain = sorted(r["ms_per_step"] for r in ab["runs"] if r["run"].startswith("plain"))
    comm = sorted(r["ms_per_step"] for r in ab["runs"] if r["run"].startswith("comm"))
    assert len(plain) == 3 and len(comm) == 3 and abs(ab["median_ms_per_step"]["plain"] - plain[1]) < 1e-9
    assert len({r["logz"] for r in ab["runs"]}) == 1                     # the sharded code path changes no bit of the evidence
    assert ab["median_ms_per_step"]["ratio"] < 1.2
    p = json.load(open(os.path.join(ROOT, "profiles", "r02_propose_pmc.json")))
    for scen in ("tight", "mid", "wide"):
        assert p["round2"]["pmc"][scen]["SQ_INSTS_VALU"] < 0.85 * p["round1"]["pmc"][scen]["SQ_INSTS_VALU"]
    p3 = json.load(open(os.path.join(ROOT, "profiles", "r03_propose_pmc.json")))           # the shorter RNG chain, same box
    for scen in ("tight", "mid", "wide"):
        assert p3["this_round"]["pmc"][scen]["SQ_INSTS_VALU"] < 0.95 * p3["previous_round"]["pmc"][scen]["SQ_INSTS_VALU"]
    # the row-walker kernel against the multi-lane kernel on the ensembles from the prior, same box
    runs = json.load(open(os.path.join(ROOT, "profiles", "r03_propose_d50_d100.json")))["runs"]
    med = {(r["lib"], r["kernel"], r["n"], r["d"], r["scenario"], r["variant"], round(r.get("mean_attempts_probe", 0) / 100)): r["median_us"]
           for r in runs}
    for kern in ("rwm", "tpcn"):
        a = [v for k, v in med.items() if k[:6] == ("libtempest_hip.so", kern, 65536, 50, "prior", 3) and k[6] < 2]
        b = [v for k, v in med.items() if k[:6] == ("libtempest_hip.so", kern, 65536, 50, "prior", 5) and k[6] < 2]
        assert a and b and min(b) < 0.6 * min(a), (kern, a, b)


def test_bench_cli_defaults():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert flag in out.stdout + out.stderr          # bench.py routes everything but the JSON line to stderr


import pytest


@pytest.mark.gpu
def test_bench_two_ranks_rehearsal_on_one_gpu(tmp_path):
    """The N > 1 control flow of bench.py (BASELINE config 4 sharded: strong scaling, max-over-ranks timing, the HIP-callback and
    weak-scaling legs, the peer-to-peer layer between two processes) walked on ONE GPU: TEMPEST_AMD_BENCH_REHEARSAL=1 puts every
    rank on cuda:0 over gloo.  The numbers mean nothing; the line must have the contract's shape and the sharded run must agree
    with the one-rank run of the same global ensemble on the evidence."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, TEMPEST_AMD_BENCH_REHEARSAL="1", TEMPEST_AMD_P2P_TIMEOUT="60")
    common = ["--full", "--steps", "2", "--warmup", "1", "--particles", "32768", "--no-roofline", "--no-cpu-baseline"]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                          "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2"] + common,
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert two.returncode == 0, two.stderr[-2000:]
    d2 = json.loads([ln for ln in two.stdout.splitlines() if ln.startswith("{")][-1])
    assert d2["n_gpus"] == 2 and d2["scaling"] == "strong" and "REHEARSAL" in d2["data"]
    assert d2["config"]["particles_global"] == 32768 and d2["config"]["particles_per_gpu"] == 16384
    assert d2["hip_callbacks"]["value"] and d2["hip_callbacks"]["same_schedule_as_value_run"]
    assert d2["weak_scaling"]["particles_global"] == 65536 and d2["weak_scaling"]["value"] > 0
    phases = d2["comm"]["phase_ms_per_iteration_by_rank"]        # every rank's time per phase: which one is the straggler
    assert set(phases) >= {"reweight", "train", "resample", "mutate", "commit"}
    assert all(len(v) == 2 and all(t >= 0.0 for t in v) for v in phases.values()) and max(phases["mutate"]) > 0.0
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--no-hip-callbacks"] + common, capture_output=True,
                         text=True, timeout=600, cwd=ROOT)
    assert one.returncode == 0, one.stderr[-2000:]
    d1 = json.loads([ln for ln in one.stdout.splitlines() if ln.startswith("{")][-1])
    assert d1["iterations_total"] == d2["iterations_total"] and d1["timed_mcmc_steps"] == d2["timed_mcmc_steps"]
    # the sharded sampler is the same sampler: equal to rounding at this size and seed (DESIGN.md section 7 describes the one
    # way two world sizes can part -- a rounding-level tie at the trim percentile -- and where it was seen)
    assert abs(d1["logz"] - d2["logz"]) < 1e-9


@pytest.mark.gpu
def test_bench_four_ranks_rehearsal_with_clustering_on_one_gpu():
    """The N > 1 control flow once more with FOUR ranks and the Sampler's default clustering=True (the clustered working set is
    gathered and the EM runs replicated, labels identical on every rank), all on cuda:0 over gloo: the line carries the `comm`
    block -- world size, backend, the peer-to-peer layer on every rank, collectives and shuffle volume per iteration -- and the
    sharded run ends where the one-rank run of the same global ensemble ends (statistically: see below).  (Eight processes on one card are beyond this pool's process guard; the
    eight-rank run is the driver's.)"""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, TEMPEST_AMD_BENCH_REHEARSAL="1", TEMPEST_AMD_P2P_TIMEOUT="60")
    common = ["--full", "--steps", "2", "--warmup", "1", "--particles", "16384", "--no-roofline", "--no-cpu-baseline", "--clustering",
              "--no-hip-callbacks", "--no-weak", "--no-second-run"]
    four = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr",
                           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "4"] + common,
                          capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert four.returncode == 0, four.stderr[-3000:]
    d4 = json.loads([ln for ln in four.stdout.splitlines() if ln.startswith("{")][-1])
    assert d4["n_gpus"] == 4 and d4["config"]["clustering"] is True and d4["config"]["particles_per_gpu"] == 4096
    c = d4["comm"]
    assert c["world_size"] == 4 and c["backend"] == "gloo" and c["p2p_active_on_every_rank"] is True
    per = c["per_iteration_on_rank0"]
    assert per["p2p_exchanges"] > 5 and per["shuffle_rows"] > 0
    assert abs(per["shuffle_bytes"] - per["shuffle_rows"] * 22 * 8) < 200          # records of 2 d + 2 doubles (both figures rounded)
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert one.returncode == 0, one.stderr[-3000:]
    d1 = json.loads([ln for ln in one.stdout.splitlines() if ln.startswith("{")][-1])
    assert "comm" not in d1
    # With clustering the two world sizes are two runs of the same sampler, not the same run: the recursive BIC split search
    # makes a discrete decision per candidate split from moment sums that the ranks form in a different order, and Rosenbrock
    # sits on such ties (K ~ 14 clusters; without clustering the two-rank test above pins the evidence to 1e-9).  Same schedule
    # length, evidences a few hundredths apart (seed-to-seed sigma of this target: 0.07-0.12), both near the analytic value.
    assert abs(d1["iterations_total"] - d4["iterations_total"]) <= 2
    assert abs(d1["logz"] - d4["logz"]) < 0.4, (d1["logz"], d4["logz"])
    assert abs(d4["logz"] - d4["analytic_logz"]) < 1.2 and abs(d1["logz"] - d1["analytic_logz"]) < 1.2


@pytest.mark.gpu
def test_bench_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
    """A plain run (no --full) prints the headline fields and none of the legs that take runs of their own; --steps sets the
    number of timed steps; --dump-outputs writes the state the last timed step returned as float64 .npy files (within 64 MB),
    and a second run with the same arguments writes the same arrays."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lines = []
    for run in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                              "--particles", "32768", "--dump-outputs", str(tmp_path / run)],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines.append(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]))
    d = lines[0]
    assert d["steps"] == 3 and d["timed_iterations"] == 3 and d["warmup"] == 1
    first, last = d["timed_iteration_range_of_run"]
    assert last - first + 1 == 3
    assert d["higher_is_better"] is True and d["dtype"] == "f64" and d["unit"] == "particle-mutation-steps/s"
    assert abs(d["value"] - d["timed_mcmc_steps"] * d["config"]["particles_global"] / (d["ms_per_step"] * d["steps"] * 1e-3)) \
        < 1e-6 * d["value"]
    for key in ("roofline", "cpu_baseline", "hip_callbacks", "whole_run", "whole_run_warm", "mutation_only", "digest", "logz"):
        assert key not in d, key
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"u.npy", "x.npy", "logl.npy", "rows.npy", "beta.npy", "logz.npy"} <= set(names)
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 * 2 ** 20
    u = np.load(tmp_path / "a" / "u.npy")
    assert u.shape == (32768, 10) and np.load(tmp_path / "a" / "logl.npy").shape == (32768,)
    assert 0.0 < float(np.load(tmp_path / "a" / "beta.npy")) <= 1.0
    for n in names:
        va, vb = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert va.dtype in (np.float32, np.float64), n
        np.testing.assert_array_equal(va, vb, err_msg=n)


def test_bench_rank_that_fails_exits_nonzero_at_once(tmp_path):
    """bench.py's failure path: an exception anywhere ends the rank with exit code 1 through os._exit (no interpreter shutdown
    that could wait on a dead communicator, no re-exec).  Exercised without a GPU: WORLD_SIZE disagrees with --gpus."""
    env = dict(os.environ, WORLD_SIZE="3")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True, timeout=300,
                         env=env, cwd=ROOT)
    assert out.returncode != 0 and "WORLD_SIZE" in (out.stderr + out.stdout)
