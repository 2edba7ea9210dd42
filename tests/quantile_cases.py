"""What tests/test_quantile.py (host) and tests/test_quantile_gpu.py (device) share: the fixed sample for tphu_ndtri / tphu_erfinv of
tempest_amd/csrc/quantile.h, its truth from mpmath at 40 digits, the error in ulps, and the measured bounds."""
import functools
import math
import subprocess
from pathlib import Path

import numpy as np

CSRC = Path(__file__).resolve().parent.parent / "tempest_amd" / "csrc"

# The largest error of the HOST build (g++ -O2 -ffp-contract=off, glibc's log) on the sample below against mpmath, in ulps of the
# true value: measured, recorded in DESIGN.md section 11, and asserted as they stand.
NDTRI_HOST_ULP = 5.95           # at p = 2.79e-184 (the far tail); the mean is 0.90
ERFINV_HOST_ULP = 5.36          # at y = -0.4497 (the central region, then the scaling by sqrt(1/2)); the mean is 1.00
# the device's log may differ from the host's in the last place: that moves r = sqrt(-log t) by half an ulp and the result by about one
DEVICE_EXTRA_ULP = 2.0

EDGE_CENTRAL = (0.075, 0.925)                      # |q| = 0.425
EDGE_TAIL = math.exp(-25.0)                        # r = 5

HOST_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "quantile.h"
// argv[1]: a file of doubles; argv[2]: gets tphu_ndtri of each, then tphu_erfinv of each
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<double> in(bytes / sizeof(double)), out(2 * in.size());
  if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 4;
  std::fclose(f);
  for (size_t i = 0; i < in.size(); ++i) {
    out[i] = tphu_ndtri(in[i]);
    out[in.size() + i] = tphu_erfinv(in[i]);
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return 5;
  if (std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 6;
  std::fclose(f);
  return 0;
}
"""


def build_host(directory, name="quantile_host", extra=()):
    """The stand-alone program over quantile.h, built with g++ into `directory`; returns its path."""
    directory = Path(directory)
    src = directory / (name + ".cpp")
    src.write_text(HOST_PROGRAM)
    exe = directory / name
    subprocess.run(["g++", "-O2", "-ffp-contract=off", *extra, f"-I{CSRC}", str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    return exe


def run_host(exe, values, directory):
    """(tphu_ndtri(values), tphu_erfinv(values)) from the program."""
    directory = Path(directory)
    values = np.ascontiguousarray(values, dtype=np.float64)
    fin, fout = directory / (Path(exe).name + ".in"), directory / (Path(exe).name + ".out")
    values.tofile(fin)
    subprocess.run([str(exe), str(fin), str(fout)], check=True, capture_output=True, text=True)
    out = np.fromfile(fout, dtype=np.float64)
    assert out.size == 2 * values.size
    return out[:values.size], out[values.size:]


def _neighbours(v, k=2):
    """The doubles from k below v to k above it."""
    out = [v]
    lo = hi = v
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return sorted(float(x) for x in out)


def edge_runs():
    """Ascending runs of consecutive doubles across every region edge of tphu_ndtri: |q| = 0.425, t = exp(-25) on both sides, p = 0.5."""
    return [np.array(_neighbours(v, 3)) for v in EDGE_CENTRAL + (EDGE_TAIL, 1.0 - EDGE_TAIL, 0.5)]


@functools.lru_cache(maxsize=None)
def sample_p():
    """About 20 000 probabilities in (0, 1), seeded: uniform draws, both 15 % tails, 10^-U(0, 300), 1 - 2^-k, 0.5 +- 10^-U(3, 17), the
    doubles round the region edges, the smallest subnormal, 2^-1022 and 1 - 2^-53."""
    rs = np.random.RandomState(20241020)
    h = 10.0 ** -rs.uniform(3.0, 17.0, 2500)
    parts = [rs.uniform(0.0, 1.0, 10000), rs.uniform(0.0, 0.15, 2000), 1.0 - rs.uniform(0.0, 0.15, 2000),
             10.0 ** -rs.uniform(0.0, 300.0, 3000), 1.0 - 2.0 ** -np.arange(1.0, 54.0), 0.5 + h[:1250], 0.5 - h[1250:],
             np.concatenate(edge_runs()), np.array([5e-324, 2.0 ** -1022, 1.0 - 2.0 ** -53])]
    p = np.concatenate(parts)
    p = p[(p > 0.0) & (p < 1.0)]
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def sample_y():
    """The arguments of tphu_erfinv: 2 p - 1 over the probabilities (those that stay inside (-1, 1)) and +-10^-U(0, 300)."""
    rs = np.random.RandomState(20241021)
    tiny = 10.0 ** -rs.uniform(0.0, 300.0, 1000) * np.where(rs.uniform(size=1000) < 0.5, -1.0, 1.0)
    y = np.concatenate([2.0 * sample_p() - 1.0, tiny])
    y = y[np.abs(y) < 1.0]
    y.setflags(write=False)
    return y


# special arguments and what both functions return for them (torch.special.ndtri's and torch.erfinv's conventions)
SPECIAL_P = np.array([0.0, 1.0, 0.5, 5e-324, -5e-324, -0.0, -0.25, 1.0 + 2.0 ** -52, 2.0, -np.inf, np.inf, np.nan])
SPECIAL_Y = np.array([-1.0, 1.0, 0.0, -0.0, 5e-324, -5e-324, 1.0 + 2.0 ** -52, -1.0 - 2.0 ** -52, 3.0, -np.inf, np.inf, np.nan])


def _truth_ndtri_one(p, x0):
    import mpmath as mp
    p = mp.mpf(p)
    upper = p > 0.5
    t = 1 - p if upper else p                      # exact: 40 digits hold every bit of a double and of 1 - it
    lt = mp.log(t)
    x = mp.findroot(lambda x: mp.log(mp.ncdf(x)) - lt, mp.mpf(-abs(x0)), df=lambda x: mp.npdf(x) / mp.ncdf(x), solver="newton",
                    tol=mp.mpf(10) ** -36, verify=False) if t != 0.5 else mp.mpf(0)
    return -x if upper else x


def _truth_erfinv_one(y, x0):
    import mpmath as mp
    a = abs(mp.mpf(y))
    if a == 0:
        return mp.mpf(0)
    c = 2 / mp.sqrt(mp.pi)
    if a <= 0.5:                                   # log erf(x) = log |y|
        la = mp.log(a)
        x = mp.findroot(lambda x: mp.log(mp.erf(x)) - la, mp.mpf(abs(x0)), df=lambda x: c * mp.exp(-x * x) / mp.erf(x),
                        solver="newton", tol=mp.mpf(10) ** -36, verify=False)
    else:                                          # log erfc(x) = log(1 - |y|), 1 - |y| exact
        lt = mp.log(1 - a)
        x = mp.findroot(lambda x: mp.log(mp.erfc(x)) - lt, mp.mpf(abs(x0)), df=lambda x: -c * mp.exp(-x * x) / mp.erfc(x),
                        solver="newton", tol=mp.mpf(10) ** -36, verify=False)
    return -x if y < 0 else x


def _truth(one, args, start):
    """(the truth rounded to double, the error of `start` against the unrounded truth in ulps of the truth) per argument."""
    import mpmath as mp
    with mp.workdps(40):
        exact = [one(float(a), float(s)) for a, s in zip(args, start)]
        near = np.array([float(x) for x in exact])
        ulp = [mp.mpf(math.ulp(v)) for v in near]
        resid = np.array([float((x - mp.mpf(float(v))) / u) for x, v, u in zip(exact, near, ulp)])
    near.setflags(write=False)
    resid.setflags(write=False)
    return near, resid


@functools.lru_cache(maxsize=None)
def truth_ndtri():
    """(truth to the nearest double, truth - that double in ulps) over sample_p(): mpmath, 40 digits, Phi(x) = p solved on the log
    scale from the replay's value."""
    from tempest_amd.trace import ndtri_host
    return _truth(_truth_ndtri_one, sample_p(), ndtri_host(sample_p()))


@functools.lru_cache(maxsize=None)
def truth_erfinv():
    from tempest_amd.trace import erfinv_host
    return _truth(_truth_erfinv_one, sample_y(), erfinv_host(sample_y()))


def ulp_error(got, truth):
    """|got - truth| in ulps of the truth, the truth given as (nearest double, remainder in ulps): exact where got is within 2^52 ulp."""
    near, resid = truth
    got = np.asarray(got, dtype=np.float64)
    ulp = np.array([math.ulp(v) for v in near])
    return np.abs((got - near) / ulp - resid)
