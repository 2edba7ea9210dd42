"""User callbacks as HIP device functions, compiled into the MCMC step.

    cb = tempest_amd.HipCallbacks(n_dim=10, source='''
        __device__ void prior_transform(const double* u, double* x) {
          for (int j = 0; j < N_DIM; ++j) x[j] = 20.0 * u[j] - 10.0;
        }
        __device__ double log_likelihood(const double* x) {
          double s = 0.0;
          for (int j = 0; j < N_DIM; j += 2) {
            double a = x[j] * x[j] - x[j + 1], b = x[j] - 1.0;
            s += 10.0 * a * a + b * b;
          }
          return -s;
        }''')
    sampler = tempest_amd.Sampler(cb.prior_transform, cb.log_likelihood, 10, vectorize=True, ...)

`cb.prior_transform` / `cb.log_likelihood` are ordinary vectorised callbacks (torch-ROCm tensors or NumPy arrays in,
the same kind out), so everything that calls them generically keeps working; when a Sampler is given BOTH from the same
object, the mutation step skips them and launches the plugin's fused kernel instead (proposal -> [x' = prior(u'),
l' = loglike(x'), Metropolis update] -> adaptation: three launches per step instead of a chain of elementwise ones).

The source is compiled with hipcc for gfx950 into a shared library cached by content hash (in-tree under
tempest_amd/_plugins/ when writable, else ~/.cache/tempest_amd/plugins).  The reference has no counterpart: its
callbacks are Python functions evaluated on the host (mcmc.py:152-160, core.py:317-358).
"""
import ctypes as C
from collections import namedtuple
import hashlib
import keyword
import math
import os
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from ._cdecl import prototypes
from ._lib import HEADER_PATH, TempestHipError
from .device import TAG_REP_NORMAL, TAG_REP_UNIFORM

_CSRC = Path(__file__).resolve().parent / "csrc"
_TEMPLATE = _CSRC / "user_plugin.hip.in"
_ARCH = "gfx950"
_FLAGS = ["-O3", "-std=c++17", "-fPIC", "-shared", f"--offload-arch={_ARCH}", "-ffp-contract=on", "-Wno-unused-function"]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise TempestHipError("HipCallbacks needs hipcc (set HIPCC or install ROCm) to compile the user source")


def _cache_dirs():
    yield Path(__file__).resolve().parent / "_plugins"
    yield Path(os.environ.get("XDG_CACHE_HOME", Path.home() / ".cache")) / "tempest_amd" / "plugins"
    yield Path(tempfile.gettempdir()) / "tempest_amd_plugins"


# The order of the sum over observations (log_likelihood_term): chunks of SUM_LAYOUT[0] consecutive terms, blocks of SUM_LAYOUT[1]
# consecutive chunk sums, the block sums in order.  Design constants of the template: changing them changes
# the bits of every term-form likelihood.
SUM_LAYOUT = (256, 64)

# Which of the two evaluations of a term-form likelihood runs: the split kernel (k_user_like_split) in the first band whose
# n_terms_min is reached, below that band's particle count; the lane-per-particle kernels elsewhere.  Both give the same bits, so
# this table decides time only.  Measured on one MI355X with tools/bench_data_like.py: from 1000 terms on the split kernel takes
# 0.03-0.4x the lane path's time up to 16 384 particles (0.01-0.18x at 100 000 terms), 0.5-0.77x at 65 536, and the two tie (0.88-1.0x) at
# 262 144, where the lane path fills the machine by itself; at 100 terms the lane path wins at every size (1.0-2.8x).  Not
# measured between 100 and 1000 terms: the lane path keeps that ground.
DATA_LIKE_THRESHOLDS = {
    "source": "profiles/data_like_sweep.json (tools/bench_data_like.py: cheap and dear term, n = 256 ... 1 048 576, n_terms = 1e2 ... 1e6)",
    # (n_terms_min, split below this many particles) -- the first row whose n_terms_min <= n_terms
    "bands": ((1_000, 262_144),),
    # split kernel: the particle tile of a workgroup is quartered (64 -> 16 -> 4) while the grid has fewer workgroups than this
    # (the CUs of the device the sweep ran on): 256 particles x 100 000 terms took 707 / 142 / 118 us with 64 / 16 / 4 (64 pinned in an earlier run of the tool)
    "min_workgroups": 256,
}

_MAX_TABLES = 64
# derived(x, out): the N_DERIVED values of a row are registers of the lane that owns it, beside the row's N_DIM
MAX_DERIVED = 32
# rows per workgroup of the row-major derived kernel (k_user_derived): the largest whose two LDS images -- rows x (n_dim | 1) and
# rows x (n_derived | 1) doubles -- fit DERIVED_LDS_BYTES; none fits: the direct (lane per row) kernel.  The template's rule, restated.
DERIVED_TILES = (256, 128, 64)
DERIVED_LDS_BYTES = 65536
_RESERVED = ("n_terms",)

# predict(x, r): the order of the sums over rows behind predictive()'s mean and var -- chunks of PREDICT_SUM_LAYOUT[0] consecutive
# rows (a wave: its 64 values are added by the shuffle tree v[:h] + v[h:2h], h = 32, 16, ... 1), blocks of PREDICT_SUM_LAYOUT[1]
# consecutive chunk sums in chunk order, the block sums in block order.  Design constants of the template.
PREDICT_SUM_LAYOUT = (64, 16)
MAX_QUANTILES = 8
PREDICT_MAX_TILE = 64              # indices per workgroup, at most (TPHU_PRED_RT)
PREDICT_TABLES = 24                # (index, quantile) bucket tables a workgroup of the select keeps in LDS (TPHU_PRED_TAB)
# Tile rule of predictive(): halve the indices per workgroup from 64 while the moment kernel's grid -- row blocks x index tiles -- has
# fewer workgroups than this (4 per CU of a 256-CU device), and cut the rows into as many slabs for the select as bring its grid
# there.  Chosen by that count alone, WITHOUT a run of tools/bench_predictive.py on the device behind it; the tile and the slab
# decide time only, never a bit of the result.
PREDICT_MIN_WORKGROUPS = 1024
PREDICT_SCRATCH_WORDS = 1 << 23    # 64 MiB of batch scratch at most: more indices than fit go through in batches

# pointwise(): its sums over rows run in PREDICT_SUM_LAYOUT too.  Tile rule: halve the indices per workgroup from 64 while the grid of
# its two sweeps -- row blocks x index tiles -- has fewer workgroups than this (4 per CU of a 256-CU device).  Chosen by that count
# alone, WITHOUT a timing on the device behind it; the tile decides time only, never a bit of the result.
POINTWISE_MAX_TILE = 64            # indices per workgroup, at most (TPHU_PW_RT)
POINTWISE_MIN_WORKGROUPS = 1024
POINTWISE_SCRATCH_WORDS = 1 << 23  # 64 MiB of batch scratch at most: more indices than fit go through in batches
# replicated(): the noise of replicate(x, r, g) is Philox at (item = row, draw = k >> 1, tick = r, tag), these two tags for g.normal /
# g.uniform (the tags are one number space: device.py); its sums over rows run in PREDICT_SUM_LAYOUT, discrepancy's sum over
# r in SUM_LAYOUT; tiles by predict_tiles.
REPLICATE_TAGS = (TAG_REP_NORMAL, TAG_REP_UNIFORM)
POINTWISE_KEYS = ("lppd", "mean", "p_waic", "elpd_waic", "elpd_loo", "ess_loo")      # the rows of tphu_pointwise's output
# psis_loo(): Pareto-smoothed importance-sampling LOO over equally weighted rows.  The tail of an observation -- its
# ceil(min(0.2 n, 3 sqrt(n))) largest ratios, at most PSIS_MAX_TAIL (TPHU_PSIS_MAXTAIL: what a workgroup of the fit sorts in LDS; n up to
# 1 864 135 rows is not clamped), none below PSIS_MIN_TAIL -- is sorted and refitted by one workgroup; body sums run in PREDICT_SUM_LAYOUT,
# tiles by pointwise_tiles, the select's slab by predict_tiles.  Neither decides a bit of the result.
PSIS_MAX_TAIL = 4096
PSIS_MIN_TAIL = 5
PSIS_SCRATCH_WORDS = 1 << 23       # 64 MiB of batch scratch at most: more indices than fit go through in batches
PSIS_KEYS = ("pareto_k", "elpd_psis", "ess_psis")                                     # the rows of tphu_psis's output


def prefer_split(n: int, n_terms: int) -> bool:
    for t_min, n_below in DATA_LIKE_THRESHOLDS["bands"]:
        if n_terms >= t_min:
            return n < n_below
    return False


def derived_tiles(n_dim: int, n_derived: int):
    """The LDS tiles (rows per workgroup) the row-major derived kernel can take at this shape, largest first; () where it falls
    back to the direct kernel."""
    return tuple(r for r in DERIVED_TILES if r * ((n_dim | 1) + (n_derived | 1)) * 8 <= DERIVED_LDS_BYTES)


# the optional callbacks of a source: what defines one, and what its extent argument n_<name>= is
_OPTIONAL = {"derived": ("void derived(const double* x, double* out)", "how many values it writes"),
             "predict": ("double predict(const double* x, int64_t r)", "an int, or the name of a data entry"),
             "replicate": ("double replicate(const double* x, int64_t r, const tphu_noise& g)", "an int, or the name of a data entry"),
             "discrepancy": ("double discrepancy(const double* x, int64_t r, double y)", None)}


def _defines(source: str, name: str) -> bool:
    """The source DEFINES the optional callback `name` (`void derived(`, `double predict(`, ...): the word alone, in a comment or a
    name, is not a definition."""
    return re.search(rf"\b{_OPTIONAL[name][0].split()[0]}\s+{name}\s*\(", source) is not None


def _defined_and_given(source: str, name: str, given) -> bool:
    """_defines, for a callback that goes with an argument n_<name>=: one without the other is refused."""
    has = _defines(source, name)
    if has and given is None:
        raise ValueError(f"HipCallbacks: the source defines {name}(...): give n_{name}= ({_OPTIONAL[name][1]})")
    if given is not None and not has:
        raise ValueError(f"HipCallbacks: n_{name}= goes with a source that defines __device__ {_OPTIONAL[name][0]}")
    return has


def _extent(v, what, host, prefix="HipCallbacks", below=None, of_an_entry=False) -> int:
    """`what`= as an extent: the name of a data entry (its length, or its rows), or a positive int [below `below`] [that some entry
    has as that extent]."""
    if isinstance(v, str):
        if v not in host:
            raise ValueError(f"{prefix}: {what}={v!r} names no data entry")
        return int(host[v].shape[0])
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) <= 0 or (below is not None and int(v) >= below):
        raise ValueError(f"{prefix}: {what} must be a positive int or the name of a data entry, got {v!r}")
    if of_an_entry and not any(a.shape[0] == int(v) for a in host.values()):
        raise ValueError(f"{prefix}: {what}={int(v)} is the length (or the number of rows) of no data entry: the traced function "
                         "has nothing to read per term")
    return int(v)


def _check_n_derived(source, n_derived) -> int:
    if not _defined_and_given(source, "derived", n_derived):
        return 0
    if isinstance(n_derived, bool) or not isinstance(n_derived, (int, np.integer)) or not 0 < int(n_derived) <= MAX_DERIVED:
        raise ValueError(f"HipCallbacks: n_derived must be a positive int, at most {MAX_DERIVED}, got {n_derived!r}")
    return int(n_derived)


def _check_n_replicate(source, n_replicate, observed, host):
    """(n_replicate, name of the observed entry or None, the source has discrepancy()) of a checked HipCallbacks(n_replicate=, observed=)."""
    disc = _defines(source, "discrepancy")
    if not _defined_and_given(source, "replicate", n_replicate):
        if observed is not None:
            raise ValueError("HipCallbacks: observed= goes with a source that defines replicate(...) (and n_replicate=)")
        if disc:
            raise ValueError("HipCallbacks: the source defines discrepancy(...): it goes with a source that defines replicate(...) "
                             "(and n_replicate=, observed=)")
        return 0, None, False
    n_rep = _extent(n_replicate, "n_replicate", host, below=2 ** 31)
    if observed is not None:
        if not isinstance(observed, str) or observed not in host:
            raise ValueError(f"HipCallbacks: observed={observed!r} names no data entry")
        if host[observed].ndim != 1 or host[observed].shape[0] != n_rep:
            raise ValueError(f"HipCallbacks: observed={observed!r} must be a 1-D data entry of length n_replicate = {n_rep}, got shape "
                             f"{host[observed].shape}")
    elif disc:
        raise ValueError("HipCallbacks: the source defines discrepancy(...): give observed= (the name of the data entry it is compared on)")
    return n_rep, observed, disc


def _row_blocks(n: int) -> int:
    """Blocks of PREDICT_SUM_LAYOUT[0] x PREDICT_SUM_LAYOUT[1] consecutive rows that n rows make."""
    return -(-n // (PREDICT_SUM_LAYOUT[0] * PREDICT_SUM_LAYOUT[1]))


def _batched_words(fixed: int, per_r: int, count: int, cap: int) -> int:
    """8-byte words of a driver's scratch: its `fixed` words and `per_r` for each index of a batch -- all `count` indices, or as many as
    `cap` words hold (one at least).  The plugin's drivers divide what they get by the same two numbers (tphu_plan)."""
    return fixed + per_r * min(count, max(1, cap // per_r))


def _halved_tile(n: int, count: int, max_tile: int, min_workgroups: int) -> int:
    """Indices per workgroup of a sweep over row blocks x index tiles: halved from max_tile while the grid has fewer workgroups than
    min_workgroups."""
    n_blocks, tile = _row_blocks(n), max_tile
    while tile > 1 and n_blocks * -(-count // tile) < min_workgroups:
        tile //= 2
    return tile


def replicate_scratch_words(n: int, n_replicate: int, n_q: int) -> int:
    """8-byte words of scratch tphu_replicated gets for this call: W, the block sums of w, sum k, the p-value count, the PIT counters,
    the chunk and block sums of u T, and for a batch of indices what predictive() keeps -- all n_replicate indices, or as many as
    PREDICT_SCRATCH_WORDS hold."""
    n_blocks = _row_blocks(n)
    return _batched_words(3 + 3 * n_blocks + 3 * n_replicate + 2 * -(-n // PREDICT_SUM_LAYOUT[0]), n_blocks + 258 * n_q + 1, n_replicate,
                          PREDICT_SCRATCH_WORDS)


def predict_tiles(n: int, n_predict: int, n_q: int):
    """(indices per workgroup, rows per workgroup of the select) predictive() launches with: the rule of PREDICT_MIN_WORKGROUPS."""
    tile = _halved_tile(n, n_predict, PREDICT_MAX_TILE, PREDICT_MIN_WORKGROUPS)
    rts = max(1, min(tile, PREDICT_TABLES // max(1, n_q)))
    slabs = max(1, min(-(-n // 256), -(-PREDICT_MIN_WORKGROUPS // -(-n_predict // rts))))
    return tile, max(256, -(-(-(-n // slabs)) // 256) * 256, -(-(-(-n // 65535)) // 256) * 256)


def predict_scratch_words(n: int, n_predict: int, n_q: int) -> int:
    """8-byte words of scratch tphu_predictive gets for this call: W and the block sums of w, and for a batch of indices the block
    sums, bucket totals, prefixes, targets and NaN flags -- all n_predict indices, or as many as PREDICT_SCRATCH_WORDS hold."""
    n_blocks = _row_blocks(n)
    return _batched_words(1 + n_blocks, n_blocks + 258 * n_q + 1, n_predict, PREDICT_SCRATCH_WORDS)


def pointwise_tiles(n: int, n_terms: int) -> int:
    """Indices per workgroup pointwise() launches with: the rule of POINTWISE_MIN_WORKGROUPS."""
    return _halved_tile(n, n_terms, POINTWISE_MAX_TILE, POINTWISE_MIN_WORKGROUPS)


def pointwise_scratch_words(n: int, n_terms: int) -> int:
    """8-byte words of scratch tphu_pointwise gets for this call: W and the block sums of w, and for a batch of indices four arrays
    of block values and the two shifts -- all n_terms indices, or as many as POINTWISE_SCRATCH_WORDS hold."""
    n_blocks = _row_blocks(n)
    return _batched_words(1 + n_blocks, 4 * n_blocks + 2, n_terms, POINTWISE_SCRATCH_WORDS)


def psis_tail_len(n: int) -> int:
    """The tail length M of psis_loo() over n rows: ceil(min(0.2 n, 3 sqrt(n))), at most PSIS_MAX_TAIL; below PSIS_MIN_TAIL nothing is
    smoothed."""
    return min(int(math.ceil(min(0.2 * n, 3.0 * math.sqrt(n)))), PSIS_MAX_TAIL)


def psis_k_threshold(n: int) -> float:
    """The pareto_k above which an estimate from n rows is not to be trusted: min(1 - 1 / log10(n), 0.7)."""
    return min(1.0 - 1.0 / math.log10(n), 0.7) if n > 1 else float("-inf")


def psis_scratch_words(n: int, n_terms: int) -> int:
    """8-byte words of scratch tphu_psis gets for this call: W and the block sums of w, and for a batch of indices the bucket totals,
    prefix, target, NaN flag, slot counter, cut, mean and the two shifts (264 words), three arrays of block values and the tail's M
    slots -- all n_terms indices, or as many as PSIS_SCRATCH_WORDS hold."""
    n_blocks, tail = _row_blocks(n), psis_tail_len(n)
    return _batched_words(1 + n_blocks, 3 * n_blocks + 264 + (tail if tail >= PSIS_MIN_TAIL else 0), n_terms, PSIS_SCRATCH_WORDS)


def compare_pointwise(a, b, key="elpd_loo"):
    """Two models on the SAME observations by a pointwise value (`key` of what pointwise() returned for each, or two arrays):
    {"diff": sum (a - b), "se": sqrt(n x the population variance of a - b), "n"}.  Unequal lengths are refused."""
    va, vb = (np.asarray(v[key] if isinstance(v, dict) else v, dtype=np.float64) for v in (a, b))
    if va.ndim != 1 or va.shape != vb.shape or va.size == 0:
        raise ValueError(f"compare_pointwise: expected two (n,) arrays of the same observations, got {va.shape} and {vb.shape}")
    with np.errstate(invalid="ignore", over="ignore"):
        d = va - vb
        return {"diff": _total(d), "se": float(np.sqrt(d.size * np.var(d))), "n": int(d.size)}


def _total(v) -> float:
    """The sum of pointwise values: exact (math.fsum); +inf beside -inf among them: what a plain sum makes of them."""
    try:
        return math.fsum(v)
    except (ValueError, OverflowError):
        with np.errstate(invalid="ignore", over="ignore"):
            return float(np.sum(v))


def psis_totals(res, k_threshold) -> dict:
    """The totals of psis_loo()'s pointwise arrays: elpd_psis, elpd_psis_se, n_high_k (a NaN or infinite pareto_k counts)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return {"elpd_psis": _total(res["elpd_psis"]), "elpd_psis_se": float(np.sqrt(len(res["elpd_psis"]) * np.var(res["elpd_psis"]))),
                "n_high_k": int(np.sum(~(res["pareto_k"] <= k_threshold)))}


def _quantiles(quantiles, what):
    """The quantile levels of predictive() / replicated() as a checked float64 array."""
    qs = np.atleast_1d(np.asarray(quantiles, dtype=np.float64))
    if qs.ndim != 1 or len(qs) > MAX_QUANTILES or not np.all((qs >= 0.0) & (qs <= 1.0)):
        raise ValueError(f"{what}: quantiles must be at most {MAX_QUANTILES} numbers in [0, 1], got {quantiles!r}")
    return qs


def _table_spec(data):
    """Validated ((name, rank), ...) and the float64 host arrays of a `data=` mapping (insertion order)."""
    if not isinstance(data, dict):
        raise ValueError(f"data must be a dict of name -> array, got {type(data).__name__}")
    if len(data) > _MAX_TABLES:
        raise ValueError(f"data: at most {_MAX_TABLES} entries")
    spec, arrays, members = [], {}, set(_RESERVED)
    for name, a in data.items():
        if not isinstance(name, str) or not re.fullmatch(r"[A-Za-z_][A-Za-z0-9_]*", name) or keyword.iskeyword(name) \
                or name in _C_KEYWORDS:
            raise ValueError(f"data: {name!r} is not a usable C identifier")
        arr = _host_array(name, a)
        mine = (name, name + "_len") if arr.ndim == 1 else (name, name + "_rows", name + "_cols")
        clash = members.intersection(mine)
        if clash:
            raise ValueError(f"data: entry {name!r} collides with the generated member {sorted(clash)[0]!r} of tphu_data")
        members.update(mine)
        spec.append((name, arr.ndim))
        arrays[name] = arr
    return tuple(spec), arrays


_C_KEYWORDS = frozenset("""auto bool break case char class const continue default delete do double else enum extern float for friend
goto if inline int long namespace new operator private protected public register return short signed sizeof static struct switch
template this typedef union unsigned using virtual void volatile while""".split())


def _host_array(name, a):
    """One data entry as a C-contiguous float64 NumPy array (1-D or 2-D, not empty)."""
    try:
        import torch
        if isinstance(a, torch.Tensor):
            if a.is_complex() or a.dtype == torch.bool:
                raise ValueError(f"data[{name!r}]: expected real numbers, got {a.dtype}")
            a = a.detach().to("cpu", torch.float64).numpy()
    except ImportError:
        pass
    try:
        arr = np.asarray(a)
    except Exception as e:
        raise ValueError(f"data[{name!r}]: not an array ({e})")
    if arr.dtype == object or not (np.issubdtype(arr.dtype, np.floating) or np.issubdtype(arr.dtype, np.integer)):
        raise ValueError(f"data[{name!r}]: expected real numbers, got dtype {arr.dtype}")
    if arr.ndim not in (1, 2):
        raise ValueError(f"data[{name!r}]: expected a 1-D or 2-D array, got {arr.ndim}-D")
    if arr.size == 0:
        raise ValueError(f"data[{name!r}]: empty array")
    return np.ascontiguousarray(arr, dtype=np.float64)


def _struct_text(tables) -> str:
    lines = ["struct tphu_data {"]
    for name, rank in tables:
        lines.append(f"  const double* {name};")
        lines.append(f"  int64_t {name}_len;" if rank == 1 else f"  int64_t {name}_rows, {name}_cols;      // row-major")
    lines.append("  int64_t n_terms;      // terms of the sum (log_likelihood_term form), else 0")
    lines.append("};")
    return "\n".join(lines)


_PREDICT_LAYOUT = PREDICT_SUM_LAYOUT + (PREDICT_MAX_TILE, PREDICT_TABLES)
# the entry points every plugin has; their prototypes, like those of the parts' entries, are read from the plugin's text (_Parts.bind)
_ENTRIES = ("tphu_last_error", "tphu_prior", "tphu_like", "tphu_accept", "tphu_step", "tphu_run")


# One optional part of a plugin -- everything the host knows about it; a new part is a new row of _PARTS and a field of _Parts.
# name: the field of _Parts that says whether a plugin has it; mark: its lines of the template, dropped whole without it; define, word:
# what it adds to the compiler's command line and to the cache key -- present only with the part, so every other source keeps its file
# name; entry: its entry point, which the plugin must export; report, layout, mismatch: the handshake -- tphu_*_layout(i), or one
# exported function per figure, the tuple they must return [as a function of (n_dim, parts)], and what "does / do not match this
# package" otherwise.
_Part = namedtuple("_Part", "name mark define word entry report layout mismatch", defaults=(None, None, None, None))
_PARTS = (
    _Part("term", "//@T", None, "", "tphu_like_split"),
    _Part("n_derived", "//@X", "-DN_DERIVED={n_derived}", "|derived={n_derived}", "tphu_derived",
          ("tphu_n_derived", "tphu_derived_rows"), lambda n_dim, p: (p.n_derived, (derived_tiles(n_dim, p.n_derived) or (0,))[0]),
          "derived() shape or tile rule does"),
    _Part("predict", "//@P", "-DTPHU_PREDICT", "|predict", "tphu_predictive",
          "tphu_predict_layout", _PREDICT_LAYOUT, "predict() sum layout or tile limits do"),
    _Part("pointwise", "//@W", "-DTPHU_POINTWISE", "|pointwise", "tphu_pointwise",
          "tphu_pointwise_layout", PREDICT_SUM_LAYOUT + (POINTWISE_MAX_TILE,), "pointwise sum layout or tile limit does"),
    _Part("psis", "//@K", "-DTPHU_PSIS", "|psis", "tphu_psis",
          "tphu_psis_layout", PREDICT_SUM_LAYOUT + (POINTWISE_MAX_TILE, PREDICT_TABLES, PSIS_MAX_TAIL), "psis sum layout, tile limits or tail limit do"),
    _Part("replicate", "//@Y", "-DTPHU_REPLICATE", "|replicate", "tphu_replicated",
          "tphu_replicate_layout", _PREDICT_LAYOUT + SUM_LAYOUT + REPLICATE_TAGS, "replicate() sum layouts, tile limits or RNG tags do"),
    _Part("discrepancy", None, "-DTPHU_DISCREPANCY", "|discrepancy"),
)


class _Parts(namedtuple("_Parts", "tables term n_derived predict pointwise replicate discrepancy traced psis",
                        defaults=(None, False, 0, False, False, False, False, False, False))):
    """What a plugin has beside the two callbacks of x: the record every difference between two plugins derives from -- the template
    lines kept, the -D list, the words of the key, the entry points bound and the layouts checked.  tables None: callbacks of x alone
    (the template as it always was, byte for byte); ((name, rank), ...): the callbacks take `const tphu_data& D` and every kernel and
    entry point carries the table; term: the source gives log_likelihood_term and the library owns the sum; n_derived > 0: it gives
    derived(x, out) (k_user_derived / tphu_derived); predict: predict(x, r) (the k_user_predict_* kernels / tphu_predictive);
    pointwise (term form only): the k_user_pw_* kernels / tphu_pointwise; replicate: replicate(x, r, g) (tphu_noise, the k_user_rep_*
    kernels / tphu_replicated), with discrepancy where the source also gives discrepancy(); traced: the source calls the helpers of
    tempest_amd.trace (tphu_tr_max / tphu_tr_min); psis (with pointwise, which then was given as "psis"): the k_user_psis_* kernels /
    tphu_psis."""
    __slots__ = ()

    @classmethod
    def of(cls, source, tables=None, term=False, n_derived=0, predict=False, pointwise=False, replicate=False, discrepancy=False):
        return cls(() if term and tables is None else tables, bool(term), max(0, int(n_derived)), bool(predict), bool(pointwise),
                   bool(replicate), bool(replicate and discrepancy), re.search(r"\btphu_tr_(max|min)\s*\(", source) is not None,
                   isinstance(pointwise, str) and pointwise == "psis")

    def build_args(self) -> dict:          # the keyword arguments of build_plugin that give this record back
        args = {k: v for k, v in self._asdict().items() if k not in ("traced", "psis")}
        if self.psis:                      # the level travels in `pointwise`
            args["pointwise"] = "psis"
        return args

    def present(self):
        return [part for part in _PARTS if getattr(self, part.name)]

    def text(self, source: str) -> str:
        """The translation unit for `source`."""
        # lines of one part only are dropped whole without it; //@D: the data form; //@Q: what predict, pointwise and replicate share --
        # the layout constants, the row loads, the sum of the weights, and on the host the batch plan, the scratch carver and the weight
        # sum of their drivers; //@S: what predict, replicate and psis share -- the ONE body of the moment kernels and of the select's
        # pass (the parts' kernels of those names are wrappers that hand it their row value), the fold of the block sums, the select's key
        # and its narrowing kernel, and on the host the quantile check, the moment pair and the select loop; //@R: the helpers a traced
        # source calls
        rows = self.predict or self.pointwise or self.replicate
        keep = {"//@D": self.tables is not None, "//@S": self.predict or self.replicate or self.psis, "//@Q": rows, "//@R": self.traced}
        keep.update((part.mark, bool(getattr(self, part.name))) for part in _PARTS if part.mark)
        out = []
        for line in _TEMPLATE.read_text().split("\n"):
            if line[:4] in keep and line[4:5] in ("", " "):
                if keep[line[:4]]:
                    out.append(line[5:])
            else:
                out.append(line)
        text = "\n".join(out)
        on = self.tables is not None
        for mark, val in (("@D_PARAM@", ", const tphu_data D"), ("@D_REF@", ", const tphu_data& Dt"), ("@D_TARG@", ", Dt"), ("@D_ARG@", ", D"),
                          ("@D_HOST@", ", const tphu_data* Dh"), ("@D_LAUNCH@", ", *Dh"), ("@D_KARG@", ", (void*)Dh"),
                          ("@D_NONNULL@", " && Dh")):
            text = text.replace(mark, val if on else "")
        if on:
            text = text.replace("@DATA_STRUCT@", _struct_text(self.tables))
        if self.term or self.replicate:
            text = text.replace("@TPHU_CHUNK@", str(SUM_LAYOUT[0])).replace("@TPHU_BLOCK@", str(SUM_LAYOUT[1]))
        if rows:
            text = text.replace("@TPHU_PCHUNK@", str(PREDICT_SUM_LAYOUT[0])).replace("@TPHU_PBLOCK@", str(PREDICT_SUM_LAYOUT[1]))
        return text.replace("@USER_SOURCE@", source)

    def defines(self, n_dim: int):
        return [f"-DN_DIM={int(n_dim)}"] + [part.define.format(**self._asdict()) for part in self.present() if part.define]

    def key(self, n_dim: int) -> str:
        """What build_plugin hashes beside the text and the headers: dimension, architecture, flags, toolchain, a word per part."""
        return f"|{n_dim}|{_ARCH}|{' '.join(_FLAGS)}|{_toolchain_id()}" + "".join(part.word.format(**self._asdict()) for part in self.present())

    def bind(self, lib, n_dim: int, path, text: str):
        """Declare the entry points of the loaded plugin from `text`, the translation unit it was compiled from (its extern "C"
        block says what each takes, the trailing tphu_data pointer of a data-carrying plugin included), and check that it was built
        for this package's layouts; returns the ctypes type of tphu_data (None without tables)."""
        struct = None
        if self.tables is not None:            # a data-carrying plugin: every entry point takes the host copy of tphu_data last
            fields = [f for name, rank in self.tables for f in
                      [(name, C.c_void_p)] + [(name + end, C.c_int64) for end in (("_len",) if rank == 1 else ("_rows", "_cols"))]]
            struct = type("tphu_data", (C.Structure,), {"_fields_": fields + [("n_terms", C.c_int64)]})
            if lib.tphu_data_abi() != 1 or lib.tphu_data_size() != C.sizeof(struct):
                raise TempestHipError(f"plugin {path}: data table layout does not match this package")
        declared = prototypes(text, "tphu_")
        for name in _ENTRIES + tuple(part.entry for part in self.present() if part.entry):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = declared[name]
        if lib.tphu_n_dim() != n_dim:
            raise TempestHipError(f"plugin {path} was built for n_dim={lib.tphu_n_dim()}")
        for part in self.present():            # every exported figure is an int, ctypes' default
            if part.report is not None:
                want = part.layout(n_dim, self) if callable(part.layout) else part.layout
                got = tuple(getattr(lib, part.report)(i) for i in range(len(want))) if isinstance(part.report, str) \
                    else tuple(getattr(lib, name)() for name in part.report)
                if got != want:
                    raise TempestHipError(f"plugin {path}: {part.mismatch} not match this package")
        return struct


def plugin_source(source: str, tables=None, term: bool = False, *, derived: bool = False, predict: bool = False,
                  pointwise: bool = False, replicate: bool = False) -> str:
    """The translation unit for `source` with these parts (see _Parts)."""
    return _Parts.of(source, tables, term, int(derived), predict, pointwise, replicate).text(source)


_TOOLCHAIN = None


def _toolchain_id() -> str:
    """What identifies the compiler for the cache key: `hipcc --version` (a plugin shares struct layouts and inlined device
    code with libtempest_hip: a cached object from another toolchain must not be picked up silently)."""
    global _TOOLCHAIN
    if _TOOLCHAIN is None:
        try:
            r = subprocess.run([_hipcc(), "--version"], capture_output=True, text=True, timeout=60)
            _TOOLCHAIN = (r.stdout + r.stderr).strip() or "unknown"
        except Exception:
            _TOOLCHAIN = "unknown"
    return _TOOLCHAIN


def plugin_key(n_dim: int, *, n_derived: int = 0, predict: bool = False, pointwise: bool = False, replicate: bool = False,
               discrepancy: bool = False) -> str:
    """The cache key of a plugin with these parts beside the text and the headers (see _Parts.key)."""
    return _Parts.of("", None, False, n_derived, predict, pointwise, replicate, discrepancy).key(n_dim)


def build_plugin(source: str, n_dim: int, verbose: bool = False, tables=None, term: bool = False, *, n_derived: int = 0,
                 predict: bool = False, pointwise: bool = False, replicate: bool = False, discrepancy: bool = False) -> Path:
    """Compile (or find in the cache) the plugin for `source`; returns the path of the shared library.  The arguments after
    `verbose` are the fields of _Parts: names, ranks and the element type of the data entries are in the generated text and so in
    the key; values and extents are not -- one compile serves every data set of that shape of table.  A -D and a word of the key exist
    only with their part, so every other source keeps the file name it had."""
    parts = _Parts.of(source, tables, term, n_derived, predict, pointwise, replicate, discrepancy)
    text, defs, key = parts.text(source), parts.defines(n_dim), parts.key(n_dim)
    deps = (_CSRC / "common.h").read_bytes() + Path(HEADER_PATH).read_bytes()
    tag = hashlib.sha256(text.encode() + deps + key.encode()).hexdigest()[:20]
    name = f"tphu_{n_dim}d_{tag}.so"
    for d in _cache_dirs():
        if (d / name).exists():
            return d / name
    last = None
    for d in _cache_dirs():
        try:
            d.mkdir(parents=True, exist_ok=True)
            with tempfile.TemporaryDirectory(dir=d) as tmp:
                src = Path(tmp) / "plugin.hip"
                src.write_text(text)
                out = Path(tmp) / name
                cmd = [_hipcc(), *_FLAGS, *defs, f"-I{_CSRC}", str(src), "-o", str(out)]
                if verbose:
                    print(" ".join(cmd))
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:
                    raise TempestHipError("HipCallbacks: hipcc failed\n" + r.stderr[-4000:])
                os.replace(out, d / name)        # atomic: concurrent ranks compile the same hash to the same name
            return d / name
        except OSError as e:                     # read-only location: try the next one
            last = e
    raise TempestHipError(f"HipCallbacks: no writable plugin cache directory ({last})")


class HipCallbacks:
    """prior_transform + log_likelihood as HIP device functions (see the module docstring)."""

    # a source of x alone: no tables, no term form, no optional part (class defaults; __init__ fills in what its arguments give)
    parts = _Parts()
    term, tables, n_terms, sum_layout = False, None, 0, SUM_LAYOUT
    data_like = None                       # "lane" | "split" pins a path of the term-form likelihood (TEMPEST_AMD_DATA_LIKE, read once)
    split_tile = 0                         # > 0 pins the particles per workgroup of the split kernel (64, 16, 4, 1)
    n_derived, derived_tile = 0, 0         # tile > 0 pins the row-major derived kernel: 256 / 128 / 64 rows per workgroup, 1 = direct
    # tile > 0 pins the indices per workgroup of predictive() (1 .. 64); (tile, slab) also the rows per workgroup of its select
    n_predict, predict_tile, predict_sum_layout = 0, 0, PREDICT_SUM_LAYOUT
    pointwise_enabled, pointwise_tile = False, 0      # tile > 0 pins the indices per workgroup of pointwise() (1 .. 64)
    psis_enabled, psis_scratch_cap = False, 0         # cap > 0 pins the words of batch scratch psis_loo() asks for (tests: several batches)
    n_replicate, observed, has_discrepancy = 0, None, False
    run_groups = 0                         # > 0 limits the workgroups of tphu_run's launch (tests: several tiles per workgroup)
    _device = _dev_tables = _dstruct = _struct_type = _bsum = _pscratch = _wscratch = _yscratch = _kscratch = None

    def __init__(self, source: str, n_dim: int, fused: bool = True, verbose: bool = False, whole_step: bool = True,
                 persistent: bool = False, data=None, n_terms=None, n_derived=None, n_predict=None, *,
                 pointwise=False, n_replicate=None, observed=None):
        if not isinstance(n_dim, int) or n_dim <= 0:
            raise ValueError(f"n_dim must be a positive int, got {n_dim!r}")
        for fn in ("prior_transform", "log_likelihood"):
            if fn not in source:
                raise ValueError(f"HipCallbacks source must define __device__ {fn}(...)")
        has_term = re.search(r"\blog_likelihood_term\s*\(", source) is not None
        if has_term and re.search(r"\blog_likelihood\s*\(", source) is not None:
            raise ValueError("HipCallbacks source defines both log_likelihood and log_likelihood_term: give one of them")
        if has_term and n_terms is None:
            raise ValueError("HipCallbacks: log_likelihood_term needs n_terms= (an int, or the name of a data entry)")
        if n_terms is not None and not has_term:
            raise ValueError("HipCallbacks: n_terms= goes with a source that defines log_likelihood_term")
        if not isinstance(pointwise, (bool, np.bool_)) and not (isinstance(pointwise, str) and pointwise == "psis"):
            raise ValueError(f"HipCallbacks: pointwise must be True or False, got {pointwise!r}")
        if pointwise and not has_term:
            raise ValueError("HipCallbacks: pointwise=True goes with a source that defines log_likelihood_term (and n_terms=)")
        self.n_derived = _check_n_derived(source, n_derived)
        tables, self._host = (None, {}) if data is None else _table_spec(data)
        if _defined_and_given(source, "predict", n_predict):
            self.n_predict = _extent(n_predict, "n_predict", self._host, below=2 ** 31)
        self.n_replicate, self.observed, self.has_discrepancy = _check_n_replicate(source, n_replicate, observed, self._host)
        if has_term:
            self.n_terms = _extent(n_terms, "n_terms", self._host)
        mode = os.environ.get("TEMPEST_AMD_DATA_LIKE", "").strip().lower()
        if mode not in ("", "lane", "split"):
            raise ValueError(f"TEMPEST_AMD_DATA_LIKE must be 'lane' or 'split', got {mode!r}")
        self.data_like = mode or None
        self.n_dim, self.source, self.fused = n_dim, source, bool(fused)
        self.whole_step = whole_step           # False: proposal and evaluate+accept as two kernels; "always": at any size
        # A whole run of steps in ONE cooperative launch (tphu_run) where the whole-step kernel applies.  OFF by default: measured
        # at 131 072 particles (profiles/r04_persistent_run.json) a step costs 32.5 us inside that launch against 30.0 us step by
        # step under the captured hipGraph -- 23.0 us whole-step kernel + 6.8 us tph_adapt + 0.4 us between them; the grid
        # barrier plus every workgroup's own sum of the tile partials cost more than the adaptation launch they replace.
        # TEMPEST_AMD_PERSISTENT=1/0 overrides the argument.
        env = os.environ.get("TEMPEST_AMD_PERSISTENT")
        self.persistent = bool(persistent) if env is None else env != "0"
        self.parts = _Parts.of(source, tables, has_term, self.n_derived, self.n_predict, pointwise, self.n_replicate, self.has_discrepancy)
        self.tables, self.term, self.pointwise_enabled = self.parts.tables, self.parts.term, self.parts.pointwise
        self.psis_enabled = self.parts.psis
        self.path = build_plugin(source, n_dim, verbose, **self.parts.build_args())
        import torch  # noqa: F401  (its HIP runtime must be the one in the process, as for libtempest_hip)
        self.lib = C.CDLL(str(self.path))
        self._struct_type = self.parts.bind(self.lib, n_dim, self.path, self.parts.text(source))

    # ---------------------------------------------------------------------------------- data tables
    @property
    def device(self):
        """Where host inputs and the data tables go: set by the sampler that owns this object (None: the current device)."""
        return self._device

    @device.setter
    def device(self, dev):
        import torch
        self._device = None if dev is None else torch.device(dev)
        if self._dev_tables is not None and self._device is not None and self._device.type == "cuda":
            cur = next(iter(self._dev_tables.values()), None)
            if cur is not None and cur.device != self._device:       # used on another device before: that copy moves
                self._dev_tables = {k: v.to(self._device) for k, v in self._dev_tables.items()}
                self._fill_struct()

    def _fill_struct(self):
        s = self._struct_type()
        for name, rank in self.tables:
            t = self._dev_tables[name]
            setattr(s, name, t.data_ptr())
            if rank == 1:
                setattr(s, name + "_len", t.shape[0])
            else:
                setattr(s, name + "_rows", t.shape[0])
                setattr(s, name + "_cols", t.shape[1])
        s.n_terms = self.n_terms
        self._dstruct = s

    def _data(self):
        """The trailing argument(s) of a data-carrying plugin's entry points (uploads the tables on first use)."""
        if self.tables is None:
            return ()
        if self._dstruct is None:
            import torch
            dev = self._device or torch.device("cuda", torch.cuda.current_device())
            self._dev_tables = {k: torch.from_numpy(v).to(dev) for k, v in self._host.items()}
            self._fill_struct()
        return (C.byref(self._dstruct),)

    def update_data(self, name, array):
        """New values for one data entry, same shape: copied into the SAME device buffer on the current stream, so a captured
        graph (which has the pointer baked in) sees them at its next replay."""
        if self.tables is None or name not in self._host:
            raise ValueError(f"update_data: no data entry {name!r}")
        arr = _host_array(name, array)
        if arr.shape != self._host[name].shape:
            raise ValueError(f"update_data: {name!r} has shape {self._host[name].shape}, got {arr.shape} "
                             "(another shape needs a new HipCallbacks object)")
        self._host[name] = arr
        if self._dev_tables is not None:
            import torch
            self._dev_tables[name].copy_(torch.from_numpy(arr), non_blocking=False)

    # ---------------------------------------------------------------------------- which path sums
    def use_split(self, n) -> bool:
        """Term-form likelihoods: True where the sum over the data is split over workgroups (k_user_like_split), False where
        the lane that owns a particle walks it.  Same bits either way."""
        if not self.term:
            return False
        if self.data_like is not None:
            return self.data_like == "split"
        return prefer_split(int(n), self.n_terms)

    def can_fuse_accept(self, n) -> bool:
        """Callbacks inside the Metropolis kernel (tphu_accept)?  Not where the split kernel is the faster likelihood: the step
        then calls prior_transform / log_likelihood between tph_propose and tph_accept."""
        return self.fused and not self.use_split(n)

    def _tile(self, n, n_blocks) -> int:
        if self.split_tile:
            return int(self.split_tile)
        tile = 64                               # a wave = 64 particles at one r (uniform data reads) ...
        while tile > 1 and tile // 4 >= n:      # ... fewer particles than that: the chunks go over the lanes instead
            tile //= 4
        while tile > 4 and -(-n // tile) * n_blocks < DATA_LIKE_THRESHOLDS["min_workgroups"]:   # ... or too few workgroups
            tile //= 4
        return tile

    # ------------------------------------------------------------------------------------ helpers
    def _check(self, rc, what):
        if rc != 0:
            raise TempestHipError(f"{what}: {self.lib.tphu_last_error().decode()}")

    @staticmethod
    def _stream(t):
        import torch
        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

    def _soa(self, a):
        """(n, d) rows [or one (d,) row] -> (tensor (d, n) contiguous, was_numpy, was_1d).  Host inputs go to `self.device`
        (set by the sampler that owns this object; the current device otherwise)."""
        import torch
        was_np = not isinstance(a, torch.Tensor)
        dev = getattr(self, "device", None) or torch.device("cuda", torch.cuda.current_device())
        if was_np:
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        one = a.dim() == 1
        if one:
            a = a.reshape(1, -1)
        if a.dim() != 2 or a.shape[1] != self.n_dim:
            raise ValueError(f"expected (..., {self.n_dim}) points, got {tuple(a.shape)}")
        if not a.is_cuda:
            a = a.to(dev)
        if a.dtype != torch.float64:
            a = a.to(torch.float64)
        t = a.T
        return (t if t.is_contiguous() else t.contiguous()), was_np, one

    def _kept_scratch(self, attr, words, device):
        """The buffer kept under `attr`, of at least `words` 8-byte words on `device`: grown on demand, no allocation per call."""
        import torch
        buf = getattr(self, attr)
        if buf is None or buf.numel() < words or buf.device != device:
            buf = torch.empty(words, dtype=torch.int64, device=device)
            setattr(self, attr, buf)
        return buf

    def _on_device(self, a):
        """A tensor or array as a contiguous float64 tensor on a device: host inputs go to `self.device` (the current one if None)."""
        import torch
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
        if not a.is_cuda:
            a = a.to(self._device or torch.device("cuda", torch.cuda.current_device()))
        return a.to(torch.float64).contiguous()

    def _predict_launch(self, n, R, nq):
        """(indices per workgroup, rows per workgroup of the select) of predictive() / replicated(): predict_tiles, or the pin."""
        tile, slab = predict_tiles(n, R, nq)
        pin = self.predict_tile
        if pin:
            tile, slab = (int(pin[0]), int(pin[1])) if isinstance(pin, (tuple, list)) else (int(pin), slab)
        return tile, slab

    # ---------------------------------------------------------------------------------- callbacks
    def prior_transform(self, u):
        """(n, n_dim) unit-cube points [or one point] -> parameters, same container kind as the input."""
        import torch
        us, was_np, one = self._soa(u)
        n = us.shape[1]
        xs = torch.empty_like(us)
        self._check(self.lib.tphu_prior(self._stream(us), us.data_ptr(), n, n, xs.data_ptr(), n, *self._data()), "tphu_prior")
        x = xs.T                                   # (n, d) strided view of the SoA buffer: no copy on the way back
        x = x[0] if one else x
        return x.cpu().numpy() if was_np else x

    def log_likelihood(self, x):
        import torch
        xs, was_np, one = self._soa(x)
        n = xs.shape[1]
        ll = torch.empty(n, dtype=torch.float64, device=xs.device)
        if self.use_split(n):
            span = self.sum_layout[0] * self.sum_layout[1]
            n_blocks = -(-self.n_terms // span)
            bsum = self._kept_scratch("_bsum", n * n_blocks, xs.device)
            self._check(self.lib.tphu_like_split(self._stream(xs), xs.data_ptr(), n, n, ll.data_ptr(), bsum.data_ptr(),
                                                 bsum.numel(), self._tile(n, n_blocks), *self._data()), "tphu_like_split")
        else:
            self._check(self.lib.tphu_like(self._stream(xs), xs.data_ptr(), n, n, ll.data_ptr(), *self._data()), "tphu_like")
        ll = ll[0] if one else ll
        return ll.cpu().numpy() if was_np else ll

    def _on_table_device(self, t, what="derived"):
        """The data tables are pointers into ONE device's memory: rows on another device must not meet them in a kernel."""
        if self.tables:
            self._data()
            tab = next(iter(self._dev_tables.values()))
            if tab.device != t.device:
                raise ValueError(f"HipCallbacks.{what}: the points are on {t.device}, the data tables on {tab.device}")

    def derived(self, x):
        """(n, n_dim) points [or one point] -> (n, n_derived) values of the source's derived() [or (n_derived,)], same container
        kind as the input.  Contiguous rows go through the row-major kernel as they are (what posterior() hands over); any other
        view is read dimension-major, like the other callbacks.  Same bits either way."""
        import torch
        if not self.n_derived:
            raise TempestHipError("HipCallbacks.derived: the source defines no derived(...) (give it and n_derived=)")
        k = self.n_derived
        rows = isinstance(x, torch.Tensor) and x.dim() == 2 and x.is_cuda and x.dtype == torch.float64 and x.is_contiguous()
        if not isinstance(x, torch.Tensor):
            xa = np.asarray(x, dtype=np.float64)
            rows = xa.ndim in (1, 2) and xa.shape[-1] == self.n_dim
        if rows:
            was_np, one = not isinstance(x, torch.Tensor), False
            if was_np:
                one = xa.ndim == 1
                x = self._on_device(xa.reshape(-1, self.n_dim))
            if x.shape[1] != self.n_dim:
                raise ValueError(f"expected (..., {self.n_dim}) points, got {tuple(x.shape)}")
            n = x.shape[0]
            out = torch.empty((n, k), dtype=torch.float64, device=x.device)
            if n:
                self._on_table_device(x)
                self._check(self.lib.tphu_derived(self._stream(x), x.data_ptr(), n, self.n_dim, out.data_ptr(), k, 1,
                                                  int(self.derived_tile), *self._data()), "tphu_derived")
        else:
            xs, was_np, one = self._soa(x)
            n = xs.shape[1]
            outs = torch.empty((k, n), dtype=torch.float64, device=xs.device)
            if n:
                self._on_table_device(xs)
                self._check(self.lib.tphu_derived(self._stream(xs), xs.data_ptr(), n, n, outs.data_ptr(), n, 0, 0, *self._data()),
                            "tphu_derived")
            out = outs.T
        out = out[0] if one else out
        return out.cpu().numpy() if was_np else out

    def _rows_and_weights(self, x, w, what):
        """The (n, n_dim) points and (n,) weights of predictive() / pointwise() as contiguous float64 device tensors, checked: n > 0,
        weights finite, >= 0, with a positive sum.  Returns (x, w, n, sum w, sum w^2)."""
        import torch
        x, w = self._on_device(x), self._on_device(w)
        if x.dim() != 2 or x.shape[1] != self.n_dim or x.shape[0] == 0:
            raise ValueError(f"{what}: expected (n, {self.n_dim}) points with n > 0, got {tuple(x.shape)}")
        n = x.shape[0]
        if w.dim() != 1 or w.shape[0] != n or w.device != x.device:
            raise ValueError(f"{what}: expected ({n},) weights beside the points, got {tuple(w.shape)} on {w.device}")
        s1, s2, bad = (float(v) for v in torch.stack([w.sum(), (w * w).sum(), (~(torch.isfinite(w) & (w >= 0))).sum().double()]).cpu())
        if bad or not s1 > 0.0 or not np.isfinite(s1):
            raise ValueError(f"{what}: the weights must be finite, >= 0 and have a positive sum")
        self._on_table_device(x, what)
        return x, w, n, s1, s2

    def predictive(self, x, w, quantiles=(0.025, 0.5, 0.975)):
        """Posterior predictive of the source's predict(x, r), r = 0 .. n_predict - 1, over the (n, n_dim) points x with weights w
        (n; >= 0, finite, positive sum, not necessarily normalised; torch-ROCm tensors or NumPy arrays): a dict of NumPy arrays
        "mean", "var" (n_predict,), "quantiles" (len(quantiles), n_predict) -- the weighted inverted CDF, always one of the
        predictions -- and "n_rows", "ess" = (sum w)^2 / sum w^2.  Nothing of size n x n_predict is formed; only the results come
        to the host.  The scratch is one buffer kept on this object (like the split likelihood's): calls on
        the same object from two streams at once would share it -- give each stream its own HipCallbacks object (same plugin)."""
        import torch
        if not self.n_predict:
            raise TempestHipError("HipCallbacks.predictive: the source defines no predict(...) (give it and n_predict=)")
        qs = _quantiles(quantiles, "predictive")
        x, w, n, s1, s2 = self._rows_and_weights(x, w, "predictive")
        R, nq = self.n_predict, len(qs)
        tile, slab = self._predict_launch(n, R, nq)
        scratch = self._kept_scratch("_pscratch", predict_scratch_words(n, R, nq), x.device)
        out = torch.empty((2 + nq, R), dtype=torch.float64, device=x.device)
        self._check(self.lib.tphu_predictive(self._stream(x), x.data_ptr(), w.data_ptr(), n, R, qs.ctypes.data, nq, out.data_ptr(),
                                             scratch.data_ptr(), scratch.numel(), tile, slab, *self._data()), "tphu_predictive")
        res = out.cpu().numpy()
        return {"mean": res[0].copy(), "var": res[1].copy(), "quantiles": res[2:].copy(), "n_rows": n, "ess": s1 * s1 / s2}

    def replicated(self, x, w, quantiles=(0.025, 0.5, 0.975), seed=0):
        """Posterior predictive check with replicated data y_rep[i, r] = replicate(x_i, r, g), r = 0 .. n_replicate - 1, over the (n,
        n_dim) points x with weights w (as predictive(): >= 0, finite, positive sum; torch-ROCm tensors or NumPy arrays; n < 2^32): a
        dict of NumPy arrays "mean", "var" (n_replicate,), "quantiles" (len(quantiles), n_replicate) -- the weighted inverted CDF of
        y_rep[:, r] --, and "n_rows", "ess", "seed"; with observed=: "pit" (n_replicate,), the weighted share of y_rep[:, r] below the
        observed y_r plus half the share equal to it (NaN where a replicate with weight, or y_r, is NaN); with discrepancy() in the
        source: "p_value" = the weighted share of rows with T_rep_i >= T_obs_i, "t_obs_mean", "t_rep_mean" (floats), T_. the sums of
        discrepancy over r at the observed and the replicated values.  The draws of g belong to (seed, the row's INDEX i in x, r): the
        same call gives the same bits, and permuting the rows (with their weights) gives another -- equally valid -- set of draws.
        Nothing of size n x n_replicate is formed.  The scratch is one buffer kept on this object."""
        import torch
        if not self.n_replicate:
            raise TempestHipError("HipCallbacks.replicated: the source defines no replicate(...) (give it and n_replicate=)")
        qs = _quantiles(quantiles, "replicated")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"replicated: seed must be an int in [0, 2^64), got {seed!r}")
        x, w, n, s1, s2 = self._rows_and_weights(x, w, "replicated")
        if n >= 2 ** 32:
            raise ValueError(f"replicated: at most 2^32 - 1 rows (the row index is a 32-bit counter word of the noise), got {n}")
        R, nq = self.n_replicate, len(qs)
        tile, slab = self._predict_launch(n, R, nq)
        scratch = self._kept_scratch("_yscratch", replicate_scratch_words(n, R, nq), x.device)
        out = torch.empty((3 + nq) * R + 3, dtype=torch.float64, device=x.device)
        data = self._data()
        obs = self._dev_tables[self.observed].data_ptr() if self.observed is not None else None
        self._check(self.lib.tphu_replicated(self._stream(x), x.data_ptr(), w.data_ptr(), n, R, qs.ctypes.data, nq, int(seed), obs,
                                             1 if self.has_discrepancy else 0, out.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                             tile, slab, *data), "tphu_replicated")
        flat = out.cpu().numpy()
        res = flat[:(3 + nq) * R].reshape(3 + nq, R)
        ret = {"mean": res[0].copy(), "var": res[1].copy(), "quantiles": res[2:2 + nq].copy(), "n_rows": n, "ess": s1 * s1 / s2,
               "seed": int(seed)}
        if self.observed is not None:
            ret["pit"] = res[2 + nq].copy()
        if self.has_discrepancy:
            ret.update(p_value=float(flat[-3]), t_obs_mean=float(flat[-2]), t_rep_mean=float(flat[-1]))
        return ret

    def pointwise(self, x, w):
        """Pointwise log predictive densities of a term-form source built with pointwise=True, over the (n, n_dim) points x with
        weights w (n; >= 0, finite, positive sum, not necessarily normalised; torch-ROCm tensors or NumPy arrays).  With a_ir =
        log_likelihood_term(x_i, r, D) and u_i = w_i / sum w, a dict of NumPy arrays (n_terms,): "lppd" = log sum u exp(a), "mean" =
        sum u a, "p_waic" = sum u (a - mean)^2, "elpd_waic" = lppd - p_waic, "elpd_loo" = -log sum u exp(-a) (importance-sampling
        leave-one-out), "ess_loo" = (sum v)^2 / sum v^2 with v = u exp(-a) -- the effective number of rows behind elpd_loo[r]: a small
        one marks an estimate not to be trusted --; and "n_rows", "ess" = (sum w)^2 / sum w^2, "totals": the sums over r (math.fsum)
        elpd_waic, p_waic, lppd, elpd_loo, p_loo = lppd - elpd_loo, and elpd_waic_se, elpd_loo_se = sqrt(n_terms x the population
        variance of the pointwise values).  Nothing of size n x n_terms is formed; only the (6, n_terms) results come to the host
        (DESIGN.md section 11).  The scratch is one buffer kept on this object, as for predictive()."""
        import torch
        if not self.pointwise_enabled:
            raise TempestHipError("HipCallbacks.pointwise: the object was built without pointwise=True (give it, with a source that defines "
                                  "log_likelihood_term)")
        x, w, n, s1, s2 = self._rows_and_weights(x, w, "pointwise")
        R = self.n_terms
        tile = int(self.pointwise_tile) or pointwise_tiles(n, R)
        words = pointwise_scratch_words(n, R)
        scratch = self._kept_scratch("_wscratch", words, x.device)
        out = torch.empty((len(POINTWISE_KEYS), R), dtype=torch.float64, device=x.device)
        self._check(self.lib.tphu_pointwise(self._stream(x), x.data_ptr(), w.data_ptr(), n, R, out.data_ptr(), scratch.data_ptr(),
                                            words, tile, *self._data()), "tphu_pointwise")
        res = {k: v.copy() for k, v in zip(POINTWISE_KEYS, out.cpu().numpy())}
        tot = {k: _total(res[k]) for k in ("elpd_waic", "p_waic", "lppd", "elpd_loo")}
        tot["p_loo"] = tot["lppd"] - tot["elpd_loo"]
        with np.errstate(invalid="ignore", over="ignore"):
            for k in ("elpd_waic", "elpd_loo"):
                tot[k + "_se"] = float(np.sqrt(R * np.var(res[k])))
        res.update(n_rows=n, ess=s1 * s1 / s2, totals=tot)
        return res

    def psis_loo(self, x):
        """Pareto-smoothed importance-sampling leave-one-out (Vehtari, Gelman & Gabry) of a term-form source built with
        pointwise="psis", over the (n, n_dim) EQUALLY weighted rows x (torch-ROCm tensor or NumPy array).  Per observation r, with a_i =
        log_likelihood_term(x_i, r, D) and the log ratios l_i = min a - a_i: the M = "tail_len" largest ratios are refitted by a
        generalised Pareto distribution (Zhang & Stephens, as loo::gpdfit) and replaced by its order statistics.  A dict of NumPy arrays
        (n_terms,): "pareto_k", the fitted shape -- above "k_threshold" = min(1 - 1 / log10(n), 0.7) the estimate is not to be trusted;
        +inf where nothing was smoothed (M < 5, a degenerate tail) and "elpd_psis" is the plain importance-sampling value --, "elpd_psis",
        "ess_psis" = 1 / sum v^2 over the normalised smoothed ratios v; and "tail_len", "n_rows", "k_threshold", "totals": elpd_psis
        (math.fsum), elpd_psis_se = sqrt(n_terms x the population variance), n_high_k = how many pareto_k exceed the threshold (a NaN
        counts).  A NaN term makes all three NaN; min a = -inf or +inf is elpd_psis, with pareto_k and ess_psis NaN.  Nothing of size n x
        n_terms is formed; no tile, batch or launch shape changes a bit.  The scratch is one buffer kept on this
        object, as for predictive()."""
        import torch
        if not self.psis_enabled:
            raise TempestHipError('HipCallbacks.psis_loo: the object was built without pointwise="psis" (give it, with a source that '
                                  "defines log_likelihood_term)")
        x = self._on_device(x)
        if x.dim() != 2 or x.shape[1] != self.n_dim or x.shape[0] == 0:
            raise ValueError(f"psis_loo: expected (n, {self.n_dim}) points with n > 0, got {tuple(x.shape)}")
        self._on_table_device(x, "psis_loo")
        n, R = x.shape[0], self.n_terms
        tail = psis_tail_len(n)
        tile = int(self.pointwise_tile) or pointwise_tiles(n, R)
        slab = predict_tiles(n, R, 1)[1]
        words = int(self.psis_scratch_cap) or psis_scratch_words(n, R)
        scratch = self._kept_scratch("_kscratch", words, x.device)
        ones = torch.ones(n, dtype=torch.float64, device=x.device)
        out = torch.empty((len(PSIS_KEYS), R), dtype=torch.float64, device=x.device)
        self._check(self.lib.tphu_psis(self._stream(x), x.data_ptr(), ones.data_ptr(), n, R, tail, out.data_ptr(), scratch.data_ptr(),
                                       words, tile, slab, *self._data()), "tphu_psis")
        res = {k: v.copy() for k, v in zip(PSIS_KEYS, out.cpu().numpy())}
        res.update(tail_len=tail, n_rows=n, k_threshold=psis_k_threshold(n), totals=psis_totals(res, psis_k_threshold(n)))
        return res

    # ------------------------------------------------------------------------------ fused MCMC step
    def accept(self, kernel_id, beta, u, x, logl, uprime, maha_u, maha_up, assign, K, dof, seed, tick, item0, sums,
               ctl=None, partials=None, pending=None):
        """tph_accept with the two callbacks evaluated inside the kernel (u, x: (d, n) SoA tensors, updated in place)."""
        n = u.shape[1]
        if partials is None or partials.numel() < ((n + 255) // 256) * (1 + K):
            raise TempestHipError("HipCallbacks.accept: partials buffer missing or too small")
        for t in (u, logl, uprime) + ((x,) if x is not None else ()):
            if not (t.is_cuda and t.is_contiguous()):
                raise TempestHipError("HipCallbacks.accept: expected contiguous device tensors")
        p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        self._check(self.lib.tphu_accept(self._stream(u), int(kernel_id), float(beta), p(u), p(x), p(logl), p(uprime),
                                         p(maha_u), p(maha_up), p(assign), n, n, int(K), p(dof), int(seed), int(tick),
                                         int(item0), p(sums), p(ctl), p(partials), p(pending), *self._data()), "tphu_accept")

    def can_fuse_step(self, K, has_assign, n) -> bool:
        """The whole step (proposal + callbacks + Metropolis update) in ONE kernel: register proposal kernel only
        (n_dim <= 16), one proposal mode, and shards up to 512 K particles -- measured: 45 -> 41 us per step at 131 072
        particles, where the step is latency-bound, but 157 -> 165 us at 1 048 576, where the proposal kernel is VALU-bound
        and the longer kernel only lowers its occupancy."""
        return (self.fused and self.whole_step and self.n_dim <= 16 and K == 1 and not has_assign
                and (self.whole_step == "always" or n <= 512 * 1024) and not self.use_split(n))

    def can_run(self, K, has_assign, n) -> bool:
        """A whole run of steps (the loop of mcmc.py:142-208) in ONE cooperative launch: where the whole-step kernel applies
        (one process; the caller checks that), unless a launch was refused before (no cooperative launch on the device)."""
        return bool(self.persistent) and self.can_fuse_step(K, has_assign, n)

    def run(self, kernel_id, u, logl, maha_u, modes, sigmas, bc, seed, tick_propose, tick_accept, item0, ctl, partials2, barrier,
            counts, n_global, n_steps, n_max, mailbox, slots, max_steps, redraw_lanes=0) -> bool:
        """tphu_run: steps until the stopping rule of `ctl` fires, adaptation included, in one launch (partials2: 2 x tiles x 2
        doubles; barrier: 4 int32 words; mailbox: (slots + 1) x 8 pinned doubles, the last row takes the final record).  False:
        the device refused the launch -- nothing ran, step the usual way."""
        n = u.shape[1]
        tiles = (n + 255) // 256
        if partials2.numel() < 4 * tiles or barrier.numel() < 4 or mailbox.numel() < 8 * (slots + 1):
            raise TempestHipError("HipCallbacks.run: buffers too small")
        for t in (u, logl, maha_u):
            if not (t.is_cuda and t.is_contiguous()):
                raise TempestHipError("HipCallbacks.run: expected contiguous device tensors")
        p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        winv = getattr(modes, "winv_dev", None)
        if winv is None:
            import torch
            winv = torch.linalg.inv(modes.chol_dev)
        rc = self.lib.tphu_run(self._stream(u), int(kernel_id), p(u), p(logl), p(maha_u), n, n, p(modes.means_dev), p(modes.chol_dev),
                               p(winv), p(modes.dof_dev), p(sigmas), p(bc), int(seed), int(tick_propose), int(tick_accept), int(item0),
                               p(ctl), p(partials2), p(barrier), p(counts), float(n_global), int(n_steps), int(n_max), p(mailbox),
                               int(slots), int(max_steps), int(redraw_lanes), int(self.run_groups), *self._data())
        if rc == -3:
            self.persistent = False
            return False
        self._check(rc, "tphu_run")
        return True

    def step(self, kernel_id, u, logl, maha_u, modes, sigmas, bc, seed, tick_propose, tick_accept, item0, ctl, partials,
             redraw_lanes=0):
        """tph_propose + tphu_accept in one launch (u: (d, n) SoA, updated in place; x is not maintained)."""
        n = u.shape[1]
        if partials is None or partials.numel() < ((n + 255) // 256) * 2:
            raise TempestHipError("HipCallbacks.step: partials buffer missing or too small")
        for t in (u, logl, maha_u):
            if not (t.is_cuda and t.is_contiguous()):
                raise TempestHipError("HipCallbacks.step: expected contiguous device tensors")
        p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        winv = getattr(modes, "winv_dev", None)
        if winv is None:               # mode statistics built outside ModeStatistics: L^-1 from the factors
            import torch
            winv = torch.linalg.inv(modes.chol_dev)
        self._check(self.lib.tphu_step(self._stream(u), int(kernel_id), 0.0, p(u), p(logl), p(maha_u), n, n,
                                       p(modes.means_dev), p(modes.chol_dev), p(winv), p(modes.dof_dev), p(sigmas),
                                       p(bc), int(seed), int(tick_propose), int(tick_accept), int(item0), p(ctl), p(partials),
                                       int(redraw_lanes), *self._data()), "tphu_step")


def fused_plugin(prior_transform, log_likelihood):
    """The HipCallbacks object both callbacks belong to (and that allows fusion), else None."""
    a = getattr(prior_transform, "__self__", None)
    b = getattr(log_likelihood, "__self__", None)
    if isinstance(a, HipCallbacks) and a is b and a.fused:
        return a
    return None
