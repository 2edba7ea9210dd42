"""`Noise`: the host twin of the counter-based stream a plugin's replicate() draws from."""
from functools import partialmethod

import numpy as np
import torch

from .._philox_host import normal_pair, uniform_pair

MAX_DRAW = 2 ** 31              # k of g.normal(k) / g.uniform(k): the device takes it as an int


def _draw_index(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < MAX_DRAW:
        return None
    return int(k)


class Noise:
    """The host twin of the device's `tphu_noise`: Noise(seed, items, n_replicate).normal(k) / .uniform(k) are (len(items),
    n_replicate) float64 tensors (on `device`; default: the CPU) whose element [i, r] is the draw g.normal(k) / g.uniform(k) the
    device hands replicate(x, r, g) for the row of index items[i] in the x that cb.replicated(x, w, seed=seed) was given.  Philox4x32-10
    with key = seed, counter (item = the row's index, draw = k >> 1, tick = r, tag = 10 for normals, 11 for uniforms), lane k & 1 of
    the pair.

    The uniforms are 53-bit integers scaled by 2^-53: they EQUAL the device's bits.  The normals are Box-Muller on the same two
    uniforms, r = sqrt(-2 log u1), angle 2 pi u2, with NumPy's log / cos / sin where the device has its own lean versions: they agree
    with the device's to rounding, not to the bit.  A function that thresholds a normal (g.normal(k) > c) can therefore differ
    from the device at a tie; one that thresholds a uniform cannot.  The same k asked twice is the same tensor."""

    def __init__(self, seed, items, n_replicate, device=None):
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"Noise: seed must be an int in [0, 2^64), got {seed!r}")
        if isinstance(n_replicate, bool) or not isinstance(n_replicate, (int, np.integer)) or not 0 < int(n_replicate) < 2 ** 31:
            raise ValueError(f"Noise: n_replicate must be an int in (0, 2^31), got {n_replicate!r}")
        items = np.asarray(items)
        if items.ndim != 1 or items.dtype.kind not in "iu" or (items.size and (int(items.min()) < 0 or int(items.max()) >= 2 ** 32)):
            raise ValueError("Noise: items must be a 1-D array of row indices in [0, 2^32)")
        self.seed, self.n_replicate, self.device = int(seed), int(n_replicate), device
        self.items = items.astype(np.uint64)
        self._pairs, self._out = {}, {}

    def _get(self, kind, k):
        from ..hipcallbacks import REPLICATE_TAGS
        i = _draw_index(k)
        if i is None:
            raise ValueError(f"Noise.{kind}: k must be an int with 0 <= k < 2^31, got {k!r}")
        if (kind, i) not in self._out:
            if (kind, i >> 1) not in self._pairs:
                pair, tag = (normal_pair, REPLICATE_TAGS[0]) if kind == "normal" else (uniform_pair, REPLICATE_TAGS[1])
                self._pairs[(kind, i >> 1)] = pair(self.seed, self.items[:, None], i >> 1, np.arange(self.n_replicate, dtype=np.uint64)[None, :], tag)
            t = torch.from_numpy(np.ascontiguousarray(self._pairs[(kind, i >> 1)][i & 1]))
            self._out[(kind, i)] = t if self.device is None else t.to(self.device)
        return self._out[(kind, i)]

    normal, uniform = partialmethod(_get, "normal"), partialmethod(_get, "uniform")
