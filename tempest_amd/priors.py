"""Independent priors, column by column, as a prior_transform the tracer understands.

    prior = tp.Prior([tp.priors.Uniform(-5, 5), tp.priors.Normal(0.0, 2.0), tp.priors.LogNormal(0.0, 0.5)])
    cb = tp.trace_callbacks(prior.transform, log_likelihood, prior.n_dim)          # traced: no HIP written
    cb = tp.HipCallbacks(prior.hip_source() + LIKELIHOOD_SOURCE, prior.n_dim)      # beside a hand-written likelihood

`Prior.transform` maps the unit cube to the parameters with traceable torch operations only, every constant formed on the host in
float64; the Gaussian family goes through the inverse normal CDF, torch.special.ndtri -- on the device csrc/quantile.h, whose text
is `DEVICE_HELPERS`.  `Prior.hip_source()` is the trace of `transform`, so the hand-written route and the
traced one run the same statements.

A unit-cube coordinate of exactly 0 (or 1) under a column of unbounded support maps to -inf (+inf), as the quantile function
does; the sampler treats such a point as it treats any infinite parameter a user's own prior_transform returns.
"""
import math

import numpy as np

from .trace import TV, emit_function, quantile_header, trace_function

DEVICE_HELPERS = quantile_header()
_LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def _number(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or math.isnan(float(v)):
        raise ValueError(f"{what} must be a number, got {v!r}")
    return float(v)


def _finite(v, what):
    v = _number(v, what)
    if math.isinf(v):
        raise ValueError(f"{what} must be finite, got {v!r}")
    return v


def _positive(v, what):
    v = _finite(v, what)
    if v <= 0.0:
        raise ValueError(f"{what} must be positive, got {v!r}")
    return v


def _phi(z):
    """The standard normal CDF at a Python float, without cancellation in the lower tail."""
    return 0.5 * math.erfc(-z * math.sqrt(0.5))


def _ndtri(p):
    import torch
    return torch.special.ndtri(p)


def _outside(x, lo, hi, logp):
    """logp inside [lo, hi], -inf outside (a NaN stays a NaN)."""
    import torch
    return torch.where((x < lo) | (x > hi), torch.full_like(x, -math.inf), logp)


class Distribution:
    """One column of a Prior: transform(u) maps a column of unit-cube coordinates (a tensor, or the tracer's value) to the parameter
    with traceable operations; log_prob(x) is the log density of a float64 tensor, -inf outside the support."""

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in self.__dict__.items() if not k.startswith('_'))})"


class Uniform(Distribution):
    """Uniform on [a, b]: a + (b - a) u."""

    def __init__(self, a, b):
        self.a, self.b = _finite(a, "Uniform: a"), _finite(b, "Uniform: b")
        if not self.a < self.b:
            raise ValueError(f"Uniform: a < b is required, got a={a!r}, b={b!r}")
        self._w = self.b - self.a

    def transform(self, u):
        return self.a + self._w * u

    def log_prob(self, x):
        import torch
        return _outside(x, self.a, self.b, torch.full_like(x, -math.log(self._w)))


class LogUniform(Distribution):
    """Uniform in log x on [a, b], 0 < a < b: exp(log a + (log b - log a) u)."""

    def __init__(self, a, b):
        self.a, self.b = _positive(a, "LogUniform: a"), _positive(b, "LogUniform: b")
        if not self.a < self.b:
            raise ValueError(f"LogUniform: a < b is required, got a={a!r}, b={b!r}")
        self._la = math.log(self.a)
        self._w = math.log(self.b) - self._la

    def transform(self, u):
        import torch
        return torch.exp(self._la + self._w * u)

    def log_prob(self, x):
        import torch
        return _outside(x, self.a, self.b, -torch.log(x) - math.log(self._w))


class Normal(Distribution):
    """N(mu, s^2): mu + s ndtri(u)."""

    def __init__(self, mu, s):
        self.mu, self.s = _finite(mu, "Normal: mu"), _positive(s, "Normal: s")

    def transform(self, u):
        return self.mu + self.s * _ndtri(u)

    def log_prob(self, x):
        z = (x - self.mu) / self.s
        return -0.5 * z * z - (math.log(self.s) + _LOG_SQRT_2PI)


class LogNormal(Distribution):
    """log x ~ N(mu, s^2): exp(mu + s ndtri(u))."""

    def __init__(self, mu, s):
        self.mu, self.s = _finite(mu, "LogNormal: mu"), _positive(s, "LogNormal: s")

    def transform(self, u):
        import torch
        return torch.exp(self.mu + self.s * _ndtri(u))

    def log_prob(self, x):
        import torch
        lx = torch.log(x)
        z = (lx - self.mu) / self.s
        return torch.where(x <= 0.0, torch.full_like(x, -math.inf), -0.5 * z * z - (math.log(self.s) + _LOG_SQRT_2PI) - lx)


class HalfNormal(Distribution):
    """|N(0, s^2)|: s ndtri(0.5 + 0.5 u)."""

    def __init__(self, s):
        self.s = _positive(s, "HalfNormal: s")

    def transform(self, u):
        return self.s * _ndtri(0.5 + 0.5 * u)

    def log_prob(self, x):
        z = x / self.s
        return _outside(x, 0.0, math.inf, -0.5 * z * z - (math.log(self.s) + _LOG_SQRT_2PI - math.log(2.0)))


class Exponential(Distribution):
    """Density rate exp(-rate x) on x >= 0: -log1p(-u) / rate."""

    def __init__(self, rate):
        self.rate = _positive(rate, "Exponential: rate")
        self._scale = 1.0 / self.rate

    def transform(self, u):
        import torch
        return -torch.log1p(-u) * self._scale

    def log_prob(self, x):
        return _outside(x, 0.0, math.inf, math.log(self.rate) - self.rate * x)


class TruncatedNormal(Distribution):
    """N(mu, s^2) kept to [lo, hi] (either may be infinite): mu + s ndtri(Pa + (Pb - Pa) u), clamped to [lo, hi], with Pa and Pb the
    normal CDF at the standardised bounds.  Where the standardised lo is positive -- the whole interval in the upper tail, Pa and Pb
    next to 1 -- the mirrored problem is solved instead, mu - s ndtri((1 - Pa) - (Pb - Pa) u): the arguments of ndtri then stay below 0.5
    and keep their relative accuracy."""

    def __init__(self, mu, s, lo=-math.inf, hi=math.inf):
        self.mu, self.s = _finite(mu, "TruncatedNormal: mu"), _positive(s, "TruncatedNormal: s")
        self.lo, self.hi = _number(lo, "TruncatedNormal: lo"), _number(hi, "TruncatedNormal: hi")
        if not self.lo < self.hi:
            raise ValueError(f"TruncatedNormal: lo < hi is required, got lo={lo!r}, hi={hi!r}")
        alpha, beta = (self.lo - self.mu) / self.s, (self.hi - self.mu) / self.s
        self._mirrored = alpha > 0.0
        # the end of the interval of ndtri's argument that u = 0 maps to, and its signed width
        self._p0, p1 = (_phi(-alpha), _phi(-beta)) if self._mirrored else (_phi(alpha), _phi(beta))
        self._w = p1 - self._p0
        if self._w == 0.0:
            raise ValueError(f"TruncatedNormal: [lo, hi] = [{lo!r}, {hi!r}] holds no probability of N({mu!r}, {s!r}^2) in double "
                             "precision (Pb - Pa == 0)")
        self._sign = -self.s if self._mirrored else self.s

    def transform(self, u):
        import torch
        x = self.mu + self._sign * _ndtri(self._p0 + self._w * u)
        lo, hi = (None if math.isinf(v) else v for v in (self.lo, self.hi))
        return x if lo is None and hi is None else torch.clamp(x, min=lo, max=hi)

    def log_prob(self, x):
        z = (x - self.mu) / self.s
        return _outside(x, self.lo, self.hi, -0.5 * z * z - (math.log(self.s) + _LOG_SQRT_2PI + math.log(abs(self._w))))


class Prior:
    """Independent columns: Prior([Uniform(-5, 5), Normal(0, 2), ...]).  n_dim: the number of columns; transform: the vectorised
    prior_transform (torch tensor -> torch tensor, NumPy -> NumPy), traceable as it is; log_prob: the (n,) log density; hip_source:
    the HIP text of transform for a hand-written HipCallbacks source."""

    def __init__(self, distributions):
        dists = list(distributions)
        if not dists:
            raise ValueError("Prior: at least one distribution is required")
        for d in dists:
            if not isinstance(d, Distribution):
                raise ValueError(f"Prior: expected distributions of tempest_amd.priors, got {d!r}")
        self.distributions, self.n_dim = tuple(dists), len(dists)

    def __repr__(self):
        return f"Prior([{', '.join(map(repr, self.distributions))}])"

    def _columns(self, a, what, each):
        """each(distribution, column) over the columns of `a`, stacked; the container kind of `a` is kept."""
        import torch
        was_np = not isinstance(a, torch.Tensor)
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)) if was_np else a.to(torch.float64)
        one = t.dim() == 1
        if one:
            t = t.reshape(1, -1)
        if t.dim() != 2 or t.shape[1] != self.n_dim:
            raise ValueError(f"Prior.{what}: expected (..., {self.n_dim}) points, got {tuple(t.shape)}")
        out = torch.stack([each(d, t[:, j]) for j, d in enumerate(self.distributions)], dim=1)
        return out, was_np, one

    def transform(self, u):
        """(n, n_dim) unit-cube points [or one point] -> parameters."""
        if isinstance(u, TV):               # under the tracer: the same statements on the symbolic columns
            import torch
            return torch.stack([d.transform(u[:, j]) for j, d in enumerate(self.distributions)], dim=1)
        x, was_np, one = self._columns(u, "transform", lambda d, c: d.transform(c))
        x = x[0] if one else x
        return x.numpy() if was_np else x

    def log_prob(self, x):
        """(n, n_dim) parameters [or one point] -> (n,) log density of the prior, -inf outside its support."""
        lp, was_np, one = self._columns(x, "log_prob", lambda d, c: d.log_prob(c))
        lp = lp.sum(dim=1)
        lp = lp[0] if one else lp
        return lp.numpy() if was_np else lp

    def hip_source(self):
        """`__device__ void prior_transform(const double* u, double* x)` as trace_callbacks(prior.transform, ...) emits it, behind
        the text of csrc/quantile.h where a column needs it: to go in front of a hand-written log_likelihood."""
        g = trace_function(self.transform, self.n_dim, self.n_dim, "prior_transform")
        parts = [DEVICE_HELPERS.rstrip("\n")] if g.needs_quantile_header() else []
        return "\n".join(parts + [emit_function(g, "prior_transform")]) + "\n"
