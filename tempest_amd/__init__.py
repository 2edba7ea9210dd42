"""tempest_amd -- MI355X-native Persistent Sampling: the hot path of minaskar/tempest (reweight, resample,
MCMC mutation, proposal fit) as hand-written HIP kernels for gfx950 behind the reference's Sampler API."""
__version__ = "0.1.0"

from .sampler import Sampler

__all__ = ["Sampler", "HipCallbacks", "trace_callbacks", "Noise", "Prior", "priors", "compare_pointwise"]


def __getattr__(name):          # lazy: importing the package must not need hipcc or a GPU
    if name == "HipCallbacks":
        from .hipcallbacks import HipCallbacks
        return HipCallbacks
    if name == "trace_callbacks":
        from .trace import trace_callbacks
        return trace_callbacks
    if name == "Noise":         # the host twin of a plugin's tphu_noise: the g of trace_callbacks(replicate=) in eager use
        from .trace import Noise
        return Noise
    if name == "Prior":         # independent priors column by column: a traceable prior_transform, its HIP text, its log density
        from .priors import Prior
        return Prior
    if name == "compare_pointwise":     # two models on the same observations by a pointwise value of Sampler.pointwise()
        from .hipcallbacks import compare_pointwise
        return compare_pointwise
    if name == "priors":
        import importlib
        return importlib.import_module(".priors", __name__)
    raise AttributeError(name)
