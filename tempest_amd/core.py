"""Run coordinator (reference: tempest/core.py): wires the four steps around one StateManager, runs the
Persistent Sampling loop, evaluates the stopping rule and assembles posterior()/evidence().

The user's callbacks are adapted once (`CallbackAdapter`) to the device layout: particle tensors are
(n_dim, n) SoA in HBM and a callback sees `tensor.T`, an (n, n_dim) strided view, so `x[:, ::2]` etc. work
without any copy.  backend="torch" hands torch-ROCm tensors to the callbacks (no host round trip),
backend="numpy" stages through the host for NumPy likelihoods (drop-in, PCIe-bound), "auto" probes.
"""
import warnings
from collections import namedtuple
from pathlib import Path
from typing import Optional, Union

import numpy as np

from .config import (BETA_RTOL, BETA_TOLERANCE, DOF_FALLBACK, ESS_TOLERANCE, METRIC_ATOL, METRIC_ATOL_CV, TRIM_BINS,
                     TRIM_ESS, SamplerConfig)
from .mcmc import PhiloxStream
from .state_manager import StateManager


class CallbackAdapter:
    """prior_transform / log_likelihood of the reference's contract -> device callables on SoA tensors."""

    def __init__(self, config: SamplerConfig, device, get_distribute_func):
        self.cfg = config
        self.device = device
        self.backend = None if config.backend == "auto" else config.backend
        self.batch_prior = config.batch_prior
        self._distribute = get_distribute_func
        from .hipcallbacks import fused_plugin
        self.hip_plugin = fused_plugin(config.prior_transform, config.log_likelihood)   # HipCallbacks pair -> fused step
        for cb in (config.prior_transform, config.log_likelihood):                       # host inputs land on OUR device
            owner = getattr(cb, "__self__", None)
            if owner is not None and hasattr(owner, "_soa"):
                owner.device = device

    # ------------------------------------------------------------------ probing
    def _probe(self):
        import torch
        cfg = self.cfg
        d = cfg.n_dim
        us = torch.linspace(0.05, 0.95, 4 * d, dtype=torch.float64, device=self.device).reshape(d, 4).T  # (4, d) view
        if self.backend is None:
            self.backend = "torch"
            try:
                xs = cfg.prior_transform(us)
                ok = isinstance(xs, torch.Tensor) and tuple(xs.shape) == (4, d) and xs.device == us.device
                if not ok:
                    xs0 = cfg.prior_transform(us[0])
                    ok = isinstance(xs0, torch.Tensor) and tuple(xs0.shape) == (d,)
                    xs = torch.stack([cfg.prior_transform(r) for r in us]) if ok else None
                if ok and cfg.vectorize:
                    ll = cfg.log_likelihood(xs)
                    ok = isinstance(ll, torch.Tensor) and ll.numel() == 4
                elif ok:
                    ok = False          # per-sample likelihoods run on the host
            except Exception:
                ok = False
            if not ok:
                self.backend = "numpy"
        if self.batch_prior is None:
            try:
                if self.backend == "torch":
                    xb = cfg.prior_transform(us)
                    xr = torch.stack([cfg.prior_transform(r) for r in us])
                    self.batch_prior = bool(isinstance(xb, torch.Tensor) and xb.shape == xr.shape
                                            and torch.equal(xb, xr))
                else:
                    uh = us.cpu().numpy().copy()
                    xb = np.asarray(cfg.prior_transform(uh))
                    xr = np.array([cfg.prior_transform(r) for r in uh])
                    self.batch_prior = bool(xb.shape == xr.shape and np.array_equal(xb, xr))
            except Exception:
                self.batch_prior = False
            if not self.batch_prior:
                warnings.warn("prior_transform is not batch-safe: it will be applied row by row "
                              "(the reference's convention), which serialises every MCMC step.", stacklevel=3)

    # ---------------------------------------------------------------- callbacks
    def prior(self, u_soa):
        """(d, n) SoA unit-cube tensor -> (d, n) SoA parameter tensor."""
        import torch
        if self.backend is None or self.batch_prior is None:
            self._probe()
        if self.backend == "torch":
            uv = u_soa.T
            xv = self.cfg.prior_transform(uv) if self.batch_prior else torch.stack(
                [self.cfg.prior_transform(r) for r in uv])
            if xv.dtype != torch.float64:
                xv = xv.to(torch.float64)
            xt = xv.T
            return xt if xt.is_contiguous() else xt.contiguous()
        uh = np.ascontiguousarray(u_soa.cpu().numpy().T)
        xh = np.asarray(self.cfg.prior_transform(uh)) if self.batch_prior else np.array(
            [self.cfg.prior_transform(r) for r in uh])
        return torch.from_numpy(np.ascontiguousarray(np.asarray(xh, dtype=np.float64).T)).to(self.device)

    def loglike(self, x_soa, return_blobs=False):
        """(d, n) SoA parameter tensor -> (n,) log-likelihood tensor (FP64, on the device); with `return_blobs` the pair
        (tensor, blobs): the likelihood's auxiliary outputs as a host array (None without them), core.py:317-358."""
        import torch
        if self.backend is None:
            self._probe()
        cfg = self.cfg
        if cfg.vectorize and self.backend == "torch":
            ll = cfg.log_likelihood(x_soa.T)
            if ll.dtype != torch.float64:
                ll = ll.to(torch.float64)
            ll = ll.reshape(-1).contiguous()
            return (ll, None) if return_blobs else ll
        xh = np.ascontiguousarray(x_soa.cpu().numpy().T)
        ll, blobs = self.loglike_host(xh)
        ll = torch.from_numpy(np.ascontiguousarray(ll, dtype=np.float64).reshape(-1)).to(self.device)
        return (ll, blobs) if return_blobs else ll

    def loglike_host(self, x):
        """The reference's SamplerCore._log_like on host arrays (core.py:317-358)."""
        cfg = self.cfg
        if cfg.vectorize:
            return np.asarray(cfg.log_likelihood(x)), None
        if cfg.pool is not None:
            results = list(self._distribute()(cfg.log_likelihood, x))
        else:
            results = list(map(cfg.log_likelihood, x))
        if results and isinstance(results[0], (tuple, list)) and len(results[0]) > 1:
            logl = np.array([float(r[0]) for r in results])
            return logl, _pack_blobs([r[1:] for r in results], cfg.blobs_dtype)
        return np.array([float(v) for v in results]), None


def _pack_blobs(rows, dtype=None):
    """The per-sample auxiliary outputs of a non-vectorised likelihood as ONE host array with the sample axis first.
    The element type is the configured `blobs_dtype`, else that of the first sample (text and anything NumPy cannot type
    become `object`); axes of length one behind the sample axis are dropped, so one scalar per sample gives shape (n,).
    Behaviour of the reference's blob handling (core.py:335-352); host data the device path never sees."""
    if dtype is None:
        try:
            dtype = np.asarray(rows[0]).dtype
        except ValueError:               # ragged sample
            dtype = np.dtype(object)
        if dtype.kind in ("U", "S"):
            dtype = np.dtype(object)
    arr = np.array(rows, dtype=dtype)
    shape = arr.shape[:1] + tuple(m for m in arr.shape[1:] if m != 1)
    return arr if shape == arr.shape else arr.reshape(shape)


_Selection = namedtuple("_Selection", "w_dev sel m_sel wdiv m s1")       # SamplerCore._select
_Derived = namedtuple("_Derived", "fn on_device width")                  # SamplerCore._derived_source

class SamplerCore:
    """Internal coordinator; `Sampler` delegates to it (core.py:20-108)."""

    def __init__(self, config: SamplerConfig, state: StateManager):
        from .steps import Mutator, Resampler, Reweighter, Trainer
        self.config = config
        self.state = state
        comm = state.comm
        self.world = comm.world_size if comm is not None else 1
        if config.n_particles % self.world:
            raise ValueError(f"n_particles ({config.n_particles}) must be divisible by the number of GPUs ({self.world})")
        self.n_local = config.n_particles // self.world
        # random_state seeds the counter-based stream; without it the seed is taken from NumPy's global
        # stream, so `np.random.seed(k)` makes a run reproducible the way it does for the reference
        seed = config.random_state if config.random_state is not None else int(np.random.randint(0, 2 ** 62))
        if comm is not None and comm.active:      # every rank must walk the same counter-based stream
            seed = comm.sum_int(seed if comm.rank == 0 else 0)
        self.rng = PhiloxStream(seed)
        self.callbacks = None

        self.reweighter = Reweighter(state=state, pbar=None, n_particles=config.n_particles, ess_ratio=config.ess_ratio,
                                     volume_variation=config.volume_variation, ESS_TOLERANCE=ESS_TOLERANCE,
                                     BETA_TOLERANCE=BETA_TOLERANCE, BETA_RTOL=BETA_RTOL, METRIC_ATOL=METRIC_ATOL,
                                     METRIC_ATOL_CV=METRIC_ATOL_CV)
        clusterer = None
        if config.clustering:
            from .cluster import HierarchicalGaussianMixture
            clusterer = HierarchicalGaussianMixture(
                n_init=1,
                max_iterations=1000 if config.n_max_clusters is None else config.n_max_clusters - 1,
                min_points=None if config.n_max_clusters is None else 4 * config.n_dim,
                threshold_modifier=config.split_threshold, covariance_type="full", verbose=False,
                normalize=config.normalize)
        self.trainer = Trainer(state=state, pbar=None, clusterer=clusterer, cluster_every=config.cluster_every,
                               clustering=config.clustering, TRIM_ESS=TRIM_ESS, TRIM_BINS=TRIM_BINS,
                               DOF_FALLBACK=DOF_FALLBACK, rng=self.rng, student_em=config.student_em)
        self.resampler = Resampler(state=state, n_particles=self.n_local, resample=config.resample,
                                   clusterer=clusterer, clustering=config.clustering,
                                   have_blobs=config.blobs_dtype is not None, rng=self.rng)
        self.mutator = Mutator(state=state, prior_transform=config.prior_transform, log_likelihood=self._log_like,
                               pbar=None, n_particles=self.n_local, n_dim=config.n_dim, n_steps=config.n_steps,
                               n_max_steps=config.n_max_steps, sampler=config.sample, periodic=config.periodic,
                               reflective=config.reflective, have_blobs=config.blobs_dtype is not None, rng=self.rng,
                               graph=config.graph)
        self.pbar = None
        self.t0 = 0
        self.timing = {"reweight": 0.0, "train": 0.0, "resample": 0.0, "mutate": 0.0, "commit": 0.0}

    # ---------------------------------------------------------------------------- run loop
    def _ensure_callbacks(self):
        w = getattr(self, "_warm", None)
        if w is not None:
            w.wait()                      # the process's one-time start-up, running in parallel since the construction
        if self.callbacks is None:
            self.callbacks = CallbackAdapter(self.config, self.state.device, self._get_distribute_func)
            self.mutator.device_callbacks = (self.callbacks.prior, self.callbacks.loglike)

    def run_sampling(self, n_total: int = 4096, progress: bool = True,
                     resume_state_path: Optional[Union[str, Path]] = None, save_every: Optional[int] = None) -> None:
        if resume_state_path is not None:
            self._initialize_from_resume(resume_state_path)
            it = self.state.get_current("iter")
            t0 = int(it) if it is not None else 0
            if it is None:
                self.state.set_current("iter", t0)
        else:
            t0 = 0
            self._initialize_fresh()
        self.n_total = int(n_total)
        self.t0 = t0
        from .tools import ProgressBar
        show = progress and (self.state.comm is None or self.state.comm.rank == 0)
        self.pbar = ProgressBar(show, initial=t0)
        self._update_progress_bar_initial()
        self.reweighter.pbar = self.pbar
        self.trainer.pbar = self.pbar
        self.mutator.pbar = self.pbar if show else None

        while self._not_termination():
            self.execute_iteration(save_every=save_every, t0=t0, return_state=False)

        _, logz = self._logz_at(1.0)
        self.state.set_current("logz", logz)
        self.logz_err = None
        if save_every is not None:
            self.save_sampler_state(self._checkpoint_path("final"))
        self.pbar.close()

    def _checkpoint_path(self, tag: str) -> Path:
        """{output_dir}/{label}_{tag}.state (core.py:154-171); a sharded run writes a checkpoint directory, `.ckpt`."""
        comm = self.state.comm
        sharded = comm is not None and comm.active
        return self.config.output_dir / f"{self.config.output_label}_{tag}{'.ckpt' if sharded else '.state'}"

    def execute_iteration(self, save_every: Optional[int] = None, t0: int = 0, return_state: bool = True):
        """One PS iteration: reweight -> train -> resample -> mutate -> commit (core.py:162-185).  Returns host copies
        of the current state like the reference unless return_state=False (the run loop does not need them: for 10^5+
        particles that copy is megabytes over PCIe per iteration)."""
        self._ensure_callbacks()
        if self.state.get_current("iter") is None:
            self._initialize_fresh()
        if save_every is not None:
            it = self.state.get_current("iter")
            if (it - t0) % int(save_every) == 0 and it != t0:
                self.save_sampler_state(self._checkpoint_path(str(it)))
        if getattr(self, "profile", False):
            return self._execute_iteration_profiled()
        weights = self.reweighter.run()
        mode_stats = self.trainer.run(weights)
        self.resampler.run(weights)
        self.mutator.run(mode_stats)
        self._update_progress_bar()
        self.state.commit_current_to_history()
        return self.state.get_current() if return_state else None

    def _execute_iteration_profiled(self):
        """Same pipeline with a device synchronisation after each phase; accumulates wall seconds in self.timing
        (diagnostics only: the synchronisations remove the overlap the normal path has)."""
        import time
        import torch
        dev = self.state.device

        def lap(name, t0):
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            self.timing[name] += t1 - t0
            return t1
        t = time.perf_counter()
        weights = self.reweighter.run(); t = lap("reweight", t)
        mode_stats = self.trainer.run(weights); t = lap("train", t)
        self.resampler.run(weights); t = lap("resample", t)
        self.mutator.run(mode_stats); t = lap("mutate", t)
        self.state.commit_current_to_history(); lap("commit", t)
        return None

    def _logz_at(self, beta):
        m, s1, s2 = self.state.reweight_eval([beta])[0]
        return float(s1 * s1 / s2), float(m + np.log(s1))

    def _not_termination(self) -> bool:
        """Continue while (1 - beta >= 1e-4) or ESS(beta=1) < n_total (core.py:360-374)."""
        if self.state.get_history_length() == 0:
            return True
        beta = self.state.get_current("beta")
        if 1.0 - beta >= 1e-4:            # the first clause decides: ESS(beta = 1) -- one pass over the history -- is not needed
            return True
        ess, _ = self._logz_at(1.0)
        return ess < getattr(self, "n_total", 0)

    # ------------------------------------------------------------------------------ outputs
    def _select(self, trim_importance_weights, ess_trim, bins_trim):
        """The history rows a result uses, on this shard: a _Selection of the device weights at beta = 1 (w_dev), the device indices of
        the kept rows (sel; None: the first m_sel), their number and what their weights are divided by (wdiv), and the (m, s1) of the
        reweighting pass -- from the trim threshold and the compaction, both on the device.  On a sharded run the threshold is a
        statistic of the GLOBAL weight distribution, which the library finds without moving the weights
        (tph_trim_threshold_global), and the weights are already normalised by the global sum; m_sel is this shard's share of the
        kept rows, counted here, and a shard that keeps none has sel None."""
        st = self.state
        ctx = st.ctx
        ctx.use_current_stream()
        m, s1, _ = st.reweight_eval([1.0])[0]
        w_dev = ctx.weights(1.0, m, s1)
        sel, m_sel, wdiv = None, ctx.size, 1.0
        if trim_importance_weights:
            sharded = st.comm is not None and st.comm.active
            thr_dev, out = ctx.trim_threshold(w_dev, ess_trim, bins_trim, sync=True, global_=sharded)
            wdiv = float(out[1])
            m_sel = int((w_dev >= thr_dev[0]).sum().item()) if sharded else int(out[2])
            sel = ctx.compact_indices(w_dev, thr_dev[0:1], m_sel) if m_sel else None
        return _Selection(w_dev, sel, m_sel, wdiv, m, s1)

    def compute_posterior(self, resample=False, return_blobs=False, trim_importance_weights=True, return_logw=False,
                          ess_trim=0.99, bins_trim=1000):
        """Weighted posterior samples from the whole history (core.py:187-242): select, gather the rows, attach their blobs, on a
        sharded run gather the ranks' parts (every rank returns the posterior over the WHOLE history: rows of all shards, rank
        order), resample.  Threshold, compaction and the gather into row-major (M, d) stay on the device; only the kept rows
        cross PCIe or travel between ranks."""
        import torch
        from .tools import systematic_draw
        st = self.state
        ctx = st.ctx
        comm = st.comm if (st.comm is not None and st.comm.active) else None
        s = self._select(trim_importance_weights, ess_trim, bins_trim)
        sel, m_sel = s.sel, s.m_sel
        logw = None
        if return_logw:       # the untrimmed, normalised log-weights (core.py:233-242)
            nh = st.n_history_global()
            logw = ctx.logw(1.0, nh).cpu().numpy() - (float(s.m + np.log(s.s1)) + np.log(nh))
        x_dev, logl_dev, w_sel = ctx.posterior_rows(sel, m_sel, w=s.w_dev, wdiv=s.wdiv)
        if resample and comm is None:
            # one shard: the draw composes with the selection on the device and the rows are gathered once more
            pick = systematic_draw(ctx, w_sel, m_sel, np.random.random())
            sel = pick if sel is None else ctx.index_compose(sel, pick)
            x_dev, logl_dev, w_sel = ctx.posterior_rows(sel, m_sel)
        blobs = st.get_history("blobs", flat=True) if (self.config.blobs_dtype is not None and st._blobs) else None
        # derived quantities: pure functions of x, evaluated on the rows this call returns while they are on the device (a rank
        # with no kept rows: an empty (0, k) block)
        derive = self._derived_fn() if (return_blobs and blobs is None) else None
        if derive is not None:
            blobs = derive(x_dev)
        elif blobs is not None and sel is not None:
            blobs = blobs[sel.cpu().numpy()]
        x, logl = x_dev.cpu().numpy(), logl_dev.cpu().numpy()
        weights = np.ones(m_sel) / m_sel if w_sel is None else w_sel.cpu().numpy()
        if comm is not None:
            x, logl, weights = comm.gather_rows(x), comm.gather_rows(logl), comm.gather_rows(weights)
            if blobs is not None:
                blobs = comm.gather_rows(blobs)
            if logw is not None:
                logw = comm.gather_rows(logw)
            if resample:      # on the gathered host rows; the total is NumPy's sum of the gathered weights
                wt = torch.from_numpy(np.ascontiguousarray(weights)).to(ctx.device)
                idx = systematic_draw(ctx, wt, len(weights), np.random.random(), total=float(weights.sum())).cpu().numpy()
                x, logl = x[idx], logl[idx]
                if blobs is not None:
                    blobs = blobs[idx]
                weights = np.ones(len(idx)) / len(idx)
        out = [x, weights, logl]
        if return_blobs and blobs is not None:
            if derive is not None and blobs.ndim == 2 and blobs.shape[1] == 1:
                blobs = blobs[:, 0]              # one value per sample: (M,), the rule of _pack_blobs
            out.append(blobs)
        if return_logw:
            out.append(logw)
        return tuple(out)

    def _hip_owner(self, what, has, needs):
        """The HipCallbacks object the likelihood belongs to, with the optional part Sampler.`what` reduces over: refused otherwise."""
        from ._lib import TempestHipError
        from .hipcallbacks import HipCallbacks
        owner = getattr(self.config.log_likelihood, "__self__", None)
        if not isinstance(owner, HipCallbacks) or not getattr(owner, has):
            raise TempestHipError(f"Sampler.{what}: the likelihood is no HipCallbacks source {needs}")
        return owner

    def _weighted_rows(self, what, unbuilt, trim_importance_weights, ess_trim, bins_trim, owner=None, with_sel=False):
        """(x_dev, w_sel): the rows and weights compute_posterior returns (same selection and row order: the same _select and
        posterior_rows call), left on the device -- for `owner`, a HipCallbacks object, on its device; with_sel: (x_dev, w_sel, sel), sel their device indices into the history (None:
        its first rows).  One shard only: Sampler.`what` needs `unbuilt` to fold the ranks' parts."""
        st = self.state
        if st.comm is not None and st.comm.active:
            raise NotImplementedError(f"Sampler.{what} is not available on a sharded run yet: every rank holds a part of the rows, and "
                                      f"{unbuilt} (DESIGN.md section 10)")
        if owner is not None:
            self._with_device(owner)
        s = self._select(trim_importance_weights, ess_trim, bins_trim)
        x_dev, _, w_sel = st.ctx.posterior_rows(s.sel, s.m_sel, w=s.w_dev, wdiv=s.wdiv)
        return (x_dev, w_sel, s.sel) if with_sel else (x_dev, w_sel)

    def _with_device(self, hc):
        """`hc`, a HipCallbacks object, on this run's device if it has none yet."""
        if hc.device is None:
            hc.device = self.state.device
        return hc

    def compute_predictive(self, quantiles=(0.025, 0.5, 0.975), trim_importance_weights=True, ess_trim=0.99, bins_trim=1000):
        """Posterior predictive mean, variance and quantiles of the HipCallbacks source's predict(x, r) over the rows and weights
        compute_posterior returns (same selection, on the device): the rows are gathered and reduced there, only the
        (n_predict,) results reach the host."""
        owner = self._hip_owner("predictive", "n_predict", "that defines predict(...) (give it and n_predict=)")
        x_dev, w_sel = self._weighted_rows("predictive", "folding per-rank partial sums and bucket totals is not built",
                                           trim_importance_weights, ess_trim, bins_trim, owner)
        return owner.predictive(x_dev, w_sel, quantiles)

    def compute_replicated(self, quantiles=(0.025, 0.5, 0.975), seed=None, trim_importance_weights=True, ess_trim=0.99, bins_trim=1000):
        """Replicated-data bands, PIT and Bayesian p-value of the HipCallbacks source's replicate(x, r, g) over the rows and weights
        compute_posterior returns (same selection and row order, on the device): the rows are gathered and reduced there, only the
        (n_replicate,) results reach the host.  seed None: the run's seed."""
        owner = self._hip_owner("replicated", "n_replicate", "that defines replicate(...) (give it and n_replicate=)")
        x_dev, w_sel = self._weighted_rows("replicated", "a global row index for the draws and folding per-rank sums and counts are not built",
                                           trim_importance_weights, ess_trim, bins_trim, owner)
        return owner.replicated(x_dev, w_sel, quantiles, seed=self.rng.seed if seed is None else seed)

    _psis_rows = None          # the equally weighted rows the last compute_pointwise handed to psis_loo (tests)

    def compute_pointwise(self, trim_importance_weights=True, ess_trim=0.99, bins_trim=1000, psis_draws=None, seed=None):
        """Pointwise log predictive densities, WAIC and importance-sampling LOO of a pointwise-enabled HipCallbacks source over the
        rows and weights compute_posterior returns (same selection, on the device): the rows are gathered and reduced there, only
        the (n_terms,) results reach the host.  A source built with pointwise="psis" adds the Pareto-smoothed values of
        HipCallbacks.psis_loo over psis_draws (None: as many as there are weighted rows) equally weighted rows, drawn from the
        weighted ones by systematic resampling on the device at the offset `seed` (None: the run's seed) gives."""
        owner = self._hip_owner("pointwise", "pointwise_enabled",
                                "built with pointwise=True (give it, with a source that defines log_likelihood_term)")
        x_dev, w_sel, sel = self._weighted_rows("pointwise", "folding per-rank maxima, minima and partial sums is not built",
                                                trim_importance_weights, ess_trim, bins_trim, owner, with_sel=True)
        res = owner.pointwise(x_dev, w_sel)
        if owner.psis_enabled:
            from .hipcallbacks import PSIS_KEYS
            from .tools import systematic_draw
            n_draws = x_dev.shape[0] if psis_draws is None else psis_draws
            if isinstance(n_draws, bool) or not isinstance(n_draws, (int, np.integer)) or int(n_draws) <= 0:
                raise ValueError(f"Sampler.pointwise: psis_draws must be a positive int, got {psis_draws!r}")
            ctx = self.state.ctx
            u0 = float(np.random.default_rng(self.rng.seed if seed is None else seed).random())
            pick = systematic_draw(ctx, w_sel, int(n_draws), u0)
            rows, _, _ = ctx.posterior_rows(pick if sel is None else ctx.index_compose(sel, pick), int(n_draws))
            self._psis_rows = rows
            ps = owner.psis_loo(rows)
            res.update((k, ps[k]) for k in PSIS_KEYS)
            res["totals"].update(ps["totals"], p_psis=res["totals"]["lppd"] - ps["totals"]["elpd_psis"], k_threshold=ps["k_threshold"])
        return res

    def compute_marginals(self, bins=64, range=None, quantiles=(0.025, 0.16, 0.5, 0.84, 0.975), pairs=None, bins_2d=32, derived=True,
                          trim_importance_weights=True, ess_trim=0.99, bins_trim=1000):
        """Marginal means, variances, quantiles and 1-D / 2-D histograms of the parameters -- and, with `derived`, of the derived
        quantities -- over the rows and weights compute_posterior returns (same selection, on the device): the rows stay there,
        only per-column arrays and the tables reach the host (HipContext.marginals)."""
        import torch
        x_dev, w_sel = self._weighted_rows("marginals", "folding per-rank minima, maxima, block sums and tables is not built",
                                           trim_importance_weights, ess_trim, bins_trim)
        n_dim, n_derived = x_dev.shape[1], 0
        src = self._derived_source() if derived else None
        if src is not None:
            if src.width is not None:        # a plugin's columns: evaluated where the rows are, and left there
                extra = src.fn(x_dev)
            else:                            # a user's function: its host (M, k) block is uploaded
                extra = torch.from_numpy(self._derived_fn(src)(x_dev)).to(x_dev.device)
            extra = extra.to(torch.float64).reshape(x_dev.shape[0], -1)
            n_derived = extra.shape[1]
            x_dev = torch.cat([x_dev, extra], dim=1).contiguous()
        out = self.state.ctx.marginals(x_dev, w_sel, bins=bins, range=range, quantiles=quantiles, pairs=pairs, bins_2d=bins_2d)
        out.update(n_dim=int(n_dim), n_derived=int(n_derived))
        return out

    def _derived_source(self):
        """Where the derived quantities come from -- config.derived, else the `derived` of the HipCallbacks object the likelihood
        belongs to -- as a _Derived: fn, on_device (fn takes the device rows; else their host copy) and width (a plugin's column
        count, known without a call; None for a user's function).  None without a derived function."""
        from .hipcallbacks import HipCallbacks
        fn = self.config.derived
        owner = getattr(self.config.log_likelihood, "__self__", None)
        if fn is None and isinstance(owner, HipCallbacks) and owner.n_derived > 0:
            fn = owner.derived
        if fn is None:
            return None
        plugin = getattr(fn, "__self__", None)
        if isinstance(plugin, HipCallbacks):
            return _Derived(fn, True, self._with_device(plugin).n_derived)
        backend = self.config.backend
        if backend == "auto":
            self._ensure_callbacks()
            if self.callbacks.backend is None:
                self.callbacks._probe()
            backend = self.callbacks.backend
        return _Derived(fn, backend == "torch", None)

    def _derived_fn(self, src=None):
        """rows (M, d) on the device -> the derived quantities of _derived_source (`src`, if the caller has it) as a host (M, k)
        float64 array, or None without a derived function."""
        import torch
        if src is None:
            src = self._derived_source()
        if src is None:
            return None
        fn, on_device, width = src

        def run(x_dev):
            m = x_dev.shape[0]
            if m == 0 and width is not None:     # a rank with no kept rows: an empty (0, k) block, nothing launched
                return np.empty((0, width), dtype=np.float64)
            # (a user's callable gets the (0, d) array itself -- no made-up row that might lie outside its domain -- and must
            # answer with (0, k), as every vectorised NumPy / torch expression does)
            b = fn(x_dev) if on_device else fn(x_dev.cpu().numpy())
            if isinstance(b, torch.Tensor):
                b = b.detach().to("cpu", torch.float64).numpy()
            b = np.ascontiguousarray(b, dtype=np.float64)
            if b.ndim == 1:
                b = b.reshape(m, 1)
            if b.ndim != 2 or b.shape[0] != m:
                raise ValueError(f"derived: expected ({m}, k) values for ({m}, {x_dev.shape[1]}) points, got shape {b.shape}")
            return b
        return run

    def compute_evidence(self):
        return self.state.get_current("logz"), getattr(self, "logz_err", None)

    # -------------------------------------------------------------------------- persistence
    def save_sampler_state(self, path: Union[str, Path], format: Optional[str] = None):
        """Reference layout {_current, _history, n_dim, random_state, n_total, logz_err} (core.py:249-279);
        the callbacks are not pickled (the reference's `sampler=dill.dumps(core)` entry is omitted).  `format="native"`,
        a path ending in ".ckpt", or a sharded run write the directory format of tempest_amd/checkpoint.py instead."""
        import dill
        from . import checkpoint
        path = Path(path)
        if checkpoint.wants_native(path, format, self.state.comm):
            return checkpoint.save(self, path)
        path.parent.mkdir(parents=True, exist_ok=True)
        d = self.state.to_dict()
        d["random_state"] = self.config.random_state
        d["n_total"] = getattr(self, "n_total", None)
        d["logz_err"] = getattr(self, "logz_err", None)
        d["rng"] = (self.rng.seed, self.rng.tick)
        with open(path, "wb") as f:
            dill.dump(d, f)

    def load_sampler_state(self, path: Union[str, Path]):
        """Restore current state AND history (the reference drops the history, core.py:289)."""
        import dill
        from . import checkpoint
        if checkpoint.is_native(path):
            checkpoint.load(self, path)
            defaults = {"iter": 0, "calls": 0, "beta": 0.0, "logz": 0.0, "steps": 0, "acceptance": 0.0,
                        "efficiency": 0.0, "cv": None}
            for key, val in defaults.items():
                if self.state.get_current(key) is None:
                    self.state.set_current(key, val)
            return
        with open(Path(path), "rb") as f:
            d = dill.load(f)
        self.state.update_from_dict(d)
        defaults = {"iter": 0, "calls": 0, "beta": 0.0, "logz": 0.0, "steps": 0, "acceptance": 0.0, "efficiency": 0.0,
                    "cv": None}
        for key, val in defaults.items():
            if self.state.get_current(key) is None:
                self.state.set_current(key, val)
        if "n_total" in d:
            self.n_total = d["n_total"]
        if "logz_err" in d:
            self.logz_err = d["logz_err"]
        if d.get("rng") is not None:
            self.rng.seed, self.rng.tick = d["rng"]
        elif d.get("random_state") is not None:
            np.random.seed(d["random_state"])

    # ------------------------------------------------------------------------------ helpers
    def _log_like(self, x):
        """Host-array likelihood in the reference's (logl, blobs) convention (core.py:317-358)."""
        self._ensure_callbacks()
        return self.callbacks.loglike_host(np.asarray(x))

    def _initialize_fresh(self):
        self.state.update_current({"iter": 0, "calls": 0, "beta": 0.0, "logz": 0.0})

    def _initialize_from_resume(self, path):
        self.load_sampler_state(path)
        it = self.state.get_current("iter")
        self.t0 = int(it) if it is not None else 0

    def _update_progress_bar_initial(self):
        if self.pbar is not None:
            self.pbar.update_stats(dict(beta=0.0, calls=0, ESS=int(self.config.ess_ratio * self.config.n_particles),
                                        logZ=0.0, logL=0.0, acc=0.0, steps=0, eff=0.0, K=1))

    def _update_progress_bar(self):
        if self.pbar is None or self.pbar.progress_bar.disable:
            return
        cur = self.state._current
        logl = cur["logl"]
        stats = dict(calls=cur["calls"], beta=cur["beta"], ESS=int(cur["ess"]), logZ=cur["logz"],
                     logL=float(logl.mean().item()) if logl is not None else 0.0, acc=cur["acceptance"],
                     steps=cur["steps"], eff=cur["efficiency"])
        if cur.get("cv") is not None:
            stats["CV"] = cur["cv"]
        self.pbar.update_stats(stats)

    def _get_distribute_func(self):
        pool = self.config.pool
        if pool is None:
            return map
        if isinstance(pool, int) and pool > 1:
            if getattr(self, "_pool", None) is None:       # one pool for the run, not one per call
                from multiprocess import Pool
                self._pool = Pool(pool)
            return self._pool.map
        return pool.map
