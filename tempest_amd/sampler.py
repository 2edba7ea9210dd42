"""Public facade: `tempest_amd.Sampler` is a drop-in for `tempest.Sampler` (tempest/sampler.py:12-406):
same constructor parameters and defaults, same methods, same read-only properties.  Everything numeric runs
on the MI355X through libtempest_hip.so; GPU-specific options are keyword-only."""
from __future__ import annotations

from pathlib import Path
from typing import Optional, Union

from .config import SamplerConfig
from .core import SamplerCore
from .state_manager import StateManager
from .tools import FunctionWrapper


class Sampler:
    def __init__(
        self,
        prior_transform: callable,
        log_likelihood: callable,
        n_dim: int,
        n_particles: Optional[int] = None,
        ess_ratio: float = 2.0,
        volume_variation: Optional[float] = None,
        log_likelihood_args: Optional[list] = None,
        log_likelihood_kwargs: Optional[dict] = None,
        vectorize: bool = False,
        blobs_dtype: Optional[str] = None,
        periodic: Optional[list] = None,
        reflective: Optional[list] = None,
        pool: Optional[Union[int, object]] = None,
        clustering: bool = True,
        normalize: bool = True,
        cluster_every: int = 1,
        split_threshold: float = 1.0,
        n_max_clusters: Optional[int] = None,
        sample: str = "tpcn",
        n_steps: Optional[int] = None,
        n_max_steps: Optional[int] = None,
        resample: str = "mult",
        output_dir: Optional[str] = None,
        output_label: Optional[str] = None,
        random_state: Optional[int] = None,
        *,
        device: Optional[Union[int, str]] = None,
        backend: str = "auto",
        batch_prior: Optional[bool] = None,
        graph: Optional[bool] = None,
        distributed: Optional[bool] = None,
        student_em: bool = False,
        derived: Optional[callable] = None,
    ):
        """GPU additions (keyword-only):
        device      -- GPU index (default: current torch device; LOCAL_RANK under torchrun).
        backend     -- "torch": callbacks receive torch-ROCm FP64 tensors (x is an (n, n_dim) strided view of the
                       SoA buffer) and return tensors; "numpy": callbacks receive NumPy arrays staged through the
                       host; "auto" (default) probes.
        batch_prior -- True if prior_transform accepts an (n, n_dim) batch (probed when None).
        graph       -- True: with device callbacks the MCMC step (proposal, both callbacks, Metropolis update,
                       adaptation) is captured once as a hipGraph and replayed; the callbacks must then be pure device
                       functions of their argument (no host synchronisation, no Python side effects per call -- a
                       callback that cannot be captured falls back with a warning).  False: launch every step's
                       kernels one by one.  None (default): graph when the shard is small enough for the step to be
                       launch-bound (n_particles_per_gpu * n_dim <= 2^19).
        student_em  -- True: every proposal mode's (mu, Sigma, nu) comes from the Student-t EM of tempest/student.py:66-116 with a
                       working degrees-of-freedom update, started from the default estimator (an EXTENSION: the reference's
                       own loop returns its start values with nu = inf -> dof_fallback; see tempest_amd/student.py).  One GPU only.
        derived     -- vectorised callable (n, n_dim) -> (n, k) [or (n,)]: derived quantities that are pure functions of x (and of
                       the data the callable holds).  Evaluated only by posterior(return_blobs=True), on the returned rows, and
                       handed back as the blobs (float64).  It gets a torch tensor under backend="torch", a NumPy array otherwise.
                       None (default): the `derived` of the HipCallbacks object `log_likelihood` belongs to, if its source has one.
                       Not state: never written into a checkpoint.  On a sharded run a rank that keeps no rows calls it with
                       a (0, n_dim) array and expects (0, k) back.
        distributed -- shard the particles over the ranks of the initialised torch.distributed group
                       (default: yes if a group is initialised); n_particles is the GLOBAL count."""
        if (log_likelihood_args or log_likelihood_kwargs) and \
                type(getattr(log_likelihood, "__self__", None)).__name__ == "HipCallbacks":
            raise ValueError("log_likelihood_args / log_likelihood_kwargs cannot reach a HipCallbacks likelihood (a device function): "
                             "pass the arrays as HipCallbacks(source, n_dim, data={...}) and read them from the table `D`")
        wrapped = FunctionWrapper(log_likelihood, log_likelihood_args, log_likelihood_kwargs) \
            if (log_likelihood_args or log_likelihood_kwargs) else log_likelihood
        config = SamplerConfig(
            prior_transform=prior_transform, log_likelihood=wrapped, n_dim=n_dim, n_particles=n_particles,
            ess_ratio=ess_ratio, volume_variation=volume_variation, log_likelihood_args=log_likelihood_args,
            log_likelihood_kwargs=log_likelihood_kwargs, vectorize=vectorize, blobs_dtype=blobs_dtype,
            periodic=periodic, reflective=reflective, pool=pool, clustering=clustering, normalize=normalize,
            cluster_every=cluster_every, split_threshold=split_threshold, n_max_clusters=n_max_clusters,
            sample=sample, n_steps=n_steps, n_max_steps=n_max_steps, resample=resample, output_dir=output_dir,
            output_label=output_label, random_state=random_state, device=device, backend=backend,
            batch_prior=batch_prior, graph=graph, student_em=student_em, derived=derived)
        comm = None
        if distributed is not False:
            from .comm import Comm
            c = Comm()
            if c.active:
                comm = c
            elif distributed:
                raise ValueError("distributed=True needs an initialised torch.distributed process group")
        if config.student_em and comm is not None:
            # rejected here, before any rank has sampled the prior: inside the first Trainer.run the other ranks would already
            # be waiting at a collective
            raise ValueError("student_em=True is not available on a sharded run (the Student-t EM is a one-GPU extension)")
        # reserve the history of a typical run (~40-60 PS iterations) up front: growing it later means hipMalloc + copy +
        # hipFree of gigabytes in the middle of the run (measured: one 230 ms stall at the 16M -> 32M row step)
        world = comm.world_size if (comm is not None and comm.active) else 1
        state = StateManager(n_dim, device=device, comm=comm, capacity_hint=64 * max(1, config.n_particles // world))
        self._core = SamplerCore(config, state)
        self.state = state
        # process start-up (first-use code-object loads, copy path, device context) in parallel, behind the construction
        from . import _warm
        self._core._warm = _warm.start(config, state)

    @property
    def startup_breakdown(self) -> dict:
        """What the parallel start-up of this Sampler's process cost (tempest_amd/_warm.py); empty for later Samplers."""
        w = getattr(self._core, "_warm", None)
        return w.breakdown() if w is not None else {}

    # ------------------------------------------------------------------------------- methods
    def run(self, n_total: int = 4096, progress: bool = True, resume_state_path: Union[str, Path, None] = None,
            save_every: Optional[int] = None):
        """Run Persistent Sampling until beta = 1 and the ESS of the whole history reaches n_total."""
        return self._core.run_sampling(n_total=n_total, progress=progress, resume_state_path=resume_state_path,
                                       save_every=save_every)

    def sample(self, save_every: Optional[int] = None, t0: int = 0, *, return_state: bool = True) -> dict:
        """One iteration (reweight, train, resample, mutate, commit); returns host copies of the current state
        (the reference's contract).  return_state=False skips that device-to-host copy."""
        return self._core.execute_iteration(save_every=save_every, t0=t0, return_state=return_state)

    def posterior(self, resample: bool = False, return_blobs: bool = False, trim_importance_weights: bool = True,
                  return_logw: bool = False, ess_trim: float = 0.99, bins_trim: int = 1000) -> tuple:
        """(x, weights, logl[, blobs][, logw]) over the whole history, NumPy, C-contiguous, copies.  The blobs are the host
        likelihood's (blobs_dtype), or the derived quantities of the returned rows (`derived=`, or a HipCallbacks source with
        derived()): evaluated here, on the device, from x.  Without either there is no blobs entry."""
        return self._core.compute_posterior(resample=resample, return_blobs=return_blobs,
                                            trim_importance_weights=trim_importance_weights, return_logw=return_logw,
                                            ess_trim=ess_trim, bins_trim=bins_trim)

    def predictive(self, quantiles=(0.025, 0.5, 0.975), trim_importance_weights: bool = True, ess_trim: float = 0.99,
                   bins_trim: int = 1000) -> dict:
        """Posterior predictive of a HipCallbacks source's predict(x, r), r = 0 .. n_predict - 1, over the weighted rows posterior()
        returns: {"mean", "var": (n_predict,), "quantiles": (len(quantiles), n_predict), "n_rows", "ess"}, NumPy.  The rows stay on
        the device; nothing of size rows x n_predict is formed.  Not available on a sharded run (NotImplementedError)."""
        return self._core.compute_predictive(quantiles=quantiles, trim_importance_weights=trim_importance_weights,
                                             ess_trim=ess_trim, bins_trim=bins_trim)

    def replicated(self, quantiles=(0.025, 0.5, 0.975), seed: Optional[int] = None, trim_importance_weights: bool = True,
                   ess_trim: float = 0.99, bins_trim: int = 1000) -> dict:
        """Posterior predictive check of a HipCallbacks source's replicate(x, r, g), r = 0 .. n_replicate - 1, over the weighted rows
        posterior() returns, in its row order: {"mean", "var": (n_replicate,), "quantiles": (len(quantiles), n_replicate), "n_rows",
        "ess", "seed"}, with observed= "pit" (n_replicate,), with discrepancy() "p_value", "t_obs_mean", "t_rep_mean", NumPy
        (HipCallbacks.replicated; the same numbers as cb.replicated(x, w, seed=seed) on posterior()'s x and w).  seed None: the run's
        seed.  The rows stay on the device; nothing of size rows x n_replicate is formed.  Not available on a sharded run
        (NotImplementedError)."""
        return self._core.compute_replicated(quantiles=quantiles, seed=seed, trim_importance_weights=trim_importance_weights,
                                             ess_trim=ess_trim, bins_trim=bins_trim)

    def pointwise(self, trim_importance_weights: bool = True, ess_trim: float = 0.99, bins_trim: int = 1000,
                  psis_draws: Optional[int] = None, seed: Optional[int] = None) -> dict:
        """Pointwise log predictive densities of a HipCallbacks term-form source built with pointwise=True, over the weighted rows
        posterior() returns: {"lppd", "mean", "p_waic", "elpd_waic", "elpd_loo", "ess_loo": (n_terms,), "n_rows", "ess", "totals"},
        NumPy (HipCallbacks.pointwise).  The rows stay on the device; nothing of size rows x n_terms is formed.  Not available on a
        sharded run (NotImplementedError).

        A source built with pointwise="psis" adds "pareto_k", "elpd_psis", "ess_psis" (n_terms,) and, in "totals", elpd_psis,
        elpd_psis_se, p_psis = lppd - elpd_psis, n_high_k and k_threshold (HipCallbacks.psis_loo).  Pareto smoothing is defined for
        equally weighted rows: psis_draws of them (None: as many as there are weighted rows) are drawn from the weighted ones by
        systematic resampling on the device, at the offset `seed` gives (None: the run's seed) -- the same seed, the same bits."""
        return self._core.compute_pointwise(trim_importance_weights=trim_importance_weights, ess_trim=ess_trim, bins_trim=bins_trim,
                                            psis_draws=psis_draws, seed=seed)

    def marginals(self, bins: int = 64, range=None, quantiles=(0.025, 0.16, 0.5, 0.84, 0.975), pairs=None, bins_2d: int = 32,
                  derived: bool = True, trim_importance_weights: bool = True, ess_trim: float = 0.99, bins_trim: int = 1000) -> dict:
        """Marginals of the posterior over the weighted rows posterior() returns, reduced on the device: {"mean", "var": (c,),
        "quantiles": (len(quantiles), c), "range": (c, 2), "edges", "counts", "mass": (c, bins), "outside", "pairs", "counts_2d":
        (P, bins_2d, bins_2d), "outside_2d", "edges_2d", "sum_k", "n_rows", "ess", "n_dim", "n_derived"}, NumPy, c = n_dim +
        n_derived columns (derived=False: the parameters alone).  `range`: (lo, hi) or (c, 2), else the weighted rows' own; `pairs`:
        None, "all" or index pairs.  Works with every kind of callback; the rows stay on the device (HipContext.marginals,
        tempest_amd.marginals.hpd_levels for contour heights).  Not available on a sharded run (NotImplementedError)."""
        return self._core.compute_marginals(bins=bins, range=range, quantiles=quantiles, pairs=pairs, bins_2d=bins_2d, derived=derived,
                                            trim_importance_weights=trim_importance_weights, ess_trim=ess_trim, bins_trim=bins_trim)

    def evidence(self) -> tuple:
        """(logZ, None): the reference never computes an error estimate (core.py:151,244-247)."""
        return self._core.compute_evidence()

    def results(self):
        return self.state.compute_results()

    def save_state(self, path: Union[str, Path], *, format: Optional[str] = None):
        """format=None: the reference's dill layout, unless `path` ends in ".ckpt" or the run is sharded over several
        GPUs -- then (and with format="native") a checkpoint directory of raw per-shard dumps (checkpoint.py)."""
        self._core.save_sampler_state(Path(path), format=format)

    def load_state(self, path: Union[str, Path]):
        self._core.load_sampler_state(Path(path))

    # ---------------------------------------------------------------------------- properties
    n_dim = property(lambda self: self._core.config.n_dim)
    n_particles = property(lambda self: self._core.config.n_particles)
    ess_ratio = property(lambda self: self._core.config.ess_ratio)
    volume_variation = property(lambda self: self._core.config.volume_variation)
    n_steps = property(lambda self: self._core.config.n_steps)
    n_max_steps = property(lambda self: self._core.config.n_max_steps)
    n_total = property(lambda self: getattr(self._core, "n_total", None))
    resample = property(lambda self: self._core.config.resample)
    clustering = property(lambda self: self._core.config.clustering)
    vectorize = property(lambda self: self._core.config.vectorize)
    output_dir = property(lambda self: self._core.config.output_dir)
    output_label = property(lambda self: self._core.config.output_label)
    random_state = property(lambda self: self._core.config.random_state)
    periodic = property(lambda self: self._core.config.periodic)
    reflective = property(lambda self: self._core.config.reflective)
    beta = property(lambda self: self.state.get_current("beta"))
    logz = property(lambda self: self.state.get_current("logz"))
    ess = property(lambda self: self.state.get_current("ess"))
    cv = property(lambda self: self.state.get_current("cv"))
