"""MCMC mutation on the device (reference: tempest/mcmc.py).

Host control only: the per-step loop of BaseMCMCRunner.run (mcmc.py:142-208) with its proposal,
acceptance, sigma adaptation and adaptive stopping rule executed by the HIP kernels of
csrc/mutate.hip.  The two user callbacks are the only other work in a step.  Steps before the
minimum step count need no host synchronisation (the rule cannot fire earlier, mcmc.py:119-131);
afterwards one 48-byte state read per step decides whether to stop, exactly where the reference
evaluates `_check_convergence`; that read overlaps with the (speculative) proposal of the next step.
"""
from typing import Callable, Optional

import numpy as np

from .regime import REGIME_THRESHOLDS, Regime, RegimeOptions, regime_band  # noqa: F401  (the d > 16 proposal rule: regime.py)


class PhiloxStream:
    """Host side of the counter-based RNG: a 64-bit seed and the tick handed to each RNG-consuming launch."""

    def __init__(self, seed: int):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.tick = 0

    def next(self) -> int:
        self.tick = (self.tick + 1) & 0xFFFFFFFF
        return self.tick


def _bc_flags(n_dim, periodic, reflective):
    f = np.zeros(n_dim, dtype=np.uint8)
    if periodic is not None and len(periodic):
        f[np.asarray(periodic, dtype=int)] = 1
    if reflective is not None and len(reflective):
        f[np.asarray(reflective, dtype=int)] = 2
    return f


def apply_boundary_conditions(u, periodic=None, reflective=None):
    """Wrap periodic and fold reflective coordinates into [0, 1] (mcmc.py:326-366).  Host utility with the
    same arithmetic as the device proposal kernel (`v % 1.0`; floor parity flip)."""
    out = np.array(u, dtype=np.float64, copy=True)
    flags = _bc_flags(out.shape[-1], periodic, reflective)
    for j in np.nonzero(flags == 1)[0]:
        out[..., j] = np.mod(out[..., j], 1.0)
    for j in np.nonzero(flags == 2)[0]:
        v = out[..., j]
        k = np.floor(v)
        frac = v - k
        out[..., j] = np.where(np.mod(k, 2.0) == 0.0, frac, 1.0 - frac)
    return out


def check_bounds(u, periodic=None, reflective=None):
    """True where every coordinate WITHOUT a boundary condition lies in [0, 1] (mcmc.py:369-411)."""
    u = np.asarray(u)
    strict = np.nonzero(_bc_flags(u.shape[-1], periodic, reflective) == 0)[0]
    if strict.size == 0:
        return True if u.ndim == 1 else np.ones(u.shape[0], dtype=bool)
    s = u[..., strict]
    inside = (s >= 0) & (s <= 1)
    return bool(inside.all()) if u.ndim == 1 else inside.all(axis=-1)


class StepEngine:
    """One MCMC step -- proposal, the two user callbacks, Metropolis update, sigma adaptation -- as a replayable
    hipGraph over persistent device buffers.

    A step at BASELINE config 4's shard size (131 072 particles, d = 10) is ~15 launches of 5-50 us kernels: issued one
    by one from Python the host cannot keep the GPU busy.  Everything that changes from step to step (RNG tick, stop
    flag) and from one PS iteration to the next (beta, tick base, proposal modes, the active set itself) lives in device
    memory -- the step-control block of tempest_hip.h and the buffers below -- so the graph is captured once per
    (n, K) and replayed for every later step of the run.  Steps launched past the stopping rule are no-ops on the
    device, so the host may run one step ahead of the 64-byte state read that tells it when to stop.

    With a communicator the per-rank sums are all-reduced between the Metropolis kernel and tph_adapt: by the library's
    peer-to-peer exchange kernel when that is attached (tph_comm_p2p_*; part of the step and of its graph), else by the
    host through the process group between the replay and an eagerly launched tph_adapt.  The user callbacks must be pure device functions of their argument
    (they are traced once); `graph=False` keeps the step-by-step launch path."""

    SLOTS = 64          # mailbox ring: the host never runs more than a few steps ahead of the record it waits for
    _epoch = 0          # version counter of the mode statistics handed to the library (TPH_OPT_MODES_EPOCH)
    blocked = property(lambda self: self.regime.blocked)        # the regime's parts, read by tests and tools
    staged = property(lambda self: self.regime.staged)
    unstaged = property(lambda self: self.regime.unstaged)
    sm_lanes = property(lambda self: self.regime.sm_lanes)

    def __init__(self, ctx, kernel, n, K, has_assign, bc, log_likelihood, prior_transform, seed, item0, n_global,
                 n_steps, n_max, comm_active, use_graph=True, plugin=None):
        import os
        import torch
        from types import SimpleNamespace
        from .device import STEP_STATE_LEN, vshards_for
        self.plugin = plugin
        d = ctx.n_dim
        self.ctx, self.kernel, self.n, self.K, self.bc = ctx, kernel, n, K, bc
        self.loglike, self.prior = log_likelihood, prior_transform
        self.seed, self.item0, self.n_global = seed, item0, n_global
        self.n_steps, self.n_max, self.comm_active = n_steps, n_max, comm_active
        # with the library's peer-to-peer exchange attached, the all-reduce of the step's sums is a kernel on the ctx stream:
        # it belongs to the step (and to its graph) like every other launch; otherwise the host calls the process group
        # (this rank's shard sums -- vl (1 + K) doubles, vl = its virtual shards of the canonical partition -- must fit one slot)
        world = max(1, int(round(n_global / n))) if n else 1
        vl = vshards_for(n * world) // world if (n * world) % 256 == 0 and vshards_for(n * world) % world == 0 else 1
        self.inline_reduce = bool(comm_active and ctx.p2p_active and 8 * vl * (1 + K) <= 32768)   # one exchange slot (p2p.h)
        self.up, self.maha_u, self.maha_up = ctx.empty(d, n), ctx.empty(n), ctx.empty(n)
        self.u = self.logl = self.assign = self.modes = None
        if use_graph:       # fixed-address copies of everything a captured step reads or writes
            self.u, self.logl = ctx.empty(d, n), ctx.empty(n)
            self.assign = torch.empty(n, dtype=torch.int32, device=ctx.device) if has_assign else None
            self.modes = SimpleNamespace(K=K, means_dev=ctx.empty(K, d), chol_dev=ctx.empty(K, d, d),
                                         winv_dev=ctx.empty(K, d, d), dof_dev=ctx.empty(K))
        self.has_assign = has_assign
        self.sigmas, self.counts, self.sums = ctx.empty(K), ctx.empty(K), ctx.zeros(1 + K)
        self.partials = ctx.empty(((n + 255) // 256) * (1 + K))     # fixed address: the library's scratch may move
        # deferred Metropolis update: tph_accept records the decisions here, the NEXT tph_propose moves the accepted
        # proposals into place (its FP64 work hides the copy; in place it was a bandwidth-bound kernel of its own)
        self.pending = torch.zeros(n, dtype=torch.uint8, device=ctx.device)
        self.ctl = ctx.zeros(STEP_STATE_LEN)
        self.ctl_host = torch.zeros(STEP_STATE_LEN, dtype=torch.float64).pin_memory()
        self._opts = RegimeOptions.from_env()      # the regime's debugging switches, read here and nowhere in the step path
        self.regime = Regime.initial(d, K, has_assign, self._opts)      # the d > 16 proposal kernel of the next steps (regime.py)
        env = os.environ.get("TEMPEST_AMD_STEP_TIMEOUT")
        self._step_timeout = float(env) if env else None      # seconds a step's record may take (None: until the stream goes idle)
        # written by tph_adapt, polled here: the ring of step records and, behind it, the last record of a run made in ONE launch
        self._mail_all = torch.zeros(self.SLOTS + 1, 8, dtype=torch.float64).pin_memory()
        self.mailbox = self._mail_all[:self.SLOTS]
        self.mailbox_np = self.mailbox.numpy()
        self._run_bufs = None
        self.use_graph, self.graph, self.graph_error = bool(use_graph), None, None
        self._keep, self.runs, self._own = None, 0, None
        self._retired_graphs = []

    def load(self, u, x, logl, assign, modes, beta, tick_base, sigma_init, counts):
        """Start a run: active set, proposal modes and the step-control block.  A graph needs fixed addresses, so
        the data is copied into the engine's persistent buffers; without one the caller's tensors are used as they are."""
        import torch
        from .device import OPT_MODES_EPOCH
        self.runs += 1
        if self.use_graph:
            if self._own is None:
                self._own = (self.u, self.logl, self.assign, self.modes)
            self.u, self.logl, self.assign, self.modes = self._own
            self.u.copy_(u); self.logl.copy_(logl)
            if self.assign is not None:
                self.assign.copy_(assign)
            m = self.modes
            m.means_dev.copy_(modes.means_dev.reshape(m.means_dev.shape)); m.chol_dev.copy_(modes.chol_dev.reshape(m.chol_dev.shape))
            winv = modes.winv_dev if hasattr(modes, "winv_dev") else None
            if winv is None:            # mode statistics built outside ModeStatistics: L^-1 from the factors
                winv = torch.linalg.inv(modes.chol_dev.reshape(m.chol_dev.shape))
            m.winv_dev.copy_(winv.reshape(m.winv_dev.shape)); m.dof_dev.copy_(modes.dof_dev.reshape(m.dof_dev.shape))
        else:
            self.u, self.logl, self.assign, self.modes = u, logl, assign, modes
        if self.ctx.n_dim > 16:        # new mode statistics: the library rebuilds its blocked copies of L and L^-1 once
            StepEngine._epoch += 1
            self.ctx.set_option(OPT_MODES_EPOCH, StepEngine._epoch)
            self._push_options()       # the proposal regime is an option of the ctx, which engines of other shapes share: re-assert this engine's
        self.sigmas.fill_(sigma_init)
        self.pending.zero_()
        self.counts.copy_(counts)
        self.mailbox_np[:, 7] = -1.0          # no record yet (the device is idle or running no-op steps: see step())
        h = self.ctl_host
        h.zero_()
        h[6], h[7] = float(beta), float(tick_base)
        self.ctl.copy_(h, non_blocking=True)

    def _enqueue(self):
        """The launches of one step on the current stream (ticks are offsets: the device adds base + 2 * steps done)."""
        from .device import KERNEL_ID
        ctx = self.ctx
        if (self.plugin is not None and (not self.comm_active or self.inline_reduce)
                and self.plugin.can_fuse_step(self.K, self.assign is not None, self.n)):
            # proposal, callbacks and Metropolis update in ONE kernel of the user's plugin (hipcallbacks.py); with ranks only
            # when tph_adapt exchanges the sums itself (otherwise the host needs them between two launches)
            self.plugin.step(KERNEL_ID[self.kernel], self.u, self.logl, self.maha_u, self.modes, self.sigmas, self.bc,
                             self.seed, 1, 2, self.item0, self.ctl, self.partials)
            self._adapt(fold=True)
            return None, None
        ctx.propose(self.kernel, self.u, self.assign, self.modes, self.sigmas, self.bc, self.seed, 1, self.item0,
                    self.up, self.maha_u, self.maha_up, ctl=self.ctl, pending=self.pending)
        # the block partials of the Metropolis kernel are summed inside tph_adapt (one launch less per step), which on a
        # sharded run also exchanges the shard sums with the peers (tph_comm_p2p_*); without that exchange the ranks are combined
        # between the two launches (step(): tph_accept_sums_global)
        sums = None
        if self.plugin is not None and self.plugin.can_fuse_accept(self.n):   # callbacks compiled into the Metropolis kernel
            xp = lp = None                                                     # (hipcallbacks.py; not where its sum over data is split)
            self.plugin.accept(KERNEL_ID[self.kernel], 0.0, self.u, None, self.logl, self.up, self.maha_u, self.maha_up,
                               self.assign, self.K, self.modes.dof_dev, self.seed, 2, self.item0, sums,
                               ctl=self.ctl, partials=self.partials, pending=self.pending)
        else:
            xp = self.prior(self.up)
            lp = self.loglike(xp)
            ctx.accept(self.kernel, 0.0, self.u, None, self.logl, self.up, xp, lp, self.maha_u, self.maha_up,
                       self.assign, self.K, self.modes.dof_dev, self.seed, 2, self.item0, sums, ctl=self.ctl,
                       partials=self.partials, pending=self.pending)
        if not self.comm_active or self.inline_reduce:
            self._adapt(fold=True)
        return xp, lp

    def _adapt(self, fold=False):
        self.ctx.adapt(self.kernel, self.sums, self.counts, self.K, self.n_global, self.n_steps, self.n_max,
                       self.sigmas, self.ctl, mailbox=self.mailbox, partials=self.partials if fold else None, n=self.n)

    def can_run_all(self):
        """The whole run in one launch (HipCallbacks.run: every step, adaptation and stopping rule inside one cooperative kernel)?"""
        return (self.plugin is not None and not self.comm_active
                and self.plugin.can_run(self.K, self.assign is not None, self.n))

    def run_all(self):
        """Launch the run loaded by load() as ONE kernel and wait for its last step's record; None if the device refused the
        launch (nothing ran: step as usual)."""
        import torch
        from ._lib import TempestHipError
        from .device import KERNEL_ID
        if self._run_bufs is None:
            tiles = (self.n + 255) // 256
            self._run_bufs = (self.ctx.empty(4 * tiles), torch.zeros(4, dtype=torch.int32, device=self.ctx.device))
        partials2, barrier = self._run_bufs
        last = self._mail_all.numpy()[self.SLOTS]
        last[7] = -1.0
        d = self.ctx.n_dim
        if not self.plugin.run(KERNEL_ID[self.kernel], self.u, self.logl, self.maha_u, self.modes, self.sigmas, self.bc, self.seed,
                               1, 2, self.item0, self.ctl, partials2, barrier, self.counts, self.n_global, self.n_steps,
                               self.n_max, self._mail_all, self.SLOTS, self.n_max * d + 1):
            return None
        self._poll(last, None)
        if last[1] < 0.0:
            raise TempestHipError("MCMC run in one launch was abandoned on the device (a workgroup timed out at the grid barrier)")
        if last[1] == 0.0:
            raise TempestHipError("MCMC run in one launch ended without its stopping rule having fired")
        return last[:6].copy()

    def _poll(self, rec, step, timeout=None, late=None):
        """Spin on a pinned record until its sequence field shows `step` (None: the record of a run in one launch, any step).  The
        wait ends with an error only when the stream has gone IDLE without delivering the record (like tph_reweight_eval's poll)
        or, if a `timeout` in seconds is given (TEMPEST_AMD_STEP_TIMEOUT), after that long: a step may legitimately take minutes
        (an expensive likelihood, a callback that compiles on first use, a shared GPU).  `late` is called at every look at the
        clock once the wait has lasted two seconds."""
        import time
        import torch
        if timeout is None:
            timeout = self._step_timeout
        spins, t0 = 0, None
        while (not rec[7] >= 0.0 if step is None else rec[7] != step):
            spins += 1
            if spins & 0x3FFF == 0:
                # (everything an error needs is fetched here, off the path of a record that is already there: the step loop with
                # torch callbacks shows a microsecond of host work per step, profiles/regime_refactor_ab.json)
                from ._lib import TempestHipError
                what, record = ("the run", "the record") if step is None else (f"MCMC step {step}", "the step's record")
                now = time.monotonic()
                t0 = t0 or now
                if now - t0 > 0.05:
                    time.sleep(0)                 # long wait: let other Python threads run between polls
                if now - t0 > 2.0 and late is not None:
                    late()
                if (now - t0 > 2.0 and torch.cuda.current_stream(self.ctx.device).query()
                        and (not rec[7] >= 0.0 if step is None else rec[7] != step)):
                    raise TempestHipError(f"{what}: the stream is idle and the device never delivered {record}")
                if timeout is not None and now - t0 > timeout:
                    raise TempestHipError(f"{what}: no record from the device after {timeout} s")

    def wait_record(self, step, timeout=None):
        """State record (tph_adapt's state[0..5]) of step `step`, polled from the pinned mailbox; its redraw probe goes to the
        regime rule."""
        rec = self.mailbox_np[step % self.SLOTS]
        self._poll(rec, step, timeout, late=self.ctx.p2p_status)      # (raises if a peer never arrived at an exchange)
        self._regime(rec[6])
        return rec[:6].copy()

    def _push_options(self):
        """The engine's regime as options of the ctx: the one place that sets them."""
        from . import device
        for name, value in self.regime.options(self.ctx.n_dim, self._opts):
            self.ctx.set_option(getattr(device, name), value)

    def _regime(self, mean_attempts):
        """One reading of the redraw probe: the rule decides (Regime.next), the engine applies -- the regime's options into the
        ctx, and a captured graph, which has its kernels baked in, retired when the rule asks for another KERNEL than it holds
        (the step is captured again at its next launch)."""
        old = self.regime
        new = self.regime = old.next(mean_attempts, n_dim=self.ctx.n_dim, n=self.n, K=self.K, opts=self._opts,
                                     captured=self.graph is not None)
        if new is old:                 # nothing read (always so at d <= 16)
            return
        if new[:4] != old[:4]:
            self._push_options()
        if self.graph is not None and new.kernel != old.kernel:
            # retired, not destroyed: its last replay may still be in flight (and its pool holds the callbacks' outputs)
            self._retired_graphs.append((self.graph, self._keep))
            self.graph, self._keep = None, None

    def _capture(self):
        """Stream capture of one step (torch.cuda.CUDAGraph without torch.cuda.graph's empty_cache(), which would hand
        the allocator's cached blocks back to the driver in the middle of a run)."""
        import gc
        import torch
        ctx = self.ctx
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=ctx.device)
        side.wait_stream(torch.cuda.current_stream(ctx.device))
        began = False
        # No finaliser may run while the stream is capturing: one that frees device memory or synchronises (a tensor, a
        # HipContext or a CUDAGraph of an earlier Sampler that the cyclic collector happens to reach now) is an illegal call
        # during capture and aborts the process.  The collector is kept off for the duration of the capture (with it off no
        # cyclic garbage is ever finalised here; a full collection in front of every capture, as torch.cuda.graph() makes one,
        # cost 60 ms each -- 0.3 s of a 1 000-particle run's 2 s -- for nothing the switch does not already guarantee).
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.stream(side):
                ctx.use_current_stream()          # the capturing stream
                g.capture_begin()
                began = True
                self._keep = self._enqueue()      # callback outputs live in the graph's private pool
                g.capture_end()
            self.graph = g
        except Exception as e:                    # callbacks that synchronise or branch on data cannot be captured
            if began:
                try:
                    with torch.cuda.stream(side):
                        g.capture_end()
                except Exception:
                    pass
            self.graph, self.graph_error, self.use_graph, self._keep = None, e, False, None
            import warnings
            warnings.warn(f"MCMC step could not be captured as a graph ({type(e).__name__}: {e}); "
                          "launching step by step", stacklevel=2)
        finally:
            if gc_was_on:
                gc.enable()
            ctx.use_current_stream()
            torch.cuda.current_stream(ctx.device).wait_stream(side)

    def step(self, comm=None):
        """Enqueue one full step.  An engine's first run is launched step by step (it sizes the library's scratch, warms
        the callbacks, and a shape that never repeats -- a cluster count that changes every iteration -- never pays for a
        capture); the graph is captured after the first step of its second run and replayed from then on."""
        if self.graph is not None:
            self.graph.replay()
        else:
            self._enqueue()
            if self.use_graph and self.runs >= 2:
                self._capture()
        if self.comm_active and not self.inline_reduce:
            self.ctx.accept_sums_global(self.partials, self.n, self.K, self.sums)
            self._adapt()


class DeviceMCMC:
    """One mutation run over the active set held on a GPU context."""

    def __init__(self, ctx, kernel: str, beta: float, mode_stats, log_likelihood: Callable, prior_transform: Callable,
                 n_steps: int, n_max: int, periodic=None, reflective=None, rng: Optional[PhiloxStream] = None,
                 comm=None, item0: int = 0, n_global: Optional[int] = None, progress_bar=None, verbose=True,
                 engines: Optional[dict] = None, graph: Optional[bool] = None, plugin=None):
        """`engines`: a dict kept by the caller across runs; given one, the steps go through a StepEngine (persistent
        buffers + device-side step control), replayed as a hipGraph unless `graph` is False."""
        import torch
        self.engines, self.graph, self.plugin = engines, graph, plugin
        self.ctx, self.kernel, self.beta, self.modes = ctx, kernel, float(beta), mode_stats
        self.loglike, self.prior = log_likelihood, prior_transform
        self.n_steps, self.n_max = int(n_steps), int(n_max)
        self.rng = rng if rng is not None else PhiloxStream(np.random.randint(0, 2 ** 62))
        self.comm, self.item0, self.n_global = comm, int(item0), n_global
        self.pbar, self.verbose = progress_bar, verbose
        d = ctx.n_dim
        flags = _bc_flags(d, periodic, reflective)
        self.bc = torch.from_numpy(flags).to(ctx.device) if flags.any() else None
        self.sigma_0 = 2.38 / np.sqrt(d)

    def run(self, u, x, logl, assignments, blobs=None):
        """u, x: (d, n) device tensors (updated in place); logl (n,); assignments int32 (n,) or None.
        `blobs` (host array, one entry per particle): the likelihood's auxiliary outputs; those of accepted moves replace
        the current ones (mcmc.py:176-177) -- the log-likelihood callback is then called with return_blobs=True and must
        return (tensor, blobs); the evolved array is left in `self.blobs`.
        Returns (efficiency, acceptance, iterations, n_calls) like mcmc.py:196-208."""
        import torch
        from .device import KERNEL_ID
        self.blobs = None if blobs is None else np.array(blobs, copy=True)
        if blobs is not None and (self.engines is not None or self.plugin is not None):
            raise ValueError("blobs follow the step-by-step path (host callbacks): engines and plugin must be None")
        ctx, modes, d = self.ctx, self.modes, self.ctx.n_dim
        n = u.shape[1]
        n_global = n if self.n_global is None else self.n_global
        K = modes.K
        assign = assignments if K > 1 else None
        sig0 = min(self.sigma_0, 0.99) if self.kernel == "tpcn" else self.sigma_0      # mcmc.py:222-223,298-299
        counts = ctx.cluster_counts(assign, n, K)
        if self.engines is not None:
            return self._run_engine(u, x, logl, assign, K, n, n_global, sig0, counts)
        sigmas = torch.full((K,), sig0, dtype=torch.float64, device=ctx.device)
        state = ctx.zeros(6)
        sums = ctx.empty(1 + K)
        up, maha_u, maha_up = ctx.empty(d, n), ctx.empty(n), ctx.empty(n)
        active = self.comm is not None and self.comm.active
        if active:
            self.comm.all_reduce_sum(counts)
        n_min = self.n_steps * d
        it, calls = 0, 0
        st = None
        state_host = torch.empty(6, dtype=torch.float64).pin_memory()
        ev = torch.cuda.Event()
        speculated = False
        partials = ctx.empty(((n + 255) // 256) * (1 + K))

        def propose():
            ctx.propose(self.kernel, u, assign, modes, sigmas, self.bc, self.rng.seed, self.rng.next(), self.item0,
                        up, maha_u, maha_up)
        while True:
            it += 1
            if not speculated:
                propose()
            speculated = False
            calls += n_global
            if self.plugin is not None and self.plugin.can_fuse_accept(n):   # callbacks compiled into the Metropolis kernel
                # (hipcallbacks.py; not where its sum over data is split)
                self.plugin.accept(KERNEL_ID[self.kernel], self.beta, u, x, logl, up, maha_u, maha_up, assign, K,
                                   modes.dof_dev, self.rng.seed, self.rng.next(), self.item0, None, partials=partials)
            else:
                xp = self.prior(up)                   # (d, n) SoA tensor
                if self.blobs is None:
                    lp = self.loglike(xp)             # (n,) tensor
                else:
                    lp, bp = self.loglike(xp, return_blobs=True)
                ctx.accept(self.kernel, self.beta, u, x, logl, up, xp, lp, maha_u, maha_up, assign, K, modes.dof_dev,
                           self.rng.seed, self.rng.next(), self.item0, None, partials=partials)
                if self.blobs is not None:
                    # an accepted row now holds its proposal, bit for bit (a proposal equal to the current point -- the
                    # redraw cap -- has the current point's blob anyway)
                    moved = (u == up).all(dim=0).cpu().numpy()
                    self.blobs[moved] = np.asarray(bp)[moved]
            if active:          # this path runs host callbacks (or blobs): the ranks are paced by them, not by the device
                ctx.accept_sums_global(partials, n, K, sums, host_paced=True)
            # one GPU: tph_adapt sums the Metropolis kernel's block partials itself (one launch less per step)
            ctx.adapt(self.kernel, sums, counts, K, n_global, self.n_steps, self.n_max, sigmas, state,
                      partials=None if active else partials, n=n)
            if it >= n_min:
                # read the 48-byte step state while the NEXT step's proposal (which only needs the adapted sigma,
                # already ordered on the stream) is being generated; if the stopping rule fired it is discarded
                state_host.copy_(state, non_blocking=True)
                ev.record()
                propose()
                speculated = True
                ev.synchronize()
                st = state_host.numpy().copy()
                self._progress(n_global, st, it)
                if st[1] != 0.0:
                    break
        return float(st[4]), float(st[3]), it, calls

    def _progress(self, calls, st, steps):
        """Step record `st` to the progress bar, with `calls` more likelihood calls."""
        if self.pbar is not None and self.verbose:
            self.pbar.update_stats({"calls": self.pbar.info.get("calls", 0) + calls, "acc": st[3], "steps": steps, "eff": st[4]})

    def _run_engine(self, u, x, logl, assign, K, n, n_global, sig0, counts):
        ctx, d = self.ctx, self.ctx.n_dim
        active = self.comm is not None and self.comm.active
        if active:
            self.comm.all_reduce_sum(counts)
        key = (self.kernel, n, K, assign is not None, active, id(self.plugin))
        eng = self.engines.get(key)
        if eng is None:
            if len(self.engines) >= 2:        # at most two engines (and graph memory pools) alive at a time
                self.engines.pop(next(iter(self.engines)))
            eng = StepEngine(ctx, self.kernel, n, K, assign is not None, self.bc, self.loglike, self.prior, self.rng.seed,
                             self.item0, n_global, self.n_steps, self.n_max, active, use_graph=self.graph is not False,
                             plugin=self.plugin)
            self.engines[key] = eng
        eng.loglike, eng.prior, eng.plugin = self.loglike, self.prior, self.plugin
        tick_base = self.rng.tick
        eng.load(u, x, logl, assign, self.modes, self.beta, tick_base, sig0, counts)
        n_min = self.n_steps * d
        it, st = 0, None
        if eng.can_run_all():
            st = eng.run_all()                # every step of the run in one launch (None: refused, nothing ran)
            if st is not None:
                it = int(st[0])
                self._progress(it * n_global, st, it)
        if st is None:
            eng.step(self.comm)
        while st is None or st[1] == 0.0:
            it += 1                           # step `it` is enqueued
            eng.step(self.comm)               # one step ahead of the read; a no-op on the device if the rule has fired
            if it < n_min:
                if it == 2 and d > 16 and eng.runs == 1 and eng.graph is None:
                    eng.wait_record(2)        # first run of this engine: learn the proposal kernel's regime after two steps
            else:                             # the rule cannot fire earlier (mcmc.py:119-131)
                st = eng.wait_record(it)
                self._progress(n_global, st, it)
                if st[1] != 0.0:
                    break
        if eng.u is not u:                    # graph mode: the step worked on the engine's fixed-address buffers
            u.copy_(eng.u); logl.copy_(eng.logl)
        # x = prior_transform(u) is not maintained step by step (tph_accept with x = NULL writes half the bytes): one
        # evaluation for the final positions -- the same elementwise function of the same u, hence the same values
        x.copy_(self.prior(u))
        # two ticks per step + the proposal of the step that was launched ahead (same count as the step-by-step path)
        self.rng.tick = (tick_base + 2 * it + 1) & 0xFFFFFFFF
        return float(st[4]), float(st[3]), it, it * n_global


def parallel_mcmc(u, x, logl, blobs, assignments, beta, mode_stats, log_likelihood, prior_transform,
                  progress_bar=None, n_steps: int = 100, n_max: int = 1000, sample: str = "tpcn", periodic=None,
                  reflective=None, verbose: bool = True):
    """Drop-in for tempest.mcmc.parallel_mcmc (mcmc.py:414-508) on host arrays: u, x (n, d), logl (n,),
    callbacks in the reference's convention (prior_transform per row, log_likelihood(x) -> (logl, blobs)).
    Returns (u, x, logl, blobs, efficiency, acceptance, iterations, n_calls)."""
    import torch
    from .tools import _ctx
    u = np.asarray(u, dtype=np.float64)
    n, d = u.shape
    ctx = _ctx(d)
    dev = ctx.device

    def prior_dev(up):
        uh = np.ascontiguousarray(up.cpu().numpy().T)
        xh = np.array([prior_transform(row) for row in uh])
        return torch.from_numpy(np.ascontiguousarray(xh.T)).to(dev)

    def like_dev(xp, return_blobs=False):
        xh = np.ascontiguousarray(xp.cpu().numpy().T)
        ll, bl = log_likelihood(xh)
        ll = torch.from_numpy(np.ascontiguousarray(ll, dtype=np.float64)).to(dev)
        return (ll, bl) if return_blobs else ll

    to_soa = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).T)).to(dev)  # noqa: E731
    ut, xt = to_soa(u), to_soa(x)
    lt = torch.from_numpy(np.array(logl, dtype=np.float64)).to(dev)
    at = torch.from_numpy(np.asarray(assignments, dtype=np.int32)).to(dev)
    if mode_stats.means_dev.device != dev:
        raise ValueError("mode_stats lives on another device")
    run = DeviceMCMC(ctx, "rwm" if sample == "rwm" else "tpcn", beta, mode_stats, like_dev, prior_dev, n_steps, n_max,
                     periodic, reflective, progress_bar=progress_bar, verbose=verbose)
    eff, acc, it, calls = run.run(ut, xt, lt, at, blobs=blobs)
    back = lambda t: np.ascontiguousarray(t.cpu().numpy().T)  # noqa: E731
    return back(ut), back(xt), lt.cpu().numpy(), run.blobs, eff, acc, it, calls


def parallel_t_preconditioned_crank_nicolson(u, x, logl, blobs, assignments, beta, mode_stats, log_likelihood, prior_transform,
                                             progress_bar=None, n_steps: int = 100, n_max: int = 1000, periodic=None,
                                             reflective=None, verbose: bool = True):
    """tempest.mcmc.parallel_t_preconditioned_crank_nicolson (mcmc.py:511-589): parallel_mcmc with the tpCN kernel."""
    return parallel_mcmc(u, x, logl, blobs, assignments, beta, mode_stats, log_likelihood, prior_transform,
                         progress_bar=progress_bar, n_steps=n_steps, n_max=n_max, sample="tpcn", periodic=periodic,
                         reflective=reflective, verbose=verbose)


def parallel_random_walk_metropolis(u, x, logl, blobs, assignments, beta, mode_stats, log_likelihood, prior_transform,
                                    progress_bar=None, n_steps: int = 1000, n_max: int = 10000, periodic=None,
                                    reflective=None, verbose: bool = True):
    """tempest.mcmc.parallel_random_walk_metropolis (mcmc.py:592-676): parallel_mcmc with the RWM kernel (note the
    reference's larger defaults for n_steps / n_max)."""
    return parallel_mcmc(u, x, logl, blobs, assignments, beta, mode_stats, log_likelihood, prior_transform,
                         progress_bar=progress_bar, n_steps=n_steps, n_max=n_max, sample="rwm", periodic=periodic,
                         reflective=reflective, verbose=verbose)
