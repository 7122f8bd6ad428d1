"""v-objective diffusion on the gfx950 kernels: `VDiffusion` (training loss) and `VSampler`
(DDIM-style loop) and `VInpainter` (RePaint-style resampling loop), API-compatible with
/root/reference/audio_diffusion_pytorch/diffusion.py:15-30, :62-95, :133-190, :300-354.
`VMultistepSampler` (second-order two-step integrator, one net evaluation per step) is this package's own, and so is
`VThresholdSampler`, which puts the reference's `clip` (dynamic thresholding, diffusion.py:36-54) inside the sampling loop,
and `VStochasticSampler` (DDIM with eta > 0 on noise formed inside the update kernel).  Rectified flow (`RFDiffusion`,
`RFSampler`) builds on these classes from rf.py, Karras (EDM) diffusion (`KDiffusion`, `KSampler`) from edm.py.

Differences from the reference are structural, not numerical:
  * noising (x_noisy, v_target) is one fused kernel (2 reads, 2 writes) instead of ~6 elementwise ops;
  * the default MSE loss and its gradient are fused kernels; a user `loss_fn` still works (autograd);
  * the sampler keeps the sigma schedule on the host and the (alpha, beta) table on the device: the
    loop never reads device memory (the reference's tqdm f-string syncs every step, diffusion.py:188),
    so one step (U-Net forward + rotation kernel) is captured in a hipGraph and replayed.
"""
from contextlib import nullcontext
from math import pi
from typing import Any, Optional, Tuple

import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor
from tqdm import tqdm

from . import ops
from .capture import (CapturedStep, StepCache, ctx_tables_under, kwarg_structure, param_signature, static_kwargs,
                      tracked_parameters, warm_up)
from .capture import kw_spec as _kw_spec  # noqa: F401  (re-export: the name it had while it lived here)
from .graphed import GRAPHS_OF, TrainStepGraphs


def _on_device_of(t: Tensor):
    """Kernel launches go to the current HIP device's stream: make the tensor's device current for the call."""
    return torch.cuda.device(t.device) if t.is_cuda else nullcontext()


""" Distributions """


class Distribution:
    """Interface used by different distributions"""

    def __call__(self, num_samples: int, device: torch.device):
        raise NotImplementedError()


class UniformDistribution(Distribution):
    def __init__(self, vmin: float = 0.0, vmax: float = 1.0):
        super().__init__()
        self.vmin, self.vmax = vmin, vmax

    def __call__(self, num_samples: int, device: torch.device = torch.device("cpu")):
        return (self.vmax - self.vmin) * torch.rand(num_samples, device=device) + self.vmin


def extend_dim(x: Tensor, dim: int):
    return x.view(*x.shape + (1,) * (dim - x.ndim))


def alpha_beta(sigmas: Tensor) -> Tuple[Tensor, Tensor]:
    """The v-objective's (alpha, beta) = (cos, sin) of sigma * pi / 2: what every `get_alpha_beta` below returns."""
    angle = sigmas * pi / 2
    return torch.cos(angle), torch.sin(angle)


def _is_number(v) -> bool:
    """A number, not a bool: what the samplers' scalar arguments must be."""
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _ab_rows(alphas: Tensor, betas: Tensor, ahead: int = 1) -> Tensor:
    """The first-order rows (a_i, b_i, a_j, b_j) [N, 4] for j = i + ahead, from the N + 1 values of the schedule."""
    n = alphas.shape[0] - 1
    return torch.stack([alphas[:-1], betas[:-1], alphas[ahead:n + ahead], betas[ahead:n + ahead]], dim=1).contiguous()


def pad_dims(x: Tensor, ndim: int) -> Tensor:
    """Pads `ndim` dimensions of size 1 to the right of the tensor (diffusion.py:36-38)."""
    return x.view(*x.shape, *((1,) * ndim))


@torch.no_grad()
def clip(x: Tensor, dynamic_threshold: float = 0.0) -> Tensor:
    """diffusion.py:41-54 on the kernels of include/adp_clip.h, for float32 x [B, ...], forward only.
    dynamic_threshold == 0: clamp(x, -1, 1).  Otherwise s = max(quantile_q(|x|), 1) per batch item (torch.quantile's linear
    rule, selected exactly without a sort) and clamp(x, -s, s) / s."""
    if not 0.0 <= dynamic_threshold <= 1.0:
        raise ValueError(f"clip: dynamic_threshold must be in [0, 1]; got {dynamic_threshold!r}")
    if x.dim() < 1:
        raise ValueError("clip: x must be [B, ...]")
    with _on_device_of(x):
        x = x.contiguous()
        if dynamic_threshold == 0.0:
            scale = torch.ones(x.shape[0], dtype=torch.float32, device=x.device)  # (x / 1 is exact)
        else:
            scale = ops.clip_scale(x, dynamic_threshold, min_scale=1.0)
        return ops.clip_apply(x, scale)


""" Diffusion """


class Diffusion(nn.Module):
    """Interface used by different diffusion methods"""


class _VNoise(torch.autograd.Function):
    """x_noisy = a x + b n ; v_target = a n - b x  (diffusion.py:90-92) as one kernel."""

    @staticmethod
    def forward(ctx, x, noise, sigmas):
        x_noisy, v_target = ops.v_noise(x.contiguous(), noise.contiguous(), sigmas.contiguous())
        ctx.mark_non_differentiable(x_noisy, v_target)
        return x_noisy, v_target

    @staticmethod
    def backward(ctx, *g):  # data and noise are not differentiated on the training path
        return None, None, None


class _MSE(torch.autograd.Function):
    """F.mse_loss(v_pred, v_target) (diffusion.py:95) with a fused backward."""

    @staticmethod
    def forward(ctx, v_pred, v_target):
        v_pred, v_target = v_pred.contiguous(), v_target.contiguous()
        ctx.save_for_backward(v_pred, v_target)
        return ops.mse_fwd(v_pred, v_target)

    @staticmethod
    def backward(ctx, gloss):
        v_pred, v_target = ctx.saved_tensors
        return ops.mse_bwd(v_pred, v_target, gloss.contiguous()), None


def fused_mse_loss(v_pred: Tensor, v_target: Tensor) -> Tensor:
    return _MSE.apply(v_pred, v_target)


class VDiffusion(Diffusion):
    GRAPH_DISTRIBUTIONS: Tuple[type, ...] = (UniformDistribution,)  # exact classes whose draw the replayed step may capture

    def __init__(self, net: nn.Module, sigma_distribution: Distribution = UniformDistribution(),
                 loss_fn: Any = F.mse_loss, use_graph: bool = True):
        """`use_graph` (not in the reference): replay the training step from hipGraphs where that is safe (graphed.py) --
        the README loop `loss = model(x); loss.backward()` then costs two graph launches instead of ~700 kernel launches
        issued from Python; False (or ADP_TRAIN_GRAPH=0) = launch every kernel eagerly."""
        super().__init__()
        self.net = net
        self.sigma_distribution = sigma_distribution
        self.loss_fn = loss_fn
        self.use_graph = use_graph

    def get_alpha_beta(self, sigmas: Tensor) -> Tuple[Tensor, Tensor]:
        return alpha_beta(sigmas)

    def forward(self, x: Tensor, noise: Optional[Tensor] = None, **kwargs) -> Tensor:
        """`noise` (optional, default torch.randn_like(x) as at diffusion.py:88) lets a harness inject the draw."""
        if self._graph_path_ok(x, noise):
            with _on_device_of(x):
                loss = self.train_graphs().run(x, noise, kwargs)
            if loss is not None:
                return loss
        return self._forward_eager(x, noise, **kwargs)

    def train_graphs(self):
        """The captured training steps of this module (kept OFF the module: hipGraphs can be neither deep-copied nor pickled,
        and an EMA copy.deepcopy(model) / torch.save(model) must keep working after a step has been captured)."""
        graphs = GRAPHS_OF.get(self)
        if graphs is None:
            graphs = GRAPHS_OF[self] = TrainStepGraphs(self)
        return graphs

    def _graph_path_ok(self, x: Tensor, noise: Optional[Tensor]) -> bool:
        """Whether this call may be served by the replayed step (graphed.py lists the conditions)."""
        if not (self.use_graph and x.is_cuda and x.dtype == torch.float32 and torch.is_grad_enabled()) or x.requires_grad:
            return False
        if noise is not None and (not noise.is_cuda or noise.requires_grad or noise.shape != x.shape):
            return False
        if type(self.sigma_distribution) not in self.GRAPH_DISTRIBUTIONS or os.environ.get("ADP_TRAIN_GRAPH", "1") == "0":
            return False
        if torch.cuda.is_current_stream_capturing():  # (a caller's own whole-step capture: bench.py, parallel.capture_step)
            return False
        hooked = self.__dict__.get("_hook_sites")
        if hooked is None:  # the U-Nets whose backward may carry a data-parallel hook (collectives: not captured implicitly)
            hooked = self.__dict__["_hook_sites"] = [m for m in self.net.modules() if hasattr(m, "_param_offsets")]
        return all(getattr(m, "_grad_ready_hook", None) is None for m in hooked)

    def _forward_eager(self, x: Tensor, noise: Optional[Tensor] = None, **kwargs) -> Tensor:
        batch_size, device = x.shape[0], x.device
        with _on_device_of(x):
            sigmas = self.sigma_distribution(num_samples=batch_size, device=device)
            if noise is None:
                noise = torch.randn_like(x)
            x_noisy, v_target = _VNoise.apply(x, noise, sigmas.to(torch.float32))
            v_pred = self.net(x_noisy, sigmas, **kwargs)
            if self.loss_fn is F.mse_loss:
                return fused_mse_loss(v_pred, v_target)
            return self.loss_fn(v_pred, v_target)


""" Schedules """


class Schedule(nn.Module):
    """Interface used by different sampling schedules"""

    def forward(self, num_steps: int, device: torch.device) -> Tensor:
        raise NotImplementedError()


class LinearSchedule(Schedule):
    def __init__(self, start: float = 1.0, end: float = 0.0):
        super().__init__()
        self.start, self.end = start, end

    def forward(self, num_steps: int, device: Any) -> Tensor:
        return torch.linspace(self.start, self.end, num_steps, device=device)


""" Samplers """


class Sampler(nn.Module):
    pass


class _CapturedSteps:
    """The cache of captured steps that `VSampler`, `VInpainter` and `ar.ARVSampler` share (mixed into an nn.Module with a
    `net`): one step = net forward + update kernel in place on a static x, captured once per call STRUCTURE and replayed.
    An entry is a `capture.CapturedStep` extended by the class that builds it; the rules are capture.py's."""

    GRAPH_CACHE_ENTRIES = 4  # captured steps kept (LRU); each owns its private activation pool

    def _init_graph_cache(self):
        self._graph_cache = StepCache()
        self.graph_captures = 0  # (visible to tests: steps captured / sampling runs served by replays)
        self.graph_replays = 0

    def __getstate__(self):
        """copy.deepcopy (an EMA copy) and pickling (torch.save) leave the captured steps behind: hipGraphs can be neither
        copied nor pickled, and a copy's graphs would read the original's weights.  The copy captures its own."""
        state = super().__getstate__()
        state.update(_graph_cache=StepCache(), graph_captures=0, graph_replays=0)
        return state

    def _captured_step(self, x: Tensor, kwargs, build, extra_key=()):
        """The cache entry for this call structure, the caller's kwarg tensors copied into its static ones -- or None (eager
        fallback) for kwargs that cannot be made static or hold a CPU tensor.  The key is (x shape, device, kwarg names, tensor
        shapes / dtypes, python scalar values, `extra_key`).  A missing entry, also one dropped because the net's parameters
        moved or were replaced, is captured: `build(skw)` takes the static kwargs and returns (static x, step, the owner's
        static tensors by name); `step(warm)` runs once on a side stream outside capture (warm=True: it must leave the static
        x as it is), then once under capture (warm=False: in place)."""
        found = kwarg_structure(kwargs, lambda t: t.is_cuda)
        if found is None:
            return None
        names, live, specs = found
        key = (tuple(x.shape), x.device, specs) + tuple(extra_key)
        psig = param_signature(tracked_parameters(self.net))
        entry = self._graph_cache.fetch(key, psig)
        if entry is None:
            statics, skw = static_kwargs(kwargs, names, live)
            sx, step, own = build(skw)
            warm_up(lambda: step(True))
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step(False)
            entry = CapturedStep(graph, sx, statics, psig, ctx_tables_under(self.net), **own)
            self._graph_cache.store(key, entry, self.GRAPH_CACHE_ENTRIES)
            self.graph_captures += 1
        for st, t in zip(entry.statics, live):
            st.copy_(t)
        return entry


class VSampler(_CapturedSteps, Sampler):

    diffusion_types = [VDiffusion]

    def __init__(self, net: nn.Module, schedule: Schedule = LinearSchedule(), use_graph: bool = True):
        super().__init__()
        self.net = net
        self.schedule = schedule
        self.use_graph = use_graph
        self._init_graph_cache()

    def get_alpha_beta(self, sigmas: Tensor) -> Tuple[Tensor, Tensor]:
        return alpha_beta(sigmas)

    def _tables(self, num_steps: int, b: int, device):
        """sigma table [N+1, B] and per-step (a_i, b_i, a_{i+1}, b_{i+1}) table [N, 4], both on the device.
        The schedule is a pure function of num_steps, so nothing here (or in the loop) syncs with the host."""
        sigmas = self.schedule(num_steps + 1, device=device).to(torch.float32)
        alphas, betas = self.get_alpha_beta(sigmas)
        return sigmas[:, None].expand(num_steps + 1, b).contiguous(), _ab_rows(alphas, betas)

    def _step_buffers(self, x: Tensor) -> Tuple[Tensor, ...]:
        """Tensors of x's shape that the step update carries from one step to the next (a subclass's history); owned by the
        sampling run (eager) or by the graph cache entry (replay).  The first-order rotation has none."""
        return ()

    def _step(self, x: Tensor, v: Tensor, row: Tensor, bufs: Tuple[Tensor, ...], out: Optional[Tensor]) -> Tensor:
        """x_{i+1} from (x_i, v_i) and row i of `_tables`' per-step table; `out` may be x (each element is read, then
        written).  The one piece a subclass replaces: everything around it in forward / _forward_graph is shared."""
        return ops.v_step(x, v, row, out=out)

    def _step_key(self) -> Tuple:
        """What of this sampler's configuration a captured step depends on beyond the call structure (part of the cache key)."""
        return ()

    HOIST_MAX_BYTES = 512 << 20  # cap of the hoisted conditioning table (README net: 360 KB per step and batch element)

    def _conditioning_table(self, sig: Tensor, num_steps: int, b: int, kwargs) -> Optional[Tensor]:
        """[num_steps, B, bank_total] or None.  The time values of ALL steps are known before the loop starts, and what the
        U-Net derives from them (time MLP, then the conditioning bank: one row of 90 K scale / shift values per call in the
        README configuration, 184 MB of weights streamed per call) does not depend on x: one batched pass in front of the
        loop replaces eight launches per step.  Only for a bare UNetV0 (the plugin wrappers re-shape their arguments) without
        `features`; ADP_SAMPLER_HOIST=0 keeps the per-step conditioning (A/B)."""
        table_fn = getattr(self.net, "conditioning_table", None)
        if table_fn is None or kwargs.get("features") is not None or os.environ.get("ADP_SAMPLER_HOIST", "1") == "0":
            return None
        total = getattr(self.net, "bank_total", 0)
        if total <= 0 or 4 * num_steps * b * total > self.HOIST_MAX_BYTES:
            return None
        table = table_fn(sig[:num_steps])
        return None if table is None else table.view(num_steps, b, total)

    @torch.no_grad()
    def forward(self, x_noisy: Tensor, num_steps: int, show_progress: bool = False, **kwargs) -> Tensor:
        with _on_device_of(x_noisy):
            b = x_noisy.shape[0]
            sig, ab = self._tables(num_steps, b, x_noisy.device)
            x = x_noisy.contiguous().clone()
            prepare = getattr(self.net, "prepare_sampling_kwargs", None)
            if prepare is not None:  # e.g. text -> embedding tensor, once per sampling run
                kwargs = prepare(x, kwargs)
            cond = self._conditioning_table(sig, num_steps, b, kwargs)
            if self.use_graph and x.is_cuda and not show_progress:
                out = self._forward_graph(x, sig, ab, num_steps, kwargs, cond)
                if out is not None:
                    return out
            bar = tqdm(range(num_steps), disable=not show_progress)
            host_sigmas = torch.linspace(self.schedule.start, self.schedule.end, num_steps + 1).tolist() \
                if (show_progress and isinstance(self.schedule, LinearSchedule)) else None
            bufs = self._step_buffers(x)
            for i in bar:
                v = self.net(x, sig[i], **kwargs) if cond is None else self.net(x, sig[i], conditioning=cond[i], **kwargs)
                x = self._step(x, v.contiguous(), ab[i], bufs, None)
                if host_sigmas is not None:
                    bar.set_description(f"Sampling (noise={host_sigmas[i + 1]:.2f})")
            return x

    def _forward_graph(self, x: Tensor, sig: Tensor, ab: Tensor, num_steps: int, kwargs,
                       cond: Optional[Tensor] = None) -> Optional[Tensor]:
        """One step = U-Net forward + rotation kernel, captured once per call STRUCTURE and replayed.  The cache key
        is (x shape, kwarg names, tensor shapes/dtypes, python scalar values); the entry owns static copies of every
        tensor kwarg (also those nested in `channels`) and the caller's tensors are copied into them before the
        replays, so fresh conditioning tensors per call reuse the graph and can never be read after they are freed.
        An entry is recaptured when a parameter of the net moved or was replaced (the graph holds their addresses), and it
        keeps the context-bank tables it was captured with alive (capture.py).
        Per step only two tiny device-to-device copies (sigma row, alpha/beta row) precede the replay.  Returns None
        (eager fallback) for kwargs that cannot be made static."""
        def build(skw):
            sx, ssig, sab = torch.empty_like(x), torch.empty_like(sig[0]), torch.empty_like(ab[0])
            scond = torch.empty_like(cond[0]) if cond is not None else None  # this step's rows of the hoisted conditioning
            bufs = self._step_buffers(sx)
            sx.copy_(x)
            ssig.copy_(sig[0])
            sab.copy_(ab[0])
            if scond is not None:
                scond.copy_(cond[0])
                skw["conditioning"] = scond

            def step(warm: bool):
                v = self.net(sx, ssig, **skw)
                # captured in place: each element is read then written
                self._step(sx, v.contiguous(), sab, bufs, torch.empty_like(sx) if warm else sx)

            return sx, step, dict(ssig=ssig, sab=sab, scond=scond, bufs=bufs)

        entry = self._captured_step(x, kwargs, build, (cond is not None,) + tuple(self._step_key()))
        if entry is None:
            return None
        self.graph_replays += 1
        graph, sx, ssig, sab, scond = entry.graph, entry.sx, entry.ssig, entry.sab, entry.scond
        sx.copy_(x)
        for i in range(num_steps):
            if scond is not None:
                scond.copy_(cond[i])  # (the captured step no longer reads the sigma row)
            else:
                ssig.copy_(sig[i])
            sab.copy_(ab[i])
            graph.replay()
        return sx.clone()


class VMultistepSampler(VSampler):
    """Second-order two-step (Adams-Bashforth style) exponential integrator for the v-objective: ONE net evaluation per step
    like `VSampler`, error falling with the square of the step size.  Not in the reference.

    The probability-flow ODE in the angle phi = sigma * pi / 2 is dx/dphi = -sin(phi) x0 + cos(phi) eps.  `VSampler` integrates
    it with (x0, eps) held constant over a step; this sampler extrapolates both linearly in phi through the previous step's
    values and integrates that exactly.  With d = phi_{i+1} - phi_i, g = phi_i - phi_{i-1}:

        x_{i+1} = a_{i+1} x0_i + b_{i+1} eps_i + ca_i (x0_i - x0_{i-1}) + cb_i (eps_i - eps_{i-1})
        ca_i = (d a_{i+1} - b_{i+1} + b_i) / g      cb_i = (d b_{i+1} + a_{i+1} - a_i) / g      ca_0 = cb_0 = 0

    so the first step is the `VSampler` step and one captured graph (U-Net forward + adp_v_step2 in place on x and on the two
    history buffers of the cache entry) serves every step: steps differ only in their coefficient row, and a row with
    ca = cb = 0 does not read the history, so nothing of an earlier run can reach the next one.
    `order=1` is `VSampler`'s arithmetic (A/B in one class)."""

    def __init__(self, net: nn.Module, schedule: Schedule = LinearSchedule(), order: int = 2, use_graph: bool = True):
        if not _is_number(order) or order not in (1, 2):
            raise ValueError(f"VMultistepSampler: order must be 1 or 2; got {order!r}")
        super().__init__(net=net, schedule=schedule, use_graph=use_graph)
        self.order = order

    def _tables(self, num_steps: int, b: int, device):
        """sigma table [N+1, B] and per-step rows (a_i, b_i, a_{i+1}, b_{i+1}, ca_i, cb_i) [N, 6] on the device.  ca, cb are
        differences of nearly equal numbers (about d**2 / 2): the table is formed in float64 on the host (one small
        device-to-host copy per sampling run, none in the loop) and rounded to float32 once."""
        if self.order == 1:
            return super()._tables(num_steps, b, device)
        sigmas = self.schedule(num_steps + 1, device=device).to(torch.float32)  # (what the net is given)
        phi = sigmas.to(device="cpu", dtype=torch.float64) * (pi / 2)
        a, bt = torch.cos(phi), torch.sin(phi)
        d = phi[1:] - phi[:-1]
        ca, cb = torch.zeros(num_steps, dtype=torch.float64), torch.zeros(num_steps, dtype=torch.float64)
        if num_steps > 1:
            g = d[:-1]
            if bool((g == 0).any()):
                raise ValueError("VMultistepSampler: the schedule repeats a sigma (zero step before step "
                                 f"{int((g == 0).nonzero()[0]) + 1}); neighbouring sigmas must differ")
            ca[1:] = (d[1:] * a[2:] - bt[2:] + bt[1:-1]) / g
            cb[1:] = (d[1:] * bt[2:] + a[2:] - a[1:-1]) / g
        coef = torch.stack([a[:-1], bt[:-1], a[1:], bt[1:], ca, cb], dim=1).to(torch.float32).contiguous()
        return sigmas[:, None].expand(num_steps + 1, b).contiguous(), coef.to(device)

    def _step_buffers(self, x: Tensor) -> Tuple[Tensor, ...]:
        # (x0_{i-1}, eps_{i-1}); left uninitialised: the first step of every run writes them without reading them
        return () if self.order == 1 else (torch.empty_like(x), torch.empty_like(x))

    def _step(self, x: Tensor, v: Tensor, row: Tensor, bufs: Tuple[Tensor, ...], out: Optional[Tensor]) -> Tensor:
        if self.order == 1:
            return super()._step(x, v, row, bufs, out)
        hist_x0, hist_eps = bufs
        return ops.v_step2(x, v, hist_x0, hist_eps, row, out=out, hist_x0_out=hist_x0, hist_eps_out=hist_eps)[0]


class _Thresholded:
    """The dynamic-threshold glue of `VThresholdSampler`, `VStochasticSampler`, `rf.RFSampler` and `edm.KSampler` (mixed into a `VSampler`
    that sets `self.dynamic_threshold`): None = no clipping, 0.0 = the static clamp to [-1, 1], q in (0, 1] = the per-item
    quantile scale of include/adp_clip.h, selected in front of the update kernel from the step's own (x, v, coefficient row)."""

    @staticmethod
    def _threshold(owner: str, dynamic_threshold, none_ok: bool) -> Optional[float]:
        """The checked constructor argument as a float (or None where the class allows it)."""
        if dynamic_threshold is None and none_ok:
            return None
        if not (_is_number(dynamic_threshold) and 0.0 <= dynamic_threshold <= 1.0):
            raise ValueError(f"{owner}: dynamic_threshold must be {'None or ' if none_ok else ''}a number in [0, 1]; "
                             f"got {dynamic_threshold!r}")
        return float(dynamic_threshold)

    def _dynamic(self) -> bool:
        return self.dynamic_threshold is not None and self.dynamic_threshold > 0.0

    def _threshold_buffers(self, x: Tensor) -> Tuple[Tensor, ...]:
        """(scale [B], select workspace) when the threshold is dynamic: they lead the class's own step buffers.  Left
        uninitialised: every step zeroes the workspace it uses and writes the scale before reading it."""
        if not self._dynamic():
            return ()
        return (torch.empty(x.shape[0], dtype=torch.float32, device=x.device), ops.clip_ws(x))

    def _threshold_scale(self, x: Tensor, v: Tensor, coef: Tensor, bufs: Tuple[Tensor, ...]):
        """(this step's scale [B] or None, the step buffers behind `_threshold_buffers`'); coef: the row holding (a0, b0)."""
        if not self._dynamic():
            return None, bufs
        scale, ws = bufs[:2]
        ops.clip_scale(x, self.dynamic_threshold, v=v, coef=coef, min_scale=1.0, ws=ws, out=scale)
        return scale, bufs[2:]


class VThresholdSampler(_Thresholded, VMultistepSampler):
    """`VSampler` (order=1) or `VMultistepSampler` (order=2) with the predicted clean signal thresholded at every step: what
    keeps a bounded signal (audio in [-1, 1]) bounded under classifier-free guidance, where x0 = a x - b v leaves the range at
    the noisy end of the schedule.  Not in the reference, whose `clip` (diffusion.py:41-54) has no caller.

        x0  = a_i x - b_i v            eps = b_i x + a_i v
        x0c = clip(x0, dynamic_threshold)
        order 1:  x_{i+1} = a_{i+1} x0c + b_{i+1} eps
        order 2:  x_{i+1} = a_{i+1} x0c + b_{i+1} eps + ca_i (x0c - x0c_{i-1}) + cb_i (eps - eps_{i-1})

    eps is kept from the RAW prediction, the usual form of thresholded DDIM: re-deriving it from the clipped x0 would divide by
    b_i, which goes to 0 at the clean end of the schedule.  The second-order history holds the clipped x0.

    `dynamic_threshold=q` > 0: per batch item s = max(quantile_q(|x0|), 1), x0c = clamp(x0, -s, s) / s -- an exact order
    statistic by a three-pass radix select over the bits of |x0| (include/adp_clip.h), five small launches in front of the
    update kernel, no sort and no host read, so the whole step still replays from one hipGraph.  `dynamic_threshold=0.0` is
    the static clamp to [-1, 1]: the update kernel alone.  The scale row, the select's workspace and the history are step
    buffers: a captured step owns its own, and (threshold, order) are part of its cache key."""

    def __init__(self, net: nn.Module, schedule: Schedule = LinearSchedule(), dynamic_threshold: float = 0.995,
                 order: int = 1, use_graph: bool = True):
        if not _is_number(order) or order not in (1, 2):
            raise ValueError(f"VThresholdSampler: order must be 1 or 2; got {order!r}")
        threshold = self._threshold("VThresholdSampler", dynamic_threshold, none_ok=False)
        super().__init__(net=net, schedule=schedule, order=order, use_graph=use_graph)
        self.dynamic_threshold = threshold

    def _step_key(self) -> Tuple:
        return (float(self.dynamic_threshold), self.order)

    def _step_buffers(self, x: Tensor) -> Tuple[Tensor, ...]:
        """The threshold's buffers, then `VMultistepSampler`'s history."""
        return self._threshold_buffers(x) + tuple(super()._step_buffers(x))

    def _step(self, x: Tensor, v: Tensor, row: Tensor, bufs: Tuple[Tensor, ...], out: Optional[Tensor]) -> Tensor:
        scale, hist = self._threshold_scale(x, v, row, bufs)
        if self.order == 1:
            return ops.clip_step(x, v, row, scale, out=out)
        hist_x0, hist_eps = hist
        return ops.clip_step(x, v, row, scale, hist_x0, hist_eps, out=out, hist_x0_out=hist_x0, hist_eps_out=hist_eps)[0]


class VStochasticSampler(_Thresholded, VSampler):
    """DDIM with eta > 0 on the v-objective: the usual `sample(model, x, steps, eta)` loop of v-diffusion, optionally with
    the predicted clean signal thresholded as in `VThresholdSampler` (the usual pair under classifier-free guidance).  Not
    in the reference.

        x0  = a_i x - b_i v            eps = b_i x + a_i v            x0c = x0, or clip(x0, dynamic_threshold)
        cz_i = eta (b_{i+1} / b_i) sqrt(b_i^2 - b_{i+1}^2) / a_{i+1}      (0 where b_i = 0 or b_{i+1} = 0)
        ce_i = sqrt(b_{i+1}^2 - cz_i^2)
        x_{i+1} = a_{i+1} x0c + ce_i eps + cz_i z_i ,   z_i ~ N(0, 1)

    eta = 0 is `VSampler` (ce = b_{i+1}, cz = 0); from pure noise with eta = 1 the first step is the DDPM step (ce = 0); the
    last step (sigma = 0) adds no noise.  For eta in [0, 1] ce is real because b_i <= 1.  eps is kept from the raw v.

    One step is one net evaluation and ONE update kernel (adp_v_step_eta, include/adp_sde.h) that forms z in registers
    from the library's counter-based generator (include/adp_rng.h): no noise tensor is written or read, torch's generator
    is not called, and the step replays from one hipGraph like `VSampler`'s.  `forward(..., seed=...)` fixes every draw of
    the run on any backend: step i uses draw 1 + i of the seed, draw 0 is the start noise where the sampler draws it.  Each
    step reads one row of a device table built once per run: (a_i, b_i, a_{i+1}, ce_i, cz_i), formed in float64 on the host
    and rounded to float32 once, next to (seed_lo, seed_hi, draw, 0).  A captured step depends on whether eta > 0 and on the
    threshold, not on the value of eta or the seed.  With eta == 0 the step is the parent's kernel (`VSampler`'s, or
    `VThresholdSampler(order=1)`'s), bit for bit.

    `dynamic_threshold`: None (no thresholding), 0.0 (static clamp to [-1, 1]) or q in (0, 1] (`VThresholdSampler`'s
    quantile scale, five small launches in front of the update kernel).

    Variation: `forward(x_noisy, num_steps, start=clip, strength=s)` starts from `a_s start + b_s noise` at the run's first
    sigma and runs the sigmas `s * schedule(num_steps + 1)`; noise is x_noisy, or draw 0 of the seed where x_noisy is None.

    Out of scope: a second-order stochastic update (there is no `order`), `VInpainter` and `ar.ARVSampler`."""

    def __init__(self, net: nn.Module, schedule: Schedule = LinearSchedule(), eta: float = 1.0,
                 dynamic_threshold: Optional[float] = None, use_graph: bool = True):
        if not _is_number(eta) or not 0.0 <= eta <= 1.0:
            raise ValueError(f"VStochasticSampler: eta must be a number in [0, 1]; got {eta!r}")
        threshold = self._threshold("VStochasticSampler", dynamic_threshold, none_ok=True)
        super().__init__(net=net, schedule=schedule, use_graph=use_graph)
        self.eta = float(eta)
        self.dynamic_threshold = threshold
        self._run = (0, 1.0)  # (seed, strength) of the sampling run in progress: what `forward` hands to `_tables`

    def _sigmas(self, num_steps: int, device) -> Tensor:
        """The run's sigmas [N+1], float32 on the device: what the net is given."""
        sigmas = self.schedule(num_steps + 1, device=device).to(torch.float32)
        strength = self._run[1]
        return sigmas if strength == 1.0 else sigmas * strength

    def _tables(self, num_steps: int, b: int, device):
        """sigma table [N+1, B] and the per-step table.  eta == 0: `VSampler`'s rows (a_i, b_i, a_{i+1}, b_{i+1}) [N, 4]
        float32.  eta > 0: [N, 9] int32 words, the bits of (a_i, b_i, a_{i+1}, ce_i, cz_i) float32 next to
        (seed_lo, seed_hi, 1 + i, 0).  The coefficients are formed in float64 on the host (one small device-to-host copy
        per sampling run, none in the loop) and rounded to float32 once."""
        sigmas = self._sigmas(num_steps, device)
        sig = sigmas[:, None].expand(num_steps + 1, b).contiguous()
        if self.eta == 0.0:
            return sig, _ab_rows(*self.get_alpha_beta(sigmas))
        s64 = sigmas.to(device="cpu", dtype=torch.float64)
        phi = s64 * (pi / 2)
        a, bt = torch.cos(phi), torch.sin(phi)
        b0, b1, a1 = bt[:-1], bt[1:], a[1:]
        if bool((b1 > b0).any()):
            raise ValueError("VStochasticSampler: the schedule increases at step "
                             f"{int((b1 > b0).nonzero()[0])} (b_{{i+1}} > b_i); the noise level must not grow")
        zero = (b0 == 0) | (b1 == 0)
        ratio = torch.where(zero, torch.zeros_like(b0), b1 / torch.where(zero, torch.ones_like(b0), b0))
        num = self.eta * ratio * torch.sqrt((b0 * b0 - b1 * b1).clamp_min(0.0))
        bad = (num > 0) & (s64[1:] == 1.0)
        if bool(bad.any()):
            raise ValueError(f"VStochasticSampler: step {int(bad.nonzero()[0])} adds noise towards sigma = 1, where "
                             "a_{i+1} = 0 and cz is not defined")
        cz = torch.where(num > 0, num / a1, torch.zeros_like(num))
        ce = torch.sqrt((b1 * b1 - cz * cz).clamp_min(0.0))
        coef = torch.stack([a[:-1], b0, a1, ce, cz], dim=1).to(torch.float32).contiguous()
        rng = ops.rng_rows(self._run[0], range(1, 1 + num_steps))
        table = torch.cat([coef.view(torch.int32), rng], dim=1).contiguous()
        return sig, table.to(device)

    def _step_key(self) -> Tuple:
        return (self.eta > 0.0, self.dynamic_threshold)

    def _step_buffers(self, x: Tensor) -> Tuple[Tensor, ...]:
        return self._threshold_buffers(x)

    def _step(self, x: Tensor, v: Tensor, row: Tensor, bufs: Tuple[Tensor, ...], out: Optional[Tensor]) -> Tensor:
        noisy = row.dtype == torch.int32  # (the row of an eta > 0 table)
        coef, rng = (row[:5].view(torch.float32), row[5:]) if noisy else (row, None)
        scale, _ = self._threshold_scale(x, v, coef, bufs)
        if noisy:
            return ops.v_step_eta(x, v, coef, rng, scale=scale, clip=self.dynamic_threshold is not None, out=out)
        if self.dynamic_threshold is None:
            return ops.v_step(x, v, row, out=out)
        return ops.clip_step(x, v, row, scale, out=out)

    @torch.no_grad()
    def forward(self, x_noisy: Optional[Tensor], num_steps: int, show_progress: bool = False, *,
                seed: Optional[int] = None, start: Optional[Tensor] = None, strength: float = 1.0, **kwargs) -> Tensor:
        """`seed`: the integer all draws of this run follow; None = one drawn from torch's default CPU generator (so
        torch.manual_seed governs it), without touching the device.  `start`, `strength`: variation (class docstring)."""
        if not _is_number(strength) or not 0.0 < strength <= 1.0:
            raise ValueError(f"VStochasticSampler: strength must be a number in (0, 1]; got {strength!r}")
        if start is None:
            if strength != 1.0:
                raise ValueError("VStochasticSampler: strength != 1.0 needs start= (the clip to vary)")
            if x_noisy is None:
                raise ValueError("VStochasticSampler: x_noisy=None needs start= (pure noise is given by the caller)")
        elif x_noisy is not None and x_noisy.shape != start.shape:
            raise ValueError(f"VStochasticSampler: start must have x_noisy's shape {tuple(x_noisy.shape)}; "
                             f"got {tuple(start.shape)}")
        if seed is None:
            seed = int(torch.randint(0, 1 << 62, (1,)).item())  # (a CPU tensor: no device sync)
        self._run = (int(seed), float(strength))
        try:
            if start is not None:
                with _on_device_of(start):
                    src = start.to(torch.float32).contiguous()
                    if x_noisy is not None:
                        noise = x_noisy.to(torch.float32).contiguous()
                    else:
                        noise = ops.randn(src, ops.rng_rows(seed, [0])[0].to(src.device))
                    first = self._sigmas(num_steps, src.device)[0].expand(src.shape[0]).contiguous()
                    x_noisy = ops.v_noise(src, noise, first)[0]
            return super().forward(x_noisy, num_steps, show_progress, **kwargs)
        finally:
            self._run = (0, 1.0)


""" Inpainters """


class Inpainter(nn.Module):
    pass


class VInpainter(_CapturedSteps, Inpainter):
    """diffusion.py:306-354.  Per resample the reference runs ~10 elementwise ops; here the rotation to the next
    noise level, the re-noising of the source and the masked blend are ONE kernel (adp_v_inpaint_step).  By default the
    noise draws stay on torch's generator (`torch.randn_like(source)`, same call order as the reference) so seeding
    behaves identically; the (alpha, beta) table lives on the device and the loop never syncs with the host.

    `noise="philox"` (not in the reference) takes the noise from the library's counter-based generator instead
    (include/adp_rng.h): `forward(..., seed=...)` fixes every draw of the run -- the start noise is draw 0, the resample
    (i, r) uses draw 1 + i * num_resamples + r -- on any backend, and the update kernel (adp_v_inpaint_step_rng) forms the
    noise in registers: no noise tensor is written or read.  Each resample reads one row of a device table built once per
    run, (a_i, b_i, a_j, b_j) next to (seed_lo, seed_hi, draw, 0).
    `use_graph=True` (philox only) captures one resample -- U-Net forward + update in place on a static x -- and replays it
    for every (step, resample) pair behind a device-to-device copy of the pair's row, with `VSampler`'s cache rules (key,
    recapture when parameters move, LRU, copies start empty).  It falls back to the eager loop for kwargs that cannot be
    made static, for CPU tensors and for show_progress=True."""

    diffusion_types = [VDiffusion]
    NOISE_SOURCES = ("torch", "philox")

    def __init__(self, net: nn.Module, schedule: Schedule = LinearSchedule(), noise: str = "torch",
                 use_graph: bool = False):
        if noise not in self.NOISE_SOURCES:
            raise ValueError(f"VInpainter: noise must be one of {self.NOISE_SOURCES}; got {noise!r}")
        if use_graph and noise != "philox":
            raise ValueError("VInpainter: use_graph=True needs noise='philox' (torch's generator cannot be replayed)")
        super().__init__()
        self.net = net
        self.schedule = schedule
        self.noise = noise
        self.use_graph = use_graph
        self._init_graph_cache()

    def get_alpha_beta(self, sigmas: Tensor) -> Tuple[Tensor, Tensor]:
        return alpha_beta(sigmas)

    @torch.no_grad()
    def forward(self, source: Tensor, mask: Tensor, num_steps: int, num_resamples: int, show_progress: bool = False,
                x_noisy: Optional[Tensor] = None, seed: Optional[int] = None, **kwargs) -> Tensor:
        """`seed` (noise="philox" only): the integer all draws of this run follow; None = one drawn from torch's default CPU
        generator (so torch.manual_seed governs it), without touching the device."""
        if self.noise != "philox":
            if seed is not None:
                raise ValueError("VInpainter: seed= needs noise='philox'; with noise='torch' seed torch's generator instead")
            with _on_device_of(source):
                return self._run(source, mask, num_steps, num_resamples, show_progress, x_noisy, kwargs)
        if seed is None:
            seed = int(torch.randint(0, 1 << 62, (1,)).item())  # (a CPU tensor: no device sync)
        with _on_device_of(source):
            return self._run_philox(source, mask, num_steps, num_resamples, show_progress, x_noisy, int(seed), kwargs)

    def _tables(self, num_steps: int, b: int, device):
        """sigma table [N+1, B] and the rows (a_i, b_i, a_j, b_j) for j = i (re-noise at the same level) and j = i + 1
        (move on), [N, 4] each, on the device."""
        sigmas = self.schedule(num_steps + 1, device=device).to(torch.float32)
        alphas, betas = self.get_alpha_beta(sigmas)
        sig = sigmas[:, None].expand(num_steps + 1, b).contiguous()
        return sig, _ab_rows(alphas, betas, ahead=0), _ab_rows(alphas, betas)

    def _run(self, source, mask, num_steps, num_resamples, show_progress, x_noisy, kwargs) -> Tensor:
        x = (x_noisy if x_noisy is not None else torch.randn_like(source)).contiguous()
        prepare = getattr(self.net, "prepare_sampling_kwargs", None)
        if prepare is not None:
            kwargs = prepare(x, kwargs)
        sig, ab_stay, ab_next = self._tables(num_steps, x.shape[0], x.device)
        src = source.to(torch.float32).contiguous()
        mask_u8 = mask.expand_as(src).to(torch.uint8).contiguous()
        host_sigmas = self.schedule(num_steps + 1, device="cpu").tolist() if show_progress else None
        bar = tqdm(range(num_steps), disable=not show_progress)
        for i in bar:
            for r in range(num_resamples):
                v = self.net(x, sig[i], **kwargs)
                last = r == num_resamples - 1
                x = ops.v_inpaint_step(x, v.contiguous(), src, torch.randn_like(src), mask_u8,
                                       (ab_next if last else ab_stay)[i])
            if host_sigmas is not None:
                bar.set_description(f"Inpainting (noise={host_sigmas[i + 1]:.2f})")
        return x

    def _run_philox(self, source, mask, num_steps, num_resamples, show_progress, x_noisy, seed, kwargs) -> Tensor:
        src = source.to(torch.float32).contiguous()
        mask_u8 = mask.expand_as(src).to(torch.uint8).contiguous()
        dev = src.device
        if x_noisy is not None:
            x = x_noisy.to(torch.float32).contiguous()
        else:
            x = ops.randn(src, ops.rng_rows(seed, [0])[0].to(dev))
        prepare = getattr(self.net, "prepare_sampling_kwargs", None)
        if prepare is not None:
            kwargs = prepare(x, kwargs)
        sig, ab_stay, ab_next = self._tables(num_steps, x.shape[0], dev)
        # the run's table [S, 8] (int32 words), one row per (step, resample) pair in loop order, S = num_steps * num_resamples:
        # the bits of (a_i, b_i, a_j, b_j) f32 next to (seed_lo, seed_hi, draw, 0).  Every resample of a step but the last
        # stays at its level.  Built once per run; the generator half comes from the host in one copy, nothing is read back.
        total = num_steps * num_resamples
        if total == 0:
            return x
        ab = ab_stay[:, None, :].repeat(1, num_resamples, 1)
        ab[:, num_resamples - 1] = ab_next
        rng = ops.rng_rows(seed, range(1, 1 + total)).to(dev)
        table = torch.cat([ab.reshape(total, 4).view(torch.int32), rng], dim=1).contiguous()
        if self.use_graph and x.is_cuda and not show_progress:
            out = self._forward_graph(x, src, mask_u8, sig, table, num_steps, num_resamples, kwargs)
            if out is not None:
                return out
        host_sigmas = self.schedule(num_steps + 1, device="cpu").tolist() if show_progress else None
        bar = tqdm(range(num_steps), disable=not show_progress)
        for i in bar:
            for r in range(num_resamples):
                v = self.net(x, sig[i], **kwargs)
                row = table[i * num_resamples + r]
                x = ops.v_inpaint_step_rng(x, v.contiguous(), src, mask_u8, row[:4].view(torch.float32), row[4:])
            if host_sigmas is not None:
                bar.set_description(f"Inpainting (noise={host_sigmas[i + 1]:.2f})")
        return x

    def _forward_graph(self, x, src, mask_u8, sig, table, num_steps, num_resamples, kwargs) -> Optional[Tensor]:
        """One resample = U-Net forward + adp_v_inpaint_step_rng in place on the static x, captured once per call structure
        (`_CapturedSteps`) and replayed for every (step, resample) pair.  The entry owns static copies of source, mask, the
        sigma row, the pair's table row and every tensor kwarg; one tiny device-to-device copy (the row) precedes each
        replay, and one more (the sigma row) when the step changes.  None = eager fallback."""
        def build(skw):
            sx, ssig, srow = torch.empty_like(x), torch.empty_like(sig[0]), torch.empty_like(table[0])
            ssrc, smask = torch.empty_like(src), torch.empty_like(mask_u8)
            for st, t in ((sx, x), (ssig, sig[0]), (srow, table[0]), (ssrc, src), (smask, mask_u8)):
                st.copy_(t)
            sab, srng = srow[:4].view(torch.float32), srow[4:]

            def step(warm: bool):
                v = self.net(sx, ssig, **skw)
                # captured in place: each element is read, then written, by the lane that owns it
                ops.v_inpaint_step_rng(sx, v.contiguous(), ssrc, smask, sab, srng, out=torch.empty_like(sx) if warm else sx)

            return sx, step, dict(ssig=ssig, srow=srow, ssrc=ssrc, smask=smask)

        entry = self._captured_step(x, kwargs, build)
        if entry is None:
            return None
        self.graph_replays += 1
        graph, sx, ssig, srow = entry.graph, entry.sx, entry.ssig, entry.srow
        for st, t in ((sx, x), (entry.ssrc, src), (entry.smask, mask_u8)):
            st.copy_(t)
        for i in range(num_steps):
            ssig.copy_(sig[i])
            for r in range(num_resamples):
                srow.copy_(table[i * num_resamples + r])
                graph.replay()
        return sx.clone()
