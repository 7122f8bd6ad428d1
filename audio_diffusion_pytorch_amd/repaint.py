"""RePaint inpainting (Lugmayr et al. 2022) for the three objectives on the gfx950 kernels of include/adp_repaint.h:
`VRepainter` (v-objective), `RFRepainter` (rectified flow) and `KRepainter` (Karras / EDM).  Not in the reference, whose
`VInpainter` re-noises only the known region: on every resample but the last it rotates (x, v) from level i to
(x_pred, noise_pred) and back to level i, which is the identity on the generated region, so `num_resamples` buys it nothing
there.  Here a resample steps to the LESS noisy level and then jumps the generated region back up with fresh noise, which
is what re-harmonises it with the known one; DESIGN.md section 6, "RePaint inpainting".

Write a level as x_l = a_l x0 + b_l n, with (a, b) = (cos, sin)(sigma pi / 2) | (1 - t, t) | (1, sigma) for v | rf | Karras.
The start state is a_0 (mask ? source : 0) + b_0 n0.  For step i = 0 .. N - 1 and resample r = 0 .. R - 1:

    p = net(state, level_i)                            (what the objective's sampler passes: sigma | t | ln(sigma) / 4)
    y = the objective's first-order deterministic update from level i to i + 1, x0 optionally thresholded
        (`VSampler` / `VThresholdSampler(order=1)` | `RFSampler(order=1)` | `KSampler(order=1, eta=0)`, bit for bit)
    r < R - 1:  y <- A y + S z,  A = a_i / a_{i+1},  S = sqrt(b_i^2 - (A b_{i+1})^2)        (q(x_i | x_{i+1}); j = i)
    r = R - 1:  y stays                                                                     (j = i + 1)
    state = mask ? a_j source + b_j z : y

One resample is the net and ONE update kernel, which forms z in registers from the library's counter-based generator
(include/adp_rng.h): draw 0 is the start noise, the pair (i, r) uses draw 1 + i R + r of `forward(..., seed=)`.  Each
resample reads one row of a device table built once per run in float64 and rounded once (`ops.repaint_table`) next to
(seed_lo, seed_hi, draw, 0); nothing in the loop reads device memory from the host, so one captured resample (net, optional
scale selection, update in place on a static x) replays for every pair.
"""
from typing import Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor
from tqdm import tqdm

from . import ops
from .diffusion import (Inpainter, LinearSchedule, Schedule, VDiffusion, _CapturedSteps, _is_number, _on_device_of,
                        _Thresholded)
from .edm import KDiffusion
from .rf import RFDiffusion


class _Repainter(_Thresholded, _CapturedSteps, Inpainter):
    """What the three inpainters share: the checks, the run's table, the eager loop and the captured resample.  An
    objective contributes its levels, what the net is given for them and its start state; its step row and (A, S, P, Q) are
    `ops.repaint_table`'s for `OBJECTIVE`."""

    OBJECTIVE = ""

    def __init__(self, net: nn.Module, schedule: Schedule, dynamic_threshold: Optional[float], use_graph: bool):
        threshold = self._threshold(type(self).__name__, dynamic_threshold, none_ok=True)
        super().__init__()
        self.net = net
        self.schedule = schedule
        self.dynamic_threshold = threshold
        self.use_graph = use_graph
        self._init_graph_cache()

    # ---- what an objective states
    sigma_data = 0.5  # (read by "k" alone)

    def _levels(self, num_steps: int, device) -> Tensor:
        """The run's levels [N+1], float32 on the device."""
        return self.schedule(num_steps + 1, device=device).to(torch.float32)

    def _net_arg(self, levels: Tensor) -> Tensor:
        """[N+1] what the net is given at each level."""
        return levels

    def _start(self, known: Tensor, noise: Tensor, first: Tensor) -> Tensor:
        """a_0 known + b_0 noise by the objective's noising kernel; first: the first level, one per item."""
        raise NotImplementedError()

    # ---- the run
    @torch.no_grad()
    def forward(self, source: Tensor, mask: Tensor, num_steps: int, num_resamples: int, show_progress: bool = False,
                x_noisy: Optional[Tensor] = None, seed: Optional[int] = None, **kwargs) -> Tensor:
        """`mask`: bool, True keeps the source; broadcast to the source's shape.  `x_noisy`: the unit start noise (default:
        draw 0).  `seed`: the integer all draws of this run follow; None = one drawn from torch's default CPU generator (so
        torch.manual_seed governs it), without touching the device.  `**kwargs` reach the net."""
        name = type(self).__name__
        if source.dtype != torch.float32:
            raise ValueError(f"{name}: source must be float32; got {source.dtype}")
        if mask.dtype != torch.bool:
            raise ValueError(f"{name}: mask must be a bool tensor (True keeps the source); got {mask.dtype}")
        try:
            mask = mask.expand_as(source)
        except RuntimeError:
            raise ValueError(f"{name}: mask of shape {tuple(mask.shape)} does not broadcast to the source's shape "
                             f"{tuple(source.shape)}") from None
        if not _is_number(num_resamples) or int(num_resamples) != num_resamples or num_resamples < 1:
            raise ValueError(f"{name}: num_resamples must be an integer >= 1; got {num_resamples!r}")
        if not _is_number(num_steps) or int(num_steps) != num_steps or num_steps < 0:
            raise ValueError(f"{name}: num_steps must be an integer >= 0; got {num_steps!r}")
        if x_noisy is not None and x_noisy.shape != source.shape:
            raise ValueError(f"{name}: x_noisy must have the source's shape {tuple(source.shape)}; got {tuple(x_noisy.shape)}")
        if seed is None:
            seed = int(torch.randint(0, 1 << 62, (1,)).item())  # (a CPU tensor: no device sync)
        with _on_device_of(source):
            return self._run(source, mask, int(num_steps), int(num_resamples), show_progress, x_noisy, int(seed), kwargs)

    def _table(self, levels: Tensor, num_resamples: int, seed: int) -> Tensor:
        """The run's table [N R, W + 8] (int32 words), one row per (step, resample) pair in loop order: the bits of the
        float32 row of `ops.repaint_table` next to (seed_lo, seed_hi, 1 + i R + r, 0).  Built once per run on the host (one
        small device-to-host copy of the levels, none in the loop) and copied to the device once."""
        try:
            coef = ops.repaint_table(self.OBJECTIVE, levels, num_resamples, self.sigma_data)
        except ValueError as e:
            raise ValueError(f"{type(self).__name__}: the schedule does not fit ({e})") from None
        rng = ops.rng_rows(seed, range(1, 1 + coef.shape[0]))
        return torch.cat([coef.view(torch.int32), rng], dim=1).contiguous().to(levels.device)

    def _run(self, source, mask, num_steps, num_resamples, show_progress, x_noisy, seed, kwargs) -> Tensor:
        src = source.contiguous()
        mask_u8 = mask.to(torch.uint8).contiguous()
        dev, b = src.device, src.shape[0]
        levels = self._levels(num_steps, dev)
        table = self._table(levels, num_resamples, seed)
        if x_noisy is not None:
            noise = x_noisy.to(torch.float32).contiguous()
        else:
            noise = ops.randn(src, ops.rng_rows(seed, [0])[0].to(dev))
        x = self._start(torch.where(mask, src, src.new_zeros(())), noise, levels[0].expand(b).contiguous())
        prepare = getattr(self.net, "prepare_sampling_kwargs", None)
        if prepare is not None:
            kwargs = prepare(x, kwargs)
        if table.shape[0] == 0:
            return x
        arg = self._net_arg(levels)[:, None].expand(num_steps + 1, b).contiguous()
        if self.use_graph and x.is_cuda and not show_progress:
            out = self._forward_graph(x, src, mask_u8, arg, table, num_steps, num_resamples, kwargs)
            if out is not None:
                return out
        host_levels = levels.tolist() if show_progress else None
        bar = tqdm(range(num_steps), disable=not show_progress)
        bufs = self._threshold_buffers(x)
        for i in bar:
            for r in range(num_resamples):
                p = self.net(x, arg[i], **kwargs)
                x = self._resample(x, p.contiguous(), src, mask_u8, table[i * num_resamples + r], bufs, None)
            if host_levels is not None:
                bar.set_description(f"Inpainting (noise={host_levels[i + 1]:.2f})")
        return x

    def _resample(self, x: Tensor, p: Tensor, src: Tensor, mask_u8: Tensor, row: Tensor, bufs: Tuple[Tensor, ...],
                  out: Optional[Tensor]) -> Tensor:
        """The update behind the net: the scale selection where the threshold is dynamic, on the step's own (a0, b0) as in
        the samplers, then the kernel; `out` may be x (each element is read, then written)."""
        words = row.numel() - 4
        coef, rng = row[:words].view(torch.float32), row[words:]
        scale, _ = self._threshold_scale(x, p, coef, bufs)
        return ops.repaint_step(self.OBJECTIVE, x, p, src, mask_u8, coef, rng, scale=scale,
                                clip=self.dynamic_threshold is not None, out=out)

    def _forward_graph(self, x, src, mask_u8, arg, table, num_steps, num_resamples, kwargs) -> Optional[Tensor]:
        """One resample = net forward [+ scale selection] + update in place on the static x, captured once per call
        structure (`_CapturedSteps`) and replayed for every (step, resample) pair.  The entry owns static copies of source,
        mask, the level row, the pair's table row, the threshold's buffers and every tensor kwarg; one tiny device-to-device
        copy (the row) precedes each replay, and one more (the level row) when the step changes.  None = eager fallback."""
        def build(skw):
            sx, sarg, srow = torch.empty_like(x), torch.empty_like(arg[0]), torch.empty_like(table[0])
            ssrc, smask = torch.empty_like(src), torch.empty_like(mask_u8)
            for st, t in ((sx, x), (sarg, arg[0]), (srow, table[0]), (ssrc, src), (smask, mask_u8)):
                st.copy_(t)
            bufs = self._threshold_buffers(sx)

            def step(warm: bool):
                p = self.net(sx, sarg, **skw)
                # captured in place: each element is read, then written, by the lane that owns it
                self._resample(sx, p.contiguous(), ssrc, smask, srow, bufs, torch.empty_like(sx) if warm else sx)

            return sx, step, dict(sarg=sarg, srow=srow, ssrc=ssrc, smask=smask, bufs=bufs)

        entry = self._captured_step(x, kwargs, build, (self.dynamic_threshold,))
        if entry is None:
            return None
        self.graph_replays += 1
        graph, sx, sarg, srow = entry.graph, entry.sx, entry.sarg, entry.srow
        for st, t in ((sx, x), (entry.ssrc, src), (entry.smask, mask_u8)):
            st.copy_(t)
        for i in range(num_steps):
            sarg.copy_(arg[i])
            for r in range(num_resamples):
                srow.copy_(table[i * num_resamples + r])
                graph.replay()
        return sx.clone()


class VRepainter(_Repainter):
    """RePaint inpainting for a v-objective net (module docstring): levels are the schedule's sigmas in [0, 1], the net reads
    sigma, the step is `VSampler`'s (dynamic_threshold None) or `VThresholdSampler(order=1)`'s."""

    diffusion_types = [VDiffusion]
    OBJECTIVE = "v"

    def __init__(self, net: nn.Module, schedule: Schedule = LinearSchedule(), dynamic_threshold: Optional[float] = None,
                 use_graph: bool = True):
        super().__init__(net, schedule, dynamic_threshold, use_graph)

    def _start(self, known: Tensor, noise: Tensor, first: Tensor) -> Tensor:
        return ops.v_noise(known, noise, first)[0]


class RFRepainter(_Repainter):
    """RePaint inpainting for a rectified-flow net (module docstring): levels are the schedule's times in [0, 1], the net
    reads t, the step is `RFSampler(order=1)`'s."""

    diffusion_types = [RFDiffusion]
    OBJECTIVE = "rf"

    def __init__(self, net: nn.Module, schedule: Schedule = LinearSchedule(), dynamic_threshold: Optional[float] = None,
                 use_graph: bool = True):
        super().__init__(net, schedule, dynamic_threshold, use_graph)

    def _start(self, known: Tensor, noise: Tensor, first: Tensor) -> Tensor:
        return ops.rf_noise(known, noise, first)[0]


class KRepainter(_Repainter):
    """RePaint inpainting for an EDM-trained net (module docstring) on `KSampler`'s SCALED state c_in(sigma) x: levels are the
    schedule's noise levels (`KarrasSchedule`: the last is 0), the net reads ln(sigma) / 4, the step is
    `KSampler(order=1, eta=0)`'s, and the run ends unscaled."""

    diffusion_types = [KDiffusion]
    OBJECTIVE = "k"

    def __init__(self, net: nn.Module, schedule: Schedule, sigma_data: float = 0.5,
                 dynamic_threshold: Optional[float] = None, use_graph: bool = True):
        sd = ops._check_sigma_data("KRepainter", sigma_data)
        super().__init__(net, schedule, dynamic_threshold, use_graph)
        self.sigma_data = sd

    def _net_arg(self, levels: Tensor) -> Tensor:
        """ln(sigma_i) / 4; the last entry, where sigma may be 0, is 0 and is never read."""
        return torch.cat([torch.log(levels[:-1]) * 0.25, torch.zeros(1, dtype=torch.float32, device=levels.device)])

    def _start(self, known: Tensor, noise: Tensor, first: Tensor) -> Tensor:
        return ops.edm_noise(known, noise, first, self.sigma_data)[0]
