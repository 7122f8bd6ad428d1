"""Rectified flow (flow matching on the straight path between data and noise) on the gfx950 kernels of include/adp_rf.h:
`RFDiffusion` (training loss), `RFSampler` (first- and second-order integrator) and `LogitNormalDistribution` (the usual
distribution of training times).  Not in the reference; DESIGN.md section 6, "Rectified flow".

Time t lies in [0, 1]: t = 1 is noise, t = 0 is data, and the net reads t where it reads sigma under the v-objective
(`net(x_t, t, **kwargs)`), so the time embedding and `LinearSchedule(1 -> 0)` are reused as they are.

    training:  x_t = (1 - t) x + t n          u_target = n - x          loss = loss_fn(net(x_t, t), u_target)
    sampling:  x0 = x - t u     eps = x + (1 - t) u     x_next = (1 - t') clip(x0) + t' eps  [+ cb (w - w_prev)]

Both steps run where the v-objective's run: the training step replays from two hipGraphs (graphed.py), the sampler step
(U-Net forward + adp_rf_step in place) from one (`diffusion._CapturedSteps`).
"""
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from . import ops
from .diffusion import (Distribution, LinearSchedule, Schedule, UniformDistribution, VDiffusion, VSampler, _Thresholded,
                        _is_number, _on_device_of, fused_mse_loss)


class LogitNormalDistribution(Distribution):
    """t = sigmoid(mean + std * z), z ~ N(0, 1): training times concentrated around sigmoid(mean), strictly inside (0, 1)
    but for float32's rounding of the tails.  Drawn with torch ops on the device asked for, so the draw can be captured in a
    hipGraph and every replay takes fresh values from torch's registered generator, as `UniformDistribution`'s does."""

    def __init__(self, mean: float = 0.0, std: float = 1.0):
        super().__init__()
        if not _is_number(mean):
            raise ValueError(f"LogitNormalDistribution: mean must be a number; got {mean!r}")
        if not _is_number(std) or not std > 0.0:
            raise ValueError(f"LogitNormalDistribution: std must be a positive number; got {std!r}")
        self.mean, self.std = float(mean), float(std)

    def __call__(self, num_samples: int, device: torch.device = torch.device("cpu"), generator=None):
        z = torch.randn(num_samples, device=device, dtype=torch.float32, generator=generator)
        return torch.sigmoid(self.mean + self.std * z)

    def graph_key(self) -> Tuple:
        """What a captured training step bakes in of this distribution (graphed.py)."""
        return ("logit-normal", self.mean, self.std)


class _RFNoise(torch.autograd.Function):
    """x_t = (1 - t) x + t n ; u_target = n - x as one kernel; data and draws are not differentiated."""

    @staticmethod
    def forward(ctx, x, noise, times):
        x_t, u_target = ops.rf_noise(x.contiguous(), noise.contiguous(), times.contiguous())
        ctx.mark_non_differentiable(x_t, u_target)
        return x_t, u_target

    @staticmethod
    def backward(ctx, *g):
        return None, None, None


class RFDiffusion(VDiffusion):
    """The rectified-flow training loss.  Arguments, `forward(x, noise=None, **kwargs)`, the replayed step and its conditions
    are `VDiffusion`'s (`sigma_distribution` draws the times t); the replayed step also takes `LogitNormalDistribution`."""

    GRAPH_DISTRIBUTIONS = (UniformDistribution, LogitNormalDistribution)

    def _forward_eager(self, x: Tensor, noise: Optional[Tensor] = None, **kwargs) -> Tensor:
        with _on_device_of(x):
            times = self.sigma_distribution(num_samples=x.shape[0], device=x.device)
            if noise is None:
                noise = torch.randn_like(x)
            x_t, u_target = _RFNoise.apply(x, noise, times.to(torch.float32))
            u_pred = self.net(x_t, times, **kwargs)
            if self.loss_fn is F.mse_loss:
                return fused_mse_loss(u_pred, u_target)
            return self.loss_fn(u_pred, u_target)


class RFSampler(_Thresholded, VSampler):
    """Integrates the rectified-flow ODE dx/dt = u(x, t) from the schedule's first time to its last, one net evaluation per
    step, optionally with the predicted data thresholded at every step (as `VThresholdSampler` does for the v-objective).

        x0  = x_i - t_i u_i                    eps = x_i + (1 - t_i) u_i        (eps always from the raw u)
        x0c = x0 | clamp(x0, -1, 1) | clamp(x0, -s_r, s_r) / s_r                (dynamic_threshold None | 0.0 | q)
        w   = eps - x0c                        (the velocity actually used: u where nothing was clipped)
        x_{i+1} = (1 - t_{i+1}) x0c + t_{i+1} eps + cb_i (w_i - w_{i-1})
        cb_i = (t_{i+1} - t_i)**2 / (2 (t_i - t_{i-1}))  for order 2 and i > 0, else 0

    Without clipping, cb = 0 is the Euler step x + (t_{i+1} - t_i) u and cb as above the variable-step two-step
    Adams-Bashforth method, with a history of one tensor.  eps is not re-derived from the clipped x0: that would divide by
    t_i, which goes to 0 at the data end.  The dynamic scale is the reference's `clip`: s_r = max(quantile_q(|x0_r|), 1) per
    batch item, by adp_clip_scale on (x, u) and the step's own coefficient row, five small launches in front of the update.

    One step is the net and ONE update kernel (adp_rf_step), which reads its row (1, t_i, 1 - t_i, t_{i+1}, 1 - t_{i+1},
    cb_i) from a device table built once per run in float64 and rounded once.  The loop, the hoisted conditioning and the
    captured-step cache are `VSampler`'s: one captured graph serves every `num_steps`; `order` and the clip mode are part of
    its key.  A row with cb = 0 does not read the history, so nothing of an earlier run reaches the next one.

    Variation: `forward(x_noisy, num_steps, start=clip, strength=s)` starts from (1 - s) start + s x_noisy at t = s and runs
    the schedule's times mapped affinely onto [s, the schedule's last time]."""

    diffusion_types = [RFDiffusion]

    def __init__(self, net: nn.Module, schedule: Schedule = LinearSchedule(), order: int = 2,
                 dynamic_threshold: Optional[float] = None, use_graph: bool = True):
        if not _is_number(order) or order not in (1, 2):
            raise ValueError(f"RFSampler: order must be 1 or 2; got {order!r}")
        threshold = self._threshold("RFSampler", dynamic_threshold, none_ok=True)
        super().__init__(net=net, schedule=schedule, use_graph=use_graph)
        self.order = order
        self.dynamic_threshold = threshold
        self._strength = 1.0  # of the sampling run in progress: what `forward` hands to `_tables`

    def _times(self, num_steps: int, device) -> Tensor:
        """The run's times [N+1], float32 on the device: what the net is given."""
        times = self.schedule(num_steps + 1, device=device).to(torch.float32)
        if self._strength == 1.0:
            return times
        end = times[-1]  # (device values: nothing is read back)
        return end + (times - end) * ((self._strength - end) / (times[0] - end))

    def _tables(self, num_steps: int, b: int, device):
        """time table [N+1, B] and the per-step rows of `ops.rf_table` [N, 6], both on the device.  cb is a quotient of small
        differences: the rows are formed in float64 on the host (one small device-to-host copy per sampling run, none in the
        loop) from the float32 times the net is given, and rounded to float32 once."""
        times = self._times(num_steps, device)
        try:
            coef = ops.rf_table(times, self.order)
        except ValueError as e:
            raise ValueError(f"RFSampler: the schedule repeats a time ({e}); neighbouring times must differ") from None
        return times[:, None].expand(num_steps + 1, b).contiguous(), coef.to(device)

    def _step_key(self) -> Tuple:
        return (self.order, self.dynamic_threshold)

    def _step_buffers(self, x: Tensor) -> Tuple[Tensor, ...]:
        """The threshold's buffers, then the history w_{i-1} for order 2, left uninitialised: the first step of every run
        (cb = 0) writes it without reading it."""
        return self._threshold_buffers(x) + ((torch.empty_like(x),) if self.order == 2 else ())

    def _step(self, x: Tensor, v: Tensor, row: Tensor, bufs: Tuple[Tensor, ...], out: Optional[Tensor]) -> Tensor:
        scale, hist = self._threshold_scale(x, v, row, bufs)
        clip = self.dynamic_threshold is not None
        if self.order == 1:
            return ops.rf_step(x, v, row, scale=scale, clip=clip, out=out)
        return ops.rf_step(x, v, row, scale=scale, clip=clip, order=2, hist=hist[0], out=out, hist_out=hist[0])[0]

    @torch.no_grad()
    def forward(self, x_noisy: Tensor, num_steps: int, show_progress: bool = False, *, start: Optional[Tensor] = None,
                strength: float = 1.0, **kwargs) -> Tensor:
        """`start`, `strength`: variation (class docstring); x_noisy is then the noise mixed into `start`."""
        if not _is_number(strength) or not 0.0 < strength <= 1.0:
            raise ValueError(f"RFSampler: strength must be a number in (0, 1]; got {strength!r}")
        if start is None and strength != 1.0:
            raise ValueError("RFSampler: strength != 1.0 needs start= (the clip to vary)")
        if start is not None and start.shape != x_noisy.shape:
            raise ValueError(f"RFSampler: start must have x_noisy's shape {tuple(x_noisy.shape)}; got {tuple(start.shape)}")
        self._strength = float(strength)
        try:
            if start is not None:
                with _on_device_of(start):
                    src, noise = start.to(torch.float32).contiguous(), x_noisy.to(torch.float32).contiguous()
                    first = self._times(num_steps, src.device)[0].expand(src.shape[0]).contiguous()
                    x_noisy = ops.rf_noise(src, noise, first)[0]
            return super().forward(x_noisy, num_steps, show_progress, **kwargs)
        finally:
            self._strength = 1.0
