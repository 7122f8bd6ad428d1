"""Karras (EDM) diffusion -- the preconditioned denoiser of Karras et al. 2022 on the variance-exploding path x + sigma n --
on the gfx950 kernels of include/adp_edm.h: `KDiffusion` (training loss), `KSampler` (Euler / Euler-ancestral /
DPM-Solver++(2M)), `KarrasSchedule` (the rho schedule) and `LogNormalDistribution` (the usual distribution of training noise
levels).  Not in the reference as it stands (early releases of it had these names); DESIGN.md section 6, "Karras (EDM)
diffusion".

With sd = sigma_data and r = sqrt(sigma^2 + sd^2):

    c_in = 1 / r     c_skip = sd^2 / r^2     c_out = sigma sd / r     c_noise = ln(sigma) / 4
    D(x, sigma) = c_skip x + c_out F(c_in x, c_noise)                      (F: the net)

    training:  x_in = c_in (x + sigma n)     target = (x - c_skip (x + sigma n)) / c_out     loss = loss_fn(F(x_in, c_noise), target)
    sampling:  on the scaled state xs = c_in(sigma_i) x_i, which is what the net reads:
               x0 = D     nh = (x - D) / sigma     xs' = g (clip(x0) + s_down nh + s_up z) + cb (x0c - x0c_prev)

The net reads c_noise where it reads sigma under the v-objective (`net(x_in, c_noise, **kwargs)`), so the time embedding is
reused as it is.  Both steps run where the v-objective's run: the training step replays from two hipGraphs (graphed.py), the
sampler step (U-Net forward + adp_edm_step in place) from one (`diffusion._CapturedSteps`).
"""
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from . import ops
from .diffusion import (Distribution, Schedule, VDiffusion, VSampler, _Thresholded, _is_number, _on_device_of,
                        fused_mse_loss, pad_dims)


class LogNormalDistribution(Distribution):
    """sigma = exp(mean + std * z), z ~ N(0, 1): the training noise levels of Karras et al. (P_mean = -1.2, P_std = 1.2).
    Drawn with torch ops on the device asked for, so the draw can be captured in a hipGraph and every replay takes fresh
    values from torch's registered generator, as `UniformDistribution`'s does."""

    def __init__(self, mean: float = -1.2, std: float = 1.2):
        super().__init__()
        if not _is_number(mean):
            raise ValueError(f"LogNormalDistribution: mean must be a number; got {mean!r}")
        if not _is_number(std) or not std > 0.0:
            raise ValueError(f"LogNormalDistribution: std must be a positive number; got {std!r}")
        self.mean, self.std = float(mean), float(std)

    def __call__(self, num_samples: int, device: torch.device = torch.device("cpu"), generator=None):
        z = torch.randn(num_samples, device=device, dtype=torch.float32, generator=generator)
        return torch.exp(self.mean + self.std * z)

    def graph_key(self) -> Tuple:
        """What a captured training step bakes in of this distribution (graphed.py)."""
        return ("log-normal", self.mean, self.std)


class KarrasSchedule(Schedule):
    """The rho schedule of Karras et al. (eq. 5) followed by 0: `forward(n, device)` returns the n - 1 noise levels

        sigma_i = (sigma_max^(1/rho) + i / (n - 2) (sigma_min^(1/rho) - sigma_max^(1/rho)))^rho,    i = 0 .. n - 2

    and then sigma = 0, so a sampler run of N steps (`schedule(N + 1)`) takes N - 1 steps on the rho schedule from sigma_max
    to sigma_min and a last one to the data.  Formed in float64 on the host and rounded to float32 once: a pure function of
    n, nothing is read from the device."""

    def __init__(self, sigma_min: float, sigma_max: float, rho: float = 7.0):
        super().__init__()
        if not _is_number(sigma_min) or not sigma_min > 0.0:
            raise ValueError(f"KarrasSchedule: sigma_min must be a positive number; got {sigma_min!r}")
        if not _is_number(sigma_max) or not sigma_max > sigma_min:
            raise ValueError(f"KarrasSchedule: sigma_max must be a number above sigma_min = {sigma_min!r}; got {sigma_max!r}")
        if not _is_number(rho) or not rho > 0.0:
            raise ValueError(f"KarrasSchedule: rho must be a positive number; got {rho!r}")
        self.sigma_min, self.sigma_max, self.rho = float(sigma_min), float(sigma_max), float(rho)

    def forward(self, num_steps: int, device) -> Tensor:
        n = int(num_steps) - 1
        if n < 0:
            raise ValueError(f"KarrasSchedule: num_steps must be at least 1 (the closing 0); got {num_steps!r}")
        ramp = torch.arange(n, dtype=torch.float64) / max(n - 1, 1)
        lo, hi = self.sigma_min ** (1.0 / self.rho), self.sigma_max ** (1.0 / self.rho)
        sigmas = (hi + ramp * (lo - hi)) ** self.rho
        return torch.cat([sigmas, torch.zeros(1, dtype=torch.float64)]).to(torch.float32).to(device)


class _EDMNoise(torch.autograd.Function):
    """x_in = c_in (x + sigma n) ; target = (x - c_skip (x + sigma n)) / c_out as one kernel; data and draws are not
    differentiated."""

    @staticmethod
    def forward(ctx, x, noise, sigmas, sigma_data):
        x_in, target = ops.edm_noise(x.contiguous(), noise.contiguous(), sigmas.contiguous(), sigma_data)
        ctx.mark_non_differentiable(x_in, target)
        return x_in, target

    @staticmethod
    def backward(ctx, *g):
        return None, None, None, None


class KDiffusion(VDiffusion):
    """The EDM training loss.  Karras' weighted loss (1 / c_out^2) |D - x|^2 equals the unweighted loss of the net's output
    against (x - c_skip (x + sigma n)) / c_out (their eq. 8), so the step is one noising kernel in front of `VDiffusion`'s
    loss path.  `forward(x, noise=None, **kwargs)`, the replayed step and its conditions are `VDiffusion`'s;
    `sigma_distribution` draws the noise levels sigma > 0, and the replayed step takes `LogNormalDistribution`.  `sigma_data`
    (the standard deviation of the data) is fixed at construction: a captured step has it baked in."""

    GRAPH_DISTRIBUTIONS = (LogNormalDistribution,)

    def __init__(self, net: nn.Module, sigma_data: float = 0.5, sigma_distribution: Distribution = LogNormalDistribution(),
                 loss_fn=F.mse_loss, use_graph: bool = True):
        sd = ops._check_sigma_data("KDiffusion", sigma_data)
        super().__init__(net=net, sigma_distribution=sigma_distribution, loss_fn=loss_fn, use_graph=use_graph)
        self._sd = sd

    @property
    def sigma_data(self) -> float:
        return self._sd

    def _forward_eager(self, x: Tensor, noise: Optional[Tensor] = None, **kwargs) -> Tensor:
        with _on_device_of(x):
            sigmas = self.sigma_distribution(num_samples=x.shape[0], device=x.device).to(torch.float32)
            if noise is None:
                noise = torch.randn_like(x)
            x_in, target = _EDMNoise.apply(x, noise, sigmas, self._sd)
            pred = self.net(x_in, torch.log(sigmas) * 0.25, **kwargs)
            if self.loss_fn is F.mse_loss:
                return fused_mse_loss(pred, target)
            return self.loss_fn(pred, target)

    def denoise(self, x_noisy: Tensor, sigmas: Tensor, **kwargs) -> Tensor:
        """D(x_noisy, sigma) = c_skip x_noisy + c_out F(c_in x_noisy, ln(sigma) / 4) for x_noisy [B, ...] and sigmas [B] > 0:
        the denoiser itself, for callers who want it (an evaluation, a sampler of their own).  Off the training and the
        sampling path, whose kernels never form D on its own: the scalings here are torch elementwise ops."""
        with _on_device_of(x_noisy):
            sigmas = torch.as_tensor(sigmas, dtype=torch.float32, device=x_noisy.device).expand(x_noisy.shape[0])
            s = pad_dims(sigmas, x_noisy.ndim - 1)
            r2 = s * s + self._sd * self._sd
            out = self.net((x_noisy * torch.rsqrt(r2)).contiguous(), torch.log(sigmas) * 0.25, **kwargs)
            return (self._sd * self._sd / r2) * x_noisy + (s * self._sd * torch.rsqrt(r2)) * out


class KSampler(_Thresholded, VSampler):
    """Samples an EDM-trained net along the schedule's noise levels sigma_0 > ... > sigma_N (`KarrasSchedule`: sigma_N = 0),
    one net evaluation per step, optionally with the predicted data thresholded at every step (as `VThresholdSampler` does).
    The state is the SCALED value xs_i = c_in(sigma_i) x_i, exactly what the net reads: no scaling pass runs in front of the
    net, and the state stays O(1) at every sigma.  With F_i = net(xs_i, ln(sigma_i) / 4), sd = sigma_data, r = sqrt(s^2 + sd^2):

        x0  = (sd^2 / r_i) xs_i + (sigma_i sd / r_i) F_i         (the denoiser's output D)
        nh  = (sigma_i / r_i) xs_i - (sd / r_i) F_i              (the predicted noise (x - D) / sigma, from the raw F)
        x0c = x0 | clamp(x0, -1, 1) | clamp(x0, -s_r, s_r) / s_r (dynamic_threshold None | 0.0 | q)
        xs_{i+1} = g (x0c + s_down nh + s_up z_i) + cb_i (x0c - x0c_{i-1})
        g = c_in(sigma_{i+1}), and 1 on the last step: the run ends unscaled with no extra kernel
        s_up = min(sigma_{i+1}, eta sqrt(sigma_{i+1}^2 (sigma_i^2 - sigma_{i+1}^2) / sigma_i^2)),  s_down = sqrt(sigma_{i+1}^2 - s_up^2)

    `eta=0` is the Euler (DDIM) step D + sigma_{i+1} nh, `eta=1` Euler-ancestral; z_i is draw 1 + i of `forward(..., seed=)`,
    formed in registers from the generator of include/adp_rng.h.  `order=2` (with eta = 0 only) is DPM-Solver++(2M): with
    h_i = ln(sigma_i / sigma_{i+1}), cb_i = g (1 - sigma_{i+1} / sigma_i) h_i / (2 h_{i-1}), and 0 on the first step and
    where sigma_{i+1} = 0.  The history is one tensor (the clipped x0); a row with cb = 0 does not read it, so nothing of an
    earlier run reaches the next one.

    One step is the net and ONE update kernel (adp_edm_step), which reads its row (a0, b0, e0, f0, c1, d1, s1, cb) -- for
    eta > 0 next to (seed_lo, seed_hi, 1 + i, 0) -- from a device table built once per run in float64 and rounded once
    (`ops.edm_table`).  The loop, the hoisted conditioning and the captured-step cache are `VSampler`'s: one captured graph
    serves every `num_steps`; `order`, whether eta > 0 and the clip mode are part of its key.

    `forward(x_noisy, num_steps, start=clip)`: x_noisy is UNIT noise; the run starts from start + sigma_0 x_noisy (start
    omitted: zero), formed by adp_edm_noise, whose first output is already the scaled state.

    The inpainter on this state is `repaint.KRepainter`.  Out of scope: `ar.ARVSampler`, a second-order stochastic update, Heun / two-evaluation steps."""

    diffusion_types = [KDiffusion]

    def __init__(self, net: nn.Module, schedule: Schedule, sigma_data: float = 0.5, order: int = 2, eta: float = 0.0,
                 dynamic_threshold: Optional[float] = None, use_graph: bool = True):
        sd = ops._check_sigma_data("KSampler", sigma_data)
        if not _is_number(order) or order not in (1, 2):
            raise ValueError(f"KSampler: order must be 1 or 2; got {order!r}")
        if not _is_number(eta) or not 0.0 <= eta <= 1.0:
            raise ValueError(f"KSampler: eta must be a number in [0, 1]; got {eta!r}")
        if eta > 0.0 and order == 2:
            raise ValueError("KSampler: eta > 0 needs order=1 (there is no second-order stochastic update)")
        threshold = self._threshold("KSampler", dynamic_threshold, none_ok=True)
        super().__init__(net=net, schedule=schedule, use_graph=use_graph)
        self.sigma_data = sd
        self.order = order
        self.eta = float(eta)
        self.dynamic_threshold = threshold
        self._seed = 0  # of the sampling run in progress: what `forward` hands to `_tables`

    def _sigmas(self, num_steps: int, device) -> Tensor:
        """The run's noise levels [N+1], float32 on the device."""
        return self.schedule(num_steps + 1, device=device).to(torch.float32)

    def _tables(self, num_steps: int, b: int, device):
        """The c_noise table [N+1, B] the net is given (ln(sigma_i) / 4; its last row, where sigma may be 0, is 0 and is never
        read) and the per-step rows of `ops.edm_table`: [N, 8] float32 for eta == 0, [N, 12] int32 words for eta > 0, the bits
        of the coefficients next to (seed_lo, seed_hi, 1 + i, 0).  The rows are formed in float64 on the host (one small
        device-to-host copy per sampling run, none in the loop) from the float32 sigmas and rounded to float32 once."""
        sigmas = self._sigmas(num_steps, device)
        try:
            coef = ops.edm_table(sigmas, self.sigma_data, self.order, self.eta)
        except ValueError as e:
            raise ValueError(f"KSampler: the schedule does not fit ({e})") from None
        c_noise = torch.cat([torch.log(sigmas[:-1]) * 0.25, torch.zeros(1, dtype=torch.float32, device=sigmas.device)])
        c_noise = c_noise[:, None].expand(num_steps + 1, b).contiguous()
        if self.eta == 0.0:
            return c_noise, coef.to(device)
        rng = ops.rng_rows(self._seed, range(1, 1 + num_steps))
        return c_noise, torch.cat([coef.view(torch.int32), rng], dim=1).contiguous().to(device)

    def _step_key(self) -> Tuple:
        return (self.order, self.eta > 0.0, self.dynamic_threshold)

    def _step_buffers(self, x: Tensor) -> Tuple[Tensor, ...]:
        """The threshold's buffers, then the history x0c_{i-1} for order 2, left uninitialised: the first step of every run
        (cb = 0) writes it without reading it."""
        return self._threshold_buffers(x) + ((torch.empty_like(x),) if self.order == 2 else ())

    def _step(self, x: Tensor, v: Tensor, row: Tensor, bufs: Tuple[Tensor, ...], out: Optional[Tensor]) -> Tensor:
        noisy = row.dtype == torch.int32  # (the row of an eta > 0 table)
        coef, rng = (row[:8].view(torch.float32), row[8:]) if noisy else (row, None)
        scale, hist = self._threshold_scale(x, v, coef, bufs)
        clip = self.dynamic_threshold is not None
        if self.order == 1:
            return ops.edm_step(x, v, coef, rng, scale=scale, clip=clip, out=out)
        return ops.edm_step(x, v, coef, rng, scale=scale, clip=clip, order=2, hist=hist[0], out=out, hist_out=hist[0])[0]

    @torch.no_grad()
    def forward(self, x_noisy: Tensor, num_steps: int, show_progress: bool = False, *, seed: Optional[int] = None,
                start: Optional[Tensor] = None, **kwargs) -> Tensor:
        """`seed` (eta > 0): the integer all draws of this run follow; None = one drawn from torch's default CPU generator
        (so torch.manual_seed governs it), without touching the device.  `start`: the run begins at start + sigma_0 x_noisy."""
        if start is not None and start.shape != x_noisy.shape:
            raise ValueError(f"KSampler: start must have x_noisy's shape {tuple(x_noisy.shape)}; got {tuple(start.shape)}")
        if seed is None:
            seed = int(torch.randint(0, 1 << 62, (1,)).item()) if self.eta > 0.0 else 0  # (a CPU tensor: no device sync)
        self._seed = int(seed)
        try:
            with _on_device_of(x_noisy):
                noise = x_noisy.to(torch.float32).contiguous()
                src = torch.zeros_like(noise) if start is None else start.to(torch.float32).contiguous()
                first = self._sigmas(num_steps, noise.device)[0].expand(noise.shape[0]).contiguous()
                xs = ops.edm_noise(src, noise, first, self.sigma_data)[0]
            return super().forward(xs, num_steps, show_progress, **kwargs)
        finally:
            self._seed = 0
