"""Autoregressive v-diffusion on the gfx950 kernels: `ARVDiffusion`, `ARVSampler` and the `DiffusionAR` wrapper,
API-compatible with /root/reference/audio_diffusion_pytorch/diffusion.py:98-130, :193-296 and models.py:227-250.

    from audio_diffusion_pytorch_amd.ar import DiffusionAR, ARVDiffusion, ARVSampler

(The package's top-level name `DiffusionAR` still is the out-of-scope stub that the test-suite pins; it points here.
DESIGN.md section 7.)

A window of `length` positions is cut into `num_splits` splits and every split carries its own noise level, which the net
reads as one extra input channel (the "sigma plane").  Training noises each split to a level of its own; sampling first
denoises one window with a uniform schedule, then runs a "ladder" of levels (zero over the first half of the window, which is
the context; decreasing towards it over the second half) and shifts the window by one split per ladder pass, which yields
audio of unbounded length.

What is organised around the kernels rather than around torch ops:
  * noising, targets and the sigma plane are one kernel (adp_arv_noise); a sampler update and the next step's plane are one
    kernel (adp_arv_step), in place; the trigonometry is evaluated per split, not per element;
  * `[x_noisy | sigma plane]` is never formed around a UNetV0: its depth-0 convs read the plane through their second input
    pointer (`x_append`); around any other net the concat is one strided-copy kernel pair (ops.concat_channels);
  * noise levels are constant within a split and equal over the batch, so a loop's schedule is a [steps, num_splits, 5] table
    built on the host and kept on the device: the loop never reads device memory, and ONE captured step (net forward +
    adp_arv_step in place on x and on the plane) serves the uniform start and every ladder pass.  Per step only the
    [num_splits, 5] row block is copied in front of the replay;
  * the training step replays from hipGraphs through graphed.TrainStepGraphs, under VDiffusion's conditions;
  * the window is shifted with strided row copies (adp_copy2d) out of / into one preallocated output.
"""
from typing import Any, Callable, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Generator, Tensor
from tqdm import tqdm

from . import ops
from .components import _accepts_x_append, _ConcatChannels
from .diffusion import (Diffusion, Sampler, UniformDistribution, VDiffusion, _CapturedSteps, _on_device_of, alpha_beta,
                        fused_mse_loss)
from .models import DiffusionModel


class _ARVNoise(torch.autograd.Function):
    """(x_noisy, v_target, sigma plane) of diffusion.py:118-127 as one kernel; data and draws are not differentiated."""

    @staticmethod
    def forward(ctx, x, noise, sigmas):
        outs = ops.arv_noise(x.contiguous(), noise.contiguous(), sigmas.contiguous())
        ctx.mark_non_differentiable(*outs)
        return outs

    @staticmethod
    def backward(ctx, *g):
        return None, None, None


class ARVDiffusion(Diffusion):
    def __init__(self, net: nn.Module, length: int, num_splits: int, loss_fn: Any = F.mse_loss, use_graph: bool = True):
        """`use_graph` (not in the reference): as VDiffusion's -- replay the training step from hipGraphs where that is safe."""
        super().__init__()
        assert length % num_splits == 0, "length must be divisible by num_splits"
        self.net = net
        self.length = length
        self.num_splits = num_splits
        self.split_length = length // num_splits
        self.loss_fn = loss_fn
        self.use_graph = use_graph
        # (what the replayed step is keyed on besides loss_fn: the levels are torch.rand draws, U(0, 1))
        self.sigma_distribution = UniformDistribution()
        self.two_pointer = _accepts_x_append(net)

    def get_alpha_beta(self, sigmas: Tensor) -> Tuple[Tensor, Tensor]:
        return alpha_beta(sigmas)

    # the captured-step cache and the conditions under which it may serve a call are VDiffusion's
    train_graphs = VDiffusion.train_graphs
    _graph_path_ok = VDiffusion._graph_path_ok
    GRAPH_DISTRIBUTIONS = VDiffusion.GRAPH_DISTRIBUTIONS

    def forward(self, x: Tensor, noise: Optional[Tensor] = None, sigmas: Optional[Tensor] = None, **kwargs) -> Tensor:
        """Diffusion loss of the v-objective with one noise level per split.  `sigmas` ([b, 1, num_splits]) and `noise` (x's
        shape) let a harness inject the draws; by default they are torch.rand((b, 1, num_splits)) and then
        torch.randn_like(x), on x's device, as at diffusion.py:118-121."""
        assert x.shape[-1] == self.length, "input length must match length"
        if self._graph_path_ok(x, noise):
            with _on_device_of(x):
                # (an injected `sigmas` travels with the keyword tensors: the entry owns a static copy of it)
                loss = self.train_graphs().run(x, noise, kwargs if sigmas is None else dict(kwargs, sigmas=sigmas))
            if loss is not None:
                return loss
        return self._forward_eager(x, noise, sigmas=sigmas, **kwargs)

    def _forward_eager(self, x: Tensor, noise: Optional[Tensor] = None, sigmas: Optional[Tensor] = None, **kwargs) -> Tensor:
        b, n = x.shape[0], self.num_splits
        with _on_device_of(x):
            if sigmas is None:
                sigmas = torch.rand((b, 1, n), device=x.device, dtype=x.dtype)
            elif sigmas.numel() != b * n:
                raise ValueError(f"sigmas must be [batch, 1, num_splits] = {(b, 1, n)}; got {tuple(sigmas.shape)}")
            if noise is None:
                noise = torch.randn_like(x)
            x_noisy, v_target, plane = _ARVNoise.apply(x, noise, sigmas.reshape(b, n).to(torch.float32))
            if self.two_pointer:
                v_pred = self.net(x_noisy, x_append=plane, **kwargs)
            else:
                v_pred = self.net(_ConcatChannels.apply(x_noisy, plane), **kwargs)
            if self.loss_fn is F.mse_loss:
                return fused_mse_loss(v_pred, v_target)
            return self.loss_fn(v_pred, v_target)


def _randn(shape, device, generator: Optional[Generator]) -> Tensor:
    """N(0, 1) where the reference draws it (on the device) -- or, with a CPU `generator`, on the host in the same order and
    shapes and then copied, so that seeded runs see the same noise on any backend."""
    if generator is None:
        return torch.randn(shape, device=device)
    return torch.randn(shape, generator=generator, device=generator.device).to(device)


class ARVSampler(_CapturedSteps, Sampler):
    def __init__(self, net: nn.Module, in_channels: int, length: int, num_splits: int, use_graph: bool = True):
        super().__init__()
        assert length % num_splits == 0, "length must be divisible by num_splits"
        self.length = length
        self.in_channels = in_channels
        self.num_splits = num_splits
        self.split_length = length // num_splits
        self.net = net
        self.use_graph = use_graph
        self.two_pointer = _accepts_x_append(net)
        self._init_graph_cache()  # (graph_replays counts loops served by replays)

    @property
    def device(self):
        return next(self.net.parameters()).device

    def get_alpha_beta(self, sigmas: Tensor) -> Tuple[Tensor, Tensor]:
        return alpha_beta(sigmas)

    def _ladder_splits(self, num_steps_per_split: int) -> Tensor:
        """Host [i + 1, 2 * (num_splits // 2)]: the ladder's level per step and split (diffusion.py:213-221 without the
        repeats over batch and positions)."""
        i, n_half = num_steps_per_split, self.num_splits // 2
        sig = torch.linspace(1, 0, i * n_half).view(n_half, i).t()    # "(n i) -> i n"
        sig = torch.flip(sig, dims=[-1])                               # lowest noise level first
        sig = F.pad(sig, pad=[0, 0, 0, 1])                             # add index i + 1
        sig[-1, 1:] = sig[0, :-1]                                      # loop back at index i + 1
        return torch.cat([torch.zeros_like(sig), sig], dim=-1)         # the context half stays clean

    def get_sigmas_ladder(self, num_items: int, num_steps_per_split: int) -> Tensor:
        """[i + 1, b, 1, T] like the reference's.  Formed on the host (the same values on every backend), then moved."""
        sig = self._ladder_splits(num_steps_per_split)
        steps, n2 = sig.shape
        full = sig[:, None, None, :, None].expand(steps, num_items, 1, n2, self.split_length)
        return full.reshape(steps, num_items, 1, n2 * self.split_length).to(self.device)

    def _loop_tables(self, sig: Tensor, device) -> Tuple[Tensor, Tensor]:
        """Host levels [K + 1, num_splits] -> device (first row [num_splits], per-step rows [K, num_splits, 5] of
        (a_i, b_i, a_{i+1}, b_{i+1}, sigma_{i+1})).  Nothing here, or in the loop, reads device memory."""
        sig = sig.to(torch.float32)
        alphas, betas = self.get_alpha_beta(sig)
        coef = torch.stack([alphas[:-1], betas[:-1], alphas[1:], betas[1:], sig[1:]], dim=-1).contiguous()
        return sig[0].contiguous().to(device), coef.to(device)

    def _net_v(self, x: Tensor, plane: Tensor, kwargs) -> Tensor:
        if self.two_pointer:
            return self.net(x, x_append=plane, **kwargs).contiguous()
        return self.net(ops.concat_channels(x, plane), **kwargs).contiguous()

    def _build_step(self, x: Tensor, skw):
        """`_CapturedSteps._captured_step`'s `build` for x's shape: one step = net forward + adp_arv_step."""
        b, _, t = x.shape
        sx = torch.zeros_like(x)
        splane = torch.zeros((b, 1, t), dtype=torch.float32, device=x.device)
        scoef = torch.zeros((self.num_splits, 5), dtype=torch.float32, device=x.device)

        def step(warm: bool):
            # captured in place on x and on the plane: each element is read, then written
            ops.arv_step(sx, self._net_v(sx, splane, skw), scoef, out=torch.empty_like(sx) if warm else sx,
                         plane_out=torch.empty_like(splane) if warm else splane)

        return sx, step, dict(splane=splane, scoef=scoef)

    def _loop(self, x: Tensor, plane: Tensor, first: Tensor, coef: Tensor, graph, scoef, show_progress: bool, kwargs) -> None:
        """sample_loop (diffusion.py:223-238) in place on x; `plane` is the step's sigma channel."""
        b, _, t = x.shape
        ops.arv_plane(first, b, t, out=plane)
        if graph is not None:
            self.graph_replays += 1
            for i in range(coef.shape[0]):
                scoef.copy_(coef[i])
                graph.replay()
            return
        for i in tqdm(range(coef.shape[0]), disable=not show_progress):
            ops.arv_step(x, self._net_v(x, plane, kwargs), coef[i], out=x, plane_out=plane)

    @torch.no_grad()
    def forward(self, num_items: int, num_chunks: int, num_steps: int, start: Optional[Tensor] = None,
                show_progress: bool = False, generator: Optional[Generator] = None, **kwargs) -> Tensor:
        """[num_items, in_channels, num_chunks * split_length].  `start` is accepted and ignored, as in the reference.
        `generator` (not in the reference): None draws on the device in the reference's order; a CPU generator draws the
        same shapes in the same order on the host."""
        b, c, n, l, t = num_items, self.in_channels, self.num_splits, self.split_length, self.length
        assert num_chunks >= n, f"required at least {n} chunks"
        shifts = num_chunks > n
        if shifts:
            if n % 2:
                raise ValueError(f"ARVSampler: num_splits={n} is odd, so the half ladder plus its context covers only "
                                 f"{n - 1} of the {n} splits; generating num_chunks={num_chunks} > num_splits needs an even "
                                 f"num_splits")
            assert num_steps >= n, "num_steps must be greater than num_splits"
        device = self.device
        with _on_device_of(next(self.net.parameters())):
            prepare = getattr(self.net, "prepare_sampling_kwargs", None)
            x = _randn((b, c, t), device, generator).contiguous()  # (times sigmas[0] = 1 in the reference)
            if prepare is not None:
                kwargs = prepare(x, kwargs)
            entry = None
            if self.use_graph and x.is_cuda and not show_progress:
                entry = self._captured_step(x, kwargs, lambda skw: self._build_step(x, skw))
            if entry is not None:
                graph, sx, plane, scoef = entry.graph, entry.sx, entry.splane, entry.scoef
                sx.copy_(x)
                x = sx
            else:
                graph, scoef = None, None
                plane = torch.empty((b, 1, t), dtype=torch.float32, device=device)
            # sample_start: the same schedule over all splits
            uniform = torch.linspace(1, 0, num_steps + 1)[:, None].expand(num_steps + 1, n)
            self._loop(x, plane, *self._loop_tables(uniform, device), graph, scoef, show_progress, kwargs)
            if not shifts:
                return x.clone()
            sig = self._ladder_splits(num_steps // n)
            first, coef = self._loop_tables(sig, device)
            # noise the start to ladder row 0 (alphas[0] * start + betas[0] * randn_like(start)); all windows live in `out`
            total = (n + num_chunks) * l
            out = torch.empty((b, c, total), dtype=torch.float32, device=device)
            flat, rows = out.view(-1), b * c
            renoised = ops.arv_noise(x, _randn((b, c, t), device, generator).contiguous(),
                                     first[None].expand(b, n).contiguous())[0]
            ops.copy_rows(renoised.view(-1), t, flat, total, rows, t)
            for j in tqdm(range(num_chunks), disable=not show_progress):
                # fresh noise chunk behind the window, then decrease the ladder noise of the last n chunks
                if j > 0:
                    ops.copy_rows(_randn((b, c, l), device, generator).contiguous().view(-1), l,
                                  flat[(n + j - 1) * l:], total, rows, l)
                ops.copy_rows(flat[j * l:], total, x.view(-1), t, rows, t)
                self._loop(x, plane, first, coef, graph, scoef, show_progress, kwargs)
                ops.copy_rows(x.view(-1), t, flat[j * l:], total, rows, t)
            _randn((b, c, l), device, generator)  # (the reference's last chunk: never used, drawn to keep the generator in step)
            return out[:, :, :num_chunks * l].contiguous()


class DiffusionAR(DiffusionModel):
    """models.py:227-250: a U-Net without time conditioning or modulation whose extra input channel is the sigma plane."""

    def __init__(self, in_channels: int, length: int, num_splits: int, diffusion_t: Callable = ARVDiffusion,
                 sampler_t: Callable = ARVSampler, **kwargs):
        super().__init__(
            in_channels=in_channels + 1,
            out_channels=in_channels,
            diffusion_t=diffusion_t,
            diffusion_length=length,
            diffusion_num_splits=num_splits,
            sampler_t=sampler_t,
            sampler_in_channels=in_channels,
            sampler_length=length,
            sampler_num_splits=num_splits,
            use_time_conditioning=False,
            use_modulation=False,
            **kwargs,
        )
