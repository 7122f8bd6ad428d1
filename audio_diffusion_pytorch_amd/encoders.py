"""Mel encoder for `DiffusionAE` on the gfx950 kernels: `MelE1d` and `TanhBottleneck`, the encoder of the reference README's
"Diffusion Autoencoder" example (there imported from the third-party package audio_encoders_pytorch).

    from audio_diffusion_pytorch_amd.encoders import MelE1d, TanhBottleneck

The architecture is that package's MelE1d as specified in DESIGN.md section 6 ("Mel encoder"); the package is not available
to this project, so checkpoint interchange with it is NOT claimed.  With c_i = channels * multipliers[i]:

    mel                  vocoder.MelSpectrogram                       [B, C, T]        -> [B, C, F, L] viewed as [B, C F, L]
    to_in                Conv1d(C F, c_0, 1)
    downsample[i].down   Conv1d(c_i, c_{i+1}, 2 f_i + 1, stride f_i, padding f_i)       L -> ceil(L / f_i)
    downsample[i].blocks[j]   h + conv2(silu(norm2(conv1(silu(norm1(h))))))             GroupNorm(resnet_groups), k = 3 convs
    to_out               Conv1d(c_last, out_channels, 1)              (only when out_channels is given)
    bottleneck           tanh                                         (only with TanhBottleneck())

The parameters live in plain torch.nn modules (PyTorch's initialisation and state-dict keys) that only HOLD them: their own
`forward` is never called.  The k = 1 and k = 3 convs, GroupNorm + SiLU and all their gradients run on the conv families and
norm kernels of include/adp.h exactly as the U-Net's ResnetBlock does (unet.py: `resnet` below 64 channels, `resnet_wide`
from there on); the overlapping strided downsample, which those families do not take, and the tanh run on csrc/encoder.hip
(include/adp_enc.h).  The whole stack is ONE autograd node whose backward walks a tape of closures in reverse; the waveform
is not differentiated.
"""
from contextlib import nullcontext
from math import prod
from typing import Optional, Sequence

import torch
import torch.nn as nn
from torch import Tensor

from . import ops
from .models import EncoderBase
from .unet import ACT_MATERIALIZE_MIN_C
from .vocoder import MelSpectrogram


class TanhBottleneck(nn.Module):
    """Marker for MelE1d(bottleneck=...): the latent goes through tanh (adp_enc_tanh_fwd / _bwd inside the encoder)."""

    def forward(self, x: Tensor, with_info: bool = False):
        if x.dtype != torch.float32:
            raise TypeError(f"TanhBottleneck takes float32; got {x.dtype}")
        if x.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("TanhBottleneck on its own does not differentiate; inside MelE1d it is part of the encoder's "
                               "autograd node")
        with torch.cuda.device(x.device) if x.is_cuda else nullcontext():
            z = ops.enc_tanh_fwd(x.contiguous())
        return (z, {}) if with_info else z


class _ResnetBlock(nn.Module):
    """Parameter holder of one block: h + conv2(silu(norm2(conv1(silu(norm1(h))))))."""

    def __init__(self, channels: int, groups: int):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, channels)
        self.conv1 = nn.Conv1d(channels, channels, 3, padding=1)
        self.norm2 = nn.GroupNorm(groups, channels)
        self.conv2 = nn.Conv1d(channels, channels, 3, padding=1)


class _DownsampleStage(nn.Module):
    """Parameter holder of one stage: the overlapping strided `down` conv, then `blocks`."""

    def __init__(self, in_channels: int, out_channels: int, factor: int, num_blocks: int, groups: int):
        super().__init__()
        self.factor = factor
        self.down = nn.Conv1d(in_channels, out_channels, 2 * factor + 1, stride=factor, padding=factor)
        self.blocks = nn.ModuleList([_ResnetBlock(out_channels, groups) for _ in range(num_blocks)])


class _EncoderFn(torch.autograd.Function):
    """The encoder stack behind the mel front end as one node: forward records the tape, backward walks it in reverse."""

    @staticmethod
    def forward(ctx, enc: "MelE1d", mel: Tensor, *params: Tensor) -> Tensor:
        ctx.tape, ctx.params = [], params
        return enc._run(mel, ctx.tape)

    @staticmethod
    def backward(ctx, dz: Tensor):
        grads = {}
        g = dz.contiguous()
        for bwd in reversed(ctx.tape):
            g = bwd(g, grads)
        ctx.tape = None
        return (None, None) + tuple(grads.get(id(p)) if need else None
                                    for p, need in zip(ctx.params, ctx.needs_input_grad[2:]))


class MelE1d(EncoderBase):
    """waveform [B, in_channels, T] -> latent [B, out_channels, ceil(frames / prod(factors))]; see the module docstring."""

    def __init__(self, in_channels: int, channels: int, multipliers: Sequence[int], factors: Sequence[int],
                 num_blocks: Sequence[int], mel_channels: int, mel_sample_rate: int, mel_n_fft: int = 1024,
                 mel_hop_length: Optional[int] = None, mel_win_length: Optional[int] = None, mel_normalize: bool = False,
                 mel_normalize_log: bool = False, resnet_groups: int = 8, out_channels: Optional[int] = None,
                 bottleneck: Optional[nn.Module] = None):
        super().__init__()
        multipliers, factors, num_blocks = list(multipliers), [int(f) for f in factors], [int(n) for n in num_blocks]
        if not (len(multipliers) == len(factors) + 1 == len(num_blocks) + 1):
            raise ValueError(f"MelE1d needs len(multipliers) == len(factors) + 1 == len(num_blocks) + 1; got "
                             f"{len(multipliers)}, {len(factors)}, {len(num_blocks)}")
        for f in factors:
            if f < 2 or f > 4:
                raise NotImplementedError(f"factors={factors}: the native downsample conv takes factors 2, 3 and 4")
        if bottleneck is not None and not isinstance(bottleneck, TanhBottleneck):
            raise NotImplementedError(f"bottleneck {type(bottleneck).__name__} is not implemented: MelE1d takes None or "
                                      "TanhBottleneck()")
        hop = int(mel_hop_length) if mel_hop_length is not None else int(mel_n_fft) // 4
        win = int(mel_win_length) if mel_win_length is not None else int(mel_n_fft)
        cs = [int(channels) * int(m) for m in multipliers]
        self.in_channels, self.mel_channels, self.groups = int(in_channels), int(mel_channels), int(resnet_groups)
        self.factors = factors
        self.mel = MelSpectrogram(int(mel_n_fft), hop, win, int(mel_sample_rate), int(mel_channels),
                                  normalize=mel_normalize, normalize_log=mel_normalize_log)
        self.to_in = nn.Conv1d(self.in_channels * self.mel_channels, cs[0], 1)
        self.downsample = nn.ModuleList([_DownsampleStage(cs[i], cs[i + 1], factors[i], num_blocks[i], self.groups)
                                         for i in range(len(factors))])
        if out_channels is not None:
            self.to_out = nn.Conv1d(cs[-1], int(out_channels), 1)
        self.bottleneck = bottleneck
        self.out_channels = int(out_channels) if out_channels is not None else cs[-1]
        self.downsample_factor = hop * prod(factors)

    # ---- the stack on the kernels; `tape` (a list, or None when nothing needs a gradient) receives closures
    # bwd(g, grads) -> gradient of the step's input, which leave parameter gradients in grads[id(parameter)]
    def _gn_part(self, C: int) -> Optional[ops.GnPart]:
        """A GnPart for the conv about to produce a C-channel tensor a GroupNorm reads next (unet._Run.gn_part_for)."""
        return ops.GnPart() if (C // self.groups) % 4 == 0 else None

    def _stats(self, x: Tensor, gn: Optional[ops.GnPart]) -> Tensor:
        if gn is not None and gn.covers(x):
            return ops.gn_finalize(gn.part, self.groups)
        return ops.gn_stats(x, self.groups)

    def _stats_act(self, x: Tensor, gn: Optional[ops.GnPart], norm: nn.GroupNorm):
        G = self.groups
        if gn is not None and gn.covers(x):
            part = gn.part
            if (x.shape[1] // G // 4) * part.shape[2] <= 1024:
                return ops.gn_finalize_act(x, part, G, norm.weight, norm.bias)
            st = ops.gn_finalize(part, G)
            return st, ops.gn_act(x, st, G, norm.weight, norm.bias)
        return ops.gn_stats_act(x, G, norm.weight, norm.bias)

    def _pointwise(self, conv: nn.Conv1d, x: Tensor, tape, need_dx: bool) -> Tensor:
        y = ops.conv1d(x, conv.weight, conv.bias)
        if tape is not None:
            def bwd(g, grads):
                grads[id(conv.weight)], grads[id(conv.bias)] = ops.conv1d_wgrad(x, g, 1)
                return ops.conv1d(g, conv.weight, None, transposed=True) if need_dx else None
            tape.append(bwd)
        return y

    def _down(self, stage: _DownsampleStage, x: Tensor, tape) -> Tensor:
        conv, f = stage.down, stage.factor
        y = ops.enc_down_fwd(x, conv.weight, conv.bias, f)
        if tape is not None:
            def bwd(g, grads):
                grads[id(conv.weight)], grads[id(conv.bias)] = ops.enc_down_wgrad(x, g, f)
                return ops.enc_down_dgrad(g, conv.weight, f, x.shape[2])
            tape.append(bwd)
        return y

    def _block(self, p: _ResnetBlock, x: Tensor, tape) -> Tensor:
        """One ResnetBlock, as unet._Run.resnet / resnet_wide: below ACT_MATERIALIZE_MIN_C channels SiLU(GroupNorm(.)) is the
        convs' prologue, from there on it is materialised once.  norm2's statistics come from conv1's epilogue where the
        dispatched family writes them; norm1's (behind a residual add or the down conv) from a pass over the tensor."""
        G = self.groups
        wide = x.shape[1] >= ACT_MATERIALIZE_MIN_C and x.shape[0] * x.shape[1] <= 65535
        gn_mid = self._gn_part(x.shape[1])
        if wide:
            st1, a1 = self._stats_act(x, None, p.norm1)
            h1 = ops.conv1d(a1, p.conv1.weight, p.conv1.bias, pad=1, gn=gn_mid)
            st2, a2 = self._stats_act(h1, gn_mid, p.norm2)
            y = ops.conv1d(a2, p.conv2.weight, p.conv2.bias, pad=1, res=x)
        else:
            st1 = self._stats(x, None)
            a1 = a2 = None
            h1 = ops.conv1d(x, p.conv1.weight, p.conv1.bias, pad=1, prologue=1, pro_stats=st1, pro_gamma=p.norm1.weight,
                            pro_beta=p.norm1.bias, groups=G, gn=gn_mid)
            st2 = self._stats(h1, gn_mid)
            y = ops.conv1d(h1, p.conv2.weight, p.conv2.bias, pad=1, prologue=1, pro_stats=st2, pro_gamma=p.norm2.weight,
                           pro_beta=p.norm2.bias, groups=G, res=x)
        if tape is not None:
            def wgrad(inp, act, g, st, norm):
                if wide:
                    return ops.conv1d_wgrad(act, g, 3, pad=1)
                return ops.conv1d_wgrad(inp, g, 3, pad=1, prologue=1, pro_stats=st, pro_gamma=norm.weight,
                                        pro_beta=norm.bias, groups=G)

            def bwd(gy, grads):
                grads[id(p.conv2.weight)], grads[id(p.conv2.bias)] = wgrad(h1, a2, gy, st2, p.norm2)
                gb2 = ops.GnBwdPart(h1, st2, p.norm2.weight, p.norm2.bias, G)
                dact2 = ops.conv1d(gy, p.conv2.weight, None, pad=1, transposed=True, gnb=gb2)
                dh1, grads[id(p.norm2.weight)], grads[id(p.norm2.bias)] = ops.gn_silu_bwd(
                    h1, dact2, st2, p.norm2.weight, p.norm2.bias, G, ab=gb2.ab)
                grads[id(p.conv1.weight)], grads[id(p.conv1.bias)] = wgrad(x, a1, dh1, st1, p.norm1)
                gb1 = ops.GnBwdPart(x, st1, p.norm1.weight, p.norm1.bias, G)
                dact1 = ops.conv1d(dh1, p.conv1.weight, None, pad=1, transposed=True, gnb=gb1)
                dx, grads[id(p.norm1.weight)], grads[id(p.norm1.bias)] = ops.gn_silu_bwd(
                    x, dact1, st1, p.norm1.weight, p.norm1.bias, G, dres=gy, ab=gb1.ab)
                return dx
            tape.append(bwd)
        return y

    def _run(self, mel: Tensor, tape) -> Tensor:
        h = self._pointwise(self.to_in, mel, tape, need_dx=False)   # (the spectrogram comes from data: no gradient)
        for stage in self.downsample:
            h = self._down(stage, h, tape)
            for block in stage.blocks:
                h = self._block(block, h, tape)
        if hasattr(self, "to_out"):
            h = self._pointwise(self.to_out, h, tape, need_dx=True)
        if self.bottleneck is not None:
            z = ops.enc_tanh_fwd(h)
            if tape is not None:
                tape.append(lambda g, grads: ops.enc_tanh_bwd(z, g))
            h = z
        return h

    def forward(self, x: Tensor, with_info: bool = False):
        if x.dim() != 3 or x.shape[1] != self.in_channels:
            raise ValueError(f"MelE1d takes [batch, {self.in_channels}, length]; got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise TypeError(f"MelE1d takes a float32 waveform; got {x.dtype}")
        if self.to_in.weight.device != x.device:
            raise RuntimeError(f"MelE1d lives on {self.to_in.weight.device}, the waveform on {x.device}; move the module "
                               "with .to(device)")
        B = x.shape[0]
        with torch.cuda.device(x.device) if x.is_cuda else nullcontext():
            mel = self.mel(x)                                                   # [B, C, F, L]
            mel = mel.view(B, self.in_channels * self.mel_channels, mel.shape[3])  # "b c f l -> b (c f) l", no copy
            params = [p for n, p in self.named_parameters()]
            if torch.is_grad_enabled() and any(p.requires_grad for p in params):
                z = _EncoderFn.apply(self, mel, *params)
            else:
                with torch.no_grad():
                    z = self._run(mel, None)
        return (z, {}) if with_info else z
