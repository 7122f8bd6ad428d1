"""Learned-transform front end on the gfx950 kernels: `LTPlugin`, API-compatible with
/root/reference/audio_diffusion_pytorch/components.py:113-159.

    from audio_diffusion_pytorch_amd.lt import LTPlugin

(The package's top-level name `LTPlugin` still is the out-of-scope stub that the test-suite pins; it points here.
DESIGN.md section 7.)

`LTPlugin(net_t, num_filters=F, window_length=W, stride=s)` returns a factory; with p = W // 2 - s // 2 the module it builds
runs the net on a learned filterbank instead of on raw samples:

    encode  Conv1d(C, C F, W, stride s, padding p, padding_mode="reflect", bias=False)   [B, C, T]   -> [B, C F, L]
    net     net_t(in_channels=C F, out_channels=Cout F, **kwargs)                         [B, C F, L] -> [B, Cout F, L]
    decode  ConvTranspose1d(Cout F, Cout, W, stride s, padding p, bias=False)             -> [B, Cout, (L - 1) s - 2 p + W]

`encode` and `decode` are an `nn.Conv1d` and an `nn.ConvTranspose1d` (the reference's initialisation, parameter shapes and
registration order [encode, decode, net]) that only HOLD the weights: the arithmetic of both layers and of all their
gradients is three kernels of csrc/lt.hip (include/adp_lt.h), because the two layers are each other's adjoints:

    encode forward   lt_conv  (reflect)      decode forward   lt_convt (plain)
    encode d/dx      lt_convt (fold)         decode d/dx      lt_conv  (zero)
    encode d/dw      lt_wgrad (reflect)      decode d/dw      lt_wgrad (zero)

The encode data gradient is launched only when the input requires grad: in diffusion training the noised input does not.
Both layers run INSIDE the net call, so the captured training step (graphed.py) and the captured sampler steps hold them.
"""
from contextlib import nullcontext
from typing import Callable, Optional

import torch
import torch.nn as nn
from torch import Tensor

from . import ops


class _EncodeFn(torch.autograd.Function):
    """Conv1d(stride, padding=pad, padding_mode="reflect", bias=False) on adp_lt_conv; d/dw on adp_lt_wgrad, d/dx on
    adp_lt_convt's fold mode."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, stride: int, pad: int) -> Tensor:
        ctx.save_for_backward(x, weight)
        ctx.stride, ctx.pad = stride, pad
        return ops.lt_conv(x, weight, stride, pad, ops.LT_REFLECT)

    @staticmethod
    def backward(ctx, g: Tensor):
        x, weight = ctx.saved_tensors
        g = g.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = ops.lt_convt(g, weight, ctx.stride, ctx.pad, ops.LT_FOLD, T=x.shape[2])
        if ctx.needs_input_grad[1]:
            dw = ops.lt_wgrad(g, x, weight.shape[2], ctx.stride, ctx.pad, ops.LT_REFLECT)
        return dx, dw, None, None


class _DecodeFn(torch.autograd.Function):
    """ConvTranspose1d(stride, padding=pad, bias=False) on adp_lt_convt; d/dw on adp_lt_wgrad, d/dx on adp_lt_conv's zero
    mode."""

    @staticmethod
    def forward(ctx, y: Tensor, weight: Tensor, stride: int, pad: int) -> Tensor:
        ctx.save_for_backward(y, weight)
        ctx.stride, ctx.pad = stride, pad
        return ops.lt_convt(y, weight, stride, pad, ops.LT_PLAIN)

    @staticmethod
    def backward(ctx, g: Tensor):
        y, weight = ctx.saved_tensors
        g = g.contiguous()
        dy = dw = None
        if ctx.needs_input_grad[0]:
            dy = ops.lt_conv(g, weight, ctx.stride, ctx.pad, ops.LT_ZERO)
        if ctx.needs_input_grad[1]:
            dw = ops.lt_wgrad(y, g, weight.shape[2], ctx.stride, ctx.pad, ops.LT_ZERO)
        return dy, dw, None, None


def _check(t: Tensor, channels: int, what: str) -> None:
    if t.dim() != 3 or t.shape[1] != channels:
        raise ValueError(f"{what} must be [batch, {channels}, length]; got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32; got {t.dtype}")


def lt_encode(x: Tensor, conv: nn.Conv1d) -> Tensor:
    """conv(x) for the plugin's `encode` module on the native kernels."""
    _check(x, conv.in_channels, "the learned transform's input")
    with torch.cuda.device(x.device) if x.is_cuda else nullcontext():
        return _EncodeFn.apply(x.contiguous(), conv.weight.contiguous(), conv.stride[0], conv.padding[0])


def lt_decode(y: Tensor, conv: nn.ConvTranspose1d) -> Tensor:
    """conv(y) for the plugin's `decode` module on the native kernels."""
    _check(y, conv.in_channels, "the net's output in the transformed domain")
    with torch.cuda.device(y.device) if y.is_cuda else nullcontext():
        return _DecodeFn.apply(y.contiguous(), conv.weight.contiguous(), conv.stride[0], conv.padding[0])


class LTNet(nn.Module):
    """Module returned by LTPlugin(net_t, ...)(...): parameters in the reference's order [encode, decode, net]."""

    def __init__(self, encode: nn.Conv1d, decode: nn.ConvTranspose1d, net: nn.Module):
        super().__init__()
        self.encode = encode
        self.decode = decode
        self.net = net
        self.window_length, self.stride, self.padding = encode.kernel_size[0], encode.stride[0], encode.padding[0]

    def num_frames(self, length: int) -> int:
        return (length + 2 * self.padding - self.window_length) // self.stride + 1

    def _check_length(self, T: int) -> None:
        W, s, p = self.window_length, self.stride, self.padding
        if T <= p:
            raise ValueError(f"signal length {T} must exceed the reflect padding window_length // 2 - stride // 2 = {p}")
        back = (self.num_frames(T) - 1) * s - 2 * p + W
        if T + 2 * p < W or back != T:
            raise ValueError(f"signal length {T} does not survive the learned transform: decode(encode(x)) would have length "
                             f"{back} (window_length={W}, stride={s}, padding={p}; the length must be a multiple of the "
                             f"stride, and window_length and stride both even or both odd halves)")

    def prepare_sampling_kwargs(self, x: Tensor, kwargs: dict) -> dict:
        inner = getattr(self.net, "prepare_sampling_kwargs", None)
        return inner(x, kwargs) if inner is not None else kwargs

    def forward(self, x: Tensor, *args, **kwargs) -> Tensor:
        _check(x, self.encode.in_channels, "the learned transform's input")
        self._check_length(x.shape[2])
        extra = kwargs.get("append_channels")
        if torch.is_tensor(extra) and extra.shape[-1] != self.num_frames(x.shape[2]):
            raise ValueError(f"append_channels reaches the wrapped net in the transformed domain: its length must be the "
                             f"{self.num_frames(x.shape[2])} frames of a signal of length {x.shape[2]}; got {extra.shape[-1]}")
        y = lt_encode(x, self.encode)
        y = self.net(y, *args, **kwargs)
        return lt_decode(y, self.decode)


def LTPlugin(net_t: Callable, num_filters: int, window_length: int, stride: int) -> Callable[..., nn.Module]:
    """Learned Transform Plugin (components.py:113-159): the same signature and return contract."""
    num_filters, window_length, stride = int(num_filters), int(window_length), int(stride)
    if num_filters < 1 or window_length < 1 or stride < 1:
        raise ValueError(f"num_filters={num_filters}, window_length={window_length} and stride={stride} must be positive")
    padding = window_length // 2 - stride // 2
    if padding < 0:
        raise ValueError(f"window_length={window_length} is shorter than stride={stride}: the padding window_length // 2 - "
                         f"stride // 2 = {padding} would be negative")

    def Net(dim: int, in_channels: int, out_channels: Optional[int] = None, **kwargs) -> nn.Module:
        if dim != 1:
            raise NotImplementedError(f"LTPlugin is implemented for dim=1 (the reference's decode is a ConvTranspose1d); "
                                      f"got dim={dim}")
        out_channels = in_channels if out_channels is None else out_channels
        encode = nn.Conv1d(in_channels=in_channels, out_channels=in_channels * num_filters, kernel_size=window_length,
                           stride=stride, padding=padding, padding_mode="reflect", bias=False)
        decode = nn.ConvTranspose1d(in_channels=out_channels * num_filters, out_channels=out_channels,
                                    kernel_size=window_length, stride=stride, padding=padding, bias=False)
        net = net_t(dim=dim, in_channels=in_channels * num_filters, out_channels=out_channels * num_filters, **kwargs)
        return LTNet(encode, decode, net)

    return Net
