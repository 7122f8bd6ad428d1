"""Spectral training losses on the gfx950 kernels (`adp_stft_loss_*`, csrc/resample.hip).

`MultiResolutionSTFTLoss` is the loss the reference's own test trains with (tests/testcustomloss.py passes auraloss's
`MultiResolutionSTFTLoss()` as `loss_fn`).  Keyword names and defaults follow auraloss 0.4.  The contract, for input x
(= v_pred) and target y (= v_target), fp32 [B, C, L], each of the B*C rows transformed on its own; per resolution
(N = fft_size, h = hop_size, W = win_length):

  X   = torch.stft(row, N, h, W, hann_window(W), center=True, pad_mode="reflect", onesided=True)
        (periodic Hann w[m] = 0.5 - 0.5 cos(2 pi m / W), zero-padded and centred in N; reflect padding N//2 on each side;
        1 + L//h frames, N//2 + 1 bins)
  m   = sqrt(max(Re^2 + Im^2, eps))
  SC  = ||m_y - m_x||_F / ||m_y||_F      (both norms over the whole [rows, bins, frames] tensor)
  LM  = mean |log m_x - log m_y|
  LIN = mean |m_x - m_y|
  STFTLoss = w_sc SC + w_log_mag LM + w_lin_mag LIN;   MultiResolutionSTFTLoss = mean of the per-resolution values.

auraloss's other options are accepted at their defaults only here (any other value raises NotImplementedError naming it);
the mel scale, the perceptual pre-filter and the stereo sum/difference loss are in `spectral.py`, on kernels of their own.
Only the input is differentiated: the gradient is the exact adjoint of the above, scaled by the incoming gradient read on
the device.  No host synchronisation and no host->device copy, so a `VDiffusion` training step with this `loss_fn` is
captured and replayed by graphed.py like the MSE step.
"""
from typing import Sequence, Tuple

import torch
from torch import Tensor, nn

from . import ops

# auraloss options the native loss implements only at these values
_FIXED = dict(window="hann_window", w_phs=0.0, sample_rate=None, scale=None, n_bins=None, perceptual_weighting=False,
              scale_invariance=False, output="loss", reduction="mean", mag_distance="L1")
MAX_RESOLUTIONS = 4  # per loss (one kernel launch per resolution, one shared reduction)


def _check_options(opts: dict):
    for name, value in opts.items():
        if name not in _FIXED:
            raise TypeError(f"unexpected keyword argument {name!r}")
        default = _FIXED[name]
        if value != default:
            raise NotImplementedError(f"{name}={value!r} is not supported by the native STFT loss "
                                      f"(only {name}={default!r})")


def _check_resolution(fft_size: int, hop_size: int, win_length: int) -> Tuple[int, int, int]:
    N, h, W = int(fft_size), int(hop_size), int(win_length)
    if N < 64 or N > 4096 or N & (N - 1):
        raise NotImplementedError(f"fft_size={fft_size}: the native STFT loss supports powers of two in [64, 4096]")
    if h < 1:
        raise ValueError(f"hop_size={hop_size} must be at least 1")
    if W < 1 or W > N:
        raise ValueError(f"win_length={win_length} must be in [1, fft_size={N}]")
    return N, h, W


class _STFTLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, res, weights):
        loss, ws = ops.stft_loss_fwd(x, y, res, *weights)
        ctx.save_for_backward(x, y)
        ctx.ws, ctx.res, ctx.weights = ws, res, weights
        return loss

    @staticmethod
    def backward(ctx, gloss):
        x, y = ctx.saved_tensors
        return ops.stft_loss_bwd(x, y, gloss.contiguous(), ctx.ws, ctx.res, *ctx.weights), None, None, None


def _stft_loss(x: Tensor, y: Tensor, res: Tuple[Tuple[int, int, int], ...], w_sc: float, w_log: float, w_lin: float,
               eps: float) -> Tensor:
    if x.dim() != 3 or x.shape != y.shape:
        raise ValueError(f"input and target must both be [batch, channels, length]; got {tuple(x.shape)} and "
                         f"{tuple(y.shape)}")
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise TypeError(f"the native STFT loss takes float32 tensors; got {x.dtype} and {y.dtype}")
    if x.device != y.device:
        raise ValueError(f"input and target are on different devices ({x.device}, {y.device})")
    if y.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("the native STFT loss differentiates its input only; the target requires grad "
                           "(pass target.detach())")
    L = x.shape[-1]
    for N, _, _ in res:
        if L <= N // 2:
            raise ValueError(f"input length {L} must exceed fft_size // 2 = {N // 2} (reflect padding)")
    return _STFTLossFn.apply(x.contiguous(), y.contiguous(), res, (float(w_sc), float(w_log), float(w_lin), float(eps)))


class STFTLoss(nn.Module):
    """One resolution of the contract above (auraloss.freq.STFTLoss)."""

    def __init__(self, fft_size: int = 1024, hop_size: int = 256, win_length: int = 1024, window: str = "hann_window",
                 w_sc: float = 1.0, w_log_mag: float = 1.0, w_lin_mag: float = 0.0, w_phs: float = 0.0,
                 sample_rate=None, scale=None, n_bins=None, perceptual_weighting: bool = False,
                 scale_invariance: bool = False, eps: float = 1e-8, output: str = "loss", reduction: str = "mean",
                 mag_distance: str = "L1", device=None):
        super().__init__()
        _check_options(dict(window=window, w_phs=w_phs, sample_rate=sample_rate, scale=scale, n_bins=n_bins,
                            perceptual_weighting=perceptual_weighting, scale_invariance=scale_invariance,
                            output=output, reduction=reduction, mag_distance=mag_distance))
        self.fft_size, self.hop_size, self.win_length = _check_resolution(fft_size, hop_size, win_length)
        self.w_sc, self.w_log_mag, self.w_lin_mag, self.eps = float(w_sc), float(w_log_mag), float(w_lin_mag), float(eps)

    def forward(self, input: Tensor, target: Tensor) -> Tensor:
        res = ((self.fft_size, self.hop_size, self.win_length),)
        return _stft_loss(input, target, res, self.w_sc, self.w_log_mag, self.w_lin_mag, self.eps)


class MultiResolutionSTFTLoss(nn.Module):
    """Mean of STFTLoss over (fft_sizes, hop_sizes, win_lengths) (auraloss.freq.MultiResolutionSTFTLoss), all
    resolutions in one native call (at most MAX_RESOLUTIONS)."""

    def __init__(self, fft_sizes: Sequence[int] = (1024, 2048, 512), hop_sizes: Sequence[int] = (120, 240, 50),
                 win_lengths: Sequence[int] = (600, 1200, 240), window: str = "hann_window", w_sc: float = 1.0,
                 w_log_mag: float = 1.0, w_lin_mag: float = 0.0, w_phs: float = 0.0, sample_rate=None, scale=None,
                 n_bins=None, perceptual_weighting: bool = False, scale_invariance: bool = False, **kwargs):
        super().__init__()
        if not len(fft_sizes) == len(hop_sizes) == len(win_lengths):
            raise ValueError("fft_sizes, hop_sizes and win_lengths must have the same length")
        if not 1 <= len(fft_sizes) <= MAX_RESOLUTIONS:
            raise NotImplementedError(f"the native STFT loss takes 1 to {MAX_RESOLUTIONS} resolutions; "
                                      f"got {len(fft_sizes)}")
        eps = kwargs.pop("eps", 1e-8)
        kwargs.pop("device", None)  # (auraloss places its window tensors with it; the kernels build the window)
        _check_options(dict(window=window, w_phs=w_phs, sample_rate=sample_rate, scale=scale, n_bins=n_bins,
                            perceptual_weighting=perceptual_weighting, scale_invariance=scale_invariance, **kwargs))
        self.resolutions = tuple(_check_resolution(*r) for r in zip(fft_sizes, hop_sizes, win_lengths))
        self.w_sc, self.w_log_mag, self.w_lin_mag, self.eps = float(w_sc), float(w_log_mag), float(w_lin_mag), float(eps)

    def forward(self, input: Tensor, target: Tensor) -> Tensor:
        return _stft_loss(input, target, self.resolutions, self.w_sc, self.w_log_mag, self.w_lin_mag, self.eps)
