"""Stereo sum/difference, mel-scaled and pre-filtered STFT losses on the gfx950 kernels of include/adp_spec.h
(`adp_spec_*`, csrc/spectral.hip).

`losses.STFTLoss` / `losses.MultiResolutionSTFTLoss` implement auraloss's defaults only.  The classes here take the options
the usual stereo recipe needs: a mel scale (`scale="mel"`), a perceptual pre-filter (`perceptual_weighting=True`, or any FIR
with `prefilter=`) and the sum-and-difference (mid/side) pairing of `SumAndDifferenceSTFTLoss`.  Keyword names follow
auraloss 0.4 AS RECALLED: the package is not available where this was written, so fidelity to it -- names, defaults and above
all the numbers of its mel filterbank and of its A-weighting filter -- is UNVERIFIED.  What is computed is stated here in full.

Contract.  Input x and target y are float32 [B, C, L]; only x is differentiated.

  1. Groups.  Plain losses have one group, the B*C rows.  SumAndDifferenceSTFTLoss needs C == 2 and has two groups of B rows:
     s = x[:, 0] + x[:, 1] and d = x[:, 0] - x[:, 1] (the same for y).
  2. Pre-filter (optional; taps h, odd length T <= 255): every row becomes conv1d(row, h, padding=T // 2), i.e.
     x'[i] = sum_j h[j] x[i + j - T // 2] with zeros outside [0, L); x and y alike.  (Filtering is linear: the channels are
     filtered, then paired.)
  3. Per group and resolution (N, hop, W): X and m = sqrt(max(|X|^2, eps)) exactly as in the losses.py docstring;
     M = fb @ m with fb [n_bins, N/2 + 1] when scale="mel", else M = m;
     SC = ||M_y - M_x||_F / ||M_y||_F, LM = mean |log M_x - log M_y|, LIN = mean |M_x - M_y| over the group's whole
     [rows, bins, frames] tensor; value = w_sc SC + w_log_mag LM + w_lin_mag LIN, averaged over the resolutions.
  4. Plain losses return the group's value; sum/difference returns (w_sum value(s) + w_diff value(d)) / 2.
  5. The mel filterbank is librosa.filters.mel(sr, n_fft, n_mels) with its defaults as documented (Slaney scale, fmin = 0,
     fmax = sr / 2, Slaney area normalisation), restated in `mel_filterbank`; built on the host in float64 at construction,
     kept as float32 buffers.  A filter without a nonzero bin would make log M infinite: ValueError at construction.
  6. The gradient is the exact adjoint of the above with respect to x, scaled by the incoming gradient read on the device.
  7. No atomics, bit-identical from call to call; x == y gives loss 0.0 and an all-zero gradient bit for bit; no host read
     and no host->device copy inside the call, so a training step with these losses is captured and replayed by graphed.py.

With none of the options, the loss and its gradient are those of the `losses` classes bit for bit.  Left out (each raises
NotImplementedError naming the option): scale="chroma", the phase term (w_phs), scale_invariance, output="full", reductions
other than "mean", mag_distance other than "L1", windows other than "hann_window", fft sizes that are no power of two in
[64, 4096].  `vocoder.DiffusionVocoder` packs its channels into the batch, so sum/difference does not apply to its rows.
"""
from math import log
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from . import ops
from .losses import MAX_RESOLUTIONS, _check_resolution

# auraloss options implemented only at these values
_FIXED = dict(window="hann_window", w_phs=0.0, scale_invariance=False, output="loss", reduction="mean", mag_distance="L1")
MAX_TAPS = 255


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (log(6.4) / 27.0), f / (200.0 / 3.0))


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_filterbank(sample_rate: int, n_fft: int, n_mels: int) -> Tensor:
    """float64 [n_mels, n_fft // 2 + 1]: librosa.filters.mel(sr=sample_rate, n_fft=n_fft, n_mels=n_mels) as documented
    (Slaney mel scale, fmin = 0, fmax = sample_rate / 2, norm="slaney")."""
    freqs = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(sample_rate) / n_fft)
    pts = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sample_rate / 2.0), n_mels + 2))
    diff = np.diff(pts)
    ramps = pts[:, None] - freqs[None, :]
    lower, upper = -ramps[:-2] / diff[:-1, None], ramps[2:] / diff[1:, None]
    weights = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (pts[2:] - pts[:-2]))[:, None]
    return torch.from_numpy(weights)


def a_weighting_fir(sample_rate: int, ntaps: int = 101) -> Tensor:
    """float32 [ntaps]: a symmetric (linear-phase), odd-length FIR whose magnitude follows the analog IEC 61672 A-curve

        R_A(f) = 12194.217^2 f^4 / ((f^2 + 20.598997^2) sqrt((f^2 + 107.65265^2)(f^2 + 737.86223^2)) (f^2 + 12194.217^2))

    times 10^(1.9997 / 20) (0 dB at 1 kHz).  Design: the curve sampled at 1025 points on [0, fs/2], the linear phase of a
    delay of (ntaps - 1) / 2, inverse real FFT, the first ntaps samples, a Hamming window.  With 101 taps it is within 0.5 dB of
    the curve at 1, 2, 4 and 8 kHz for 44100 and 48000 Hz (worst 0.40 dB, at 1 kHz with 48 kHz).  101 taps cannot follow the
    curve below about 300 Hz: about -9 dB instead of -19 dB at 100 Hz.  These are NOT auraloss's taps (its design, as recalled,
    goes through scipy's bilinear / freqz / firwin2, and scipy is no dependency here)."""
    ntaps = int(ntaps)
    if ntaps < 1 or ntaps > MAX_TAPS or ntaps % 2 == 0:
        raise ValueError(f"ntaps={ntaps} must be odd and in [1, {MAX_TAPS}]")
    k = np.arange(1025, dtype=np.float64)
    f2 = (k / 1024.0 * (float(sample_rate) / 2.0)) ** 2
    mag = 12194.217 ** 2 * f2 ** 2 / ((f2 + 20.598997 ** 2) * np.sqrt((f2 + 107.65265 ** 2) * (f2 + 737.86223 ** 2)) *
                                      (f2 + 12194.217 ** 2)) * 10.0 ** (1.9997 / 20.0)
    h = np.fft.irfft(mag * np.exp(-1j * np.pi * (ntaps - 1) / 2.0 * k / 1024.0), 2048)[:ntaps] * np.hamming(ntaps)
    h = 0.5 * (h + h[::-1])  # symmetric bit for bit
    return torch.from_numpy(h).to(torch.float32)


def _ranges(nonzero: Tensor) -> Tensor:
    """int32 [rows, 2]: per row of the bool matrix the columns [lo, hi) that hold every True ([0, 0) for none)."""
    n = nonzero.shape[1]
    idx = torch.arange(n)[None, :]
    lo = torch.where(nonzero, idx, n).min(dim=1).values
    hi = torch.where(nonzero, idx + 1, 0).max(dim=1).values
    return torch.stack([torch.minimum(lo, hi), hi], dim=1).to(torch.int32).contiguous()


def _check_options(opts: dict):
    for name, value in opts.items():
        if name not in _FIXED:
            raise TypeError(f"unexpected keyword argument {name!r}")
        if value != _FIXED[name]:
            raise NotImplementedError(f"{name}={value!r} is not supported by the native STFT loss "
                                      f"(only {name}={_FIXED[name]!r})")


class _SpecLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, m):
        if m.taps is not None:
            x, y = ops.spec_fir(x, m.taps), ops.spec_fir(y, m.taps)
        args = (m.pair, m.resolutions, m.bins, m.mel_fb, m.mel_range)
        loss, ws = ops.spec_loss_fwd(x, y, *args, *m.weights)
        ctx.save_for_backward(x, y, ws)
        ctx.m = m
        return loss

    @staticmethod
    def backward(ctx, gloss):
        x, y, ws = ctx.saved_tensors
        m = ctx.m
        dx = ops.spec_loss_bwd(x, y, gloss.contiguous(), ws, m.pair, m.resolutions, m.bins, m.mel_fb, m.mel_range,
                               m.bin_range, *m.weights)
        if m.taps is not None:
            dx = ops.spec_fir(dx, m.taps_rev)  # the adjoint of the pre-filter: the same FIR with reversed taps
        return dx, None, None


class _SpecLoss(nn.Module):
    """What the classes below share: the options' checks, the buffers (filterbanks, ranges, taps) and the call."""
    pair = False

    def _setup(self, resolutions, w_sc, w_log_mag, w_lin_mag, eps, sample_rate, scale, n_bins, perceptual_weighting,
               prefilter, w_sum=1.0, w_diff=1.0):
        self.resolutions = tuple(_check_resolution(*r) for r in resolutions)
        self.w_sc, self.w_log_mag, self.w_lin_mag, self.eps = float(w_sc), float(w_log_mag), float(w_lin_mag), float(eps)
        self.w_sum, self.w_diff = float(w_sum), float(w_diff)
        self.sample_rate, self.scale, self.n_bins = sample_rate, scale, n_bins
        if scale not in (None, "mel"):
            raise NotImplementedError(f"scale={scale!r} is not supported by the native STFT loss (only scale=None or 'mel')")
        fbs, mel_ranges, bin_ranges = [], [], []
        if scale == "mel":
            if sample_rate is None or n_bins is None:
                raise ValueError("scale='mel' needs sample_rate and n_bins")
            if int(n_bins) < 1:
                raise ValueError(f"n_bins={n_bins} must be at least 1")
            for N, h, W in self.resolutions:
                fb = mel_filterbank(int(sample_rate), N, int(n_bins)).to(torch.float32)
                nz = fb != 0
                empty = (~nz.any(dim=1)).nonzero().reshape(-1).tolist()
                if empty or int(n_bins) > N // 2 - 1:
                    raise ValueError(f"resolution (fft_size={N}, hop_size={h}, win_length={W}): n_bins={n_bins} mel filters at "
                                     f"sample_rate={sample_rate} leave filter(s) {empty[:4]} without a nonzero bin among "
                                     f"{N // 2 + 1} (log M would be infinite); use fewer bins or a larger fft_size")
                fbs.append(fb.reshape(-1))
                mel_ranges.append(_ranges(nz))
                bin_ranges.append(_ranges(nz.t()))
        self.bins = tuple(int(n_bins) for _ in self.resolutions) if scale == "mel" else None
        if perceptual_weighting:
            if sample_rate is None:
                raise ValueError("perceptual_weighting=True needs sample_rate")
            if prefilter is not None:
                raise ValueError("perceptual_weighting=True and prefilter= both set the pre-filter; give one of them")
            prefilter = a_weighting_fir(int(sample_rate))
        if prefilter is not None:
            prefilter = torch.as_tensor(prefilter).detach().to("cpu", torch.float32)
            if prefilter.dim() != 1 or prefilter.numel() % 2 == 0 or prefilter.numel() > MAX_TAPS:
                raise ValueError(f"prefilter must be a 1-D tensor of an odd number of taps, at most {MAX_TAPS}; got shape "
                                 f"{tuple(prefilter.shape)}")
        # (derived from the constructor arguments: not part of the state dict; one buffer holds every resolution's part)
        self.register_buffer("mel_fb", torch.cat(fbs).contiguous() if fbs else None, persistent=False)
        self.register_buffer("mel_range", torch.cat(mel_ranges).contiguous() if fbs else None, persistent=False)
        self.register_buffer("bin_range", torch.cat(bin_ranges).contiguous() if fbs else None, persistent=False)
        self.register_buffer("taps", prefilter.contiguous() if prefilter is not None else None, persistent=False)
        self.register_buffer("taps_rev", prefilter.flip(0).contiguous() if prefilter is not None else None,
                             persistent=False)

    @property
    def weights(self) -> Tuple[float, ...]:
        return (self.w_sc, self.w_log_mag, self.w_lin_mag, self.eps, self.w_sum, self.w_diff)

    def forward(self, input: Tensor, target: Tensor) -> Tensor:
        x, y = input, target
        if x.dim() != 3 or x.shape != y.shape:
            raise ValueError(f"input and target must both be [batch, channels, length]; got {tuple(x.shape)} and "
                             f"{tuple(y.shape)}")
        if self.pair and x.shape[1] != 2:
            raise ValueError(f"the sum-and-difference loss takes stereo [batch, 2, length] tensors; got {x.shape[1]} "
                             "channel(s)")
        if x.dtype != torch.float32 or y.dtype != torch.float32:
            raise TypeError(f"the native STFT loss takes float32 tensors; got {x.dtype} and {y.dtype}")
        if x.device != y.device:
            raise ValueError(f"input and target are on different devices ({x.device}, {y.device})")
        if y.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("the native STFT loss differentiates its input only; the target requires grad "
                               "(pass target.detach())")
        L = x.shape[-1]
        for N, _, _ in self.resolutions:
            if L <= N // 2:
                raise ValueError(f"input length {L} must exceed fft_size // 2 = {N // 2} (reflect padding)")
        for buf in (self.mel_fb, self.taps):
            if buf is not None and buf.device != x.device:
                raise RuntimeError(f"the loss's buffers live on {buf.device}, the input on {x.device}; move the module "
                                   "with .to(device)")
        return _SpecLossFn.apply(x.contiguous(), y.contiguous(), self)


class STFTLoss(_SpecLoss):
    """One resolution of the contract above: `losses.STFTLoss` with scale="mel", perceptual_weighting and prefilter=."""

    def __init__(self, fft_size: int = 1024, hop_size: int = 256, win_length: int = 1024, window: str = "hann_window",
                 w_sc: float = 1.0, w_log_mag: float = 1.0, w_lin_mag: float = 0.0, w_phs: float = 0.0,
                 sample_rate=None, scale=None, n_bins=None, perceptual_weighting: bool = False,
                 scale_invariance: bool = False, eps: float = 1e-8, output: str = "loss", reduction: str = "mean",
                 mag_distance: str = "L1", device=None, prefilter: Optional[Tensor] = None):
        super().__init__()
        _check_options(dict(window=window, w_phs=w_phs, scale_invariance=scale_invariance, output=output,
                            reduction=reduction, mag_distance=mag_distance))
        self._setup(((fft_size, hop_size, win_length),), w_sc, w_log_mag, w_lin_mag, eps, sample_rate, scale, n_bins,
                    perceptual_weighting, prefilter)
        self.fft_size, self.hop_size, self.win_length = self.resolutions[0]


class MelSTFTLoss(STFTLoss):
    """STFTLoss(scale="mel", n_bins=n_mels) (auraloss.freq.MelSTFTLoss)."""

    def __init__(self, sample_rate, fft_size: int = 1024, hop_size: int = 256, win_length: int = 1024,
                 window: str = "hann_window", w_sc: float = 1.0, w_log_mag: float = 1.0, w_lin_mag: float = 0.0,
                 w_phs: float = 0.0, n_mels: int = 128, **kwargs):
        super().__init__(fft_size, hop_size, win_length, window, w_sc, w_log_mag, w_lin_mag, w_phs,
                         sample_rate=sample_rate, scale="mel", n_bins=n_mels, **kwargs)


class MultiResolutionSTFTLoss(_SpecLoss):
    """Mean of STFTLoss over (fft_sizes, hop_sizes, win_lengths), all resolutions in one native call (at most
    MAX_RESOLUTIONS): `losses.MultiResolutionSTFTLoss` with scale="mel", perceptual_weighting and prefilter=."""

    def __init__(self, fft_sizes: Sequence[int] = (1024, 2048, 512), hop_sizes: Sequence[int] = (120, 240, 50),
                 win_lengths: Sequence[int] = (600, 1200, 240), window: str = "hann_window", w_sc: float = 1.0,
                 w_log_mag: float = 1.0, w_lin_mag: float = 0.0, w_phs: float = 0.0, sample_rate=None, scale=None,
                 n_bins=None, perceptual_weighting: bool = False, scale_invariance: bool = False, **kwargs):
        super().__init__()
        self._init_multi(fft_sizes, hop_sizes, win_lengths, window, w_sc, w_log_mag, w_lin_mag, w_phs, sample_rate, scale,
                         n_bins, perceptual_weighting, scale_invariance, kwargs)

    def _init_multi(self, fft_sizes, hop_sizes, win_lengths, window, w_sc, w_log_mag, w_lin_mag, w_phs, sample_rate, scale,
                    n_bins, perceptual_weighting, scale_invariance, kwargs, w_sum=1.0, w_diff=1.0):
        if not len(fft_sizes) == len(hop_sizes) == len(win_lengths):
            raise ValueError("fft_sizes, hop_sizes and win_lengths must have the same length")
        if not 1 <= len(fft_sizes) <= MAX_RESOLUTIONS:
            raise NotImplementedError(f"the native STFT loss takes 1 to {MAX_RESOLUTIONS} resolutions; "
                                      f"got {len(fft_sizes)}")
        kwargs = dict(kwargs)
        eps = kwargs.pop("eps", 1e-8)
        prefilter = kwargs.pop("prefilter", None)
        kwargs.pop("device", None)  # (auraloss places its window tensors with it; the kernels build the window)
        _check_options(dict(window=window, w_phs=w_phs, scale_invariance=scale_invariance, **kwargs))
        self._setup(tuple(zip(fft_sizes, hop_sizes, win_lengths)), w_sc, w_log_mag, w_lin_mag, eps, sample_rate, scale,
                    n_bins, perceptual_weighting, prefilter, w_sum, w_diff)


class SumAndDifferenceSTFTLoss(MultiResolutionSTFTLoss):
    """(w_sum value(L + R) + w_diff value(L - R)) / 2 of the multi-resolution loss on stereo [B, 2, L] tensors
    (auraloss.freq.SumAndDifferenceSTFTLoss), in one native call: the sum and the difference are formed inside the kernels.
    `kwargs` are MultiResolutionSTFTLoss's."""
    pair = True

    def __init__(self, fft_sizes: Sequence[int] = (1024, 2048, 512), hop_sizes: Sequence[int] = (120, 240, 50),
                 win_lengths: Sequence[int] = (600, 1200, 240), window: str = "hann_window", w_sum: float = 1.0,
                 w_diff: float = 1.0, output: str = "loss", **kwargs):
        nn.Module.__init__(self)
        kw = dict(w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, w_phs=0.0, sample_rate=None, scale=None, n_bins=None,
                  perceptual_weighting=False, scale_invariance=False)
        kw.update({k: kwargs.pop(k) for k in list(kwargs) if k in kw})
        self._init_multi(fft_sizes, hop_sizes, win_lengths, window, kw["w_sc"], kw["w_log_mag"], kw["w_lin_mag"], kw["w_phs"],
                         kw["sample_rate"], kw["scale"], kw["n_bins"], kw["perceptual_weighting"], kw["scale_invariance"],
                         dict(kwargs, output=output), w_sum, w_diff)
