"""Diffusion vocoder (mel spectrogram -> waveform) on the gfx950 kernels: `MelSpectrogram` and `DiffusionVocoder`,
API-compatible with /root/reference/audio_diffusion_pytorch/components.py:188-236 and models.py:168-224.

    from audio_diffusion_pytorch_amd.vocoder import DiffusionVocoder, MelSpectrogram

(The package's top-level names `DiffusionVocoder` / `MelSpectrogram` still are the out-of-scope stubs that the test-suite
pins; they point here.  DESIGN.md section 7.)

Mel front end (`adp_mel_spectrogram`, csrc/resample.hip), the reference's forward with torchaudio's documented defaults:

    pad   = (n_fft - hop) // 2, reflect, both sides
    X     = stft(padded, n_fft, hop, win, periodic hann(win) zero-padded and centred in n_fft, center=False, onesided)
    mel   = fb^T |X|,  fb = [n_fft // 2 + 1, n_mels]: HTK scale, f_min 0, f_max sample_rate // 2, norm None, bin
            frequencies linspace(0, sample_rate // 2, n_fft // 2 + 1), triangles max(0, min(down, up))
    normalize:      mel = 2 * (mel / max(mel over the whole tensor)) ** 0.25 - 1
    normalize_log:  mel = log(max(mel, 1e-5))        (after normalize, as in the reference)

The filterbank is built on the host in float64, rounded once to float32 and held as a module buffer together with the bin
range of every triangle (the kernel visits only those bins; the skipped terms are exact zeros).  The maximum of `normalize`
is found on the device: the call has no host synchronisation and no host-to-device copy.  An all-silent input with
`normalize=True` returns -1 everywhere (mel / max is taken as 0 where the reference divides zero by zero and returns NaN).
The input is not differentiated.

`to_flat` is a plain `nn.ConvTranspose1d` (reference initialisation and state-dict key); its arithmetic runs on
`adp_tflat_fwd` / `adp_tflat_wgrad`.  In training it is evaluated INSIDE the net call (`_VocoderNet`), so that the
captured training step (graphed.py) holds mel -> flat + the U-Net in its forward graph and the weight gradient in its
backward graph, and the mel tensor reaches the diffusion as a plain keyword tensor that does not require grad.
"""
from contextlib import nullcontext
from math import log10
from typing import Callable, Optional

import torch
import torch.nn as nn
from torch import Generator, Tensor

from . import ops
from .components import _AppendChannelsNet
from .models import DiffusionModel, _split_prefixed, _start_noise


def mel_filterbank(n_fft: int, sample_rate: int, n_mels: int) -> Tensor:
    """float64 [n_fft // 2 + 1, n_mels]: torchaudio.functional.melscale_fbanks(n_freqs, 0, sample_rate // 2, n_mels,
    sample_rate, norm=None, mel_scale="htk") as documented."""
    n_freqs = n_fft // 2 + 1
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=torch.float64)
    m_min = 2595.0 * log10(1.0 + 0.0 / 700.0)
    m_max = 2595.0 * log10(1.0 + float(sample_rate // 2) / 700.0)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2, dtype=torch.float64)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.minimum(down, up), min=0.0)


def _nonzero_ranges(fb: Tensor) -> Tensor:
    """int32 [n_mels, 2]: per column of fb the bins [lo, hi) that hold every nonzero entry ([0, 0) for an empty filter)."""
    nz = fb != 0
    n_freqs = fb.shape[0]
    idx = torch.arange(n_freqs)[:, None]
    lo = torch.where(nz, idx, n_freqs).min(dim=0).values
    hi = torch.where(nz, idx + 1, 0).max(dim=0).values
    lo = torch.minimum(lo, hi)
    return torch.stack([lo, hi], dim=1).to(torch.int32).contiguous()


class MelSpectrogram(nn.Module):
    """[..., T] float32 -> [..., n_mel_channels, frames] (components.py:188-236), frames = 1 + (T + 2 pad - n_fft) // hop."""

    def __init__(self, n_fft: int, hop_length: int, win_length: int, sample_rate: int, n_mel_channels: int,
                 center: bool = False, normalize: bool = False, normalize_log: bool = False):
        super().__init__()
        n_fft, hop_length, win_length = int(n_fft), int(hop_length), int(win_length)
        if n_fft < 64 or n_fft > 4096 or n_fft & (n_fft - 1):
            raise NotImplementedError(f"n_fft={n_fft}: the native mel spectrogram supports powers of two in [64, 4096]")
        if center:
            raise NotImplementedError("center=True is not supported by the native mel spectrogram (only center=False, "
                                      "the reference's default)")
        if hop_length < 1 or hop_length > n_fft:
            raise ValueError(f"hop_length={hop_length} must be in [1, n_fft={n_fft}]")
        if win_length < 1 or win_length > n_fft:
            raise ValueError(f"win_length={win_length} must be in [1, n_fft={n_fft}]")
        if int(n_mel_channels) < 1:
            raise ValueError(f"n_mel_channels={n_mel_channels} must be at least 1")
        self.n_fft, self.hop_length, self.win_length = n_fft, hop_length, win_length
        self.sample_rate, self.n_mel_channels = int(sample_rate), int(n_mel_channels)
        self.padding = (n_fft - hop_length) // 2
        self.normalize = bool(normalize)
        self.normalize_log = bool(normalize_log)
        fb = mel_filterbank(n_fft, self.sample_rate, self.n_mel_channels).to(torch.float32).contiguous()
        # (derived from the constructor arguments: not part of the state dict)
        self.register_buffer("fb", fb, persistent=False)
        self.register_buffer("fb_range", _nonzero_ranges(fb), persistent=False)

    def num_frames(self, length: int) -> int:
        return 1 + (length + 2 * self.padding - self.n_fft) // self.hop_length

    def forward(self, waveform: Tensor) -> Tensor:
        if waveform.dtype != torch.float32:
            raise TypeError(f"the native mel spectrogram takes float32 waveforms; got {waveform.dtype}")
        if waveform.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("the native mel spectrogram does not differentiate its input; the waveform requires grad "
                               "(pass waveform.detach())")
        T = waveform.shape[-1]
        if T <= self.padding:
            raise ValueError(f"waveform length {T} must exceed the reflect padding (n_fft - hop_length) // 2 = {self.padding}")
        if self.fb.device != waveform.device:
            raise RuntimeError(f"MelSpectrogram lives on {self.fb.device}, the waveform on {waveform.device}; move the "
                               "module with .to(device)")
        rows = waveform.reshape(-1, T).contiguous()
        with torch.cuda.device(waveform.device) if waveform.is_cuda else nullcontext():
            mel = ops.mel_spectrogram(rows, self.fb, self.fb_range, self.n_fft, self.hop_length, self.win_length,
                                      self.normalize, self.normalize_log)
        return mel.view(*waveform.shape[:-1], mel.shape[1], mel.shape[2])


class _ToFlatFn(torch.autograd.Function):
    """ConvTranspose1d(M, 1, K, stride=hop, padding=(K - hop) // 2, bias=False) on adp_tflat_fwd; weight gradient on
    adp_tflat_wgrad; the spectrogram gets none."""

    @staticmethod
    def forward(ctx, spec: Tensor, weight: Tensor, hop: int) -> Tensor:
        ctx.save_for_backward(spec)
        ctx.K, ctx.hop = weight.shape[2], hop
        return ops.tflat_fwd(spec, weight.contiguous(), hop)

    @staticmethod
    def backward(ctx, g: Tensor):
        (spec,) = ctx.saved_tensors
        dw = ops.tflat_wgrad(spec, g.contiguous(), ctx.K, ctx.hop) if ctx.needs_input_grad[1] else None
        return None, dw, None


def to_flat(spec: Tensor, conv: nn.ConvTranspose1d) -> Tensor:
    """conv(spec) for the vocoder's `to_flat` module ([N, M, L] -> [N, 1, (L - 1) hop - 2 pad + K]) on the native kernels."""
    if spec.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("to_flat does not differentiate the spectrogram (it comes from data); it requires grad "
                           "(pass spectrogram.detach())")
    if spec.dim() != 3 or spec.shape[1] != conv.in_channels:
        raise ValueError(f"spectrogram must be [N, {conv.in_channels}, L]; got {tuple(spec.shape)}")
    if spec.dtype != torch.float32:
        raise TypeError(f"to_flat takes a float32 spectrogram; got {spec.dtype}")
    K, hop = conv.kernel_size[0], conv.stride[0]
    assert conv.out_channels == 1 and conv.bias is None and conv.padding[0] == (K - hop) // 2 and \
        conv.output_padding[0] == 0 and conv.dilation[0] == 1 and conv.groups == 1, "not the vocoder's to_flat geometry"
    with torch.cuda.device(spec.device) if spec.is_cuda else nullcontext():
        return _ToFlatFn.apply(spec.contiguous(), conv.weight, hop)


class _VocoderNet(_AppendChannelsNet):
    """AppendChannelsPlugin(net_t, channels=1)(...) that also owns `to_flat`: forward takes either `spectrogram`
    ([N, mel_channels, L], flattened here, inside the net call and so inside the captured step) or a ready
    `append_channels` (the sampler: flattened once per sampling run)."""

    def __init__(self, net: nn.Module, to_flat_conv: nn.ConvTranspose1d):
        super().__init__(net)
        self.to_flat = to_flat_conv

    def forward(self, x: Tensor, *args, spectrogram: Optional[Tensor] = None, append_channels: Optional[Tensor] = None,
                **kwargs) -> Tensor:
        if (spectrogram is None) == (append_channels is None):
            raise TypeError("the vocoder net takes exactly one of `spectrogram` and `append_channels`")
        if append_channels is None:
            append_channels = to_flat(spectrogram, self.to_flat)
        return super().forward(x, *args, append_channels=append_channels, **kwargs)


class DiffusionVocoder(DiffusionModel):
    """Mel spectrogram -> waveform by diffusion (models.py:168-224): every wave channel is a batch row of a one-channel
    U-Net conditioned on `to_flat(mel)` as an appended input channel."""

    def __init__(self, net_t: Callable, mel_channels: int, mel_n_fft: int, mel_hop_length: Optional[int] = None,
                 mel_win_length: Optional[int] = None, in_channels: int = 1, **kwargs):
        # (`in_channels` is ignored as in the reference: channels are batched)
        hop = int(mel_hop_length) if mel_hop_length is not None else int(mel_n_fft) // 4
        win = int(mel_win_length) if mel_win_length is not None else int(mel_n_fft)
        routed, kwargs = _split_prefixed(kwargs, "mel_")
        if hop < 1 or win < hop:
            raise ValueError(f"mel_win_length={win} must be at least mel_hop_length={hop} >= 1 (to_flat's padding "
                             "(win - hop) // 2)")

        def vocoder_net(in_channels: int, out_channels: Optional[int] = None, **net_kwargs) -> nn.Module:
            out_channels = in_channels if out_channels is None else out_channels
            net = net_t(in_channels=in_channels + 1, out_channels=out_channels, **net_kwargs)
            conv = nn.ConvTranspose1d(in_channels=mel_channels, out_channels=1, kernel_size=win, stride=hop,
                                      padding=(win - hop) // 2, bias=False)
            return _VocoderNet(net, conv)

        super().__init__(net_t=vocoder_net, in_channels=1, **kwargs)
        self.to_spectrogram = MelSpectrogram(n_fft=mel_n_fft, hop_length=hop, win_length=win,
                                             n_mel_channels=mel_channels, **routed["mel_"])
        self.to_flat = self.net.to_flat  # the reference's attribute and state-dict key; ONE module, shared with the net

    def _check_flat_length(self, T: int) -> None:
        mel = self.to_spectrogram
        hop, win = mel.hop_length, mel.win_length
        if T % hop != 0:
            raise ValueError(f"waveform length {T} is not a multiple of mel_hop_length={hop}: to_flat(mel) would not have "
                             f"the waveform's length")
        frames = mel.num_frames(T)
        flat = (frames - 1) * hop - 2 * ((win - hop) // 2) + win
        if flat != T:
            odd = [f"mel_n_fft - mel_hop_length = {mel.n_fft - hop}"] if (mel.n_fft - hop) % 2 else []
            odd += [f"mel_win_length - mel_hop_length = {win - hop}"] if (win - hop) % 2 else []
            raise ValueError(f"to_flat(mel) has length {flat}, the waveform {T}: " + (" and ".join(odd) + " must be even"
                             if odd else f"mel_n_fft={mel.n_fft}, mel_hop_length={hop}, mel_win_length={win} do not tile it"))

    def forward(self, x: Tensor, *args, **kwargs) -> Tensor:
        if x.dim() != 3:
            raise ValueError(f"DiffusionVocoder.forward takes [batch, channels, length]; got {tuple(x.shape)}")
        B, C, T = x.shape
        self._check_flat_length(T)
        mel = self.to_spectrogram(x)                                        # [B, C, F, L]
        spectrogram = mel.view(B * C, mel.shape[2], mel.shape[3])           # "b c f l -> (b c) f l"
        return super().forward(x.reshape(B * C, 1, T), *args, spectrogram=spectrogram, **kwargs)

    @torch.no_grad()
    def sample(self, spectrogram: Tensor, generator: Optional[Generator] = None, **kwargs) -> Tensor:
        if spectrogram.dim() < 2:
            raise ValueError(f"DiffusionVocoder.sample takes [..., mel_channels, frames]; got {tuple(spectrogram.shape)}")
        lead = spectrogram.shape[:-2]
        packed = spectrogram.reshape(-1, spectrogram.shape[-2], spectrogram.shape[-1])  # "* f l"
        flat = to_flat(packed, self.to_flat)
        noise = _start_noise(flat.shape, flat, generator)
        wave = super().sample(noise, append_channels=flat, **kwargs)        # [N, 1, T]
        return wave.reshape(*lead, wave.shape[-1])
