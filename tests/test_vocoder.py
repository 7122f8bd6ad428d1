"""The diffusion vocoder (audio_diffusion_pytorch_amd.vocoder): native mel spectrogram, `to_flat` (transposed convolution and
its weight gradient), the gradient of appended channels in the U-Net, and `DiffusionVocoder` end to end.

The oracle of the mel front end is the float64 restatement below (`mel_ref`): F.pad(reflect), torch.stft(center=False), the
HTK filterbank formula and a matmul.  torchaudio is not installed where this suite runs, so the restatement rests on
torchaudio's DOCUMENTED behaviour (transforms.Spectrogram / MelScale / functional.melscale_fbanks defaults), not on a run of
it.

Tolerances are measured against a yardstick, not guessed: the same restatement evaluated in float32 by CPU torch, against
float64, on the same input.  The native kernels get MARGIN = 4 times that (the factor tests/test_optim.py uses): the FFT
here forms W^2 and W^3 from float32 twiddles by complex products and so rounds more often than torch's.  No case needed a
wider margin (a widened one would have been capped at 1e-4, LOSS_TOL of tests/test_stft_loss.py, which covers the same FFT
code).  Measured error / yardstick ratios are listed next to MEL_CASES.  `to_flat` uses the same scheme against
F.conv_transpose1d.  normalize + normalize_log is ill-conditioned by construction (log of 2 r^(1/4) - 1 right above its
1e-5 clamp): its yardstick is 1e-4 .. 6e-4 on these inputs and the native error is a fraction of that.
"""
import copy
import ctypes
import io
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import audio_diffusion_pytorch_amd as adp
from audio_diffusion_pytorch_amd import _C, ops, vocoder
from audio_diffusion_pytorch_amd.components import _AppendChannelsNet
from conftest import rel_err
from oracle import vdiffusion as ovd
from oracle.a_unet_restatement import AppendChannelsOracle, UNetV0Oracle
from test_multistep_sampler import PARITY_TOL, multistep_ref
from test_unet import FixedSigmas, compare_grads

TOL = 1e-3       # the project's parity bound (tests/test_unet.py:12)
MARGIN = 4.0     # native error <= MARGIN x (float32 CPU torch error), as in tests/test_optim.py

# (n_fft, hop, win, sample_rate, n_mels, T): frames = T / hop, the flat length equals T, no filter is empty.
# Measured native error / yardstick on an MI355X for (plain, normalize_log, normalize, both), in the order below:
#   (0.09, 0.73, 0.30, 0.45), (0.18, 1.07, 0.48, 0.16), (0.26, 0.84, 0.48, 0.07), (0.36, 0.36, 0.32, 0.52); DESIGN.md section 6.
MEL_CASES = [(1024, 256, 1024, 48000, 80, 2 ** 15), (256, 64, 256, 16000, 32, 4096), (512, 128, 400, 22050, 40, 8192),
             (64, 16, 64, 8000, 8, 2048)]
MEL_OPTS = [dict(), dict(normalize_log=True), dict(normalize=True), dict(normalize=True, normalize_log=True)]


def fb_ref(n_fft, sample_rate, n_mels, dtype=torch.float64):
    """torchaudio.functional.melscale_fbanks(n_fft // 2 + 1, 0, sample_rate // 2, n_mels, sample_rate, norm=None, "htk")."""
    n_freqs = n_fft // 2 + 1
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=dtype)
    m_max = 2595.0 * math.log10(1.0 + (sample_rate // 2) / 700.0)
    m_pts = torch.linspace(0.0, m_max, n_mels + 2, dtype=dtype)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1, dtype=dtype), torch.min(down, up))


def mel_ref(x, n_fft, hop, win, sample_rate, n_mels, normalize=False, normalize_log=False, dtype=torch.float64):
    """The reference's MelSpectrogram.forward (components.py:218-236) restated on torch ops in `dtype`."""
    lead, T = x.shape[:-1], x.shape[-1]
    w = x.reshape(-1, T).to(dtype)
    pad = (n_fft - hop) // 2
    w = F.pad(w[:, None], [pad, pad], mode="reflect")[:, 0]
    spec = torch.stft(w, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, dtype=dtype), center=False,
                      onesided=True, normalized=False, return_complex=True).abs()         # [rows, n_freqs, frames]
    mel = torch.matmul(spec.transpose(-1, -2), fb_ref(n_fft, sample_rate, n_mels, dtype)).transpose(-1, -2)
    if normalize:
        mel = mel / torch.max(mel)
        mel = 2 * torch.pow(mel, 0.25) - 1
    if normalize_log:
        mel = torch.log(torch.clamp(mel, min=1e-5))
    return mel.reshape(*lead, n_mels, mel.shape[-1])


def wave(shape, seed):
    """A decaying-spectrum test signal (noise + a few tones), so that the mel bands differ by orders of magnitude."""
    g = torch.Generator().manual_seed(seed)
    T = shape[-1]
    t = torch.arange(T, dtype=torch.float64)
    x = 0.3 * torch.randn(shape, generator=g, dtype=torch.float64)
    for k, f in enumerate((0.011, 0.043, 0.17)):
        x = x + (0.8 / (k + 1)) * torch.sin(2 * math.pi * f * t + k)
    return x.to(torch.float32)


# ------------------------------------------------------------------ 1. mel against the restatement
@pytest.mark.parametrize("opts", MEL_OPTS, ids=["plain", "log", "norm", "norm+log"])
@pytest.mark.parametrize("case", MEL_CASES, ids=[f"fft{c[0]}" for c in MEL_CASES])
def test_mel_matches_restatement(dev, case, opts):
    n_fft, hop, win, sr, n_mels, T = case
    x = wave((2, 2, T), seed=n_fft)
    ref = mel_ref(x, n_fft, hop, win, sr, n_mels, **opts)
    yard = rel_err(mel_ref(x, n_fft, hop, win, sr, n_mels, dtype=torch.float32, **opts), ref)
    assert ref.shape == (2, 2, n_mels, T // hop)
    assert (fb_ref(n_fft, sr, n_mels).max(dim=0).values > 0).all(), "an empty filter"
    mel = vocoder.MelSpectrogram(n_fft, hop, win, sr, n_mels, **opts).to(dev)
    out = mel(x.to(dev))
    err = rel_err(out, ref)
    print(f"mel {case} {opts}: err {err:.3e} yardstick {yard:.3e} ratio {err / yard:.2f}")
    assert out.shape == ref.shape and out.dtype == torch.float32
    assert err <= MARGIN * yard, (err, yard)


def test_filterbank_is_the_documented_one():
    for n_fft, _, _, sr, n_mels, _ in MEL_CASES:
        fb = vocoder.mel_filterbank(n_fft, sr, n_mels)
        assert fb.dtype == torch.float64 and torch.equal(fb, fb_ref(n_fft, sr, n_mels))
        rng = vocoder._nonzero_ranges(fb.float())
        for m in range(n_mels):  # every nonzero entry of a column lies inside its range
            nz = torch.nonzero(fb.float()[:, m]).flatten()
            assert rng[m, 0] <= nz.min() and nz.max() < rng[m, 1]


def test_mel_dense_and_ranged_products_agree(dev):
    """The C-ABI contract is the dense product: without ranges every bin is visited, and the result is the same bits."""
    n_fft, hop, win, sr, n_mels, T = MEL_CASES[1]
    x = wave((3, T), seed=5).to(dev)
    mel = vocoder.MelSpectrogram(n_fft, hop, win, sr, n_mels).to(dev)
    a = ops.mel_spectrogram(x, mel.fb, mel.fb_range, n_fft, hop, win, False, False)
    b = ops.mel_spectrogram(x, mel.fb, None, n_fft, hop, win, False, False)
    assert torch.equal(a, b)


# ------------------------------------------------------------------ 2. silence
def test_mel_of_silence(dev):
    """A silent row with normalize_log gives exactly float32(log(1e-5)); an all-silent input with normalize returns -1
    everywhere (mel / max is taken as 0; the reference divides zero by zero and returns NaN), and log(1e-5) after the log."""
    n_fft, hop, win, sr, n_mels, T = MEL_CASES[3]
    x = wave((2, 2, T), seed=1)
    x[0, 1] = 0.0
    floor = torch.tensor(math.log(1e-5), dtype=torch.float32)   # log(1e-5) rounded to float32 once
    out = vocoder.MelSpectrogram(n_fft, hop, win, sr, n_mels, normalize_log=True).to(dev)(x.to(dev))
    assert torch.isfinite(out).all() and torch.equal(out[0, 1].cpu(), floor.expand_as(out[0, 1]))
    assert (out[0, 0] > floor.item()).any()
    z = torch.zeros(2, T).to(dev)
    out = vocoder.MelSpectrogram(n_fft, hop, win, sr, n_mels, normalize=True).to(dev)(z)
    assert torch.equal(out.cpu(), torch.full((2, n_mels, T // hop), -1.0))
    out = vocoder.MelSpectrogram(n_fft, hop, win, sr, n_mels, normalize=True, normalize_log=True).to(dev)(z)
    assert torch.equal(out.cpu(), floor.expand(2, n_mels, T // hop))


# ------------------------------------------------------------------ 3. determinism, errors, C-ABI
def test_mel_is_deterministic_and_checks_its_arguments(dev):
    n_fft, hop, win, sr, n_mels, T = MEL_CASES[2]
    x = wave((2, 2, T), seed=2).to(dev)
    mel = vocoder.MelSpectrogram(n_fft, hop, win, sr, n_mels, normalize=True, normalize_log=True).to(dev)
    assert torch.equal(mel(x), mel(x))
    with pytest.raises(RuntimeError, match="requires grad"):
        mel(x.clone().requires_grad_(True))
    with torch.no_grad():
        mel(x.clone().requires_grad_(True))  # (nothing is recorded: allowed)
    for bad in (1000, 8192, 32):
        with pytest.raises(NotImplementedError, match=str(bad)):
            vocoder.MelSpectrogram(bad, hop, win, sr, n_mels)
    with pytest.raises(NotImplementedError, match="center"):
        vocoder.MelSpectrogram(n_fft, hop, win, sr, n_mels, center=True)
    with pytest.raises(ValueError, match="exceed"):
        mel(x[..., :(n_fft - hop) // 2])
    assert mel(x[0, 0]).shape == (n_mels, T // hop)  # [..., T] -> [..., n_mels, frames]
    assert "fb" not in mel.state_dict()


def test_c_abi_mel_and_tflat_return_error_codes(dev):
    lib, s = _C.lib(), _C.stream()
    ERR_SHAPE, ERR_UNSUPPORTED, ERR_NULL = -1, -2, -5
    n_fft, hop, win, n_mels, T = 64, 16, 64, 8, 256
    x = torch.randn(2, T).to(dev)
    fb = torch.rand(n_fft // 2 + 1, n_mels).to(dev)
    out = torch.empty(2, n_mels, T // hop).to(dev)
    ws = torch.empty(64).to(dev)

    def mel(**kw):
        a = dict(x=x.data_ptr(), fb=fb.data_ptr(), rng=None, rows=2, T=T, n=n_fft, hop=hop, win=win, m=n_mels, norm=1, log=0,
                 out=out.data_ptr(), ws=ws.data_ptr())
        a.update(kw)
        return lib.adp_mel_spectrogram(*a.values(), s)

    assert mel() == 0
    for k in ("x", "fb", "out", "ws"):
        assert mel(**{k: None}) == ERR_NULL, k
    assert mel(ws=None, norm=0) == 0  # the workspace is needed with normalize only
    for kw in (dict(n=1000), dict(n=8192), dict(n=32), dict(hop=0), dict(hop=128), dict(win=0), dict(win=65)):
        assert mel(**kw) == ERR_UNSUPPORTED, kw
    for kw in (dict(rows=0), dict(T=0), dict(T=(n_fft - hop) // 2), dict(m=0)):
        assert mel(**kw) == ERR_SHAPE, kw
    assert lib.adp_mel_spectrogram_ws_bytes(2, T, 1000, hop, win, n_mels) == ERR_UNSUPPORTED
    assert lib.adp_mel_spectrogram_ws_bytes(2, T, n_fft, hop, win, n_mels) >= 4 * 2
    assert lib.adp_mel_frames(T, n_fft, hop) == T // hop
    assert _C.SIGNATURES["adp_mel_spectrogram"] == (ctypes.c_int, [_C.P] * 3 + [_C.I] * 8 + [_C.P] * 3)

    M, K, L = 8, 64, 16
    spec, w = torch.randn(2, M, L).to(dev), torch.randn(M, 1, K).to(dev)
    flat = torch.empty(2, 1, L * hop).to(dev)
    dw = torch.empty(M, 1, K).to(dev)
    ws = torch.empty(lib.adp_tflat_wgrad_ws_bytes(2, M, L, K, hop) // 4).to(dev)
    p = lambda t: t.data_ptr()  # noqa: E731
    assert lib.adp_tflat_out_len(L, K, hop) == L * hop
    assert lib.adp_tflat_fwd(p(spec), p(w), 2, M, L, K, hop, p(flat), s) == 0
    assert lib.adp_tflat_wgrad(p(spec), p(flat), 2, M, L, K, hop, p(dw), p(ws), s) == 0
    for k in range(2):
        a = [p(spec), p(w)]
        a[k] = None
        assert lib.adp_tflat_fwd(*a, 2, M, L, K, hop, p(flat), s) == ERR_NULL
        assert lib.adp_tflat_wgrad(*a, 2, M, L, K, hop, p(dw), p(ws), s) == ERR_NULL
    assert lib.adp_tflat_fwd(p(spec), p(w), 2, M, L, K, hop, None, s) == ERR_NULL
    assert lib.adp_tflat_wgrad(p(spec), p(flat), 2, M, L, K, hop, None, p(ws), s) == ERR_NULL
    assert lib.adp_tflat_wgrad(p(spec), p(flat), 2, M, L, K, hop, p(dw), None, s) == ERR_NULL
    for bad in (dict(N=0), dict(M=0), dict(L=0)):
        a = dict(N=2, M=M, L=L)
        a.update(bad)
        assert lib.adp_tflat_fwd(p(spec), p(w), a["N"], a["M"], a["L"], K, hop, p(flat), s) == ERR_SHAPE, bad
        assert lib.adp_tflat_wgrad_ws_bytes(a["N"], a["M"], a["L"], K, hop) == ERR_SHAPE, bad
    assert lib.adp_tflat_fwd(p(spec), p(w), 2, M, L, K, 0, p(flat), s) == ERR_UNSUPPORTED     # hop >= 1
    assert lib.adp_tflat_fwd(p(spec), p(w), 2, M, L, 8, hop, p(flat), s) == ERR_UNSUPPORTED   # K >= hop


# ------------------------------------------------------------------ 4. to_flat
TFLAT_CASES = [(80, 1024, 256, 12), (32, 256, 64, 40), (40, 400, 128, 33), (8, 64, 16, 130), (6, 24, 24, 50), (5, 7, 3, 45)]


@pytest.mark.parametrize("M,K,hop,L", TFLAT_CASES, ids=[f"M{c[0]}K{c[1]}h{c[2]}" for c in TFLAT_CASES])
def test_to_flat_forward_and_weight_gradient(dev, M, K, hop, L):
    """(M, K, hop) of the four mel cases, K = hop, and an odd geometry that takes the per-output path."""
    g = torch.Generator().manual_seed(M)
    N, pad = 3, (K - hop) // 2
    spec, w = torch.randn(N, M, L, generator=g), torch.randn(M, 1, K, generator=g) / math.sqrt(M)
    gout = torch.randn(N, 1, (L - 1) * hop - 2 * pad + K, generator=g)

    def torch_side(dtype):
        wd = w.to(dtype).requires_grad_(True)
        y = F.conv_transpose1d(spec.to(dtype), wd, stride=hop, padding=pad)
        y.backward(gout.to(dtype))
        return y.detach(), wd.grad

    (y64, dw64), (y32, dw32) = torch_side(torch.float64), torch_side(torch.float32)
    y = ops.tflat_fwd(spec.to(dev), w.to(dev), hop)
    dw = ops.tflat_wgrad(spec.to(dev), gout.to(dev), K, hop)   # (NaN-filled first under ADP_DEBUG_POISON=1: conftest.py)
    assert y.shape == y64.shape and dw.shape == dw64.shape
    assert torch.isfinite(dw).all(), "a slice of the weight gradient was not written"
    ey, yy = rel_err(y, y64), rel_err(y32, y64)
    ew, yw = rel_err(dw, dw64), rel_err(dw32, dw64)
    print(f"to_flat M{M} K{K} hop{hop}: fwd {ey:.3e} / yardstick {yy:.3e} = {ey / yy:.2f}; wgrad {ew:.3e} / {yw:.3e} = {ew / yw:.2f}")
    assert ey <= MARGIN * yy and ew <= MARGIN * yw
    assert torch.equal(dw, ops.tflat_wgrad(spec.to(dev), gout.to(dev), K, hop))
    # through the module: nn.ConvTranspose1d holds the weight, the kernels do the arithmetic
    conv = nn.ConvTranspose1d(M, 1, K, stride=hop, padding=pad, bias=False).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w)
    out = vocoder.to_flat(spec.to(dev), conv)
    out.backward(gout.to(dev))
    assert torch.equal(out.detach(), y) and torch.equal(conv.weight.grad, dw)
    with pytest.raises(RuntimeError, match="requires grad"):
        vocoder.to_flat(spec.to(dev).requires_grad_(True), conv)


# ------------------------------------------------------------------ 5. gradient of appended channels
def _append_pair(cfg, C, C2, dev, seed=0):
    torch.manual_seed(seed)
    oracle = AppendChannelsOracle(lambda **kw: UNetV0Oracle(**kw), channels=C2)(in_channels=C, **cfg)
    net = adp.AppendChannelsPlugin(adp.UNetV0, channels=C2)(in_channels=C, dim=1, **cfg)
    net.net.load_oracle_state_dict(oracle.net.state_dict())
    return oracle, net.to(dev)


@pytest.mark.parametrize("factor", [1, 2])
@pytest.mark.parametrize("ch0", [3, 8], ids=["ch0==in", "ch0!=in"])
def test_appended_channels_get_their_gradient(dev, factor, ch0):
    """x_append requires grad, x does not.  channels[0] equal to / different from the net's input channel count (2 + 1); the
    depth-0 skip adapter itself is present in both (the appended channel widens the input past out_channels)."""
    C, C2, T = 2, 1, 256
    cfg = dict(channels=[ch0, 16], factors=[factor, 2], items=[1, 1], modulation_features=32, resnet_groups=1 if ch0 == 3 else 8)
    if ch0 == 3:
        cfg["channels"] = [3, 15]
        cfg["resnet_groups"] = 3
    oracle, net = _append_pair(cfg, C, C2, dev)
    g = torch.Generator().manual_seed(4)
    x, app, tgt = (torch.randn(2, c, T, generator=g) for c in (C, C2, C))
    sig = torch.tensor([0.3, 0.8])
    app_ref = app.clone().requires_grad_(True)
    loss_ref = F.mse_loss(oracle(x, sig, append_channels=app_ref), tgt)
    loss_ref.backward()

    def run(two_pointer):
        net.zero_grad()
        net.two_pointer = two_pointer
        a = app.to(dev).requires_grad_(True)
        loss = F.mse_loss(net(x.to(dev), sig.to(dev), append_channels=a), tgt.to(dev))
        loss.backward()
        return loss, a.grad

    loss, ga = run(True)
    assert ga is not None and ga.shape == app.shape
    assert abs(loss.item() - loss_ref.item()) <= TOL * abs(loss_ref.item())
    assert rel_err(ga, app_ref.grad) <= TOL
    compare_grads(net.net, oracle.net)
    own = {n: p.grad.clone() for n, p in net.named_parameters()}
    loss_c, ga_c = run(False)  # this package's own _ConcatChannels path
    assert rel_err(ga, ga_c) <= TOL and abs(loss.item() - loss_c.item()) <= TOL * abs(loss_c.item())
    for n, p in net.named_parameters():
        assert rel_err(own[n], p.grad) <= TOL or p.grad.abs().max() < 1e-6, n


def test_appended_channels_without_grad_are_unchanged(dev):
    """An appended tensor that does not require grad: same results bit for bit between two runs, and its slot of the U-Net
    node's backward stays None (no extra launch on the DiffusionUpsampler path)."""
    from audio_diffusion_pytorch_amd import unet
    cfg = dict(channels=[8, 16], factors=[1, 2], items=[1, 1], modulation_features=32)
    _, net = _append_pair(cfg, 2, 2, dev)
    g = torch.Generator().manual_seed(4)
    x, app = torch.randn(2, 2, 256, generator=g).to(dev), torch.randn(2, 2, 256, generator=g).to(dev)
    sig = torch.tensor([0.3, 0.8]).to(dev)
    seen = []
    orig = unet._UNetFn.backward

    def spy(ctx, gy):
        out = orig(ctx, gy)
        seen.append(out[5])
        return out

    outs = []
    unet._UNetFn.backward = staticmethod(spy)
    try:
        for _ in range(2):
            net.zero_grad()
            y = net(x, sig, append_channels=app)
            y.square().mean().backward()
            outs.append((y.detach().clone(), [p.grad.clone() for p in net.parameters()]))
    finally:
        unet._UNetFn.backward = staticmethod(orig)
    assert seen == [None, None]
    assert torch.equal(outs[0][0], outs[1][0]) and all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))


# ------------------------------------------------------------------ 6. DiffusionVocoder end to end
VOC = dict(mel_channels=8, mel_n_fft=64, mel_sample_rate=8000, channels=[8, 16], factors=[1, 2], items=[1, 1],
           modulation_features=32)
NET_KEYS = ("channels", "factors", "items", "modulation_features")


def _vocoder_pair(dev, sig=None, seed=0, **kw):
    torch.manual_seed(seed)
    cfg = dict(VOC, **kw)
    oracle = AppendChannelsOracle(lambda **k: UNetV0Oracle(**k), channels=1)(in_channels=1, **{k: cfg[k] for k in NET_KEYS})
    extra = dict(diffusion_sigma_distribution=FixedSigmas(sig)) if sig is not None else {}
    model = vocoder.DiffusionVocoder(net_t=adp.UNetV0, **extra, **cfg)
    model.net.net.load_oracle_state_dict(oracle.net.state_dict())
    n_fft = cfg["mel_n_fft"]
    hop, win = cfg.get("mel_hop_length") or n_fft // 4, cfg.get("mel_win_length") or n_fft
    flat64 = nn.ConvTranspose1d(cfg["mel_channels"], 1, win, stride=hop, padding=(win - hop) // 2, bias=False).double()
    with torch.no_grad():
        flat64.weight.copy_(model.to_flat.weight)
    return oracle, flat64, model.to(dev)


@pytest.mark.parametrize("log", [False, True], ids=["plain", "normalize_log"])
def test_vocoder_training_step_matches_composed_oracle(dev, log):
    B, C, T = 2, 2, 512
    sig = [0.2, 0.5, 0.7, 0.9]
    oracle, flat64, model = _vocoder_pair(dev, sig, mel_normalize_log=log)
    g = torch.Generator().manual_seed(9)
    x, noise = wave((B, C, T), seed=3), torch.randn(B * C, 1, T, generator=g)
    mel = mel_ref(x, 64, 16, 64, 8000, 8, normalize_log=log).reshape(B * C, 8, T // 16)
    flat = flat64(mel)
    loss_ref = ovd.v_loss(oracle.double(), x.reshape(B * C, 1, T).double(), noise.double(), torch.tensor(sig, dtype=torch.float64),
                          append_channels=flat)
    loss_ref.backward()
    loss = model(x.to(dev), noise=noise.to(dev))
    loss.backward()
    assert abs(loss.item() - loss_ref.item()) <= TOL * abs(loss_ref.item())
    assert rel_err(model.to_flat.weight.grad, flat64.weight.grad) <= TOL
    compare_grads(model.net.net, oracle.net)
    names = [n for n, _ in model.named_parameters()]
    assert names.count("to_flat.weight") + names.count("net.to_flat.weight") == 1   # yielded once
    sd = model.state_dict()
    assert "to_flat.weight" in sd and sd["to_flat.weight"].shape == (8, 1, 64)
    assert model.to_flat is model.net.to_flat and isinstance(model.to_flat, nn.ConvTranspose1d)


# ------------------------------------------------------------------ 7. sample()
def test_vocoder_sample(dev):
    oracle, flat64, model = _vocoder_pair(dev)
    B, C, Fm, L = 2, 2, 8, 32
    g = torch.Generator().manual_seed(2)
    spec = torch.rand(B, C, Fm, L, generator=g)
    out = model.sample(spec.to(dev), num_steps=3, generator=torch.Generator().manual_seed(11))
    assert out.shape == (B, C, L * 16)
    again = model.sample(spec.to(dev), num_steps=3, generator=torch.Generator().manual_seed(11))
    assert torch.equal(out, again)
    assert model.sample(spec[0, 0].to(dev), num_steps=2).shape == (L * 16,)
    start = torch.randn(B * C, 1, L * 16, generator=torch.Generator().manual_seed(11))   # models._start_noise: host draw
    with torch.no_grad():
        flat = flat64(spec.reshape(B * C, Fm, L).double())
    ref = ovd.v_sample(oracle.double(), start.double(), 3, append_channels=flat)
    assert rel_err(out.reshape(B * C, 1, -1), ref) <= TOL
    # second-order sampler: against the float64 restatement of tests/test_multistep_sampler.py at that file's tolerance
    torch.manual_seed(0)
    multi = vocoder.DiffusionVocoder(net_t=adp.UNetV0, sampler_t=adp.VMultistepSampler, **VOC)
    multi.load_state_dict(model.state_dict())
    multi = multi.to(dev)
    assert type(multi.sampler) is adp.VMultistepSampler
    out2 = multi.sample(spec.to(dev), num_steps=6, generator=torch.Generator().manual_seed(11))
    ref2 = multistep_ref(oracle, start.double(), 6, append_channels=flat)
    assert out2.shape == (B, C, L * 16) and rel_err(out2.reshape(B * C, 1, -1), ref2) <= PARITY_TOL


# ------------------------------------------------------------------ 8. GPU only: replayed steps, copies, the README shape
def _grads(model):
    return {n: p.grad.clone() for n, p in model.named_parameters()}


@pytest.mark.gpu
def test_vocoder_training_step_replays_and_equals_eager(hip):
    _, _, m_g = _vocoder_pair(hip, mel_normalize_log=True)
    _, _, m_e = _vocoder_pair(hip, mel_normalize_log=True, diffusion_use_graph=False)
    g = torch.Generator().manual_seed(5)
    for step in range(5):
        x = wave((2, 2, 512), seed=20 + step).to(hip)
        noise = torch.randn(4, 1, 512, generator=g).to(hip)
        losses = []
        for m in (m_g, m_e):
            m.zero_grad()
            torch.manual_seed(100 + step)  # the sigma draw
            loss = m(x, noise=noise)
            loss.backward()
            losses.append(loss.detach().clone())
        assert torch.equal(losses[0], losses[1]), step
        ge, gg = _grads(m_e), _grads(m_g)
        # (named_parameters() names the shared module by its first registration, under the net)
        assert "net.to_flat.weight" in gg and gg["net.to_flat.weight"].abs().max() > 0
        assert torch.equal(m_g.to_flat.weight.grad, m_e.to_flat.weight.grad)
        for n in ge:
            assert torch.equal(gg[n], ge[n]), (step, n)
    assert m_g.diffusion.train_graphs().captures == 1 and m_g.diffusion.train_graphs().replays == 5
    assert m_e.diffusion.train_graphs().captures == 0
    # EMA copy / checkpoint after a capture
    cp = copy.deepcopy(m_g)
    torch.save(m_g, io.BytesIO())
    assert cp.to_flat is cp.net.to_flat and cp.to_flat is not m_g.to_flat
    x = wave((2, 2, 512), seed=40).to(hip)
    cp.zero_grad()
    loss = cp(x)
    loss.backward()
    assert torch.isfinite(loss) and cp.to_flat.weight.grad is not None
    spec = cp.to_spectrogram(x)
    out = cp.sample(spec, num_steps=3, generator=torch.Generator().manual_seed(1))
    assert out.shape == (2, 2, 512) and torch.isfinite(out).all()
    assert torch.equal(out, m_g.sample(spec, num_steps=3, generator=torch.Generator().manual_seed(1)))


@pytest.mark.gpu
def test_readme_vocoder_configuration_runs(hip):
    import time
    t0 = time.time()
    torch.manual_seed(0)
    model = vocoder.DiffusionVocoder(
        mel_n_fft=1024, mel_channels=80, mel_sample_rate=48000, mel_normalize_log=True, net_t=adp.UNetV0,
        channels=[8, 32, 64, 256, 256, 512, 512, 1024, 1024], factors=[1, 4, 4, 4, 2, 2, 2, 2, 2],
        items=[1, 2, 2, 2, 2, 2, 2, 4, 4]).to(hip)
    audio = wave((1, 2, 2 ** 18), seed=8).to(hip)
    loss = model(audio)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(model.to_flat.weight.grad).all()
    assert model.to_flat.weight.grad.abs().max() > 0
    spec = model.to_spectrogram(audio)
    assert spec.shape == (1, 2, 80, 1024)
    out = model.sample(spec, num_steps=3)
    torch.cuda.synchronize()
    assert out.shape == (1, 2, 2 ** 18) and torch.isfinite(out).all()
    assert time.time() - t0 < 300, "the README vocoder example took more than five minutes"


# ------------------------------------------------------------------ 9. argument errors
def test_vocoder_argument_errors(dev):
    _, _, model = _vocoder_pair(dev)
    with pytest.raises(ValueError, match="mel_hop_length"):
        model(torch.randn(1, 1, 500).to(dev))            # 500 % 16 != 0
    with pytest.raises(TypeError, match="sample_rate"):
        vocoder.DiffusionVocoder(net_t=adp.UNetV0, **{k: v for k, v in VOC.items() if k != "mel_sample_rate"})
    odd = vocoder.DiffusionVocoder(net_t=adp.UNetV0, mel_hop_length=16, mel_win_length=33, **VOC).to(dev)
    with pytest.raises(ValueError, match="mel_win_length - mel_hop_length"):
        odd(torch.randn(1, 1, 512).to(dev))
    with pytest.raises(NotImplementedError, match="vocoder"):   # the top-level names still are the stubs and point here
        adp.DiffusionVocoder(net_t=None)
