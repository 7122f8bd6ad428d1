"""The mel encoder (audio_diffusion_pytorch_amd/encoders.py) and its kernels (csrc/encoder.hip, include/adp_enc.h).

Kernel parity: the overlapping strided downsample conv (forward, data gradient, weight and bias gradient) and the tanh pair
against float64 torch on the CPU, outputs pre-filled with NaN, bound 1e-4 (the single-kernel bound of tests/test_kernels.py).
Module parity: the whole encoder, its variants and DiffusionAE end to end against the torch.nn composition of the module's
own submodules, bound 1e-3 (the module bound of tests/test_unet.py).  Every test runs on the SIMT emulator and, with -m gpu,
on the gfx950 library."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import audio_diffusion_pytorch_amd as adp
from audio_diffusion_pytorch_amd import _C, ops
from audio_diffusion_pytorch_amd.encoders import MelE1d, TanhBottleneck
from conftest import rel_err

TOL = 1e-4       # single kernels
TOL_MODULE = 1e-3

# (B, R, M, L, f): everything odd; exactly one MFMA tile; channel and length tails past a tile; tiny; N = 1 (only taps
# f .. 2f inside); and SPLIT, one batch row whose 70 output frames the split rule (about 512 workgroups over tiles x
# segments of whole 32-frame chunks) cuts into 3 segments: the reduction crosses partials inside a batch row
SPLIT = (1, 4, 8, 140, 2)
SHAPES = [(2, 5, 7, 37, 2), (1, 32, 32, 64, 2), (2, 40, 72, 130, 4), (1, 3, 2, 10, 3), (1, 4, 4, 1, 2), SPLIT]
GEOMS = {"vec16": (2, 8, 8, 64, 4), "odd": (2, 5, 7, 37, 3)}   # tests/test_encoder_placement.py


@functools.lru_cache(maxsize=None)
def case(shape):
    """Inputs and float64 references of one downsample geometry (CPU tensors, computed once, never modified), and of the
    tanh pair on the same data."""
    if isinstance(shape, str):
        shape = GEOMS[shape]
    B, R, M, L, f = shape
    g = torch.Generator().manual_seed(1000 * L + 10 * R + f)
    x = torch.randn(B, R, L, generator=g)
    w = torch.randn(M, R, 2 * f + 1, generator=g) / (R * (2 * f + 1)) ** 0.5
    bias = torch.randn(M, generator=g)
    xd = x.double().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    y = F.conv1d(xd, wd, bd, stride=f, padding=f)
    N = (L - 1) // f + 1
    assert y.shape == (B, M, N)
    dy = torch.randn(B, M, N, generator=g)
    dx, dw, dbias = torch.autograd.grad(y, (xd, wd, bd), dy.double())
    hd = x.double().reshape(-1)
    dz = torch.randn(hd.numel(), generator=g)
    zd = torch.tanh(hd)
    return dict(B=B, R=R, M=M, L=L, N=N, f=f, x=x, w=w, bias=bias, dy=dy, y=y.detach(), dx=dx, dw=dw, dbias=dbias,
                h=x.reshape(-1), z=zd, zf=zd.float(), dz=dz, dh=dz.double() * (1 - zd.float().double() ** 2))


def nan_like(shape, dev):
    return torch.full(tuple(shape), float("nan"), dtype=torch.float32, device=dev)


def p(t):
    return _C.ptr(t)


def check(name, got, want):
    assert torch.isfinite(got).all(), f"{name}: an element was left unwritten (NaN pre-fill) or is not finite"
    err = rel_err(got, want)
    print(f"{name}: rel err {err:.3e} (bound {TOL:.0e})")
    assert err < TOL, (name, err)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B{}R{}M{}L{}f{}".format(*s))
def test_down_conv_kernels(dev, shape):
    d = case(shape)
    B, R, M, L, N, f = (d[k] for k in "BRMLNf")
    lib, s = _C.lib(), _C.stream()
    x, w, bias, dy = (d[k].to(dev) for k in ("x", "w", "bias", "dy"))
    assert lib.adp_enc_down_out_len(L, f) == N
    y = nan_like((B, M, N), dev)
    assert lib.adp_enc_down_fwd(p(x), p(w), p(bias), B, R, M, L, f, p(y), s) == 0
    check("down_fwd", y, d["y"])
    dx = nan_like((B, R, L), dev)
    assert lib.adp_enc_down_dgrad(p(dy), p(w), B, R, M, L, f, p(dx), s) == 0
    check("down_dgrad", dx, d["dx"])
    nbytes = lib.adp_enc_down_wgrad_ws_bytes(B, R, M, L, f)
    per = M * R * (2 * f + 1) * 4
    assert nbytes > 0 and nbytes % per == 0
    if shape == SPLIT:
        assert nbytes // per == 3, "the split rule no longer cuts this shape into 3 partials: choose another shape"
    runs = []
    for _ in range(2):
        dw, dbias, ws = nan_like((M, R, 2 * f + 1), dev), nan_like((M,), dev), nan_like((nbytes // 4,), dev)
        assert lib.adp_enc_down_wgrad(p(x), p(dy), B, R, M, L, f, p(dw), p(dbias), p(ws), s) == 0
        runs.append((dw, dbias))
    check("down_wgrad dw", runs[0][0], d["dw"])
    check("down_wgrad dbias", runs[0][1], d["dbias"])
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "weight gradient not bit-identical"


def test_down_conv_ops_wrappers(dev):
    """The ops.py wrappers marshal the same calls (and NaN-fill what they allocate under ADP_DEBUG_POISON)."""
    d = case(SHAPES[0])
    x, w, bias, dy = (d[k].to(dev) for k in ("x", "w", "bias", "dy"))
    check("ops.enc_down_fwd", ops.enc_down_fwd(x, w, bias, d["f"]), d["y"])
    check("ops.enc_down_dgrad", ops.enc_down_dgrad(dy, w, d["f"], d["L"]), d["dx"])
    dw, dbias = ops.enc_down_wgrad(x, dy, d["f"])
    check("ops.enc_down_wgrad dw", dw, d["dw"])
    check("ops.enc_down_wgrad dbias", dbias, d["dbias"])


@pytest.mark.parametrize("numel", [1, 5, 4099])
def test_tanh_kernels(dev, numel):
    """On an offset-by-one view (the scalar path) and on the aligned tensor itself (16-byte accesses + scalar tail)."""
    g = torch.Generator().manual_seed(numel)
    h, dz = 3 * torch.randn(numel, generator=g), torch.randn(numel, generator=g)
    z_ref = torch.tanh(h.double())
    for off in (1, 0):
        hb, gb = torch.zeros(numel + 4), torch.zeros(numel + 4)
        hb[off:off + numel], gb[off:off + numel] = h, dz
        hv, gv = hb.to(dev)[off:off + numel], gb.to(dev)[off:off + numel]
        assert (hv.data_ptr() % 16 == 0) == (off == 0)
        zb, db = nan_like((numel + 4,), dev), nan_like((numel + 4,), dev)
        z = ops.enc_tanh_fwd(hv)
        check(f"tanh_fwd n{numel} off{off}", z, z_ref)
        assert _C.lib().adp_enc_tanh_fwd(p(hv), numel, p(zb[off:off + numel]), _C.stream()) == 0
        assert torch.equal(zb[off:off + numel], z) and torch.isnan(zb[:off]).all() and torch.isnan(zb[off + numel:]).all()
        assert _C.lib().adp_enc_tanh_bwd(p(zb[off:off + numel]), p(gv), numel, p(db[off:off + numel]), _C.stream()) == 0
        check(f"tanh_bwd n{numel} off{off}", db[off:off + numel], dz.double() * (1 - z.double().cpu() ** 2))
        assert torch.isnan(db[:off]).all() and torch.isnan(db[off + numel:]).all()
        assert torch.equal(ops.enc_tanh_bwd(z, gv), db[off:off + numel])


def test_error_codes(dev):
    d = case(SHAPES[0])
    B, R, M, L, N, f = (d[k] for k in "BRMLNf")
    lib, s = _C.lib(), _C.stream()
    x, w, bias, dy = (d[k].to(dev) for k in ("x", "w", "bias", "dy"))
    y, dx, dw, dbias = nan_like((B, M, N), dev), nan_like((B, R, L), dev), nan_like((M, R, 2 * f + 1), dev), nan_like((M,), dev)
    ws = nan_like((lib.adp_enc_down_wgrad_ws_bytes(B, R, M, L, f) // 4,), dev)
    NULL, SHAPE, UNSUPPORTED = -5, -1, -2
    fwd = lambda *a: lib.adp_enc_down_fwd(*a, s)
    assert fwd(None, p(w), p(bias), B, R, M, L, f, p(y)) == NULL
    assert fwd(p(x), None, p(bias), B, R, M, L, f, p(y)) == NULL
    assert fwd(p(x), p(w), None, B, R, M, L, f, p(y)) == NULL
    assert fwd(p(x), p(w), p(bias), B, R, M, L, f, None) == NULL
    for bad in ((0, R, M, L), (B, 0, M, L), (B, R, 0, L), (B, R, M, 0), (B, R, M, -3)):
        assert fwd(p(x), p(w), p(bias), *bad, f, p(y)) == SHAPE
        assert lib.adp_enc_down_dgrad(p(dy), p(w), *bad, f, p(dx), s) == SHAPE
        assert lib.adp_enc_down_wgrad(p(x), p(dy), *bad, f, p(dw), p(dbias), p(ws), s) == SHAPE
        assert lib.adp_enc_down_wgrad_ws_bytes(*bad, f) == SHAPE
    for bad_f in (5, 1, 0):
        assert fwd(p(x), p(w), p(bias), B, R, M, L, bad_f, p(y)) == UNSUPPORTED
        assert lib.adp_enc_down_dgrad(p(dy), p(w), B, R, M, L, bad_f, p(dx), s) == UNSUPPORTED
        assert lib.adp_enc_down_wgrad(p(x), p(dy), B, R, M, L, bad_f, p(dw), p(dbias), p(ws), s) == UNSUPPORTED
        assert lib.adp_enc_down_wgrad_ws_bytes(B, R, M, L, bad_f) == UNSUPPORTED
        assert lib.adp_enc_down_out_len(L, bad_f) == UNSUPPORTED
    assert lib.adp_enc_down_out_len(0, 2) == SHAPE
    assert lib.adp_enc_down_dgrad(None, p(w), B, R, M, L, f, p(dx), s) == NULL
    assert lib.adp_enc_down_dgrad(p(dy), p(w), B, R, M, L, f, None, s) == NULL
    assert lib.adp_enc_down_wgrad(p(x), p(dy), B, R, M, L, f, p(dw), None, p(ws), s) == NULL
    assert lib.adp_enc_down_wgrad(p(x), p(dy), B, R, M, L, f, p(dw), p(dbias), None, s) == NULL
    assert lib.adp_enc_tanh_fwd(None, 4, p(y), s) == NULL and lib.adp_enc_tanh_fwd(p(x), 0, p(y), s) == SHAPE
    assert lib.adp_enc_tanh_bwd(p(x), None, 4, p(y), s) == NULL and lib.adp_enc_tanh_bwd(p(x), p(x), 0, p(y), s) == SHAPE
    # a refused call writes nothing
    for t in (y, dx, dw, dbias, ws):
        assert torch.isnan(t).all()


# ------------------------------------------------------------------------------------------------------------ the module
TINY = dict(in_channels=2, channels=8, multipliers=[1, 2], factors=[2], num_blocks=[2], mel_channels=4, mel_sample_rate=8000,
            mel_n_fft=64, mel_hop_length=16, mel_normalize_log=True, resnet_groups=4, out_channels=3)


def tiny_encoder(seed=0, **over):
    cfg = dict(TINY, bottleneck=TanhBottleneck())
    cfg.update(over)
    torch.manual_seed(seed)
    enc = MelE1d(**cfg)
    with torch.no_grad():   # non-trivial norms, so that their gradients are exercised
        for n, q in enc.named_parameters():
            if "norm" in n:
                q.add_(0.1 * torch.randn_like(q))
    return enc


def torch_stack(enc, mel):
    """The encoder behind its mel front end composed from torch ops on `enc`'s own nn submodules (any dtype / device)."""
    h = F.conv1d(mel, enc.to_in.weight, enc.to_in.bias)
    for stage in enc.downsample:
        f = stage.factor
        h = F.conv1d(h, stage.down.weight, stage.down.bias, stride=f, padding=f)
        for b in stage.blocks:
            a = F.silu(F.group_norm(h, enc.groups, b.norm1.weight, b.norm1.bias, 1e-5))
            a = F.conv1d(a, b.conv1.weight, b.conv1.bias, padding=1)
            a = F.silu(F.group_norm(a, enc.groups, b.norm2.weight, b.norm2.bias, 1e-5))
            h = h + F.conv1d(a, b.conv2.weight, b.conv2.bias, padding=1)
    if hasattr(enc, "to_out"):
        h = F.conv1d(h, enc.to_out.weight, enc.to_out.bias)
    return torch.tanh(h) if enc.bottleneck is not None else h


def native_mel(enc, x):
    m = enc.mel(x)
    return m.view(x.shape[0], -1, m.shape[3])


def parity(dev, enc, T, seed=3):
    """z and every parameter gradient under a random dz against the float64 CPU composition fed the native mel output."""
    enc = enc.to(dev)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, enc.in_channels, T, generator=g)
    z, info = enc(x.to(dev), with_info=True)
    assert info == {}
    frames = enc.mel.num_frames(T)
    want_len = -(-frames // (enc.downsample_factor // enc.mel.hop_length))
    assert z.shape == (2, enc.out_channels, want_len), z.shape
    dz = torch.randn(z.shape, generator=g)
    z.backward(dz.to(dev))
    ref = copy.deepcopy(enc).cpu().double()
    for q in ref.parameters():
        q.grad = None
    with torch.no_grad():
        mel = native_mel(enc, x.to(dev)).cpu().double()
    z_ref = torch_stack(ref, mel)
    z_ref.backward(dz.double())
    err = rel_err(z, z_ref)
    print(f"z: rel err {err:.3e}")
    assert err < TOL_MODULE, err
    own, theirs = dict(enc.named_parameters()), dict(ref.named_parameters())
    assert set(own) == set(theirs)
    for n, q in own.items():
        assert q.grad is not None and torch.isfinite(q.grad).all(), n
        e = rel_err(q.grad, theirs[n].grad)
        print(f"{n}: grad rel err {e:.3e}")
        assert e < TOL_MODULE, (n, e)
    return z


def test_encoder_parity(dev):
    enc = tiny_encoder()
    assert isinstance(enc, adp.EncoderBase) and enc.out_channels == 3 and enc.downsample_factor == 32
    assert sorted(n for n, _ in enc.named_parameters() if n.startswith("downsample.0.blocks.1")) == sorted(
        f"downsample.0.blocks.1.{m}.{q}" for m in ("norm1", "conv1", "norm2", "conv2") for q in ("weight", "bias"))
    assert enc.downsample[0].down.weight.shape == (16, 8, 5) and enc.to_in.weight.shape == (8, 8, 1)
    z = parity(dev, enc, 512)
    assert z.shape == (2, 3, 16) and z.abs().max() <= 1
    with torch.no_grad():   # the no-grad path issues the same kernels
        x = torch.randn(2, 2, 512, generator=torch.Generator().manual_seed(3))
        assert torch.equal(enc(x.to(dev)), z.detach())


def test_encoder_odd_length(dev):
    """T = 400: 25 frames, 13 latent positions (the ceil rule)."""
    assert parity(dev, tiny_encoder(1), 400).shape == (2, 3, 13)


def test_encoder_two_stages(dev):
    enc = tiny_encoder(2, multipliers=[1, 2, 2], factors=[2, 4], num_blocks=[1, 1])
    assert enc.downsample_factor == 16 * 8
    assert parity(dev, enc, 512).shape == (2, 3, 4)


def test_encoder_plain_output(dev):
    enc = tiny_encoder(3, out_channels=None, bottleneck=None)
    assert enc.out_channels == 16 and not hasattr(enc, "to_out")
    assert parity(dev, enc, 512).shape == (2, 16, 16)


def test_encoder_wide_blocks(dev):
    """64 channels: the blocks take the materialised SiLU(GroupNorm) path the U-Net's wide ResnetBlocks take."""
    enc = tiny_encoder(4, channels=64, multipliers=[1, 1], factors=[3], num_blocks=[1], resnet_groups=8)
    assert parity(dev, enc, 256).shape == (2, 3, 6)


def test_constructor_and_input_errors(dev):
    with pytest.raises(NotImplementedError, match="Identity"):
        MelE1d(**TINY, bottleneck=torch.nn.Identity())
    with pytest.raises(ValueError):
        MelE1d(**dict(TINY, multipliers=[1, 2, 2]))
    with pytest.raises(NotImplementedError):
        MelE1d(**dict(TINY, factors=[8]))
    assert MelE1d(in_channels=1, channels=8, multipliers=[1, 1], factors=[2], num_blocks=[1], mel_channels=4,
                  mel_sample_rate=8000, mel_n_fft=64).downsample_factor == 16 * 2   # hop defaults to n_fft // 4
    enc = tiny_encoder().to(dev)
    with pytest.raises(TypeError):
        enc(torch.zeros(2, 2, 512, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        enc(torch.zeros(2, 3, 512, device=dev))
    if dev.type != "cpu":
        with pytest.raises(RuntimeError):
            enc(torch.zeros(2, 2, 512))


def test_no_library_ops_on_the_path(dev, monkeypatch):
    enc = tiny_encoder().to(dev)
    x = torch.randn(2, 2, 512, generator=torch.Generator().manual_seed(5)).to(dev)

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"{name} called on the native encoder path")
        return f
    for mod, name in ((F, "conv1d"), (F, "group_norm"), (F, "silu"), (torch, "tanh"), (torch, "conv1d"), (torch, "group_norm"),
                      (torch.Tensor, "tanh")):
        monkeypatch.setattr(mod, name, refuse(name))
    z = enc(x)
    z.backward(torch.ones_like(z))
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in enc.parameters())


class FixedSigmas(adp.Distribution):
    def __init__(self, vals):
        self.vals = torch.tensor(vals, dtype=torch.float32)

    def __call__(self, num_samples, device=torch.device("cpu")):
        return self.vals[:num_samples].to(device)


class TorchEncoder(adp.EncoderBase):
    """The float32 torch.nn restatement of a MelE1d (its own submodules, the native mel front end) as an EncoderBase."""

    def __init__(self, enc):
        super().__init__()
        self.enc = enc
        self.out_channels, self.downsample_factor = enc.out_channels, enc.downsample_factor

    def forward(self, x, with_info=False):
        z = torch_stack(self.enc, native_mel(self.enc, x))
        return (z, {}) if with_info else z


def test_diffusion_autoencoder_end_to_end(dev):
    torch.manual_seed(0)
    enc = tiny_encoder(6)
    ae = adp.DiffusionAE(net_t=adp.UNetV0, in_channels=2, encoder=enc, inject_depth=2, channels=[8, 16, 16],
                         factors=[2, 4, 4], items=[1, 1, 1], modulation_features=32,
                         diffusion_sigma_distribution=FixedSigmas([0.3, 0.7]), sampler_use_graph=False).to(dev)
    ref = copy.deepcopy(ae)
    ref.encoder = TorchEncoder(ref.encoder)
    g = torch.Generator().manual_seed(2)
    x, noise = torch.randn(2, 2, 512, generator=g).to(dev), torch.randn(2, 2, 512, generator=g).to(dev)
    loss = ae(x, noise=noise)
    loss.backward()
    loss_ref = ref(x, noise=noise)
    loss_ref.backward()
    print(f"loss {loss.item():.6f} reference {loss_ref.item():.6f}")
    assert abs(loss.item() - loss_ref.item()) < TOL_MODULE * abs(loss_ref.item())
    theirs = dict(ref.encoder.enc.named_parameters())
    for n, q in ae.encoder.named_parameters():
        e = rel_err(q.grad, theirs[n].grad)
        print(f"{n}: grad rel err {e:.3e}")
        assert e < TOL_MODULE, (n, e)
    with torch.no_grad():
        z = ae.encode(x)
    assert z.shape == (2, 3, 16) and not z.requires_grad
    assert ae.decode(z, num_steps=2).shape == (2, 2, 512)
