"""Native multi-resolution STFT loss (audio_diffusion_pytorch_amd/losses.py over adp_stft_loss_* in csrc/resample.hip)
against a float64 restatement of its contract on CPU torch.stft + autograd."""
import importlib.util

import pytest
import torch

import audio_diffusion_pytorch_amd as adp
from audio_diffusion_pytorch_amd import graphed
from audio_diffusion_pytorch_amd.losses import MultiResolutionSTFTLoss, STFTLoss
from conftest import rel_err
from oracle import vdiffusion as ovd
from oracle.a_unet_restatement import UNetV0Oracle

DEFAULT_RES = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
SMALL_RES = ((256, 30, 150), (128, 13, 64))
LOSS_TOL, GRAD_TOL = 1e-4, 1e-3


def mrstft_ref(x, y, res=DEFAULT_RES, w_sc=1.0, w_log=1.0, w_lin=0.0, eps=1e-8, dtype=torch.float64):
    """The contract (losses.py docstring) in float64 (or `dtype`) on CPU torch.stft; differentiable in x."""
    L = x.shape[-1]
    xr, yr = x.to(dtype).cpu().reshape(-1, L), y.to(dtype).cpu().reshape(-1, L)
    total = 0.0
    for N, h, W in res:
        win = torch.hann_window(W, dtype=dtype)

        def mag(s):
            X = torch.stft(s, N, h, W, win, center=True, pad_mode="reflect", onesided=True, return_complex=True)
            return torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=eps))

        mx, my = mag(xr), mag(yr)
        sc = torch.linalg.vector_norm(my - mx) / torch.linalg.vector_norm(my)
        lm = (torch.log(mx) - torch.log(my)).abs().mean()
        lin = (mx - my).abs().mean()
        total = total + w_sc * sc + w_log * lm + w_lin * lin
    return total / len(res)


def _crit(res, **kw):
    return MultiResolutionSTFTLoss(fft_sizes=[r[0] for r in res], hop_sizes=[r[1] for r in res],
                                   win_lengths=[r[2] for r in res], **kw)


def _pair(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(shape, generator=g)
    return y + 0.3 * torch.randn(shape, generator=g), y


def _run(crit, x, y, dev, divide=None):
    xd = x.to(dev).detach().clone().requires_grad_(True)
    loss = crit(xd, y.to(dev))
    (loss if divide is None else loss / divide).backward()
    return loss.detach().cpu(), xd.grad.detach().cpu()


def _check_against_ref(crit, res, x, y, dev, **weights):
    loss, grad = _run(crit, x, y, dev)
    xr = x.double().detach().requires_grad_(True)
    ref = mrstft_ref(xr, y, res, **weights)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= LOSS_TOL * abs(ref.item()), (loss.item(), ref.item())
    assert rel_err(grad, xr.grad) <= GRAD_TOL, rel_err(grad, xr.grad)
    return loss, grad


@pytest.mark.parametrize("L", [4096, 5000])  # 5000: no hop divides the length
def test_matches_restatement(dev, L):
    _check_against_ref(_crit(SMALL_RES), SMALL_RES, *_pair((2, 2, L)), dev)


def test_weights_and_every_fft_shape(dev):
    """w_lin_mag on, non-default weights, the two-transforms-per-pass (512) and sixteen-per-pass (64) sizes."""
    res = ((512, 100, 400), (64, 16, 64))
    crit = _crit(res, w_sc=0.5, w_log_mag=2.0, w_lin_mag=1.5)
    _check_against_ref(crit, res, *_pair((1, 3, 3000), 1), dev, w_sc=0.5, w_log=2.0, w_lin=1.5)
    single = STFTLoss(fft_size=256, hop_size=64, win_length=256, w_lin_mag=1.0)
    _check_against_ref(single, ((256, 64, 256),), *_pair((2, 1, 1500), 2), dev, w_lin=1.0)


def test_identical_inputs_give_zero_loss_and_gradient(dev):
    x, _ = _pair((2, 2, 4096), 3)
    loss, grad = _run(_crit(SMALL_RES), x, x.clone(), dev)
    assert loss.item() == 0.0
    assert torch.count_nonzero(grad) == 0


def test_silence_gives_no_nan_and_zero_gradient_where_clamped(dev):
    x, y = _pair((2, 2, 4096), 4)
    x[0, :, 1000:3000] = 0
    y[0, :, 1000:3000] = 0
    x[1, 1] = 0
    y[1, 1] = 0
    _, grad = _check_against_ref(_crit(SMALL_RES), SMALL_RES, x, y, dev)
    assert torch.isfinite(grad).all()
    # every frame that touches these samples lies in the silence (frames span at most 256 samples)
    assert torch.count_nonzero(grad[0, :, 1000 + 256:3000 - 256]) == 0
    assert torch.count_nonzero(grad[1, 1]) == 0


def test_two_calls_are_bit_identical(dev):
    x, y = _pair((2, 2, 5000), 5)
    crit = _crit(SMALL_RES)
    l1, g1 = _run(crit, x, y, dev)
    l2, g2 = _run(crit, x, y, dev)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_upstream_gradient_scales_exactly(dev):
    x, y = _pair((2, 2, 4096), 6)
    crit = _crit(SMALL_RES)
    _, g = _run(crit, x, y, dev)
    _, g4 = _run(crit, x, y, dev, divide=4)
    assert torch.equal(g4, g / 4)


@pytest.mark.parametrize("kw", [dict(w_phs=1.0), dict(perceptual_weighting=True), dict(scale="mel"), dict(n_bins=64),
                                dict(sample_rate=44100), dict(scale_invariance=True), dict(output="full"),
                                dict(reduction="sum"), dict(mag_distance="L2"), dict(window="hamming_window")])
def test_unsupported_options_raise_and_name_the_option(kw):
    name = next(iter(kw))
    with pytest.raises(NotImplementedError, match=name):
        MultiResolutionSTFTLoss(**kw)
    with pytest.raises(NotImplementedError, match=name):
        STFTLoss(**kw)


def test_unsupported_resolutions_raise():
    with pytest.raises(NotImplementedError, match="fft_size"):
        STFTLoss(fft_size=1000, win_length=600)
    with pytest.raises(NotImplementedError, match="fft_size"):
        STFTLoss(fft_size=8192, win_length=8192)
    with pytest.raises(ValueError, match="win_length"):
        STFTLoss(fft_size=256, win_length=512)
    with pytest.raises(ValueError, match="hop_size"):
        STFTLoss(fft_size=256, hop_size=0, win_length=256)
    with pytest.raises(NotImplementedError, match="resolutions"):
        MultiResolutionSTFTLoss(fft_sizes=[64] * 5, hop_sizes=[16] * 5, win_lengths=[64] * 5)


def test_short_input_and_differentiable_target_raise():
    crit = MultiResolutionSTFTLoss()
    with pytest.raises(ValueError, match="fft_size // 2"):
        crit(torch.randn(1, 1, 1024), torch.randn(1, 1, 1024))  # 1024 <= 2048 // 2
    with pytest.raises(RuntimeError, match="target"):
        crit(torch.randn(1, 1, 4096), torch.randn(1, 1, 4096, requires_grad=True))


def test_restatement_matches_auraloss():
    if importlib.util.find_spec("auraloss") is None:
        pytest.skip("auraloss is not installed")
    from auraloss.freq import MultiResolutionSTFTLoss as AuralossMRSTFT
    x, y = _pair((2, 2, 8192), 7)
    ref = AuralossMRSTFT()(x.double(), y.double())
    assert abs(mrstft_ref(x, y).item() - ref.item()) <= 1e-6 * abs(ref.item())


@pytest.mark.gpu
def test_default_resolutions_at_the_headline_shape(hip):
    """Loss within 1e-4 of the float64 restatement.  The gradient is held to what an fp32 transform can reach here, measured
    with torch.stft itself in fp32: the log-magnitude term weighs a bin by 1/m_x, and the near-zero bins of 2**21 rows x frames
    of the 512-point resolution carry the fp32 rounding of their whole frame (torch.stft in fp32 is ~1.4e-2 off float64 in
    the max norm, ~8e-3 normwise, at this shape; the small shapes above meet 1e-3)."""
    x, y = _pair((4, 2, 2 ** 18), 8)
    loss, grad = _run(MultiResolutionSTFTLoss(), x, y, hip)
    grads = {}
    for dtype in (torch.float64, torch.float32):
        xr = x.to(dtype).detach().requires_grad_(True)
        ref = mrstft_ref(xr, y, dtype=dtype)
        ref.backward()
        grads[dtype] = xr.grad.double()
        if dtype == torch.float64:
            assert abs(loss.item() - ref.item()) <= LOSS_TOL * abs(ref.item()), (loss.item(), ref.item())
    g64, g32 = grads[torch.float64], grads[torch.float32]

    def norm_err(a):
        return ((a.double() - g64).norm() / g64.norm()).item()
    assert rel_err(grad, g64) <= max(GRAD_TOL, rel_err(g32, g64)), (rel_err(grad, g64), rel_err(g32, g64))
    assert norm_err(grad) <= max(GRAD_TOL, norm_err(g32)), (norm_err(grad), norm_err(g32))


TINY = dict(in_channels=2, channels=[8, 32, 64], factors=[1, 4, 4], items=[1, 2, 2], modulation_features=128)


@pytest.mark.gpu
def test_training_step_with_the_native_loss_replays(hip):
    """DiffusionModel(loss_fn=MultiResolutionSTFTLoss()) takes the graph-replayed step (graphed.py), equals the eager step
    bit for bit, and the eager step equals UNetV0Oracle + mrstft_ref."""
    torch.manual_seed(0)
    oracle = UNetV0Oracle(**TINY)

    def model(use_graph):
        m = adp.DiffusionModel(net_t=adp.UNetV0, loss_fn=MultiResolutionSTFTLoss(), diffusion_use_graph=use_graph, **TINY)
        m.net.load_oracle_state_dict(oracle.state_dict())
        return m.to(hip)

    m_g, m_e = model(True), model(False)
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(2, 2, 4096, generator=g) for _ in range(3)]
    ns = [torch.randn(2, 2, 4096, generator=g) for _ in range(3)]
    out = {}
    for name, m in (("graph", m_g), ("eager", m_e)):
        torch.cuda.manual_seed(7)
        out[name] = []
        for x, n in zip(xs, ns):
            for p in m.parameters():
                p.grad = None
            loss = m(x.to(hip), noise=n.to(hip))
            loss.backward()
            out[name].append((loss.detach().clone(), {k: p.grad.clone() for k, p in m.net.named_parameters()}))
    gr = graphed.GRAPHS_OF[m_g.diffusion]
    assert gr.captures == 1 and gr.replays == 3 and not gr.eager_only
    assert graphed.GRAPHS_OF.get(m_e.diffusion) is None
    for (lg, gg), (le, ge) in zip(out["graph"], out["eager"]):
        assert torch.equal(lg, le)
        assert all(torch.equal(gg[k], ge[k]) for k in gg)
    # the first eager step against the oracle, with the same sigma draw (UniformDistribution: torch.rand on the device)
    torch.cuda.manual_seed(7)
    sigmas = torch.rand(2, device=hip).cpu()
    loss_ref = ovd.v_loss(oracle, xs[0], ns[0], sigmas, loss_fn=lambda a, b: mrstft_ref(a, b))
    loss_ref.backward()
    loss0, grads0 = out["eager"][0]
    assert abs(loss0.item() - loss_ref.item()) <= 1e-3 * abs(loss_ref.item()), (loss0.item(), loss_ref.item())
    own = m_e.net.oracle_named_grads(grads0)
    gmax = max(p.grad.abs().max().item() for p in oracle.parameters())
    for k, p in oracle.named_parameters():
        a, b = own[k].detach().double().cpu(), p.grad.double()
        assert (a - b).abs().max().item() / max(b.abs().max().item(), 1e-3 * gmax) < 1e-3, k


@pytest.mark.gpu
def test_diffusion_autoencoder_step_with_the_native_loss(hip):
    """The reference test's recipe (DiffusionAE + MultiResolutionSTFTLoss) with a tiny torch encoder."""
    class Enc(adp.EncoderBase):
        def __init__(self):
            super().__init__()
            self.out_channels, self.downsample_factor = 3, 4
            self.conv = torch.nn.Conv1d(2, 3, kernel_size=4, stride=4)

        def forward(self, x, with_info=False):
            z = torch.tanh(self.conv(x))
            return (z, {"z": z}) if with_info else z

    torch.manual_seed(0)
    ae = adp.DiffusionAE(net_t=adp.UNetV0, in_channels=2, encoder=Enc(), inject_depth=1,
                         loss_fn=MultiResolutionSTFTLoss(), channels=[8, 16], factors=[2, 2], items=[1, 1],
                         modulation_features=32).to(hip)
    loss = ae(torch.randn(1, 2, 8192, device=hip))
    loss.backward()
    assert torch.isfinite(loss).item()
    g = ae.encoder.conv.weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().max().item() > 0
