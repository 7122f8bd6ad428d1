"""VMultistepSampler: the second-order two-step exponential integrator for the v-objective (one net evaluation per step).

Nothing in the reference provides it, so the contract is the mathematics, restated here in float64 (`coef_table`,
`multistep_ref`: a plain Python loop over torch CPU tensors) and checked against a closed-form ODE solution.

  phi_i = sigma_i pi / 2, a_i = cos phi_i, b_i = sin phi_i, v_i = net(x_i, sigma_i)
  x0_i = a_i x_i - b_i v_i ; eps_i = b_i x_i + a_i v_i
  x_{i+1} = a_{i+1} x0_i + b_{i+1} eps_i + ca_i (x0_i - x0_{i-1}) + cb_i (eps_i - eps_{i-1})
  ca_i = (d a_{i+1} - b_{i+1} + b_i) / g ; cb_i = (d b_{i+1} + a_{i+1} - a_i) / g ; ca_0 = cb_0 = 0
  d = phi_{i+1} - phi_i ; g = phi_i - phi_{i-1}
"""
import copy
import ctypes
from math import pi

import pytest
import torch
import torch.nn as nn

import audio_diffusion_pytorch_amd as adp
from audio_diffusion_pytorch_amd import _C, ops
from conftest import rel_err
from oracle import vdiffusion as ovd
from oracle.a_unet_restatement import AppendChannelsOracle, ClassifierFreeGuidanceOracle, UNetV0Oracle
from test_full_parity import FULL
from test_stft_loss import TINY
from test_unet import ATTN

KERNEL_TOL = 2e-6   # <= 7 fp32 roundings of 2**-24 per output on intermediates up to ~2x the output's size: < 1e-6, doubled
PARITY_TOL = 1e-3   # the project's parity contract (smoke()'s sampler check)


# ------------------------------------------------------------------ float64 restatement of the contract
def coef_table(sigmas: torch.Tensor) -> torch.Tensor:
    """Rows (a_i, b_i, a_{i+1}, b_{i+1}, ca_i, cb_i) in float64 for sigma_0..sigma_N."""
    phi = sigmas.double() * (pi / 2)
    n = phi.numel() - 1
    rows = []
    for i in range(n):
        a0, b0, a1, b1 = torch.cos(phi[i]), torch.sin(phi[i]), torch.cos(phi[i + 1]), torch.sin(phi[i + 1])
        ca = cb = torch.zeros((), dtype=torch.float64)
        if i > 0:
            d, g = phi[i + 1] - phi[i], phi[i] - phi[i - 1]
            ca = (d * a1 - b1 + b0) / g
            cb = (d * b1 + a1 - a0) / g
        rows.append(torch.stack([a0, b0, a1, b1, ca, cb]))
    return torch.stack(rows)


def step_ref(x, v, hx, he, row):
    """One update in float64: (x_next, x0, eps); the history is not used where ca = cb = 0."""
    x, v = x.double(), v.double()
    a0, b0, a1, b1, ca, cb = [r.double() for r in row]
    x0 = a0 * x - b0 * v
    eps = b0 * x + a0 * v
    xn = a1 * x0 + b1 * eps
    if ca != 0 or cb != 0:
        xn = xn + ca * (x0 - hx.double()) + cb * (eps - he.double())
    return xn, x0, eps


@torch.no_grad()
def multistep_ref(net, x, num_steps, schedule=None, **kw):
    """The sampler in float64 (state and coefficients); `net` is evaluated in float32 on the CPU, as the oracle is."""
    schedule = schedule if schedule is not None else adp.LinearSchedule()
    sigmas = schedule(num_steps + 1, device="cpu").to(torch.float32)
    table = coef_table(sigmas)
    x = x.double().cpu()
    hx = he = torch.zeros_like(x)
    for i in range(num_steps):
        v = net(x.float(), sigmas[i].expand(x.shape[0]), **kw)
        x, hx, he = step_ref(x, v, hx, he, table[i])
    return x


# ------------------------------------------------------------------ 1. kernel vs restatement
def _kernel_case(n, seed=0):
    g = torch.Generator().manual_seed(seed + n)
    x, v, hx, he = [torch.randn(n, generator=g) for _ in range(4)]
    row = coef_table(torch.tensor([0.62, 0.55, 0.5]))[1].to(torch.float32)  # (the fp32 row the kernel is given)
    assert row[4] != 0 and row[5] != 0
    return x, v, hx, he, row


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("n", [1, 3, 1000, 4099, 2 * 2 ** 18])
def test_kernel_matches_restatement(dev, n, inplace):
    x, v, hx, he, row = _kernel_case(n)
    ref = step_ref(x, v, hx, he, row)
    dx, dv, dhx, dhe, drow = [t.to(dev) for t in (x, v, hx, he, row)]
    if inplace:
        out = ops.v_step2(dx, dv, dhx, dhe, drow, out=dx, hist_x0_out=dhx, hist_eps_out=dhe)
        assert out[0] is dx and out[1] is dhx and out[2] is dhe
    else:
        out = ops.v_step2(dx, dv, dhx, dhe, drow)
        assert torch.equal(dx.cpu(), x) and torch.equal(dhx.cpu(), hx) and torch.equal(dhe.cpu(), he)
    assert torch.equal(dv.cpu(), v)
    errs = [rel_err(o, r) for o, r in zip(out, ref)]
    print(f"v_step2 n={n} inplace={inplace}: rel_err x / x0 / eps = {errs}")
    assert all(e <= KERNEL_TOL for e in errs), errs


@pytest.mark.parametrize("n", [3, 4099])
def test_first_step_does_not_read_the_history(dev, n):
    """ca = cb = 0: NaN-filled history inputs cannot reach x, and the result is VSampler's step."""
    x, v, _, _, row = _kernel_case(n)
    row = row.clone()
    row[4:] = 0.0
    nan = torch.full((n,), float("nan"))
    xo, hxo, heo = ops.v_step2(x.to(dev), v.to(dev), nan.to(dev), nan.clone().to(dev), row.to(dev))
    first = ops.v_step(x.to(dev), v.to(dev), row[:4].contiguous().to(dev))
    assert torch.isfinite(xo).all() and torch.isfinite(hxo).all() and torch.isfinite(heo).all()
    assert rel_err(xo, first) <= KERNEL_TOL
    ref = step_ref(x, v, nan, nan, row)
    assert all(rel_err(o, r) <= KERNEL_TOL for o, r in zip((xo, hxo, heo), ref))


def test_v_step2_wrapper_rejects_mismatched_sizes(emul):
    x = torch.randn(8)
    row = torch.zeros(6)
    with pytest.raises(ValueError):
        ops.v_step2(x, torch.randn(7), x.clone(), x.clone(), row)
    with pytest.raises(ValueError):
        ops.v_step2(x, x.clone(), x.clone(), x.clone(), torch.zeros(4))


# ------------------------------------------------------------------ 2. C-ABI
def test_c_abi_v_step2_returns_error_codes(dev):
    lib = _C.lib()
    s = _C.stream()
    ERR_SHAPE, ERR_NULL = -1, -5
    x = torch.randn(64).to(dev)
    p = x.data_ptr()
    for k in (0, 1, 2, 3, 4, 6, 7, 8):  # every pointer argument in turn
        args = [p, p, p, p, p, x.numel(), p, p, p]
        args[k] = None
        assert lib.adp_v_step2(*args, s) == ERR_NULL, k
    assert lib.adp_v_step2(p, p, p, p, p, 0, p, p, p, s) == ERR_SHAPE
    assert lib.adp_v_step2(p, p, p, p, p, -4, p, p, p, s) == ERR_SHAPE
    assert _C.SIGNATURES["adp_v_step2"] == (ctypes.c_int, [_C.P] * 5 + [_C.I] + [_C.P] * 4)


# ------------------------------------------------------------------ 3. order of convergence on a problem with a known answer
class GaussianV(nn.Module):
    """The optimal v-prediction for data that is elementwise N(0, s**2) (a plain module, not a U-Net):
    v(x, phi) = cos(phi) sin(phi) (1 - s**2) / (cos(phi)**2 s**2 + sin(phi)**2) x.  The probability-flow ODE then has the
    exact solution x(phi_N) = x(phi_0) sqrt(var(phi_N) / var(phi_0)), var(phi) = cos(phi)**2 s**2 + sin(phi)**2."""

    def __init__(self, s: float):
        super().__init__()
        self.s = s

    def forward(self, x, sigmas):
        phi = (sigmas * (pi / 2)).view(-1, *([1] * (x.ndim - 1)))
        c, sn = torch.cos(phi), torch.sin(phi)
        return c * sn * (1 - self.s ** 2) / (c * c * self.s ** 2 + sn * sn) * x

    def exact(self, x_start, sigma_start: float, sigma_end: float):
        var = lambda sg: torch.cos(torch.tensor(sg * pi / 2, dtype=torch.float64)) ** 2 * self.s ** 2 + \
            torch.sin(torch.tensor(sg * pi / 2, dtype=torch.float64)) ** 2
        return x_start.double() * torch.sqrt(var(sigma_end) / var(sigma_start))


class QuadraticSchedule(adp.Schedule):
    def forward(self, num_steps, device):
        return torch.linspace(1.0, 0.0, num_steps, device=device) ** 2


def _errors(sampler_t, s, dev, schedule, steps):
    net = GaussianV(s)
    x = torch.randn(4, 2, 64, generator=torch.Generator().manual_seed(3))
    exact = net.exact(x, 1.0, 0.0)
    sampler = sampler_t(net=net, schedule=schedule)
    return {n: rel_err(sampler(x.to(dev), num_steps=n), exact) for n in steps}


@pytest.mark.parametrize("s", [0.3, 1.5])
def test_second_order_convergence(dev, s):
    new = _errors(adp.VMultistepSampler, s, dev, adp.LinearSchedule(), (10, 20, 40, 80))
    old = _errors(adp.VSampler, s, dev, adp.LinearSchedule(), (10, 20, 40, 80))
    print(f"s={s} linear: multistep {new} ratios {[new[n] / new[2 * n] for n in (10, 20, 40)]}; "
          f"VSampler {old} ratios {[old[n] / old[2 * n] for n in (10, 20, 40)]}")
    for n in (20, 40):
        assert new[n] / new[2 * n] >= 3.0, (n, new)          # theory 4
        assert old[n] / old[2 * n] < 2.5, (n, old)           # first order: the test tells the two apart
    for n in (10, 20, 40):
        assert new[n] < old[2 * n], (n, new, old)            # better at N steps than VSampler at 2N
    quad = _errors(adp.VMultistepSampler, s, dev, QuadraticSchedule(), (20, 40, 80))
    print(f"s={s} quadratic: multistep {quad} ratios {[quad[n] / quad[2 * n] for n in (20, 40)]}")
    for n in (20, 40):
        assert quad[n] / quad[2 * n] >= 3.0, (n, quad)


def test_restatement_is_second_order():
    """The float64 loop of this file on the same problem (so the numbers the other tests compare against are themselves
    the method): ratios near 4, and the product's coefficient table equals the restatement's."""
    net = GaussianV(0.3)
    x = torch.randn(4, 2, 64, generator=torch.Generator().manual_seed(3))
    err = {n: rel_err(multistep_ref(net, x, n), net.exact(x, 1.0, 0.0)) for n in (20, 40, 80)}
    assert 3.5 <= err[20] / err[40] <= 4.5 and 3.5 <= err[40] / err[80] <= 4.5, err
    sampler = adp.VMultistepSampler(net=net)
    _, coef = sampler._tables(40, 4, "cpu")
    ref = coef_table(torch.linspace(1.0, 0.0, 41)).to(torch.float32)
    assert coef.shape == (40, 6) and coef.dtype == torch.float32
    assert torch.equal(coef[0, 4:], torch.zeros(2))
    # both are float64 values rounded to float32 once: at most one float32 ulp (2**-23 relative) apart
    assert torch.allclose(coef, ref, rtol=2 ** -23, atol=1e-12)


def test_bad_arguments_raise():
    net = GaussianV(0.3)
    for order in (0, 3, "2"):
        with pytest.raises(ValueError, match="order"):
            adp.VMultistepSampler(net=net, order=order)

    class Repeats(adp.Schedule):
        def forward(self, num_steps, device):
            sig = torch.linspace(1.0, 0.0, num_steps, device=device)
            sig[2] = sig[1]
            return sig

    with pytest.raises(ValueError, match="sigma"):
        adp.VMultistepSampler(net=net, schedule=Repeats())(torch.randn(1, 2, 8), num_steps=5)
    assert "VMultistepSampler" in adp.__all__ and issubclass(adp.VMultistepSampler, adp.VSampler)


# ------------------------------------------------------------------ 4. sampler vs restatement through a real U-Net
def _tiny_pair(dev, sampler_t=None, **sampler_kw):
    torch.manual_seed(0)
    oracle = UNetV0Oracle(**TINY)
    kw = {f"sampler_{k}": v for k, v in sampler_kw.items()}
    model = adp.DiffusionModel(net_t=adp.UNetV0, sampler_t=sampler_t or adp.VMultistepSampler, **kw, **TINY)
    model.net.load_oracle_state_dict(oracle.state_dict())
    return oracle, model.to(dev)


def test_sampler_matches_restatement_through_a_unet(dev):
    oracle, model = _tiny_pair(dev)
    _, first_order = _tiny_pair(dev, sampler_t=adp.VSampler)
    _, order1 = _tiny_pair(dev, order=1)
    noise = torch.randn(2, 2, 4096, generator=torch.Generator().manual_seed(1))
    outs = {}
    for steps in (1, 2, 7):
        outs[steps] = model.sample(noise.to(dev), num_steps=steps)
        err = rel_err(outs[steps], multistep_ref(oracle, noise, steps))
        print(f"tiny U-Net, {steps} steps: rel_err vs restatement {err}")
        assert outs[steps].shape == noise.shape and err <= PARITY_TOL, (steps, err)
    assert rel_err(outs[1], first_order.sample(noise.to(dev), num_steps=1)) <= 1e-6
    first7 = first_order.sample(noise.to(dev), num_steps=7)
    assert rel_err(order1.sample(noise.to(dev), num_steps=7), first7) <= 1e-6
    # and the second-order result is a different trajectory, not the first-order one under another name
    assert rel_err(outs[7], first7) > 1e-4


# ------------------------------------------------------------------ 5. replay equals eager
@pytest.mark.gpu
def test_replay_equals_eager(hip):
    _, m_g = _tiny_pair(hip)
    _, m_e = _tiny_pair(hip, use_graph=False)
    g = torch.Generator().manual_seed(2)
    noise, noise2 = torch.randn(2, 2, 4096, generator=g).to(hip), torch.randn(2, 2, 4096, generator=g).to(hip)
    out7, out3 = m_g.sample(noise, num_steps=7), m_g.sample(noise, num_steps=3)
    assert m_g.sampler.graph_captures == 1 and m_g.sampler.graph_replays == 2 and len(m_g.sampler._graph_cache) == 1
    assert m_e.sampler.graph_captures == 0
    assert torch.equal(out7, m_e.sample(noise, num_steps=7)) and torch.equal(out3, m_e.sample(noise, num_steps=3))
    assert torch.equal(m_g.sample(noise, num_steps=7), out7), "the previous run's history leaked into this one"
    # a run from NaN leaves NaN in the entry's history buffers; the next run must not see it
    poisoned = m_g.sample(torch.full_like(noise, float("nan")), num_steps=3)
    assert torch.isnan(poisoned).all()
    assert all(torch.isnan(b).all() for b in next(iter(m_g.sampler._graph_cache.values())).bufs)
    out = m_g.sample(noise2, num_steps=5)
    assert torch.isfinite(out).all() and torch.equal(out, m_e.sample(noise2, num_steps=5))
    assert m_g.sampler.graph_captures == 1
    # a deep copy (an EMA copy) leaves graphs and history behind and captures its own
    cp = copy.deepcopy(m_g)
    assert len(cp.sampler._graph_cache) == 0 and cp.sampler.graph_captures == 0 and cp.sampler.order == 2
    assert torch.equal(cp.sample(noise2, num_steps=5), out)
    assert cp.sampler.graph_captures == 1 and m_g.sampler.graph_captures == 1


# ------------------------------------------------------------------ 6. wrappers
@pytest.mark.gpu
def test_diffusion_model_with_sampler_t(hip):
    oracle, model = _tiny_pair(hip)
    assert type(model.sampler) is adp.VMultistepSampler
    noise = torch.randn(2, 2, 4096, generator=torch.Generator().manual_seed(4))
    assert rel_err(model.sample(noise.to(hip), num_steps=6), multistep_ref(oracle, noise, 6)) <= PARITY_TOL


@pytest.mark.gpu
def test_upsampler_sample(hip):
    torch.manual_seed(0)
    cfg = dict(TINY)
    cfg.pop("in_channels")
    up = adp.DiffusionUpsampler(net_t=adp.UNetV0, in_channels=2, upsample_factor=4, sampler_t=adp.VMultistepSampler, **cfg)
    oracle = AppendChannelsOracle(lambda **kw: UNetV0Oracle(**kw), channels=2)(in_channels=2, **cfg)
    up.net.net.load_oracle_state_dict(oracle.net.state_dict())
    up = up.to(hip)
    low = torch.randn(2, 2, 1024, generator=torch.Generator().manual_seed(9))
    cond = ovd.upsample(low, 4)
    torch.manual_seed(77)
    out = up.sample(low.to(hip), num_steps=5)
    torch.manual_seed(77)
    ref = multistep_ref(oracle, torch.randn(cond.shape), 5, append_channels=cond)
    assert out.shape == (2, 2, 4096) and rel_err(out, ref) <= PARITY_TOL


@pytest.mark.gpu
def test_autoencoder_decode(hip):
    class Enc(adp.EncoderBase):
        def __init__(self):
            super().__init__()
            self.out_channels, self.downsample_factor = 3, 4
            self.conv = torch.nn.Conv1d(2, 3, kernel_size=4, stride=4)

        def forward(self, x, with_info=False):
            z = torch.tanh(self.conv(x))
            return (z, {"z": z}) if with_info else z

    torch.manual_seed(0)
    cfg = dict(channels=[8, 16], factors=[2, 2], items=[1, 1], modulation_features=32)
    ae = adp.DiffusionAE(net_t=adp.UNetV0, in_channels=2, encoder=Enc(), inject_depth=1, sampler_t=adp.VMultistepSampler,
                         **cfg)
    oracle = UNetV0Oracle(in_channels=2, context_channels=[0, 3], **cfg)
    ae.net.load_oracle_state_dict(oracle.state_dict())
    ae = ae.to(hip)
    z = torch.tanh(torch.randn(2, 3, 256, generator=torch.Generator().manual_seed(6)))
    out = ae.decode(z.to(hip), num_steps=5, generator=torch.Generator(device=hip).manual_seed(5))
    start = torch.randn((2, 2, 1024), device=hip, dtype=z.dtype, generator=torch.Generator(device=hip).manual_seed(5))
    ref = multistep_ref(oracle, start.cpu(), 5, channels=[None, z])
    assert out.shape == (2, 2, 1024) and rel_err(out, ref) <= PARITY_TOL


@pytest.mark.gpu
def test_classifier_free_guidance(hip):
    """embedding_scale != 1 doubles the batch inside the net only: the history has x's shape."""
    torch.manual_seed(0)
    inner = UNetV0Oracle(**ATTN)
    oracle = ClassifierFreeGuidanceOracle(inner, embedding_max_length=7, embedding_features=12)
    model = adp.DiffusionModel(net_t=adp.UNetV0, use_embedding_cfg=True, embedding_max_length=7,
                               sampler_t=adp.VMultistepSampler, **ATTN)
    model.net.net.load_oracle_state_dict(inner.state_dict())
    with torch.no_grad():
        model.net.fixed_embedding.weight.copy_(oracle.fixed_embedding.weight)
    model = model.to(hip)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3, 2, 96, generator=g)
    emb = torch.randn(3, 5, 12, generator=g)
    out = model.sample(x.to(hip), num_steps=4, embedding=emb.to(hip), embedding_scale=2.0)
    ref = multistep_ref(lambda xx, tt: oracle(xx, tt, embedding=emb, embedding_scale=2.0), x, 4)
    assert model.sampler.graph_captures == 1
    assert all(b.shape == x.shape for b in next(iter(model.sampler._graph_cache.values())).bufs)
    assert rel_err(out, ref) <= PARITY_TOL


# ------------------------------------------------------------------ 7. full size
@pytest.mark.gpu
def test_full_size_25_steps(hip):
    """The bench configuration, [1, 2, 2**18], 25 steps, against the restatement with UNetV0Oracle on the CPU."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    torch.manual_seed(0)
    oracle = UNetV0Oracle(**FULL)
    noise = torch.randn(1, 2, 2 ** 18, generator=torch.Generator().manual_seed(0))
    ref = multistep_ref(oracle, noise, 25)
    model = adp.DiffusionModel(net_t=adp.UNetV0, sampler_t=adp.VMultistepSampler, **FULL)
    model.net.load_oracle_state_dict(oracle.state_dict())
    model = model.to(hip)
    out = model.sample(noise.to(hip), num_steps=25)
    err = rel_err(out, ref)
    print(f"full size, 25 steps: rel_err vs restatement {err}")
    assert out.shape == ref.shape and err <= PARITY_TOL
