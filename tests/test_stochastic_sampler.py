"""VStochasticSampler: DDIM with eta > 0 on the v-objective, its noise formed inside the update kernel (include/adp_sde.h).

Nothing in the reference provides it, so the contract is the mathematics, restated here in float64 (`coef_table`, `step_ref`,
`stochastic_ref`: a plain Python loop) with the noise taken from `ops.randn` on the same (seed, draw) row:

  phi_i = sigma_i pi / 2, a_i = cos phi_i, b_i = sin phi_i, v_i = net(x_i, sigma_i)
  x0_i = a_i x_i - b_i v_i ; eps_i = b_i x_i + a_i v_i ; x0c_i = x0_i, clamp(x0_i, -s_r, s_r) / s_r or clamp(x0_i, -1, 1)
  cz_i = eta (b_{i+1} / b_i) sqrt(b_i^2 - b_{i+1}^2) / a_{i+1}   (0 where b_i = 0 or b_{i+1} = 0) ; ce_i = sqrt(b_{i+1}^2 - cz_i^2)
  x_{i+1} = a_{i+1} x0c_i + ce_i eps_i + cz_i z_i ;  z_i = draw 1 + i of the seed (draw 0: the start noise)

STEP_TOL.  The kernel rounds b0 v and the fused multiply-add behind it (2) and the division by the scale (1) on the way to
x0c, a0 v and its multiply-add (2) and ce eps (1) on the way to the second term, then two more multiply-adds: 8 float32
roundings of 2**-24 on the longest path, each relative to an intermediate of at most twice the largest output (coefficients
<= 1, inputs of the output's size).  8 * 2**-24 * 2 = 9.5e-7 in the max norm; the bound is twice that, as KERNEL_TOL of
tests/test_multistep_sampler.py is."""
import copy
from math import pi, sqrt

import pytest
import torch
import torch.nn as nn

import audio_diffusion_pytorch_amd as adp
from audio_diffusion_pytorch_amd import diffusion, ops
from conftest import rel_err
from oracle import vdiffusion as ovd
from oracle.a_unet_restatement import AppendChannelsOracle, ClassifierFreeGuidanceOracle, UNetV0Oracle
from test_full_parity import FULL
from test_multistep_sampler import PARITY_TOL, GaussianV
from test_stft_loss import TINY
from test_threshold_sampler import clip_ref
from test_unet import ATTN

STEP_TOL = 2 * (8 * 2.0 ** -24 * 2)   # 1.9e-6 (module docstring)
LOOP_TOL = 1e-5                       # sampler against the restatement on the same net and backend (tests/test_inpaint_graph.py)
SEED = 0x1D872B41C9F0A5E3


# ------------------------------------------------------------------ float64 restatement of the contract
def coef_table(sigmas: torch.Tensor, eta: float) -> torch.Tensor:
    """Rows (a_i, b_i, a_{i+1}, ce_i, cz_i) in float64 for sigma_0..sigma_N."""
    phi = sigmas.double() * (pi / 2)
    rows = []
    for i in range(phi.numel() - 1):
        a0, b0, a1, b1 = torch.cos(phi[i]), torch.sin(phi[i]), torch.cos(phi[i + 1]), torch.sin(phi[i + 1])
        cz = torch.zeros((), dtype=torch.float64)
        if b0 != 0 and b1 != 0 and eta != 0:
            cz = eta * (b1 / b0) * torch.sqrt(b0 * b0 - b1 * b1) / a1
        # (real for eta in [0, 1]; where it is 0 -- eta = 1 from pure noise -- float64 may land a rounding below)
        ce = torch.sqrt((b1 * b1 - cz * cz).clamp_min(0.0))
        rows.append(torch.stack([a0, b0, a1, ce, cz]))
    return torch.stack(rows)


def step_ref(x, v, row, z, clip=False, scale=None):
    """One update in float64.  `scale` [B] or None; clip without a scale is the static clamp.  eps from the raw v."""
    x, v = x.double(), v.double()
    a0, b0, a1, ce, cz = [r.double() for r in row]
    x0, eps = a0 * x - b0 * v, b0 * x + a0 * v
    if clip and scale is not None:
        s = diffusion.pad_dims(scale.double(), x.ndim - 1)
        x0 = x0.clamp(-s, s) / s
    elif clip:
        x0 = x0.clamp(-1.0, 1.0)
    xn = a1 * x0 + ce * eps
    return xn + cz * z.double() if cz != 0 else xn


def draw(seed, d, like):
    """Draw d of the seed in the shape of `like`, from the library's generator on `like`'s backend."""
    return ops.randn(like, ops.rng_rows(seed, [d])[0].to(like.device))


@torch.no_grad()
def stochastic_ref(net, x, num_steps, eta, seed, q=None, sigmas=None, scales=None, **kw):
    """The sampler in float64 (state, coefficients, quantile).  `net` runs in float32 wherever x lives; the noise of step i is
    draw 1 + i from `ops.randn` there.  `scales`, a list, receives each step's scale row."""
    if sigmas is None:
        sigmas = adp.LinearSchedule()(num_steps + 1, device="cpu").to(torch.float32)
    table = coef_table(sigmas, eta)
    dev = x.device
    x = x.double()
    for i in range(num_steps):
        v = net(x.float(), sigmas[i].expand(x.shape[0]).to(dev), **kw).double()
        scale = None
        if q:
            scale = clip_ref((table[i][0] * x - table[i][1] * v).cpu(), q)[1].to(dev)
            if scales is not None:
                scales.append(scale.cpu())
        z = draw(seed, 1 + i, x.float()) if table[i][4] != 0 else torch.zeros_like(x)
        x = step_ref(x, v, table[i].to(dev), z, clip=q is not None, scale=scale)
    return x


# ------------------------------------------------------------------ 1. kernel against the restatement
ROW = coef_table(torch.tensor([0.62, 0.55, 0.5]), 0.7)[1].to(torch.float32)   # (the fp32 row the kernel is given)
assert ROW[4] > 0.01 and ROW[3] > 0.01


def _rng(dev, d=3):
    return ops.rng_rows(SEED, [d])[0].to(dev)


def _kernel_case(shape):
    g = torch.Generator().manual_seed(shape[-1])
    return [torch.randn(shape, generator=g) * 1.5 for _ in range(2)]


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("mode", ["plain", "static", "scale"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 3), (1, 1000), (1, 4099), (1, 2 * 2 ** 18), (3, 1365)], ids=str)
def test_kernel_matches_restatement(dev, shape, mode, inplace):
    x, v = _kernel_case(shape)
    scale = torch.tensor([1.0, 1.7, 2.5][:shape[0]]) if mode == "scale" else None
    assert shape != (3, 1365) or 1365 % 4 != 0   # a group of four straddles two items
    dx, dv, drow, rng = x.to(dev), v.to(dev), ROW.to(dev), _rng(dev)
    z = ops.randn(dx, rng).cpu()
    want = step_ref(x, v, ROW, z, clip=mode != "plain", scale=scale)
    out = ops.v_step_eta(dx, dv, drow, rng, scale=None if scale is None else scale.to(dev), clip=mode != "plain",
                         out=dx if inplace else None)
    assert (out is dx) == inplace
    if not inplace:
        assert torch.equal(dx.cpu(), x)
    assert torch.equal(dv.cpu(), v) and torch.equal(drow.cpu(), ROW) and torch.equal(rng.cpu(), _rng("cpu"))
    err = rel_err(out, want)
    print(f"adp_v_step_eta {shape} {mode} inplace={inplace}: rel_err {err:.3e} (bound {STEP_TOL:.2e})")
    assert out.shape == x.shape and err <= STEP_TOL


# ------------------------------------------------------------------ 2. the noise is the library's stream, exactly
@pytest.mark.parametrize("n", [2048, 1001])
def test_noise_is_randn_of_the_same_row(dev, n):
    zero = torch.zeros(1, n, device=dev)
    only_noise = torch.tensor([0.3, 0.9, 0.5, 0.0, 1.0], device=dev)   # x = v = 0, ce = 0, cz = 1
    rng = _rng(dev)
    want = ops.randn(zero, rng)
    aligned = ops.v_step_eta(zero, zero, only_noise, rng)
    assert aligned.data_ptr() % 16 == 0 and torch.equal(aligned, want)
    backing = torch.zeros(n + 4, device=dev)
    odd = backing[1:1 + n].view(1, n)
    assert odd.data_ptr() % 16 == 4
    assert ops.v_step_eta(zero, zero, only_noise, rng, out=odd) is odd and torch.equal(odd, want)
    assert backing[0] == 0 and bool((backing[1 + n:] == 0).all())
    other = ops.v_step_eta(zero, zero, only_noise, _rng(dev, d=4))
    assert not torch.equal(other, want) and torch.equal(other, ops.randn(zero, _rng(dev, d=4)))
    assert abs(want.var().item() - 1) < 0.2 and want.abs().max().item() < 5.9


@pytest.mark.parametrize("n", [3, 4099])
def test_a_row_without_noise_does_not_read_the_generator(dev, n):
    """cz = 0: a NaN-filled row, or none at all, cannot reach x, and the step is VSampler's."""
    x, v = _kernel_case((1, n))
    row = ROW.clone()
    row[4] = 0.0
    nan_row = torch.full((4,), 0x7FC00000, dtype=torch.int32)
    first = ops.v_step(x.to(dev), v.to(dev), row[:4].contiguous().to(dev))
    for rng in (nan_row.to(dev), None):
        out = ops.v_step_eta(x.to(dev), v.to(dev), row.to(dev), rng)
        assert torch.isfinite(out).all() and rel_err(out, first) <= STEP_TOL
        assert rel_err(out, step_ref(x, v, row, torch.zeros_like(x))) <= STEP_TOL
    # noise asked for without a row: NaN, not a read through a null pointer
    assert torch.isnan(ops.v_step_eta(x.to(dev), v.to(dev), ROW.to(dev), None)).all()


def test_wrapper_rejects_bad_arguments(emul):
    x, row, rng = torch.zeros(2, 8), torch.zeros(5), _rng("cpu")
    for call in (lambda: ops.v_step_eta(x, torch.zeros(2, 7), row, rng),
                 lambda: ops.v_step_eta(x, x, torch.zeros(4), rng),
                 lambda: ops.v_step_eta(x, x, row.double(), rng),
                 lambda: ops.v_step_eta(x, x, row, rng.float()),
                 lambda: ops.v_step_eta(x, x, row, rng[:3]),
                 lambda: ops.v_step_eta(x, x, row, rng, scale=torch.ones(2)),              # a scale without clip
                 lambda: ops.v_step_eta(x, x, row, rng, scale=torch.ones(3), clip=True),
                 lambda: ops.v_step_eta(x, x, row, rng, clip=1),
                 lambda: ops.v_step_eta(x, x, row, rng, out=torch.zeros(16)),
                 lambda: ops.v_step_eta(torch.zeros(()), torch.zeros(()), row, rng)):
        with pytest.raises(ValueError):
            call()
    assert torch.equal(x, torch.zeros(2, 8))


# ------------------------------------------------------------------ 4. the table
def _words(table):
    return table[:, :5].contiguous().view(torch.float32), table[:, 5:]


def test_table_matches_restatement(emul):
    net = GaussianV(0.3)
    sampler = adp.VStochasticSampler(net, eta=0.7)
    sampler._run = (SEED, 1.0)
    sig, table = sampler._tables(40, 3, "cpu")
    assert sig.shape == (41, 3) and table.shape == (40, 9) and table.dtype == torch.int32
    coef, rng = _words(table)
    ref = coef_table(torch.linspace(1.0, 0.0, 41), 0.7).to(torch.float32)
    # both are float64 values rounded to float32 once: at most one float32 ulp apart
    assert torch.allclose(coef, ref, rtol=2 ** -23, atol=1e-12)
    assert torch.equal(rng, ops.rng_rows(SEED, range(1, 41)))
    assert rng[:, 2].tolist() == list(range(1, 41)) and len(set(rng[:, 2].tolist())) == 40
    assert coef[-1, 4] == 0 and coef[-1, 3] == 0 and coef[-1, 2] == 1      # the last step returns x0c
    assert bool((coef[:-1, 4] > 0).all())
    full, _ = _words(adp.VStochasticSampler(net, eta=1.0)._tables(40, 3, "cpu")[1])
    assert abs(full[0, 3].item()) < 1e-6                                   # from pure noise with eta = 1: the DDPM step
    zero = coef_table(torch.linspace(1.0, 0.0, 41), 0.0)
    assert torch.equal(zero[:, 4], torch.zeros(40, dtype=torch.float64))
    assert torch.allclose(zero[:, 3], torch.sin(torch.linspace(1.0, 0.0, 41).double() * (pi / 2))[1:], rtol=0, atol=1e-15)
    # eta = 0 is the parent's table, bit for bit
    plain = adp.VStochasticSampler(net, eta=0.0)._tables(40, 3, "cpu")[1]
    assert plain.dtype == torch.float32 and torch.equal(plain, adp.VSampler(net)._tables(40, 3, "cpu")[1])


def test_bad_arguments_raise(emul):
    net = GaussianV(0.3)
    for bad in (-0.1, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="eta"):
            adp.VStochasticSampler(net, eta=bad)
    for bad in (-0.1, 1.5, float("nan"), "0.9", True):
        with pytest.raises(ValueError, match="dynamic_threshold"):
            adp.VStochasticSampler(net, dynamic_threshold=bad)
    s = adp.VStochasticSampler(net)
    assert s.eta == 1.0 and s.dynamic_threshold is None and s.use_graph
    assert "VStochasticSampler" in adp.__all__ and issubclass(adp.VStochasticSampler, adp.VSampler)

    class Increases(adp.Schedule):
        def forward(self, num_steps, device):
            sig = torch.linspace(1.0, 0.0, num_steps, device=device)
            sig[3] = sig[1]
            return sig

    with pytest.raises(ValueError, match="step 2"):
        adp.VStochasticSampler(net, schedule=Increases(), eta=0.5)(torch.randn(1, 2, 8), num_steps=5)
    x = torch.randn(1, 2, 8)
    with pytest.raises(ValueError, match="strength"):
        s(x, num_steps=2, strength=0.5)                  # strength without a start
    with pytest.raises(ValueError, match="x_noisy"):
        s(None, num_steps=2)                             # nothing to start from
    for bad in (0.0, 1.5, -1.0, "1", True):
        with pytest.raises(ValueError, match="strength"):
            s(x, num_steps=2, start=x, strength=bad)


# ------------------------------------------------------------------ 5. sampler against the restatement through a net
SHAPE, STEPS = (2, 2, 64), 4


def tiny_net(dev, seed=0):
    torch.manual_seed(seed)
    return adp.UNetV0(dim=1, **TINY).to(dev).eval()


class Counting(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net, self.calls = net, 0

    def forward(self, x, time, **kw):
        self.calls += 1
        return self.net(x, time, **kw)


def _start(dev, seed=1):
    return (2 * torch.randn(SHAPE, generator=torch.Generator().manual_seed(seed))).to(dev)


def _no_torch_noise(m):
    def forbidden(*a, **kw):
        raise AssertionError("a torch random function inside the sampling run")

    for name in ("randn", "randn_like", "rand"):
        m.setattr(torch, name, forbidden)


_OUTS = {}


@pytest.mark.parametrize("q", [None, 0.9], ids=["plain", "q0.9"])
@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_sampler_matches_restatement_through_a_unet(dev, monkeypatch, eta, q):
    net, x = tiny_net(dev), _start(dev)
    counting = Counting(net)
    sampler = adp.VStochasticSampler(counting, eta=eta, dynamic_threshold=q, use_graph=False)
    kept = x.clone()
    with monkeypatch.context() as m:
        _no_torch_noise(m)
        out = sampler(x, num_steps=STEPS, seed=SEED)
    assert counting.calls == STEPS, "one net evaluation per step"
    assert torch.equal(x, kept)
    scales = []
    want = stochastic_ref(net, x, STEPS, eta, SEED, q=q, scales=scales)
    if q:   # the condition under which the thresholded case says anything
        assert any(s > 1 for row in scales for s in row.tolist()), scales
    err = rel_err(out, want)
    print(f"VStochasticSampler eta={eta} q={q}: rel_err vs float64 loop {err:.3e} (bound {LOOP_TOL:.0e})")
    assert out.shape == x.shape and err <= LOOP_TOL
    # and eta matters: the other case of this threshold is another trajectory (an emulated forward takes seconds: the
    # comparison is between the cases' kept results, no further run)
    _OUTS[(dev.type, eta, q)] = out.cpu()
    twin = _OUTS.get((dev.type, 1.5 - eta, q))
    assert twin is None or rel_err(out, twin) > 1e-2


def wide_net():
    """The closed-form v of N(0, 1.5**2) data: a net that depends on sigma and whose x0 leaves [-1, 1], at no cost."""
    return GaussianV(1.5)


def test_seed_governs_the_run(dev):
    net, x = wide_net(), _start(dev)
    s = adp.VStochasticSampler(net, eta=1.0, use_graph=False)
    a = s(x, num_steps=2, seed=7)
    assert torch.equal(a, s(x, num_steps=2, seed=7)) and not torch.equal(a, s(x, num_steps=2, seed=8))
    torch.manual_seed(123)
    d1, d2 = s(x, num_steps=2), s(x, num_steps=2)
    torch.manual_seed(123)
    assert torch.equal(d1, s(x, num_steps=2)) and not torch.equal(d1, d2)


# ------------------------------------------------------------------ 6. eta = 0 is today's path
def test_eta_zero_is_the_deterministic_sampler(dev):
    net, x = wide_net(), _start(dev)
    out = adp.VStochasticSampler(net, eta=0.0)(x, num_steps=STEPS, seed=SEED)
    assert torch.equal(out, adp.VSampler(net)(x, num_steps=STEPS))
    for q in (0.0, 0.9):
        out = adp.VStochasticSampler(net, eta=0.0, dynamic_threshold=q)(x, num_steps=STEPS)
        assert torch.equal(out, adp.VThresholdSampler(net, dynamic_threshold=q, order=1)(x, num_steps=STEPS)), q


# ------------------------------------------------------------------ 7. statistics on a problem with a known answer
STAT_S, STAT_STEPS, STAT_SHAPE = 0.3, 20, (4, 2, 8192)
STAT_TOL = 5 * sqrt(2 / 65536)   # five standard deviations of a sample variance over 65536 values: 2.8 %


def analytic_variance(eta, s=STAT_S, steps=STAT_STEPS):
    """Elementwise variance of the scheme's output for x ~ N(0, 1) and the optimal v of N(0, s**2) data, v = g x: every
    step is x <- m_i x + cz_i z, so var <- m_i^2 var + cz_i^2."""
    sigmas = torch.linspace(1.0, 0.0, steps + 1)
    table = coef_table(sigmas, eta)
    phi = sigmas.double() * (pi / 2)
    var = 1.0
    for i in range(steps):
        a0, b0, a1, ce, cz = table[i].tolist()
        c, sn = torch.cos(phi[i]).item(), torch.sin(phi[i]).item()
        g = c * sn * (1 - s * s) / (c * c * s * s + sn * sn)
        m = a1 * (a0 - b0 * g) + ce * (b0 + a0 * g)
        var = m * m * var + cz * cz
    return var


def test_output_variance_is_the_schemes_own(dev):
    want, plain = analytic_variance(1.0), analytic_variance(0.0)
    assert abs(want - 0.06013) < 5e-5 and abs(plain - 0.07186) < 5e-5   # the figures of the design note
    assert abs(plain / want - 1) > 2 * STAT_TOL                          # the test can tell the two apart
    net = GaussianV(STAT_S)
    x = torch.randn(STAT_SHAPE, generator=torch.Generator().manual_seed(11)).to(dev)
    loop = stochastic_ref(net, x, STAT_STEPS, 1.0, SEED).var().item()
    print(f"variance: analytic {want:.5f} (eta = 0: {plain:.5f}); float64 loop {loop:.5f}; bound {STAT_TOL:.4f} relative")
    assert abs(loop / want - 1) <= STAT_TOL and abs(loop / plain - 1) > STAT_TOL
    got = adp.VStochasticSampler(net, eta=1.0)(x, num_steps=STAT_STEPS, seed=SEED).double().var().item()
    print(f"variance: product {got:.5f}")
    assert abs(got / want - 1) <= STAT_TOL and abs(got / plain - 1) > STAT_TOL


# ------------------------------------------------------------------ 8. replay
@pytest.mark.gpu
def test_replay_equals_eager(hip):
    net, x = tiny_net(hip), _start(hip)
    g = adp.VStochasticSampler(net, eta=1.0, dynamic_threshold=0.9)
    e = adp.VStochasticSampler(net, eta=1.0, dynamic_threshold=0.9, use_graph=False)
    out = g(x, num_steps=STEPS, seed=7)
    assert torch.equal(out, e(x, num_steps=STEPS, seed=7)) and torch.equal(out, g(x, num_steps=STEPS, seed=7))
    other = g(x, num_steps=STEPS, seed=8)
    assert torch.equal(other, e(x, num_steps=STEPS, seed=8)) and not torch.equal(other, out)
    g.eta = e.eta = 0.5
    half = g(x, num_steps=6, seed=7)
    assert torch.equal(half, e(x, num_steps=6, seed=7)) and not torch.equal(half, out)
    assert g.graph_captures == 1 and g.graph_replays == 4 and len(g._graph_cache) == 1 and e.graph_captures == 0
    entry = next(iter(g._graph_cache.values()))
    assert len(entry.bufs) == 2 and entry.bufs[0].shape == (2,) and entry.sab.dtype == torch.int32
    # eta = 0 and another threshold are other steps
    g.eta = e.eta = 0.0
    assert torch.equal(g(x, num_steps=STEPS), e(x, num_steps=STEPS)) and g.graph_captures == 2
    g.eta = e.eta = 1.0
    g.dynamic_threshold = e.dynamic_threshold = None
    assert torch.equal(g(x, num_steps=STEPS, seed=7), e(x, num_steps=STEPS, seed=7)) and g.graph_captures == 3
    g.dynamic_threshold = 0.9
    assert torch.equal(g(x, num_steps=STEPS, seed=7), out) and g.graph_captures == 3
    # a deep copy (an EMA copy) leaves the captured steps behind and captures its own
    cp = copy.deepcopy(g)
    assert len(cp._graph_cache) == 0 and cp.graph_captures == 0 and cp.eta == 1.0 and cp.dynamic_threshold == 0.9
    assert torch.equal(cp(x, num_steps=STEPS, seed=7), out) and cp.graph_captures == 1 and g.graph_captures == 3


# ------------------------------------------------------------------ 9. wrappers
def _tiny_pair(dev, **sampler_kw):
    torch.manual_seed(0)
    oracle = UNetV0Oracle(**TINY)
    kw = {f"sampler_{k}": v for k, v in sampler_kw.items()}
    model = adp.DiffusionModel(net_t=adp.UNetV0, sampler_t=adp.VStochasticSampler, **kw, **TINY)
    model.net.load_oracle_state_dict(oracle.state_dict())
    return oracle, model.to(dev)


def _on_cpu(oracle):
    """The oracle net (CPU, float32) as a net of `stochastic_ref` run on the GPU: the state lives where the draws are made."""
    def net(x, t, **kw):
        return oracle(x.cpu(), t.cpu(), **kw).to(x.device)
    return net


@pytest.mark.gpu
def test_diffusion_model_with_sampler_t(hip):
    oracle, model = _tiny_pair(hip, eta=0.5)
    assert type(model.sampler) is adp.VStochasticSampler and model.sampler.eta == 0.5
    noise = torch.randn(2, 2, 1024, generator=torch.Generator().manual_seed(4)).to(hip)
    out = model.sample(noise, num_steps=5, seed=SEED)
    assert model.sampler.graph_captures == 1
    assert rel_err(out, stochastic_ref(_on_cpu(oracle), noise, 5, 0.5, SEED)) <= PARITY_TOL


@pytest.mark.gpu
def test_upsampler_sample(hip):
    torch.manual_seed(0)
    cfg = dict(TINY)
    cfg.pop("in_channels")
    up = adp.DiffusionUpsampler(net_t=adp.UNetV0, in_channels=2, upsample_factor=4, sampler_t=adp.VStochasticSampler,
                                sampler_eta=0.5, sampler_dynamic_threshold=0.9, **cfg)
    oracle = AppendChannelsOracle(lambda **kw: UNetV0Oracle(**kw), channels=2)(in_channels=2, **cfg)
    up.net.net.load_oracle_state_dict(oracle.net.state_dict())
    up = up.to(hip)
    low = torch.randn(2, 2, 256, generator=torch.Generator().manual_seed(9))
    cond = ovd.upsample(low, 4)
    torch.manual_seed(77)
    out = up.sample(low.to(hip), num_steps=5, seed=SEED)
    torch.manual_seed(77)
    start = torch.randn(cond.shape).to(hip)
    ref = stochastic_ref(_on_cpu(oracle), start, 5, 0.5, SEED, q=0.9, append_channels=cond)
    assert out.shape == (2, 2, 1024) and rel_err(out, ref) <= PARITY_TOL


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
    ae = adp.DiffusionAE(net_t=adp.UNetV0, in_channels=2, encoder=Enc(), inject_depth=1, sampler_t=adp.VStochasticSampler,
                         sampler_eta=1.0, **cfg)
    oracle = UNetV0Oracle(in_channels=2, context_channels=[0, 3], **cfg)
    ae.net.load_oracle_state_dict(oracle.state_dict())
    ae = ae.to(hip)
    z = torch.tanh(torch.randn(2, 3, 256, generator=torch.Generator().manual_seed(6)))
    out = ae.decode(z.to(hip), num_steps=5, generator=torch.Generator(device=hip).manual_seed(5), seed=SEED)
    start = torch.randn((2, 2, 1024), device=hip, dtype=z.dtype, generator=torch.Generator(device=hip).manual_seed(5))
    ref = stochastic_ref(_on_cpu(oracle), start, 5, 1.0, SEED, channels=[None, z])
    assert out.shape == (2, 2, 1024) and rel_err(out, ref) <= PARITY_TOL


@pytest.mark.gpu
def test_classifier_free_guidance(hip):
    """embedding_scale = 5 with the thresholded stochastic step: replay equals eager, and the restatement on the oracle."""
    torch.manual_seed(0)
    inner = UNetV0Oracle(**ATTN)
    oracle = ClassifierFreeGuidanceOracle(inner, embedding_max_length=7, embedding_features=12)

    def build(use_graph):
        model = adp.DiffusionModel(net_t=adp.UNetV0, use_embedding_cfg=True, embedding_max_length=7,
                                   sampler_t=adp.VStochasticSampler, sampler_eta=1.0, sampler_dynamic_threshold=0.9,
                                   sampler_use_graph=use_graph, **ATTN)
        model.net.net.load_oracle_state_dict(inner.state_dict())
        with torch.no_grad():
            model.net.fixed_embedding.weight.copy_(oracle.fixed_embedding.weight)
        return model.to(hip)

    m_g, m_e = build(True), build(False)
    g = torch.Generator().manual_seed(4)
    x = (2 * torch.randn(3, 2, 96, generator=g)).to(hip)
    emb = torch.randn(3, 5, 12, generator=g)
    out = m_g.sample(x, num_steps=4, seed=SEED, embedding=emb.to(hip), embedding_scale=5.0)
    assert m_g.sampler.graph_captures == 1 and torch.isfinite(out).all()
    assert torch.equal(out, m_e.sample(x, num_steps=4, seed=SEED, embedding=emb.to(hip), embedding_scale=5.0))
    net = _on_cpu(lambda xx, tt: oracle(xx, tt, embedding=emb, embedding_scale=5.0))
    assert rel_err(out, stochastic_ref(net, x, 4, 1.0, SEED, q=0.9)) <= PARITY_TOL


# ------------------------------------------------------------------ 10. variation
def variation_ref(net, start, noise, num_steps, eta, seed, strength):
    sigmas = (adp.LinearSchedule()(num_steps + 1, device="cpu").to(torch.float32) * strength)
    phi = sigmas[0].double() * (pi / 2)
    x = torch.cos(phi) * start.double() + torch.sin(phi) * noise.double()
    return stochastic_ref(net, x, num_steps, eta, seed, sigmas=sigmas)


def test_variation_matches_restatement(dev, monkeypatch):
    net = wide_net()
    start, noise = _start(dev, seed=2) * 0.25, _start(dev, seed=3) * 0.5
    sampler = adp.VStochasticSampler(net, eta=0.5, use_graph=False)
    with monkeypatch.context() as m:
        _no_torch_noise(m)
        given = sampler(noise, num_steps=STEPS, seed=SEED, start=start, strength=0.5)
        drawn = sampler(None, num_steps=STEPS, seed=SEED, start=start, strength=0.5)
    errs = (rel_err(given, variation_ref(net, start, noise, STEPS, 0.5, SEED, 0.5)),
            rel_err(drawn, variation_ref(net, start, draw(SEED, 0, start), STEPS, 0.5, SEED, 0.5)))
    print(f"variation, strength 0.5: rel_err vs float64 loop {errs} (bound {LOOP_TOL:.0e})")
    assert all(e <= LOOP_TOL for e in errs) and not torch.equal(given, drawn)
    # strength = 1: the start point is the noise but for a_s = cos(float32(pi / 2)) = -4.4e-8
    full = sampler(noise, num_steps=STEPS, seed=SEED, start=start, strength=1.0)
    assert rel_err(full, sampler(noise, num_steps=STEPS, seed=SEED)) <= 1e-6


# ------------------------------------------------------------------ 11. one full-size case
@pytest.mark.gpu
def test_full_size(hip):
    torch.manual_seed(0)
    net = adp.UNetV0(dim=1, **FULL).to(hip).eval()
    x = torch.randn(1, 2, 2 ** 18, generator=torch.Generator().manual_seed(0)).to(hip)
    g = adp.VStochasticSampler(net, eta=1.0, dynamic_threshold=0.995)
    out = g(x, num_steps=4, seed=SEED)
    assert out.shape == x.shape and torch.isfinite(out).all() and g.graph_captures == 1
    e = adp.VStochasticSampler(net, eta=1.0, dynamic_threshold=0.995, use_graph=False)
    assert torch.equal(out, e(x, num_steps=4, seed=SEED))
