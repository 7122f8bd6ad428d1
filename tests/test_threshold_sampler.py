"""Dynamic thresholding: `diffusion.clip` / `pad_dims`, the kernels of include/adp_clip.h and `VThresholdSampler`.

The contract is restated here on a sort (`quantile_ref`: torch.quantile's linear rule with its float32 rank arithmetic and
torch.lerp; `clip_ref`), pinned to the live reference's `clip` through tests/golden/clip_golden.pt (and to the reference itself
where it is present), and everything else is compared against that restatement: the GPU tests never read the reference.

Bounds.  The quantile of |x| selects two elements exactly and interpolates with three float32 roundings: 2**-22 relative, and
bit-equal where the weight is 0 or the two order statistics coincide.  The fused quantile of |a0 x - b0 v| is compared against
float64: an order statistic is 1-Lipschitz in the sup norm, so the error is at most the largest rounding error of an element,
4 * 2**-24 * max(|a0 x| + |b0 v|).  The step kernel has `tests/test_multistep_sampler.py`'s count of roundings (KERNEL_TOL)."""
import copy
import os

import pytest
import torch

import audio_diffusion_pytorch_amd as adp
from audio_diffusion_pytorch_amd import _C, diffusion, ops
from conftest import rel_err
from oracle import vdiffusion as ovd
from oracle.a_unet_restatement import AppendChannelsOracle, ClassifierFreeGuidanceOracle, UNetV0Oracle
from oracle.reference_loader import load_reference, reference_available
from test_multistep_sampler import KERNEL_TOL, PARITY_TOL, coef_table
from test_stft_loss import TINY
from test_unet import ATTN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_golden.pt")
LERP_TOL = 2.0 ** -22   # three float32 roundings of 2**-24 in torch.lerp's formula, relative to the result
CLIP_TOL = 2.0 ** -21   # the scale's LERP_TOL and one division, relative to the largest output


# ------------------------------------------------------------------ the restatement
def rank_of(q: float, per: int):
    """(lo, hi, w) of torch.quantile's linear rule: the rank is formed in float32."""
    rank = torch.tensor(q, dtype=torch.float32) * torch.tensor(per - 1, dtype=torch.float32)
    lo = torch.floor(rank)
    w = rank - lo
    return int(lo), int(lo) + int(w > 0), w


def quantile_ref(a: torch.Tensor, q: float) -> torch.Tensor:
    """Per-row q-quantile of a [rows, per] (float32 or float64) on a sort; NaN for a row that holds a NaN."""
    lo, hi, w = rank_of(q, a.shape[1])
    s = a.sort(dim=1).values
    out = torch.lerp(s[:, lo], s[:, hi], w.to(a.dtype))
    return torch.where(torch.isnan(a).any(dim=1), torch.full_like(out, float("nan")), out)


def clip_ref(x: torch.Tensor, q: float):
    """(clip(x, q), scale [B]): the reference's `clip` restated; float32 in, float32 out (float64 in, float64 out)."""
    if q == 0.0:
        return x.clamp(-1.0, 1.0), torch.ones(x.shape[0], dtype=x.dtype)
    scale = quantile_ref(x.flatten(1).abs(), q).clamp(min=1.0)
    s = diffusion.pad_dims(scale, x.ndim - 1)
    return x.clamp(-s, s) / s, scale


def threshold_step_ref(x, v, hx, he, row, scale):
    """One update in float64: (x_next, clipped x0, eps); `scale` [B] or None (static clamp).  eps from the raw v."""
    x, v = x.double(), v.double()
    a0, b0, a1, b1 = [r.double() for r in row[:4]]
    ca, cb = (row[4].double(), row[5].double()) if len(row) == 6 else (0.0, 0.0)
    x0, eps = a0 * x - b0 * v, b0 * x + a0 * v
    if scale is None:
        x0c = x0.clamp(-1.0, 1.0)
    else:
        s = diffusion.pad_dims(scale.double(), x.ndim - 1)
        x0c = x0.clamp(-s, s) / s
    xn = a1 * x0c + b1 * eps
    if ca != 0 or cb != 0:
        xn = xn + ca * (x0c - hx.double()) + cb * (eps - he.double())
    return xn, x0c, eps


@torch.no_grad()
def threshold_ref(net, x, num_steps, q, order, stats=None, **kw):
    """The sampler in float64 (state, coefficients, quantile); `net` runs in float32 on the CPU, as the oracle does.
    `stats`, a list, receives per step (scale [B], fraction of elements left unclamped per item [B], max |x0|)."""
    sigmas = adp.LinearSchedule()(num_steps + 1, device="cpu").to(torch.float32)
    table = coef_table(sigmas)
    x = x.double().cpu()
    hx = he = torch.zeros_like(x)
    for i in range(num_steps):
        v = net(x.float(), sigmas[i].expand(x.shape[0]), **kw).double()
        row = table[i] if order == 2 else table[i][:4]
        x0 = row[0] * x - row[1] * v
        scale = clip_ref(x0, q)[1]
        if stats is not None:
            inside = (x0.flatten(1).abs() < scale[:, None]).double().mean(dim=1)
            stats.append((scale.clone(), inside, x0.abs().max().item()))
        x, hx, he = threshold_step_ref(x, v, hx, he, row, None if q == 0.0 else scale)
    return x


# ------------------------------------------------------------------ 1. restatement vs reference
def test_restatement_equals_the_reference_clip():
    gold = torch.load(GOLDEN)
    D = load_reference()[0] if reference_available() else None
    for name in ("bct", "bt"):
        x = gold[f"{name}/x"]
        for q in gold["thresholds"].tolist():
            mine = clip_ref(x, q)[0]
            assert torch.equal(mine, gold[f"{name}/clip/{q}"]), (name, q)
            if D is not None:
                assert torch.equal(mine, D.clip(x.clone(), dynamic_threshold=q)), (name, q)
    assert diffusion.pad_dims(torch.zeros(3), 2).shape == (3, 1, 1)
    if D is not None:
        assert D.pad_dims(torch.zeros(3, 2), 1).shape == diffusion.pad_dims(torch.zeros(3, 2), 1).shape


# ------------------------------------------------------------------ 2. quantile kernel on |x|
LENGTHS = [1, 2, 3, 7, 1000, 4099, 65537]   # (a workgroup's span is 4096 values: 65537 merges 17 workgroups per row)
QS = [1e-3, 0.5, 0.995, 1.0]
KINDS = ("gauss", "equal", "zero", "shared", "straddle", "denormal", "negative")
TRIPLES = (("gauss", "equal", "straddle"), ("zero", "shared", "denormal"), ("negative", "straddle", "gauss"))


def values(kind: str, per: int, q: float, g: torch.Generator) -> torch.Tensor:
    if kind == "gauss":
        return torch.randn(per, generator=g) * 2
    if kind == "equal":
        return torch.full((per,), 0.75)
    if kind == "zero":
        return torch.zeros(per)
    perm = torch.randperm(per, generator=g)
    if kind == "shared":     # keys that differ in their low bits only
        return (1.0 + torch.arange(per, dtype=torch.float64) * 2.0 ** -23).to(torch.float32)[perm]
    if kind == "straddle":   # lo is the last zero, hi the first 3.0: the two ranks part in the first pass
        lo = rank_of(q, per)[0]
        return torch.cat([torch.zeros(lo + 1), torch.full((per - lo - 1,), 3.0)])[perm]
    if kind == "denormal":
        pool = torch.tensor([1e-40, -1e-40, -0.0])
        return pool[torch.randint(0, 3, (per,), generator=g)]
    if kind == "negative":
        return -(torch.rand(per, generator=g) * 1e30 + 1e20)
    raise KeyError(kind)


def rows_of(triple, per, q, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + per)
    return torch.stack([values(k, per, q, g) for k in triple])


def check_quantile(scale, a, q, what):
    """scale against torch.quantile of a [rows, per] (non-negative): LERP_TOL relative; equal where nothing is interpolated."""
    want = torch.quantile(a, q, dim=-1)
    lo, hi, w = rank_of(q, a.shape[1])
    s = a.sort(dim=1).values
    exact = (s[:, lo] == s[:, hi]) | bool(w == 0)
    scale = scale.cpu()
    rel = ((scale - want).abs() / want.abs().clamp_min(torch.finfo(torch.float32).tiny)).masked_fill(scale == want, 0.0)
    print(f"{what}: relative difference to torch.quantile {rel.tolist()} (bound {LERP_TOL:.3e}), exact rows {exact.tolist()}")
    assert bool((rel <= LERP_TOL).all()), (what, scale.tolist(), want.tolist())
    assert torch.equal(scale[exact], want[exact]), (what, scale.tolist(), want.tolist())


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("per", LENGTHS)
def test_quantile_of_abs_x(dev, per, q):
    assert set(k for t in TRIPLES for k in t) == set(KINDS)
    for triple in TRIPLES:
        x = rows_of(triple, per, q)
        scale = ops.clip_scale(x.to(dev), q, min_scale=0.0)
        check_quantile(scale, x.abs(), q, f"per={per} q={q} {triple}")
        # the sampler's floor
        floored = ops.clip_scale(x.to(dev), q, min_scale=1.0).cpu()
        assert torch.equal(floored, scale.cpu().clamp(min=1.0))


@pytest.mark.parametrize("per", [7, 4099])
def test_a_nan_marks_its_row_only(dev, per):
    for q in (0.5, 0.995):
        x = rows_of(TRIPLES[0], per, q)
        clean = ops.clip_scale(x.to(dev), q, min_scale=0.0).cpu()
        x[0, per // 2] = float("nan")
        got = ops.clip_scale(x.to(dev), q, min_scale=0.0).cpu()
        assert torch.isnan(got[0]) and torch.equal(got[1:], clean[1:])


def test_infinities_do_not_stall_the_select(dev):
    x = rows_of(TRIPLES[0], 1000, 0.5)
    x[0, 3], x[1, 5] = float("inf"), float("-inf")
    got = ops.clip_scale(x.to(dev), 0.5, min_scale=0.0).cpu()
    assert torch.equal(got, torch.quantile(x.abs(), 0.5, dim=-1))


# ------------------------------------------------------------------ 3. fused quantile of |a0 x - b0 v|
@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("per", LENGTHS)
def test_fused_quantile(dev, per, q):
    g = torch.Generator().manual_seed(per)
    x, v = torch.randn(3, per, generator=g) * 2, torch.randn(3, per, generator=g)
    coef = torch.tensor([0.8910065, 0.4539905, 0.9, 0.43])   # (a0, b0, ...): only the first two are read
    a0, b0 = coef[0].double(), coef[1].double()
    want = quantile_ref((a0 * x.double() - b0 * v.double()).abs(), q)
    bound = 4 * 2.0 ** -24 * ((a0 * x.double()).abs() + (b0 * v.double()).abs()).max().item()
    scale = ops.clip_scale(x.to(dev), q, v=v.to(dev), coef=coef.to(dev), min_scale=0.0)
    err = (scale.cpu().double() - want).abs().max().item()
    print(f"fused quantile per={per} q={q}: abs error {err:.3e} (bound {bound:.3e})")
    assert err <= bound


# ------------------------------------------------------------------ 4. statelessness
def test_workspace_needs_no_initialising_and_keeps_nothing(dev):
    q = 0.995
    x, y = rows_of(TRIPLES[0], 4099, q).to(dev), rows_of(TRIPLES[2], 1000, q, seed=1).to(dev)
    ws = ops.clip_ws(x)
    assert ws.numel() * 4 >= _C.query("adp_clip_ws_bytes", 3, 1000)
    results = []
    for t in (x, x, y, x):
        scale = torch.empty(3, device=dev)
        if len(results) != 1:   # (the second call finds what the first one left)
            ws.view(torch.int32).fill_(-1)
        scale.view(torch.int32).fill_(-1)
        results.append(ops.clip_scale(t, q, min_scale=0.0, ws=ws, out=scale).cpu().clone())
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[3])
    check_quantile(results[2], y.cpu().abs(), q, "another length in the same workspace")
    assert torch.equal(results[0], ops.clip_scale(x, q, min_scale=0.0).cpu())


# ------------------------------------------------------------------ 5. step kernel
def _step_case(shape, order, seed=0):
    g = torch.Generator().manual_seed(seed + shape[-1])
    x, v, hx, he = [torch.randn(shape, generator=g) * 1.5 for _ in range(4)]
    row = coef_table(torch.tensor([0.62, 0.55, 0.5]))[1].to(torch.float32)
    scale = torch.tensor([1.0, 1.7, 2.5][:shape[0]])
    return x, v, hx, he, (row if order == 2 else row[:4].contiguous()), scale


@pytest.mark.parametrize("dynamic", [True, False], ids=["scale", "static"])
@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("shape", [(3, 1), (2, 3, 683), (2, 2, 1024)], ids=str)
def test_step_kernel_matches_restatement(dev, shape, order, inplace, dynamic):
    x, v, hx, he, row, scale = _step_case(shape, order)
    ref = threshold_step_ref(x, v, hx, he, row, scale if dynamic else None)
    assert (ref[1].abs() == 1).any() or shape[-1] == 1   # something is clipped
    dx, dv, dhx, dhe, drow = [t.to(dev) for t in (x, v, hx, he, row)]
    dscale = scale.to(dev) if dynamic else None
    if order == 1:
        out = ops.clip_step(dx, dv, drow, dscale, out=dx if inplace else None)
        outs, refs = (out,), ref[:1]
        assert (out is dx) == inplace
    elif inplace:
        outs = ops.clip_step(dx, dv, drow, dscale, dhx, dhe, out=dx, hist_x0_out=dhx, hist_eps_out=dhe)
        refs = ref
        assert outs[0] is dx and outs[1] is dhx and outs[2] is dhe
    else:
        outs, refs = ops.clip_step(dx, dv, drow, dscale, dhx, dhe), ref
        assert torch.equal(dhx.cpu(), hx) and torch.equal(dx.cpu(), x)
    errs = [rel_err(o, r) for o, r in zip(outs, refs)]
    print(f"adp_clip_step {shape} order {order}: rel_err {errs} (bound {KERNEL_TOL:.0e})")
    assert all(e <= KERNEL_TOL for e in errs), errs


@pytest.mark.parametrize("shape", [(2, 3, 683), (2, 2, 1024)], ids=str)
def test_first_step_does_not_read_the_history(dev, shape):
    x, v, _, _, row, scale = _step_case(shape, 2)
    row = row.clone()
    row[4:] = 0.0
    nan = torch.full(shape, float("nan"))
    xo, hxo, heo = ops.clip_step(x.to(dev), v.to(dev), row.to(dev), scale.to(dev), nan.to(dev), nan.to(dev))
    ref = threshold_step_ref(x, v, nan, nan, row, scale)
    assert all(torch.isfinite(t).all() for t in (xo, hxo, heo))
    assert all(rel_err(o, r) <= KERNEL_TOL for o, r in zip((xo, hxo, heo), ref))


# ------------------------------------------------------------------ 6. diffusion.clip
def test_clip_matches_restatement(dev):
    gold = torch.load(GOLDEN)
    for name in ("bct", "bt"):
        x = gold[f"{name}/x"]
        for q in gold["thresholds"].tolist():
            got = diffusion.clip(x.to(dev), dynamic_threshold=q)
            want = clip_ref(x, q)[0]
            err = rel_err(got, want)
            print(f"clip {name} q={q}: rel_err {err:.3e} (bound {CLIP_TOL:.3e})")
            assert got.shape == x.shape and err <= CLIP_TOL
            if q == 0.0:
                assert torch.equal(got.cpu(), want)
    with pytest.raises(ValueError):
        diffusion.clip(gold["bt/x"].to(dev), dynamic_threshold=1.5)


# ------------------------------------------------------------------ 7. sampler vs a float64 loop
STEPS, SEED = 6, 1
# A freshly initialised TINY net is close to the identity (v = x + 0.08 at most), whatever the seed: x0 = (a - b) x then
# shrinks below 1 after two steps and the threshold idles.  The output convolution is scaled so that the prediction keeps a
# component of its own; 20 was picked on the CPU, from the restatement alone, as the smallest round gain at which the scale
# exceeds 1 by a clear margin (1.3) in half of the (step, item) pairs -- the test asserts that condition before it compares.
OUT_GAIN = 20.0


def _tiny_pair(dev, sampler_t=None, gain=OUT_GAIN, **sampler_kw):
    torch.manual_seed(0)
    oracle = UNetV0Oracle(**TINY)
    with torch.no_grad():
        oracle.blocks[0].up.weight.mul_(gain)
        oracle.blocks[0].up.bias.mul_(gain)
    kw = {f"sampler_{k}": v for k, v in sampler_kw.items()}
    model = adp.DiffusionModel(net_t=adp.UNetV0, sampler_t=sampler_t or adp.VThresholdSampler, **kw, **TINY)
    model.net.load_oracle_state_dict(oracle.state_dict())
    return oracle, model.to(dev)


def _start(seed=SEED):
    return 2 * torch.randn(2, 2, 256, generator=torch.Generator().manual_seed(seed))


_REFS = {}


def sampler_reference(q, order):
    """(float64 result, per-step stats) of the restatement for the shared start noise; computed once."""
    if (q, order) not in _REFS:
        stats = []
        oracle, _ = _tiny_pair("cpu")
        _REFS[(q, order)] = (threshold_ref(oracle, _start(), STEPS, q, order, stats), stats)
    return _REFS[(q, order)]


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("q", [0.9, 0.0])
def test_sampler_matches_float64_loop(dev, q, order):
    ref, stats = sampler_reference(q, order)
    # the condition under which this test says anything: the threshold is at work in most steps, and never clips everything
    if q > 0:
        active = sum(int(s > 1) for scale, _, _ in stats for s in scale.tolist())
        assert 2 * active >= STEPS * 2, [scale.tolist() for scale, _, _ in stats]
    else:
        assert sum(int(m > 1) for _, _, m in stats) * 2 >= STEPS
    assert all(0 < f for _, inside, _ in stats for f in inside.tolist())
    _, model = _tiny_pair(dev, dynamic_threshold=q, order=order)
    assert type(model.sampler) is adp.VThresholdSampler
    out = model.sample(_start().to(dev), num_steps=STEPS)
    err = rel_err(out, ref)
    print(f"VThresholdSampler q={q} order={order}: rel_err vs float64 loop {err:.3e} (bound {PARITY_TOL:.0e}); "
          f"scales {[[round(s, 3) for s in scale.tolist()] for scale, _, _ in stats]}")
    assert out.shape == ref.shape and err <= PARITY_TOL


def test_nothing_to_clip_is_the_plain_sampler(dev):
    """Control: where every |x0| stays below 1 the threshold changes nothing.  The start is 0.12 of the usual one: the largest
    round factor at which the restatement keeps max |x0| below 1 with a margin (0.85).  Smaller is worse, not safer: the
    net's normalisation layers make it ill-conditioned on small inputs (at 0.05 a one-ulp change of the start moves
    `VSampler`'s own result by 5e-6, above the bound; here by 1e-6)."""
    small = 0.12 * _start(seed=3)
    stats = []
    oracle, model = _tiny_pair(dev, gain=1.0, dynamic_threshold=0.9)   # (the net as initialised: close to the identity)
    threshold_ref(oracle, small, STEPS, 0.9, 1, stats)
    assert all(m < 1 for _, _, m in stats), [m for _, _, m in stats]
    _, plain = _tiny_pair(dev, sampler_t=adp.VSampler, gain=1.0)
    _, static = _tiny_pair(dev, gain=1.0, dynamic_threshold=0.0)
    want = plain.sample(small.to(dev), num_steps=STEPS)
    assert rel_err(model.sample(small.to(dev), num_steps=STEPS), want) <= KERNEL_TOL
    assert rel_err(static.sample(small.to(dev), num_steps=STEPS), want) <= KERNEL_TOL


# ------------------------------------------------------------------ 8. replay
@pytest.mark.gpu
def test_replay_equals_eager(hip):
    _, m_g = _tiny_pair(hip, dynamic_threshold=0.9, order=2)
    _, m_e = _tiny_pair(hip, dynamic_threshold=0.9, order=2, use_graph=False)
    noise = _start().to(hip)
    out6, out3 = m_g.sample(noise, num_steps=6), m_g.sample(noise, num_steps=3)
    assert m_g.sampler.graph_captures == 1 and m_g.sampler.graph_replays == 2 and len(m_g.sampler._graph_cache) == 1
    assert m_e.sampler.graph_captures == 0
    assert torch.equal(out6, m_e.sample(noise, num_steps=6)) and torch.equal(out3, m_e.sample(noise, num_steps=3))
    assert torch.equal(m_g.sample(noise, num_steps=6), out6), "state of the previous run leaked into this one"
    entry = next(iter(m_g.sampler._graph_cache.values()))
    assert len(entry.bufs) == 4 and entry.bufs[0].shape == (2,)   # scale, workspace, history: owned by the entry
    # a second threshold is a second captured step; the first one is kept
    m_g.sampler.dynamic_threshold = m_e.sampler.dynamic_threshold = 0.5
    other = m_g.sample(noise, num_steps=6)
    assert m_g.sampler.graph_captures == 2 and len(m_g.sampler._graph_cache) == 2
    assert torch.equal(other, m_e.sample(noise, num_steps=6)) and not torch.equal(other, out6)
    m_g.sampler.dynamic_threshold = 0.9
    assert torch.equal(m_g.sample(noise, num_steps=6), out6) and m_g.sampler.graph_captures == 2
    # the static clamp launches no quantile and owns no scale
    m_g.sampler.dynamic_threshold = m_e.sampler.dynamic_threshold = 0.0
    assert torch.equal(m_g.sample(noise, num_steps=6), m_e.sample(noise, num_steps=6))
    assert m_g.sampler.graph_captures == 3
    # a deep copy (an EMA copy) leaves the captured steps behind and captures its own
    m_g.sampler.dynamic_threshold = 0.9
    cp = copy.deepcopy(m_g)
    assert len(cp.sampler._graph_cache) == 0 and cp.sampler.graph_captures == 0
    assert cp.sampler.order == 2 and cp.sampler.dynamic_threshold == 0.9
    assert torch.equal(cp.sample(noise, num_steps=6), out6) and cp.sampler.graph_captures == 1


@pytest.mark.gpu
def test_classifier_free_guidance_stays_bounded(hip):
    """embedding_scale = 5 pushes x0 far outside [-1, 1]; the thresholded x0 of every step keeps its 0.9-quantile at 1."""
    def build(use_graph):
        torch.manual_seed(0)
        model = adp.DiffusionModel(net_t=adp.UNetV0, use_embedding_cfg=True, embedding_max_length=7,
                                   sampler_t=adp.VThresholdSampler, sampler_dynamic_threshold=0.9, sampler_order=2,
                                   sampler_use_graph=use_graph, **ATTN)
        return model.to(hip)

    m_g, m_e = build(True), build(False)
    g = torch.Generator().manual_seed(4)
    x = (2 * torch.randn(3, 2, 96, generator=g)).to(hip)
    emb = torch.randn(3, 5, 12, generator=g).to(hip)
    seen = []
    step = m_e.sampler._step

    def recording(xx, v, row, bufs, out):
        r = step(xx, v, row, bufs, out)
        seen.append(bufs[2].clone())   # the history now holds this step's clipped x0
        return r

    m_e.sampler._step = recording
    eager = m_e.sample(x, num_steps=5, embedding=emb, embedding_scale=5.0)
    out = m_g.sample(x, num_steps=5, embedding=emb, embedding_scale=5.0)
    assert m_g.sampler.graph_captures == 1 and torch.isfinite(out).all() and torch.equal(out, eager)
    assert len(seen) == 5
    for x0c in seen:
        assert bool((torch.quantile(x0c.flatten(1).abs().cpu(), 0.9, dim=-1) <= 1).all())
        assert x0c.abs().max().item() <= 1


# ------------------------------------------------------------------ 9. routing and errors
def test_diffusion_model_routes_the_threshold(dev):
    _, model = _tiny_pair(dev, dynamic_threshold=0.9)
    assert type(model.sampler) is adp.VThresholdSampler and model.sampler.dynamic_threshold == 0.9
    assert model.sampler.order == 1
    out = model.sample(_start()[:, :, :64].contiguous().to(dev), num_steps=2)
    assert out.shape == (2, 2, 64) and torch.isfinite(out).all()
    assert "VThresholdSampler" in adp.__all__ and issubclass(adp.VThresholdSampler, adp.VMultistepSampler)


@pytest.mark.gpu
def test_upsampler_sample(hip):
    torch.manual_seed(0)
    cfg = dict(TINY)
    cfg.pop("in_channels")
    up = adp.DiffusionUpsampler(net_t=adp.UNetV0, in_channels=2, upsample_factor=4, sampler_t=adp.VThresholdSampler,
                                sampler_dynamic_threshold=0.9, **cfg)
    oracle = AppendChannelsOracle(lambda **kw: UNetV0Oracle(**kw), channels=2)(in_channels=2, **cfg)
    up.net.net.load_oracle_state_dict(oracle.net.state_dict())
    up = up.to(hip)
    low = torch.randn(2, 2, 512, generator=torch.Generator().manual_seed(9))
    cond = ovd.upsample(low, 4)
    torch.manual_seed(77)
    out = up.sample(low.to(hip), num_steps=5)
    torch.manual_seed(77)
    ref = threshold_ref(oracle, torch.randn(cond.shape), 5, 0.9, 1, append_channels=cond)
    assert out.shape == (2, 2, 2048) and rel_err(out, ref) <= PARITY_TOL


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
    ae = adp.DiffusionAE(net_t=adp.UNetV0, in_channels=2, encoder=Enc(), inject_depth=1, sampler_t=adp.VThresholdSampler,
                         sampler_dynamic_threshold=0.9, sampler_order=2, **cfg)
    oracle = UNetV0Oracle(in_channels=2, context_channels=[0, 3], **cfg)
    ae.net.load_oracle_state_dict(oracle.state_dict())
    ae = ae.to(hip)
    z = torch.tanh(torch.randn(2, 3, 256, generator=torch.Generator().manual_seed(6)))
    out = ae.decode(z.to(hip), num_steps=5, generator=torch.Generator(device=hip).manual_seed(5))
    start = torch.randn((2, 2, 1024), device=hip, dtype=z.dtype, generator=torch.Generator(device=hip).manual_seed(5))
    ref = threshold_ref(oracle, start.cpu(), 5, 0.9, 2, channels=[None, z])
    assert out.shape == (2, 2, 1024) and rel_err(out, ref) <= PARITY_TOL


def test_bad_arguments_raise(emul):
    net = torch.nn.Identity()
    for bad in (-0.1, 1.5, float("nan"), "0.9", None, True):
        with pytest.raises(ValueError):
            adp.VThresholdSampler(net, dynamic_threshold=bad)
    for bad in (0, 3, "2"):
        with pytest.raises(ValueError):
            adp.VThresholdSampler(net, order=bad)
    s = adp.VThresholdSampler(net)
    assert s.dynamic_threshold == 0.995 and s.order == 1 and s.use_graph
    # more values per item than float32 counts exactly: refused from the shape alone, before anything is touched
    huge = torch.empty(1, 2 ** 24 + 1, device="meta")
    for call in (lambda: ops.clip_scale(huge, 0.5), lambda: ops.clip_ws(huge), lambda: ops.clip_apply(huge, huge),
                 lambda: ops.clip_step(huge, huge, huge)):
        with pytest.raises(ValueError, match="2\\*\\*24"):
            call()
    assert _C.lib().adp_clip_ws_bytes(1, 2 ** 24 + 1) == -1 and _C.lib().adp_clip_ws_bytes(1, 2 ** 24) > 0
    x = torch.zeros(2, 8)
    with pytest.raises(ValueError):
        ops.clip_scale(x, 1.5)
    with pytest.raises(ValueError):
        ops.clip_scale(x, 0.5, v=x)                       # v without its coefficients
    with pytest.raises(ValueError):
        ops.clip_scale(x, 0.5, v=torch.zeros(2, 4), coef=torch.zeros(4))
    with pytest.raises(ValueError):
        ops.clip_scale(x, 0.5, ws=torch.zeros(8))         # a workspace that is too small
    with pytest.raises(ValueError):
        ops.clip_apply(x, torch.ones(3))
    with pytest.raises(ValueError):
        ops.clip_step(x, x, torch.zeros(5))
    with pytest.raises(ValueError):
        ops.clip_step(x, x, torch.zeros(6))               # second order without a history
    with pytest.raises(ValueError):
        ops.clip_step(x, x, torch.zeros(4), hist_x0=x, hist_eps=x)


def test_c_abi_returns_error_codes(dev):
    L = _C.lib()
    s = _C.stream()
    x = torch.zeros(2, 16, device=dev)
    scale, coef = torch.ones(2, device=dev), torch.zeros(6, device=dev)
    ws = ops.clip_ws(x)
    p = lambda t, off=0: ctypes_ptr(t, off)
    assert L.adp_clip_scale(None, None, None, 2, 16, 0, 0.0, 1.0, p(ws), p(scale), s) == -5
    assert L.adp_clip_scale(p(x), p(x), None, 2, 16, 0, 0.0, 1.0, p(ws), p(scale), s) == -5
    assert L.adp_clip_scale(p(x), None, None, 2, 16, 16, 0.0, 1.0, p(ws), p(scale), s) == -1
    assert L.adp_clip_scale(p(x), None, None, 2, 16, 15, 0.5, 1.0, p(ws), p(scale), s) == -1
    assert L.adp_clip_scale(p(x), None, None, 2, 16, 0, 1.0, 1.0, p(ws), p(scale), s) == -1
    assert L.adp_clip_scale(p(x), None, None, 2, 2 ** 24 + 1, 0, 0.0, 1.0, p(ws), p(scale), s) == -1
    assert L.adp_clip_scale(p(x), None, None, 65536, 1, 0, 0.0, 1.0, p(ws), p(scale), s) == -2
    assert L.adp_clip_scale(p(x, 2), None, None, 2, 4, 0, 0.0, 1.0, p(ws), p(scale), s) == -3
    assert L.adp_clip_scale(p(x), None, None, 0, 16, 0, 0.0, 1.0, p(ws), p(scale), s) == 0
    assert L.adp_clip_apply(p(x), None, 2, 16, p(x), s) == -5 and L.adp_clip_apply(p(x), p(scale), 2, -1, p(x), s) == -1
    assert L.adp_clip_apply(p(x), p(scale, 1), 2, 4, p(x), s) == -3
    assert L.adp_clip_step(p(x), p(x), None, None, p(coef), 2, p(scale), 2, 16, p(x), None, None, s) == -5
    assert L.adp_clip_step(p(x), p(x), None, None, p(coef), 3, p(scale), 2, 16, p(x), None, None, s) == -1
    assert L.adp_clip_step(p(x), p(x), None, None, p(coef), 1, p(scale), 2, 4, p(x, 2), None, None, s) == -3
    assert L.adp_clip_step(p(x), p(x), None, None, p(coef), 1, None, 2, 16, p(x), None, None, s) == 0
    assert torch.equal(x.cpu(), torch.zeros(2, 16)) and torch.equal(scale.cpu(), torch.ones(2))


def ctypes_ptr(t, byte_offset=0):
    return t.data_ptr() + byte_offset
