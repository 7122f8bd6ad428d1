"""Autoregressive v-diffusion (audio_diffusion_pytorch_amd/ar.py, include/adp_ar.h): the three kernels against fp64 formulas,
parity with the reference's ARVDiffusion / ARVSampler from tests/golden/ar_golden.pt (tools/make_ar_golden.py), the public
interface, and the graph-replayed sampler / training step on the GPU."""
import copy
import math
import os

import pytest
import torch
import torch.nn as nn

import audio_diffusion_pytorch_amd as adp
from audio_diffusion_pytorch_amd import _C, graphed, ops
from conftest import rel_err
from oracle.a_unet_restatement import UNetV0Oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ar_golden.pt")
KERNEL_TOL = 1e-6   # test_kernels.py::test_v_noise_mse_step's bound on v_noise / v_step
TOL = 1e-3          # the project's parity contract (test_unet.TOL, test_full_parity's 50 VSampler steps)

# (B, C, T, N): l = 6 and 7 are not multiples of 4, T = 24 / 35 / 300 are not multiples of 256, N = 1, and a 16-byte case
SHAPES = [(2, 3, 24, 4), (2, 2, 35, 5), (1, 2, 300, 1), (3, 1, 2048, 8)]


def _ar():
    from audio_diffusion_pytorch_amd import ar
    return ar


def _golden():
    return torch.load(GOLDEN, weights_only=True)


def per_position(per_split: torch.Tensor, T: int) -> torch.Tensor:
    """[..., N] -> [..., T]: position t takes the value of split t // (T // N)."""
    return per_split.repeat_interleave(T // per_split.shape[-1], dim=-1)


def noise_ref(x, noise, sigma):
    """fp64 ARVDiffusion.forward lines 118-127: (x_noisy, v_target, sigma plane [B, 1, T])."""
    s = per_position(sigma.double(), x.shape[-1])[:, None, :]
    a, b = torch.cos(s * math.pi / 2), torch.sin(s * math.pi / 2)
    return a * x.double() + b * noise.double(), a * noise.double() - b * x.double(), s


def step_ref(x, v, coef):
    """fp64 sample_loop update (lines 231-235) with coef rows (a_i, b_i, a_{i+1}, b_{i+1}, sigma_{i+1}) per split."""
    c = per_position(coef.double().t(), x.shape[-1])   # [5, T]
    x, v = x.double(), v.double()
    return c[2] * (c[0] * x - c[1] * v) + c[3] * (c[1] * x + c[0] * v), c[4]


def case_data(B, C, T, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    x, v = torch.randn(B, C, T, generator=g), torch.randn(B, C, T, generator=g)
    sigma = torch.rand(B, N, generator=g)
    sigma[0, 0] = 0.0
    sigma[-1, -1] = 1.0
    ang = torch.rand(N, 2, generator=g) * (math.pi / 2)
    coef = torch.cat([torch.cos(ang[:, :1]), torch.sin(ang[:, :1]), torch.cos(ang[:, 1:]), torch.sin(ang[:, 1:]),
                      torch.rand(N, 1, generator=g)], dim=1).contiguous()
    coef[0] = torch.tensor([1.0, 0.0, 1.0, 0.0, 0.0])   # the context half of the ladder
    return x, v, sigma, coef


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("B,C,T,N", SHAPES)
def test_arv_kernels_against_fp64(dev, B, C, T, N):
    x, v, sigma, coef = case_data(B, C, T, N)
    xd, vd = x.to(dev), v.to(dev)
    x_noisy, v_target, plane = ops.arv_noise(xd, vd, sigma.to(dev))
    xn_ref, vt_ref, plane_ref = noise_ref(x, v, sigma)
    for name, got, want in (("x_noisy", x_noisy, xn_ref), ("v_target", v_target, vt_ref)):
        err = rel_err(got, want)
        print(f"arv_noise {name}: rel err {err:.3e}")
        assert err < KERNEL_TOL
    assert plane.shape == (B, 1, T) and torch.equal(plane.cpu(), plane_ref.float())

    out_ref, next_ref = step_ref(x, v, coef)
    next_plane = torch.full((B, 1, T), float("nan")).to(dev)
    out = ops.arv_step(xd, vd, coef.to(dev), plane_out=next_plane)
    err = rel_err(out, out_ref)
    print(f"arv_step: rel err {err:.3e}")
    assert err < KERNEL_TOL
    assert torch.equal(next_plane.cpu(), next_ref.float().expand(B, 1, T))
    l = T // N
    assert torch.equal(out[..., :l], xd[..., :l]), "a (1, 0, 1, 0, .) row must keep its split bit-identical"
    assert torch.equal(ops.arv_step(xd, vd, coef.to(dev)), out)   # plane_out is optional
    inplace = xd.clone()
    assert ops.arv_step(inplace, vd, coef.to(dev), out=inplace) is inplace
    assert torch.equal(inplace, out)
    assert torch.equal(inplace[..., :l], xd[..., :l])

    first = ops.arv_plane(sigma[0].contiguous().to(dev), B, T)
    assert torch.equal(first.cpu(), per_position(sigma[0], T).expand(B, 1, T))


def test_arv_kernels_refuse_indivisible_lengths(dev):
    B, C, T, N = 2, 2, 30, 4
    x, v, _, _ = case_data(B, C, 32, N)
    x, v = x[..., :T].contiguous().to(dev), v[..., :T].contiguous().to(dev)
    sigma, coef = torch.rand(B, N).to(dev), torch.rand(N, 5).to(dev)
    outs = [torch.full((B, C, T), 7.0).to(dev) for _ in range(2)] + [torch.full((B, 1, T), 7.0).to(dev)]
    lib, p, s = _C.lib(), _C.ptr, _C.stream()
    assert lib.adp_arv_noise(p(x), p(v), p(sigma), B, C, T, N, p(outs[0]), p(outs[1]), p(outs[2]), s) == -1
    assert lib.adp_arv_step(p(x), p(v), p(coef), B, C, T, N, p(outs[0]), p(outs[2]), s) == -1
    assert lib.adp_arv_plane(p(sigma), B, T, N, p(outs[2]), s) == -1
    assert lib.adp_arv_noise(p(x), p(v), p(sigma), B, 0, T, 2, p(outs[0]), p(outs[1]), p(outs[2]), s) == -1
    assert lib.adp_arv_step(p(x), p(v), p(coef), 0, C, T, 2, p(outs[0]), p(outs[2]), s) == -1
    assert lib.adp_arv_plane(p(sigma), B, T, 0, p(outs[2]), s) == -1
    assert lib.adp_arv_step(p(x), None, p(coef), B, C, T, 2, p(outs[0]), None, s) == -5
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs), "a refused call must leave its outputs untouched"
    with pytest.raises(ValueError):
        ops.arv_noise(x, v, sigma)
    with pytest.raises(ValueError):
        ops.arv_step(x, v, coef)
    with pytest.raises(ValueError):
        ops.arv_plane(sigma[0].contiguous(), B, T)
    with pytest.raises(ValueError):
        ops.arv_step(x, v, torch.rand(2, 4).to(dev))
    with pytest.raises(ValueError):
        ops.arv_step(x, v[:1].contiguous(), torch.rand(2, 5).to(dev))


# --------------------------------------------------------------------------------------------- parity with the reference
def _model_from(gold, dev, **extra):
    ar = _ar()
    cfg = {k: v for k, v in gold["cfg"].items() if k not in ("in_channels", "out_channels", "use_modulation",
                                                              "use_time_conditioning")}
    model = ar.DiffusionAR(net_t=adp.UNetV0, in_channels=gold["in_channels"], length=gold["length"],
                           num_splits=gold["num_splits"], **cfg, **extra)
    model.net.load_oracle_state_dict(gold["state_dict"])
    return model.to(dev)


def test_arv_diffusion_matches_the_reference(dev):
    gold = _golden()
    t = gold["train"]
    model = _model_from(gold, dev)
    x, noise, sigmas = t["x"].to(dev), t["noise"].to(dev), t["sigmas"].to(dev)
    x_noisy, v_target, plane = ops.arv_noise(x, noise, sigmas.reshape(x.shape[0], -1).contiguous())
    for name, got, want in (("x_noisy", x_noisy, t["x_noisy"]), ("v_target", v_target, t["v_target"])):
        err = rel_err(got, want)
        print(f"{name} against the reference: rel err {err:.3e}")
        assert err < KERNEL_TOL
    assert torch.equal(plane.cpu()[:, 0], per_position(t["sigmas"][:, 0], x.shape[-1]))
    loss = model(x, noise=noise, sigmas=sigmas)
    loss.backward()
    err = abs(loss.item() - t["loss"].item()) / abs(t["loss"].item())
    print(f"loss {loss.item():.7f} against the reference's {t['loss'].item():.7f}: rel err {err:.3e}")
    assert err < TOL
    # test_unet.compare_grads' conventions: every parameter, denominators floored at 1e-3 of the largest gradient
    own = {n: p.grad for n, p in model.net.named_parameters()}
    assert all(g is not None for g in own.values())
    mapped = model.net.oracle_named_grads(own)
    gmax = max(g.abs().max().item() for g in t["grads"].values())
    worst = ("", 0.0)
    for name, want in t["grads"].items():
        assert name in mapped, name
        a, b = mapped[name].detach().double().cpu(), want.double()
        e = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-3 * gmax)
        worst = max(worst, (name, e), key=lambda w: w[1])
    print(f"worst parameter gradient: {worst}")
    assert worst[1] < TOL, worst


def test_sigma_ladder_is_the_references():
    gold = _golden()
    ar = _ar()
    net = nn.Conv1d(3, 2, 1)
    assert len(gold["ladders"]) >= 3
    for lad in gold["ladders"]:
        sampler = ar.ARVSampler(net, in_channels=2, length=lad["length"], num_splits=lad["num_splits"])
        got = sampler.get_sigmas_ladder(num_items=lad["num_items"], num_steps_per_split=lad["num_steps_per_split"])
        assert got.shape == lad["sigmas"].shape == (lad["num_steps_per_split"] + 1, lad["num_items"], 1, lad["length"])
        assert torch.equal(got, lad["sigmas"]), (lad["num_splits"], lad["num_steps_per_split"])


def test_arv_sampler_matches_the_reference(dev):
    gold = _golden()
    model = _model_from(gold, dev)
    runs = gold["samples"]
    assert any(r["num_chunks"] == gold["num_splits"] for r in runs) and any(r["num_chunks"] > gold["num_splits"] for r in runs)
    for run in runs:
        args = {k: v for k, v in run.items() if k not in ("seed", "output")}
        out = model.sample(generator=torch.Generator().manual_seed(run["seed"]), **args)
        assert out.shape == run["output"].shape
        err = rel_err(out, run["output"])
        print(f"ARVSampler {args}: rel err {err:.3e}")
        assert err < TOL, (args, err)


def test_state_dict_round_trip_with_the_oracle(emul):
    gold = _golden()
    model = _model_from(gold, emul)
    oracle = UNetV0Oracle(**gold["cfg"])
    oracle.load_state_dict(gold["state_dict"])
    back = model.net.oracle_named_grads(dict(model.net.named_parameters()))
    assert set(back) == set(gold["state_dict"])
    for name, want in oracle.state_dict().items():
        assert torch.equal(back[name].detach().cpu(), want), name
    twin = adp.UNetV0(dim=1, **gold["cfg"])
    assert {n: tuple(p.shape) for n, p in twin.named_parameters()} == \
        {n: tuple(p.shape) for n, p in model.net.named_parameters()}
    # and the oracle computes what the native net computes on [x | sigma plane]
    g = torch.Generator().manual_seed(2)
    x, plane = torch.randn(2, 2, 64, generator=g), torch.rand(2, 1, 64, generator=g)
    with torch.no_grad():
        assert rel_err(model.net(x, x_append=plane), oracle(torch.cat([x, plane], dim=1))) < TOL


# -------------------------------------------------------------------------------------------------------------------- API
NET = dict(channels=[8, 16], factors=[2, 2], items=[1, 1], resnet_groups=4)


class Opaque(nn.Module):
    """A net_t whose result is not recognised as a UNetV0 (the [x | plane] tensor has to exist), around the same U-Net."""

    def __init__(self, **kwargs):
        super().__init__()
        self.kwargs = kwargs
        self.inner = adp.UNetV0(**kwargs)

    def forward(self, x, **kwargs):
        assert x.shape[1] == self.kwargs["in_channels"]
        return self.inner(x, **kwargs)


class PlainConv(nn.Module):
    def __init__(self, dim, in_channels, out_channels, **kwargs):
        super().__init__()
        self.seen = dict(kwargs, in_channels=in_channels, out_channels=out_channels)
        self.conv = nn.Conv1d(in_channels, out_channels, 3, padding=1)

    def forward(self, x):
        return torch.tanh(self.conv(x))


def test_api_and_kwarg_routing(emul):
    from audio_diffusion_pytorch_amd.ar import ARVDiffusion, ARVSampler, DiffusionAR
    model = DiffusionAR(net_t=PlainConv, in_channels=2, length=32, num_splits=4, diffusion_use_graph=False,
                        sampler_use_graph=False, some_net_option=5)
    assert isinstance(model, adp.DiffusionModel)
    assert isinstance(model.diffusion, ARVDiffusion) and isinstance(model.diffusion, adp.Diffusion)
    assert isinstance(model.sampler, ARVSampler) and isinstance(model.sampler, adp.Sampler)
    assert model.diffusion.net is model.net and model.sampler.net is model.net
    assert model.net.seen == dict(in_channels=3, out_channels=2, use_time_conditioning=False, use_modulation=False,
                                  some_net_option=5)
    d, s = model.diffusion, model.sampler
    assert (d.length, d.num_splits, d.split_length, d.use_graph) == (32, 4, 8, False)
    assert (s.length, s.num_splits, s.split_length, s.in_channels, s.use_graph) == (32, 4, 8, 2, False)
    assert not d.two_pointer and not s.two_pointer
    loss = model(torch.randn(2, 2, 32))
    loss.backward()
    assert loss.dim() == 0 and torch.isfinite(loss) and model.net.conv.weight.grad.abs().sum() > 0
    out = model.sample(num_items=2, num_chunks=6, num_steps=4, start=torch.zeros(1))   # `start` is ignored
    assert out.shape == (2, 2, 48) and torch.isfinite(out).all()
    assert model.sample(num_items=1, num_chunks=4, num_steps=2).shape == (1, 2, 32)
    # seeding: the same CPU generator state gives the same sample
    a = model.sample(num_items=1, num_chunks=5, num_steps=4, generator=torch.Generator().manual_seed(3))
    b = model.sample(num_items=1, num_chunks=5, num_steps=4, generator=torch.Generator().manual_seed(3))
    assert torch.equal(a, b)
    with pytest.raises(AssertionError, match="length must match"):
        model(torch.randn(2, 2, 16))
    with pytest.raises(AssertionError, match="divisible by num_splits"):
        ARVDiffusion(model.net, length=30, num_splits=4)
    with pytest.raises(AssertionError, match="divisible by num_splits"):
        ARVSampler(model.net, in_channels=2, length=30, num_splits=4)


def test_sampler_assertions_and_odd_splits(emul):
    ar = _ar()
    net = PlainConv(1, 3, 2)
    sampler = ar.ARVSampler(net, in_channels=2, length=32, num_splits=4)
    with pytest.raises(AssertionError, match="required at least 4 chunks"):
        sampler(num_items=1, num_chunks=3, num_steps=4)
    with pytest.raises(AssertionError, match="num_steps must be greater than num_splits"):
        sampler(num_items=1, num_chunks=5, num_steps=3)
    assert sampler(num_items=1, num_chunks=4, num_steps=3).shape == (1, 2, 32)   # without shifts any step count will do
    odd = ar.ARVSampler(net, in_channels=2, length=30, num_splits=3)
    with pytest.raises(ValueError, match="odd"):
        odd(num_items=1, num_chunks=4, num_steps=6)
    assert odd(num_items=1, num_chunks=3, num_steps=2).shape == (1, 2, 30)


def test_concat_path_matches_the_two_pointer_path(dev):
    ar = _ar()
    torch.manual_seed(4)
    direct = ar.DiffusionAR(net_t=adp.UNetV0, in_channels=2, length=64, num_splits=4, **NET).to(dev)
    opaque = ar.DiffusionAR(net_t=Opaque, in_channels=2, length=64, num_splits=4, **NET).to(dev)
    opaque.net.inner.load_state_dict(direct.net.state_dict())
    assert direct.diffusion.two_pointer and direct.sampler.two_pointer
    assert not opaque.diffusion.two_pointer and not opaque.sampler.two_pointer
    g = torch.Generator().manual_seed(5)
    x, noise = torch.randn(2, 2, 64, generator=g).to(dev), torch.randn(2, 2, 64, generator=g).to(dev)
    sigmas = torch.rand(2, 1, 4, generator=g).to(dev)
    la, lb = direct(x, noise=noise, sigmas=sigmas), opaque(x, noise=noise, sigmas=sigmas)
    la.backward()
    lb.backward()
    assert abs(la.item() - lb.item()) <= 1e-5 * abs(la.item())
    for (n, p), q in zip(direct.net.named_parameters(), opaque.net.inner.parameters()):
        assert rel_err(q.grad, p.grad) < 1e-4, n
    sa = direct.sample(num_items=1, num_chunks=6, num_steps=4, generator=torch.Generator().manual_seed(6))
    sb = opaque.sample(num_items=1, num_chunks=6, num_steps=4, generator=torch.Generator().manual_seed(6))
    assert rel_err(sb, sa) < 1e-4


def test_default_draws_are_the_references(emul):
    """Without injected draws: torch.rand((b, 1, N)) and then torch.randn_like(x), on x's device."""
    ar = _ar()
    torch.manual_seed(8)
    model = ar.DiffusionAR(net_t=adp.UNetV0, in_channels=2, length=64, num_splits=4, **NET)
    x = torch.randn(2, 2, 64)
    torch.manual_seed(21)
    sigmas, noise = torch.rand((2, 1, 4)), torch.randn_like(x)
    torch.manual_seed(21)
    drawn = model(x)
    assert drawn.item() == model(x, noise=noise, sigmas=sigmas).item()
    with pytest.raises(ValueError):
        model(x, sigmas=torch.rand(2, 1, 3))


def test_top_level_stub_points_at_the_module():
    with pytest.raises(NotImplementedError, match="DiffusionAR") as e:
        adp.DiffusionAR(in_channels=2, length=64, num_splits=4)
    assert "audio_diffusion_pytorch_amd.ar" in str(e.value)


# ---------------------------------------------------------------------------------------------------------- graphs (GPU)
GPU_NET = dict(channels=[8, 32, 64], factors=[1, 4, 4], items=[1, 2, 2])


def _gpu_model(hip, seed=0, **extra):
    torch.manual_seed(seed)
    return _ar().DiffusionAR(net_t=adp.UNetV0, in_channels=2, length=2048, num_splits=8, **GPU_NET, **extra).to(hip)


@pytest.mark.gpu
def test_sampler_replays_one_captured_step(hip):
    model = _gpu_model(hip)
    s = model.sampler

    def run(use_graph, seed, **kw):
        s.use_graph = use_graph
        return model.sample(num_items=2, generator=torch.Generator().manual_seed(seed), **kw)

    graphed_out = run(True, 1, num_chunks=11, num_steps=16)
    assert graphed_out.shape == (2, 2, 11 * 256)
    assert s.graph_captures == 1 and s.graph_replays >= 1
    eager_out = run(False, 1, num_chunks=11, num_steps=16)
    err = rel_err(graphed_out, eager_out)
    print(f"replayed against eager: rel err {err:.3e}")
    assert err < 1e-5
    # other chunk and step counts, same shapes: the uniform start and every ladder pass replay the same graph
    replays = s.graph_replays
    again = run(True, 2, num_chunks=9, num_steps=8)
    assert s.graph_captures == 1 and s.graph_replays == replays + 1 + 9 and len(s._graph_cache) == 1
    assert rel_err(again, run(False, 2, num_chunks=9, num_steps=8)) < 1e-5
    assert rel_err(run(True, 3, num_chunks=8, num_steps=5), run(False, 3, num_chunks=8, num_steps=5)) < 1e-5
    assert s.graph_captures == 1
    # an EMA-style copy leaves the graphs behind and captures its own
    s.use_graph = True
    twin = copy.deepcopy(model)
    assert twin.sampler.use_graph and twin.sampler.graph_captures == 0 and len(twin.sampler._graph_cache) == 0
    out = twin.sample(num_items=2, num_chunks=9, num_steps=8, generator=torch.Generator().manual_seed(2))
    assert twin.sampler.graph_captures == 1 and s.graph_captures == 1
    assert rel_err(out, again) < 1e-5


@pytest.mark.gpu
def test_sampler_recaptures_moved_parameters_and_bounds_its_cache(hip):
    """The shared cache rules on ARVSampler: a graph over dead parameter addresses is never replayed, and the cache is an LRU of
    GRAPH_CACHE_ENTRIES captured steps."""
    model = _gpu_model(hip)
    s = model.sampler

    def run(use_graph, num_items=2):
        s.use_graph = use_graph
        return model.sample(num_items=num_items, num_chunks=9, num_steps=8, generator=torch.Generator().manual_seed(1))

    out = run(True)
    assert s.graph_captures == 1 and len(s._graph_cache) == 1
    # new weights in fresh storage (allocated while the old storage is alive): the old graph holds dead addresses
    gen = torch.Generator().manual_seed(4)
    sd = {k: v + 0.05 * v.abs().mean() * torch.randn(v.shape, generator=gen).to(v.device)
          for k, v in model.net.state_dict().items()}
    model.net.load_state_dict(sd, assign=True)
    out_new = run(True)
    assert s.graph_captures == 2 and len(s._graph_cache) == 1, "the stale entry was not recaptured"
    err = rel_err(out_new, run(False))
    print(f"recaptured against eager on the new weights: rel err {err:.3e}")
    assert err < 1e-5
    assert not torch.equal(out_new, out)
    del sd

    # the bound, on a sampler of its own: five batch sizes are five call structures
    model = _gpu_model(hip)
    s = model.sampler
    for b in range(1, 6):
        run(True, num_items=b)
    assert s.graph_captures == 5 and len(s._graph_cache) == _ar().ARVSampler.GRAPH_CACHE_ENTRIES
    run(True, num_items=1)
    assert s.graph_captures == 6, "num_items=1 was the least recently used entry: evicted, captured again"


@pytest.mark.gpu
def test_training_step_replays_and_equals_the_eager_step(hip):
    m_g, m_e = _gpu_model(hip), _gpu_model(hip, diffusion_use_graph=False)
    g = torch.Generator().manual_seed(9)
    steps = 3
    for i in range(steps):
        x, noise = torch.randn(2, 2, 2048, generator=g).to(hip), torch.randn(2, 2, 2048, generator=g).to(hip)
        sigmas = torch.rand(2, 1, 8, generator=g).to(hip)
        got = []
        for m in (m_g, m_e):
            for p in m.parameters():
                p.grad = None
            loss = m(x, noise=noise, sigmas=sigmas)
            loss.backward()
            got.append((loss.item(), [p.grad.clone() for p in m.parameters()]))
        assert got[0][0] == got[1][0], (i, got[0][0], got[1][0])
        for a, b in zip(got[0][1], got[1][1]):
            assert torch.equal(a, b)
    graphs = m_g.diffusion.train_graphs()
    assert graphs.captures == 1 and graphs.replays == steps
    assert graphed.GRAPHS_OF.get(m_e.diffusion) is None
    # un-injected draws: seeded replays draw what the seeded eager loop draws, fresh values every step
    losses = []
    for m in (m_g, m_e):
        torch.manual_seed(5)
        torch.cuda.manual_seed(5)
        losses.append([m(x).item() for _ in range(3)])
    assert losses[0] == losses[1] and len(set(losses[0])) == 3
    assert m_g.diffusion.train_graphs().captures == 2   # (a second call structure: no injected tensors)


@pytest.mark.gpu
def test_training_step_with_the_stft_loss(hip):
    model = _gpu_model(hip, loss_fn=adp.MultiResolutionSTFTLoss())
    x = torch.randn(2, 2, 2048, device=hip)
    for _ in range(2):
        for p in model.parameters():
            p.grad = None
        loss = model(x)
        loss.backward()
        assert torch.isfinite(loss)
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert any(float(p.grad.abs().sum()) > 0 for p in model.parameters())
