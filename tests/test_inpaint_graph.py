"""VInpainter with the library's own noise (noise="philox") and as a replayed step (use_graph=True).

The defaults are pinned by tests/test_oracle.py and restated here; the philox path is checked against the oracle's
`v_inpaint` (oracle/vdiffusion.py) fed with the same draws through a monkeypatched `torch.randn_like`.  The net is the small
time-conditioned UNetV0 of tests/test_multistep_sampler.py; shape [2, 2, 64], 3 steps x 2 resamples."""
import copy
import os
import sys

import pytest
import torch
import torch.nn as nn

import audio_diffusion_pytorch_amd as adp
from audio_diffusion_pytorch_amd import ops
from conftest import rel_err
from oracle import vdiffusion as ovd
from test_stft_loss import TINY

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden import StubNet  # noqa: E402

GOLD = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vdiffusion_golden.pt"))
SHAPE, STEPS, RESAMPLES = (2, 2, 64), 3, 2


def tiny_net(dev, seed=0):
    torch.manual_seed(seed)
    return adp.UNetV0(dim=1, **TINY).to(dev).eval()


def case(dev, shape=SHAPE, seed=5):
    g = torch.Generator().manual_seed(seed)
    source = torch.randn(shape, generator=g)
    mask = torch.rand(shape, generator=g) > 0.5
    return source.to(dev), mask.to(dev)


class Counting(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net, self.calls = net, 0

    def forward(self, x, time, **kw):
        self.calls += 1
        return self.net(x, time, **kw)


def draw(seed, d, like):
    return ops.randn(like, ops.rng_rows(seed, [d])[0].to(like.device))


# ------------------------------------------------------------------ 1. the defaults are today's path
def test_default_inpainter_still_matches_golden(dev, monkeypatch):
    """tests/test_oracle.py::test_product_inpainter_matches_golden, restated: VInpainter(net) draws with torch.randn_like in
    the reference's call order and reproduces the live reference's fixtures."""
    host_randn_like = torch.randn_like
    monkeypatch.setattr(torch, "randn_like", lambda t, **kw: host_randn_like(t.cpu(), **kw).to(t.device))
    net = StubNet().to(dev)
    inp = adp.VInpainter(net)
    assert inp.noise == "torch" and inp.use_graph is False
    for steps, res in ((4, 3), (6, 1)):
        torch.manual_seed(77)
        out = inp(GOLD["vi_source"].to(dev), GOLD["vi_mask"].to(dev), num_steps=steps, num_resamples=res)
        assert out.device.type == dev.type
        assert rel_err(out, GOLD[f"vi_out_{steps}_{res}"]) < 1e-5
    assert inp.graph_captures == 0 and len(inp._graph_cache) == 0


def test_bad_arguments_raise(emul):
    net = StubNet()
    with pytest.raises(ValueError, match="use_graph"):
        adp.VInpainter(net, use_graph=True)
    with pytest.raises(ValueError, match="use_graph"):
        adp.VInpainter(net, noise="torch", use_graph=True)
    with pytest.raises(ValueError, match="noise"):
        adp.VInpainter(net, noise="curand")
    source, mask = case(emul)
    with pytest.raises(ValueError, match="seed"):
        adp.VInpainter(net, noise="torch")(source, mask, num_steps=2, num_resamples=1, seed=3)


# ------------------------------------------------------------------ 2. eager philox path
SEED = 7
_EAGER = {}


def eager_run(dev, monkeypatch):
    """(net, source, mask, result) of the eager noise="philox" run with seed 7, once per backend (an emulated U-Net forward
    takes seconds) and never modified.  While it runs, torch.randn_like raises and the net's calls are counted."""
    if dev.type not in _EAGER:
        net = tiny_net(dev)
        source, mask = case(dev)
        counting = Counting(net)

        def forbidden(*a, **kw):
            raise AssertionError("torch.randn_like on the philox path")

        with monkeypatch.context() as m:
            m.setattr(torch, "randn_like", forbidden)
            out = adp.VInpainter(counting, noise="philox")(source, mask, num_steps=STEPS, num_resamples=RESAMPLES, seed=SEED)
        assert counting.calls == STEPS * RESAMPLES, "one U-Net evaluation per resample"
        _EAGER[dev.type] = (net, source, mask, out)
    return _EAGER[dev.type]


def test_philox_run_matches_oracle_fed_with_the_same_draws(dev, monkeypatch):
    net, source, mask, out = eager_run(dev, monkeypatch)
    assert out.shape == source.shape and torch.isfinite(out).all()
    # the last sigma is 0: the known region is the source, exactly
    assert torch.equal(out[mask], source[mask]) and not torch.equal(out[~mask], source[~mask])
    draws = iter(range(1, 1 + STEPS * RESAMPLES))
    with monkeypatch.context() as m:
        m.setattr(torch, "randn_like", lambda t, **kw: draw(SEED, next(draws), t))
        with torch.no_grad():
            want = ovd.v_inpaint(net, source, mask, STEPS, RESAMPLES, x_noisy=draw(SEED, 0, source))
    assert next(draws, None) is None
    err = rel_err(out, want)
    print(f"philox VInpainter vs oracle on the same draws: rel_err {err:.3e} (bound 1e-5)")
    assert err < 1e-5


def test_same_seed_same_result_with_use_graph(dev, monkeypatch):
    """A second inpainter with use_graph=True: the replayed step on the GPU, the eager fallback on the CPU.  The same seed
    gives the same bits either way."""
    net, source, mask, out = eager_run(dev, monkeypatch)
    g = adp.VInpainter(net, noise="philox", use_graph=True)
    assert torch.equal(g(source, mask, num_steps=STEPS, num_resamples=RESAMPLES, seed=SEED), out)
    if dev.type == "cuda":
        assert g.graph_captures == 1 and g.graph_replays == 1
    else:
        assert g.graph_captures == 0 and g.graph_replays == 0


def test_another_seed_another_result(dev, monkeypatch):
    net, source, mask, out = eager_run(dev, monkeypatch)
    other = adp.VInpainter(net, noise="philox")(source, mask, num_steps=STEPS, num_resamples=RESAMPLES, seed=SEED + 1)
    assert not torch.equal(out, other)
    assert torch.equal(other[mask], source[mask])


def test_given_start_and_missing_seed(dev, monkeypatch):
    """One step, one resample (cheap): a given x_noisy replaces draw 0 and nothing else; a missing seed comes from torch's
    default CPU generator, so torch.manual_seed governs it and two runs in a row differ."""
    net, source, mask, _ = eager_run(dev, monkeypatch)
    inp = adp.VInpainter(net, noise="philox")
    start = draw(SEED, 0, source)
    kept = start.clone()
    a = inp(source, mask, num_steps=1, num_resamples=1, seed=SEED)
    assert torch.equal(a, inp(source, mask, num_steps=1, num_resamples=1, seed=SEED, x_noisy=start))
    assert torch.equal(start, kept)
    torch.manual_seed(123)
    d1 = inp(source, mask, num_steps=1, num_resamples=1)
    d2 = inp(source, mask, num_steps=1, num_resamples=1)
    torch.manual_seed(123)
    d3 = inp(source, mask, num_steps=1, num_resamples=1)
    assert torch.equal(d1, d3) and not torch.equal(d1, d2)
    assert torch.equal(inp(source, mask, num_steps=0, num_resamples=2, seed=SEED, x_noisy=start), start)   # (no resample at all)


# ------------------------------------------------------------------ 3. the replayed step
@pytest.mark.gpu
def test_replay_equals_eager(hip):
    net = tiny_net(hip)
    source, mask = case(hip)
    g = adp.VInpainter(net, noise="philox", use_graph=True)
    e = adp.VInpainter(net, noise="philox")
    out = g(source, mask, num_steps=STEPS, num_resamples=RESAMPLES, seed=7)
    assert torch.equal(out, e(source, mask, num_steps=STEPS, num_resamples=RESAMPLES, seed=7))
    assert torch.equal(out[mask], source[mask])
    out2 = g(source, mask, num_steps=5, num_resamples=3, seed=8)
    assert torch.equal(out2, e(source, mask, num_steps=5, num_resamples=3, seed=8))
    assert g.graph_captures == 1 and g.graph_replays == 2 and len(g._graph_cache) == 1 and e.graph_captures == 0
    # other source / mask / start through the same entry; the caller's tensors are not touched
    source2, mask2 = case(hip, seed=6)
    start = torch.randn(SHAPE, generator=torch.Generator().manual_seed(9)).to(hip)
    kept = start.clone()
    out3 = g(source2, mask2, num_steps=STEPS, num_resamples=RESAMPLES, seed=7, x_noisy=start)
    assert torch.equal(out3, e(source2, mask2, num_steps=STEPS, num_resamples=RESAMPLES, seed=7, x_noisy=start))
    assert torch.equal(start, kept) and g.graph_captures == 1
    # show_progress is served eagerly
    assert torch.equal(g(source, mask, num_steps=STEPS, num_resamples=RESAMPLES, seed=7, show_progress=True), out)
    assert g.graph_replays == 3
    # a second shape captures a second entry
    source4, mask4 = case(hip, shape=(1, 2, 128))
    out4 = g(source4, mask4, num_steps=2, num_resamples=2, seed=3)
    assert torch.equal(out4, e(source4, mask4, num_steps=2, num_resamples=2, seed=3))
    assert g.graph_captures == 2 and len(g._graph_cache) == 2


@pytest.mark.gpu
def test_recapture_after_parameters_moved_and_deepcopy(hip):
    net = tiny_net(hip)
    source, mask = case(hip)
    g = adp.VInpainter(net, noise="philox", use_graph=True)
    out = g(source, mask, num_steps=STEPS, num_resamples=RESAMPLES, seed=7)
    cp = copy.deepcopy(g)
    assert len(cp._graph_cache) == 0 and cp.graph_captures == 0 and cp.graph_replays == 0
    assert cp.noise == "philox" and cp.use_graph
    assert torch.equal(cp(source, mask, num_steps=STEPS, num_resamples=RESAMPLES, seed=7), out)
    assert cp.graph_captures == 1 and g.graph_captures == 1
    # new weights in fresh storage (allocated while the old storage is alive): the old graph holds dead addresses
    gen = torch.Generator().manual_seed(4)
    sd = {k: v + 0.05 * v.abs().mean() * torch.randn(v.shape, generator=gen).to(v.device) for k, v in net.state_dict().items()}
    net.load_state_dict(sd, assign=True)
    out_new = g(source, mask, num_steps=STEPS, num_resamples=RESAMPLES, seed=7)
    assert g.graph_captures == 2 and len(g._graph_cache) == 1, "the stale entry was not recaptured"
    eager = adp.VInpainter(net, noise="philox")(source, mask, num_steps=STEPS, num_resamples=RESAMPLES, seed=7)
    assert torch.equal(out_new, eager) and not torch.equal(out_new, out)
