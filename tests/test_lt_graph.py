"""LTPlugin under the captured steps (GPU only): the README training loop of an LT model replays from the two hipGraphs of
graphed.py with both transform layers inside them, and the sampler captures its step with the transform inside it; both give
the eager launches' numbers bit for bit."""
import pytest
import torch

import audio_diffusion_pytorch_amd as adp
from audio_diffusion_pytorch_amd import graphed
from audio_diffusion_pytorch_amd.lt import LTPlugin

NET = dict(in_channels=2, channels=[8, 32, 64], factors=[1, 4, 4], items=[1, 2, 2], modulation_features=128)


def _model(dev, **extra):
    torch.manual_seed(0)
    return adp.DiffusionModel(net_t=LTPlugin(adp.UNetV0, num_filters=4, window_length=8, stride=4), **NET, **extra).to(dev)


@pytest.mark.gpu
def test_lt_training_step_replays_and_matches_the_eager_step(hip):
    m_g, m_e = _model(hip), _model(hip, diffusion_use_graph=False)
    xs = [torch.randn(2, 2, 4096, device=hip) for _ in range(3)]
    for m in (m_g, m_e):
        torch.manual_seed(123)
        torch.cuda.manual_seed(123)
        m.losses, m.grads = [], []
        for x in xs:
            for p in m.parameters():
                p.grad = None
            loss = m(x)
            loss.backward()
            m.losses.append(loss.item())
            m.grads.append({n: p.grad.clone() for n, p in m.named_parameters()})
    g = graphed.GRAPHS_OF[m_g.diffusion]
    assert g.captures == 1 and g.replays == 3
    assert graphed.GRAPHS_OF.get(m_e.diffusion) is None
    for i in range(3):
        assert m_g.losses[i] == m_e.losses[i], (i, m_g.losses, m_e.losses)
        assert set(m_g.grads[i]) == set(m_e.grads[i]) and {"net.encode.weight", "net.decode.weight"} <= set(m_g.grads[i])
        for n, a in m_g.grads[i].items():
            assert torch.equal(a, m_e.grads[i][n]), (i, n)
        assert m_g.grads[i]["net.encode.weight"].abs().max() > 0 and m_g.grads[i]["net.decode.weight"].abs().max() > 0
    assert len({round(v, 9) for v in m_g.losses}) == 3, "every replay must draw fresh sigmas / noise"


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", ["VSampler", "VMultistepSampler"])
def test_lt_sampler_step_is_captured_and_matches_the_eager_sampler(hip, sampler):
    extra = {} if sampler == "VSampler" else dict(sampler_t=adp.VMultistepSampler)
    m_g, m_e = _model(hip, **extra), _model(hip, sampler_use_graph=False, **extra)
    noise = torch.randn(1, 2, 4096, device=hip)
    a = m_g.sample(noise, num_steps=3)
    b = m_e.sample(noise, num_steps=3)
    assert m_g.sampler.graph_captures >= 1 and m_e.sampler.graph_captures == 0
    assert torch.isfinite(a).all() and torch.equal(a, b)
