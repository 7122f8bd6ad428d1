"""The replayed training step (graphed.py) and the replayed sampler step (VSampler._forward_graph) over a model's lifetime:
after whatever else the model has done -- a validation forward, a sample() call, a capture at another shape, swapped
parameters, a deepcopy / torch.save, a second forward before the backward, a new loss_fn or sigma range -- a replay must
still equal the eager step of the same call.

Twin-model pattern of test_train_graph.py: two models from the same seed, one with every graph path switched off, driven
identically.  The reference of each call is the eager path of the same call (the eager kernels are checked against fp32 /
fp64 references elsewhere).  Every model is text-conditional (an `embedding` kwarg, eight cross-attention items), so the
context bank (attention.CtxBank) and its device pointer tables are part of every captured graph.  Every test asserts the
capture / replay counters and the bank runs (a replay runs no Python, so the count stays put), so that none of them can pass
by quietly running eagerly."""
import copy
import gc
import io
import weakref

import pytest
import torch

import audio_diffusion_pytorch_amd as adp
from audio_diffusion_pytorch_amd import graphed
from audio_diffusion_pytorch_amd.losses import MultiResolutionSTFTLoss
from audio_diffusion_pytorch_amd.unet import UNetV0Net
from conftest import rel_err

CFG = dict(in_channels=2, channels=[8, 32, 64], factors=[1, 4, 4], items=[1, 2, 2], modulation_features=64,
           cross_attentions=[0, 1, 1], attention_heads=2, attention_features=16, embedding_features=24)
L_TRAIN, L_SAMPLE, STEPS = 2048, 1024, 3


def _twins(dev, seed=0):
    """(graph-replaying model, eager twin) with identical weights."""
    torch.manual_seed(seed)
    m_g = adp.DiffusionModel(net_t=adp.UNetV0, **CFG).to(dev)
    torch.manual_seed(seed)
    m_e = adp.DiffusionModel(net_t=adp.UNetV0, diffusion_use_graph=False, sampler_use_graph=False, **CFG).to(dev)
    return m_g, m_e


def _inputs(dev, batch=2, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, 2, L_TRAIN, generator=g).to(dev)
    noise = torch.randn(batch, 2, L_SAMPLE, generator=g).to(dev)
    emb = torch.randn(batch, 5, 24, generator=g).to(dev)
    return x, noise, emb


def _unet(m) -> UNetV0Net:
    return next(mod for mod in m.modules() if isinstance(mod, UNetV0Net))


def _bank_runs(m) -> int:
    return getattr(_unet(m), "_ctx_bank_runs", 0)


def _zero(m):
    for p in m.parameters():
        p.grad = None


def _grads(m):
    return [None if p.grad is None else p.grad.clone() for p in m.parameters()]


def _train(m, x, emb, seed):
    """One README step (zero grads, loss = model(x), backward) from a fixed seed: (loss, every parameter gradient)."""
    _zero(m)
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    loss = m(x, embedding=emb)
    loss.backward()
    return loss.detach().clone(), _grads(m)


def _assert_same_grads(ga, gb):
    assert len(ga) == len(gb)
    for i, (a, b) in enumerate(zip(ga, gb)):
        assert (a is None) == (b is None), i
        if a is not None:
            assert torch.equal(a, b), i


def _assert_same_step(a, b):
    # identical kernels, identical sigma / noise draws (same seed): identical numbers
    assert torch.equal(a[0], b[0]), (a[0].item(), b[0].item())
    _assert_same_grads(a[1], b[1])


def _sample(m, noise, emb):
    return m.sample(noise, num_steps=STEPS, embedding=emb)


def _churn(dev):
    """Hand freed device blocks back out: return the allocator's cache to the driver, then allocate and fill a few hundred
    small tensors of the context tables' sizes (I pointers, E floats)."""
    torch.cuda.empty_cache()
    return [torch.full((n,), 7 + i, dtype=torch.int64, device=dev) for i in range(60) for n in (3, 8, 24, 64, 256)]


def _table_refs(m):
    tabs = _unet(m)._ctx_tables
    assert tabs is not None, "the context bank built its tables"
    refs = [weakref.ref(v) for v in tabs.values() if isinstance(v, torch.Tensor) and v.is_cuda]
    assert len(refs) == 5  # tab, dw_off, dgb_off, ones, zeros
    return refs


def _eager_validation_forward(m, x, emb):
    with torch.no_grad():
        return m.net(x, torch.rand(x.shape[0], device=x.device), embedding=emb)


# ------------------------------------------------------------------ H: structural checks (nothing replayed after the eager call)

def test_ctx_tables_survive_a_proxied_forward(emul):
    """The capture runs the net under graphed._ProxyParameters (new Parameter objects over the same storage); the next eager
    forward sees the real objects again and rebuilds the parameter caches.  The context-bank tables are keyed on the
    parameters' addresses, which did not change: they must stay the same objects (a captured graph reads them by address).
    New storage must still rebuild them."""
    torch.manual_seed(0)
    m = adp.DiffusionModel(net_t=adp.UNetV0, **CFG)
    g = torch.Generator().manual_seed(2)
    x, emb = torch.randn(2, 2, 256, generator=g), torch.randn(2, 5, 24, generator=g)
    net = _unet(m)
    runs = _bank_runs(m)
    _eager_validation_forward(m, x, emb)
    tabs = net._ctx_tables
    assert tabs is not None and _bank_runs(m) == runs + 1
    with graphed._ProxyParameters(m.diffusion):
        _eager_validation_forward(m, x, emb)
    assert net._ctx_tables is tabs
    _eager_validation_forward(m, x, emb)
    assert net._ctx_tables is tabs and _bank_runs(m) == runs + 3
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()}, assign=True)
    _eager_validation_forward(m, x, emb)
    assert net._ctx_tables is not tabs and _bank_runs(m) == runs + 4
    items = [p for p in net.modules() if hasattr(p, "to_kv") and hasattr(p, "norm_context")]
    assert len(items) >= 2
    assert sorted(net._ctx_tables["tab"][0].tolist()) == sorted(p.to_kv.weight.data_ptr() for p in items)


@pytest.mark.gpu
def test_training_capture_keeps_its_ctx_tables_alive(hip):
    """H, training graph: the tables a capture baked in stay alive across an eager forward (nothing is replayed here)."""
    m, _ = _twins(hip)
    x, _, emb = _inputs(hip)
    runs = _bank_runs(m)
    _train(m, x, emb, 3)
    g = graphed.GRAPHS_OF[m.diffusion]
    assert g.captures == 1 and g.replays == 1 and _bank_runs(m) > runs
    refs = _table_refs(m)
    _eager_validation_forward(m, x, emb)
    gc.collect()
    assert all(r() is not None for r in refs), "a device table the captured training step reads was freed"


@pytest.mark.gpu
def test_sampler_capture_keeps_its_ctx_tables_alive(hip):
    """H, sampler graph: a training capture and an eager forward after a sampler capture leave its tables alive."""
    m, _ = _twins(hip)
    x, noise, emb = _inputs(hip)
    runs = _bank_runs(m)
    _sample(m, noise, emb)
    assert len(m.sampler._graph_cache) == 1 and _bank_runs(m) > runs
    refs = _table_refs(m)
    _train(m, x, emb, 3)
    assert graphed.GRAPHS_OF[m.diffusion].captures == 1
    _eager_validation_forward(m, x, emb)
    gc.collect()
    assert all(r() is not None for r in refs), "a device table the captured sampler step reads was freed"


# ------------------------------------------------------------------ A-D: replays after the model did something else

@pytest.mark.gpu
def test_replay_after_a_validation_forward(hip):
    """A: capture + replay, an eager no_grad forward, allocator churn, replay again."""
    m_g, m_e = _twins(hip)
    x, _, emb = _inputs(hip)
    for seed in (10, 11):
        _assert_same_step(_train(m_g, x, emb, seed), _train(m_e, x, emb, seed))
    runs = _bank_runs(m_g)
    for m in (m_g, m_e):
        _eager_validation_forward(m, x, emb)
    assert _bank_runs(m_g) == runs + 1
    junk = _churn(hip)
    e_runs = _bank_runs(m_e)
    _assert_same_step(_train(m_g, x, emb, 12), _train(m_e, x, emb, 12))
    g = graphed.GRAPHS_OF[m_g.diffusion]
    assert g.captures == 1 and g.replays == 3
    assert _bank_runs(m_g) == runs + 1, "the last step was replayed, not run eagerly"
    assert _bank_runs(m_e) == e_runs + 1
    del junk


@pytest.mark.gpu
def test_training_and_sampling_interleaved(hip):
    """B: train (capture), sample (capture), train, sample, train -- every result against the eager twin."""
    m_g, m_e = _twins(hip)
    x, noise, emb = _inputs(hip)
    runs = _bank_runs(m_g)
    for i, what in enumerate(("train", "sample", "train", "sample", "train")):
        if what == "train":
            _assert_same_step(_train(m_g, x, emb, 20 + i), _train(m_e, x, emb, 20 + i))
        else:
            assert rel_err(_sample(m_g, noise, emb), _sample(m_e, noise, emb)) < 1e-5, i
        if i == 1:
            assert _bank_runs(m_g) > runs
            runs = _bank_runs(m_g)
    g = graphed.GRAPHS_OF[m_g.diffusion]
    assert g.captures == 1 and g.replays == 3
    assert m_g.sampler.graph_captures == 1 and m_g.sampler.graph_replays == 2 and len(m_g.sampler._graph_cache) == 1
    assert _bank_runs(m_g) == runs, "after both captures every call was replayed"
    assert _bank_runs(m_e) >= 3 + 2 * STEPS  # (the eager twin ran the bank in every call)


@pytest.mark.gpu
def test_capture_at_a_second_shape(hip):
    """C: batch 2 (capture), batch 1 -- a short last batch -- (second capture), allocator churn, batch 2 again (replay)."""
    m_g, m_e = _twins(hip)
    x, _, emb = _inputs(hip)
    _assert_same_step(_train(m_g, x, emb, 30), _train(m_e, x, emb, 30))
    _assert_same_step(_train(m_g, x[:1], emb[:1], 31), _train(m_e, x[:1], emb[:1], 31))
    runs = _bank_runs(m_g)
    junk = _churn(hip)
    _assert_same_step(_train(m_g, x, emb, 32), _train(m_e, x, emb, 32))
    g = graphed.GRAPHS_OF[m_g.diffusion]
    assert g.captures == 2 and g.replays == 3 and len(g.cache) == 2
    assert _bank_runs(m_g) == runs, "the last step was replayed"
    del junk


@pytest.mark.gpu
def test_sampler_follows_swapped_parameters(hip):
    """D: sample, then new parameter objects (load_state_dict(assign=True), perturbed), sample; then new storage under the same
    objects (p.data = clone) while the old storage is kept alive and overwritten, sample.  Each must equal eager sampling with
    the weights the model holds now."""
    m_g, m_e = _twins(hip)
    _, noise, emb = _inputs(hip)
    s0 = _sample(m_g, noise, emb)
    assert rel_err(s0, _sample(m_e, noise, emb)) < 1e-5
    assert m_g.sampler.graph_captures == 1
    gen = torch.Generator().manual_seed(4)
    sd = {k: v + 0.05 * v.abs().mean() * torch.randn(v.shape, generator=gen).to(v.device) for k, v in m_g.state_dict().items()}
    m_g.load_state_dict({k: v.clone() for k, v in sd.items()}, assign=True)
    m_e.load_state_dict({k: v.clone() for k, v in sd.items()}, assign=True)
    runs = _bank_runs(m_g)
    s1 = _sample(m_g, noise, emb)
    assert m_g.sampler.graph_captures == 2 and len(m_g.sampler._graph_cache) == 1, "the stale entry was recaptured"
    assert _bank_runs(m_g) > runs
    assert rel_err(s1, _sample(m_e, noise, emb)) < 1e-5
    assert rel_err(s1, s0) > 1e-3, "the new weights were used"
    old = []
    with torch.no_grad():
        for p in m_g.parameters():
            old.append(p.data)
            p.data = p.data.clone()
        for t in old:  # a graph still reading the old storage would see these values
            t.mul_(-3.0)
    s2 = _sample(m_g, noise, emb)
    assert m_g.sampler.graph_captures == 3 and m_g.sampler.graph_replays == 3
    assert rel_err(s2, _sample(m_e, noise, emb)) < 1e-5
    runs = _bank_runs(m_g)
    assert torch.equal(_sample(m_g, noise, emb), s2) and _bank_runs(m_g) == runs  # (a plain replay: nothing recaptured)
    assert m_g.sampler.graph_captures == 3
    del old


# ------------------------------------------------------------------ E-G

@pytest.mark.gpu
def test_deepcopy_and_save_after_gpu_sampling(hip):
    """E: an EMA-style deepcopy and torch.save after the sampler captured a step; the copy never shares graphs with the
    original."""
    m_g, _ = _twins(hip)
    _, noise, emb = _inputs(hip)
    s0 = _sample(m_g, noise, emb)
    assert len(m_g.sampler._graph_cache) == 1
    buf = io.BytesIO()
    torch.save(m_g, buf)
    cp = copy.deepcopy(m_g)
    assert len(cp.sampler._graph_cache) == 0
    gen = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for p in cp.parameters():
            p.add_(0.05 * p.abs().mean() * torch.randn(p.shape, generator=gen).to(hip))
    runs = _bank_runs(cp)
    s_cp = _sample(cp, noise, emb)
    assert cp.sampler.graph_captures == 1 and len(cp.sampler._graph_cache) == 1 and _bank_runs(cp) > runs
    cp.sampler.use_graph = False
    assert rel_err(s_cp, _sample(cp, noise, emb)) < 1e-5
    assert rel_err(s_cp, s0) > 1e-3, "the copy's own weights were used"
    runs = _bank_runs(m_g)
    assert torch.equal(_sample(m_g, noise, emb), s0), "the original is untouched by its copy"
    assert m_g.sampler.graph_replays == 2 and _bank_runs(m_g) == runs
    buf.seek(0)
    loaded = torch.load(buf, weights_only=False)
    assert len(loaded.sampler._graph_cache) == 0
    assert rel_err(_sample(loaded, noise, emb), s0) < 1e-5 and loaded.sampler.graph_captures == 1


@pytest.mark.gpu
def test_two_forwards_before_one_backward(hip):
    """F: `(model(x1) + model(x2)).backward()` and `l1 = model(x1); model(x2); l1.backward()` -- the second forward runs
    eagerly while the replayed loss waits for its backward -- equal the eager twin; once the pending loss is backpropagated or
    dropped, the next steps replay again."""
    m_g, m_e = _twins(hip)
    x, _, emb = _inputs(hip)
    x2 = torch.flip(x, dims=[2]).contiguous()
    _assert_same_step(_train(m_g, x, emb, 40), _train(m_e, x, emb, 40))
    g = graphed.GRAPHS_OF[m_g.diffusion]
    assert g.captures == 1 and g.replays == 1

    def pair_sum(m):
        _zero(m)
        torch.manual_seed(41)
        torch.cuda.manual_seed(41)
        (m(x, embedding=emb) + m(x2, embedding=emb)).backward()
        return _grads(m)

    runs = _bank_runs(m_g)
    # (each parameter receives exactly two gradients, summed once: a + b == b + a, so the sum is bit-exact whichever
    #  backward finishes first)
    _assert_same_grads(pair_sum(m_g), pair_sum(m_e))
    assert g.replays == 2 and _bank_runs(m_g) == runs + 1, "the first forward replayed, the second ran eagerly"

    def stray_forward(m):
        _zero(m)
        torch.manual_seed(42)
        torch.cuda.manual_seed(42)
        l1 = m(x, embedding=emb)
        m(x2, embedding=emb)
        l1.backward()
        return _grads(m)

    _assert_same_grads(stray_forward(m_g), stray_forward(m_e))
    assert g.replays == 3 and _bank_runs(m_g) == runs + 2
    # a replayed loss dropped without a backward does not block later replays either
    dropped = m_g(x, embedding=emb)
    del dropped
    assert g.replays == 4
    runs = _bank_runs(m_g)
    for seed in (44, 45):
        _assert_same_step(_train(m_g, x, emb, seed), _train(m_e, x, emb, seed))
    assert g.replays == 6 and g.captures == 1 and _bank_runs(m_g) == runs


@pytest.mark.gpu
def test_replays_follow_loss_fn_and_sigma_range(hip):
    """G: switching `loss_fn` (MSE -> native multi-resolution STFT -> MSE) or the sigma range after the first step changes what
    the next replay computes, as it changes the eager step."""
    m_g, m_e = _twins(hip)
    x, _, emb = _inputs(hip)
    stft = MultiResolutionSTFTLoss(fft_sizes=(64, 128), hop_sizes=(16, 32), win_lengths=(64, 96))
    losses = []
    for loss_fn in (torch.nn.functional.mse_loss, stft, stft, torch.nn.functional.mse_loss):
        for m in (m_g, m_e):
            del m.diffusion.loss_fn  # (nn.Module refuses to put a plain function where a child module is registered)
            m.diffusion.loss_fn = loss_fn
        a, b = _train(m_g, x, emb, 50), _train(m_e, x, emb, 50)
        _assert_same_step(a, b)
        losses.append(a[0].item())
    g = graphed.GRAPHS_OF[m_g.diffusion]
    assert losses[0] == losses[3] and losses[1] == losses[2] and losses[0] != losses[1]
    assert g.captures == 2 and g.replays == 4  # (MSE and STFT each own an entry; switching back replays the MSE one)
    for m in (m_g, m_e):
        m.diffusion.sigma_distribution = adp.UniformDistribution(vmin=0.2, vmax=0.6)
    runs = _bank_runs(m_g)
    a, b = _train(m_g, x, emb, 50), _train(m_e, x, emb, 50)
    _assert_same_step(a, b)
    assert a[0].item() != losses[0]
    assert g.captures == 3 and g.replays == 5 and _bank_runs(m_g) > runs
