"""The native T5 v1.1 / flan-T5 encoder (text.T5GatedEncoder) and its gated feed-forward GEMM (csrc/gated.hip,
include/adp_gated.h).

Kernel parity against float64 torch on the CPU, outputs and workspaces pre-filled with NaN; module parity against
tests/t5_gated_ref.py; t5_gated_ref.py itself against transformers.T5EncoderModel(feed_forward_proj="gated-gelu") where
transformers is importable.  The bounds are tests/test_t5.py's (TOL for one kernel, TOL_MODULE for the module, conftest.rel_err
against float64).  Every `dev` test runs on the SIMT emulator and, with -m gpu, on the gfx950 library."""
import functools

import pytest
import torch

import audio_diffusion_pytorch_amd as adp
from audio_diffusion_pytorch_amd import _C, ops, text
from audio_diffusion_pytorch_amd.text import T5Embedder, T5Encoder, T5GatedEncoder
from conftest import rel_err
from test_t5 import NULL, SHAPE, TEXTS, TOL, TOL_MODULE, UNET, UNSUPPORTED, HashTokenizer, check, nan_like, p, prefix_mask

import t5_gated_ref
import t5_ref

GELU_NEW = 1


def hf_config(transformers, cfg, proj):
    return transformers.T5Config(
        vocab_size=cfg.vocab_size, d_model=cfg.d_model, d_kv=cfg.d_kv, d_ff=cfg.d_ff, num_layers=cfg.num_layers,
        num_heads=cfg.num_heads, relative_attention_num_buckets=cfg.num_buckets,
        relative_attention_max_distance=cfg.max_distance, layer_norm_epsilon=cfg.eps, feed_forward_proj=proj,
        dropout_rate=0.0)


# ------------------------------------------------------------------------------------- the restatement is the transformers encoder
@pytest.mark.parametrize("m", [5, 64, 150])
@pytest.mark.parametrize("cfg", [t5_gated_ref.TINY, t5_gated_ref.FLAN1], ids=["tiny", "flan1"])
def test_restatement_against_transformers(cfg, m):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(7)
    hf = transformers.T5EncoderModel(hf_config(transformers, cfg, "gated-gelu")).eval()
    with torch.no_grad():
        for name, q in hf.named_parameters():
            if name.endswith("layer_norm.weight"):
                q.copy_(1 + 0.2 * torch.randn_like(q))
            elif name.endswith("relative_attention_bias.weight"):
                q.copy_(torch.randn_like(q))
    g = torch.Generator().manual_seed(m)
    ids = torch.randint(0, cfg.vocab_size, (3, m), generator=g)
    for what, mask in (("prefix", prefix_mask(3, m)), ("zero", torch.zeros(3, m, dtype=torch.int64))):
        with torch.no_grad():
            want = hf(input_ids=ids, attention_mask=mask).last_hidden_state
        got = t5_gated_ref.encode(hf.state_dict(), cfg, ids, mask)
        err = rel_err(got, want)
        print(f"t5_gated_ref vs transformers, m {m}, {what} mask: rel err {err:.3e}")
        assert err < TOL, (what, err)


# -------------------------------------------------------------------------------------------------------------- kernel
# tails in T, K and F, tile edges at 32 and 64; (70, 130, 45): a cut with a ragged last segment (96 + 34); (64, 768, 48): 2
# tiles, so a cut into 6 segments of 128
GATED_SHAPES = [(1, 1, 1), (5, 7, 3), (33, 40, 31), (70, 130, 45), (64, 768, 48)]
GATED_CUT = GATED_SHAPES[-2:]
shape_id = lambda s: "T{}K{}F{}".format(*s)   # noqa: E731


@functools.lru_cache(maxsize=None)
def gated_case(shape, gate_scale):
    """Inputs and the float64 reference of one shape (CPU tensors, computed once, never modified)."""
    T, K, F = shape
    g = torch.Generator().manual_seed(100 * T + 10 * K + F)
    x = torch.randn(T, K, generator=g)
    wg, wu = (torch.randn(F, K, generator=g) / K ** 0.5 for _ in range(2))
    wg = wg * gate_scale
    gate = x.double() @ wg.double().T
    return dict(x=x, wg=wg, wu=wu, gate=gate, want=t5_gated_ref.gelu_new(gate) * (x.double() @ wu.double().T))


def run_gated(dev, shape, d):
    """Two calls on NaN-filled outputs and workspaces: ADP_OK, finite, within TOL, bit-identical, inputs unchanged."""
    T, K, F = shape
    lib, s = _C.lib(), _C.stream()
    x, wg, wu = (d[k].to(dev) for k in ("x", "wg", "wu"))
    nbytes = lib.adp_gated_linear_ws_bytes(T, K, F)
    assert nbytes >= 0 and nbytes % (2 * T * F * 4) == 0
    if shape in GATED_CUT:
        assert nbytes > 0, "the split rule no longer cuts this shape: choose another shape"
    if K <= 128:
        assert nbytes == 0
    runs = []
    for _ in range(2):
        ws = nan_like((nbytes // 4,), dev) if nbytes else None
        y = nan_like((T, F), dev)
        assert lib.adp_gated_linear(p(x), p(wg), p(wu), T, K, F, GELU_NEW, p(y), p(ws), s) == 0
        runs.append(y)
    check(f"gated_linear {shape_id(shape)}", runs[0], d["want"])
    assert torch.equal(runs[0], runs[1]), "not bit-identical from call to call"
    assert torch.equal(x.cpu(), d["x"]) and torch.equal(wg.cpu(), d["wg"]) and torch.equal(wu.cpu(), d["wu"])
    return x, wg, wu, runs[0]


@pytest.mark.parametrize("shape", GATED_SHAPES, ids=shape_id)
def test_gated_linear_kernel(dev, shape):
    x, wg, wu, y = run_gated(dev, shape, gated_case(shape, 1.0))
    assert torch.equal(ops.gated_linear(x, wg, wu), y)
    assert ops.gated_linear_ws_bytes(*shape) == _C.lib().adp_gated_linear_ws_bytes(*shape)
    out = nan_like(shape[::2], dev)
    assert ops.gated_linear(x, wg, wu, out=out) is out and torch.equal(out, y)


# ---------------------------------------------------------------------------------------------------------- gate range
@pytest.mark.parametrize("shape", GATED_SHAPES, ids=shape_id)
def test_gate_range(dev, shape):
    """w_gate scaled by 6: the gate sums spread to about +-20, where 1 + tanh cancels on the negative side."""
    d = gated_case(shape, 6.0)
    print(f"gate values in [{d['gate'].min().item():.1f}, {d['gate'].max().item():.1f}]")
    run_gated(dev, shape, d)


def test_gate_extremes(dev):
    """x[t] = (g_t, 1), w_gate[f] = (1, 0), w_up[f] = (0, u_f): the gate sum is g_t and the up sum u_f, both exact."""
    gates = torch.tensor([-1e4, -30.0, -1e-8, 0.0, 1e-8, 30.0, 1e4])
    ups = torch.tensor([1.5, -2.0, 0.25])
    T, K, F = gates.numel(), 2, ups.numel()
    x = torch.stack([gates, torch.ones(T)], dim=1)
    wg = torch.tensor([[1.0, 0.0]]).repeat(F, 1)
    wu = torch.stack([torch.zeros(F), ups], dim=1)
    want = t5_gated_ref.gelu_new(gates.double())[:, None] * ups.double()[None, :]
    y = nan_like((T, F), dev)
    assert _C.lib().adp_gated_linear(p(x.to(dev)), p(wg.to(dev)), p(wu.to(dev)), T, K, F, GELU_NEW, p(y), None,
                                     _C.stream()) == 0
    check("gated_linear extremes", y, want)
    for t in range(T):   # per row: the rows differ in scale by 1e12
        check(f"gate {gates[t].item():g}", y[t], want[t])
    y = y.cpu()
    assert (y[3] == 0).all(), "0 * up is 0"
    assert (y[0] == 0).all() and (y[1] == 0).all(), "a large negative gate gives 0, not NaN"


# --------------------------------------------------------------------------------------------------------- error codes
def test_gated_error_codes(dev):
    lib, s = _C.lib(), _C.stream()
    x, wg, wu, y = torch.randn(4, 8).to(dev), torch.randn(3, 8).to(dev), torch.randn(3, 8).to(dev), nan_like((4, 3), dev)
    gl = lambda *a: lib.adp_gated_linear(*a, s)   # noqa: E731
    assert gl(p(x), p(wg), p(wu), 4, 8, 3, GELU_NEW, p(y), None) == 0
    assert torch.isfinite(y).all()
    y.fill_(float("nan"))
    assert gl(None, p(wg), p(wu), 4, 8, 3, GELU_NEW, p(y), None) == NULL
    assert gl(p(x), None, p(wu), 4, 8, 3, GELU_NEW, p(y), None) == NULL
    assert gl(p(x), p(wg), None, 4, 8, 3, GELU_NEW, p(y), None) == NULL
    assert gl(p(x), p(wg), p(wu), 4, 8, 3, GELU_NEW, None, None) == NULL
    for bad in ((0, 8, 3), (4, 0, 3), (4, 8, 0), (4, -1, 3), (1 << 20, 1 << 20, 3)):
        assert gl(p(x), p(wg), p(wu), *bad, GELU_NEW, p(y), None) == SHAPE
        assert lib.adp_gated_linear_ws_bytes(*bad) == SHAPE
    cut = GATED_CUT[-1]
    big, y2 = torch.randn(64, 768).to(dev), nan_like(cut[::2], dev)
    nbytes = lib.adp_gated_linear_ws_bytes(*cut)
    assert nbytes > 0
    ws = nan_like((nbytes // 4,), dev)
    assert gl(p(big), p(big), p(big), *cut, GELU_NEW, p(y2), None) == NULL   # a workspace is needed and missing
    for act in (0, 2):
        assert gl(p(x), p(wg), p(wu), 4, 8, 3, act, p(y), None) == UNSUPPORTED
        assert gl(p(big), p(big), p(big), *cut, act, p(y2), p(ws)) == UNSUPPORTED
    # NULL before SHAPE before UNSUPPORTED; the missing workspace, known only after the sizes passed, between the last two
    assert gl(None, p(wg), p(wu), 0, 8, 3, 2, p(y), None) == NULL
    assert gl(p(x), p(wg), p(wu), 0, 8, 3, 2, p(y), None) == SHAPE
    assert gl(p(big), p(big), p(big), *cut, 2, p(y2), None) == NULL
    for t in (y, y2, ws):   # a refused call writes nothing
        assert torch.isnan(t).all()


# ------------------------------------------------------------------------------------------------------------ the module
def native(cfg, sd, dev):
    enc = T5GatedEncoder(cfg.vocab_size, cfg.d_model, cfg.d_kv, cfg.d_ff, cfg.num_layers, cfg.num_heads, cfg.num_buckets,
                         cfg.max_distance, cfg.eps)
    enc.load_hf_state_dict(sd)
    return enc.to(dev)


@functools.lru_cache(maxsize=None)
def module_case(name, B, m, kind):
    cfg = getattr(t5_gated_ref, name)
    sd = t5_gated_ref.random_state_dict(cfg, seed=1)
    ids = torch.randint(0, cfg.vocab_size, (B, m), generator=torch.Generator().manual_seed(m))
    mask = {"none": None, "prefix": prefix_mask(B, m), "zero": torch.zeros(B, m, dtype=torch.int64)}[kind]
    return cfg, sd, ids, mask, t5_gated_ref.encode(sd, cfg, ids, mask)


@pytest.mark.parametrize("kind", ["none", "prefix", "zero"])
@pytest.mark.parametrize("m", [5, 64, 150])
def test_gated_encoder_tiny(dev, m, kind):
    cfg, sd, ids, mask, want = module_case("TINY", 3, m, kind)
    enc = native(cfg, sd, dev)
    assert isinstance(enc, T5Encoder) and all(not q.requires_grad for q in enc.parameters())
    out = enc(ids.to(dev), None if mask is None else mask.to(dev))
    assert out.shape == (3, m, cfg.d_model) and not out.requires_grad
    check(f"T5GatedEncoder tiny m{m} {kind}", out, want, TOL_MODULE)


def test_gated_encoder_flan_geometry(dev):
    """flan-t5-base's widths (768 / 12 heads of 64 / 2048), 1 layer: every GEMM of the real model at its real k length, the
    gated one cut into 4 segments of 192 at these 128 tokens.  (The emulated run is about 0.9 G multiply-adds through the fiber
    emulator: the one long CPU case of this file.)"""
    cfg, sd, ids, mask, want = module_case("FLAN1", 2, 64, "prefix")
    assert ops.gated_linear_ws_bytes(2 * 64, cfg.d_model, cfg.d_ff) > 0
    out = native(cfg, sd, dev)(ids.to(dev), mask.to(dev))
    check("T5GatedEncoder flan geometry", out, want, TOL_MODULE)


# ---------------------------------------------------------------------------------------------------------------- loading
def test_gated_load_hf_state_dict_and_constructor_errors():
    cfg = t5_gated_ref.TINY
    sd = t5_gated_ref.random_state_dict(cfg, seed=2, extra_heads=True)
    enc = T5GatedEncoder(cfg.vocab_size, cfg.d_model, cfg.d_kv, cfg.d_ff, cfg.num_layers, cfg.num_heads)
    enc.load_hf_state_dict(sd)   # decoder.* / lm_head.* / encoder.embed_tokens.weight are ignored
    assert enc.w_i.shape == (cfg.num_layers, 2, cfg.d_ff, cfg.d_model) and enc.w_i[1, 0].is_contiguous()
    assert torch.equal(enc.embed, sd["shared.weight"])
    assert torch.equal(enc.w_i[1, 0], sd["encoder.block.1.layer.1.DenseReluDense.wi_0.weight"])   # the gate
    assert torch.equal(enc.w_i[1, 1], sd["encoder.block.1.layer.1.DenseReluDense.wi_1.weight"])   # the up projection
    assert torch.equal(enc.w_o2[0], sd["encoder.block.0.layer.1.DenseReluDense.wo.weight"])
    before = {k: v.clone() for k, v in enc.state_dict().items()}
    for key in ("shared.weight", "encoder.block.1.layer.1.DenseReluDense.wi_0.weight",
                "encoder.block.0.layer.1.DenseReluDense.wi_1.weight", "encoder.block.1.layer.1.DenseReluDense.wo.weight"):
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            enc.load_hf_state_dict({k: v for k, v in sd.items() if k != key})
    with pytest.raises(KeyError, match=r"DenseReluDense\.wi_0\.weight"):   # a ReLU checkpoint: wi in place of wi_0 / wi_1
        enc.load_hf_state_dict(t5_ref.random_state_dict(cfg, seed=2))
    other = {k: torch.full_like(v, 3.0) for k, v in sd.items()}   # would change every weight if any of it were written
    for i in (0, 1):
        key = f"encoder.block.0.layer.1.DenseReluDense.wi_{i}.weight"
        bad = dict(other)
        bad[key] = torch.zeros(cfg.d_ff + 1, cfg.d_model)
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            enc.load_hf_state_dict(bad)
        bad[key] = torch.zeros(cfg.d_model, cfg.d_ff)
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            enc.load_hf_state_dict(bad)
    after = enc.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before), \
        "a refused load changed the weights"
    enc.load_hf_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()})   # any float dtype, stored as fp32
    assert all(q.dtype == torch.float32 for q in enc.parameters())
    assert torch.equal(enc.w_i[0, 1], sd["encoder.block.0.layer.1.DenseReluDense.wi_1.weight"].to(torch.bfloat16).float())
    for proj in ("relu", "gated-silu", "gelu"):
        with pytest.raises(NotImplementedError, match="gated-gelu"):
            T5GatedEncoder(96, 48, 8, 80, 2, 3, feed_forward_proj=proj)
    with pytest.raises(NotImplementedError, match="d_kv"):
        T5GatedEncoder(96, 48, 12, 80, 2, 3)
    with pytest.raises(NotImplementedError, match="gated"):   # the ReLU class still refuses, and names the class that does it
        T5Encoder(96, 48, 8, 80, 2, 3, feed_forward_proj="gated-gelu")
    with pytest.raises(NotImplementedError, match="T5GatedEncoder"):
        T5Encoder(96, 48, 8, 80, 2, 3, feed_forward_proj="gated-gelu")
    with pytest.raises(ValueError):
        enc(torch.zeros(1, 513, dtype=torch.int64))
    with pytest.raises(TypeError):
        enc(torch.zeros(1, 5, dtype=torch.int32))


def test_from_pretrained_and_load_t5_encoder(dev, tmp_path):
    """A tiny random model saved with save_pretrained and loaded from that directory (local files only, nothing fetched)."""
    transformers = pytest.importorskip("transformers")
    cfg = t5_gated_ref.TINY
    ids, mask = torch.randint(0, cfg.vocab_size, (2, 7), generator=torch.Generator().manual_seed(3)), prefix_mask(2, 7)
    dirs = {}
    for proj in ("gated-gelu", "relu", "gated-silu"):
        torch.manual_seed(11)
        hf = transformers.T5EncoderModel(hf_config(transformers, cfg, proj)).eval()
        dirs[proj] = str(tmp_path / proj)
        hf.save_pretrained(dirs[proj])
        if proj == "gated-gelu":
            sd = {k: v.clone() for k, v in hf.state_dict().items()}
    want = t5_gated_ref.encode(sd, cfg, ids, mask)
    for enc in (T5GatedEncoder.from_pretrained(dirs["gated-gelu"]), text.load_t5_encoder(dirs["gated-gelu"])):
        assert type(enc) is T5GatedEncoder
        assert torch.equal(enc.w_i[0, 0], sd["encoder.block.0.layer.1.DenseReluDense.wi_0.weight"])
        check("from_pretrained gated", enc.to(dev)(ids.to(dev), mask.to(dev)), want, TOL_MODULE)
    relu = text.load_t5_encoder(dirs["relu"])
    assert type(relu) is T5Encoder and relu.w_i.shape == (cfg.num_layers, cfg.d_ff, cfg.d_model)
    with pytest.raises(NotImplementedError, match="gated-gelu"):
        T5GatedEncoder.from_pretrained(dirs["relu"])
    with pytest.raises(NotImplementedError, match="gated-gelu"):
        T5GatedEncoder.from_pretrained(dirs["gated-silu"])
    with pytest.raises(NotImplementedError, match="gated-silu"):
        text.load_t5_encoder(dirs["gated-silu"])
    with pytest.raises(NotImplementedError, match="needs the 'no-such-t5-checkpoint' weights in the local HuggingFace cache"):
        text.load_t5_encoder("no-such-t5-checkpoint")


# -------------------------------------------------------------------------------------------------------------- plumbing
def test_gated_embedder_feeds_the_unet(dev):
    cfg = t5_gated_ref.TINY
    sd = t5_gated_ref.random_state_dict(cfg, seed=4)
    tok = HashTokenizer(cfg.vocab_size)
    torch.manual_seed(0)
    model = adp.DiffusionModel(net_t=adp.UNetV0, use_text_conditioning=True,
                               text_embedder=T5Embedder(native(cfg, sd, "cpu"), tok, max_length=9), **UNET).to(dev)
    net = model.net
    assert isinstance(net, adp.components.TextConditioningNet) and isinstance(net.embedder.encoder, T5GatedEncoder)
    t = tok(TEXTS, max_length=9)
    e_ref = t5_gated_ref.encode(sd, cfg, t["input_ids"], t["attention_mask"]).float()
    e = net.embedder(TEXTS)
    assert e.shape == (2, 9, cfg.d_model) and e.device.type == dev.type
    check("T5Embedder(T5GatedEncoder)", e, e_ref, TOL_MODULE)
    g = torch.Generator().manual_seed(21)
    x, time = torch.randn(2, 2, 64, generator=g).to(dev), torch.tensor([0.2, 0.6]).to(dev)
    with torch.no_grad():
        y = net(x, time, text=TEXTS)
        check("net(text=) vs net(embedding=t5_gated_ref)", y, net.net(x, time, embedding=e_ref.to(dev)), TOL_MODULE)
        y_other = net(x, time, text=["a violin", "rain on a tin roof at night"])
    assert not torch.allclose(y, y_other), "the text does not reach cross attention"
    noise = torch.randn(2, 2, 64, generator=g).to(dev)
    out = model.sample(noise, text=TEXTS, num_steps=2)
    assert out.shape == noise.shape and torch.isfinite(out).all()
    assert not torch.allclose(out, model.sample(noise, text=TEXTS[::-1], num_steps=2))


# --------------------------------------------------------------------------------------------------------------- capture
@pytest.mark.gpu
def test_gated_encoder_replays_from_a_graph(hip):
    cfg, sd, ids, mask, _ = module_case("TINY", 3, 64, "prefix")
    enc = native(cfg, sd, hip)
    ids_a, mask_a = ids.to(hip), mask.to(hip)
    ids_b = torch.randint(0, cfg.vocab_size, ids.shape, generator=torch.Generator().manual_seed(99)).to(hip)
    mask_b = mask_a.flip(0).contiguous()
    eager_a, eager_b = enc(ids_a, mask_a).clone(), enc(ids_b, mask_b).clone()   # (the first call uploads the bucket table)
    assert not torch.equal(eager_a, eager_b)
    ids_s, mask_s = ids_a.clone(), mask_a.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enc(ids_s, mask_s)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = enc(ids_s, mask_s)
    graph.replay()
    assert torch.equal(out, eager_a)
    ids_s.copy_(ids_b)
    mask_s.copy_(mask_b)
    graph.replay()
    assert torch.equal(out, eager_b)
