"""The native T5 text encoder (audio_diffusion_pytorch_amd/text.py) and its kernels (csrc/t5.hip, include/adp_t5.h).

Kernel parity against float64 torch on the CPU, outputs pre-filled with NaN, bound 1e-4 (the single-kernel bound of
tests/test_kernels.py); module parity against tests/t5_ref.py, bound 1e-3 (the module bound of tests/test_unet.py); t5_ref.py
itself against transformers.T5EncoderModel where transformers is importable.  Every `dev` test runs on the SIMT emulator and,
with -m gpu, on the gfx950 library."""
import functools
import zlib

import pytest
import torch

import audio_diffusion_pytorch_amd as adp
from audio_diffusion_pytorch_amd import _C, ops
from audio_diffusion_pytorch_amd.text import T5Embedder, T5Encoder, relative_position_buckets
from conftest import rel_err

import t5_ref

TOL = 1e-4       # single kernels
TOL_MODULE = 1e-3
NULL, SHAPE, UNSUPPORTED = -5, -1, -2
FLT_MAX = t5_ref.FLT_MAX


def nan_like(shape, dev):
    return torch.full(tuple(shape), float("nan"), dtype=torch.float32, device=dev)


def p(t):
    return None if t is None else _C.ptr(t, t.dtype)


def check(name, got, want, tol=TOL):
    assert torch.isfinite(got).all(), f"{name}: an element was left unwritten (NaN pre-fill) or is not finite"
    err = rel_err(got, want)
    print(f"{name}: rel err {err:.3e} (bound {tol:.0e})")
    assert err < tol, (name, err)


def prefix_mask(B, m):
    """Row b keeps the first [m, max(1, m // 3), 1][b % 3] keys."""
    lens = [m, max(1, m // 3), 1]
    return torch.stack([(torch.arange(m) < lens[b % 3]).to(torch.int64) for b in range(B)])


# ------------------------------------------------------------------------------------- the restatement is the transformers encoder
@pytest.mark.parametrize("m", [5, 64, 150])
@pytest.mark.parametrize("cfg", [t5_ref.TINY, t5_ref.BASE2], ids=["tiny", "base2"])
def test_restatement_against_transformers(cfg, m):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(7)
    hf = transformers.T5EncoderModel(transformers.T5Config(
        vocab_size=cfg.vocab_size, d_model=cfg.d_model, d_kv=cfg.d_kv, d_ff=cfg.d_ff, num_layers=cfg.num_layers,
        num_heads=cfg.num_heads, relative_attention_num_buckets=cfg.num_buckets,
        relative_attention_max_distance=cfg.max_distance, layer_norm_epsilon=cfg.eps, feed_forward_proj="relu",
        dropout_rate=0.0)).eval()
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
        got = t5_ref.encode(hf.state_dict(), cfg, ids, mask)
        err = rel_err(got, want)
        print(f"t5_ref vs transformers, m {m}, {what} mask: rel err {err:.3e}")
        assert err < TOL, (what, err)


def test_bucket_table_is_the_restatements():
    for m, nb, md in ((1, 32, 128), (5, 32, 128), (150, 32, 128), (512, 32, 128), (300, 8, 20)):
        pos = torch.arange(m)
        want = t5_ref.bucket(pos[None, :] - pos[:, None], nb, md)
        got = relative_position_buckets(m, nb, md)
        assert got.dtype == torch.int32 and got.shape == (2 * m - 1,)
        assert torch.equal(got.long()[(pos[None, :] - pos[:, None]) + m - 1], want)
        assert int(got.min()) >= 0 and int(got.max()) < nb


# ------------------------------------------------------------------------------------------------------------- linear
# (64, 768, 96): 2 output tiles, so the k sum is cut into 6 segments of 128 (about 512 workgroups, segments >= 128)
LIN_SPLIT = (64, 768, 96)
LIN_SHAPES = [(1, 1, 1), (5, 7, 3), (32, 32, 32), (70, 130, 45), LIN_SPLIT]


@functools.lru_cache(maxsize=None)
def lin_case(shape):
    T, K, N = shape
    g = torch.Generator().manual_seed(100 * T + 10 * K + N)
    x, w, res = torch.randn(T, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(T, N, generator=g)
    return dict(x=x, w=w, res=res, prod=x.double() @ w.double().T)


def lin_ref(d, relu, with_res):
    y = torch.relu(d["prod"]) if relu else d["prod"]
    return y + d["res"].double() if with_res else y


@pytest.mark.parametrize("shape", LIN_SHAPES, ids=lambda s: "T{}K{}N{}".format(*s))
def test_linear_kernel(dev, shape):
    T, K, N = shape
    d = lin_case(shape)
    lib, s = _C.lib(), _C.stream()
    x, w, res = (d[k].to(dev) for k in ("x", "w", "res"))
    nbytes = lib.adp_t5_linear_ws_bytes(T, K, N)
    assert nbytes >= 0 and nbytes % (T * N * 4) == 0
    if shape == LIN_SPLIT:
        assert nbytes // (T * N * 4) == 6, "the split rule no longer cuts this shape into 6 partials: choose another shape"
    if K <= 32:
        assert nbytes == 0
    for relu in (0, 1):
        for mode in ("none", "separate", "alias"):
            runs = []
            for _ in range(2):
                ws = nan_like((nbytes // 4,), dev) if nbytes else None
                y = res.clone() if mode == "alias" else nan_like((T, N), dev)
                r = {"none": None, "separate": res, "alias": y}[mode]
                assert lib.adp_t5_linear(p(x), p(w), p(r), T, K, N, relu, p(y), p(ws), s) == 0
                runs.append(y)
            check(f"linear relu{relu} res-{mode}", runs[0], lin_ref(d, relu, mode != "none"))
            assert torch.equal(runs[0], runs[1]), "not bit-identical from call to call"
    assert torch.equal(res.cpu(), d["res"]) and torch.equal(x.cpu(), d["x"])
    check("ops.t5_linear", ops.t5_linear(x, w, res=res, relu=True), lin_ref(d, 1, True))


# ------------------------------------------------------------------------------------------------------------ rmsnorm
@pytest.mark.parametrize("shape", [(1, 1), (5, 48), (3, 768), (2, 1030)], ids=lambda s: "T{}d{}".format(*s))
def test_rmsnorm_kernel(dev, shape):
    T, d = shape
    g = torch.Generator().manual_seed(T * 1000 + d)
    x, w = torch.randn(T, d, generator=g), 1 + 0.2 * torch.randn(d, generator=g)
    x[0] *= 1e4
    x[-1] *= 1e-4 if T > 1 else 1.0
    if T == 1:   # one row: both scales, one after the other
        xs = [x, x * 1e-8]
    else:
        xs = [x]
    for xi in xs:
        want = t5_ref.rmsnorm(xi.double(), w.double(), 1e-6)
        y = nan_like((T, d), dev)
        assert _C.lib().adp_t5_rmsnorm(p(xi.to(dev)), p(w.to(dev)), T, d, 1e-6, p(y), _C.stream()) == 0
        assert torch.isfinite(y).all()
        for t in range(T):   # per row: the rows differ in scale by 1e8
            check(f"rmsnorm row {t}", y[t], want[t])
        assert torch.equal(ops.t5_rmsnorm(xi.to(dev), w.to(dev), 1e-6), y)


# -------------------------------------------------------------------------------------------------------------- embed
def test_embed_kernel(dev):
    V, d = 11, 5
    table = torch.randn(V, d, generator=torch.Generator().manual_seed(3))
    ids = torch.tensor([0, V - 1, -1, V, 4, 4, 10, 1], dtype=torch.int64)
    out = nan_like((ids.numel(), d), dev)
    assert _C.lib().adp_t5_embed(p(ids.to(dev)), p(table.to(dev)), ids.numel(), V, d, p(out), _C.stream()) == 0
    want = table[ids.clamp(0, V - 1)]
    want[2] = 0
    want[3] = 0
    assert torch.equal(out.cpu(), want)
    assert torch.equal(ops.t5_embed(ids.to(dev), table.to(dev)), out)


# --------------------------------------------------------------------------------------------------------------- attn
ATTN_SHAPES = [(1, 1, 8, 1), (2, 3, 8, 5), (1, 2, 64, 64), (2, 2, 16, 150), (1, 1, 128, 33), (1, 1, 8, 512)]
ATTN_MASKS = ["none", "prefix", "scattered", "zero_row"]
NB = 32


def attn_mask(kind, B, m, g):
    if kind == "none":
        return None
    if kind == "prefix":
        return prefix_mask(B, m).to(torch.uint8)
    if kind == "scattered":   # not a prefix: key 0 masked wherever there is a second key, random bits behind it
        mk = (torch.rand(B, m, generator=g) < 0.5).to(torch.uint8)
        mk[:, -1] = 1
        if m > 1:
            mk[:, 0] = 0
        return mk
    mk = prefix_mask(B, m).to(torch.uint8)
    mk[0] = 0   # every key of batch row 0 masked: uniform weights
    return mk


@functools.lru_cache(maxsize=None)
def attn_case(shape):
    B, H, dk, m = shape
    g = torch.Generator().manual_seed(1000 * m + 10 * dk + H)
    qkv = torch.randn(B, m, 3 * H * dk, generator=g)
    qkv[..., :H * dk] *= 2.0 / dk ** 0.5    # scores of a few units: a softmax that is neither flat nor one-hot
    table = torch.randn(NB, H, generator=g) * 8
    table[0, :], table[NB - 1, 0] = 30.0, -30.0   # entries up to +-30
    bucket = relative_position_buckets(m, NB, 128)
    pos = torch.arange(m)
    bias = table[bucket.long()[(pos[None, :] - pos[:, None]) + m - 1]].permute(2, 0, 1)   # [H, query, key]
    q, k, v = (t.reshape(B, m, H, dk).transpose(1, 2) for t in qkv.split(H * dk, dim=-1))
    refs = {}
    for kind in ATTN_MASKS:
        mk = attn_mask(kind, B, m, torch.Generator().manual_seed(m))
        o = t5_ref.attention(q, k, v, bias, mk)
        refs[kind] = (mk, o.transpose(1, 2).reshape(B, m, H * dk))
    return dict(qkv=qkv, table=table, bucket=bucket, v=v, refs=refs)


@pytest.mark.parametrize("kind", ATTN_MASKS)
@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=lambda s: "B{}H{}dk{}m{}".format(*s))
def test_attn_kernel(dev, shape, kind):
    B, H, dk, m = shape
    d = attn_case(shape)
    mk, want = d["refs"][kind]
    qkv, table, bucket = d["qkv"].to(dev), d["table"].to(dev), d["bucket"].to(dev)
    mkd = None if mk is None else mk.to(dev)
    runs = []
    for _ in range(2):
        out = nan_like((B, m, H * dk), dev)
        assert _C.lib().adp_t5_attn(p(qkv), p(table), p(bucket), p(mkd), B, H, dk, m, NB, p(out), _C.stream()) == 0
        runs.append(out)
    check(f"attn {kind}", runs[0], want)
    assert torch.equal(runs[0], runs[1]), "not bit-identical from call to call"
    if kind == "zero_row":   # uniform weights: every query of batch row 0 gets the mean of v over the keys
        mean = d["v"][0].double().mean(dim=1)                       # [H, dk]
        check("attn all-masked row", runs[0][0], mean.reshape(1, H * dk).expand(m, -1))
    if kind == "prefix" and B > 1 and m > 1:   # a masked key has the weight 0 exactly: its v does not reach the output
        qkv2 = d["qkv"].clone()
        qkv2[1, max(1, m // 3):, 2 * H * dk:] = 1e30
        out2 = nan_like((B, m, H * dk), dev)
        assert _C.lib().adp_t5_attn(p(qkv2.to(dev)), p(table), p(bucket), p(mkd), B, H, dk, m, NB, p(out2), _C.stream()) == 0
        assert torch.equal(out2[1], runs[0][1])
    assert torch.equal(ops.t5_attn(qkv, table, bucket, mkd, H), runs[0])


def test_error_codes(dev):
    lib, s = _C.lib(), _C.stream()
    x, w, y = torch.randn(4, 8).to(dev), torch.randn(3, 8).to(dev), nan_like((4, 3), dev)
    lin = lambda *a: lib.adp_t5_linear(*a, s)   # noqa: E731
    assert lin(None, p(w), None, 4, 8, 3, 0, p(y), None) == NULL
    assert lin(p(x), None, None, 4, 8, 3, 0, p(y), None) == NULL
    assert lin(p(x), p(w), None, 4, 8, 3, 0, None, None) == NULL
    for bad in ((0, 8, 3), (4, 0, 3), (4, 8, 0), (4, -1, 3), (1 << 20, 1 << 20, 3)):
        assert lin(p(x), p(w), None, *bad, 0, p(y), None) == SHAPE
        assert lib.adp_t5_linear_ws_bytes(*bad) == SHAPE
    big = torch.randn(64, 768).to(dev)
    assert lib.adp_t5_linear_ws_bytes(*LIN_SPLIT) > 0
    y2 = nan_like((64, 96), dev)
    assert lin(p(big), p(big), None, *LIN_SPLIT, 0, p(y2), None) == NULL   # a workspace is needed and missing
    g, yn = torch.ones(8).to(dev), nan_like((4, 8), dev)
    assert lib.adp_t5_rmsnorm(None, p(g), 4, 8, 1e-6, p(yn), s) == NULL
    assert lib.adp_t5_rmsnorm(p(x), None, 4, 8, 1e-6, p(yn), s) == NULL
    assert lib.adp_t5_rmsnorm(p(x), p(g), 4, 8, 1e-6, None, s) == NULL
    assert lib.adp_t5_rmsnorm(p(x), p(g), 0, 8, 1e-6, p(yn), s) == SHAPE
    assert lib.adp_t5_rmsnorm(p(x), p(g), 4, 0, 1e-6, p(yn), s) == SHAPE
    ids = torch.zeros(4, dtype=torch.int64).to(dev)
    assert lib.adp_t5_embed(None, p(w), 4, 3, 8, p(yn), s) == NULL
    assert lib.adp_t5_embed(p(ids), None, 4, 3, 8, p(yn), s) == NULL
    assert lib.adp_t5_embed(p(ids), p(w), 4, 3, 8, None, s) == NULL
    for bad in ((0, 3, 8), (4, 0, 8), (4, 3, 0)):
        assert lib.adp_t5_embed(p(ids), p(w), *bad, p(yn), s) == SHAPE
    B, H, dk, m = 1, 1, 8, 4
    qkv, table = torch.randn(B, m, 3 * H * dk).to(dev), torch.randn(NB, H).to(dev)
    bucket, out = relative_position_buckets(m, NB, 128).to(dev), nan_like((B, m, H * dk), dev)
    att = lambda *a: lib.adp_t5_attn(*a, s)   # noqa: E731
    assert att(None, p(table), p(bucket), None, B, H, dk, m, NB, p(out)) == NULL
    assert att(p(qkv), None, p(bucket), None, B, H, dk, m, NB, p(out)) == NULL
    assert att(p(qkv), p(table), None, None, B, H, dk, m, NB, p(out)) == NULL
    assert att(p(qkv), p(table), p(bucket), None, B, H, dk, m, NB, None) == NULL
    for bad in ((0, H, dk, m, NB), (B, 0, dk, m, NB), (B, H, 0, m, NB), (B, H, dk, 0, NB), (B, H, dk, m, 0), (70000, H, dk, m, NB)):
        assert att(p(qkv), p(table), p(bucket), None, *bad, p(out)) == SHAPE
    for bad_dk in (4, 12, 136, 7):
        assert att(p(qkv), p(table), p(bucket), None, B, H, bad_dk, m, NB, p(out)) == UNSUPPORTED
    assert att(p(qkv), p(table), p(bucket), None, B, H, dk, 513, NB, p(out)) == UNSUPPORTED
    assert att(None, p(table), p(bucket), None, 0, H, 4, m, NB, p(out)) == NULL      # NULL before SHAPE before UNSUPPORTED
    assert att(p(qkv), p(table), p(bucket), None, 0, H, 4, m, NB, p(out)) == SHAPE
    for t in (y, y2, yn, out):   # a refused call writes nothing
        assert torch.isnan(t).all()


# ------------------------------------------------------------------------------------------------------------ the module
def native(cfg, sd, dev):
    enc = T5Encoder(cfg.vocab_size, cfg.d_model, cfg.d_kv, cfg.d_ff, cfg.num_layers, cfg.num_heads, cfg.num_buckets,
                    cfg.max_distance, cfg.eps)
    enc.load_hf_state_dict(sd)
    return enc.to(dev)


@functools.lru_cache(maxsize=None)
def module_case(name, B, m, kind):
    cfg = getattr(t5_ref, name)
    sd = t5_ref.random_state_dict(cfg, seed=1)
    ids = torch.randint(0, cfg.vocab_size, (B, m), generator=torch.Generator().manual_seed(m))
    mask = {"none": None, "prefix": prefix_mask(B, m), "zero": torch.zeros(B, m, dtype=torch.int64)}[kind]
    return cfg, sd, ids, mask, t5_ref.encode(sd, cfg, ids, mask)


@pytest.mark.parametrize("kind", ["none", "prefix", "zero"])
@pytest.mark.parametrize("m", [5, 64, 150])
def test_encoder_tiny(dev, m, kind):
    cfg, sd, ids, mask, want = module_case("TINY", 3, m, kind)
    enc = native(cfg, sd, dev)
    assert all(not q.requires_grad for q in enc.parameters())
    out = enc(ids.to(dev), None if mask is None else mask.to(dev))
    assert out.shape == (3, m, cfg.d_model) and not out.requires_grad
    check(f"T5Encoder tiny m{m} {kind}", out, want, TOL_MODULE)


def test_encoder_base_geometry(dev):
    """t5-base's widths (768 / 12 heads of 64 / 3072), 2 layers: every GEMM of the real model at its real k length, cut and
    uncut.  (The emulated run is about 2 G multiply-adds through the fiber emulator: the one long CPU case of this file.)"""
    cfg, sd, ids, mask, want = module_case("BASE2", 2, 64, "prefix")
    out = native(cfg, sd, dev)(ids.to(dev), mask.to(dev))
    check("T5Encoder base geometry", out, want, TOL_MODULE)


def test_load_hf_state_dict_and_constructor_errors():
    cfg = t5_ref.TINY
    sd = t5_ref.random_state_dict(cfg, seed=2, extra_heads=True)
    enc = T5Encoder(cfg.vocab_size, cfg.d_model, cfg.d_kv, cfg.d_ff, cfg.num_layers, cfg.num_heads)
    enc.load_hf_state_dict(sd)   # decoder.* / lm_head.* / encoder.embed_tokens.weight are ignored
    inner = cfg.num_heads * cfg.d_kv
    assert torch.equal(enc.embed, sd["shared.weight"])
    assert torch.equal(enc.w_qkv[1][inner:2 * inner], sd["encoder.block.1.layer.0.SelfAttention.k.weight"])
    assert torch.equal(enc.rel_bias, sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"])
    assert torch.equal(enc.w_o2[0], sd["encoder.block.0.layer.1.DenseReluDense.wo.weight"])
    for key in ("shared.weight", "encoder.block.1.layer.0.SelfAttention.v.weight", "encoder.final_layer_norm.weight",
                "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight",
                "encoder.block.1.layer.1.DenseReluDense.wi.weight"):
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            enc.load_hf_state_dict({k: v for k, v in sd.items() if k != key})
    bad = dict(sd)
    bad["encoder.block.0.layer.1.DenseReluDense.wi.weight"] = torch.zeros(cfg.d_ff + 1, cfg.d_model)
    with pytest.raises(ValueError, match="DenseReluDense.wi.weight"):
        enc.load_hf_state_dict(bad)
    assert torch.equal(enc.embed, sd["shared.weight"]), "a refused load changed the weights"
    with pytest.raises(NotImplementedError, match="gated"):
        T5Encoder(96, 48, 8, 80, 2, 3, feed_forward_proj="gated-gelu")
    with pytest.raises(NotImplementedError, match="d_kv"):
        T5Encoder(96, 48, 12, 80, 2, 3)
    with pytest.raises(ValueError):
        enc(torch.zeros(1, 513, dtype=torch.int64))
    with pytest.raises(TypeError):
        enc(torch.zeros(1, 5, dtype=torch.int32))


def test_from_pretrained_without_local_weights_says_so():
    pytest.importorskip("transformers")
    with pytest.raises(NotImplementedError, match="needs the 'no-such-t5-checkpoint' weights in the local HuggingFace cache"):
        T5Encoder.from_pretrained("no-such-t5-checkpoint")


# -------------------------------------------------------------------------------------------------------------- plumbing
class HashTokenizer:
    """Stand-in tokenizer: a deterministic hash of each word to an id in [2, vocab), 1 closes the text, 0 pads."""

    def __init__(self, vocab_size):
        self.vocab_size = vocab_size

    def __call__(self, texts, truncation=True, max_length=64, padding="max_length", return_tensors="pt"):
        assert truncation and padding == "max_length" and return_tensors == "pt"
        ids = torch.zeros(len(texts), max_length, dtype=torch.int64)
        mask = torch.zeros(len(texts), max_length, dtype=torch.int64)
        for b, text in enumerate(texts):
            toks = [2 + zlib.crc32(wd.encode()) % (self.vocab_size - 2) for wd in text.split()][:max_length - 1] + [1]
            ids[b, :len(toks)] = torch.tensor(toks)
            mask[b, :len(toks)] = 1
        return {"input_ids": ids, "attention_mask": mask}


# (resnet_groups=4: with one channel per group a conv bias in front of a GroupNorm has an identically zero gradient, which no
# relative error can be taken of)
UNET = dict(in_channels=2, channels=[8, 16], factors=[2, 2], items=[1, 1], modulation_features=32, resnet_groups=4,
            cross_attentions=[0, 1], attention_heads=2, attention_features=8, embedding_features=t5_ref.TINY.d_model)
TEXTS = ["a dog barking in the rain", "piano"]


def test_embedder_feeds_the_unet(dev):
    cfg = t5_ref.TINY
    sd = t5_ref.random_state_dict(cfg, seed=4)
    tok = HashTokenizer(cfg.vocab_size)
    torch.manual_seed(0)
    net = adp.UNetV0(dim=1, use_text_conditioning=True, text_embedder=T5Embedder(native(cfg, sd, "cpu"), tok, max_length=9),
                     **UNET).to(dev)
    assert isinstance(net, adp.components.TextConditioningNet)
    t = tok(TEXTS, max_length=9)
    e_ref = t5_ref.encode(sd, cfg, t["input_ids"], t["attention_mask"]).float()
    g = torch.Generator().manual_seed(21)
    x, time = torch.randn(2, 2, 64, generator=g).to(dev), torch.tensor([0.2, 0.6]).to(dev)
    e = net.embedder(TEXTS)
    assert e.shape == (2, 9, cfg.d_model) and e.device.type == dev.type
    check("T5Embedder", e, e_ref, TOL_MODULE)
    params = dict(net.net.named_parameters())
    y = net(x, time, text=TEXTS)
    y.sum().backward()
    grads = {n: q.grad.clone() for n, q in params.items() if q.grad is not None}
    assert grads, "no parameter gradient"
    for q in params.values():
        q.grad = None
    y_ref = net.net(x, time, embedding=e_ref.to(dev))
    y_ref.sum().backward()
    check("net(text=) vs net(embedding=t5_ref)", y, y_ref, TOL_MODULE)
    for n, q in params.items():
        if q.grad is not None:
            check(f"grad {n}", grads[n], q.grad, TOL_MODULE)
    assert all(q.grad is None for q in net.embedder.parameters())
    for bad_id in (cfg.vocab_size, -1):   # refused on the host, as torch's embedding would refuse it

        def bad(texts, **kw):
            ids = torch.ones(len(texts), 9, dtype=torch.int64)
            ids[-1, 3] = bad_id
            return {"input_ids": ids, "attention_mask": torch.ones_like(ids)}
        with pytest.raises(ValueError, match="token id outside"):
            T5Embedder(net.embedder.encoder, bad, max_length=9)(TEXTS)


def test_sampling_encodes_the_text_once(dev):
    cfg = t5_ref.TINY
    enc = native(cfg, t5_ref.random_state_dict(cfg, seed=5), "cpu")
    calls = []
    enc.register_forward_hook(lambda mod, a, o: calls.append(1))
    torch.manual_seed(0)
    model = adp.DiffusionModel(net_t=adp.UNetV0, use_text_conditioning=True,
                               text_embedder=T5Embedder(enc, HashTokenizer(cfg.vocab_size), max_length=9), **UNET).to(dev)
    noise = torch.randn(2, 2, 64, generator=torch.Generator().manual_seed(22)).to(dev)
    out = model.sample(noise, text=TEXTS, num_steps=3)
    assert out.shape == noise.shape and torch.isfinite(out).all()
    assert len(calls) == 1, "one encode per sampling run"


# --------------------------------------------------------------------------------------------------------------- capture
@pytest.mark.gpu
def test_encoder_replays_from_a_graph(hip):
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
