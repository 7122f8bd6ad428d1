"""Plain-torch restatement of the T5 encoder stack (eval mode, ReLU feed-forward) for tests/test_t5.py: a state dict with
transformers' key names, a config, token ids and a key mask in, the last hidden state out, in float64 by default.  It holds
no transformers code; tests/test_t5.py checks it against transformers.T5EncoderModel where that is importable.

    1. h = shared[ids]
    per block n:
    2. a = rmsnorm(h, layer.0.layer_norm)                      x * rsqrt(mean x^2 + eps) * g, no mean subtraction, no bias
    3. q, k, v = a Wq^T, a Wk^T, a Wv^T                        bias-free, split into heads of d_kv
    4. S = q k^T + bias[bucket(j - i)] + (-FLT_MAX where the key is masked); P = softmax(S); o = P v      no 1 / sqrt(d_kv)
    5. h = h + o Wo^T
    6. a = rmsnorm(h, layer.1.layer_norm);  h = h + relu(a Wi^T) Wo^T
    7. out = rmsnorm(h, final_layer_norm)
"""
import math
from types import SimpleNamespace

import torch

FLT_MAX = torch.finfo(torch.float32).max


def config(vocab_size, d_model, d_kv, d_ff, num_layers, num_heads, num_buckets=32, max_distance=128, eps=1e-6):
    return SimpleNamespace(vocab_size=vocab_size, d_model=d_model, d_kv=d_kv, d_ff=d_ff, num_layers=num_layers,
                           num_heads=num_heads, num_buckets=num_buckets, max_distance=max_distance, eps=eps)


TINY = config(96, 48, 8, 80, 2, 3)
BASE2 = config(512, 768, 64, 3072, 2, 12)   # t5-base's geometry, 2 layers, a small vocabulary


def bucket(rel, num_buckets, max_distance):
    """T5's bidirectional bucket of the relative positions `rel` = key - query (any integer tensor), float32 formula."""
    nb = num_buckets // 2
    out = (rel > 0).long() * nb
    n = rel.abs()
    max_exact = nb // 2
    large = max_exact + (torch.log(n.clamp(min=1).to(torch.float32) / max_exact) / math.log(max_distance / max_exact)
                         * (nb - max_exact)).long()
    large = large.clamp(max=nb - 1)
    return out + torch.where(n < max_exact, n, large)


def random_state_dict(cfg, seed=0, extra_heads=False):
    """A state dict with transformers' key names: norm weights 1 + 0.2 randn, bias table randn, matrices at their fan-in
    scale.  extra_heads: also the keys of the other T5 classes that a loader must ignore."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, std=1.0: torch.randn(*s, generator=g) * std   # noqa: E731
    inner, d = cfg.num_heads * cfg.d_kv, cfg.d_model
    sd = {"shared.weight": r(cfg.vocab_size, d)}
    sd["encoder.embed_tokens.weight"] = sd["shared.weight"]
    for n in range(cfg.num_layers):
        att, ff = f"encoder.block.{n}.layer.0.", f"encoder.block.{n}.layer.1."
        for p in "qkv":
            sd[att + f"SelfAttention.{p}.weight"] = r(inner, d, std=d ** -0.5)
        sd[att + "SelfAttention.o.weight"] = r(d, inner, std=inner ** -0.5)
        if n == 0:
            sd[att + "SelfAttention.relative_attention_bias.weight"] = r(cfg.num_buckets, cfg.num_heads)
        sd[att + "layer_norm.weight"] = 1 + r(d, std=0.2)
        sd[ff + "DenseReluDense.wi.weight"] = r(cfg.d_ff, d, std=d ** -0.5)
        sd[ff + "DenseReluDense.wo.weight"] = r(d, cfg.d_ff, std=cfg.d_ff ** -0.5)
        sd[ff + "layer_norm.weight"] = 1 + r(d, std=0.2)
    sd["encoder.final_layer_norm.weight"] = 1 + r(d, std=0.2)
    if extra_heads:
        sd["decoder.block.0.layer.0.SelfAttention.q.weight"] = r(3, 5)
        sd["decoder.final_layer_norm.weight"] = r(7)
        sd["lm_head.weight"] = r(4, 4)
    return sd


def rmsnorm(x, g, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * g


def attention(q, k, v, bias, mask, dtype=torch.float64):
    """q, k, v [B, H, m, dk], bias [H, m, m], mask [B, m] (0: masked) or None -> [B, H, m, dk], the literal arithmetic."""
    S = q.to(dtype) @ k.to(dtype).transpose(-1, -2) + bias.to(dtype)[None]
    if mask is not None:
        S = S + torch.where(mask[:, None, None, :] != 0, 0.0, -FLT_MAX).to(dtype)
    S = S - S.amax(-1, keepdim=True)
    P = torch.exp(S)
    P = P / P.sum(-1, keepdim=True)
    return P @ v.to(dtype)


def position_bias(table, m, num_buckets, max_distance):
    """table [nb, H] -> [H, m(query), m(key)]."""
    pos = torch.arange(m)
    b = bucket(pos[None, :] - pos[:, None], num_buckets, max_distance)
    return table[b].permute(2, 0, 1)


def encode(sd, cfg, ids, mask=None, dtype=torch.float64):
    w = lambda k: sd[k].to(dtype)   # noqa: E731
    B, m = ids.shape
    H, dk = cfg.num_heads, cfg.d_kv
    heads = lambda t: t.view(B, m, H, dk).transpose(1, 2)   # noqa: E731
    bias = position_bias(w("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"), m, cfg.num_buckets,
                         cfg.max_distance)
    h = w("shared.weight")[ids]
    for n in range(cfg.num_layers):
        att, ff = f"encoder.block.{n}.layer.0.", f"encoder.block.{n}.layer.1."
        a = rmsnorm(h, w(att + "layer_norm.weight"), cfg.eps)
        q, k, v = (heads(a @ w(att + f"SelfAttention.{p}.weight").T) for p in "qkv")
        o = attention(q, k, v, bias, mask, dtype).transpose(1, 2).reshape(B, m, H * dk)
        h = h + o @ w(att + "SelfAttention.o.weight").T
        a = rmsnorm(h, w(ff + "layer_norm.weight"), cfg.eps)
        h = h + torch.relu(a @ w(ff + "DenseReluDense.wi.weight").T) @ w(ff + "DenseReluDense.wo.weight").T
    return rmsnorm(h, w("encoder.final_layer_norm.weight"), cfg.eps)
