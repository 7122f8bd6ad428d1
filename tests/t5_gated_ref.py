"""Plain-torch restatement of the T5 v1.1 / flan-T5 encoder stack (eval mode, gated-GELU feed-forward) for
tests/test_t5_gated.py: tests/t5_ref.py with step 6 replaced by

    6. a = rmsnorm(h, layer.1.layer_norm);  h = h + (gelu_new(a Wi0^T) * (a Wi1^T)) Wo^T
       gelu_new(g) = 0.5 g (1 + tanh(sqrt(2 / pi) (g + 0.044715 g^3)))

Everything else (norm, attention, bias table, bucket, config) is imported from t5_ref.  It holds no transformers code;
tests/test_t5_gated.py checks it against transformers.T5EncoderModel(feed_forward_proj="gated-gelu") where that is importable.
"""
import math

import torch

from t5_ref import attention, bucket, config, position_bias, rmsnorm  # noqa: F401  (bucket: re-exported for the tests)

TINY = config(96, 48, 8, 80, 2, 3)
FLAN1 = config(512, 768, 64, 2048, 1, 12)   # flan-t5-base's geometry, 1 layer, a small vocabulary


def gelu_new(g):
    return 0.5 * g * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (g + 0.044715 * g.pow(3))))


def random_state_dict(cfg, seed=0, extra_heads=False):
    """t5_ref.random_state_dict with DenseReluDense.wi_0 (the gate) and wi_1 (the up projection) in place of wi."""
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
        sd[ff + "DenseReluDense.wi_0.weight"] = r(cfg.d_ff, d, std=d ** -0.5)
        sd[ff + "DenseReluDense.wi_1.weight"] = r(cfg.d_ff, d, std=d ** -0.5)
        sd[ff + "DenseReluDense.wo.weight"] = r(d, cfg.d_ff, std=cfg.d_ff ** -0.5)
        sd[ff + "layer_norm.weight"] = 1 + r(d, std=0.2)
    sd["encoder.final_layer_norm.weight"] = 1 + r(d, std=0.2)
    if extra_heads:
        sd["decoder.block.0.layer.0.SelfAttention.q.weight"] = r(3, 5)
        sd["decoder.final_layer_norm.weight"] = r(7)
        sd["lm_head.weight"] = r(4, 4)
    return sd


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
        gated = gelu_new(a @ w(ff + "DenseReluDense.wi_0.weight").T) * (a @ w(ff + "DenseReluDense.wi_1.weight").T)
        h = h + gated @ w(ff + "DenseReluDense.wo.weight").T
    return rmsnorm(h, w("encoder.final_layer_norm.weight"), cfg.eps)
