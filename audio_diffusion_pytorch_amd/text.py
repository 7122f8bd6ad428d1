"""The frozen T5 text encoders on the kernels of include/adp_t5.h and include/adp_gated.h, and the embedder that feeds them
to the U-Net:

    encoder = load_t5_encoder("google/flan-t5-base")          # T5Encoder or T5GatedEncoder, by the local config
    encoder = T5Encoder.from_pretrained("t5-base")            # or T5Encoder(...) + load_hf_state_dict(sd)
    net = UNetV0(..., use_text_conditioning=True, text_embedder=T5Embedder(encoder, tokenizer))
    net(x, t, text=["a dog barking", ...])

`components.T5Embedder` (the stock `transformers` model, the default when no `text_embedder` is given) is unchanged.  The
encoders here are T5's encoder stack as `transformers.T5EncoderModel` computes it in eval mode (tests/t5_ref.py and
tests/t5_gated_ref.py restate it and are checked against transformers): `T5Encoder` is the original T5 layout with the ReLU
feed-forward (t5-small/base/large), `T5GatedEncoder` the T5 v1.1 / flan-T5 layout with the gated-GELU feed-forward
h + wo(gelu_new(a wi_0^T) * (a wi_1^T)).  Forward only: every parameter is frozen and no kernel has a gradient.

Launches per encode: 1 embed, per block [rmsnorm, ONE q/k/v GEMM on the [3 H dk, d] weight packed at load time, attention,
output GEMM + residual, rmsnorm, wi GEMM + ReLU (gated: ONE gated GEMM on the [2, d_ff, d] weight pair, ops.gated_linear),
wo GEMM + residual], 1 final rmsnorm; a GEMM whose k sum is cut (ops.t5_linear, ops.gated_linear) is two kernels.  No host
synchronisation; after one eager call per sequence length (which uploads that length's bucket table) the forward can be
captured into a hipGraph.
"""
import math
from typing import List, Optional

import torch
import torch.nn as nn
from torch import Tensor

from . import ops

MAX_TOKENS = 512   # adp_t5_attn's limit, and t5's own positional range in practice


def relative_position_buckets(m: int, num_buckets: int, max_distance: int) -> Tensor:
    """int32 [2m - 1]: T5's bidirectional bucket of the relative position j - i at index j - i + m - 1, by the float32
    formula of transformers (num_buckets // 2 per sign, half of those exact, the rest logarithmic up to max_distance).
    Computed on the CPU: the formula truncates a float logarithm, and a device logf may land on the other side of an integer
    at power-of-two distances."""
    rel = torch.arange(-(m - 1), m, dtype=torch.long)
    nb = num_buckets // 2
    out = (rel > 0).to(torch.long) * nb
    n = rel.abs()
    max_exact = nb // 2
    is_small = n < max_exact
    # (n = 0 is always "small"; the clamp only keeps log(0) out of the discarded branch)
    large = max_exact + (torch.log(n.clamp(min=1).float() / max_exact) / math.log(max_distance / max_exact)
                         * (nb - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return (out + torch.where(is_small, n, large)).to(torch.int32)


def _missing_weights(model: str) -> str:
    # the text of components.T5Embedder's error: the way out is the same
    return (f"TextConditioningPlugin's default T5Embedder needs the '{model}' weights in the local HuggingFace "
            "cache; pass UNetV0(..., use_text_conditioning=True, text_embedder=<module: List[str] -> [B, m, E]>) "
            "or feed `embedding=` directly")


class T5Encoder(nn.Module):
    """input_ids int64 [B, m], attention_mask [B, m] or None -> last hidden state [B, m, d_model]."""
    FEED_FORWARD = "relu"   # the feed_forward_proj this class computes

    @staticmethod
    def _refusal(feed_forward_proj: str) -> str:
        return (f"T5Encoder: feed_forward_proj={feed_forward_proj!r} is not built here; T5Encoder covers the original T5 "
                "layout (t5-small/base/large: 'relu'), and the gated feed-forward of T5 v1.1 / flan-T5 ('gated-gelu') is "
                "text.T5GatedEncoder (text.load_t5_encoder picks the class from the local config)")

    def __init__(self, vocab_size: int, d_model: int, d_kv: int, d_ff: int, num_layers: int, num_heads: int,
                 relative_attention_num_buckets: int = 32, relative_attention_max_distance: int = 128,
                 layer_norm_epsilon: float = 1e-6, feed_forward_proj: str = "relu"):
        super().__init__()
        if feed_forward_proj != self.FEED_FORWARD:
            raise NotImplementedError(self._refusal(feed_forward_proj))
        if d_kv % 8 or not 8 <= d_kv <= 128:
            raise NotImplementedError(f"T5Encoder: d_kv must be a multiple of 8 in [8, 128] (adp_t5_attn); got {d_kv}")
        if relative_attention_num_buckets < 4:
            raise ValueError("T5Encoder: relative_attention_num_buckets must be at least 4")
        self.vocab_size, self.d_model, self.d_kv, self.d_ff = vocab_size, d_model, d_kv, d_ff
        self.num_layers, self.num_heads = num_layers, num_heads
        self.num_buckets, self.max_distance = relative_attention_num_buckets, relative_attention_max_distance
        self.eps = float(layer_norm_epsilon)
        L, inner = num_layers, num_heads * d_kv

        def frozen(*shape, std=None):
            t = torch.ones(*shape) if std is None else torch.randn(*shape) * std
            return nn.Parameter(t, requires_grad=False)
        self.embed = frozen(vocab_size, d_model, std=1.0)
        self.rel_bias = frozen(relative_attention_num_buckets, num_heads, std=1.0)   # block 0's table, shared by all blocks
        self.ln_attn = frozen(L, d_model)
        self.w_qkv = frozen(L, 3 * inner, d_model, std=d_model ** -0.5)              # rows: q | k | v, head major
        self.w_o = frozen(L, d_model, inner, std=inner ** -0.5)
        self.ln_ff = frozen(L, d_model)
        self._init_wi(frozen)
        self.w_o2 = frozen(L, d_model, d_ff, std=d_ff ** -0.5)
        self.ln_final = frozen(d_model)
        self._buckets = {}   # (m, device) -> int32 [2m - 1] on that device
        self._ws_bytes = {}  # T -> workspace bytes of the largest GEMM

    # ---- the feed-forward's first half: what T5GatedEncoder replaces
    def _init_wi(self, frozen) -> None:
        self.w_i = frozen(self.num_layers, self.d_ff, self.d_model, std=self.d_model ** -0.5)

    def _get_wi(self, get, ff: str) -> Tensor:
        """Block `ff`'s slice of w_i from a state dict (`get(key, shape)` checks and converts)."""
        return get(ff + "DenseReluDense.wi.weight", (self.d_ff, self.d_model))

    def _wi_ws_bytes(self, T: int) -> int:
        return ops.t5_linear_ws_bytes(T, self.d_model, self.d_ff)

    def _wi(self, n: int, a: Tensor, f: Tensor, ws: Optional[Tensor]) -> None:
        """f [T, d_ff] = block n's activation of the normed tokens a [T, d]: one launch (two where the k sum is cut)."""
        ops.t5_linear(a, self.w_i[n], relu=True, out=f, ws=ws)

    # ---- weights
    def load_hf_state_dict(self, sd) -> None:
        """Loads a state dict with transformers' key names (that of a T5EncoderModel, T5Model or T5ForConditionalGeneration):
        shared.weight, encoder.block.N.layer.0.SelfAttention.{q,k,v,o}.weight, block 0's relative_attention_bias.weight, the
        layer_norm weights, layer.1.DenseReluDense.{wi,wo}.weight and encoder.final_layer_norm.weight.  Every other key
        (encoder.embed_tokens.weight, decoder.*, lm_head.*) is ignored.  A missing key raises KeyError naming it, a tensor
        of another shape ValueError."""
        inner, d = self.num_heads * self.d_kv, self.d_model

        def get(key, shape):
            if key not in sd:
                raise KeyError(key)
            t = sd[key]
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{type(self).__name__}.load_hf_state_dict: {key!r} has shape {tuple(t.shape)}, expected {tuple(shape)}")
            return t.detach().to(dtype=torch.float32)

        staged = {"embed": get("shared.weight", (self.vocab_size, d)),
                  "rel_bias": get("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight",
                                  (self.num_buckets, self.num_heads)),
                  "ln_final": get("encoder.final_layer_norm.weight", (d,))}
        per = {k: [] for k in ("ln_attn", "w_qkv", "w_o", "ln_ff", "w_i", "w_o2")}
        for n in range(self.num_layers):
            att, ff = f"encoder.block.{n}.layer.0.", f"encoder.block.{n}.layer.1."
            per["ln_attn"].append(get(att + "layer_norm.weight", (d,)))
            per["w_qkv"].append(torch.cat([get(att + f"SelfAttention.{p}.weight", (inner, d)) for p in "qkv"], dim=0))
            per["w_o"].append(get(att + "SelfAttention.o.weight", (d, inner)))
            per["ln_ff"].append(get(ff + "layer_norm.weight", (d,)))
            per["w_i"].append(self._get_wi(get, ff))
            per["w_o2"].append(get(ff + "DenseReluDense.wo.weight", (d, self.d_ff)))
        staged.update({k: torch.stack(v) for k, v in per.items()})
        with torch.no_grad():   # nothing is written before every key and shape has passed
            for k, v in staged.items():
                getattr(self, k).copy_(v)

    @classmethod
    def from_pretrained(cls, name_or_path: str) -> "T5Encoder":
        """Config and weights from `transformers`' local files only; never downloads."""
        try:
            from transformers import AutoConfig, T5EncoderModel
            cfg = AutoConfig.from_pretrained(name_or_path, local_files_only=True)
            sd = T5EncoderModel.from_pretrained(name_or_path, local_files_only=True).state_dict()
        except Exception as e:
            raise NotImplementedError(_missing_weights(name_or_path)) from e
        cls._check_config(cfg)
        enc = cls(cfg.vocab_size, cfg.d_model, cfg.d_kv, cfg.d_ff, cfg.num_layers, cfg.num_heads,
                  cfg.relative_attention_num_buckets, getattr(cfg, "relative_attention_max_distance", 128),
                  cfg.layer_norm_epsilon, cfg.feed_forward_proj)
        enc.load_hf_state_dict(sd)
        return enc

    @classmethod
    def _check_config(cls, cfg) -> None:
        """Refuses a local config whose feed-forward this class does not compute (here: left to the constructor)."""

    # ---- forward
    def _bucket(self, m: int, device) -> Tensor:
        key = (m, str(device))
        if key not in self._buckets:
            self._buckets[key] = relative_position_buckets(m, self.num_buckets, self.max_distance).to(device)
        return self._buckets[key]

    def _workspace(self, T: int, like: Tensor) -> Optional[Tensor]:
        if T not in self._ws_bytes:
            inner, d, f = self.num_heads * self.d_kv, self.d_model, self.d_ff
            self._ws_bytes[T] = max([ops.t5_linear_ws_bytes(T, K, N) for K, N in ((d, 3 * inner), (inner, d), (f, d))]
                                    + [self._wi_ws_bytes(T)])
        n = self._ws_bytes[T]
        return torch.empty(n // 4, dtype=torch.float32, device=like.device) if n else None

    @torch.no_grad()
    def forward(self, input_ids: Tensor, attention_mask: Optional[Tensor] = None) -> Tensor:
        if input_ids.dim() != 2 or input_ids.dtype != torch.int64:
            raise TypeError("T5Encoder: input_ids is an int64 tensor [B, m]")
        B, m = input_ids.shape
        if not 1 <= m <= MAX_TOKENS:
            raise ValueError(f"T5Encoder: 1 to {MAX_TOKENS} tokens per row; got {m}")
        if input_ids.device != self.embed.device:
            raise RuntimeError(f"T5Encoder: input_ids on {input_ids.device}, weights on {self.embed.device}")
        mask = None
        if attention_mask is not None:
            if tuple(attention_mask.shape) != (B, m):
                raise ValueError("T5Encoder: attention_mask is [B, m]")
            mask = (attention_mask != 0).to(torch.uint8).contiguous()
        bucket = self._bucket(m, input_ids.device)
        T, d, inner, H = B * m, self.d_model, self.num_heads * self.d_kv, self.num_heads
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=input_ids.device)   # noqa: E731
        ws = self._workspace(T, self.embed)
        h = ops.t5_embed(input_ids.contiguous().view(-1), self.embed)
        a, qkv, o, f = new(T, d), new(T, 3 * inner), new(T, inner), new(T, self.d_ff)
        for n in range(self.num_layers):
            ops.t5_rmsnorm(h, self.ln_attn[n], self.eps, out=a)
            ops.t5_linear(a, self.w_qkv[n], out=qkv, ws=ws)
            ops.t5_attn(qkv.view(B, m, 3 * inner), self.rel_bias, bucket, mask, H, out=o.view(B, m, inner))
            ops.t5_linear(o, self.w_o[n], res=h, out=h, ws=ws)
            ops.t5_rmsnorm(h, self.ln_ff[n], self.eps, out=a)
            self._wi(n, a, f, ws)
            ops.t5_linear(f, self.w_o2[n], res=h, out=h, ws=ws)
        return ops.t5_rmsnorm(h, self.ln_final, self.eps).view(B, m, d)


class T5GatedEncoder(T5Encoder):
    """The T5 v1.1 / flan-T5 encoder: T5Encoder with the gated-GELU feed-forward h + wo(gelu_new(a wi_0^T) * (a wi_1^T)).
    Constructor arguments are T5Encoder's with feed_forward_proj="gated-gelu".  Both first-half weights of a stack live in
    ONE frozen parameter w_i [L, 2, d_ff, d] (0: wi_0, the gate, which goes through the activation; 1: wi_1, the up
    projection), whose two contiguous slices are the two weight pointers of ops.gated_linear: one GEMM stages the normed
    tokens once, forms both products and applies the gate, so a block launches what a ReLU block launches."""
    FEED_FORWARD = "gated-gelu"

    def __init__(self, vocab_size: int, d_model: int, d_kv: int, d_ff: int, num_layers: int, num_heads: int,
                 relative_attention_num_buckets: int = 32, relative_attention_max_distance: int = 128,
                 layer_norm_epsilon: float = 1e-6, feed_forward_proj: str = "gated-gelu"):
        super().__init__(vocab_size, d_model, d_kv, d_ff, num_layers, num_heads, relative_attention_num_buckets,
                         relative_attention_max_distance, layer_norm_epsilon, feed_forward_proj)

    @staticmethod
    def _refusal(feed_forward_proj: str) -> str:
        return (f"T5GatedEncoder: feed_forward_proj={feed_forward_proj!r} is not built; T5GatedEncoder covers 'gated-gelu' "
                "(gelu_new gate: T5 v1.1, flan-T5), text.T5Encoder covers 'relu'; gated-silu and ungated gelu are not built")

    def _init_wi(self, frozen) -> None:
        self.w_i = frozen(self.num_layers, 2, self.d_ff, self.d_model, std=self.d_model ** -0.5)

    def _get_wi(self, get, ff: str) -> Tensor:
        return torch.stack([get(ff + f"DenseReluDense.wi_{i}.weight", (self.d_ff, self.d_model)) for i in (0, 1)])

    def _wi_ws_bytes(self, T: int) -> int:
        return ops.gated_linear_ws_bytes(T, self.d_model, self.d_ff)

    def _wi(self, n: int, a: Tensor, f: Tensor, ws: Optional[Tensor]) -> None:
        ops.gated_linear(a, self.w_i[n, 0], self.w_i[n, 1], out=f, ws=ws)

    @classmethod
    def _check_config(cls, cfg) -> None:
        if not getattr(cfg, "is_gated_act", False) or getattr(cfg, "dense_act_fn", None) != "gelu_new":
            raise NotImplementedError(cls._refusal(getattr(cfg, "feed_forward_proj", None)))


def load_t5_encoder(name_or_path: str) -> T5Encoder:
    """The native encoder of a local T5 checkpoint (`transformers`' local files only; never downloads): a T5Encoder where
    its config says feed_forward_proj 'relu', a T5GatedEncoder where it says 'gated-gelu'."""
    try:
        from transformers import AutoConfig
        cfg = AutoConfig.from_pretrained(name_or_path, local_files_only=True)
    except Exception as e:
        raise NotImplementedError(_missing_weights(name_or_path)) from e
    for cls in (T5Encoder, T5GatedEncoder):
        if getattr(cfg, "feed_forward_proj", None) == cls.FEED_FORWARD:
            return cls.from_pretrained(name_or_path)
    raise NotImplementedError(T5GatedEncoder._refusal(getattr(cfg, "feed_forward_proj", None)))


class T5Embedder(nn.Module):
    """List[str] -> [B, max_length, d_model]: the `text_embedder=` of UNetV0(use_text_conditioning=True) on the native
    encoder.  `tokenizer(texts, truncation=True, max_length=..., padding="max_length", return_tensors="pt")` returns
    `input_ids` and `attention_mask` -- a HuggingFace tokenizer, or any callable of that shape."""

    def __init__(self, encoder: T5Encoder, tokenizer, max_length: int = 64):   # (a T5GatedEncoder is a T5Encoder)
        super().__init__()
        self.encoder, self.tokenizer, self.max_length = encoder, tokenizer, max_length

    @torch.no_grad()
    def forward(self, texts: List[str]) -> Tensor:
        enc = self.tokenizer(texts, truncation=True, max_length=self.max_length, padding="max_length", return_tensors="pt")
        ids, mask = enc["input_ids"], enc["attention_mask"]
        # on the host, before the copy: the kernel would give a zero row where torch's embedding raises
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.encoder.vocab_size):
            raise ValueError(f"T5Embedder: token id outside [0, {self.encoder.vocab_size}) "
                             f"(min {int(ids.min())}, max {int(ids.max())})")
        device = self.encoder.embed.device
        return self.encoder(ids.to(device=device, dtype=torch.int64), mask.to(device))
