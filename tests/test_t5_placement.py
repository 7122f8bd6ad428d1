"""The entry points of include/adp_t5.h with misaligned operands and guard bands (tests/placement.py), as
tests/test_encoder_placement.py does for include/adp_enc.h: every operand of a direct call through `_C.lib()` is placed by the
test at the zero / all1 / mixed / single1 / single2 placements (offsets in elements of the operand's own type: int64 ids,
int32 buckets, uint8 mask bytes).  A placed call returns ADP_OK, agrees with the float64 reference within the kernels' own
bound (1e-4, tests/test_t5.py) and leaves every guard, offset gap and input payload bit-identical.  Two geometries: one whose
rows are whole 16-byte groups and an odd one."""
import functools

import torch

from audio_diffusion_pytorch_amd import _C
from audio_diffusion_pytorch_amd.text import relative_position_buckets
from placement import close, p, single_operand_tests, whole_call_tests
from test_t5 import TOL, prefix_mask

import t5_ref

# T tokens = B x m, d model features, N outputs of the GEMM, V table rows, H heads of dk, nb buckets; "split": a k sum long
# enough to go through the workspace
GEOMS = {"vec16": dict(B=2, m=8, d=16, N=8, V=12, H=2, dk=8, nb=8, K=16),
         "odd": dict(B=3, m=7, d=13, N=5, V=11, H=3, dk=8, nb=6, K=13),
         "split": dict(B=3, m=7, d=13, N=5, V=11, H=3, dk=8, nb=6, K=259)}


@functools.lru_cache(maxsize=None)
def case(geom):
    """Inputs and float64 references of one geometry (CPU tensors, computed once, never modified)."""
    c = dict(GEOMS[geom])
    B, m, d, N, V, H, dk, nb, K = (c[k] for k in ("B", "m", "d", "N", "V", "H", "dk", "nb", "K"))
    T = B * m
    g = torch.Generator().manual_seed(17 * d + m)
    ids = torch.randint(0, V, (T,), generator=g)
    ids[1], ids[2] = -1, V
    table = torch.randn(V, d, generator=g)
    emb = table[ids.clamp(0, V - 1)].double()
    emb[1], emb[2] = 0, 0
    x, gain = torch.randn(T, d, generator=g), 1 + 0.2 * torch.randn(d, generator=g)
    xk, w, res = torch.randn(T, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(T, N, generator=g)
    qkv = torch.randn(B, m, 3 * H * dk, generator=g)
    rel = torch.randn(nb, H, generator=g) * 4
    bucket = relative_position_buckets(m, nb, 20)
    mask = prefix_mask(B, m).to(torch.uint8)
    pos = torch.arange(m)
    bias = rel[bucket.long()[(pos[None, :] - pos[:, None]) + m - 1]].permute(2, 0, 1)
    q, k, v = (t.reshape(B, m, H, dk).transpose(1, 2) for t in qkv.split(H * dk, dim=-1))
    attn = t5_ref.attention(q, k, v, bias, mask).transpose(1, 2).reshape(B, m, H * dk)
    c.update(T=T, ids=ids, table=table, emb=emb, x=x, gain=gain, norm=t5_ref.rmsnorm(x.double(), gain.double(), 1e-6), xk=xk, w=w,
             res=res, lin=res.double() + torch.relu(xk.double() @ w.double().T), qkv=qkv, rel=rel, bucket=bucket, mask=mask,
             attn=attn)
    return c


def _embed(P, d):
    ids, table = P.inp("ids", d["ids"]), P.inp("table", d["table"])
    out = P.out("out", d["emb"].shape)
    code = _C.lib().adp_t5_embed(p(ids), p(table), d["T"], d["V"], d["d"], p(out), _C.stream())
    return code, [close("out", out, d["emb"], TOL)]


def _rmsnorm(P, d):
    x, g = P.inp("x", d["x"]), P.inp("g", d["gain"])
    y = P.out("y", d["norm"].shape)
    code = _C.lib().adp_t5_rmsnorm(p(x), p(g), d["T"], d["d"], 1e-6, p(y), _C.stream())
    return code, [close("y", y, d["norm"], TOL)]


def _linear(P, d):
    x, w, res = P.inp("x", d["xk"]), P.inp("w", d["w"]), P.inp("res", d["res"])
    y = P.out("y", d["lin"].shape)
    nbytes = _C.lib().adp_t5_linear_ws_bytes(d["T"], d["K"], d["N"])
    assert nbytes >= 0 and nbytes % 4 == 0 and (nbytes > 0) == (d["K"] > 128)
    ws = P.ws_numel("ws", nbytes // 4) if nbytes else None
    code = _C.lib().adp_t5_linear(p(x), p(w), p(res), d["T"], d["K"], d["N"], 1, p(y), p(ws), _C.stream())
    return code, [close("y", y, d["lin"], TOL)]


def _attn(P, d):
    qkv, rel = P.inp("qkv", d["qkv"]), P.inp("rel_table", d["rel"])
    bucket, mask = P.inp("bucket", d["bucket"]), P.inp("mask", d["mask"])
    out = P.out("out", d["attn"].shape)
    code = _C.lib().adp_t5_attn(p(qkv), p(rel), p(bucket), p(mask), d["B"], d["H"], d["dk"], d["m"], d["nb"], p(out),
                                _C.stream())
    return code, [close("out", out, d["attn"], TOL)]


# case -> (placing function, the entry point it places); with QUERIES they must cover _C.ABI["adp_t5.h"]
CASES = {
    "embed": (_embed, "adp_t5_embed"),
    "rmsnorm": (_rmsnorm, "adp_t5_rmsnorm"),
    "linear": (_linear, "adp_t5_linear"),
    "attn": (_attn, "adp_t5_attn"),
}
QUERIES = {"adp_t5_linear_ws_bytes": "size query, integers only"}


def _geoms(name):
    return [g for g in GEOMS if g != "split" or name == "linear"]


ALL = [(n, g) for n in CASES for g in _geoms(n)]
test_whole_call_placements = whole_call_tests(CASES, ALL, case)
test_single_operand_placements = single_operand_tests(CASES, ALL, case)


def test_every_t5_entry_point_is_placed():
    assert {entry for _, entry in CASES.values()} | set(QUERIES) == set(_C.ABI["adp_t5.h"])
