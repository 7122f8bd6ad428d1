"""The entry points of include/adp_gated.h with misaligned operands and guard bands (tests/placement.py), as
tests/test_t5_placement.py does for include/adp_t5.h: every operand of a direct call through `_C.lib()` is placed by the test
at the zero / all1 / mixed / single1 / single2 placements (offsets in floats).  A placed call returns ADP_OK, agrees with the
float64 reference within the kernels' own bound (1e-4, tests/test_t5.py) and leaves every guard, offset gap and input payload
bit-identical.  Three geometries: one whose rows are whole 16-byte groups, an odd one, and an odd one whose k sum is long
enough to go through the workspace."""
import functools

import torch

from audio_diffusion_pytorch_amd import _C
from placement import close, p, single_operand_tests, whole_call_tests
from test_t5 import TOL

import t5_gated_ref

# T tokens, K inputs, F outputs of the gated GEMM
GEOMS = {"vec16": dict(T=16, K=16, F=8), "odd": dict(T=21, K=13, F=5), "split": dict(T=21, K=259, F=5)}


@functools.lru_cache(maxsize=None)
def case(geom):
    """Inputs and the float64 reference of one geometry (CPU tensors, computed once, never modified)."""
    c = dict(GEOMS[geom])
    T, K, F = c["T"], c["K"], c["F"]
    g = torch.Generator().manual_seed(17 * K + T)
    x = torch.randn(T, K, generator=g)
    wg, wu = 2 * torch.randn(F, K, generator=g) / K ** 0.5, torch.randn(F, K, generator=g) / K ** 0.5
    c.update(x=x, wg=wg, wu=wu, y=t5_gated_ref.gelu_new(x.double() @ wg.double().T) * (x.double() @ wu.double().T))
    return c


def _gated(P, d):
    x, wg, wu = P.inp("x", d["x"]), P.inp("w_gate", d["wg"]), P.inp("w_up", d["wu"])
    y = P.out("y", d["y"].shape)
    nbytes = _C.lib().adp_gated_linear_ws_bytes(d["T"], d["K"], d["F"])
    assert nbytes >= 0 and nbytes % 4 == 0 and (nbytes > 0) == (d["K"] > 128)
    ws = P.ws_numel("ws", nbytes // 4) if nbytes else None
    code = _C.lib().adp_gated_linear(p(x), p(wg), p(wu), d["T"], d["K"], d["F"], 1, p(y), p(ws), _C.stream())
    return code, [close("y", y, d["y"], TOL)]


# case -> (placing function, the entry point it places); with QUERIES they must cover _C.ABI["adp_gated.h"]
CASES = {"gated_linear": (_gated, "adp_gated_linear")}
QUERIES = {"adp_gated_linear_ws_bytes": "size query, integers only"}


ALL = [(n, g) for n in CASES for g in GEOMS]
test_whole_call_placements = whole_call_tests(CASES, ALL, case)
test_single_operand_placements = single_operand_tests(CASES, ALL, case)


def test_every_gated_entry_point_is_placed():
    assert {entry for _, entry in CASES.values()} | set(QUERIES) == set(_C.ABI["adp_gated.h"])
