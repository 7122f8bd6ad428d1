"""The entry points of include/adp_gated.h with misaligned operands and guard bands (tests/placement.py), as
tests/test_t5_placement.py does for include/adp_t5.h: every operand of a direct call through `_C.lib()` is placed by the test
at the zero / all1 / mixed / single1 / single2 placements (offsets in floats).  A placed call returns ADP_OK, agrees with the
float64 reference within the kernels' own bound (1e-4, tests/test_t5.py) and leaves every guard, offset gap and input payload
bit-identical.  Three geometries: one whose rows are whole 16-byte groups, an odd one, and an odd one whose k sum is long
enough to go through the workspace."""
import functools
import os
import re

import pytest
import torch

from audio_diffusion_pytorch_amd import _C
from conftest import rel_err
from test_encoder_placement import PLANS, Placer, p
from test_t5 import TOL

import t5_gated_ref

OUTPUT_ROLES = ("out", "inout")
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
    ws = P.ws("ws", nbytes // 4) if nbytes else None
    code = _C.lib().adp_gated_linear(p(x), p(wg), p(wu), d["T"], d["K"], d["F"], 1, p(y), p(ws), _C.stream())
    return code, [("y", y, d["y"])]


# case -> (placing function, the entry point it places); with QUERIES they must cover _C.GATED_SIGNATURES
CASES = {"gated_linear": (_gated, "adp_gated_linear")}
QUERIES = {"adp_gated_linear_ws_bytes": "size query, integers only"}


def place_and_check(dev, name, geom, plan, what):
    fn, entry = CASES[name]
    P = Placer(dev, plan)
    code, close = fn(P, case(geom))
    assert code == 0, f"{entry} {geom} [{what}] returned {code} ({_C.ERRORS.get(code, '?')})"
    problems = []
    for label, got, want in close:
        err = rel_err(got, want)
        print(f"{entry} {name} {geom} [{what}] {label}: rel err {err:.3e} (bound {TOL:.0e})")
        if not err < TOL:
            problems.append(f"{label}: rel err {err:.3e} >= {TOL:.0e}")
    P.arena.verify()   # raises PlacementError naming the operand and the span
    assert not problems, f"{entry} {geom}, placement {what}:\n" + "\n".join(problems)
    return P


ALL = [(n, g) for n in CASES for g in GEOMS]


@pytest.mark.parametrize("kind", ["zero", "all1", "mixed"])
@pytest.mark.parametrize("name,geom", ALL)
def test_whole_call_placements(dev, name, geom, kind):
    place_and_check(dev, name, geom, PLANS[kind], kind)


@pytest.mark.parametrize("name,geom", ALL)
def test_single_operand_placements(dev, name, geom):
    """single1: each pointer operand alone at offset 1; single2: each output alone at offset 2 (the 8-byte phase)."""
    base = place_and_check(dev, name, geom, PLANS["zero"], "zero")
    for operand, role in base.operands:
        place_and_check(dev, name, geom, lambda i, n, r, t=operand: 1 if n == t else 0, f"{operand}@1")
        if role in OUTPUT_ROLES:
            place_and_check(dev, name, geom, lambda i, n, r, t=operand: 2 if n == t else 0, f"{operand}@2")


def test_every_gated_entry_point_is_placed():
    assert {entry for _, entry in CASES.values()} | set(QUERIES) == set(_C.GATED_SIGNATURES)
    for other in (_C.SIGNATURES, _C.AR_SIGNATURES, _C.LT_SIGNATURES, _C.ENC_SIGNATURES, _C.T5_SIGNATURES, _C.RNG_SIGNATURES,
                  _C.CLIP_SIGNATURES):
        assert not set(_C.GATED_SIGNATURES) & set(other)


def test_header_table_and_libraries_agree(emul):
    """include/adp_gated.h <-> _C.GATED_SIGNATURES <-> what the built libraries export."""
    import ctypes
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "adp_gated.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)   # (the comments name other functions)
    declared = set(re.findall(r"\b(adp_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_C.GATED_SIGNATURES), declared ^ set(_C.GATED_SIGNATURES)
    for name in declared:
        assert hasattr(_C.lib(), name), name            # the emulated build of the same sources
    assert os.path.exists(_C.LIB_PATH), "libadp_hip.so is not built (run __graft_entry__.build())"
    hip_lib = ctypes.CDLL(_C.LIB_PATH)
    for name in declared:
        assert hasattr(hip_lib, name), name
    # the library's dynamic symbol table holds exactly the adp_gated_* names the header declares
    syms = subprocess.run(["nm", "-D", "--defined-only", _C.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if ln.split() and ln.split()[-1].startswith("adp_gated_")}
    assert exported == declared, exported ^ declared
    source = open(os.path.join(root, "audio_diffusion_pytorch_amd", "csrc", "gated.hip")).read()
    assert '#include "adp_gated.h"' in source
