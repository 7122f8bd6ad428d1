"""The entry points of include/adp_lt.h with misaligned operands and guard bands (tests/placement.py), as
tests/test_ar_placement.py does for include/adp_ar.h: every operand of a direct call through `_C.lib()` is placed by the test
at the zero / all1 / mixed / single1 / single2 placements.  A placed call returns ADP_OK, agrees with the float64 reference
within the kernels' own bound (1e-4, tests/test_lt.py) and leaves every guard, offset gap and input payload bit-identical.
Two geometries: the one on the 16-byte paths (which a misplaced pointer must leave) and the odd one."""
import os
import re

import pytest
import torch

from audio_diffusion_pytorch_amd import _C, ops
from conftest import rel_err
from placement import Arena
from test_lt import TOL, case

GEOMS = ["vec16", "odd"]   # every 16-byte access available (which a misplaced pointer must leave); odd sizes
OUTPUT_ROLES = ("out", "inout")


def p(t):
    return None if t is None else _C.ptr(t, t.dtype)


class Placer:
    """Operands in declaration order; `plan(i, name, role)` gives operand i its offset in elements."""

    def __init__(self, dev, plan):
        self.arena, self.plan, self.operands = Arena(dev), plan, []

    def _off(self, name, role):
        self.operands.append((name, role))
        return self.plan(len(self.operands) - 1, name, role)

    def inp(self, name, data):
        return self.arena.input(name, data, self._off(name, "in"))

    def out(self, name, shape):
        return self.arena.output(name, shape, self._off(name, "out"))

    def ws(self, name, numel):
        return self.arena.workspace(name, numel, self._off(name, "ws"))


def _conv(P, d, xk, wk, mode, refk):
    x, w = P.inp("x", d[xk]), P.inp("w", d[wk])
    B, C, T = d[xk].shape
    O, K = d[wk].shape[0], d[wk].shape[2]
    y = P.out("y", d[refk].shape)
    code = _C.lib().adp_lt_conv(p(x), p(w), B, C, T, O, K, d["s"], d["p"], mode, p(y), _C.stream())
    return code, [("y", y, d[refk])]


def _convt(P, d, xk, wk, mode, refk):
    x, w = P.inp("x", d[xk]), P.inp("w", d[wk])
    B, C, L = d[xk].shape
    O, K = d[wk].shape[1], d[wk].shape[2]
    out = P.out("out", d[refk].shape)
    code = _C.lib().adp_lt_convt(p(x), p(w), B, C, L, O, K, d["s"], d["p"], mode, d["T"], p(out), _C.stream())
    return code, [("out", out, d[refk])]


def _wgrad(P, d, uk, vk, mode, refk):
    u, v = P.inp("u", d[uk]), P.inp("v", d[vk])
    B, A, L = d[uk].shape
    Bc, T = d[vk].shape[1], d[vk].shape[2]
    K = d["W"]
    dw = P.out("dw", d[refk].shape)
    nbytes = _C.lib().adp_lt_wgrad_ws_bytes(B, A, Bc, L, K)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = P.ws("ws", nbytes // 4)
    code = _C.lib().adp_lt_wgrad(p(u), p(v), B, A, Bc, L, T, K, d["s"], d["p"], mode, p(dw), p(ws), _C.stream())
    return code, [("dw", dw, d[refk])]


# case -> (placing function, its arguments, the entry point it places); with QUERIES they must cover _C.LT_SIGNATURES
CASES = {
    "encode_fwd": (_conv, ("x", "we", ops.LT_REFLECT, "y"), "adp_lt_conv"),
    "decode_dgrad": (_conv, ("go", "wd", ops.LT_ZERO, "dyin"), "adp_lt_conv"),
    "decode_fwd": (_convt, ("yin", "wd", ops.LT_PLAIN, "out"), "adp_lt_convt"),
    "encode_dgrad": (_convt, ("gy", "we", ops.LT_FOLD, "dx"), "adp_lt_convt"),
    "encode_wgrad": (_wgrad, ("gy", "x", ops.LT_REFLECT, "dwe"), "adp_lt_wgrad"),
    "decode_wgrad": (_wgrad, ("yin", "go", ops.LT_ZERO, "dwd"), "adp_lt_wgrad"),
}
QUERIES = {"adp_lt_conv_out_len": "length query, integers only", "adp_lt_convt_out_len": "length query, integers only",
           "adp_lt_wgrad_ws_bytes": "size query, integers only"}
PLANS = {"zero": lambda i, n, r: 0, "all1": lambda i, n, r: 1, "mixed": lambda i, n, r: 1 + i % 3}


def place_and_check(dev, name, geom, plan, what):
    fn, args, entry = CASES[name]
    P = Placer(dev, plan)
    code, close = fn(P, case(geom), *args)
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


@pytest.mark.parametrize("kind", ["zero", "all1", "mixed"])
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("name", list(CASES))
def test_whole_call_placements(dev, name, geom, kind):
    place_and_check(dev, name, geom, PLANS[kind], kind)


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("name", list(CASES))
def test_single_operand_placements(dev, name, geom):
    """single1: each pointer operand alone at offset 1; single2: each output alone at offset 2 (the 8-byte phase)."""
    base = place_and_check(dev, name, geom, PLANS["zero"], "zero")
    for operand, role in base.operands:
        place_and_check(dev, name, geom, lambda i, n, r, t=operand: 1 if n == t else 0, f"{operand}@1")
        if role in OUTPUT_ROLES:
            place_and_check(dev, name, geom, lambda i, n, r, t=operand: 2 if n == t else 0, f"{operand}@2")


def test_every_lt_entry_point_is_placed():
    assert {entry for _, _, entry in CASES.values()} | set(QUERIES) == set(_C.LT_SIGNATURES)
    assert not set(_C.LT_SIGNATURES) & set(_C.SIGNATURES)
    assert not set(_C.LT_SIGNATURES) & set(_C.AR_SIGNATURES)


def test_header_table_and_libraries_agree(emul):
    """include/adp_lt.h <-> _C.LT_SIGNATURES <-> what the built libraries export."""
    import ctypes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "adp_lt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)   # (the comments name other functions)
    declared = set(re.findall(r"\b(adp_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_C.LT_SIGNATURES), declared ^ set(_C.LT_SIGNATURES)
    for name in declared:
        assert hasattr(_C.lib(), name), name            # the emulated build of the same sources
    assert os.path.exists(_C.LIB_PATH), "libadp_hip.so is not built (run __graft_entry__.build())"
    hip_lib = ctypes.CDLL(_C.LIB_PATH)
    for name in declared:
        assert hasattr(hip_lib, name), name
    source = open(os.path.join(root, "audio_diffusion_pytorch_amd", "csrc", "lt.hip")).read()
    assert '#include "adp_lt.h"' in source
