"""The entry points of include/adp_enc.h with misaligned operands and guard bands (tests/placement.py), as
tests/test_lt_placement.py does for include/adp_lt.h: every operand of a direct call through `_C.lib()` is placed by the test
at the zero / all1 / mixed / single1 / single2 placements.  A placed call returns ADP_OK, agrees with the float64 reference
within the kernels' own bound (1e-4, tests/test_encoder.py) and leaves every guard, offset gap and input payload bit-identical.
Two geometries: the one on the 16-byte paths (which a misplaced pointer must leave) and the odd one."""
import os
import re

import pytest

from audio_diffusion_pytorch_amd import _C
from conftest import rel_err
from placement import Arena
from test_encoder import GEOMS, TOL, case

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


def _dims(d):
    return d["B"], d["R"], d["M"], d["L"], d["f"]


def _fwd(P, d):
    x, w, bias = P.inp("x", d["x"]), P.inp("w", d["w"]), P.inp("bias", d["bias"])
    y = P.out("y", d["y"].shape)
    code = _C.lib().adp_enc_down_fwd(p(x), p(w), p(bias), *_dims(d), p(y), _C.stream())
    return code, [("y", y, d["y"])]


def _dgrad(P, d):
    dy, w = P.inp("dy", d["dy"]), P.inp("w", d["w"])
    dx = P.out("dx", d["dx"].shape)
    code = _C.lib().adp_enc_down_dgrad(p(dy), p(w), *_dims(d), p(dx), _C.stream())
    return code, [("dx", dx, d["dx"])]


def _wgrad(P, d):
    x, dy = P.inp("x", d["x"]), P.inp("dy", d["dy"])
    dw, dbias = P.out("dw", d["dw"].shape), P.out("dbias", d["dbias"].shape)
    nbytes = _C.lib().adp_enc_down_wgrad_ws_bytes(*_dims(d))
    assert nbytes > 0 and nbytes % 4 == 0
    ws = P.ws("ws", nbytes // 4)
    code = _C.lib().adp_enc_down_wgrad(p(x), p(dy), *_dims(d), p(dw), p(dbias), p(ws), _C.stream())
    return code, [("dw", dw, d["dw"]), ("dbias", dbias, d["dbias"])]


def _tanh_fwd(P, d):
    h = P.inp("h", d["h"])
    z = P.out("z", d["z"].shape)
    code = _C.lib().adp_enc_tanh_fwd(p(h), h.numel(), p(z), _C.stream())
    return code, [("z", z, d["z"])]


def _tanh_bwd(P, d):
    z, dz = P.inp("z", d["zf"]), P.inp("dz", d["dz"])
    dh = P.out("dh", d["dh"].shape)
    code = _C.lib().adp_enc_tanh_bwd(p(z), p(dz), z.numel(), p(dh), _C.stream())
    return code, [("dh", dh, d["dh"])]


# case -> (placing function, the entry point it places); with QUERIES they must cover _C.ENC_SIGNATURES
CASES = {
    "down_fwd": (_fwd, "adp_enc_down_fwd"),
    "down_dgrad": (_dgrad, "adp_enc_down_dgrad"),
    "down_wgrad": (_wgrad, "adp_enc_down_wgrad"),
    "tanh_fwd": (_tanh_fwd, "adp_enc_tanh_fwd"),
    "tanh_bwd": (_tanh_bwd, "adp_enc_tanh_bwd"),
}
QUERIES = {"adp_enc_down_out_len": "length query, integers only", "adp_enc_down_wgrad_ws_bytes": "size query, integers only"}
PLANS = {"zero": lambda i, n, r: 0, "all1": lambda i, n, r: 1, "mixed": lambda i, n, r: 1 + i % 3}


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


@pytest.mark.parametrize("kind", ["zero", "all1", "mixed"])
@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("name", list(CASES))
def test_whole_call_placements(dev, name, geom, kind):
    place_and_check(dev, name, geom, PLANS[kind], kind)


@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("name", list(CASES))
def test_single_operand_placements(dev, name, geom):
    """single1: each pointer operand alone at offset 1; single2: each output alone at offset 2 (the 8-byte phase)."""
    base = place_and_check(dev, name, geom, PLANS["zero"], "zero")
    for operand, role in base.operands:
        place_and_check(dev, name, geom, lambda i, n, r, t=operand: 1 if n == t else 0, f"{operand}@1")
        if role in OUTPUT_ROLES:
            place_and_check(dev, name, geom, lambda i, n, r, t=operand: 2 if n == t else 0, f"{operand}@2")


def test_every_enc_entry_point_is_placed():
    assert {entry for _, entry in CASES.values()} | set(QUERIES) == set(_C.ENC_SIGNATURES)
    for other in (_C.SIGNATURES, _C.AR_SIGNATURES, _C.LT_SIGNATURES):
        assert not set(_C.ENC_SIGNATURES) & set(other)


def test_header_table_and_libraries_agree(emul):
    """include/adp_enc.h <-> _C.ENC_SIGNATURES <-> what the built libraries export."""
    import ctypes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "adp_enc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)   # (the comments name other functions)
    declared = set(re.findall(r"\b(adp_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_C.ENC_SIGNATURES), declared ^ set(_C.ENC_SIGNATURES)
    for name in declared:
        assert hasattr(_C.lib(), name), name            # the emulated build of the same sources
    assert os.path.exists(_C.LIB_PATH), "libadp_hip.so is not built (run __graft_entry__.build())"
    hip_lib = ctypes.CDLL(_C.LIB_PATH)
    for name in declared:
        assert hasattr(hip_lib, name), name
    source = open(os.path.join(root, "audio_diffusion_pytorch_amd", "csrc", "encoder.hip")).read()
    assert '#include "adp_enc.h"' in source
