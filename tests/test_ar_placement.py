"""The entry points of include/adp_ar.h with misaligned operands and guard bands (tests/placement.py), as
tests/test_operand_placement.py does for include/adp.h: every operand of a direct call through `_C.lib()` is placed by the
test at the zero / all1 / mixed / single1 / single2 placements.  A placed call returns ADP_OK, agrees with the fp64 formula
within the kernels' own bound (1e-6, tests/test_ar.py) and leaves every guard, offset gap and input payload bit-identical."""
import os
import re

import pytest
import torch

from audio_diffusion_pytorch_amd import _C
from conftest import rel_err
from placement import Arena
from test_ar import KERNEL_TOL, case_data, noise_ref, per_position, step_ref

# (B, C, T, N): l a multiple of 4 (the 16-byte paths where the pointers allow them), l = 7, and one split
SHAPES = [(2, 3, 2048, 8), (3, 2, 35, 5), (1, 2, 300, 1)]
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

    def inout(self, name, data):
        return self.arena.inout(name, data, self._off(name, "inout"))

    def out(self, name, shape):
        return self.arena.output(name, shape, self._off(name, "out"))


def arv_noise(P, B, C, T, N):
    x, v, sigma, _ = case_data(B, C, T, N, seed=3)
    xd, vd, sd = P.inp("x", x), P.inp("noise", v), P.inp("sigma", sigma)
    xn, vt, plane = P.out("x_noisy", (B, C, T)), P.out("v_target", (B, C, T)), P.out("sigma_plane", (B, T))
    code = _C.lib().adp_arv_noise(p(xd), p(vd), p(sd), B, C, T, N, p(xn), p(vt), p(plane), _C.stream())
    xn_ref, vt_ref, plane_ref = noise_ref(x, v, sigma)
    return code, [("x_noisy", xn, xn_ref), ("v_target", vt, vt_ref)], [("sigma_plane", plane, plane_ref[:, 0].float())]


def arv_step(P, B, C, T, N):
    x, v, _, coef = case_data(B, C, T, N, seed=4)
    xd, vd, cd = P.inp("x", x), P.inp("v", v), P.inp("coef", coef)
    xo, plane = P.out("x_out", (B, C, T)), P.out("sigma_plane_out", (B, T))
    code = _C.lib().adp_arv_step(p(xd), p(vd), p(cd), B, C, T, N, p(xo), p(plane), _C.stream())
    out_ref, next_ref = step_ref(x, v, coef)
    l = T // N
    return code, [("x_out", xo, out_ref)], [("sigma_plane_out", plane, next_ref.float().expand(B, T)),
                                            ("context split", xo[..., :l], x[..., :l])]


def arv_step_in_place(P, B, C, T, N):
    """x_out = x and no plane: the form the captured sampler step's first operand takes."""
    x, v, _, coef = case_data(B, C, T, N, seed=5)
    xd, vd, cd = P.inout("x", x), P.inp("v", v), P.inp("coef", coef)
    code = _C.lib().adp_arv_step(p(xd), p(vd), p(cd), B, C, T, N, p(xd), None, _C.stream())
    l = T // N
    return code, [("x", xd, step_ref(x, v, coef)[0])], [("context split", xd[..., :l], x[..., :l])]


def arv_plane(P, B, C, T, N):
    sigma = case_data(B, C, T, N, seed=6)[2][0].contiguous()
    sd, plane = P.inp("sigma", sigma), P.out("sigma_plane", (B, T))
    code = _C.lib().adp_arv_plane(p(sd), B, T, N, p(plane), _C.stream())
    return code, [], [("sigma_plane", plane, per_position(sigma, T).expand(B, T))]


# case -> the entry point it places; together they must cover _C.AR_SIGNATURES
CASES = {"arv_noise": (arv_noise, "adp_arv_noise"), "arv_step": (arv_step, "adp_arv_step"),
         "arv_step_in_place": (arv_step_in_place, "adp_arv_step"), "arv_plane": (arv_plane, "adp_arv_plane")}
PLANS = {"zero": lambda i, n, r: 0, "all1": lambda i, n, r: 1, "mixed": lambda i, n, r: 1 + i % 3}


def place_and_check(dev, case, shape, plan, what):
    fn, entry = CASES[case]
    P = Placer(dev, plan)
    code, close, exact = fn(P, *shape)
    assert code == 0, f"{entry} {shape} [{what}] returned {code} ({_C.ERRORS.get(code, '?')})"
    problems = []
    for label, got, want in close:
        err = rel_err(got, want)
        print(f"{entry} {shape} [{what}] {label}: rel err {err:.3e} (bound {KERNEL_TOL:.1e})")
        if not err < KERNEL_TOL:
            problems.append(f"{label}: rel err {err:.3e} >= {KERNEL_TOL:.1e}")
    for label, got, want in exact:
        if not torch.equal(got.cpu(), want.cpu()):
            problems.append(f"{label}: not bit-identical")
    P.arena.verify()   # raises PlacementError naming the operand and the span
    assert not problems, f"{entry} {shape}, placement {what}:\n" + "\n".join(problems)
    return P


@pytest.mark.parametrize("kind", ["zero", "all1", "mixed"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("case", list(CASES))
def test_whole_call_placements(dev, case, shape, kind):
    place_and_check(dev, case, shape, PLANS[kind], kind)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("case", list(CASES))
def test_single_operand_placements(dev, case, shape):
    """single1: each pointer operand alone at offset 1; single2: each output alone at offset 2 (the 8-byte phase)."""
    base = place_and_check(dev, case, shape, PLANS["zero"], "zero")
    for name, role in base.operands:
        place_and_check(dev, case, shape, lambda i, n, r, t=name: 1 if n == t else 0, f"{name}@1")
        if role in OUTPUT_ROLES:
            place_and_check(dev, case, shape, lambda i, n, r, t=name: 2 if n == t else 0, f"{name}@2")


def test_every_ar_entry_point_is_placed():
    assert {entry for _, entry in CASES.values()} == set(_C.AR_SIGNATURES)
    assert not set(_C.AR_SIGNATURES) & set(_C.SIGNATURES)


def test_header_table_and_libraries_agree(emul):
    """include/adp_ar.h <-> _C.AR_SIGNATURES <-> what the built libraries export."""
    import ctypes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "adp_ar.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)   # (the comments name adp.h's functions)
    declared = set(re.findall(r"\b(adp_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_C.AR_SIGNATURES), declared ^ set(_C.AR_SIGNATURES)
    for name in declared:
        assert hasattr(_C.lib(), name), name            # the emulated build of the same sources
    assert os.path.exists(_C.LIB_PATH), "libadp_hip.so is not built (run __graft_entry__.build())"
    hip_lib = ctypes.CDLL(_C.LIB_PATH)
    for name in declared:
        assert hasattr(hip_lib, name), name
    source = open(os.path.join(root, "audio_diffusion_pytorch_amd", "csrc", "elementwise.hip")).read()
    assert '#include "adp_ar.h"' in source
