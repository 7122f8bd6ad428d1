"""The entry points of include/adp_rng.h with misaligned operands and guard bands (tests/placement.py), as
tests/test_encoder_placement.py does for include/adp_enc.h: every operand of a direct call through `_C.lib()` is placed by the
test at the zero / all1 / mixed / single1 / single2 placements.  A placed call returns ADP_OK, gives the values of the
restatement (tests/test_rng.py: words exactly, normals within 1e-5 absolute, the fused step within 1e-6 in the max norm) and
leaves every guard, offset gap and input payload bit-identical.  Two lengths: one on the 16-byte paths (which a misplaced
pointer must leave) and an odd one with a partial last group."""
import os
import re

import pytest
import torch

from audio_diffusion_pytorch_amd import _C, ops
from conftest import rel_err
from placement import Arena
from test_encoder_placement import OUTPUT_ROLES, PLANS, Placer, p
from test_rng import NORMAL_TOL, STEP_TOL, reference, step_ref

SEED, DRAW = 0x299F31D0A4093822, 9
LENGTHS = {"vec": 2048, "odd": 1001}


def _row(P):
    return P.arena.input("rng4", ops.rng_rows(SEED, [DRAW])[0], P._off("rng4", "in"))


def _bits(P, n):
    r = _row(P)
    out = P.arena.output("out", (n,), P._off("out", "out"), dtype=torch.int32)
    code = _C.lib().adp_philox_bits(p(r), n, p(out), _C.stream())
    want = reference(SEED, DRAW, n)[0][:n]
    return code, lambda: [("words", float(((out.cpu().to(torch.int64) & 0xFFFFFFFF) != want).sum()), 1.0)]


def _randn(P, n):
    r = _row(P)
    out = P.out("out", (n,))
    code = _C.lib().adp_randn(p(r), n, p(out), _C.stream())
    return code, lambda: [("normals", (out.cpu().double() - reference(SEED, DRAW, n)[1]).abs().max().item(), NORMAL_TOL)]


def _step(P, n):
    g = torch.Generator().manual_seed(n)
    x, v, src = [torch.randn(n, generator=g) for _ in range(3)]
    mask = (torch.rand(n, generator=g) > 0.5).to(torch.uint8)
    ab4 = torch.tensor([0.3, 0.9, 0.5, 0.8])
    xd, vd, sd, md, ad = P.inp("x", x), P.inp("v", v), P.inp("source", src), P.inp("mask", mask), P.inp("ab4", ab4)
    r = _row(P)
    out = P.out("x_out", (n,))
    code = _C.lib().adp_v_inpaint_step_rng(p(xd), p(vd), p(sd), p(md), p(ad), p(r), n, p(out), _C.stream())
    want = step_ref(x, v, src, reference(SEED, DRAW, n)[1], mask, ab4)
    return code, lambda: [("x_out", rel_err(out, want), STEP_TOL)]


CASES = {"philox_bits": (_bits, "adp_philox_bits"), "randn": (_randn, "adp_randn"),
         "v_inpaint_step_rng": (_step, "adp_v_inpaint_step_rng")}


def place_and_check(dev, name, length, plan, what):
    fn, entry = CASES[name]
    P = Placer(dev, plan)
    code, figures = fn(P, LENGTHS[length])
    assert code == 0, f"{entry} {length} [{what}] returned {code} ({_C.ERRORS.get(code, '?')})"
    problems = []
    for label, err, bound in figures():
        print(f"{entry} {length} [{what}] {label}: {err:.3e} (bound {bound:.0e})")
        if not err < bound:
            problems.append(f"{label}: {err:.3e} >= {bound:.0e}")
    P.arena.verify()   # raises PlacementError naming the operand and the span
    assert not problems, f"{entry} {length}, placement {what}:\n" + "\n".join(problems)
    return P


@pytest.mark.parametrize("kind", ["zero", "all1", "mixed"])
@pytest.mark.parametrize("length", list(LENGTHS))
@pytest.mark.parametrize("name", list(CASES))
def test_whole_call_placements(dev, name, length, kind):
    place_and_check(dev, name, length, PLANS[kind], kind)


@pytest.mark.parametrize("length", list(LENGTHS))
@pytest.mark.parametrize("name", list(CASES))
def test_single_operand_placements(dev, name, length):
    """single1: each pointer operand alone at offset 1; single2: each output alone at offset 2 (the 8-byte phase)."""
    base = place_and_check(dev, name, length, PLANS["zero"], "zero")
    for operand, role in base.operands:
        place_and_check(dev, name, length, lambda i, n, r, t=operand: 1 if n == t else 0, f"{operand}@1")
        if role in OUTPUT_ROLES:
            place_and_check(dev, name, length, lambda i, n, r, t=operand: 2 if n == t else 0, f"{operand}@2")


def test_placement_does_not_change_the_values(dev):
    """The stream belongs to the row, not to the addresses: the 16-byte path and the single-element path agree bit for bit."""
    outs = []
    for kind in ("zero", "all1"):
        P = Placer(dev, PLANS[kind])
        r = _row(P)
        out = P.out("out", (LENGTHS["odd"],))
        assert _C.lib().adp_randn(p(r), LENGTHS["odd"], p(out), _C.stream()) == 0
        outs.append(out.cpu().clone())
    assert torch.equal(outs[0], outs[1])


def test_every_rng_entry_point_is_placed():
    assert {entry for _, entry in CASES.values()} == set(_C.RNG_SIGNATURES)
    for other in (_C.SIGNATURES, _C.AR_SIGNATURES, _C.LT_SIGNATURES, _C.ENC_SIGNATURES, _C.T5_SIGNATURES):
        assert not set(_C.RNG_SIGNATURES) & set(other)


def test_header_table_and_libraries_agree(emul):
    """include/adp_rng.h <-> _C.RNG_SIGNATURES <-> what the built libraries export."""
    import ctypes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "adp_rng.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)   # (the comments name other functions)
    declared = set(re.findall(r"\b(adp_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_C.RNG_SIGNATURES), declared ^ set(_C.RNG_SIGNATURES)
    for name in declared:
        assert hasattr(_C.lib(), name), name            # the emulated build of the same sources
    assert os.path.exists(_C.LIB_PATH), "libadp_hip.so is not built (run __graft_entry__.build())"
    hip_lib = ctypes.CDLL(_C.LIB_PATH)
    for name in declared:
        assert hasattr(hip_lib, name), name
    source = open(os.path.join(root, "audio_diffusion_pytorch_amd", "csrc", "rng.hip")).read()
    assert '#include "adp_rng.h"' in source
    assert '#include "inpaint_blend.h"' in source   # the blend is adp_v_inpaint_step's, not a restatement of it
    elementwise = open(os.path.join(root, "audio_diffusion_pytorch_amd", "csrc", "elementwise.hip")).read()
    assert '#include "inpaint_blend.h"' in elementwise and "adp_v_inpaint_blend(" in elementwise
