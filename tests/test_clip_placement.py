"""The entry points of include/adp_clip.h with misaligned operands and guard bands (tests/placement.py), as
tests/test_rng_placement.py does for include/adp_rng.h: every operand of a direct call through `_C.lib()` is placed by the test
at the zero / all1 / mixed / single1 / single2 placements.  A placed call returns ADP_OK, gives the values of the restatement
(tests/test_threshold_sampler.py: the quantile of |x| within 2**-22 relative, the fused one within its derived bound, the
elementwise kernels within their roundings) and leaves every guard, offset gap and input payload bit-identical.  Two items per
call; two lengths: one on the 16-byte paths (which a misplaced pointer must leave) and an odd one, whose second item starts
off the 16-byte grid wherever the first one is."""
import os

import torch

from audio_diffusion_pytorch_amd import _C
from conftest import rel_err
from placement import PLANS, Placer, p, single_operand_tests, whole_call_tests
from test_multistep_sampler import KERNEL_TOL, coef_table
from test_threshold_sampler import CLIP_TOL, LERP_TOL, clip_ref, quantile_ref, rank_of, threshold_step_ref

ROWS, Q = 2, 0.9
LENGTHS = {"vec": 2048, "odd": 1001}
COEF = coef_table(torch.tensor([0.62, 0.55, 0.5]))[1].to(torch.float32)   # (a0, b0, a1, b1, ca, cb), ca and cb not 0


def _data(n, count):
    g = torch.Generator().manual_seed(n)
    return [torch.randn(ROWS, n, generator=g) * 1.5 for _ in range(count)]


def _ws_numel(n):
    return (_C.query("adp_clip_ws_bytes", ROWS, n) + 3) // 4


def _scale(P, n):
    (x,) = _data(n, 1)
    xd = P.inp("x", x)
    ws, out = P.ws_numel("ws", _ws_numel(n)), P.out("scale", (ROWS,))
    lo, _, w = rank_of(Q, n)
    code = _C.lib().adp_clip_scale(p(xd), None, None, ROWS, n, lo, float(w), 0.0, p(ws), p(out), _C.stream())
    want = torch.quantile(x.abs(), Q, dim=-1)
    return code, [("scale", ((out.cpu() - want).abs() / want).max().item(), "<=", LERP_TOL)]


def _scale_fused(P, n):
    x, v = _data(n, 2)
    xd, vd, cd = P.inp("x", x), P.inp("v", v), P.inp("coef", COEF)
    ws, out = P.ws_numel("ws", _ws_numel(n)), P.out("scale", (ROWS,))
    lo, _, w = rank_of(Q, n)
    code = _C.lib().adp_clip_scale(p(xd), p(vd), p(cd), ROWS, n, lo, float(w), 1.0, p(ws), p(out), _C.stream())
    a0, b0 = COEF[0].double(), COEF[1].double()
    want = quantile_ref((a0 * x.double() - b0 * v.double()).abs(), Q).clamp(min=1.0)
    bound = 4 * 2.0 ** -24 * ((a0 * x.double()).abs() + (b0 * v.double()).abs()).max().item()
    return code, [("scale", (out.cpu().double() - want).abs().max().item(), "<=", bound)]


def _apply(P, n):
    (x,) = _data(n, 1)
    scale = torch.tensor([1.0, 1.75])
    xd, sd = P.inp("x", x), P.inp("scale", scale)
    out = P.out("out", (ROWS, n))
    code = _C.lib().adp_clip_apply(p(xd), p(sd), ROWS, n, p(out), _C.stream())
    want = x.clamp(-scale[:, None], scale[:, None]) / scale[:, None]
    return code, [("out", rel_err(out, want), "<=", CLIP_TOL)]


def _step(order, dynamic):
    def run(P, n):
        x, v, hx, he = _data(n, 4)
        scale = torch.tensor([1.0, 1.75])
        row = COEF if order == 2 else COEF[:4].contiguous()
        xd, vd = P.inp("x", x), P.inp("v", v)
        hxd = hed = None
        if order == 2:
            hxd, hed = P.inp("hist_x0", hx), P.inp("hist_eps", he)
        cd = P.inp("coef", row)
        sd = P.inp("scale", scale) if dynamic else None
        outs = [P.out("x_out", (ROWS, n))]
        if order == 2:
            outs += [P.out("hist_x0_out", (ROWS, n)), P.out("hist_eps_out", (ROWS, n))]
        code = _C.lib().adp_clip_step(p(xd), p(vd), p(hxd), p(hed), p(cd), order, p(sd), ROWS, n, p(outs[0]),
                                      p(outs[1]) if order == 2 else None, p(outs[2]) if order == 2 else None, _C.stream())
        want = threshold_step_ref(x, v, hx, he, row, scale if dynamic else None)
        return code, [(name, rel_err(o, r), "<=", KERNEL_TOL)
                      for name, o, r in zip(("x_out", "hist_x0_out", "hist_eps_out"), outs, want)]
    return run


CASES = {"scale": (_scale, "adp_clip_scale"), "scale_fused": (_scale_fused, "adp_clip_scale"),
         "apply": (_apply, "adp_clip_apply"), "step1": (_step(1, True), "adp_clip_step"),
         "step2": (_step(2, True), "adp_clip_step"), "step2_static": (_step(2, False), "adp_clip_step")}
HOST_ONLY = {"adp_clip_ws_bytes"}   # takes no pointer


ALL = [(n, l) for n in CASES for l in LENGTHS]
test_whole_call_placements = whole_call_tests(CASES, ALL, LENGTHS.get)
test_single_operand_placements = single_operand_tests(CASES, ALL, LENGTHS.get)


def test_placement_does_not_change_the_values(dev):
    """The selection is exact and the arithmetic per element: the 16-byte and the single-element paths agree bit for bit."""
    outs = []
    for kind in ("zero", "all1"):
        P = Placer(dev, PLANS[kind])
        x, v = _data(LENGTHS["vec"], 2)
        xd, vd, cd = P.inp("x", x), P.inp("v", v), P.inp("coef", COEF)
        ws, scale = P.ws_numel("ws", _ws_numel(LENGTHS["vec"])), P.out("scale", (ROWS,))
        lo, _, w = rank_of(Q, LENGTHS["vec"])
        assert _C.lib().adp_clip_scale(p(xd), p(vd), p(cd), ROWS, LENGTHS["vec"], lo, float(w), 1.0, p(ws), p(scale),
                                       _C.stream()) == 0
        out = P.out("x_out", (ROWS, LENGTHS["vec"]))
        assert _C.lib().adp_clip_step(p(xd), p(vd), None, None, p(cd), 1, p(scale), ROWS, LENGTHS["vec"], p(out), None, None,
                                      _C.stream()) == 0
        outs.append((scale.cpu().clone(), out.cpu().clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_every_clip_entry_point_is_placed():
    assert {entry for _, entry in CASES.values()} | HOST_ONLY == set(_C.ABI["adp_clip.h"])


def test_x0_is_formed_by_one_helper():
    csrc = os.path.join(os.path.dirname(_C.__file__), "csrc")
    source = open(os.path.join(csrc, "clip.hip")).read()
    # one helper forms x0 for the select's passes and for every step kernel: they must round alike.  It is defined once, on
    # the one fused multiply-add of csrc/sampler_update.h, and no kernel source that clamps x0 spells either again
    shared = open(os.path.join(csrc, "sampler_update.h")).read()
    assert shared.count("float clip_x0(") == 1 and shared.count("__fmaf_rn") == 1
    assert source.count("clip_x0(") >= 2  # the key of the passes and the step
    for unit in ("clip.hip", "sde.hip", "rf.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "sampler_update.h"' in text and "clip_x0(" in text and "__fmaf_rn" not in text, unit
