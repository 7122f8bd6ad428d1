"""The entry points of include/adp_rf.h with misaligned operands and guard bands (tests/placement.py), as
tests/test_sde_placement.py does for include/adp_sde.h: every operand of a direct call through `_C.lib()` is placed by the test
at the zero / all1 / mixed / single1 / single2 placements.  A placed call returns ADP_OK, gives the values of the restatement
(tests/test_rf.py, within its STEP_TOL / NOISE_TOL) and leaves every guard, offset gap and input payload bit-identical.  Two
items per call; two lengths: one on the 16-byte paths (which a misplaced pointer must leave) and an odd one, whose second item
starts off the 16-byte grid and inside a group of four."""
import ctypes

import pytest
import torch

from audio_diffusion_pytorch_amd import _C
from conftest import rel_err
from placement import PLANS, Placer, p, single_operand_tests, whole_call_tests
from test_rf import NOISE_TOL, ROW, STEP_TOL, rf_step_ref

ROWS = 2
LENGTHS = {"vec": 2048, "odd": 1001}
TIMES = torch.tensor([0.3, 0.85])


def _data(n, count):
    g = torch.Generator().manual_seed(n)
    return [torch.randn(ROWS, n, generator=g) * 1.5 for _ in range(count)]


def _noise(P, n):
    x, noise = _data(n, 2)
    xd, nd, td = P.inp("x", x), P.inp("noise", noise), P.inp("t", TIMES)
    xt, u = P.out("x_t_out", (ROWS, n)), P.out("u_out", (ROWS, n))
    code = _C.lib().adp_rf_noise(p(xd), p(nd), p(td), ROWS, n, p(xt), p(u), _C.stream())
    tt = TIMES.double()[:, None]
    want_xt, want_u = (1 - tt) * x.double() + tt * noise.double(), noise.double() - x.double()
    return code, [("x_t_out", rel_err(xt, want_xt), "<=", NOISE_TOL), ("u_out", rel_err(u, want_u), "<=", NOISE_TOL)]


def _step(mode, order):
    def run(P, n):
        x, u, hist = _data(n, 3)
        scale = torch.tensor([1.0, 1.75]) if mode == "scale" else None
        xd, ud = P.inp("x", x), P.inp("u", u)
        hd = P.inp("hist", hist) if order == 2 else None
        cd = P.inp("coef6", ROW)
        sd = P.inp("scale", scale) if scale is not None else None
        out = P.out("x_out", (ROWS, n))
        ho = P.out("hist_out", (ROWS, n)) if order == 2 else None
        code = _C.lib().adp_rf_step(p(xd), p(ud), p(hd), p(cd), order, int(mode != "plain"), p(sd), ROWS, n, p(out), p(ho),
                                    _C.stream())
        row = ROW.clone()
        if order == 1:
            row[5] = 0.0
        want, want_w = rf_step_ref(x, u, hist, row, clip=mode != "plain", scale=scale)

        figures = [("x_out", rel_err(out, want), "<=", STEP_TOL)]
        if order == 2:
            figures.append(("hist_out", rel_err(ho, want_w), "<=", STEP_TOL))
        return code, figures
    return run


CASES = {"noise": (_noise, "adp_rf_noise")}
CASES.update({f"step-{mode}-{order}": (_step(mode, order), "adp_rf_step")
              for mode in ("plain", "static", "scale") for order in (1, 2)})
OUTPUTS = {"adp_rf_noise": ("x_t_out", "u_out"), "adp_rf_step": ("x_out", "hist_out")}


ALL = [(n, l) for n in CASES for l in LENGTHS]
test_whole_call_placements = whole_call_tests(CASES, ALL, LENGTHS.get)
test_single_operand_placements = single_operand_tests(CASES, [(n, l) for n in ("noise", "step-scale-2", "step-plain-1") for l in LENGTHS], LENGTHS.get)


@pytest.mark.parametrize("name", ["noise", "step-scale-2", "step-static-1"])
def test_placement_does_not_change_the_values(dev, name):
    """The arithmetic is per element: the 16-byte and the single-element paths agree bit for bit, at both lengths."""
    for length in LENGTHS.values():
        outs = []
        for kind in ("zero", "all1", "mixed"):
            P = Placer(dev, PLANS[kind])
            code, _ = CASES[name][0](P, length)
            assert code == 0
            outs.append([P.arena.ops[o].view.cpu().clone() for o in OUTPUTS[CASES[name][1]] if o in P.arena.ops])
        for other in outs[1:]:
            assert len(other) == len(outs[0]) and all(torch.equal(a, b) for a, b in zip(outs[0], other))


def test_noise_refusals_in_order_write_nothing(dev):
    ERR_SHAPE, ERR_ALIGN, ERR_NULL = -1, -3, -5
    L, s = _C.lib(), _C.stream()
    x, t = torch.zeros(2, 16, device=dev), torch.zeros(2, device=dev)
    outs = [torch.full((2, 16), 7.0, device=dev) for _ in range(2)]
    q = lambda tensor, off=0: tensor.data_ptr() + off
    args = lambda: [q(x), q(x), q(t), 2, 16, q(outs[0]), q(outs[1])]
    for k in (0, 1, 2, 5, 6):
        a = args()
        a[k] = None
        a[3] = -1                        # NULL is answered before the shape
        assert L.adp_rf_noise(*a, s) == ERR_NULL, k
    for k, bad in ((3, -1), (4, -1), (3, 2 ** 62)):
        a = args()
        a[k] = bad
        a[0] = q(x, 2)                   # the shape is answered before the alignment
        assert L.adp_rf_noise(*a, s) == ERR_SHAPE, (k, bad)
    for k in (0, 1, 2, 5, 6):
        a = args()
        a[k] = a[k] + 2
        assert L.adp_rf_noise(*a, s) == ERR_ALIGN, k
    for k in (3, 4):                     # nothing to do: ADP_OK, nothing launched
        a = args()
        a[k] = 0
        assert L.adp_rf_noise(*a, s) == 0
    assert all(torch.equal(o.cpu(), torch.full((2, 16), 7.0)) for o in outs)
    assert L.adp_rf_noise(*args(), s) == 0 and all(torch.equal(o.cpu(), torch.zeros(2, 16)) for o in outs)
    assert _C.ABI["adp_rf.h"]["adp_rf_noise"] == (ctypes.c_int, [_C.P] * 3 + [_C.I] * 2 + [_C.P] * 3)


def test_step_refusals_in_order_write_nothing(dev):
    ERR_SHAPE, ERR_ALIGN, ERR_NULL = -1, -3, -5
    L, s = _C.lib(), _C.stream()
    x = torch.zeros(2, 16, device=dev)
    coef, scale = torch.zeros(6, device=dev), torch.ones(2, device=dev)
    out, hout = torch.full((2, 16), 7.0, device=dev), torch.full((2, 16), 7.0, device=dev)
    q = lambda tensor, off=0: tensor.data_ptr() + off
    # x, u, hist, coef6, order, clip, scale, rows, per, x_out, hist_out
    args = lambda: [q(x), q(x), q(x), q(coef), 2, 1, q(scale), 2, 16, q(out), q(hout)]
    for k in (0, 1, 2, 3, 9, 10):        # the pointers an order-2 call needs; scale (6) may be NULL
        a = args()
        a[k] = None
        a[7] = -1                        # NULL is answered before the shape
        assert L.adp_rf_step(*a, s) == ERR_NULL, k
    for k, bad in ((7, -1), (8, -1), (4, 0), (4, 3), (5, 2), (5, -1), (7, 2 ** 62)):
        a = args()
        a[k] = bad
        a[0] = q(x, 2)                   # the shape is answered before the alignment
        assert L.adp_rf_step(*a, s) == ERR_SHAPE, (k, bad)
    a = args()
    a[5] = 0                             # a scale without clip
    assert L.adp_rf_step(*a, s) == ERR_SHAPE
    for k in (0, 1, 2, 3, 6, 9, 10):
        a = args()
        a[k] = a[k] + 2
        assert L.adp_rf_step(*a, s) == ERR_ALIGN, k
    for k in (7, 8):                     # nothing to do: ADP_OK, nothing launched
        a = args()
        a[k] = 0
        assert L.adp_rf_step(*a, s) == 0
    assert torch.equal(out.cpu(), torch.full((2, 16), 7.0)) and torch.equal(hout.cpu(), torch.full((2, 16), 7.0))
    # order 1 does not look at the history pointers: NULL or misaligned, and writes none
    for hist, hist_out in ((None, None), (q(x, 2), q(hout, 2))):
        a = args()
        a[4], a[2], a[10] = 1, hist, hist_out
        assert L.adp_rf_step(*a, s) == 0
        assert torch.equal(out.cpu(), torch.zeros(2, 16)) and torch.equal(hout.cpu(), torch.full((2, 16), 7.0))
        out.fill_(7.0)
    assert L.adp_rf_step(*args(), s) == 0 and torch.equal(hout.cpu(), torch.zeros(2, 16))
    assert _C.ABI["adp_rf.h"]["adp_rf_step"] == (ctypes.c_int, [_C.P] * 4 + [_C.I, _C.I, _C.P, _C.I, _C.I, _C.P, _C.P, _C.P])


def test_every_rf_entry_point_is_placed():
    assert {entry for _, entry in CASES.values()} == set(_C.ABI["adp_rf.h"])
