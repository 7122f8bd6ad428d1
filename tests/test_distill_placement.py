"""The entry points of include/adp_distill.h with misaligned operands and guard bands (tests/placement.py), as
tests/test_rf_placement.py does for include/adp_rf.h: every operand of a direct call through `_C.lib()` is placed by the test
at the zero / all1 / mixed / single1 / single2 placements.  A placed call returns ADP_OK, gives the values of the float64
restatement (tests/test_distill.py, within its bounds) and leaves every guard, offset gap and input payload bit-identical.
Two items per call; two lengths: one on the 16-byte paths (which a misplaced pointer must leave) and an odd one, whose second
item starts off the 16-byte grid and inside a group of four."""
import ctypes

import pytest
import torch

from audio_diffusion_pytorch_amd import _C
from conftest import rel_err
from placement import PLANS, Placer, p, single_operand_tests, whole_call_tests
from test_distill import COEF, WMSE_TOL, _col, _comb_bound, _comb_ref

ROWS = 2
LENGTHS = {"vec": 2048, "odd": 1001}
WEIGHTS = torch.tensor([0.5, 0.75])
GLOSS = torch.tensor([0.37])


def _data(n, count):
    g = torch.Generator().manual_seed(n)
    return [torch.randn(ROWS, n, generator=g) * 1.5 for _ in range(count)]


def _comb(terms):
    def run(P, n):
        x, pp, q = _data(n, 3)
        q = q if terms == 3 else None
        coef = COEF[:terms, :ROWS].contiguous()
        xd, pd = P.inp("x", x), P.inp("p", pp)
        qd = P.inp("q", q) if q is not None else None
        cd = P.inp("coef", coef)
        out = P.out("out", (ROWS, n))
        code = _C.lib().adp_distill_comb(p(xd), p(pd), p(qd), p(cd), terms, ROWS, n, p(out), _C.stream())
        err = (out.double().cpu() - _comb_ref(x, pp, q, coef)).abs().max().item()
        return code, [("out", err, "<=", _comb_bound(x, pp, q, coef))]
    return run


def _wmse_fwd(weighted):
    def run(P, n):
        a, b = _data(n, 2)
        ad, bd = P.inp("v_pred", a), P.inp("v_target", b)
        wd = P.inp("w", WEIGHTS) if weighted else None
        loss = P.out("loss", (1,))
        ws = P.ws("ws", _C.lib().adp_distill_wmse_ws_bytes(ROWS, n))
        code = _C.lib().adp_distill_wmse_fwd(p(ad), p(bd), p(wd), ROWS, n, p(loss), p(ws), _C.stream())
        w = WEIGHTS.double() if weighted else torch.ones(ROWS, dtype=torch.float64)
        want = (_col(w, a) * (a.double() - b.double()) ** 2).mean()
        return code, [("loss", rel_err(loss, want.reshape(1)), "<=", WMSE_TOL)]
    return run


def _wmse_bwd(weighted, with_gloss):
    def run(P, n):
        a, b = _data(n, 2)
        ad, bd = P.inp("v_pred", a), P.inp("v_target", b)
        wd = P.inp("w", WEIGHTS) if weighted else None
        gd = P.inp("gloss", GLOSS) if with_gloss else None
        dv = P.out("dv", (ROWS, n))
        code = _C.lib().adp_distill_wmse_bwd(p(ad), p(bd), p(wd), p(gd), ROWS, n, p(dv), _C.stream())
        w = WEIGHTS.double() if weighted else torch.ones(ROWS, dtype=torch.float64)
        gl = GLOSS.double().item() if with_gloss else 1.0
        want = gl * 2 * _col(w, a) * (a.double() - b.double()) / a.numel()
        return code, [("dv", rel_err(dv, want), "<=", WMSE_TOL)]
    return run


CASES = {"comb-2": (_comb(2), "adp_distill_comb"), "comb-3": (_comb(3), "adp_distill_comb"),
         "wmse-fwd-w": (_wmse_fwd(True), "adp_distill_wmse_fwd"), "wmse-fwd-plain": (_wmse_fwd(False), "adp_distill_wmse_fwd"),
         "wmse-bwd-w": (_wmse_bwd(True, True), "adp_distill_wmse_bwd"),
         "wmse-bwd-plain": (_wmse_bwd(False, False), "adp_distill_wmse_bwd")}
OUTPUTS = {"adp_distill_comb": ("out",), "adp_distill_wmse_fwd": ("loss",), "adp_distill_wmse_bwd": ("dv",)}


ALL = [(n, l) for n in CASES for l in LENGTHS]
test_whole_call_placements = whole_call_tests(CASES, ALL, LENGTHS.get)
test_single_operand_placements = single_operand_tests(CASES, [(n, l) for n in ("comb-3", "wmse-fwd-w", "wmse-bwd-w") for l in LENGTHS], LENGTHS.get)


@pytest.mark.parametrize("name", list(CASES))
def test_placement_does_not_change_the_values(dev, name):
    """The arithmetic is per element and the loss is summed in a fixed order: the 16-byte and the single-element paths agree
    bit for bit, at both lengths."""
    for length in LENGTHS.values():
        outs = []
        for kind in ("zero", "all1", "mixed"):
            P = Placer(dev, PLANS[kind])
            code, _ = CASES[name][0](P, length)
            assert code == 0
            outs.append([P.arena.ops[o].view.cpu().clone() for o in OUTPUTS[CASES[name][1]]])
        for other in outs[1:]:
            assert len(other) == len(outs[0]) and all(torch.equal(a, b) for a, b in zip(outs[0], other))


ERR_SHAPE, ERR_ALIGN, ERR_NULL = -1, -3, -5


def _q(tensor, off=0):
    return tensor.data_ptr() + off


def test_comb_refusals_in_order_write_nothing(dev):
    L, s = _C.lib(), _C.stream()
    x, coef = torch.zeros(2, 16, device=dev), torch.zeros(3, 2, device=dev)
    out = torch.full((2, 16), 7.0, device=dev)
    # x, p, q, coef, terms, rows, per, out
    args = lambda: [_q(x), _q(x), _q(x), _q(coef), 3, 2, 16, _q(out)]
    for k in (0, 1, 2, 3, 7):
        a = args()
        a[k] = None
        a[5] = -1                        # NULL is answered before the shape
        assert L.adp_distill_comb(*a, s) == ERR_NULL, k
    for k, bad in ((5, -1), (6, -1), (4, 1), (4, 4), (4, 0), (5, 2 ** 62)):
        a = args()
        a[k] = bad
        a[0] = _q(x, 2)                  # the shape is answered before the alignment
        assert L.adp_distill_comb(*a, s) == ERR_SHAPE, (k, bad)
    a = args()
    a[4], a[0] = 2, _q(x, 2)             # a q with two terms
    assert L.adp_distill_comb(*a, s) == ERR_SHAPE
    for k in (0, 1, 2, 3, 7):
        a = args()
        a[k] = a[k] + 2
        assert L.adp_distill_comb(*a, s) == ERR_ALIGN, k
    for k in (5, 6):                     # nothing to do: ADP_OK, nothing launched
        a = args()
        a[k] = 0
        assert L.adp_distill_comb(*a, s) == 0
    assert torch.equal(out.cpu(), torch.full((2, 16), 7.0))
    a = args()
    a[4], a[2] = 2, None                 # two terms take no q
    assert L.adp_distill_comb(*a, s) == 0 and torch.equal(out.cpu(), torch.zeros(2, 16))
    out.fill_(7.0)
    assert L.adp_distill_comb(*args(), s) == 0 and torch.equal(out.cpu(), torch.zeros(2, 16))
    assert _C.ABI["adp_distill.h"]["adp_distill_comb"] == (ctypes.c_int, [_C.P] * 4 + [_C.I] * 3 + [_C.P] * 2)


def test_wmse_fwd_refusals_in_order_write_nothing(dev):
    L, s = _C.lib(), _C.stream()
    x, w = torch.zeros(2, 16, device=dev), torch.ones(2, device=dev)
    loss = torch.full((1,), 7.0, device=dev)
    assert L.adp_distill_wmse_ws_bytes(2, 16) > 0 and L.adp_distill_wmse_ws_bytes(0, 16) > 0
    assert L.adp_distill_wmse_ws_bytes(-1, 16) == ERR_SHAPE and L.adp_distill_wmse_ws_bytes(2, -1) == ERR_SHAPE
    assert L.adp_distill_wmse_ws_bytes(2 ** 62, 16) == ERR_SHAPE
    ws = torch.full((L.adp_distill_wmse_ws_bytes(2, 16) // 4,), 7.0, device=dev)
    # v_pred, v_target, w, rows, per, loss, ws
    args = lambda: [_q(x), _q(x), _q(w), 2, 16, _q(loss), _q(ws)]
    for k in (0, 1, 5, 6):               # w (2) may be NULL
        a = args()
        a[k] = None
        a[3] = -1
        assert L.adp_distill_wmse_fwd(*a, s) == ERR_NULL, k
    for k, bad in ((3, -1), (4, -1), (3, 2 ** 62)):
        a = args()
        a[k] = bad
        a[0] = _q(x, 2)
        assert L.adp_distill_wmse_fwd(*a, s) == ERR_SHAPE, (k, bad)
    for k in (0, 1, 2, 5, 6):
        a = args()
        a[k] = a[k] + 2
        assert L.adp_distill_wmse_fwd(*a, s) == ERR_ALIGN, k
    for k in (3, 4):
        a = args()
        a[k] = 0
        assert L.adp_distill_wmse_fwd(*a, s) == 0
    assert loss.item() == 7.0 and torch.equal(ws.cpu(), torch.full(ws.shape, 7.0))
    a = args()
    a[2] = None
    assert L.adp_distill_wmse_fwd(*a, s) == 0 and loss.item() == 0.0
    assert _C.ABI["adp_distill.h"]["adp_distill_wmse_fwd"] == (ctypes.c_int, [_C.P] * 3 + [_C.I] * 2 + [_C.P] * 3)
    assert _C.ABI["adp_distill.h"]["adp_distill_wmse_ws_bytes"] == (_C.I, [_C.I] * 2)


def test_wmse_bwd_refusals_in_order_write_nothing(dev):
    L, s = _C.lib(), _C.stream()
    x, w, gl = torch.zeros(2, 16, device=dev), torch.ones(2, device=dev), torch.ones(1, device=dev)
    dv = torch.full((2, 16), 7.0, device=dev)
    # v_pred, v_target, w, gloss, rows, per, dv
    args = lambda: [_q(x), _q(x), _q(w), _q(gl), 2, 16, _q(dv)]
    for k in (0, 1, 6):                  # w (2) and gloss (3) may be NULL
        a = args()
        a[k] = None
        a[4] = -1
        assert L.adp_distill_wmse_bwd(*a, s) == ERR_NULL, k
    for k, bad in ((4, -1), (5, -1), (4, 2 ** 62)):
        a = args()
        a[k] = bad
        a[0] = _q(x, 2)
        assert L.adp_distill_wmse_bwd(*a, s) == ERR_SHAPE, (k, bad)
    for k in (0, 1, 2, 3, 6):
        a = args()
        a[k] = a[k] + 2
        assert L.adp_distill_wmse_bwd(*a, s) == ERR_ALIGN, k
    for k in (4, 5):
        a = args()
        a[k] = 0
        assert L.adp_distill_wmse_bwd(*a, s) == 0
    assert torch.equal(dv.cpu(), torch.full((2, 16), 7.0))
    a = args()
    a[2], a[3] = None, None
    assert L.adp_distill_wmse_bwd(*a, s) == 0 and torch.equal(dv.cpu(), torch.zeros(2, 16))
    assert _C.ABI["adp_distill.h"]["adp_distill_wmse_bwd"] == (ctypes.c_int, [_C.P] * 4 + [_C.I] * 2 + [_C.P] * 2)


def test_every_distill_entry_point_is_placed():
    placed = {entry for _, entry in CASES.values()} | {"adp_distill_wmse_ws_bytes"}   # (the query takes no pointer)
    assert placed == set(_C.ABI["adp_distill.h"])
