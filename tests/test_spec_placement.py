"""The entry points of include/adp_spec.h with misaligned operands and guard bands (tests/placement.py), as
tests/test_repaint_placement.py does for include/adp_repaint.h: every operand of a direct call through `_C.lib()` -- the
filterbank, the two range arrays and the taps included -- is placed by the test at the zero / all1 / mixed / single1 / single2
placements.  A placed call returns ADP_OK, gives the values of the restatement (tests/test_spectral_loss.py) and leaves every
guard, offset gap and input payload bit-identical.  Two lengths: one whose rows start on the 16-byte grid (which a misplaced
pointer must leave) and an odd one, whose second row starts off it."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from audio_diffusion_pytorch_amd import _C, ops, spectral
from placement import PLANS, Placer, close, p, single_operand_tests, whole_call_tests
from test_spectral_loss import spec_ref
from test_stft_loss import GRAD_TOL, LOSS_TOL, _pair

RES = ((256, 64, 200), (64, 16, 64))
SR, BINS = 16000, 8
WEIGHTS = (0.5, 2.0, 1.5, 1e-8, 0.7, 1.3)   # w_sc, w_log, w_lin, eps, w_sum, w_diff
REF_KW = dict(w_sc=0.5, w_log=2.0, w_lin=1.5, w_sum=0.7, w_diff=1.3)
LENGTHS = {"vec": 1024, "odd": 1001}
FIR_TOL = 2.0 ** -23   # one rounding of the exact sum, relative to the largest output


def _bank():
    crit = spectral.MultiResolutionSTFTLoss([r[0] for r in RES], [r[1] for r in RES], [r[2] for r in RES], scale="mel",
                                            sample_rate=SR, n_bins=BINS)
    return crit.mel_fb, crit.mel_range, crit.bin_range


def _arrays(mel):
    res = ops._stft_res(RES)
    return res, ops._spec_bins(RES, [BINS] * len(RES) if mel else None)


def _ws_bytes(rows, n, pair, mel, backward):
    res, bins = _arrays(mel)
    return _C.query("adp_spec_loss_ws_bytes", rows, n, int(pair), len(RES), res, bins, backward)


def _loss(pair, mel, backward):
    def run(P, n):
        x, y = _pair((1, 2, n), n)
        res, bins = _arrays(mel)
        fb, mr, br = _bank() if mel else (None, None, None)
        if not backward:
            xd, yd = P.inp("x", x), P.inp("y", y)
            fbd, mrd = (P.inp("fb", fb), P.inp("mel_range", mr)) if mel else (None, None)
            loss, ws = P.out("loss", (1,)), P.ws("ws", _ws_bytes(2, n, pair, mel, 0))
            code = _C.lib().adp_spec_loss_fwd(p(xd), p(yd), 2, n, int(pair), len(RES), res, bins, p(fbd), p(mrd), *WEIGHTS,
                                              p(loss), p(ws), _C.stream())
            want = spec_ref(x, y, RES, pair=pair, mel=(SR, BINS) if mel else None, **REF_KW)
            return code, [("loss", abs(loss.cpu().item() - want.item()) / abs(want.item()), "<=", LOSS_TOL)]
        # the forward workspace and the incoming gradient come from an unplaced forward call
        dev = P.arena.dev
        at = lambda t: None if t is None else t.to(dev)
        _, ws_fwd = ops.spec_loss_fwd(x.to(dev), y.to(dev), pair, RES, [BINS] * len(RES) if mel else None, at(fb), at(mr),
                                      *WEIGHTS)
        xd, yd, gd, wd = P.inp("x", x), P.inp("y", y), P.inp("gloss", torch.tensor([0.25])), P.inp("ws_fwd", ws_fwd.cpu())
        fbd, mrd, brd = (P.inp("fb", fb), P.inp("mel_range", mr), P.inp("bin_range", br)) if mel else (None, None, None)
        dx, ws = P.out("dx", (1, 2, n)), P.ws("ws", _ws_bytes(2, n, pair, mel, 1))
        code = _C.lib().adp_spec_loss_bwd(p(xd), p(yd), p(gd), p(wd), 2, n, int(pair), len(RES), res, bins, p(fbd), p(mrd),
                                          p(brd), *WEIGHTS, p(dx), p(ws), _C.stream())
        xr = x.double().requires_grad_(True)
        (spec_ref(xr, y, RES, pair=pair, mel=(SR, BINS) if mel else None, **REF_KW) / 4).backward()
        return code, [close("dx", dx, xr.grad, GRAD_TOL)]
    return run


def _fir(T):
    def run(P, n):
        g = torch.Generator().manual_seed(n + T)
        x, taps = torch.randn(3, n, generator=g), torch.randn(T, generator=g)
        xd, td = P.inp("x", x), P.inp("taps", taps)
        out = P.out("out", (3, n))
        code = _C.lib().adp_spec_fir(p(xd), p(td), 3, n, T, p(out), _C.stream())
        want = F.conv1d(x.double()[:, None], taps.double().view(1, 1, -1), padding=T // 2)[:, 0]
        return code, [("out", (out.cpu().double() - want).abs().max().item() / want.abs().max().item(), "<=", FIR_TOL)]
    return run


CASES = {"fwd-plain": (_loss(False, False, False), "adp_spec_loss_fwd"),
         "fwd-pair-mel": (_loss(True, True, False), "adp_spec_loss_fwd"),
         "bwd-plain": (_loss(False, False, True), "adp_spec_loss_bwd"),
         "bwd-pair-mel": (_loss(True, True, True), "adp_spec_loss_bwd"),
         "fir-5": (_fir(5), "adp_spec_fir"), "fir-101": (_fir(101), "adp_spec_fir")}
# entry points that are not placed, each with its reason
EXCLUDED = {"adp_spec_loss_ws_bytes": "host only: reads the two host arrays and launches nothing"}

ALL = [(n, l) for n in CASES for l in LENGTHS]
test_whole_call_placements = whole_call_tests(CASES, ALL, LENGTHS.get)
test_single_operand_placements = single_operand_tests(
    CASES, [(n, l) for n in ("fwd-pair-mel", "bwd-pair-mel", "fir-101") for l in LENGTHS], LENGTHS.get)


@pytest.mark.parametrize("name", ["fwd-pair-mel", "bwd-pair-mel", "fir-101"])
def test_placement_does_not_change_the_values(dev, name):
    """The loss kernels read single elements; the FIR stages with 16-byte loads where the row's offset allows and single
    elements otherwise: the same bits either way, at both lengths."""
    target = {"fwd-pair-mel": "loss", "bwd-pair-mel": "dx", "fir-101": "out"}[name]
    for length in LENGTHS.values():
        outs = []
        for plan in (PLANS["zero"], PLANS["all1"], PLANS["mixed"]):
            P = Placer(dev, plan)
            code, _ = CASES[name][0](P, length)
            assert code == 0
            outs.append(P.arena.ops[target].view.cpu().clone())
        assert all(torch.equal(outs[0], other) for other in outs[1:])


def test_refusals_in_order_write_nothing(dev):
    ERR_SHAPE, ERR_UNSUPPORTED, ERR_ALIGN, ERR_NULL = -1, -2, -3, -5
    lib, s = _C.lib(), _C.stream()
    n = 512
    x = torch.zeros(2, n, device=dev)
    fb, mr, br = (t.to(dev) for t in _bank())
    loss, ws = torch.full((1,), 7.0, device=dev), torch.full((8192,), 7.0, device=dev)
    dx, gl = torch.full((2, n), 7.0, device=dev), torch.ones(1, device=dev)
    res, bins = _arrays(True)
    q = lambda t, off=0: t.data_ptr() + off
    # x, y, rows, length, pair, nres, res, n_bins, fb, mel_range, 6 floats, loss, ws
    fwd = lambda: [q(x), q(x), 2, n, 1, len(RES), res, bins, q(fb), q(mr), *WEIGHTS, q(loss), q(ws)]
    # x, y, gloss, ws_fwd, rows, length, pair, nres, res, n_bins, fb, mel_range, bin_range, 6 floats, dx, ws
    bwd = lambda: [q(x), q(x), q(gl), q(ws), 2, n, 1, len(RES), res, bins, q(fb), q(mr), q(br), *WEIGHTS, q(dx), q(ws)]
    for fn, args, ptrs, rows_at, optional in ((lib.adp_spec_loss_fwd, fwd, (0, 1, 6, 8, 16, 17), 2, (9,)),
                                              (lib.adp_spec_loss_bwd, bwd, (0, 1, 3, 8, 10, 19, 20), 4, (2, 11, 12))):
        for k in ptrs:
            a = args()
            a[k] = None
            if k != rows_at + 4:
                a[rows_at] = -1              # NULL is answered before the shape (the shape cannot be read without res)
            assert fn(*a, s) == ERR_NULL, k
        for k, bad in ((rows_at, 0), (rows_at, 3), (rows_at, 65536), (rows_at + 1, 32), (rows_at + 2, 2), (rows_at + 3, 5)):
            a = args()
            a[k] = bad
            a[0] = q(x, 2)                   # the shape is answered before the alignment
            assert fn(*a, s) == ERR_SHAPE, (k, bad)
        a = args()
        a[rows_at + 5] = ops._spec_bins(RES, [BINS, 32])   # more filters than N / 2 - 1 = 31
        assert fn(*a, s) == ERR_UNSUPPORTED
        a = args()
        a[rows_at + 4] = ops._stft_res(((256, 64, 200), (96, 16, 64)))
        assert fn(*a, s) == ERR_UNSUPPORTED
        pointers = [k for k in range(len(a)) if k not in (rows_at + 4, rows_at + 5) and isinstance(a[k], int) and a[k] > 2 ** 20]
        assert set(ptrs) - {rows_at + 4} <= set(pointers) and set(optional) <= set(pointers)
        for k in pointers:
            a = args()
            a[k] = a[k] + 2
            assert fn(*a, s) == ERR_ALIGN, k
    # x, taps, rows, length, ntaps, out
    fir = lambda: [q(x), q(gl), 2, n, 1, q(dx)]
    for k in (0, 1, 5):
        a = fir()
        a[k] = None
        a[2] = -1
        assert lib.adp_spec_fir(*a, s) == ERR_NULL, k
    for k, bad in ((2, -1), (3, -1), (4, 0), (4, 2), (4, 257), (2, 2 ** 40)):
        a = fir()
        a[k] = bad
        a[0] = q(x, 2)
        assert lib.adp_spec_fir(*a, s) == ERR_SHAPE, (k, bad)
    for k in (0, 1, 5):
        a = fir()
        a[k] = a[k] + 2
        assert lib.adp_spec_fir(*a, s) == ERR_ALIGN, k
    for k in (2, 3):                         # nothing to do: ADP_OK, nothing launched
        a = fir()
        a[k] = 0
        assert lib.adp_spec_fir(*a, s) == 0
    assert _C.query("adp_spec_loss_ws_bytes", 2, n, 1, len(RES), res, bins, 0) > 0
    assert lib.adp_spec_loss_ws_bytes(2, n, 1, len(RES), None, bins, 0) == ERR_NULL
    assert lib.adp_spec_loss_ws_bytes(3, n, 1, len(RES), res, bins, 0) == ERR_SHAPE
    for t in (loss, ws, dx):
        assert torch.equal(t.cpu(), torch.full(t.shape, 7.0))
    F_, I_, P_ = _C.F, _C.I, _C.P
    assert _C.ABI["adp_spec.h"]["adp_spec_fir"] == (ctypes.c_int, [P_, P_, I_, I_, I_, P_, P_])
    assert _C.ABI["adp_spec.h"]["adp_spec_loss_fwd"] == (ctypes.c_int, [P_, P_] + [I_] * 4 + [P_] * 4 + [F_] * 6 + [P_] * 3)


def test_every_spec_entry_point_is_placed():
    assert {entry for _, entry in CASES.values()} | set(EXCLUDED) == set(_C.ABI["adp_spec.h"])
    assert all(EXCLUDED.values())
