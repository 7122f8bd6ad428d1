"""Host-side operator layer: one Python function per C-ABI entry point of include/adp.h.

These only marshal tensors (device pointers, shapes, the current HIP stream) into the hand-written
gfx950 kernels; they hold no arithmetic of their own and have no fallback.  Outputs are allocated by
the caller or with torch.empty on the input's device (PyTorch = device memory + streams only).
"""
import contextlib
import ctypes
import math
import os
from ctypes import byref
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _C
from ._C import ConvDesc, WgradDesc, ptr

GN_EPS = 1e-5
# LayerNorm epsilons of the two item families, separately switchable (oracle/a_unet_restatement.py [switch] block: a_unet's
# Modulation may carry eps=1e-6 on its own LayerNorm; unverifiable offline, both 1e-5 until tools/pin_a_unet.py says otherwise)
MODULATION_LN_EPS = 1e-5
ATTENTION_LN_EPS = 1e-5


def _ws(nbytes: int, like: Tensor) -> Tensor:
    return torch.empty(max(1, (nbytes + 3) // 4), dtype=torch.float32, device=like.device)


def conv_out_len(Lin: int, KT: int, stride: int, dil: int, pad: int, up: int) -> int:
    return (Lin * up + 2 * pad - dil * (KT - 1) - 1) // stride + 1


def conv1d(x: Tensor, w: Tensor, bias: Optional[Tensor] = None, *, stride: int = 1, dil: int = 1, pad: int = 0,
           up: int = 1, transposed: bool = False, x2: Optional[Tensor] = None, prologue: int = 0,
           pro_stats: Optional[Tensor] = None, pro_gamma: Optional[Tensor] = None, pro_beta: Optional[Tensor] = None,
           groups: int = 1, e_scale: Optional[Tensor] = None, e_bstride: int = 0, res: Optional[Tensor] = None,
           store: int = 0, sp: int = 1, N: Optional[int] = None, out: Optional[Tensor] = None,
           out_pre: Optional[Tensor] = None, gn: Optional["GnPart"] = None, gnb: Optional["GnBwdPart"] = None) -> Tensor:
    """Fused implicit-GEMM conv (adp_conv1d).  w: [M, R, KT] (or [R, M, KT] when transposed).
    `gn`: a GnPart to fill with the GroupNorm partial statistics of the output (left empty when the dispatched kernel
    family cannot produce them; the consumer then runs adp_gn_stats).
    `gnb`: a GnBwdPart naming the SiLU(GroupNorm(x)) whose output gradient this (data-gradient) launch produces: the epilogue
    leaves the first stage of that backward in gnb.ab when the dispatched kernel can (else gnb.ab stays None and
    gn_silu_bwd runs its own pass)."""
    B, R1, Lin = x.shape
    R = R1 + (x2.shape[1] if x2 is not None else 0)
    if transposed:
        Rw, M, KT = w.shape
    else:
        M, Rw, KT = w.shape
    assert Rw == R, f"weight expects {Rw} input channels, got {R}"
    if N is None:
        N = conv_out_len(Lin, KT, stride, dil, pad, up)
    if store == 0:
        oshape = (B, M, N)
    elif store == 1:
        oshape = (B, M // sp, N * sp)
    else:
        oshape = (B, M, N // sp)
    if out is None:
        out = torch.empty(oshape, dtype=torch.float32, device=x.device)
    else:
        assert tuple(out.shape) == oshape, (out.shape, oshape)
    d = ConvDesc(ptr(x), ptr(x2), ptr(w), ptr(bias), ptr(pro_stats), ptr(pro_gamma), ptr(pro_beta), ptr(e_scale),
                 ptr(res), ptr(out), ptr(out_pre), B, R, R1, Lin, M, N, KT, stride, dil, pad, up, int(transposed), prologue, groups,
                 store, sp, e_bstride, None, None)
    need = _C.query("adp_conv1d_ws_bytes", byref(d))
    if need > 0:  # split-K partial tiles (small grids: the deep layers at batch 1)
        ws = _ws(need, x)
        d.ws = ptr(ws)
    if gn is not None:
        E = _C.query("adp_conv1d_gn_entries", byref(d))
        if E > 0:
            gn.part = torch.empty((B, M // 4, E, 3), dtype=torch.float32, device=x.device)
            gn.of = out
            d.gn_part = ptr(gn.part)
    if gnb is not None and GNB_EPILOGUE:
        d.gnb_groups = gnb.groups
        d.gnb_x, d.gnb_stats, d.gnb_gamma, d.gnb_beta = ptr(gnb.x), ptr(gnb.stats), ptr(gnb.gamma), ptr(gnb.beta)
        E = _C.query("adp_conv1d_gnb_entries", byref(d))  # (some kernels look at the operands' alignment)
        if E > 0:
            gnb.ab = torch.empty((B, M, E, 2), dtype=torch.float32, device=x.device)
            d.gnb_ab = ptr(gnb.ab)
    if _C.PROFILE is not None:  # algorithmic work of this launch: A_in + A_out (+A_res) + weights
        _C.tag(flops=2 * B * M * N * R * KT,
               bytes=4 * (B * R * Lin + out.numel() + w.numel() + (res.numel() if res is not None else 0)),
               shape=f"B{B} R{R} M{M} N{N} KT{KT} s{stride} up{up} tr{int(transposed)} pro{prologue}")
    _C.call("adp_conv1d", byref(d), _C.stream())
    if _C.REPLAY is not None:
        keep = (x, x2, w, bias, pro_stats, pro_gamma, pro_beta, e_scale, res, out, out_pre, gn.part if gn is not None else None,
                (gnb.x, gnb.stats, gnb.gamma, gnb.beta, gnb.ab) if gnb is not None else None, ws if need > 0 else None)
        _C.REPLAY.append((f"B{B} R{R} M{M} N{N} KT{KT} s{stride} up{up} tr{int(transposed)} pro{prologue}",
                          4 * (B * R * Lin + out.numel() + w.numel() + (res.numel() if res is not None else 0)),
                          lambda d=d, keep=keep: _C.call("adp_conv1d", byref(d), _C.stream())))
    return out


class WgradPark:
    """Parked second stages of split weight gradients (adp_wgrad_desc.accumulate bit 1): the partial slices stay in their own
    scratch until flush() sums every parked gradient of one shape in ONE launch (adp_wgrad_reduce_batch) -- the ConvBlock
    convs of a U-Net depth share their shape, so a block side's four to eight second stages become one."""

    # whole weight-gradient CALLS are collected too (`calls`): small problems, where the inputs of a block side's gradients stay
    # in the Infinity Cache until the side is done, run as one launch per shape (adp_conv1d_wgrad_batch)
    # x + dy of one call; above it only the second stage is parked.  (Round 4: 24 MB, 40 / 80 within noise.  Round 5, with the
    # batch-aware position split of adp_conv1d_wgrad_batch -- an item of a batched launch takes 1/n of the lone split: 24 -> 40 ->
    # 80 MB 12.77 -> 12.72 -> 12.68 ms per step; 80 MB covers every layer of the README configuration)
    BATCH_BYTES = 80 << 20

    # flush() on a SIDE stream (ADP_WGRAD_SIDE=1): nothing downstream of a weight gradient is on the backward's critical path --
    # the data-gradient chain goes on while the batched launches run beside it (a branch of the captured graph), join() is where
    # somebody reads the gradients (the data-parallel hook, the end of the backward).  What the launches read stays referenced
    # until join(): freed on the main stream it could be handed to a later main-stream kernel while the side stream still reads it.
    SIDE = os.environ.get("ADP_WGRAD_SIDE", "0") != "0"
    _side_streams = {}

    def __init__(self):
        self.items = []  # (key = (partials, cnt, M, accumulate, has_bias), ws, dw, dbias)
        self.calls = []  # (shape key, WgradDesc, tensors kept alive)
        self.held = []   # what side-stream launches still read
        self.forked = None
        if "ADP_WGRAD_BATCH_MB" in os.environ:  # (A/B: 0 = only second stages are parked)
            self.BATCH_BYTES = int(os.environ["ADP_WGRAD_BATCH_MB"]) << 20

    def _fork(self, t: Tensor):
        if not (self.SIDE and t.is_cuda):
            return contextlib.nullcontext()
        side = self.forked
        if side is None:
            side = self._side_streams.get(t.device)
            if side is None:
                side = self._side_streams[t.device] = torch.cuda.Stream(device=t.device)
            self.forked = side
        side.wait_stream(torch.cuda.current_stream(t.device))  # (the inputs were produced on the main stream)
        return torch.cuda.stream(side)

    def join(self) -> None:
        """The main stream waits for the side-stream launches: gradients are final for whatever is enqueued next."""
        if self.forked is not None:
            torch.cuda.current_stream(self.forked.device).wait_stream(self.forked)
            self.forked = None
            self.held.clear()

    def add(self, key, ws: Tensor, dw: Tensor, dbias: Optional[Tensor]) -> None:
        self.items.append((key, ws, dw, dbias))

    def add_call(self, key, d: WgradDesc, keep) -> None:
        self.calls.append((key, d, keep))

    def flush(self) -> None:
        if not self.calls and not self.items:
            return
        with self._fork(self.calls[0][2][0] if self.calls else self.items[0][1]):
            self._flush()

    def _flush(self) -> None:
        if self.calls:
            groups = {}
            for key, d, keep in self.calls:
                groups.setdefault(key, []).append(d)
            calls, self.calls = self.calls, []
            for key, ds in groups.items():
                arr = (WgradDesc * len(ds))(*ds)
                if _C.PROFILE is not None:
                    B, R, _, Lin, M, N, KT = key[:7]
                    _C.tag(flops=2 * B * M * N * R * KT * len(ds), bytes=4 * len(ds) * (B * R * Lin + B * M * N + M * R * KT),
                           shape=f"n{len(ds)} B{B} R{R} M{M} N{N} KT{KT}")
                _C.call("adp_conv1d_wgrad_batch", arr, len(ds), _C.stream())
            if self.forked is not None:
                self.held.append(calls)
            del calls
        if not self.items:
            return
        groups = {}
        for key, ws, dw, dbias in self.items:
            groups.setdefault(key, []).append((ws, dw, dbias))
        if self.forked is not None:
            self.held.append(self.items)
        self.items = []
        for (partials, cnt, M, acc, has_bias), g in groups.items():
            n = len(g)
            arr = ctypes.c_void_p * n
            wsa, dwa = arr(*[ptr(t[0]) for t in g]), arr(*[ptr(t[1]) for t in g])
            dba = arr(*[ptr(t[2]) for t in g]) if has_bias else None
            _C.tag(bytes=4 * n * (partials + 1) * (cnt + M), shape=f"n{n} P{partials} cnt{cnt}")
            _C.call("adp_wgrad_reduce_batch", wsa, dwa, dba, n, partials, cnt, M, acc, _C.stream())


def conv1d_wgrad(x: Tensor, dy: Tensor, KT: int, *, stride: int = 1, dil: int = 1, pad: int = 0, up: int = 1,
                 x2: Optional[Tensor] = None, prologue: int = 0, pro_stats: Optional[Tensor] = None,
                 pro_gamma: Optional[Tensor] = None, pro_beta: Optional[Tensor] = None, groups: int = 1,
                 dw: Optional[Tensor] = None, dbias: Optional[Tensor] = None, want_bias: bool = True,
                 accumulate: bool = False, park: Optional[WgradPark] = None):
    B, R1, Lin = x.shape
    R = R1 + (x2.shape[1] if x2 is not None else 0)
    _, M, N = dy.shape
    if dw is None:
        dw = torch.empty((M, R, KT), dtype=torch.float32, device=x.device)
    if dbias is None and want_bias:
        dbias = torch.empty((M,), dtype=torch.float32, device=x.device)
    d = WgradDesc(ptr(x), ptr(x2), ptr(dy), ptr(pro_stats), ptr(pro_gamma), ptr(pro_beta), ptr(dw), ptr(dbias), None,
                  B, R, R1, Lin, M, N, KT, stride, dil, pad, up, prologue, groups, int(accumulate))
    ws = _ws(_C.query("adp_conv1d_wgrad_ws_bytes", byref(d)), x)
    d.ws = ptr(ws)
    if park is not None and x2 is None and 4 * (x.numel() + dy.numel()) <= park.BATCH_BYTES:
        # the whole call waits for park.flush(): one launch per shape with the block side's other gradients
        # (tagged there: a tag set here would ride on whatever profiled launch comes next)
        key = (B, R, R1, Lin, M, N, KT, stride, dil, pad, up, prologue, groups, int(accumulate), pro_stats is not None,
               pro_gamma is not None, pro_beta is not None, dbias is not None)
        park.add_call(key, d, (x, dy, pro_stats, pro_gamma, pro_beta, dw, dbias, ws))
        return dw, dbias
    if _C.PROFILE is not None:  # A_x + A_dy + weight-gradient write
        _C.tag(flops=2 * B * M * N * R * KT, bytes=4 * (B * R * Lin + dy.numel() + dw.numel()),
               shape=f"B{B} R{R} M{M} N{N} KT{KT} s{stride} up{up} pro{prologue}")
    if park is not None:
        partials = _C.query("adp_conv1d_wgrad_partials", byref(d))
        if partials > 1:  # the second stage waits for park.flush(); ws belongs to the parked item until then
            d.accumulate = int(accumulate) | 2
            park.add((partials, M * R * KT, M, int(accumulate), dbias is not None), ws, dw, dbias)
    _C.call("adp_conv1d_wgrad", byref(d), _C.stream())
    return dw, dbias


GNB_EPILOGUE = os.environ.get("ADP_GNB_EPILOGUE", "1") != "0"  # (A/B switch: 0 = the GroupNorm backward always runs its own first stage)


class GnBwdPart:
    """Names the SiLU(GroupNorm(x)) behind a data-gradient conv (x, its statistics and affine parameters); after the conv,
    `ab` [B, C, E, 2] holds the first stage of that GroupNorm backward if the conv's epilogue produced it (adp_conv_desc.gnb_ab)."""
    __slots__ = ("x", "stats", "gamma", "beta", "groups", "ab")

    def __init__(self, x: Tensor, stats: Tensor, gamma: Tensor, beta: Tensor, groups: int):
        self.x, self.stats, self.gamma, self.beta, self.groups = x, stats, gamma, beta, groups
        self.ab: Optional[Tensor] = None


class GnPart:
    """GroupNorm partial statistics [B, C/4, E, 3] = (mean, M2, count) per slice of a 4-channel row quad, written by
    the kernel that PRODUCED tensor `of` (conv epilogue), so that the consuming GroupNorm needs no pass of its own."""
    __slots__ = ("part", "of")

    def __init__(self):
        self.part: Optional[Tensor] = None
        self.of: Optional[Tensor] = None

    def covers(self, x: Tensor) -> bool:
        return self.part is not None and self.of is x


def gn_finalize(part: Tensor, groups: int, eps: float = GN_EPS) -> Tensor:
    """stats [B, G, 2] from producer-side partials (adp_gn_finalize)."""
    B, CQ, E, _ = part.shape
    C = CQ * 4
    stats = torch.empty((B, groups, 2), dtype=torch.float32, device=part.device)
    _C.tag(bytes=4 * part.numel(), shape=f"B{B} C{C} E{E}")
    _C.call("adp_gn_finalize", ptr(part), B, C, E, groups, eps, ptr(stats), _C.stream())
    return stats


def gn_finalize_act(x: Tensor, part: Tensor, groups: int, gamma: Tensor, beta: Tensor, eps: float = GN_EPS):
    """(stats, SiLU(GroupNorm(x))) from producer-side partials in one launch (adp_gn_finalize_act)."""
    B, C, L = x.shape
    E = part.shape[2]
    stats = torch.empty((B, groups, 2), dtype=torch.float32, device=x.device)
    act = torch.empty_like(x)
    _C.tag(bytes=8 * x.numel(), shape=f"B{B} C{C} L{L} E{E}")
    _C.call("adp_gn_finalize_act", ptr(x), ptr(part), B, C, L, E, groups, eps, ptr(gamma), ptr(beta), ptr(stats),
            ptr(act), _C.stream())
    return stats, act


def gn_act(x: Tensor, stats: Tensor, groups: int, gamma: Tensor, beta: Tensor) -> Tensor:
    """SiLU(GroupNorm(x)) materialised from finished statistics (adp_gn_act)."""
    B, C, L = x.shape
    act = torch.empty_like(x)
    _C.tag(bytes=8 * x.numel(), shape=f"B{B} C{C} L{L}")
    _C.call("adp_gn_act", ptr(x), ptr(stats), ptr(gamma), ptr(beta), B, C, L, groups, ptr(act), _C.stream())
    return act


def gn_stats(x: Tensor, groups: int, eps: float = GN_EPS, out: Optional[Tensor] = None) -> Tensor:
    B, C, L = x.shape
    stats = out if out is not None else torch.empty((B, groups, 2), dtype=torch.float32, device=x.device)
    ws = _ws(_C.query("adp_gn_stats_ws_bytes", B, C, L, groups), x)
    _C.tag(bytes=4 * x.numel(), shape=f"B{B} C{C} L{L}")
    _C.call("adp_gn_stats", ptr(x), B, C, L, groups, eps, ptr(stats), ptr(ws), _C.stream())
    return stats


def gn_stats_act(x: Tensor, groups: int, gamma: Tensor, beta: Tensor, eps: float = GN_EPS):
    """(stats [B, G, 2], act = SiLU(GroupNorm(x)) materialised) in two launches (adp_gn_stats_act)."""
    B, C, L = x.shape
    stats = torch.empty((B, groups, 2), dtype=torch.float32, device=x.device)
    act = torch.empty_like(x)
    ws = _ws(_C.query("adp_gn_stats_ws_bytes", B, C, L, groups), x)
    _C.tag(bytes=12 * x.numel(), shape=f"B{B} C{C} L{L}")
    _C.call("adp_gn_stats_act", ptr(x), B, C, L, groups, eps, ptr(gamma), ptr(beta), ptr(stats), ptr(act), ptr(ws),
            _C.stream())
    return stats, act


def gn_silu_bwd(x: Tensor, dact: Tensor, stats: Tensor, gamma: Tensor, beta: Tensor, groups: int,
                dres: Optional[Tensor] = None, dx: Optional[Tensor] = None, dgamma: Optional[Tensor] = None,
                dbeta: Optional[Tensor] = None, accumulate: bool = False, ab: Optional[Tensor] = None):
    """Backward of SiLU(GroupNorm(x)): returns (dx [+ dres], dgamma, dbeta).  `ab` [B, C, E, 2]: the first stage, already
    left by the epilogue of the conv that produced dact (GnBwdPart.ab): one launch instead of two."""
    B, C, L = x.shape
    if dx is None:
        dx = torch.empty_like(x)
    if dgamma is None:
        dgamma = torch.empty_like(gamma)
    if dbeta is None:
        dbeta = torch.empty_like(beta)
    s = _C.stream()
    NS = _C.query("adp_row_nsplit", B * C, L)
    if ab is not None:
        _C.tag(bytes=(12 + (4 if dres is not None else 0)) * x.numel(), shape=f"B{B} C{C} L{L}")
        _C.call("adp_gn_silu_bwd_apply_ab", ptr(x), ptr(dact), ptr(stats), ptr(gamma), ptr(beta), ptr(ab), ptr(dres), B, C,
                L, groups, NS, ab.shape[2], ptr(dx), ptr(dgamma), ptr(dbeta), int(accumulate), s)
        return dx, dgamma, dbeta
    ab = torch.empty((B, C, NS, 2), dtype=torch.float32, device=x.device)
    _C.tag(bytes=8 * x.numel(), shape=f"B{B} C{C} L{L}")
    _C.call("adp_gn_silu_bwd_reduce", ptr(x), ptr(dact), ptr(stats), ptr(gamma), ptr(beta), B, C, L, groups, NS,
            ptr(ab), s)
    _C.tag(bytes=(12 + (4 if dres is not None else 0)) * x.numel(), shape=f"B{B} C{C} L{L}")
    _C.call("adp_gn_silu_bwd_apply", ptr(x), ptr(dact), ptr(stats), ptr(gamma), ptr(beta), ptr(ab), ptr(dres), B, C,
            L, groups, NS, ptr(dx), ptr(dgamma), ptr(dbeta), int(accumulate), s)
    return dx, dgamma, dbeta


def modulation_fwd(x: Tensor, ss: Tensor, ss_bstride: int, eps: float = MODULATION_LN_EPS, y: Optional[Tensor] = None,
                   stats: Optional[Tensor] = None):
    """ss: 1-D view whose element [b*ss_bstride + c] is scale and [b*ss_bstride + C + c] is shift."""
    B, C, L = x.shape
    if y is None:
        y = torch.empty_like(x)
    if stats is None:
        stats = torch.empty((B, L, 2), dtype=torch.float32, device=x.device)
    _C.tag(bytes=8 * x.numel(), shape=f"B{B} C{C} L{L}")
    _C.call("adp_modulation_fwd", ptr(x), ptr(ss), ss_bstride, B, C, L, eps, ptr(y), ptr(stats), _C.stream())
    return y, stats


def modulation_ln_fwd(x: Tensor, ss: Tensor, ss_bstride: int, gamma: Tensor, beta: Tensor, gamma2: Optional[Tensor] = None,
                      beta2: Optional[Tensor] = None, eps: float = MODULATION_LN_EPS, eps_ln: float = ATTENTION_LN_EPS):
    """ModulationItem + the LayerNorm(s) of the attention item behind it in one launch (adp_modulation_ln_fwd):
    (y, stats) as modulation_fwd, (xn, xn2 or None, ln_stats) as ln_affine_fwd(y, gamma, beta, gamma2, beta2)."""
    B, C, L = x.shape
    y, xn = torch.empty_like(x), torch.empty_like(x)
    xn2 = torch.empty_like(x) if gamma2 is not None else None
    stats = torch.empty((B, L, 2), dtype=torch.float32, device=x.device)
    ln_stats = torch.empty((B, L, 2), dtype=torch.float32, device=x.device)
    _C.tag(bytes=4 * x.numel() * (4 if xn2 is not None else 3), shape=f"B{B} C{C} L{L}")
    _C.call("adp_modulation_ln_fwd", ptr(x), ptr(ss), ss_bstride, B, C, L, eps, ptr(y), ptr(stats), eps_ln, ptr(gamma),
            ptr(beta), ptr(xn), ptr(gamma2), ptr(beta2), ptr(xn2), ptr(ln_stats), _C.stream())
    return y, stats, xn, xn2, ln_stats


def modulation_bwd(x: Tensor, dy: Tensor, ss: Tensor, ss_bstride: int, stats: Tensor, dss: Tensor, dss_bstride: int,
                   dx: Optional[Tensor] = None) -> Tensor:
    B, C, L = x.shape
    if dx is None:
        dx = torch.empty_like(x)
    ws = _ws(_C.query("adp_chan_ln_bwd_ws_bytes", B, C, L), x)
    _C.tag(bytes=12 * x.numel(), shape=f"B{B} C{C} L{L}")
    _C.call("adp_modulation_bwd", ptr(x), ptr(dy), ptr(ss), ss_bstride, ptr(stats), B, C, L, ptr(dx), ptr(dss),
            dss_bstride, ptr(ws), _C.stream())
    return dx


class ModulationSums:
    """Parked second stages of Modulation backwards (adp_modulation_bwd_partial / _reduce): the per-tile channel sums of
    each backward stay in its workspace until `flush`, which sums every parked item whose scale / shift gradient slice
    lies in [lo, hi) of the conditioning-bank row -- the items of one U-Net depth, which share their shape -- in one
    launch per eight."""

    def __init__(self):
        self.items = []  # (offset into the bank row, ws, dss view, B, C, NT, dss_bstride)

    def partial(self, off: int, x: Tensor, dy: Tensor, ss: Tensor, ss_bstride: int, stats: Tensor, dss: Tensor,
                dss_bstride: int) -> Tensor:
        B, C, L = x.shape
        dx = torch.empty_like(x)
        ws = _ws(_C.query("adp_chan_ln_bwd_ws_bytes", B, C, L), x)
        _C.tag(bytes=12 * x.numel(), shape=f"B{B} C{C} L{L}")
        NT = _C.call_value("adp_modulation_bwd_partial", ptr(x), ptr(dy), ptr(ss), ss_bstride, ptr(stats), B, C, L, ptr(dx),
                           ptr(ws), _C.stream())
        self.items.append((off, ws, dss, B, C, NT, dss_bstride))
        return dx

    def partial_ln(self, off: int, x: Tensor, ss: Tensor, ss_bstride: int, stats: Tensor, dss: Tensor, dss_bstride: int,
                   y: Tensor, dxn: Tensor, gamma: Tensor, ln_stats: Tensor, dres: Optional[Tensor], dgb: Tensor) -> Tensor:
        """`partial` for a ModulationItem whose output y went through an attention item's LayerNorm (gamma, ln_stats): the
        LayerNorm's backward of d(xn) (+ dres) and this item's backward in one pass (adp_modulation_ln_bwd_partial);
        dgb = the LayerNorm's [dgamma | dbeta] destination."""
        B, C, L = x.shape
        dx = torch.empty_like(x)
        nbytes = _C.query("adp_chan_ln_bwd_ws_bytes", B, C, L)
        ws, ws_ln = _ws(nbytes, x), _ws(nbytes, x)
        _C.tag(bytes=16 * x.numel(), shape=f"B{B} C{C} L{L}")
        NT = _C.call_value("adp_modulation_ln_bwd_partial", ptr(x), ptr(ss), ss_bstride, ptr(stats), ptr(y), ptr(dxn),
                           ptr(gamma), ptr(ln_stats), ptr(dres), B, C, L, 0, ptr(dx), ptr(ws), ptr(dgb), ptr(ws_ln),
                           _C.stream())
        self.items.append((off, ws, dss, B, C, NT, dss_bstride))
        return dx

    def flush(self, lo: Optional[int] = None, hi: Optional[int] = None) -> None:
        take = [it for it in self.items if lo is None or lo <= it[0] < hi]
        if not take:
            return
        self.items = [it for it in self.items if not (lo is None or lo <= it[0] < hi)]
        groups = {}
        for it in take:
            groups.setdefault(it[3:], []).append(it)
        for (B, C, NT, bstride), its in groups.items():
            n = len(its)
            wsp = (ctypes.c_void_p * n)(*[ptr(it[1]) for it in its])
            dsp = (ctypes.c_void_p * n)(*[ptr(it[2]) for it in its])
            _C.call("adp_modulation_bwd_reduce", wsp, dsp, n, B, C, NT, bstride, _C.stream())


def ln_stats(x: Tensor, eps: float = ATTENTION_LN_EPS) -> Tensor:
    B, C, L = x.shape
    stats = torch.empty((B, L, 2), dtype=torch.float32, device=x.device)
    _C.call("adp_ln_stats", ptr(x), B, C, L, eps, ptr(stats), _C.stream())
    return stats


def ln_affine_fwd(x: Tensor, gamma: Tensor, beta: Tensor, gamma2: Optional[Tensor] = None,
                  beta2: Optional[Tensor] = None, eps: float = ATTENTION_LN_EPS):
    """(y, y2 or None, stats): y = LayerNorm_C(x) * gamma + beta, y2 likewise with (gamma2, beta2), stats [B, L, 2]."""
    B, C, L = x.shape
    y = torch.empty_like(x)
    y2 = torch.empty_like(x) if gamma2 is not None else None
    stats = torch.empty((B, L, 2), dtype=torch.float32, device=x.device)
    _C.tag(bytes=4 * x.numel() * (3 if y2 is not None else 2), shape=f"B{B} C{C} L{L}")
    _C.call("adp_ln_affine_fwd", ptr(x), B, C, L, eps, ptr(gamma), ptr(beta), ptr(y), ptr(gamma2), ptr(beta2), ptr(y2),
            ptr(stats), _C.stream())
    return y, y2, stats


def ln_bwd(x: Tensor, dxn: Tensor, stats: Tensor, gamma: Tensor, dres: Optional[Tensor] = None,
           dgb: Optional[Tensor] = None, accumulate: bool = False):
    """Backward of LayerNorm-over-channels with affine: returns (dx [+ dres], [dgamma | dbeta])."""
    B, C, L = x.shape
    dx = torch.empty_like(x)
    if dgb is None:
        dgb = torch.empty((2 * C,), dtype=torch.float32, device=x.device)
    ws = _ws(_C.query("adp_chan_ln_bwd_ws_bytes", B, C, L), x)
    _C.call("adp_ln_bwd", ptr(x), ptr(dxn), ptr(stats), ptr(gamma), ptr(dres), B, C, L, int(accumulate), ptr(dx),
            ptr(dgb), ptr(ws), _C.stream())
    return dx, dgb


LIN_ROWS = 16  # activation rows one adp_linear_* launch holds in LDS (LIN_BMAX in csrc/linear.hip)


def linear_fwd(x: Tensor, w: Tensor, bias: Optional[Tensor], act: int = 0, post: int = 0,
               y: Optional[Tensor] = None) -> Tensor:
    B, K = x.shape
    N = w.shape[0]
    if y is None:
        y = torch.empty((B, N), dtype=torch.float32, device=x.device)
    _C.tag(bytes=4 * (w.numel() + x.numel() + y.numel()), shape=f"B{B} K{K} N{N}")
    for b0 in range(0, B, LIN_ROWS):  # batches beyond 16 rows: the weight matrix is streamed once per 16 rows
        nb = min(LIN_ROWS, B - b0)
        _C.call("adp_linear_fwd", ptr(x[b0:b0 + nb]), ptr(w), ptr(bias), nb, K, N, act, post, ptr(y[b0:b0 + nb]), N,
                _C.stream())
    return y


def linear_bwd_data(dy: Tensor, w: Tensor, dxa: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    B, N = dy.shape
    K = w.shape[1]
    if dxa is None:
        dxa = torch.empty((B, K), dtype=torch.float32, device=dy.device)
    ws = _ws(_C.query("adp_linear_bwd_data_ws_bytes", min(B, LIN_ROWS), K, N), dy)
    _C.tag(bytes=4 * (w.numel() + B * N + dxa.numel()), shape=f"B{B} K{K} N{N}")
    for b0 in range(0, B, LIN_ROWS):
        nb = min(LIN_ROWS, B - b0)
        _C.call("adp_linear_bwd_data", ptr(dy[b0:b0 + nb]), N, ptr(w), nb, K, N, int(accumulate),
                ptr(dxa[b0:b0 + nb]), ptr(ws), _C.stream())
    return dxa


def linear_bwd_weight(dy: Tensor, x: Tensor, act: int = 0, dw: Optional[Tensor] = None,
                      dbias: Optional[Tensor] = None, want_bias: bool = True, accumulate: bool = False,
                      rows: Optional[int] = None, dy_bstride: Optional[int] = None):
    """dy [B, N]; or, with `rows`, a 1-D view whose element [b*dy_bstride + n] is dy[b, n] for n < rows (a column
    slice of a wider table, e.g. one depth's rows of the conditioning bank)."""
    if rows is None:
        B, N = dy.shape
        dy_bstride = N
        dy = dy.reshape(-1)
    else:
        B, N = x.shape[0], rows
    K = x.shape[1]
    if dw is None:
        dw = torch.empty((N, K), dtype=torch.float32, device=dy.device)
    if dbias is None and want_bias:
        dbias = torch.empty((N,), dtype=torch.float32, device=dy.device)
    _C.tag(bytes=4 * (dw.numel() + B * N + x.numel()), shape=f"B{B} K{K} N{N}")
    for b0 in range(0, B, LIN_ROWS):  # the second and later groups of 16 rows accumulate into dw / dbias
        nb = min(LIN_ROWS, B - b0)
        _C.call("adp_linear_bwd_weight", ptr(dy[b0 * dy_bstride:]), dy_bstride, ptr(x[b0:b0 + nb]), nb, K, N, act,
                int(accumulate or b0 > 0), ptr(dw), ptr(dbias), _C.stream())
    return dw, dbias


def time_fourier_fwd(t: Tensor, w: Tensor) -> Tensor:
    B, H = t.shape[0], w.shape[0]
    four = torch.empty((B, 2 * H + 1), dtype=torch.float32, device=t.device)
    _C.call("adp_time_fourier_fwd", ptr(t), ptr(w), B, H, ptr(four), _C.stream())
    return four


def time_fourier_bwd(t: Tensor, w: Tensor, dfour: Tensor, dw: Optional[Tensor] = None,
                     accumulate: bool = False) -> Tensor:
    B, H = t.shape[0], w.shape[0]
    if dw is None:
        dw = torch.empty_like(w)
    _C.call("adp_time_fourier_bwd", ptr(t), ptr(w), ptr(dfour), B, H, int(accumulate), ptr(dw), _C.stream())
    return dw


def act_fwd(x: Tensor, act: int) -> Tensor:
    y = torch.empty_like(x)
    _C.call("adp_act_fwd", ptr(x), x.numel(), act, ptr(y), _C.stream())
    return y


def act_bwd(x: Tensor, dy: Tensor, act: int, dx: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    if dx is None:
        dx = torch.empty_like(x)
    _C.call("adp_act_bwd", ptr(x), ptr(dy), x.numel(), act, int(accumulate), ptr(dx), _C.stream())
    return dx


def skipmod_bwd(g: Tensor, x: Tensor, scale: Tensor, scale_bstride: int, dscale: Tensor, dscale_bstride: int,
                dx: Optional[Tensor] = None) -> Tensor:
    B, C, L = x.shape
    if dx is None:
        dx = torch.empty_like(x)
    ws = _ws(_C.query("adp_skipmod_bwd_ws_bytes", B, C, L), x)
    _C.tag(bytes=12 * x.numel(), shape=f"B{B} C{C} L{L}")
    _C.call("adp_skipmod_bwd", ptr(g), ptr(x), ptr(scale), scale_bstride, B, C, L, ptr(dx), ptr(dscale),
            dscale_bstride, ptr(ws), _C.stream())
    return dx


def v_noise(x: Tensor, noise: Tensor, sigma: Tensor):
    B = x.shape[0]
    per = x.numel() // B
    x_noisy, v_target = torch.empty_like(x), torch.empty_like(x)
    _C.call("adp_v_noise", ptr(x), ptr(noise), ptr(sigma), B, per, ptr(x_noisy), ptr(v_target), _C.stream())
    return x_noisy, v_target


def mse_fwd(v_pred: Tensor, v_target: Tensor) -> Tensor:
    n = v_pred.numel()
    loss = torch.empty((), dtype=torch.float32, device=v_pred.device)
    ws = _ws(_C.query("adp_mse_ws_bytes", n), v_pred)
    _C.call("adp_mse_fwd", ptr(v_pred), ptr(v_target), n, ptr(loss), ptr(ws), _C.stream())
    return loss


def mse_bwd(v_pred: Tensor, v_target: Tensor, gloss: Optional[Tensor]) -> Tensor:
    dv = torch.empty_like(v_pred)
    _C.call("adp_mse_bwd", ptr(v_pred), ptr(v_target), ptr(gloss), v_pred.numel(), ptr(dv), _C.stream())
    return dv


def _stft_res(res) -> ctypes.Array:
    """(N, hop, win) triples -> the host int64 array adp_stft_loss_* read at the call."""
    flat = [int(v) for triple in res for v in triple]
    return (ctypes.c_int64 * len(flat))(*flat)


def stft_loss_fwd(x: Tensor, y: Tensor, res, w_sc: float, w_log: float, w_lin: float, eps: float):
    """Multi-resolution STFT loss of x against y ([..., L] rows); returns (loss, forward workspace for stft_loss_bwd)."""
    L = x.shape[-1]
    rows, arr = x.numel() // L, _stft_res(res)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    ws = _ws(_C.query("adp_stft_loss_ws_bytes", rows, L, len(res), arr, 0), x)
    _C.call("adp_stft_loss_fwd", ptr(x), ptr(y), rows, L, len(res), arr, w_sc, w_log, w_lin, eps, ptr(loss), ptr(ws),
            _C.stream())
    return loss, ws


def stft_loss_bwd(x: Tensor, y: Tensor, gloss: Optional[Tensor], ws_fwd: Tensor, res, w_sc: float, w_log: float,
                  w_lin: float, eps: float) -> Tensor:
    L = x.shape[-1]
    rows, arr = x.numel() // L, _stft_res(res)
    dx = torch.empty_like(x)
    ws = _ws(_C.query("adp_stft_loss_ws_bytes", rows, L, len(res), arr, 1), x)
    _C.call("adp_stft_loss_bwd", ptr(x), ptr(y), ptr(gloss), ptr(ws_fwd), rows, L, len(res), arr, w_sc, w_log, w_lin, eps,
            ptr(dx), ptr(ws), _C.stream())
    return dx


def _spec_bins(res, n_bins) -> ctypes.Array:
    """Filters per resolution (None: no filterbank) -> the host int64 array adp_spec_loss_* read at the call."""
    return (ctypes.c_int64 * len(res))(*([0] * len(res) if n_bins is None else [int(v) for v in n_bins]))


def spec_loss_fwd(x: Tensor, y: Tensor, pair: bool, res, n_bins, fb: Optional[Tensor], mel_range: Optional[Tensor],
                  w_sc: float, w_log: float, w_lin: float, eps: float, w_sum: float = 1.0, w_diff: float = 1.0):
    """adp_spec.h: the grouped / mel-scaled STFT loss of x against y ([..., L] rows; with `pair` consecutive rows are the two
    channels of an item); returns (loss, forward workspace for spec_loss_bwd)."""
    L = x.shape[-1]
    rows, arr, bins = x.numel() // L, _stft_res(res), _spec_bins(res, n_bins)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    ws = _ws(_C.query("adp_spec_loss_ws_bytes", rows, L, int(pair), len(res), arr, bins, 0), x)
    _C.call("adp_spec_loss_fwd", ptr(x), ptr(y), rows, L, int(pair), len(res), arr, bins, ptr(fb),
            ptr(mel_range, torch.int32), w_sc, w_log, w_lin, eps, w_sum, w_diff, ptr(loss), ptr(ws), _C.stream())
    return loss, ws


def spec_loss_bwd(x: Tensor, y: Tensor, gloss: Optional[Tensor], ws_fwd: Tensor, pair: bool, res, n_bins,
                  fb: Optional[Tensor], mel_range: Optional[Tensor], bin_range: Optional[Tensor], w_sc: float, w_log: float,
                  w_lin: float, eps: float, w_sum: float = 1.0, w_diff: float = 1.0) -> Tensor:
    L = x.shape[-1]
    rows, arr, bins = x.numel() // L, _stft_res(res), _spec_bins(res, n_bins)
    dx = torch.empty_like(x)
    ws = _ws(_C.query("adp_spec_loss_ws_bytes", rows, L, int(pair), len(res), arr, bins, 1), x)
    _C.call("adp_spec_loss_bwd", ptr(x), ptr(y), ptr(gloss), ptr(ws_fwd), rows, L, int(pair), len(res), arr, bins, ptr(fb),
            ptr(mel_range, torch.int32), ptr(bin_range, torch.int32), w_sc, w_log, w_lin, eps, w_sum, w_diff, ptr(dx),
            ptr(ws), _C.stream())
    return dx


def spec_fir(x: Tensor, taps: Tensor) -> Tensor:
    """adp_spec_fir: every [..., L] row of x filtered by the odd-length taps, zero padded (F.conv1d(row, taps, padding=T // 2));
    the adjoint is the call with the taps reversed."""
    L = x.shape[-1]
    out = torch.empty_like(x)
    _C.call("adp_spec_fir", ptr(x), ptr(taps), x.numel() // L if L else 0, L, taps.numel(), ptr(out), _C.stream())
    return out


def v_step(x: Tensor, v: Tensor, ab4: Tensor, out: Optional[Tensor] = None) -> Tensor:
    if out is None:
        out = torch.empty_like(x)
    _C.call("adp_v_step", ptr(x), ptr(v), ptr(ab4), x.numel(), ptr(out), _C.stream())
    return out


def v_step2(x: Tensor, v: Tensor, hist_x0: Tensor, hist_eps: Tensor, coef6: Tensor, out: Optional[Tensor] = None,
            hist_x0_out: Optional[Tensor] = None, hist_eps_out: Optional[Tensor] = None):
    """One second-order multistep sampler update (adp_v_step2): returns (x_next, x0, eps).  Each output may be its input
    (out=x, hist_x0_out=hist_x0, hist_eps_out=hist_eps); a coef6 row with ca = cb = 0 does not read the history."""
    n = x.numel()
    for t in (v, hist_x0, hist_eps, out, hist_x0_out, hist_eps_out):
        if t is not None and t.numel() != n:
            raise ValueError(f"v_step2: every tensor must have x's {n} elements; got {t.numel()}")
    if coef6.numel() != 6:
        raise ValueError(f"v_step2: coef6 holds (a0, b0, a1, b1, ca, cb); got {coef6.numel()} values")
    if out is None:
        out = torch.empty_like(x)
    if hist_x0_out is None:
        hist_x0_out = torch.empty_like(x)
    if hist_eps_out is None:
        hist_eps_out = torch.empty_like(x)
    _C.call("adp_v_step2", ptr(x), ptr(v), ptr(hist_x0), ptr(hist_eps), ptr(coef6), n, ptr(out), ptr(hist_x0_out),
            ptr(hist_eps_out), _C.stream())
    return out, hist_x0_out, hist_eps_out


def _arv_dims(what: str, x: Tensor, N: int):
    if x.dim() != 3:
        raise ValueError(f"{what}: x must be [B, C, T]; got {tuple(x.shape)}")
    B, C, T = x.shape
    if N < 1 or T % N != 0:
        raise ValueError(f"{what}: the length {T} must be divisible by num_splits={N}")
    return B, C, T


def arv_noise(x: Tensor, noise: Tensor, sigma: Tensor):
    """ARVDiffusion's noising (adp_arv_noise): x, noise [B, C, T], sigma [B, N] (one level per batch row and split) ->
    (x_noisy, v_target, sigma_plane [B, 1, T])."""
    if sigma.dim() != 2 or sigma.shape[0] != x.shape[0]:
        raise ValueError(f"arv_noise: sigma must be [B, num_splits]; got {tuple(sigma.shape)} for x {tuple(x.shape)}")
    N = sigma.shape[1]
    B, C, T = _arv_dims("arv_noise", x, N)
    if noise.shape != x.shape:
        raise ValueError(f"arv_noise: noise must have x's shape {tuple(x.shape)}; got {tuple(noise.shape)}")
    x_noisy, v_target = torch.empty_like(x), torch.empty_like(x)
    plane = torch.empty((B, 1, T), dtype=torch.float32, device=x.device)
    _C.call("adp_arv_noise", ptr(x), ptr(noise), ptr(sigma), B, C, T, N, ptr(x_noisy), ptr(v_target), ptr(plane),
            _C.stream())
    return x_noisy, v_target, plane


def arv_step(x: Tensor, v: Tensor, coef: Tensor, out: Optional[Tensor] = None, plane_out: Optional[Tensor] = None) -> Tensor:
    """One ARVSampler update (adp_arv_step): coef [N, 5] holds (a_i, b_i, a_{i+1}, b_{i+1}, sigma_{i+1}) per split.  `out`
    may be x; `plane_out` ([B, 1, T] or [B, T]), when given, receives the next step's sigma plane."""
    if coef.dim() != 2 or coef.shape[1] != 5:
        raise ValueError(f"arv_step: coef must be [num_splits, 5]; got {tuple(coef.shape)}")
    N = coef.shape[0]
    B, C, T = _arv_dims("arv_step", x, N)
    for t in (v, out):
        if t is not None and t.shape != x.shape:
            raise ValueError(f"arv_step: v and out must have x's shape {tuple(x.shape)}; got {tuple(t.shape)}")
    if plane_out is not None and plane_out.numel() != B * T:
        raise ValueError(f"arv_step: plane_out must hold B * T = {B * T} values; got {plane_out.numel()}")
    if out is None:
        out = torch.empty_like(x)
    _C.call("adp_arv_step", ptr(x), ptr(v), ptr(coef), B, C, T, N, ptr(out), ptr(plane_out), _C.stream())
    return out


def arv_plane(sigma: Tensor, B: int, T: int, out: Optional[Tensor] = None) -> Tensor:
    """sigma [N] -> sigma plane [B, 1, T] with plane[b, 0, t] = sigma[t // (T // N)] (adp_arv_plane)."""
    if sigma.dim() != 1:
        raise ValueError(f"arv_plane: sigma must be [num_splits]; got {tuple(sigma.shape)}")
    N = sigma.shape[0]
    if B < 1 or T < 1 or N < 1 or T % N != 0:
        raise ValueError(f"arv_plane: B={B} and T={T} must be positive and T divisible by num_splits={N}")
    if out is None:
        out = torch.empty((B, 1, T), dtype=torch.float32, device=sigma.device)
    elif out.numel() != B * T:
        raise ValueError(f"arv_plane: out must hold B * T = {B * T} values; got {out.numel()}")
    _C.call("adp_arv_plane", ptr(sigma), B, T, N, ptr(out), _C.stream())
    return out


def v_inpaint_step(x: Tensor, v: Tensor, source: Tensor, noise: Tensor, mask_u8: Tensor, ab4: Tensor,
                   out: Optional[Tensor] = None) -> Tensor:
    if out is None:
        out = torch.empty_like(x)
    _C.call("adp_v_inpaint_step", ptr(x), ptr(v), ptr(source), ptr(noise), ptr(mask_u8, torch.uint8), ptr(ab4),
            x.numel(), ptr(out), _C.stream())
    return out


# ---- include/adp_rng.h: Philox4x32-10 normals from a device (seed, draw) row

def rng_rows(seed: int, draws) -> Tensor:
    """HOST int32 table [len(draws), 4] of rows (seed_lo, seed_hi, draw, 0): the bit patterns of the uint32 words the kernels
    read (torch has no arithmetic on uint32; the kernels take the words as they are).  seed < 2^64, each draw < 2^32."""
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"rng_rows: seed must be in [0, 2^64); got {seed}")
    rows = []
    for d in draws:
        d = int(d)
        if not 0 <= d < 1 << 32:
            raise ValueError(f"rng_rows: draw must be in [0, 2^32); got {d}")
        rows.append([seed & 0xFFFFFFFF, seed >> 32, d, 0])
    words = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)
    return torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32)


def _rng_row_ptr(what: str, rng4: Tensor):
    if rng4.dtype != torch.int32 or rng4.numel() != 4:
        raise ValueError(f"{what}: rng4 must be four int32 words (seed_lo, seed_hi, draw, 0); got {rng4.dtype} "
                         f"{tuple(rng4.shape)}")
    return ptr(rng4, torch.int32)


def philox_bits(n_words: int, rng4: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """The first n_words words of the row's Philox4x32-10 stream (adp_philox_bits) as int32 bit patterns."""
    row = _rng_row_ptr("philox_bits", rng4)
    if out is None:
        out = torch.empty(int(n_words), dtype=torch.int32, device=rng4.device)
    elif out.numel() != n_words:
        raise ValueError(f"philox_bits: out must hold {n_words} words; got {out.numel()}")
    _C.call("adp_philox_bits", row, int(n_words), ptr(out, torch.int32), _C.stream())
    return out


def randn(shape_like, rng4: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """N(0, 1) values of the row's stream in the shape of `shape_like` (a tensor, or a shape on rng4's device), element i of
    the flattened tensor being normal i of the stream (adp_randn).  The same row gives the same values on every backend."""
    row = _rng_row_ptr("randn", rng4)
    shape = tuple(shape_like.shape) if isinstance(shape_like, Tensor) else tuple(int(s) for s in shape_like)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=rng4.device)
    elif tuple(out.shape) != shape:
        raise ValueError(f"randn: out must have shape {shape}; got {tuple(out.shape)}")
    _C.call("adp_randn", row, out.numel(), ptr(out), _C.stream())
    return out


def v_inpaint_step_rng(x: Tensor, v: Tensor, source: Tensor, mask_u8: Tensor, ab4: Tensor, rng4: Tensor,
                       out: Optional[Tensor] = None) -> Tensor:
    """`v_inpaint_step` whose noise is the row's stream, formed in registers (adp_v_inpaint_step_rng).  `out` may be x."""
    row = _rng_row_ptr("v_inpaint_step_rng", rng4)
    for name, t in (("v", v), ("source", source), ("mask", mask_u8), ("out", out)):
        if t is not None and t.shape != x.shape:
            raise ValueError(f"v_inpaint_step_rng: {name} must have x's shape {tuple(x.shape)}; got {tuple(t.shape)}")
    if out is None:
        out = torch.empty_like(x)
    _C.call("adp_v_inpaint_step_rng", ptr(x), ptr(v), ptr(source), ptr(mask_u8, torch.uint8), ptr(ab4), row, x.numel(),
            ptr(out), _C.stream())
    return out


# ---- include/adp_clip.h: dynamic thresholding (per-item quantile scale, clip, thresholded sampler step)

CLIP_MAX_PER = 1 << 24  # per - 1 is exact in float32 up to here (torch.quantile's own limit)


def _item_dims(what: str, x, max_per: Optional[int] = None) -> Tuple[int, int]:
    """(rows, per) of a [B, ...] batch, from its shape alone (nothing is read or launched before the checks pass).
    max_per: the quantile's cap on the values of one item."""
    shape = tuple(int(s) for s in x.shape)
    if len(shape) < 1:
        raise ValueError(f"{what}: x must be [B, ...]; got a scalar")
    rows, per = shape[0], 1
    for s in shape[1:]:
        per *= s
    if max_per is not None and per > max_per:
        raise ValueError(f"{what}: {per} values per item; the quantile is defined for at most 2**24 = {max_per}")
    return rows, per


def _check_clip(what: str, clip, scale, rows: int) -> None:
    """The clip / scale arguments of a sampler update: clip is a bool, and a scale needs it and holds one value per item."""
    if not isinstance(clip, bool):
        raise ValueError(f"{what}: clip must be a bool; got {clip!r}")
    if scale is not None:
        if not clip:
            raise ValueError(f"{what}: a scale needs clip=True")
        if scale.numel() != rows:
            raise ValueError(f"{what}: scale must hold one value per item ({rows}); got {scale.numel()}")


def _check_like(what: str, x: Tensor, x_name: str = "x", **tensors) -> None:
    """Every named tensor that is given has x's shape."""
    for name, t in tensors.items():
        if t is not None and t.shape != x.shape:
            raise ValueError(f"{what}: {name} must have {x_name}'s shape {tuple(x.shape)}; got {tuple(t.shape)}")


def _check_f32(what: str, t: Tensor, n: int, holds: str) -> None:
    """t holds n float32 values; `holds` names it and them."""
    if t.dtype != torch.float32 or t.numel() != n:
        raise ValueError(f"{what}: {holds}; got {t.dtype} {tuple(t.shape)}")


def _check_order(what: str, order, clip, scale, rows: int, hist, hist_out) -> None:
    """order is 1 or 2; then the clip / scale arguments (`_check_clip`); then the history arguments fit the order."""
    if order not in (1, 2) or isinstance(order, bool):
        raise ValueError(f"{what}: order must be 1 or 2; got {order!r}")
    _check_clip(what, clip, scale, rows)
    if order == 1:
        if hist is not None or hist_out is not None:
            raise ValueError(f"{what}: the first-order step has no history")
    elif hist is None:
        raise ValueError(f"{what}: the second-order step needs hist")


def _like(x: Tensor, out: Optional[Tensor]) -> Tensor:
    """`out`, or a new tensor like x when it is missing."""
    return torch.empty_like(x) if out is None else out


def clip_rank(q: float, per: int) -> Tuple[int, float]:
    """(lo, w) of torch.quantile's linear rule, in its float32 arithmetic: rank = float32(q) * float32(per - 1)."""
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"clip_rank: q must be in [0, 1]; got {q!r}")
    if not 1 <= per <= CLIP_MAX_PER:
        raise ValueError(f"clip_rank: per must be in [1, 2**24]; got {per}")
    rank = torch.tensor(float(q), dtype=torch.float32) * torch.tensor(float(per - 1), dtype=torch.float32)
    lo = torch.floor(rank)
    return int(lo.item()), float((rank - lo).item())


def clip_ws(x: Tensor) -> Tensor:
    """The workspace `clip_scale` needs for x [B, ...] (uninitialised: the call zeroes what it uses)."""
    rows, per = _item_dims("clip_ws", x, CLIP_MAX_PER)
    return _ws(_C.query("adp_clip_ws_bytes", rows, per), x)


def clip_scale(x: Tensor, q: float, v: Optional[Tensor] = None, coef: Optional[Tensor] = None, min_scale: float = 1.0,
               ws: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """scale [B] = max(quantile_q(|y|), min_scale) per item of x [B, ...] (adp_clip_scale), y = x, or coef[0] x - coef[1] v
    when v is given (coef: device row whose first two values are a0, b0).  torch.quantile's linear rule, exact selection,
    no sort, no host read; a row holding a NaN gets NaN."""
    rows, per = _item_dims("clip_scale", x, CLIP_MAX_PER)
    if (v is None) != (coef is None):
        raise ValueError("clip_scale: v and coef go together")
    if v is not None and v.shape != x.shape:
        raise ValueError(f"clip_scale: v must have x's shape {tuple(x.shape)}; got {tuple(v.shape)}")
    if coef is not None and coef.numel() < 2:
        raise ValueError(f"clip_scale: coef holds (a0, b0, ...); got {coef.numel()} values")
    if out is None:
        out = torch.empty(rows, dtype=torch.float32, device=x.device)
    elif out.numel() != rows:
        raise ValueError(f"clip_scale: out must hold {rows} values; got {out.numel()}")
    if rows == 0 or per == 0:
        return out
    lo, w = clip_rank(q, per)
    need = _C.query("adp_clip_ws_bytes", rows, per)
    if ws is None:
        ws = _ws(need, x)
    elif ws.numel() * ws.element_size() < need:
        raise ValueError(f"clip_scale: the workspace holds {ws.numel() * ws.element_size()} bytes; {need} needed")
    _C.call("adp_clip_scale", ptr(x), ptr(v), ptr(coef), rows, per, lo, w, float(min_scale), ptr(ws, ws.dtype), ptr(out),
            _C.stream())
    return out


def clip_apply(x: Tensor, scale: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """clamp(x, -s, s) / s with one s per item of x [B, ...] (adp_clip_apply).  `out` may be x."""
    rows, per = _item_dims("clip_apply", x, CLIP_MAX_PER)
    if scale.numel() != rows:
        raise ValueError(f"clip_apply: scale must hold one value per item ({rows}); got {scale.numel()}")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape:
        raise ValueError(f"clip_apply: out must have x's shape {tuple(x.shape)}; got {tuple(out.shape)}")
    _C.call("adp_clip_apply", ptr(x), ptr(scale), rows, per, ptr(out), _C.stream())
    return out


def clip_step(x: Tensor, v: Tensor, coef: Tensor, scale: Optional[Tensor] = None, hist_x0: Optional[Tensor] = None,
              hist_eps: Optional[Tensor] = None, out: Optional[Tensor] = None, hist_x0_out: Optional[Tensor] = None,
              hist_eps_out: Optional[Tensor] = None):
    """One thresholded v-sampler update (adp_clip_step) on x [B, ...]: the predicted x0 is clamped to the item's scale and
    divided by it (scale=None: clamped to [-1, 1]); eps comes from the raw v.  A coef row of 4 values is the first-order
    step and returns x_next; one of 6 values (a0, b0, a1, b1, ca, cb) the second-order step on the history and returns
    (x_next, clipped x0, eps).  Every output may be its input; a row with ca = cb = 0 does not read the history."""
    rows, per = _item_dims("clip_step", x, CLIP_MAX_PER)
    if coef.numel() not in (4, 6):
        raise ValueError(f"clip_step: coef holds (a0, b0, a1, b1) or (a0, b0, a1, b1, ca, cb); got {coef.numel()} values")
    order = 1 if coef.numel() == 4 else 2
    for t in (v, hist_x0, hist_eps, out, hist_x0_out, hist_eps_out):
        if t is not None and t.shape != x.shape:
            raise ValueError(f"clip_step: every tensor must have x's shape {tuple(x.shape)}; got {tuple(t.shape)}")
    if scale is not None and scale.numel() != rows:
        raise ValueError(f"clip_step: scale must hold one value per item ({rows}); got {scale.numel()}")
    if out is None:
        out = torch.empty_like(x)
    if order == 1:
        if hist_x0 is not None or hist_eps is not None or hist_x0_out is not None or hist_eps_out is not None:
            raise ValueError("clip_step: the first-order step (4 coefficients) has no history")
    else:
        if hist_x0 is None or hist_eps is None:
            raise ValueError("clip_step: the second-order step (6 coefficients) needs hist_x0 and hist_eps")
        if hist_x0_out is None:
            hist_x0_out = torch.empty_like(x)
        if hist_eps_out is None:
            hist_eps_out = torch.empty_like(x)
    _C.call("adp_clip_step", ptr(x), ptr(v), ptr(hist_x0), ptr(hist_eps), ptr(coef), order, ptr(scale), rows, per, ptr(out),
            ptr(hist_x0_out), ptr(hist_eps_out), _C.stream())
    return out if order == 1 else (out, hist_x0_out, hist_eps_out)


# ---- include/adp_sde.h: the stochastic (DDIM-eta) v-sampler step on in-register Philox noise

def v_step_eta(x: Tensor, v: Tensor, coef5: Tensor, rng4: Optional[Tensor], scale: Optional[Tensor] = None,
               clip: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """One stochastic v-sampler update (adp_v_step_eta) on x [B, ...]: a1 x0c + ce eps + cz z with coef5 = device
    (a0, b0, a1, ce, cz) and z the normals of the rng4 row's stream, formed in registers (the values `randn` gives for the
    same row).  clip=False: x0c = x0.  clip=True: x0 is clamped to the item's scale and divided by it (scale=None: clamped
    to [-1, 1]); eps comes from the raw v.  A row with cz = 0 does not read rng4, which may then be None (with cz != 0 a
    missing row gives NaN).  `out` may be x."""
    rows, per = _item_dims("v_step_eta", x)
    _check_like("v_step_eta", x, v=v, out=out)
    _check_f32("v_step_eta", coef5, 5, "coef5 holds five float32 values (a0, b0, a1, ce, cz)")
    _check_clip("v_step_eta", clip, scale, rows)
    row = None if rng4 is None else _rng_row_ptr("v_step_eta", rng4)
    out = _like(x, out)
    _C.call("adp_v_step_eta", ptr(x), ptr(v), ptr(coef5), row, int(clip), ptr(scale), rows, per, ptr(out), _C.stream())
    return out


# ---- include/adp_rf.h: rectified flow (the fused noising and the sampler update)

def rf_noise(x: Tensor, noise: Tensor, t: Tensor, x_t_out: Optional[Tensor] = None, u_out: Optional[Tensor] = None):
    """(x_t, u) = ((1 - t_r) x + t_r noise, noise - x) for x [B, ...] and one time per item, t [B] (adp_rf_noise).  t = 0
    returns x and t = 1 returns noise, bit for bit.  An output may be an input."""
    rows, per = _item_dims("rf_noise", x)
    _check_like("rf_noise", x, noise=noise, x_t_out=x_t_out, u_out=u_out)
    _check_f32("rf_noise", t, rows, f"t holds one float32 time per item ({rows})")
    x_t_out, u_out = _like(x, x_t_out), _like(x, u_out)
    _C.call("adp_rf_noise", ptr(x), ptr(noise), ptr(t), rows, per, ptr(x_t_out), ptr(u_out), _C.stream())
    return x_t_out, u_out


def rf_table(times, order: int = 2) -> Tensor:
    """The sampler's coefficient rows [N, 6] = (1, t_i, 1 - t_i, t_{i+1}, 1 - t_{i+1}, cb_i) for the times t_0 .. t_N
    (include/adp_rf.h), float32 on the CPU: formed in float64 and rounded once.  cb_0 = 0, and every cb is 0 for order 1;
    for order 2, cb_i = (t_{i+1} - t_i)**2 / (2 (t_i - t_{i-1})), the variable-step two-step Adams-Bashforth weight."""
    if order not in (1, 2):
        raise ValueError(f"rf_table: order must be 1 or 2; got {order!r}")
    t = torch.as_tensor(times).detach().to(device="cpu", dtype=torch.float64).reshape(-1)
    if t.numel() < 1:
        raise ValueError("rf_table: times must hold at least t_0")
    n = t.numel() - 1
    cb = torch.zeros(n, dtype=torch.float64)
    if order == 2 and n > 1:
        d = t[1:] - t[:-1]
        g = d[:-1]
        if bool((g == 0).any()):
            raise ValueError(f"rf_table: the times repeat (zero step before step {int((g == 0).nonzero()[0]) + 1}); "
                             "neighbouring times must differ")
        cb[1:] = d[1:] * d[1:] / (2.0 * g)
    one = torch.ones(n, dtype=torch.float64)
    return torch.stack([one, t[:-1], 1.0 - t[:-1], t[1:], 1.0 - t[1:], cb], dim=1).to(torch.float32).contiguous()


def rf_step(x: Tensor, u: Tensor, coef6: Tensor, scale: Optional[Tensor] = None, clip: bool = False, order: int = 1,
            hist: Optional[Tensor] = None, out: Optional[Tensor] = None, hist_out: Optional[Tensor] = None):
    """One rectified-flow sampler update (adp_rf_step) on x [B, ...] with coef6 = device (1, t0, 1 - t0, t1, 1 - t1, cb).
    clip=False: x0c = x0.  clip=True: x0 is clamped to the item's scale and divided by it (scale=None: clamped to [-1, 1]);
    eps comes from the raw u.  order=1 returns x_next and has no history; order=2 returns (x_next, w) and needs `hist` (the
    previous step's w), which a row with cb = 0 does not read.  Every output may be its input."""
    rows, per = _item_dims("rf_step", x)
    _check_like("rf_step", x, u=u, hist=hist, out=out, hist_out=hist_out)
    _check_f32("rf_step", coef6, 6, "coef6 holds six float32 values (1, t0, 1 - t0, t1, 1 - t1, cb)")
    _check_order("rf_step", order, clip, scale, rows, hist, hist_out)
    out = _like(x, out)
    if order == 2:
        hist_out = _like(x, hist_out)
    _C.call("adp_rf_step", ptr(x), ptr(u), ptr(hist), ptr(coef6), order, int(clip), ptr(scale), rows, per, ptr(out),
            ptr(hist_out), _C.stream())
    return out if order == 1 else (out, hist_out)


# ---- include/adp_edm.h: Karras (EDM) diffusion (the fused noising and the sampler update on the scaled state)

def _check_sigma_data(what: str, sigma_data) -> float:
    if isinstance(sigma_data, bool) or not isinstance(sigma_data, (int, float)) or not sigma_data > 0.0:
        raise ValueError(f"{what}: sigma_data must be a positive number; got {sigma_data!r}")
    return float(sigma_data)


def edm_noise(x: Tensor, noise: Tensor, sigma: Tensor, sigma_data: float = 0.5, x_in_out: Optional[Tensor] = None,
              target_out: Optional[Tensor] = None):
    """(x_in, target) = (c_in x + c_in sigma_r noise, (sigma_r / (sd r)) x - (sd / r) noise) for x [B, ...] and one sigma per
    item, sigma [B] (adp_edm_noise): what the preconditioned net reads and what it is trained towards.  x_in is the sampler's
    scaled state of x + sigma_r noise.  An output may be an input."""
    rows, per = _item_dims("edm_noise", x)
    _check_like("edm_noise", x, noise=noise, x_in_out=x_in_out, target_out=target_out)
    _check_f32("edm_noise", sigma, rows, f"sigma holds one float32 value per item ({rows})")
    sd = _check_sigma_data("edm_noise", sigma_data)
    x_in_out, target_out = _like(x, x_in_out), _like(x, target_out)
    _C.call("adp_edm_noise", ptr(x), ptr(noise), ptr(sigma), sd, rows, per, ptr(x_in_out), ptr(target_out), _C.stream())
    return x_in_out, target_out


def edm_table(sigmas, sigma_data: float = 0.5, order: int = 2, eta: float = 0.0) -> Tensor:
    """The sampler's coefficient rows [N, 8] = (a0, b0, e0, f0, c1, d1, s1, cb) for the noise levels sigma_0 .. sigma_N
    (include/adp_edm.h), float32 on the CPU: formed in float64 and rounded once.  With sd = sigma_data, r = sqrt(s^2 + sd^2):

        a0 = sd^2 / r_i    b0 = -s_i sd / r_i    e0 = s_i / r_i    f0 = -sd / r_i
        g = 1 / r_{i+1} (1 on the last step)     c1 = g            d1 = g s_down     s1 = g s_up
        s_up = min(s_{i+1}, eta sqrt(s_{i+1}^2 (s_i^2 - s_{i+1}^2) / s_i^2))         s_down = sqrt(s_{i+1}^2 - s_up^2)
        cb_i = g (1 - s_{i+1} / s_i) h_i / (2 h_{i-1}),  h_i = ln(s_i / s_{i+1})     for order 2, i > 0 and s_{i+1} > 0, else 0

    cb is DPM-Solver++(2M)'s weight of (D_i - D_{i-1}): the step in -ln(sigma) over twice the previous one.  The sigmas must
    fall strictly; only the last one may be 0."""
    if isinstance(order, bool) or order not in (1, 2):
        raise ValueError(f"edm_table: order must be 1 or 2; got {order!r}")
    if isinstance(eta, bool) or not isinstance(eta, (int, float)) or not 0.0 <= eta <= 1.0:
        raise ValueError(f"edm_table: eta must be a number in [0, 1]; got {eta!r}")
    if eta > 0.0 and order == 2:
        raise ValueError("edm_table: eta > 0 needs order=1 (there is no second-order stochastic update)")
    sd = _check_sigma_data("edm_table", sigma_data)
    s = torch.as_tensor(sigmas).detach().to(device="cpu", dtype=torch.float64).reshape(-1)
    if s.numel() < 1:
        raise ValueError("edm_table: sigmas must hold at least sigma_0")
    n = s.numel() - 1
    if not bool(torch.isfinite(s).all()):
        raise ValueError("edm_table: every sigma must be finite")
    if bool((s[:-1] <= 0).any()):
        raise ValueError(f"edm_table: sigma_{int((s[:-1] <= 0).nonzero()[0])} is not positive; only the last sigma may be 0")
    if s[-1] < 0:
        raise ValueError(f"edm_table: the last sigma must not be negative; got {s[-1].item()}")
    if bool((s[1:] >= s[:-1]).any()):
        raise ValueError(f"edm_table: the sigmas must fall strictly; sigma_{int((s[1:] >= s[:-1]).nonzero()[0]) + 1} does not")
    s0, s1 = s[:-1], s[1:]
    r0 = torch.sqrt(s0 * s0 + sd * sd)
    g = 1.0 / torch.sqrt(s1 * s1 + sd * sd)
    if n > 0:
        g[-1] = 1.0
    up = torch.minimum(s1, eta * torch.sqrt(s1 * s1 * (s0 * s0 - s1 * s1) / (s0 * s0)))
    down = torch.sqrt((s1 * s1 - up * up).clamp_min(0.0))
    cb = torch.zeros(n, dtype=torch.float64)
    if order == 2 and n > 1:
        multi = s1[1:] > 0
        h = torch.log(s0[1:] / torch.where(multi, s1[1:], s0[1:]))     # (h_i, 0 where the step ends at sigma = 0)
        h_last = torch.log(s0[:-1] / s0[1:])
        cb[1:] = torch.where(multi, g[1:] * (1.0 - s1[1:] / s0[1:]) * h / (2.0 * h_last), torch.zeros_like(h))
    rows = [sd * sd / r0, -s0 * sd / r0, s0 / r0, -sd / r0, g, g * down, g * up, cb]
    return torch.stack(rows, dim=1).to(torch.float32).contiguous()


def edm_step(xs: Tensor, f: Tensor, coef8: Tensor, rng4: Optional[Tensor] = None, scale: Optional[Tensor] = None,
             clip: bool = False, order: int = 1, hist: Optional[Tensor] = None, out: Optional[Tensor] = None,
             hist_out: Optional[Tensor] = None):
    """One Karras (EDM) sampler update (adp_edm_step) on the scaled state xs [B, ...] and the net's output f, with coef8 =
    device (a0, b0, e0, f0, c1, d1, s1, cb): c1 x0c + d1 nh [+ cb (x0c - hist)] [+ s1 z], x0 = a0 xs - b0 f, nh = e0 xs + f0 f,
    z the normals of the rng4 row's stream, formed in registers (the values `randn` gives for the same row).  clip=False:
    x0c = x0.  clip=True: x0 is clamped to the item's scale and divided by it (scale=None: clamped to [-1, 1]); nh comes from
    the raw f.  order=1 returns xs_next and has no history; order=2 returns (xs_next, x0c) and needs `hist` (the previous
    step's x0c), which a row with cb = 0 does not read.  A row with s1 = 0 does not read rng4, which may then be None (with
    s1 != 0 a missing row gives NaN).  Every output may be its input."""
    rows, per = _item_dims("edm_step", xs)
    _check_like("edm_step", xs, "xs", f=f, hist=hist, out=out, hist_out=hist_out)
    _check_f32("edm_step", coef8, 8, "coef8 holds eight float32 values (a0, b0, e0, f0, c1, d1, s1, cb)")
    _check_order("edm_step", order, clip, scale, rows, hist, hist_out)
    row = None if rng4 is None else _rng_row_ptr("edm_step", rng4)
    out = _like(xs, out)
    if order == 2:
        hist_out = _like(xs, hist_out)
    _C.call("adp_edm_step", ptr(xs), ptr(f), ptr(hist), ptr(coef8), row, order, int(clip), ptr(scale), rows, per, ptr(out),
            ptr(hist_out), _C.stream())
    return out if order == 1 else (out, hist_out)


# ---- include/adp_repaint.h: RePaint inpainting (the objective's first-order update, the jump back, the known region)

REPAINT_OBJECTIVES = {"v": ("adp_repaint_v_step", 4), "rf": ("adp_repaint_rf_step", 6), "k": ("adp_repaint_k_step", 8)}


def _repaint_objective(what: str, objective):
    if objective not in REPAINT_OBJECTIVES:
        raise ValueError(f"{what}: objective must be one of {tuple(REPAINT_OBJECTIVES)}; got {objective!r}")
    return REPAINT_OBJECTIVES[objective]


def repaint_table(objective: str, levels, num_resamples: int, sigma_data: float = 0.5) -> Tensor:
    """The coefficient rows [N * R, W + 4] of a RePaint run over the levels l_0 .. l_N with R = num_resamples
    (include/adp_repaint.h), float32 on the CPU, in loop order (step i, resample r at row i R + r): the objective's own
    first-order step row for (i, i + 1) -- `VSampler`'s (a_i, b_i, a_{i+1}, b_{i+1}) formed in float32 where `levels` lives
    (W = 4), `rf_table(order=1)`'s (W = 6), `edm_table(order=1, eta=0)`'s (W = 8) -- then (A, S, P, Q), formed in float64 and
    rounded once.  With x_l = a_l x0 + b_l n, (a, b) = (cos, sin)(l pi / 2) | (1 - l, l) | (1, l) for "v" | "rf" | "k":

        r < R - 1 (jump back to level i):  A = a_i / a_{i+1}   S = sqrt(max(b_i^2 - (A b_{i+1})^2, 0))   P = a_i       Q = b_i
        r = R - 1 (move on to level i+1):  A = 1               S = 0                                     P = a_{i+1}   Q = b_{i+1}

    For "k" the state is scaled by c_in(l) = 1 / sqrt(l^2 + sigma_data^2) and the factors fold in: A = c_in(l_i) / g with g the
    factor the step row applied, S = c_in(l_i) sqrt(l_i^2 - l_{i+1}^2), P = c_in(l_j), Q = c_in(l_j) l_j; the last row of the
    run has P = 1, Q = 0 (the run ends unscaled, on the source itself).  The levels must fall strictly; the last may be 0."""
    _, words = _repaint_objective("repaint_table", objective)
    if isinstance(num_resamples, bool) or not isinstance(num_resamples, int) or num_resamples < 1:
        raise ValueError(f"repaint_table: num_resamples must be an integer >= 1; got {num_resamples!r}")
    lv = torch.as_tensor(levels).detach()
    l = lv.to(device="cpu", dtype=torch.float64).reshape(-1)
    if l.numel() < 1:
        raise ValueError("repaint_table: levels must hold at least l_0")
    n, R = l.numel() - 1, num_resamples
    if not bool(torch.isfinite(l).all()):
        raise ValueError("repaint_table: every level of the schedule must be finite")
    if bool((l[1:] >= l[:-1]).any()):
        raise ValueError("repaint_table: the levels of the schedule must fall strictly; "
                         f"level {int((l[1:] >= l[:-1]).nonzero()[0]) + 1} does not")
    if l[-1] < 0 or (objective != "k" and l[0] > 1):
        raise ValueError(f"repaint_table: the levels of the schedule must lie in [0, {'inf)' if objective == 'k' else '1]'}; "
                         f"got {l[0].item()} .. {l[-1].item()}")
    if objective == "v":
        s32 = lv.to(torch.float32).reshape(-1)
        angle = s32 * torch.pi / 2        # (diffusion.alpha_beta's float32 arithmetic, where the levels live)
        al, be = torch.cos(angle), torch.sin(angle)
        step = torch.stack([al[:-1], be[:-1], al[1:], be[1:]], dim=1).to("cpu")
        a, b = torch.cos(l * (torch.pi / 2)), torch.sin(l * (torch.pi / 2))
    elif objective == "rf":
        step = rf_table(l, order=1)
        a, b = 1.0 - l, l
    else:
        sd = _check_sigma_data("repaint_table", sigma_data)
        step = edm_table(l, sd, order=1, eta=0.0)
        a, b = torch.ones_like(l), l
    A = a[:-1] / a[1:]
    S = torch.sqrt((b[:-1] * b[:-1] - (A * b[1:]) ** 2).clamp_min(0.0))
    jump = torch.stack([A, S, a[:-1], b[:-1]], dim=1)
    move = torch.stack([torch.ones(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), a[1:], b[1:]], dim=1)
    if objective == "k":
        c_in = 1.0 / torch.sqrt(l * l + sd * sd)
        g = c_in[1:].clone()
        if n > 0:
            g[-1] = 1.0
        jump = torch.stack([c_in[:-1] / g, c_in[:-1] * S, c_in[:-1], c_in[:-1] * b[:-1]], dim=1)
        move[:, 2], move[:, 3] = c_in[1:], c_in[1:] * b[1:]
        if n > 0:
            move[-1, 2], move[-1, 3] = 1.0, 0.0
    blend = jump[:, None, :].repeat(1, R, 1)
    blend[:, R - 1] = move
    rows = torch.cat([step[:, None, :].expand(n, R, words), blend.to(torch.float32)], dim=2)
    return rows.reshape(n * R, words + 4).contiguous()


def repaint_step(objective: str, x: Tensor, p: Tensor, source: Tensor, mask_u8: Tensor, row: Tensor,
                 rng4: Optional[Tensor] = None, scale: Optional[Tensor] = None, clip: bool = False,
                 out: Optional[Tensor] = None) -> Tensor:
    """One RePaint resample (adp_repaint_{v,rf,k}_step) on x [B, ...] and the net's output p: the objective's first-order
    update by the first W values of `row` (one row of `repaint_table`, W + 4 float32 values on the device), then with its last
    four (A, S, P, Q): y = A y + S z, and P source + Q z where mask_u8 is set; z the normals of the rng4 row's stream,
    formed in registers (the values `randn` gives for the same row).  clip, scale: as in `rf_step`.  A row with S = Q = 0
    does not read rng4, which may then be None (where a normal is needed a missing row gives NaN).  `out` may be x."""
    entry, words = _repaint_objective("repaint_step", objective)
    rows, per = _item_dims("repaint_step", x)
    _check_like("repaint_step", x, p=p, source=source, mask=mask_u8, out=out)
    _check_f32("repaint_step", row, words + 4, f"row holds {words + 4} float32 values for objective {objective!r} (the "
               f"step's {words}, then A, S, P, Q)")
    _check_clip("repaint_step", clip, scale, rows)
    rng = None if rng4 is None else _rng_row_ptr("repaint_step", rng4)
    out = _like(x, out)
    _C.call(entry, ptr(x), ptr(p), ptr(source), ptr(mask_u8, torch.uint8), ptr(row), rng, int(clip), ptr(scale), rows, per,
            ptr(out), _C.stream())
    return out


# ---- include/adp_distill.h: progressive distillation (the per-item combination and the per-item weighted squared error)

DISTILL_ROWS = ("sigma", "sigma_mid", "cos_d1", "neg_sin_d1", "c_x", "c_1", "c_2", "w")


def distill_table(levels) -> Tensor:
    """The rows [8, N] = (sigma_i, sigma_mid, cos d1, -sin d1, c_x, c_1, c_2, w_i) of the N student steps over the 2N + 1
    teacher levels (include/adp_distill.h), float32 on the CPU: formed in float64 and rounded once.  With phi = level pi / 2,
    d1 = phi_{2i} - phi_{2i+1}, d2 = phi_{2i+1} - phi_{2i+2}, D = d1 + d2: c_x = -sin d1 sin d2 / sin D,
    c_1 = cos d2 sin d1 / sin D, c_2 = sin d2 / sin D, and w_i = max(cos^2 phi_{2i}, sin^2 phi_{2i}): the truncated-SNR weight
    max(SNR, 1) on the x error of Salimans & Ho 2022, written on the v error (|dx|^2 = sin^2 phi |dv|^2)."""
    s = torch.as_tensor(levels).detach().to(device="cpu", dtype=torch.float64).reshape(-1)
    if s.numel() < 3 or s.numel() % 2 == 0:
        raise ValueError(f"distill_table: levels holds the 2N + 1 teacher levels of N >= 1 student steps; got {s.numel()}")
    if not bool(((s >= 0) & (s <= 1)).all()) or not bool((s[1:] < s[:-1]).all()):
        raise ValueError("distill_table: the levels must fall strictly inside [0, 1]")
    half = math.pi / 2
    d1, d2 = (s[0:-2:2] - s[1:-1:2]) * half, (s[1:-1:2] - s[2::2]) * half
    sin_d = torch.sin(d1 + d2)
    phi = s[0:-2:2] * half
    w = torch.maximum(torch.cos(phi) ** 2, torch.sin(phi) ** 2)
    rows = [s[0:-2:2], s[1:-1:2], torch.cos(d1), -torch.sin(d1), -torch.sin(d1) * torch.sin(d2) / sin_d,
            torch.cos(d2) * torch.sin(d1) / sin_d, torch.sin(d2) / sin_d, w]
    return torch.stack(rows, dim=0).to(torch.float32).contiguous()


def distill_comb(x: Tensor, p: Tensor, coef: Tensor, q: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """out = c0_r x + c1_r p [+ c2_r q] on x [B, ...] with one coefficient per item and term, coef [terms, B] float32 on the
    device, terms = 2 (no q) or 3 (adp_distill_comb).  `out` may be any input."""
    rows, per = _item_dims("distill_comb", x)
    _check_like("distill_comb", x, p=p, q=q, out=out)
    terms = 2 if q is None else 3
    if coef.dtype != torch.float32 or tuple(coef.shape) != (terms, rows):
        raise ValueError(f"distill_comb: coef holds {terms} float32 coefficients per item, [{terms}, {rows}]"
                         f"{'' if q is not None else ' (no q: two terms)'}; got {coef.dtype} {tuple(coef.shape)}")
    out = _like(x, out)
    _C.call("adp_distill_comb", ptr(x), ptr(p), ptr(q), ptr(coef), terms, rows, per, ptr(out), _C.stream())
    return out


def _check_wmse(what: str, v_pred: Tensor, v_target: Tensor, w: Optional[Tensor]) -> Tuple[int, int]:
    rows, per = _item_dims(what, v_pred)
    _check_like(what, v_pred, "v_pred", v_target=v_target)
    if w is not None:
        _check_f32(what, w, rows, f"w holds one float32 weight per item ({rows})")
    if rows * per == 0:
        raise ValueError(f"{what}: the mean over no elements is undefined")
    return rows, per


def distill_wmse_fwd(v_pred: Tensor, v_target: Tensor, w: Optional[Tensor] = None) -> Tensor:
    """loss = mean over all elements of w_r (v_pred - v_target)^2, one weight per item (w=None: ones), in a fixed order of
    summation (adp_distill_wmse_fwd)."""
    rows, per = _check_wmse("distill_wmse_fwd", v_pred, v_target, w)
    loss = torch.empty((), dtype=torch.float32, device=v_pred.device)
    ws = _ws(_C.query("adp_distill_wmse_ws_bytes", rows, per), v_pred)
    _C.call("adp_distill_wmse_fwd", ptr(v_pred), ptr(v_target), ptr(w), rows, per, ptr(loss), ptr(ws), _C.stream())
    return loss


def distill_wmse_bwd(v_pred: Tensor, v_target: Tensor, w: Optional[Tensor], gloss: Optional[Tensor]) -> Tensor:
    """dv = gloss * 2 * w_r * (v_pred - v_target) / numel (adp_distill_wmse_bwd); gloss=None: 1."""
    rows, per = _check_wmse("distill_wmse_bwd", v_pred, v_target, w)
    dv = torch.empty_like(v_pred)
    _C.call("adp_distill_wmse_bwd", ptr(v_pred), ptr(v_target), ptr(w), ptr(gloss), rows, per, ptr(dv), _C.stream())
    return dv


def cfg_mix(y2: Tensor, scale: float) -> Tensor:
    """y2 [2B, ...] -> y2[B:] + (y2[:B] - y2[B:]) * scale."""
    half = y2.numel() // 2
    out = torch.empty((y2.shape[0] // 2,) + tuple(y2.shape[1:]), dtype=torch.float32, device=y2.device)
    _C.call("adp_cfg_mix", ptr(y2), half, float(scale), ptr(out), _C.stream())
    return out


def select_rows(a: Tensor, b: Tensor, pick_u8: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """out[r] = pick[r] ? a[r] : b[r] for the leading dimension r."""
    rows = a.shape[0]
    per = a.numel() // rows
    if out is None:
        out = torch.empty_like(a)
    _C.call("adp_select_rows", ptr(a), ptr(b), ptr(pick_u8, torch.uint8), rows, per, ptr(out), _C.stream())
    return out


def resample(x: Tensor, kern: Tensor, fi: int, fo: int, width: int, out_len: int) -> Tensor:
    """x [B, C, length], kern [fo, J] -> [B, C, out_len] (adp_resample)."""
    B, C, length = x.shape
    J = kern.shape[-1]
    out = torch.empty((B, C, out_len), dtype=torch.float32, device=x.device)
    _C.tag(bytes=4 * (x.numel() + out.numel()), shape=f"rows{B * C} len{length} {fi}->{fo}")
    _C.call("adp_resample", ptr(x), ptr(kern), B * C, length, fi, fo, J, width, out_len, ptr(out), _C.stream())
    return out


def mel_frames(length: int, n_fft: int, hop: int) -> int:
    return _C.query("adp_mel_frames", length, n_fft, hop)


def mel_spectrogram(x: Tensor, fb: Tensor, mel_range: Optional[Tensor], n_fft: int, hop: int, win: int, normalize: bool,
                    normalize_log: bool) -> Tensor:
    """x [rows, T], fb [n_fft // 2 + 1, n_mels], mel_range int32 [n_mels, 2] or None -> [rows, n_mels, frames]
    (adp_mel_spectrogram)."""
    rows, T = x.shape
    n_mels = fb.shape[1]
    assert fb.shape[0] == n_fft // 2 + 1, "mel_spectrogram: the filterbank is [n_fft // 2 + 1, n_mels]"
    frames = mel_frames(T, n_fft, hop)
    out = torch.empty((rows, n_mels, frames), dtype=torch.float32, device=x.device)
    ws = _ws(_C.query("adp_mel_spectrogram_ws_bytes", rows, T, n_fft, hop, win, n_mels), x) if normalize else None
    _C.tag(bytes=4 * (x.numel() + out.numel()), shape=f"rows{rows} len{T} fft{n_fft} hop{hop} mel{n_mels}")
    _C.call("adp_mel_spectrogram", ptr(x), ptr(fb), ptr(mel_range, torch.int32), rows, T, n_fft, hop, win, n_mels,
            int(bool(normalize)), int(bool(normalize_log)), ptr(out), ptr(ws), _C.stream())
    return out


def tflat_fwd(spec: Tensor, w: Tensor, hop: int) -> Tensor:
    """spec [N, M, L], w [M, 1, K] -> [N, 1, Lout]: ConvTranspose1d(M, 1, K, stride=hop, padding=(K - hop) // 2) (adp_tflat_fwd)."""
    N, M, L = spec.shape
    K = w.shape[2]
    assert w.shape[0] == M and w.shape[1] == 1, "tflat_fwd: weight is [mel_channels, 1, kernel_size]"
    out = torch.empty((N, 1, _C.query("adp_tflat_out_len", L, K, hop)), dtype=torch.float32, device=spec.device)
    _C.tag(flops=2 * out.numel() * M * ((K + hop - 1) // hop), shape=f"N{N} M{M} L{L} K{K} hop{hop}")
    _C.call("adp_tflat_fwd", ptr(spec), ptr(w), N, M, L, K, hop, ptr(out), _C.stream())
    return out


def tflat_wgrad(spec: Tensor, g: Tensor, K: int, hop: int, dw: Optional[Tensor] = None) -> Tensor:
    """dW [M, 1, K] of tflat_fwd for the output gradient g [N, 1, Lout]; written, not accumulated (adp_tflat_wgrad)."""
    N, M, L = spec.shape
    assert g.shape == (N, 1, _C.query("adp_tflat_out_len", L, K, hop)), "tflat_wgrad: output gradient shape mismatch"
    if dw is None:
        dw = torch.empty((M, 1, K), dtype=torch.float32, device=spec.device)
        if os.environ.get("ADP_DEBUG_POISON", "0") == "1":  # (test-suite: a slice nobody wrote cannot pass)
            dw.fill_(float("nan"))
    ws = _ws(_C.query("adp_tflat_wgrad_ws_bytes", N, M, L, K, hop), spec)
    _C.tag(flops=2 * N * L * M * K, shape=f"N{N} M{M} L{L} K{K} hop{hop}")
    _C.call("adp_tflat_wgrad", ptr(spec), ptr(g), N, M, L, K, hop, ptr(dw), ptr(ws), _C.stream())
    return dw


# ---- learned-transform front end (include/adp_lt.h)
LT_ZERO, LT_REFLECT = 0, 1   # lt_conv / lt_wgrad: how the signal continues past its ends
LT_PLAIN, LT_FOLD = 0, 1     # lt_convt: outside positions dropped / added to their mirror positions


def _lt_out(shape, like: Tensor) -> Tensor:
    out = torch.empty(shape, dtype=torch.float32, device=like.device)
    if os.environ.get("ADP_DEBUG_POISON", "0") == "1":  # (test-suite: an element nobody wrote cannot pass)
        out.fill_(float("nan"))
    return out


def lt_conv(x: Tensor, w: Tensor, stride: int, pad: int, mode: int) -> Tensor:
    """x [B, C, T], w [O, C, K] -> [B, O, L]: the strided convolution over the reflect- / zero-continued x (adp_lt_conv)."""
    B, C, T = x.shape
    O, K = w.shape[0], w.shape[2]
    assert w.shape[1] == C, "lt_conv: weight is [out, in, kernel_size]"
    y = _lt_out((B, O, _C.query("adp_lt_conv_out_len", T, K, stride, pad)), x)
    _C.tag(flops=2 * y.numel() * C * K, shape=f"B{B} C{C} T{T} O{O} K{K} s{stride} p{pad} m{mode}")
    _C.call("adp_lt_conv", ptr(x), ptr(w), B, C, T, O, K, stride, pad, mode, ptr(y), _C.stream())
    return y


def lt_convt(x: Tensor, w: Tensor, stride: int, pad: int, mode: int, T: Optional[int] = None) -> Tensor:
    """x [B, C, L], w [C, O, K] -> [B, O, T]: the strided transposed convolution (adp_lt_convt).  LT_PLAIN: T is the
    layer's own length; LT_FOLD: T is the length of the signal lt_conv(..., LT_REFLECT) read, whose adjoint this is."""
    B, C, L = x.shape
    O, K = w.shape[1], w.shape[2]
    assert w.shape[0] == C, "lt_convt: weight is [in, out, kernel_size]"
    if T is None:
        assert mode == LT_PLAIN, "lt_convt: LT_FOLD needs the signal length T"
        T = _C.query("adp_lt_convt_out_len", L, K, stride, pad)
    out = _lt_out((B, O, T), x)
    _C.tag(flops=2 * out.numel() * C * ((K + stride - 1) // stride), shape=f"B{B} C{C} L{L} O{O} K{K} s{stride} p{pad} m{mode}")
    _C.call("adp_lt_convt", ptr(x), ptr(w), B, C, L, O, K, stride, pad, mode, T, ptr(out), _C.stream())
    return out


def lt_wgrad(u: Tensor, v: Tensor, K: int, stride: int, pad: int, mode: int, dw: Optional[Tensor] = None) -> Tensor:
    """dw [A, Bc, K] = sum over (batch, frame) of u [B, A, L] times the continued v [B, Bc, T] at l stride + k - pad;
    written, not accumulated, bit-identical from call to call (adp_lt_wgrad)."""
    B, A, L = u.shape
    Bc, T = v.shape[1], v.shape[2]
    assert v.shape[0] == B, "lt_wgrad: batch mismatch"
    if dw is None:
        dw = _lt_out((A, Bc, K), u)
    ws = _ws(_C.query("adp_lt_wgrad_ws_bytes", B, A, Bc, L, K), u)
    _C.tag(flops=2 * B * L * A * Bc * K, shape=f"B{B} A{A} Bc{Bc} L{L} K{K} s{stride} p{pad} m{mode}")
    _C.call("adp_lt_wgrad", ptr(u), ptr(v), B, A, Bc, L, T, K, stride, pad, mode, ptr(dw), ptr(ws), _C.stream())
    return dw


# ---- mel encoder (include/adp_enc.h)
def _enc_call(name: str, label: str, nbytes: int, args, keep) -> None:
    """One adp_enc_* launch; with _C.REPLAY set, the relaunch callable is recorded as ops.conv1d records its convs."""
    _C.call(name, *args, _C.stream())
    if _C.REPLAY is not None:
        _C.REPLAY.append((label, nbytes, lambda args=args, keep=keep: _C.call(name, *args, _C.stream())))


def enc_down_out_len(L: int, f: int) -> int:
    return _C.query("adp_enc_down_out_len", L, f)


def enc_down_fwd(x: Tensor, w: Tensor, bias: Tensor, f: int) -> Tensor:
    """x [B, R, L], w [M, R, 2f+1], bias [M] -> [B, M, ceil(L / f)]: Conv1d(kernel 2f+1, stride f, padding f)
    (adp_enc_down_fwd)."""
    B, R, L = x.shape
    M = w.shape[0]
    assert w.shape[1] == R and w.shape[2] == 2 * f + 1 and bias.shape == (M,), "enc_down_fwd: weight is [out, in, 2f+1]"
    y = _lt_out((B, M, enc_down_out_len(L, f)), x)
    label = f"B{B} R{R} M{M} L{L} f{f}"
    nbytes = 4 * (x.numel() + y.numel() + w.numel())
    _C.tag(flops=2 * y.numel() * R * (2 * f + 1), bytes=nbytes, shape=label)
    _enc_call("adp_enc_down_fwd", "enc_down_fwd " + label, nbytes, (ptr(x), ptr(w), ptr(bias), B, R, M, L, f, ptr(y)),
              (x, w, bias, y))
    return y


def enc_down_dgrad(dy: Tensor, w: Tensor, f: int, L: int) -> Tensor:
    """dy [B, M, ceil(L / f)], w [M, R, 2f+1] -> dx [B, R, L], the data gradient of enc_down_fwd (adp_enc_down_dgrad)."""
    B, M, N = dy.shape
    R = w.shape[1]
    assert w.shape[0] == M and w.shape[2] == 2 * f + 1, "enc_down_dgrad: weight is [out, in, 2f+1]"
    assert N == enc_down_out_len(L, f), "enc_down_dgrad: the output gradient is not the layer's output length"
    dx = _lt_out((B, R, L), dy)
    label = f"B{B} R{R} M{M} L{L} f{f}"
    nbytes = 4 * (dy.numel() + dx.numel() + w.numel())
    _C.tag(flops=2 * dy.numel() * R * (2 * f + 1), bytes=nbytes, shape=label)
    _enc_call("adp_enc_down_dgrad", "enc_down_dgrad " + label, nbytes, (ptr(dy), ptr(w), B, R, M, L, f, ptr(dx)), (dy, w, dx))
    return dx


def enc_down_wgrad(x: Tensor, dy: Tensor, f: int, dw: Optional[Tensor] = None, dbias: Optional[Tensor] = None):
    """(dw [M, R, 2f+1], dbias [M]) of enc_down_fwd for the input x [B, R, L] and the output gradient dy [B, M, ceil(L / f)];
    written, not accumulated, bit-identical from call to call (adp_enc_down_wgrad)."""
    B, R, L = x.shape
    M, N = dy.shape[1], dy.shape[2]
    assert dy.shape[0] == B and N == enc_down_out_len(L, f), "enc_down_wgrad: output gradient shape mismatch"
    if dw is None:
        dw = _lt_out((M, R, 2 * f + 1), x)
    if dbias is None:
        dbias = _lt_out((M,), x)
    ws = _ws(_C.query("adp_enc_down_wgrad_ws_bytes", B, R, M, L, f), x)
    label = f"B{B} R{R} M{M} L{L} f{f}"
    nbytes = 4 * (x.numel() + dy.numel() + dw.numel())
    _C.tag(flops=2 * dy.numel() * R * (2 * f + 1), bytes=nbytes, shape=label)
    _enc_call("adp_enc_down_wgrad", "enc_down_wgrad " + label, nbytes,
              (ptr(x), ptr(dy), B, R, M, L, f, ptr(dw), ptr(dbias), ptr(ws)), (x, dy, dw, dbias, ws))
    return dw, dbias


def enc_tanh_fwd(h: Tensor) -> Tensor:
    """tanh(h) (adp_enc_tanh_fwd)."""
    z = _lt_out(h.shape, h)
    _C.tag(bytes=8 * h.numel(), shape=f"n{h.numel()}")
    _enc_call("adp_enc_tanh_fwd", f"enc_tanh_fwd n{h.numel()}", 8 * h.numel(), (ptr(h), h.numel(), ptr(z)), (h, z))
    return z


def enc_tanh_bwd(z: Tensor, dz: Tensor) -> Tensor:
    """dz (1 - z^2) for z = tanh(h) (adp_enc_tanh_bwd)."""
    assert dz.shape == z.shape, "enc_tanh_bwd: gradient shape mismatch"
    dh = _lt_out(z.shape, z)
    _C.tag(bytes=12 * z.numel(), shape=f"n{z.numel()}")
    _enc_call("adp_enc_tanh_bwd", f"enc_tanh_bwd n{z.numel()}", 12 * z.numel(), (ptr(z), ptr(dz), z.numel(), ptr(dh)),
              (z, dz, dh))
    return dh


# ---- frozen T5 text encoder (include/adp_t5.h); forward only
def t5_embed(ids: Tensor, table: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """ids int64 [T], table [V, d] -> [T, d]; an id outside [0, V) gives a row of zeros (adp_t5_embed)."""
    T, (V, d) = ids.numel(), table.shape
    if out is None:
        out = _lt_out((T, d), table)
    _C.tag(bytes=8 * T * d, shape=f"T{T} V{V} d{d}")
    _C.call("adp_t5_embed", ptr(ids, torch.int64), ptr(table), T, V, d, ptr(out), _C.stream())
    return out


def t5_rmsnorm(x: Tensor, g: Tensor, eps: float, out: Optional[Tensor] = None) -> Tensor:
    """x [T, d] * rsqrt(mean x^2 + eps) * g [d]: T5's LayerNorm (adp_t5_rmsnorm)."""
    T, d = x.shape
    assert g.shape == (d,), "t5_rmsnorm: the weight is [d]"
    if out is None:
        out = _lt_out((T, d), x)
    _C.tag(bytes=8 * T * d, shape=f"T{T} d{d}")
    _C.call("adp_t5_rmsnorm", ptr(x), ptr(g), T, d, float(eps), ptr(out), _C.stream())
    return out


def t5_linear_ws_bytes(T: int, K: int, N: int) -> int:
    return _C.query("adp_t5_linear_ws_bytes", T, K, N)


def t5_linear(x: Tensor, w: Tensor, res: Optional[Tensor] = None, relu: bool = False, out: Optional[Tensor] = None,
              ws: Optional[Tensor] = None) -> Tensor:
    """res + act(x [T, K] @ w [N, K]^T) -> [T, N]; `out` may be `res` itself (adp_t5_linear).  `ws`: at least
    t5_linear_ws_bytes(T, K, N) bytes, allocated here when not given."""
    T, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K, "t5_linear: the weight is [out, in]"
    assert res is None or res.shape == (T, N), "t5_linear: the residual is [T, out]"
    if out is None:
        out = _lt_out((T, N), x)
    nbytes = t5_linear_ws_bytes(T, K, N)
    if ws is None and nbytes:
        ws = _ws(nbytes, x)
    assert nbytes == 0 or ws.numel() * 4 >= nbytes, "t5_linear: workspace too small"
    _C.tag(flops=2 * T * K * N, bytes=4 * (T * K + N * K + T * N), shape=f"T{T} K{K} N{N}")
    _C.call("adp_t5_linear", ptr(x), ptr(w), ptr(res), T, K, N, int(bool(relu)), ptr(out), ptr(ws) if nbytes else None,
            _C.stream())
    return out


def t5_attn(qkv: Tensor, rel_table: Tensor, bucket: Tensor, mask_u8: Optional[Tensor], heads: int,
            out: Optional[Tensor] = None) -> Tensor:
    """qkv [B, m, 3 H dk], rel_table [nb, H], bucket int32 [2m - 1], mask uint8 [B, m] or None -> [B, m, H dk]: T5
    self-attention with the relative-position bias and the key mask (adp_t5_attn)."""
    B, m, W = qkv.shape
    assert W % (3 * heads) == 0, "t5_attn: the packed projection is [B, m, 3 H dk]"
    dk, nb = W // (3 * heads), rel_table.shape[0]
    assert rel_table.shape == (nb, heads) and bucket.shape == (2 * m - 1,), "t5_attn: bias table [nb, H], bucket [2m - 1]"
    assert mask_u8 is None or mask_u8.shape == (B, m), "t5_attn: the mask is [B, m]"
    if out is None:
        out = _lt_out((B, m, heads * dk), qkv)
    _C.tag(flops=4 * B * heads * m * m * dk, bytes=4 * (qkv.numel() + out.numel()), shape=f"B{B} H{heads} dk{dk} m{m}")
    _C.call("adp_t5_attn", ptr(qkv), ptr(rel_table), ptr(bucket, torch.int32), ptr(mask_u8, torch.uint8), B, heads, dk, m, nb,
            ptr(out), _C.stream())
    return out


# ---- gated feed-forward GEMM of the T5 v1.1 / flan-T5 encoder (include/adp_gated.h); forward only
GATED_ACT_GELU_NEW = 1


def gated_linear_ws_bytes(T: int, K: int, F: int) -> int:
    return _C.query("adp_gated_linear_ws_bytes", T, K, F)


def gated_linear(x: Tensor, w_gate: Tensor, w_up: Tensor, out: Optional[Tensor] = None,
                 ws: Optional[Tensor] = None) -> Tensor:
    """gelu_new(x [T, K] @ w_gate [F, K]^T) * (x @ w_up [F, K]^T) -> [T, F] in one GEMM (adp_gated_linear); `out` overlaps
    no input.  `ws`: at least gated_linear_ws_bytes(T, K, F) bytes, allocated here when not given."""
    T, K = x.shape
    F = w_gate.shape[0]
    assert w_gate.shape == (F, K) and w_up.shape == (F, K), "gated_linear: both weights are [out, in]"
    if out is None:
        out = _lt_out((T, F), x)
    nbytes = gated_linear_ws_bytes(T, K, F)
    if ws is None and nbytes:
        ws = _ws(nbytes, x)
    assert nbytes == 0 or ws.numel() * 4 >= nbytes, "gated_linear: workspace too small"
    _C.tag(flops=4 * T * K * F, bytes=4 * (T * K + 2 * F * K + T * F), shape=f"T{T} K{K} F{F}")
    _C.call("adp_gated_linear", ptr(x), ptr(w_gate), ptr(w_up), T, K, F, GATED_ACT_GELU_NEW, ptr(out),
            ptr(ws) if nbytes else None, _C.stream())
    return out


def add(a: Tensor, b: Tensor, out: Optional[Tensor] = None) -> Tensor:
    if out is None:
        out = torch.empty_like(a)
    _C.call("adp_add", ptr(a), ptr(b), a.numel(), ptr(out), _C.stream())
    return out


def axpby(a: float, x: Tensor, b: float = 0.0, y: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """out = a * x + b * y (y optional)."""
    if out is None:
        out = torch.empty_like(x)
    _C.call("adp_axpby", float(a), ptr(x), float(b), ptr(y), x.numel(), ptr(out), _C.stream())
    return out


def sqnorm_partials(ptrs: Tensor, numels: Tensor, chunks: Tensor, partials: Tensor) -> int:
    """Per-block sums of squares (double) of the gradients named by the device tables (adp_sqnorm_partials): ptrs / numels
    int64 [T], chunks int64 [C, 3] = (tensor, first element, count); returns how many entries of `partials` were written."""
    assert partials.numel() >= 1024, "sqnorm_partials: the partials buffer holds one double per block (up to 1024)"
    return _C.call_value("adp_sqnorm_partials", ptr(ptrs, torch.int64), ptr(numels, torch.int64), ptrs.numel(),
                         ptr(chunks, torch.int64), chunks.shape[0], ptr(partials, torch.float64), _C.stream())


def adamw_step(tensors: Tensor, chunks: Tensor, *, decay: float, one_minus_beta1: float, beta2: float,
               one_minus_beta2: float, inv_bc2_sqrt: float, eps: float, step_size: float, ema_weight: float = 0.0,
               partials: Optional[Tensor] = None, n_partials: int = 0, max_grad_norm: float = 0.0,
               grad_norm_out: Optional[Tensor] = None) -> None:
    """One fused AdamW launch (adp_adamw_step) over the chunks of a device table: tensors int64 [T, 6] = (p, g, m, v, ema or 0,
    numel), chunks int64 [C, 3].  The scalars are the host's doubles; `partials` (from sqnorm_partials) switches clipping on."""
    _C.call("adp_adamw_step", ptr(tensors, torch.int64), ptr(chunks, torch.int64), chunks.shape[0], decay, one_minus_beta1,
            beta2, one_minus_beta2, inv_bc2_sqrt, eps, step_size, ema_weight, ptr(partials, torch.float64), n_partials,
            max_grad_norm, ptr(grad_norm_out), _C.stream())


def concat_channels(x: Tensor, x2: Tensor) -> Tensor:
    """torch.cat([x, x2], dim=1) of [B, C, L] tensors as two strided row copies (adp_copy2d)."""
    B, C1, L = x.shape
    C2 = x2.shape[1]
    assert x2.shape[0] == B and x2.shape[2] == L, "concat_channels: batch / length mismatch"
    out = torch.empty((B, C1 + C2, L), dtype=torch.float32, device=x.device)
    flat = out.view(-1)
    s = _C.stream()
    _C.call("adp_copy2d", ptr(x), C1 * L, ptr(flat), (C1 + C2) * L, B, C1 * L, s)
    _C.call("adp_copy2d", ptr(x2), C2 * L, ptr(flat[C1 * L:]), (C1 + C2) * L, B, C2 * L, s)
    return out


def split_channels(g: Tensor, C1: int):
    """Inverse of concat_channels: contiguous (g[:, :C1], g[:, C1:])."""
    B, C, L = g.shape
    a = torch.empty((B, C1, L), dtype=torch.float32, device=g.device)
    b = torch.empty((B, C - C1, L), dtype=torch.float32, device=g.device)
    flat = g.view(-1)
    s = _C.stream()
    _C.call("adp_copy2d", ptr(flat), C * L, ptr(a), C1 * L, B, C1 * L, s)
    _C.call("adp_copy2d", ptr(flat[C1 * L:]), C * L, ptr(b), (C - C1) * L, B, (C - C1) * L, s)
    return a, b


def unshuffle(x: Tensor, f: int) -> Tensor:
    """[B, C, L] -> [B, C*f, L/f] with out[b, c*f + k, l] = x[b, c, l*f + k] (adp_unshuffle)."""
    B, C, L = x.shape
    assert L % f == 0, "length must be divisible by the downsample factor"
    out = torch.empty((B, C * f, L // f), dtype=torch.float32, device=x.device)
    _C.call("adp_unshuffle", ptr(x), B * C, L, f, ptr(out), _C.stream())
    return out


def pool_sum(x: Tensor, f: int, res: Optional[Tensor] = None) -> Tensor:
    """[B, C, L*f] -> [B, C, L]: sums f adjacent positions (+ res) (adp_pool_sum)."""
    B, C, Lf = x.shape
    out = torch.empty((B, C, Lf // f), dtype=torch.float32, device=x.device)
    _C.call("adp_pool_sum", ptr(x), B * C, Lf // f, f, ptr(res), ptr(out), _C.stream())
    return out


def attn_fwd(q: Tensor, kv: Tensor, heads: int, head_features: int):
    """q [B, H*D, n]; kv [B, 2*H*D, m] (k = first half of the channels, v = second half) -> o [B, H*D, n], lse."""
    B, mid, n = q.shape
    m = kv.shape[2]
    H, D = heads, head_features
    assert mid == H * D and kv.shape[1] == 2 * mid
    o = torch.empty_like(q)
    lse = torch.empty((B, H, n), dtype=torch.float32, device=q.device)
    kvf = kv.view(-1)
    need = _C.query("adp_attn_fwd_ws_bytes", B, H, D, n, m)
    ws = _ws(need, q) if need > 0 else None  # key-split partials (small grids)
    _C.tag(flops=4 * B * H * n * m * D, bytes=4 * (2 * q.numel() + kv.numel()), shape=f"B{B} H{H} D{D} n{n} m{m}")
    _C.call("adp_attn_fwd", ptr(q), ptr(kvf), ptr(kvf[mid * m:]), B, H, D, n, m, mid * n, 2 * mid * m, ptr(o),
            ptr(lse), ptr(ws), _C.stream())
    return o, lse


def ctx_fold_fwd(tab: Tensor, I: int, M2: int, E: int):
    """Folded context bank of I CrossAttentionItems (adp_ctx_fold_fwd): tab = device int64 [3, I] pointers of (to_kv weight
    [M2, E], norm_context weight [E], norm_context bias [E]) -> (w_all [I*M2, E] = W_i diag(gamma_i), bias_all [I*M2] = W_i beta_i)."""
    w_all = torch.empty((I * M2, E), dtype=torch.float32, device=tab.device)
    bias_all = torch.empty((I * M2,), dtype=torch.float32, device=tab.device)
    _C.tag(bytes=8 * w_all.numel(), shape=f"I{I} M{M2} E{E}")
    _C.call("adp_ctx_fold_fwd", ptr(tab[0], torch.int64), ptr(tab[1], torch.int64), ptr(tab[2], torch.int64), I, M2, E,
            ptr(w_all), ptr(bias_all), _C.stream())
    return w_all, bias_all


def ctx_fold_bwd(tab: Tensor, dw_all: Tensor, dbias_all: Tensor, I: int, M2: int, E: int, flat: Tensor, dw_off: Tensor,
                 dgb_off: Tensor) -> None:
    """Gradients of the folded bank back to the items' parameters, written into the flat gradient buffer (adp_ctx_fold_bwd)."""
    _C.tag(bytes=12 * dw_all.numel(), shape=f"I{I} M{M2} E{E}")
    _C.call("adp_ctx_fold_bwd", ptr(tab[0], torch.int64), ptr(tab[1], torch.int64), ptr(tab[2], torch.int64), ptr(dw_all),
            ptr(dbias_all), I, M2, E, ptr(flat), ptr(dw_off, torch.int64), ptr(dgb_off, torch.int64), _C.stream())


def copy_rows(src: Tensor, src_stride: int, dst: Tensor, dst_stride: int, rows: int, cols: int) -> None:
    """dst[r * dst_stride + c] = src[r * src_stride + c] over flat fp32 views (adp_copy2d)."""
    _C.call("adp_copy2d", ptr(src), src_stride, ptr(dst), dst_stride, rows, cols, _C.stream())


def attn_bwd(q: Tensor, kv: Tensor, o: Tensor, dout: Tensor, lse: Tensor, heads: int, head_features: int,
             dkv: Optional[Tensor] = None):
    """Returns (dq [B, H*D, n], dkv [B, 2*H*D, m])."""
    B, mid, n = q.shape
    m = kv.shape[2]
    H, D = heads, head_features
    dq = torch.empty_like(q)
    if dkv is None:
        dkv = torch.empty_like(kv)
    ws = _ws(_C.query("adp_attn_bwd_ws_bytes", B, H, D, n, m), q)
    kvf, dkvf = kv.view(-1), dkv.view(-1)
    # QK^T is recomputed in both passes: dV, dP, dK in the key/value pass and dP, dQ in the query pass (7 contractions)
    _C.tag(flops=14 * B * H * n * m * D, bytes=4 * (4 * q.numel() + 2 * kv.numel()), shape=f"B{B} H{H} D{D} n{n} m{m}")
    _C.call("adp_attn_bwd", ptr(q), ptr(kvf), ptr(kvf[mid * m:]), ptr(o), ptr(dout), ptr(lse), B, H, D, n, m,
            mid * n, 2 * mid * m, ptr(dq), ptr(dkvf), ptr(dkvf[mid * m:]), ptr(ws), _C.stream())
    return dq, dkv
