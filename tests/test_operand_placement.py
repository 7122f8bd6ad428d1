"""Every C-ABI entry point with misaligned operands and guard bands (tests/placement.py).

include/adp.h promises plain device pointers: an operand needs the alignment of its element type and nothing more.
The kernels choose between 16-byte paths and fallbacks (and adp_conv1d between kernel families) by looking at the
pointers, so each table entry below is one direct call through `_C.lib()` whose operands the test places itself:

    zero    every operand at offset 0 (guards only: today's paths, checked for overruns)
    all1    every operand one element off a 16-byte boundary
    mixed   operand i at offset 1 + i mod 3
    single1 each pointer operand alone at offset 1, the others aligned
    single2 each output / residual / workspace operand alone at offset 2 (the 8-byte checks)

A placed call must return ADP_OK (ADP_ERR_ALIGN only where adp.h names the requirement: ALIGN_DOCUMENTED), match the
fp64 reference of tests/refs.py within the bound the entry point's own test uses (TOL = 1e-4 of test_kernels.py, or
the tighter bound where one exists -- no tolerance is introduced here), and leave every guard, offset gap and input
payload bit-identical (Arena.verify).
"""
import ctypes
import math
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

import refs
from audio_diffusion_pytorch_amd import _C
from conftest import rel_err
from placement import (GUARD_BYTES, PLANS, AlignRefused, Arena, PlacementError, Placer, close, exact, p,
                       place_and_check as shared_place_and_check, single)
from refs import rnd

TOL = 1e-4          # test_kernels.TOL

# entry points that are not placed, each with its reason; together with the table below this must equal _C.ABI["adp.h"]
EXCLUDED = {
    "adp_version": "no operands",
    "adp_launch_trace": "host-side introspection: writes a host string, launches nothing",
    "adp_launch_times": "host-side introspection: writes a host array, launches nothing",
    "adp_conv1d_ws_bytes": "size query (asked with the placed pointers inside the adp_conv1d cases)",
    "adp_conv1d_gn_entries": "entry-count query (asked with the placed pointers inside the adp_conv1d cases)",
    "adp_conv1d_gnb_entries": "entry-count query (asked with the placed pointers inside the adp_conv1d cases)",
    "adp_conv1d_tile": "tile query (asked with the placed pointers: the dispatch tables below)",
    "adp_conv1d_wgrad_ws_bytes": "size query (asked with the placed pointers inside the wgrad cases)",
    "adp_conv1d_wgrad_partials": "count query (asked with the placed pointers inside the parked wgrad case)",
    "adp_gn_stats_ws_bytes": "size query, integers only",
    "adp_row_nsplit": "count query, integers only",
    "adp_chan_ln_bwd_ws_bytes": "size query, integers only",
    "adp_linear_bwd_data_ws_bytes": "size query, integers only",
    "adp_skipmod_bwd_ws_bytes": "size query, integers only",
    "adp_mse_ws_bytes": "size query, integers only",
    "adp_stft_loss_ws_bytes": "size query, integers and a host array",
    "adp_mel_frames": "count query, integers only",
    "adp_mel_spectrogram_ws_bytes": "size query, integers only",
    "adp_tflat_out_len": "length query, integers only",
    "adp_tflat_wgrad_ws_bytes": "size query, integers only",
    "adp_attn_fwd_ws_bytes": "size query, integers only",
    "adp_attn_bwd_ws_bytes": "size query, integers only",
    "adp_probe_copy": "calibration probe; adp.h documents its 16-byte rule and returns ADP_ERR_ALIGN",
    "adp_probe_copy_v": "calibration probe, same 16-byte rule as adp_probe_copy",
    "adp_probe_mfma": "calibration probe: register operands, one private float per thread",
    "adp_probe_mfma_v": "calibration probe: register operands, one private float per thread",
    "adp_probe_launch": "calibration probe: empty kernel, no operands",
    "adp_probe_chase": "calibration probe: one lane, scalar int32 loads",
}


def strided_rows(rows, cols, stride):
    """Mask of the first `cols` elements of each of `rows` rows `stride` apart (a tensor of (rows-1)*stride + cols)."""
    m = torch.zeros((rows - 1) * stride + cols, dtype=torch.bool)
    for r in range(rows):
        m[r * stride:r * stride + cols] = True
    return m


def from_rows(t, rows, cols, stride):
    return torch.stack([t.reshape(-1)[r * stride:r * stride + cols] for r in range(rows)])


def to_rows(t2d, stride):
    """[rows, cols] -> flat tensor with row stride `stride` (gaps zero)."""
    rows, cols = t2d.shape
    f = torch.zeros((rows - 1) * stride + cols, dtype=t2d.dtype)
    for r in range(rows):
        f[r * stride:r * stride + cols] = t2d[r]
    return f


def stream():
    return _C.stream()


# =====================================================================================================================
# The table.  A case is `build(**shape) -> run(P)`; build makes the data and the fp64 references once per shape, run
# places the operands, makes the call(s) and returns [(label, got, want, bound), ...].
# =====================================================================================================================
CASES = []   # (id, entries covered, build, shape kwargs, env)


def case(entries, shapes, env=None):
    entries = (entries,) if isinstance(entries, str) else tuple(entries)

    def deco(fn):
        for i, sh in enumerate(shapes):
            e = dict(env or {})
            e.update(sh.pop("env", {}))
            CASES.append((f"{fn.__name__}-{i}", entries, fn, sh, e))
        return fn
    return deco


# ---------------------------------------------------------------------------------------------------- adp_conv1d
CONV_FAMILY = {}   # case id -> (family name, tile code the aligned placement must report)


# Bounds on the GroupNorm statistics that gn_part yields, per family: (mean: rel, mean: absolute alternative or None, rstd: rel),
# each the one the family's own test puts on adp_gn_finalize of the same partials, over the same groups --
# test_conv_tile32 / test_conv_tilek; test_conv_mm4_winograd_f43, test_conv_mm4_cross_workgroup_split_k and
# test_conv_tilek1_projection (4 groups); test_groupnorm_statistics_from_conv_epilogue for conv_mm's epilogues.
GN_BOUNDS = {"tile32": (2e-6, None, 2e-5), "tilek": (2e-6, None, 2e-5), "mm4": (2e-5, None, 2e-5),
             "tilek1": (2e-5, None, 2e-5), "mm": (1e-4, 1e-5, 1e-5)}


def conv_shapes():
    """At least one shape per kernel family of adp_conv1d's dispatch chain, forced the way test_kernels.py does."""
    mm4 = {"ADP_MM4_MIN_BLOCKS": "1", "ADP_CONV_TILEK": "0", "ADP_MM4_LIGHT_MIN_BLOCKS": "1000000"}
    no4 = {"ADP_CONV_WINO4": "0", "ADP_CONV_TILEK": "0", "ADP_CONV_TILEK1": "0"}
    tk = {"ADP_TILEK_MIN_R": "256", "ADP_TILEK_MIN_TILES": "1"}
    return [
        # tile32 (conv_tile.hip): 32 -> 32 channels, kernel 3; it takes bias, res, the GroupNorm prologue and gn_part
        dict(fam="tile32", tile=32064, B=1, R=32, M=32, L=128, bias=1, res=1, gn=1, env={"ADP_TILE_NW": "1"}),
        dict(fam="tile32", tile=32064, B=2, R=32, M=32, L=192, bias=1, res=1, gn=1, pro=1, env={"ADP_TILE_NW": "1"}),
        dict(fam="tile32", tile=32064, B=1, R=32, M=32, L=256, tr=1, gnb=1, env={"ADP_TILE_NW": "4"}),
        # tilek (conv_tilek.hip): deep kernel-3 layers, K split inside the workgroup
        dict(fam="tilek", tile=48000064, B=1, R=256, M=32, L=64, bias=1, res=1, gn=1, env=dict(tk, ADP_TILEK_RB="1")),
        dict(fam="tilek", tile=48000064, B=1, R=256, M=32, L=128, tr=1, res=1, gnb=1, env=dict(tk, ADP_TILEK_RB="2")),
        # mm4 (conv_mm4.hip): Winograd F(4,3) block, every epilogue operand; ragged last tile; cross-workgroup K split
        dict(fam="mm4", tile=64032128, B=1, R=64, M=32, L=128, bias=1, esc=1, res=1, pre=1, gn=1, env=mm4, tol=1e-5),
        dict(fam="mm4", tile=64032128, B=2, R=64, M=64, L=132, tr=1, bias=1, esc=1, res=1, pre=1, gn=1, env=mm4,
             tol=1e-5),
        dict(fam="mm4", tile=64032128, B=1, R=1024, M=32, L=128, bias=1, esc=1, res=1, pre=1, gn=1, want_ws=1, tol=1e-5,
             env=dict(mm4, ADP_MM4_KS_MAX="2", ADP_MM4_MIN_BLOCKS="2")),
        dict(fam="mm4", tile=64032128, B=1, R=64, M=64, L=128, tr=1, gnb=1, env=mm4, tol=1e-5),
        # tilek1 (conv_tilek1.hip): 1x1 projections
        dict(fam="tilek1", tile=47000064, B=2, R=256, M=48, L=64, KT=1, bias=1, res=1, gn=1, tol=1e-5,
             env={"ADP_TILEK1_MIN_TILES": "1", "ADP_TILEK1_NKW": "8"}),
        dict(fam="tilek1", tile=47000064, B=1, R=256, M=48, L=128, KT=1, tr=1, res=1, tol=1e-5,
             env={"ADP_TILEK1_MIN_TILES": "1", "ADP_TILEK1_NKW": "8"}),
        # mm (conv_mm.hip): direct form, Winograd F(2,3) variant, wide block, cross-workgroup K split + reduce
        dict(fam="mm", tile=4032064, B=1, R=64, M=64, L=128, bias=1, esc=1, res=1, pre=1, gn=1, pro=1,
             env=dict(no4, ADP_CONV_WINO="0")),
        dict(fam="mm", tile=4032064, B=2, R=96, M=32, L=72, KT=1, bias=1, esc=1, res=1, pre=1, gn=1,
             env=dict(no4, ADP_CONV_WINO="0")),
        dict(fam="mm-wino", tile=44032064, B=2, R=64, M=64, L=200, bias=1, esc=1, res=1, pre=1, gn=1, tol=1e-5,
             env=dict(no4, ADP_CONV_WINO="1")),
        dict(fam="mm-wino-wide", tile=42064128, B=2, R=64, M=64, L=300, tr=1, bias=1, esc=1, res=1, pre=1, gn=1, pro=1,
             tol=1e-5, env=dict(no4, ADP_CONV_WINO="1", ADP_MM_MIN_BLOCKS="1", ADP_MM_NSP="2")),
        dict(fam="mm-splitk", tile=44032064, B=1, R=512, M=64, L=64, bias=1, esc=1, res=1, pre=1, gn=1, want_ws=1,
             tol=1e-5, env=dict(no4, ADP_CONV_WINO="1")),
        dict(fam="mm-splitk", tile=44032064, B=1, R=512, M=64, L=64, tr=1, gnb=1, want_ws=1, tol=1e-5,
             env=dict(no4, ADP_CONV_WINO="1")),
        # direct (conv_direct.hip): narrow layers on the VALU; x2 concat, prologue
        dict(fam="direct", tile=8999, B=2, R=5, R2=3, M=8, L=1100, bias=1, esc=1, res=1, pre=1, pro=1, G=8),
        dict(fam="direct", tile=8999, B=1, R=2, M=6, L=516, bias=1, esc=1, res=1, pre=1),
        dict(fam="direct", tile=8999, B=1, R=8, M=32, L=256, KT=4, stride=4, pad=0, bias=1, esc=1, res=1, pre=1),
        # generic (conv1d.hip): everything else -- ragged lengths, channel counts no family wants, LayerNorm prologue
        dict(fam="generic", tile=32128, B=2, R=5, R2=3, M=6, L=90, bias=1, esc=1, res=1, pre=1, pro=1, G=4),
        dict(fam="generic", tile=32128, B=1, R=40, M=24, L=66, up=2, bias=1, esc=1, res=1, pre=1),
        dict(fam="generic", tile=64064, B=2, R=40, M=48, L=70, KT=1, pad=0, bias=1, esc=1, res=1, pre=1, pro=2),
        dict(fam="generic", tile=32128, B=1, R=16, M=32, L=128, KT=2, stride=2, pad=0, bias=1, esc=1, res=1, pre=1),
    ]


def _conv_build(fam, tile, B, R, M, L, KT=3, stride=1, pad=None, up=1, tr=0, R2=0, pro=0, G=8, bias=0, esc=0, res=0, pre=0,
                gn=0, gnb=0, want_ws=0, tol=TOL):
    pad = (KT - 1) // 2 if pad is None else pad
    Rt = R + R2
    N = (L * up + 2 * pad - (KT - 1) - 1) // stride + 1
    x = rnd(B, R, L, seed=1) * 1.3 + 0.2
    x2 = rnd(B, R2, L, seed=11) * 1.3 + 0.2 if R2 else None
    w = rnd(Rt, M, KT, seed=2, scale=Rt ** -0.5) if tr else rnd(M, Rt, KT, seed=2, scale=Rt ** -0.5)
    b = rnd(M, seed=3) if bias else None
    gamma, beta = rnd(Rt, seed=4) * 0.5 + 1, rnd(Rt, seed=5) * 0.1
    ebs = M + 5
    sc = rnd(B, M, seed=6) if esc else None
    r = rnd(B, M, N, seed=7) if res else None
    xcat = x if x2 is None else torch.cat([x, x2], 1)
    stats = None
    if pro == 1:
        stats = refs.gn_stats(xcat, G).float()
    elif pro == 2:
        stats = refs.ln_stats(xcat).float()
    a = refs.conv_input(x, x2, pro, G, gamma, beta, up)
    pre_ref = refs.conv(a, w, stride=stride, pad=pad, transposed=bool(tr))
    assert pre_ref.shape == (B, M, N)
    if bias:
        pre_ref = pre_ref + b.double()[None, :, None]
    ref = pre_ref * (sc.double()[:, :, None] if esc else 1.0) + (r.double() if res else 0.0)
    if gnb:  # this launch's output is da of SiLU(GroupNorm(gx)), gnb_groups = G
        gx = rnd(B, M, N, seed=8) * 1.5 + 0.4
        gga, gbe = rnd(M, seed=9) * 0.5 + 1, rnd(M, seed=10) * 0.2
        gst = refs.gn_stats(gx, G).float()
        _, _, _, dsx, ds = refs.gn_silu_bwd(gx, ref, G, gga, gbe)
        ab_ref = torch.stack([dsx.sum(-1), ds.sum(-1)], -1)   # [B, M, 2]: the slices of a row add up to this
    if gn:
        family = fam.split("-")[0]
        mean_rel, mean_abs, rstd_rel = GN_BOUNDS[family]
        GG = 4 if family == "tilek1" else 8      # the groups the family's own test finalizes over
        assert M % (4 * GG) == 0
        g64 = ref.reshape(B, GG, -1)
        gmean_ref, grstd_ref = g64.mean(-1), (g64.var(-1, unbiased=False) + 1e-5).rsqrt()

    def run(P):
        L_ = _C.lib()
        t = dict(x=P.inp("x", x), x2=P.inp("x2", x2) if R2 else None, w=P.inp("w", w),
                 bias=P.inp("bias", b) if bias else None,
                 pro_stats=P.inp("pro_stats", stats) if pro else None,
                 pro_gamma=P.inp("pro_gamma", gamma) if pro else None,
                 pro_beta=P.inp("pro_beta", beta) if pro else None,
                 e_scale=P.inp("e_scale", to_rows(sc, ebs)) if esc else None,
                 res=P.inp("res", r, res=True) if res else None,
                 out=P.out("out", (B, M, N)), out_pre=P.out("out_pre", (B, M, N)) if pre else None)
        d = _C.ConvDesc(p(t["x"]), p(t["x2"]), p(t["w"]), p(t["bias"]), p(t["pro_stats"]), p(t["pro_gamma"]),
                        p(t["pro_beta"]), p(t["e_scale"]), p(t["res"]), p(t["out"]), p(t["out_pre"]), B, Rt, R, L, M, N, KT,
                        stride, 1, pad, up, tr, pro, G if pro == 1 else 1, 0, 1, ebs if esc else 0, None, None)
        need = P.val(L_.adp_conv1d_ws_bytes(byref(d)) + 1, "adp_conv1d_ws_bytes") - 1
        if need > 0:
            d.ws = p(P.ws("ws", need))
        part = ab = None
        if gn:
            E = L_.adp_conv1d_gn_entries(byref(d))
            assert E >= 0, E
            if E > 0:
                part = P.out("gn_part", (B, M // 4, E, 3))
                d.gn_part = p(part)
        if gnb:
            gxd, gsd = P.inp("gnb_x", gx), P.inp("gnb_stats", gst)
            ggd, gbd = P.inp("gnb_gamma", gga), P.inp("gnb_beta", gbe)
            d.gnb_x, d.gnb_stats, d.gnb_gamma, d.gnb_beta, d.gnb_groups = p(gxd), p(gsd), p(ggd), p(gbd), G
            E = L_.adp_conv1d_gnb_entries(byref(d))
            assert E >= 0, E
            if E > 0:
                ab = P.out("gnb_ab", (B, M, E, 2))
                d.gnb_ab = p(ab)
        P.notes["tile"] = int(L_.adp_conv1d_tile(byref(d)))
        P.notes["ws"] = need
        P.notes["gn"], P.notes["gnb"] = part is not None, ab is not None
        P.call("adp_conv1d", lambda: L_.adp_conv1d(byref(d), stream()))
        checks = [("out", t["out"], ref, tol)]
        if pre:
            checks.append(("out_pre", t["out_pre"], pre_ref, tol))
        if part is not None:
            pc = part.cpu().double()
            assert pc[..., 2].sum(-1).eq(4 * N).all(), "gn_part: the slices of a row quad do not cover each element once"
            pg = pc.reshape(B, GG, -1, 3)        # a group's quads x slices; Chan's combination (what adp_gn_finalize does)
            cnt = pg[..., 2].sum(-1)
            mean = (pg[..., 0] * pg[..., 2]).sum(-1) / cnt
            m2 = (pg[..., 1] + pg[..., 2] * (pg[..., 0] - mean[..., None]) ** 2).sum(-1)
            e_mean = rel_err(mean, gmean_ref)
            print(f"gn_part mean: rel err {e_mean:.3e} (bound {mean_rel:.1e})")
            assert e_mean < mean_rel or (mean_abs is not None and (mean - gmean_ref).abs().max() < mean_abs), \
                f"gn_part mean: rel err {e_mean:.3e} >= {mean_rel:.1e}"
            checks.append(("gn_part rstd", (m2 / cnt + 1e-5).rsqrt(), grstd_ref, rstd_rel))
        if ab is not None:
            checks.append(("gnb_ab", ab.cpu().double().sum(2), ab_ref, 2e-5))
        return checks

    run.want_tile, run.want_ws, run.family = tile, want_ws, fam
    return run


for _i, _sh in enumerate(conv_shapes()):
    _env = _sh.pop("env", {})
    CASES.append((f"conv1d-{_sh['fam']}-{_i}", ("adp_conv1d",), _conv_build, _sh, _env))
    CONV_FAMILY[f"conv1d-{_sh['fam']}-{_i}"] = _sh["fam"]


# ---------------------------------------------------------------------------------------------------- weight gradients
def _wgrad_desc(t, B, Rt, R, L, M, N, KT, stride, pad, up, pro, G, acc):
    return _C.WgradDesc(p(t["x"]), p(t.get("x2")), p(t["dy"]), p(t.get("pro_stats")), p(t.get("pro_gamma")),
                        p(t.get("pro_beta")), p(t["dw"]), p(t.get("dbias")), None, B, Rt, R, L, M, N, KT, stride, 1, pad, up,
                        pro, G if pro == 1 else 1, acc)


@case(("adp_conv1d_wgrad", "adp_wgrad_reduce_batch"), [
    dict(form="mm", B=2, R=32, M=32, L=256, pro=1),                      # matrix-core family, Winograd F(4,3) form
    dict(form="mm", B=1, R=64, M=32, L=132, KT=1, pad=0, acc=1),         # 1x1, ragged last chunk, accumulated
    dict(form="mm-parked", B=2, R=32, M=32, L=4096, park=1),             # split: second stage by adp_wgrad_reduce_batch
    dict(form="mm-parked", B=1, R=32, M=64, L=4100, KT=1, pad=0, park=1, acc=1),   # ragged last chunk, accumulated, 1x1
    dict(form="direct", B=2, R=8, M=8, L=300, pro=1),                    # narrow layers on the VALU
    dict(form="direct", B=2, R=5, R2=3, M=6, L=1100, acc=1),
    dict(form="s1", B=1, R=40, M=24, L=66, up=2),                        # wide stride-1 layers no family wants
    dict(form="s1", B=2, R=48, M=80, L=70, pro=1),
    dict(form="generic", B=2, R=5, R2=3, M=6, L=90, pro=1, G=4),         # ragged length, concat
    dict(form="generic", B=1, R=16, M=32, L=128, KT=2, stride=2, pad=0),
])
def wgrad(form, B, R, M, L, KT=3, stride=1, pad=1, up=1, R2=0, pro=0, G=8, acc=0, park=0):
    Rt = R + R2
    N = (L * up + 2 * pad - (KT - 1) - 1) // stride + 1
    x = rnd(B, R, L, seed=1) * 1.3 + 0.2
    x2 = rnd(B, R2, L, seed=11) if R2 else None
    dy = rnd(B, M, N, seed=2)
    gamma, beta = rnd(Rt, seed=4) * 0.5 + 1, rnd(Rt, seed=5) * 0.1
    xcat = x if x2 is None else torch.cat([x, x2], 1)
    stats = refs.gn_stats(xcat, G).float() if pro else None
    base_w, base_b = rnd(M, Rt, KT, seed=6), rnd(M, seed=7)
    dw_ref, db_ref = refs.conv_wgrad(refs.conv_input(x, x2, pro, G, gamma, beta, up), dy, KT, stride=stride, pad=pad)
    if acc:
        dw_ref, db_ref = dw_ref + base_w.double(), db_ref + base_b.double()

    def run(P):
        L_ = _C.lib()
        t = dict(x=P.inp("x", x), dy=P.inp("dy", dy))
        if R2:
            t["x2"] = P.inp("x2", x2)
        if pro:
            t.update(pro_stats=P.inp("pro_stats", stats), pro_gamma=P.inp("pro_gamma", gamma),
                     pro_beta=P.inp("pro_beta", beta))
        if acc:
            t.update(dw=P.inout("dw", base_w), dbias=P.inout("dbias", base_b))
        else:
            t.update(dw=P.out("dw", (M, Rt, KT)), dbias=P.out("dbias", (M,)))
        d = _wgrad_desc(t, B, Rt, R, L, M, N, KT, stride, pad, up, pro, G, acc)
        ws = P.ws("ws", P.val(L_.adp_conv1d_wgrad_ws_bytes(byref(d)), "adp_conv1d_wgrad_ws_bytes"))
        d.ws = p(ws)
        partials = P.val(L_.adp_conv1d_wgrad_partials(byref(d)), "adp_conv1d_wgrad_partials")
        P.notes["partials"] = partials
        if park and partials > 1:   # as ops.conv1d_wgrad does: the second stage is parked only where the query says so
            d.accumulate = acc | 2
            P.call("adp_conv1d_wgrad", lambda: L_.adp_conv1d_wgrad(byref(d), stream()))
            arr = ctypes.c_void_p * 1
            P.ok(L_.adp_wgrad_reduce_batch(arr(p(ws)), arr(p(t["dw"])), arr(p(t["dbias"])), 1, partials, M * Rt * KT, M,
                                           acc, stream()), "adp_wgrad_reduce_batch")
        else:
            P.call("adp_conv1d_wgrad", lambda: L_.adp_conv1d_wgrad(byref(d), stream()))
        return [("dw", t["dw"], dw_ref, TOL), ("dbias", t["dbias"], db_ref, TOL)]

    run.want_partials = park
    # the kernel the aligned placement must launch (adp_launch_trace), so that the label stays true
    run.want_kernels = [{"mm": "wgrad_mm_kernel<", "direct": "wgrad_direct8_kernel<", "s1": "wgrad_s1_kernel<",
                         "generic": "wgrad_kernel<"}[form.split("-")[0]]]
    return run


@case("adp_conv1d_wgrad_batch", [dict(B=2, R=32, M=32, L=256, n=3), dict(B=1, R=40, M=24, L=66, n=2)])
def wgrad_batch(B, R, M, L, n):
    KT, pad = 3, 1
    xs = [rnd(B, R, L, seed=10 + i) for i in range(n)]
    dys = [rnd(B, M, L, seed=50 + i) for i in range(n)]
    want = [refs.conv_wgrad(xs[i].double(), dys[i], KT, pad=pad) for i in range(n)]

    def run(P):
        L_ = _C.lib()
        ts = []
        for i in range(n):
            ts.append(dict(x=P.inp(f"x{i}", xs[i]), dy=P.inp(f"dy{i}", dys[i]), dw=P.out(f"dw{i}", (M, R, KT)),
                           dbias=P.out(f"dbias{i}", (M,))))
        ds = [_wgrad_desc(t, B, R, R, L, M, L, KT, 1, pad, 1, 0, 1, 0) for t in ts]
        for i, d in enumerate(ds):
            d.ws = p(P.ws(f"ws{i}", P.val(L_.adp_conv1d_wgrad_ws_bytes(byref(d)), "adp_conv1d_wgrad_ws_bytes")))
        arr = (_C.WgradDesc * n)(*ds)
        P.ok(L_.adp_conv1d_wgrad_batch(arr, n, stream()), "adp_conv1d_wgrad_batch")
        out = []
        for i in range(n):
            out += [(f"dw{i}", ts[i]["dw"], want[i][0], TOL), (f"dbias{i}", ts[i]["dbias"], want[i][1], TOL)]
        return out
    return run


# ---------------------------------------------------------------------------------------------------- GroupNorm
GN_SHAPES = [dict(B=2, C=16, L=256, G=8), dict(B=2, C=32, L=130, G=8), dict(B=1, C=8, L=3001, G=4)]


@case("adp_gn_stats", GN_SHAPES)
def gn_stats(B, C, L, G):
    x = rnd(B, C, L, seed=1) * 1.7 + 0.3
    want = refs.gn_stats(x, G)

    def run(P):
        L_ = _C.lib()
        xd, st = P.inp("x", x), P.out("stats", (B, G, 2))
        ws = P.ws("ws", L_.adp_gn_stats_ws_bytes(B, C, L, G))
        P.ok(L_.adp_gn_stats(p(xd), B, C, L, G, 1e-5, p(st), p(ws), stream()), "adp_gn_stats")
        return [("stats", st, want, 1e-5)]
    return run


@case("adp_gn_stats_act", [dict(B=2, C=16, L=300, G=8), dict(B=1, C=64, L=1030, G=8), dict(B=2, C=512, L=24, G=8)])
def gn_stats_act(B, C, L, G):
    x = rnd(B, C, L, seed=1) * 1.7 + 0.3
    gamma, beta = rnd(C, seed=2) * 0.5 + 1, rnd(C, seed=3) * 0.1
    want_s, want_a = refs.gn_stats(x, G), refs.gn_silu(x, G, gamma, beta)

    def run(P):
        L_ = _C.lib()
        xd, ga, be = P.inp("x", x), P.inp("gamma", gamma), P.inp("beta", beta)
        st, a = P.out("stats", (B, G, 2)), P.out("act", (B, C, L))
        ws = P.ws("ws", L_.adp_gn_stats_ws_bytes(B, C, L, G))
        P.ok(L_.adp_gn_stats_act(p(xd), B, C, L, G, 1e-5, p(ga), p(be), p(st), p(a), p(ws), stream()), "adp_gn_stats_act")
        return [("stats", st, want_s, 1e-5), ("act", a, want_a, TOL)]
    return run


def _gn_partials(x, E):
    """(mean, M2, count) per slice of each 4-channel row quad: the layout conv epilogues leave (adp_conv_desc.gn_part)."""
    B, C, L = x.shape
    edges = [round(i * L / E) for i in range(E + 1)]
    part = torch.zeros(B, C // 4, E, 3, dtype=torch.float64)
    for e in range(E):
        s = x.double()[:, :, edges[e]:edges[e + 1]].reshape(B, C // 4, -1)
        part[:, :, e, 0] = s.mean(-1)
        part[:, :, e, 1] = ((s - s.mean(-1, keepdim=True)) ** 2).sum(-1)
        part[:, :, e, 2] = s.shape[-1]
    return part.float()


@case(("adp_gn_finalize", "adp_gn_finalize_act", "adp_gn_act"),
      [dict(B=2, C=32, L=256, G=8, E=4), dict(B=2, C=64, L=130, G=8, E=3), dict(B=1, C=16, L=77, G=2, E=1)])
def gn_finalize(B, C, L, G, E):
    x = rnd(B, C, L, seed=1) * 1.7 + 0.3
    part = _gn_partials(x, E)
    gamma, beta = rnd(C, seed=2) * 0.5 + 1, rnd(C, seed=3) * 0.1
    want_s, want_a = refs.gn_stats(x, G), refs.gn_silu(x, G, gamma, beta)

    def run(P):
        L_ = _C.lib()
        xd, pd, ga, be = P.inp("x", x), P.inp("part", part), P.inp("gamma", gamma), P.inp("beta", beta)
        sd = P.inp("stats_in", want_s.float())
        st, st2 = P.out("stats", (B, G, 2)), P.out("stats2", (B, G, 2))
        a, a2 = P.out("act", (B, C, L)), P.out("act2", (B, C, L))
        P.ok(L_.adp_gn_finalize(p(pd), B, C, E, G, 1e-5, p(st), stream()), "adp_gn_finalize")
        P.ok(L_.adp_gn_finalize_act(p(xd), p(pd), B, C, L, E, G, 1e-5, p(ga), p(be), p(st2), p(a2), stream()),
             "adp_gn_finalize_act")
        P.ok(L_.adp_gn_act(p(xd), p(sd), p(ga), p(be), B, C, L, G, p(a), stream()), "adp_gn_act")
        return [("stats", st, want_s, 1e-5), ("stats2", st2, want_s, 1e-5), ("act", a, want_a, TOL),
                ("act2", a2, want_a, TOL)]
    return run


@case(("adp_gn_silu_bwd_reduce", "adp_gn_silu_bwd_apply", "adp_gn_silu_bwd_apply_ab", "adp_gn_param_grad"),
      [dict(B=2, C=32, L=256, G=8), dict(B=2, C=32, L=130, G=8), dict(B=2, C=8, L=3001, G=8, acc=1)])
def gn_silu_bwd(B, C, L, G, acc=0):
    x = rnd(B, C, L, seed=1) * 1.5 + 0.4
    gamma, beta = rnd(C, seed=2) * 0.5 + 1, rnd(C, seed=3) * 0.2
    dact, dres = rnd(B, C, L, seed=4), rnd(B, C, L, seed=5)
    stats = refs.gn_stats(x, G).float()
    dx_ref, dg_ref, db_ref, dsx, ds = refs.gn_silu_bwd(x, dact, G, gamma, beta)
    dx_ref = dx_ref + dres.double()
    base_g, base_b = rnd(C, seed=6), rnd(C, seed=7)
    if acc:
        dg_ref, db_ref = dg_ref + base_g.double(), db_ref + base_b.double()
    NSab = 3   # the first stage as a conv epilogue would leave it: any partition of the row
    edges = [round(i * L / NSab) for i in range(NSab + 1)]
    ab_in = torch.stack([torch.stack([dsx[:, :, edges[e]:edges[e + 1]].sum(-1), ds[:, :, edges[e]:edges[e + 1]].sum(-1)], -1)
                         for e in range(NSab)], 2).float()   # [B, C, NSab, 2]

    def run(P):
        L_ = _C.lib()
        NS = P.val(L_.adp_row_nsplit(B * C, L), "adp_row_nsplit")
        xd, dd, sd = P.inp("x", x), P.inp("dact", dact), P.inp("stats", stats)
        ga, be, rd = P.inp("gamma", gamma), P.inp("beta", beta), P.inp("dres", dres, res=True)
        abi = P.inp("ab_in", ab_in)
        ab = P.out("ab", (B, C, NS, 2))
        s = stream()
        P.ok(L_.adp_gn_silu_bwd_reduce(p(xd), p(dd), p(sd), p(ga), p(be), B, C, L, G, NS, p(ab), s), "adp_gn_silu_bwd_reduce")
        outs = []
        for tag, fn in (("apply", lambda dx, dg, db: L_.adp_gn_silu_bwd_apply(
                p(xd), p(dd), p(sd), p(ga), p(be), p(ab), p(rd), B, C, L, G, NS, p(dx), p(dg), p(db), acc, s)),
                        ("apply_ab", lambda dx, dg, db: L_.adp_gn_silu_bwd_apply_ab(
                p(xd), p(dd), p(sd), p(ga), p(be), p(abi), p(rd), B, C, L, G, NS, NSab, p(dx), p(dg), p(db), acc, s))):
            dx = P.out(f"dx_{tag}", (B, C, L))
            dg = P.inout(f"dgamma_{tag}", base_g) if acc else P.out(f"dgamma_{tag}", (C,))
            db = P.inout(f"dbeta_{tag}", base_b) if acc else P.out(f"dbeta_{tag}", (C,))
            P.ok(fn(dx, dg, db), f"adp_gn_silu_bwd_{tag}")
            outs += [(f"dx_{tag}", dx, dx_ref, TOL), (f"dgamma_{tag}", dg, dg_ref, TOL), (f"dbeta_{tag}", db, db_ref, TOL)]
        dg = P.inout("dgamma_pg", base_g) if acc else P.out("dgamma_pg", (C,))
        db = P.inout("dbeta_pg", base_b) if acc else P.out("dbeta_pg", (C,))
        P.ok(L_.adp_gn_param_grad(p(abi), B, C, NSab, p(dg), p(db), acc, s), "adp_gn_param_grad")
        return outs + [("ab", ab.cpu().double().sum(2), torch.stack([dsx.sum(-1), ds.sum(-1)], -1), TOL),
                       ("dgamma_pg", dg, dg_ref, TOL), ("dbeta_pg", db, db_ref, TOL)]
    return run


# ---------------------------------------------------------------------------------------------------- Modulation / LayerNorm
def _mod_data(B, C, L):
    x = rnd(B, C, L, seed=1) * 1.5 + 0.4
    bs = 2 * C + 7
    ss = rnd(B, 2 * C, seed=2) * 0.5
    return x, bs, ss, to_rows(ss, bs)


MOD_SHAPES = [dict(B=2, C=32, L=72), dict(B=2, C=8, L=301), dict(B=1, C=130, L=64), dict(B=2, C=100, L=50)]


@case(("adp_modulation_fwd", "adp_modulation_ln_fwd", "adp_ln_stats", "adp_ln_affine_fwd"), MOD_SHAPES)
def modulation_fwd(B, C, L):
    x, bs, ss, ssf = _mod_data(B, C, L)
    g1, b1, g2, b2 = (rnd(C, seed=10 + i) * 0.5 + (1.0 if i % 2 == 0 else 0.0) for i in range(4))
    y_ref = refs.modulation(x, ss[:, :C], ss[:, C:])
    st_ref = refs.ln_stats(x)
    lst_ref = refs.ln_stats(y_ref)
    xn_ref, xn2_ref = refs.ln_chan(y_ref, g1, b1), refs.ln_chan(y_ref, g2, b2)
    lx_ref, lx2_ref = refs.ln_chan(x, g1, b1), refs.ln_chan(x, g2, b2)

    def run(P):
        L_ = _C.lib()
        s = stream()
        xd, sd = P.inp("x", x), P.inp("ss", ssf)
        g1d, b1d, g2d, b2d = P.inp("gamma", g1), P.inp("beta", b1), P.inp("gamma2", g2), P.inp("beta2", b2)
        y, st = P.out("y", (B, C, L)), P.out("stats", (B, L, 2))
        P.ok(L_.adp_modulation_fwd(p(xd), p(sd), bs, B, C, L, 1e-5, p(y), p(st), s), "adp_modulation_fwd")
        y2, st2 = P.out("y_ln", (B, C, L)), P.out("stats_ln", (B, L, 2))
        xn, xn2, lst = P.out("xn", (B, C, L)), P.out("xn2", (B, C, L)), P.out("ln_stats", (B, L, 2))
        P.ok(L_.adp_modulation_ln_fwd(p(xd), p(sd), bs, B, C, L, 1e-5, p(y2), p(st2), 1e-5, p(g1d), p(b1d), p(xn), p(g2d),
                                      p(b2d), p(xn2), p(lst), s), "adp_modulation_ln_fwd")
        st3 = P.out("stats_only", (B, L, 2))
        P.ok(L_.adp_ln_stats(p(xd), B, C, L, 1e-5, p(st3), s), "adp_ln_stats")
        ly, ly2, st4 = P.out("ln_y", (B, C, L)), P.out("ln_y2", (B, C, L)), P.out("ln_affine_stats", (B, L, 2))
        P.ok(L_.adp_ln_affine_fwd(p(xd), B, C, L, 1e-5, p(g1d), p(b1d), p(ly), p(g2d), p(b2d), p(ly2), p(st4), s),
             "adp_ln_affine_fwd")
        return [("y", y, y_ref, TOL), ("stats", st, st_ref, TOL), ("y_ln", y2, y_ref, TOL), ("stats_ln", st2, st_ref, TOL),
                ("xn", xn, xn_ref, TOL), ("xn2", xn2, xn2_ref, TOL), ("ln_stats", lst, lst_ref, TOL),
                ("stats_only", st3, st_ref, TOL), ("ln_y", ly, lx_ref, TOL), ("ln_y2", ly2, lx2_ref, TOL),
                ("ln_affine_stats", st4, st_ref, TOL)]
    return run


@case(("adp_modulation_bwd", "adp_modulation_bwd_partial", "adp_modulation_bwd_reduce", "adp_modulation_ln_bwd_partial",
       "adp_ln_bwd"), MOD_SHAPES)
def modulation_bwd(B, C, L):
    x, bs, ss, ssf = _mod_data(B, C, L)
    g1 = rnd(C, seed=10) * 0.5 + 1.0
    dy, dres = rnd(B, C, L, seed=3), rnd(B, C, L, seed=4)
    xr, sr, gr = x.double().requires_grad_(), ss.double().requires_grad_(), g1.double().requires_grad_()
    br = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    y = refs.modulation(xr, sr[:, :C], sr[:, C:])
    dx_ref, dss_ref = torch.autograd.grad(y, (xr, sr), dy.double(), retain_graph=True)
    xn = refs.ln_chan(y, gr, br)
    dxc_ref, dssc_ref, dgc_ref, dbc_ref = torch.autograd.grad((xn * dy.double()).sum() + (y * dres.double()).sum(),
                                                              (xr, sr, gr, br))
    # adp_ln_bwd alone: LayerNorm with affine of x
    xr2 = x.double().requires_grad_()
    xn2 = refs.ln_chan(xr2, gr, br)
    dxl_ref, dgl_ref, dbl_ref = torch.autograd.grad(xn2, (xr2, gr, br), dy.double())
    dxl_ref = dxl_ref + dres.double()
    st = refs.ln_stats(x).float()
    y32 = y.detach().float()
    lst = refs.ln_stats(y32).float()
    written = strided_rows(B, 2 * C, bs)

    def run(P):
        L_ = _C.lib()
        s = stream()
        xd, dyd, sd, std = P.inp("x", x), P.inp("dy", dy), P.inp("ss", ssf), P.inp("stats", st)
        yd, lsd, gd, rd = P.inp("y", y32), P.inp("ln_stats", lst), P.inp("gamma", g1), P.inp("dres", dres, res=True)
        nws = L_.adp_chan_ln_bwd_ws_bytes(B, C, L)
        # one call
        dx, dss, ws = P.out("dx", (B, C, L)), P.out("dss", (written.numel(),), written=written), P.ws("ws", nws)
        P.ok(L_.adp_modulation_bwd(p(xd), p(dyd), p(sd), bs, p(std), B, C, L, p(dx), p(dss), bs, p(ws), s), "adp_modulation_bwd")
        # the two stages
        dx2, dss2, ws2 = P.out("dx_partial", (B, C, L)), P.out("dss_reduce", (written.numel(),), written=written), P.ws("ws_partial", nws)
        NT = P.val(L_.adp_modulation_bwd_partial(p(xd), p(dyd), p(sd), bs, p(std), B, C, L, p(dx2), p(ws2), s),
                   "adp_modulation_bwd_partial")
        arr = ctypes.c_void_p * 1
        P.ok(L_.adp_modulation_bwd_reduce(arr(p(ws2)), arr(p(dss2)), 1, B, C, NT, bs, s), "adp_modulation_bwd_reduce")
        # chained with the attention item's LayerNorm
        dx3, dss3 = P.out("dx_chain", (B, C, L)), P.out("dss_chain", (written.numel(),), written=written)
        ws3, ws3l, dgb = P.ws("ws_chain", nws), P.ws("ws_ln", nws), P.out("dgamma_dbeta", (2 * C,))
        NT3 = P.val(L_.adp_modulation_ln_bwd_partial(p(xd), p(sd), bs, p(std), p(yd), p(dyd), p(gd), p(lsd), p(rd), B, C, L, 0,
                                                     p(dx3), p(ws3), p(dgb), p(ws3l), s), "adp_modulation_ln_bwd_partial")
        P.ok(L_.adp_modulation_bwd_reduce(arr(p(ws3)), arr(p(dss3)), 1, B, C, NT3, bs, s), "adp_modulation_bwd_reduce")
        # LayerNorm backward alone
        dx4, dgb4, ws4 = P.out("dx_ln", (B, C, L)), P.out("dgb_ln", (2 * C,)), P.ws("ws_lnb", nws)
        P.ok(L_.adp_ln_bwd(p(xd), p(dyd), p(std), p(gd), p(rd), B, C, L, 0, p(dx4), p(dgb4), p(ws4), s), "adp_ln_bwd")
        rows = lambda t: from_rows(t, B, 2 * C, bs)  # noqa: E731
        return [("dx", dx, dx_ref, TOL), ("dss", rows(dss), dss_ref, TOL), ("dx_partial", dx2, dx_ref, TOL),
                ("dss_reduce", rows(dss2), dss_ref, TOL), ("dx_chain", dx3, dxc_ref, TOL), ("dss_chain", rows(dss3), dssc_ref, TOL),
                ("dgamma_chain", dgb[:C], dgc_ref, TOL), ("dbeta_chain", dgb[C:], dbc_ref, TOL), ("dx_ln", dx4, dxl_ref, TOL),
                ("dgamma_ln", dgb4[:C], dgl_ref, TOL), ("dbeta_ln", dgb4[C:], dbl_ref, TOL)]
    return run


# ---------------------------------------------------------------------------------------------------- conditioning path
@case(("adp_linear_fwd", "adp_linear_bwd_data", "adp_linear_bwd_weight", "adp_act_fwd", "adp_act_bwd"),
      [dict(B=4, K=1024, N=36, a=1, post=0), dict(B=1, K=257, N=64, a=0, post=2), dict(B=8, K=1500, N=21, a=2, post=0),
       dict(B=3, K=64, N=4100, a=1, post=0, acc=1)])
def linear(B, K, N, a, post, acc=0):
    x, w, b, dy = rnd(B, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3), rnd(B, N, seed=4)
    xr = x.double().requires_grad_()
    wr, br = w.double().requires_grad_(), b.double().requires_grad_()
    xa = refs.act(xr, a)
    y = F.linear(xa, wr, br)
    yp = F.gelu(y) if post == 2 else y
    dxa_ref, dw_ref, db_ref = torch.autograd.grad(y, (xa, wr, br), dy.double(), retain_graph=True)
    (dx_ref,) = torch.autograd.grad(xa, xr, dy.double()[:, :1].expand(B, K).contiguous())
    base_w, base_b, base_x = rnd(N, K, seed=5), rnd(N, seed=6), rnd(B, K, seed=7)
    if acc:
        dxa_ref, dw_ref, db_ref = dxa_ref + base_x.double(), dw_ref + base_w.double(), db_ref + base_b.double()
        dx_ref = dx_ref + base_x.double()
    ybs = N + 3
    written = strided_rows(B, N, ybs)
    gact = dy[:, :1].expand(B, K).contiguous()

    def run(P):
        L_ = _C.lib()
        s = stream()
        xd, wd, bd, dyd = P.inp("x", x), P.inp("w", w), P.inp("bias", b), P.inp("dy", to_rows(dy, ybs))
        yd = P.out("y", (written.numel(),), written=written)
        P.ok(L_.adp_linear_fwd(p(xd), p(wd), p(bd), B, K, N, a, post, p(yd), ybs, s), "adp_linear_fwd")
        dxa = P.inout("dxa", base_x) if acc else P.out("dxa", (B, K))
        ws = P.ws("ws", L_.adp_linear_bwd_data_ws_bytes(B, K, N))
        P.ok(L_.adp_linear_bwd_data(p(dyd), ybs, p(wd), B, K, N, acc, p(dxa), p(ws), s), "adp_linear_bwd_data")
        dw = P.inout("dw", base_w) if acc else P.out("dw", (N, K))
        db = P.inout("dbias", base_b) if acc else P.out("dbias", (N,))
        P.ok(L_.adp_linear_bwd_weight(p(dyd), ybs, p(xd), B, K, N, a, acc, p(dw), p(db), s), "adp_linear_bwd_weight")
        ya = P.out("act_y", (B, K))
        P.ok(L_.adp_act_fwd(p(xd), B * K, a, p(ya), s), "adp_act_fwd")
        gd = P.inp("act_dy", gact)
        dx = P.inout("act_dx", base_x) if acc else P.out("act_dx", (B, K))
        P.ok(L_.adp_act_bwd(p(xd), p(gd), B * K, a, acc, p(dx), s), "adp_act_bwd")
        return [("y", from_rows(yd, B, N, ybs), yp, TOL), ("dxa", dxa, dxa_ref, TOL), ("dw", dw, dw_ref, TOL),
                ("dbias", db, db_ref, TOL), ("act_y", ya, xa, TOL), ("act_dx", dx, dx_ref, TOL)]
    return run


@case(("adp_time_fourier_fwd", "adp_time_fourier_bwd"), [dict(B=3, H=128), dict(B=2, H=33, acc=1)])
def time_fourier(B, H, acc=0):
    t = torch.tensor([0.0, 0.31, 1.0])[:B]
    w, dfour, base = rnd(H, seed=1), rnd(B, 2 * H + 1, seed=2), rnd(H, seed=3)
    wr = w.double().requires_grad_()
    four = refs.time_fourier(t, wr)
    (dw_ref,) = torch.autograd.grad(four, wr, dfour.double())
    if acc:
        dw_ref = dw_ref + base.double()

    def run(P):
        L_ = _C.lib()
        td, wd, dfd = P.inp("t", t), P.inp("w", w), P.inp("dfour", dfour)
        fo = P.out("four", (B, 2 * H + 1))
        dw = P.inout("dw", base) if acc else P.out("dw", (H,))
        P.ok(L_.adp_time_fourier_fwd(p(td), p(wd), B, H, p(fo), stream()), "adp_time_fourier_fwd")
        P.ok(L_.adp_time_fourier_bwd(p(td), p(wd), p(dfd), B, H, acc, p(dw), stream()), "adp_time_fourier_bwd")
        return [("four", fo, four, 1e-5), ("dw", dw, dw_ref, TOL)]
    return run


@case("adp_skipmod_bwd", [dict(B=2, C=8, L=2500), dict(B=2, C=6, L=333)])
def skipmod_bwd(B, C, L):
    g, x, sc = rnd(B, C, L, seed=1), rnd(B, C, L, seed=2), rnd(B, C, seed=3)
    bs = C + 5
    written = strided_rows(B, C, bs)
    dx_ref, ds_ref = sc.double()[:, :, None] * g.double(), (g.double() * x.double()).sum(-1)

    def run(P):
        L_ = _C.lib()
        gd, xd, sd = P.inp("g", g), P.inp("x", x), P.inp("scale", to_rows(sc, bs))
        dx, ds = P.out("dx", (B, C, L)), P.out("dscale", (written.numel(),), written=written)
        ws = P.ws("ws", L_.adp_skipmod_bwd_ws_bytes(B, C, L))
        P.ok(L_.adp_skipmod_bwd(p(gd), p(xd), p(sd), bs, B, C, L, p(dx), p(ds), bs, p(ws), stream()), "adp_skipmod_bwd")
        return [("dx", dx, dx_ref, TOL), ("dscale", from_rows(ds, B, C, bs), ds_ref, TOL)]
    return run


# ---------------------------------------------------------------------------------------------------- v-objective, samplers
@case(("adp_v_noise", "adp_mse_fwd", "adp_mse_bwd", "adp_v_step", "adp_v_step2", "adp_v_inpaint_step", "adp_cfg_mix",
       "adp_select_rows", "adp_add", "adp_axpby"), [dict(B=4, per=2048), dict(B=3, per=1001)])
def elementwise(B, per):
    n = B * per
    x, v, h0, h1 = rnd(B, per, seed=1), rnd(B, per, seed=2), rnd(B, per, seed=3), rnd(B, per, seed=4)
    sig = torch.tensor([0.0, 0.37, 1.0, 0.6])[:B]
    ang = sig.double()[:, None] * math.pi / 2
    ca, sa = torch.cos(ang), torch.sin(ang)
    xd64, vd64 = x.double(), v.double()
    gl = torch.tensor([0.7])
    ab4 = torch.tensor([0.3, 0.9, 0.5, 0.8])
    c6 = torch.tensor([0.3, 0.9, 0.5, 0.8, 0.25, -0.4])
    a0, b0, a1, b1, cca, ccb = (float(c) for c in c6.double())
    x0, eps = a0 * xd64 - b0 * vd64, b0 * xd64 + a0 * vd64
    step2 = a1 * x0 + b1 * eps + cca * (x0 - h0.double()) + ccb * (eps - h1.double())
    mask = (rnd(B, per, seed=5) > 0).to(torch.uint8)
    pick = torch.tensor([1, 0, 1, 1], dtype=torch.uint8)[:B]
    half = (B // 2) * per

    def run(P):
        L_ = _C.lib()
        s = stream()
        xd, vd, h0d, h1d = P.inp("x", x), P.inp("v", v), P.inp("hist_x0", h0), P.inp("hist_eps", h1)
        sd, gd, a4, c6d = P.inp("sigma", sig), P.inp("gloss", gl), P.inp("ab4", ab4), P.inp("coef6", c6)
        md, pd = P.inp("mask", mask), P.inp("pick", pick)
        o = {k: P.out(k, (B, per)) for k in ("x_noisy", "v_target", "dv", "step", "step2", "hx0_out", "heps_out", "inpaint",
                                             "select", "add", "axpby", "ax")}
        loss, mix = P.out("loss", (1,)), P.out("cfg", (half,))
        ws = P.ws("ws", L_.adp_mse_ws_bytes(n))
        P.ok(L_.adp_v_noise(p(xd), p(vd), p(sd), B, per, p(o["x_noisy"]), p(o["v_target"]), s), "adp_v_noise")
        P.ok(L_.adp_mse_fwd(p(xd), p(vd), n, p(loss), p(ws), s), "adp_mse_fwd")
        P.ok(L_.adp_mse_bwd(p(xd), p(vd), p(gd), n, p(o["dv"]), s), "adp_mse_bwd")
        P.ok(L_.adp_v_step(p(xd), p(vd), p(a4), n, p(o["step"]), s), "adp_v_step")
        P.ok(L_.adp_v_step2(p(xd), p(vd), p(h0d), p(h1d), p(c6d), n, p(o["step2"]), p(o["hx0_out"]), p(o["heps_out"]), s),
             "adp_v_step2")
        P.ok(L_.adp_v_inpaint_step(p(xd), p(vd), p(h0d), p(h1d), p(md), p(a4), n, p(o["inpaint"]), s), "adp_v_inpaint_step")
        P.ok(L_.adp_cfg_mix(p(xd), half, 1.75, p(mix), s), "adp_cfg_mix")
        P.ok(L_.adp_select_rows(p(xd), p(vd), p(pd), B, per, p(o["select"]), s), "adp_select_rows")
        P.ok(L_.adp_add(p(xd), p(vd), n, p(o["add"]), s), "adp_add")
        P.ok(L_.adp_axpby(0.5, p(xd), -2.0, p(vd), n, p(o["axpby"]), s), "adp_axpby")
        P.ok(L_.adp_axpby(0.5, p(xd), 0.0, None, n, p(o["ax"]), s), "adp_axpby")
        st = refs.v_step(x, v, 0.3, 0.9, 0.5, 0.8)
        flat = xd64.reshape(-1)
        e = 1e-6   # the bound of test_v_noise_mse_step / test_unshuffle_and_pool_sum
        return [("x_noisy", o["x_noisy"], ca * xd64 + sa * vd64, e), ("v_target", o["v_target"], ca * vd64 - sa * xd64, e),
                ("loss", loss, ((xd64 - vd64) ** 2).mean().reshape(1), e), ("dv", o["dv"], 2 * (xd64 - vd64) / n * 0.7, e),
                ("step", o["step"], st, e), ("step2", o["step2"], step2, e), ("hx0_out", o["hx0_out"], x0, e),
                ("heps_out", o["heps_out"], eps, e),
                ("inpaint", o["inpaint"], torch.where(mask.bool(), 0.5 * h0.double() + 0.8 * h1.double(), st), e),
                ("cfg", mix, flat[half:2 * half] + (flat[:half] - flat[half:2 * half]) * 1.75, e),
                ("select", o["select"], torch.where(pick.bool()[:, None], xd64, vd64), e), ("add", o["add"], xd64 + vd64, e),
                ("axpby", o["axpby"], 0.5 * xd64 - 2.0 * vd64, e), ("ax", o["ax"], 0.5 * xd64, e)]
    return run


@case(("adp_copy2d", "adp_unshuffle", "adp_pool_sum"), [dict(rows=6, L=64, f=4), dict(rows=5, L=51, f=3)])
def index_helpers(rows, L, f):
    x, r = rnd(rows, L, seed=1), rnd(rows, L // f, seed=2)
    cols, dstride = L - 3, L + 5
    written = strided_rows(rows, cols, dstride)
    xs = x[:, :L // f * f]

    def run(P):
        L_ = _C.lib()
        s = stream()
        xd, rd = P.inp("x", x), P.inp("res", r, res=True)
        xsd = P.inp("xs", xs.contiguous())
        dst = P.out("dst", (written.numel(),), written=written)
        un, pool = P.out("unshuffle", (rows * f, L // f)), P.out("pool", (rows, L // f))
        P.ok(L_.adp_copy2d(p(xd), L, p(dst), dstride, rows, cols, s), "adp_copy2d")
        P.ok(L_.adp_unshuffle(p(xsd), rows, L // f * f, f, p(un), s), "adp_unshuffle")
        P.ok(L_.adp_pool_sum(p(xsd), rows, L // f, f, p(rd), p(pool), s), "adp_pool_sum")
        v = xs.double().reshape(rows, L // f, f)
        return [("dst", from_rows(dst, rows, cols, dstride), x[:, :cols].double(), 1e-6),
                ("unshuffle", un, v.permute(0, 2, 1).reshape(rows * f, L // f), 1e-6),
                ("pool", pool, v.sum(-1) + r.double(), 1e-6)]
    return run


# ---------------------------------------------------------------------------------------------------- attention
@case(("adp_attn_fwd", "adp_attn_bwd"), [
    # want: the kernels the aligned placement must launch, i.e. the mode the switches are meant to force
    dict(B=2, H=2, D=64, n=160, m=160, env={"ADP_ATTN_FEWKEYS": "0"},
         want=["attn_fwd_kernel<true>", "attn_fwd_combine_kernel", "attn_bwd_merged_kernel<true>"]),
    dict(B=2, H=1, D=16, n=203, m=37, env={"ADP_ATTN_FEWKEYS": "0", "ADP_ATTN_MERGE": "0"},
         want=["attn_fwd_kernel<false>", "attn_bwd_q_kernel<false>", "attn_bwd_kv_kernel<false>", "attn_kv_reduce_kernel"]),
    dict(B=1, H=2, D=64, n=64, m=20, env={"ADP_ATTN_FEWKEYS": "1"}, want=["attn_fwd_fewkeys_kernel", "attn_bwd_fewkeys_kernel"]),
    dict(B=2, H=2, D=64, n=72, m=45, env={"ADP_ATTN_FEWKEYS": "1"}, want=["attn_fwd_fewkeys_kernel", "attn_bwd_fewkeys_kernel"]),
    # packed q (what ops.attn_bwd passes): the key-split dq pass with its partial copies in ws and the reduce launch
    dict(B=1, H=2, D=64, n=96, m=256, packed=1, env={"ADP_ATTN_FEWKEYS": "0", "ADP_ATTN_MERGE": "0"},
         want=["attn_bwd_q_kernel<true>", "attn_sum_splits_kernel", "attn_bwd_kv_kernel<true>"]),
])
def attention(B, H, D, n, m, want, packed=0):
    """Batch strides larger than the tensors: q / dq rows q_bstride apart (o, dout and lse are packed), k | v (and
    dk | dv) as the two halves of rows kv_bstride apart, as ops.attn_fwd passes the halves of one projection output."""
    mid = H * D
    qbs, kvbs = mid * n + (0 if packed else 8), 2 * mid * m
    q, k, v, do = rnd(B, mid * n, seed=1), rnd(B, mid * m, seed=2), rnd(B, mid * m, seed=3), rnd(B, mid * n, seed=4)
    qr, kr, vr = (t.double().requires_grad_() for t in (q, k, v))
    o_ref, lse_ref = refs.attention(qr.view(B, mid, n), kr.view(B, mid, m), vr.view(B, mid, m), H, D)
    dq_ref, dk_ref, dv_ref = torch.autograd.grad(o_ref, (qr, kr, vr), do.double().view(B, mid, n))
    kv = torch.cat([k, v], 1)                                   # [B, 2 * mid * m]: kv_bstride = the packed row
    wq = strided_rows(B, mid * n, qbs)

    def run(P):
        L_ = _C.lib()
        s = stream()
        qd, kvd = P.inp("q", to_rows(q, qbs)), P.inp("kv", kv)
        o, lse = P.out("o", (B, mid * n)), P.out("lse", (B, H, n))
        need = L_.adp_attn_fwd_ws_bytes(B, H, D, n, m)
        ws = P.ws("ws_fwd", need) if need > 0 else None
        kvf = kvd.view(-1)
        P.call("adp_attn_fwd", lambda: L_.adp_attn_fwd(p(qd), p(kvf), p(kvf[mid * m:]), B, H, D, n, m, qbs, kvbs, p(o), p(lse),
                                                       p(ws), s))
        od = P.inp("o_in", o_ref.detach().float().reshape(B, -1))
        dod, lsd = P.inp("dout", do), P.inp("lse_in", lse_ref.detach().float())
        dq, dkv = P.out("dq", (wq.numel(),), written=wq), P.out("dkv", (B, 2 * mid * m))
        wsb = P.ws("ws_bwd", L_.adp_attn_bwd_ws_bytes(B, H, D, n, m))
        dkvf = dkv.view(-1)
        P.call("adp_attn_bwd", lambda: L_.adp_attn_bwd(p(qd), p(kvf), p(kvf[mid * m:]), p(od), p(dod), p(lsd), B, H, D, n, m, qbs,
                                                       kvbs, p(dq), p(dkvf), p(dkvf[mid * m:]), p(wsb), s))
        return [("o", o, o_ref.reshape(B, -1), TOL), ("lse", lse, lse_ref, 1e-5),
                ("dq", from_rows(dq, B, mid * n, qbs), dq_ref, TOL), ("dk", dkv[:, :mid * m], dk_ref, TOL),
                ("dv", dkv[:, mid * m:], dv_ref, TOL)]

    run.want_kernels = want
    return run


@case(("adp_ctx_fold_fwd", "adp_ctx_fold_bwd"), [dict(I=3, M2=16, E=12), dict(I=2, M2=40, E=70), dict(I=5, M2=64, E=33)])
def ctx_fold(I, M2, E):
    W = [rnd(M2, E, seed=10 + i) for i in range(I)]
    ga = [rnd(E, seed=20 + i) for i in range(I)]
    be = [rnd(E, seed=30 + i) for i in range(I)]
    dw_all, db_all = rnd(I * M2, E, seed=40), rnd(I * M2, seed=41)
    per = M2 * E + 2 * E + 5
    dgb_off = torch.tensor([3 + i * per for i in range(I)], dtype=torch.int64)
    dw_off = dgb_off + 2 * E + 5
    written = torch.zeros(I * per + 3, dtype=torch.bool)
    flat_ref = torch.zeros(I * per + 3, dtype=torch.float64)
    for i in range(I):
        a = 3 + i * per
        dW, db = dw_all[i * M2:(i + 1) * M2].double(), db_all[i * M2:(i + 1) * M2].double()
        written[a:a + 2 * E] = True
        written[a + 2 * E + 5:a + per] = True
        flat_ref[a:a + E] = (dW * W[i].double()).sum(0)
        flat_ref[a + E:a + 2 * E] = db @ W[i].double()
        flat_ref[a + 2 * E + 5:a + per] = (dW * ga[i].double()[None] + db[:, None] * be[i].double()[None]).reshape(-1)
    w_ref = torch.cat([W[i].double() * ga[i].double()[None] for i in range(I)])
    b_ref = torch.cat([W[i].double() @ be[i].double() for i in range(I)])

    def run(P):
        L_ = _C.lib()
        s = stream()
        Wd = [P.inp(f"w{i}", W[i]) for i in range(I)]
        gd = [P.inp(f"gamma{i}", ga[i]) for i in range(I)]
        bd = [P.inp(f"beta{i}", be[i]) for i in range(I)]
        tabs = [P.inp(nm, torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64))
                for nm, ts in (("w_table", Wd), ("gamma_table", gd), ("beta_table", bd))]
        wa, ba = P.out("w_all", (I * M2, E)), P.out("bias_all", (I * M2,))
        P.ok(L_.adp_ctx_fold_fwd(p(tabs[0]), p(tabs[1]), p(tabs[2]), I, M2, E, p(wa), p(ba), s), "adp_ctx_fold_fwd")
        dwd, dbd = P.inp("dw_all", dw_all), P.inp("dbias_all", db_all)
        flat = P.out("flat", (written.numel(),), written=written)
        o1, o2 = P.inp("dw_off", dw_off), P.inp("dgb_off", dgb_off)
        P.ok(L_.adp_ctx_fold_bwd(p(tabs[0]), p(tabs[1]), p(tabs[2]), p(dwd), p(dbd), I, M2, E, p(flat), p(o1), p(o2), s),
             "adp_ctx_fold_bwd")
        out, fl = [("w_all", wa, w_ref, TOL), ("bias_all", ba, b_ref, TOL)], flat.cpu().double()
        for i in range(I):   # each item's dW, dgamma and dbeta against its own scale, as test_ctx_fold_fwd_bwd does
            a = 3 + i * per
            for nm, lo, hi in (("dgamma", a, a + E), ("dbeta", a + E, a + 2 * E), ("dW", a + 2 * E + 5, a + per)):
                out.append((f"{nm}{i}", fl[lo:hi], flat_ref[lo:hi], TOL))
        return out
    return run


# ---------------------------------------------------------------------------------------------------- audio front / back ends
@case("adp_resample", [dict(rows=4, length=256, fi=2, fo=3), dict(rows=3, length=203, fi=3, fo=2), dict(rows=2, length=130, fi=1, fo=4)])
def resample(rows, length, fi, fo):
    width = 6
    J = 2 * width + fi
    kern = rnd(fo, J, seed=2, scale=J ** -0.5)
    x = rnd(rows, length, seed=1)
    out_len = int(fo * length / fi)
    want = refs.resample(x, kern, fi, fo, width, out_len)

    def run(P):
        L_ = _C.lib()
        xd, kd, o = P.inp("x", x), P.inp("kern", kern), P.out("out", (rows, out_len))
        P.ok(L_.adp_resample(p(xd), p(kd), rows, length, fi, fo, J, width, out_len, p(o), stream()), "adp_resample")
        return [("out", o, want, TOL)]
    return run


@case(("adp_stft_loss_fwd", "adp_stft_loss_bwd"), [dict(rows=2, length=1024, eps=1e-4), dict(rows=3, length=701, eps=1e-4),
                                                     dict(rows=3, length=703, eps=1e-8)])
def stft_loss(rows, length, eps):
    """The log term's gradient carries 1 / m, so the rounding of a nearly-vanishing bin is amplified by 1 / m and one such
    bin of a random input decides the max-norm error of the whole gradient.  At rows x length 3 x 701 and the default
    eps = 1e-8 the kernels are at 1.098e-3 of the float64 gradient, at every placement, the aligned one included: samples
    695-699 of row 0, from the DC bin of the last frame with |X|^2 = 2e-7 (float32 torch is at 2.7e-5 there and at 1.1e-4
    over the tensor; the kernels' median error equals float32 torch's).  That is the conditioning of the problem, not a
    placement matter, and GRAD_TOL stays as test_stft_loss.py sets it; so the first two shapes clamp the magnitudes at 1e-2
    (eps = 1e-4: magnitudes are of order 10, the amplification of float32 rounding is bounded near 1e3 x 1e-7), and the
    third keeps the public default eps on an input that is well conditioned by the reference's own measure.  That measure
    is asserted below for every shape: the float32 torch restatement must be within GRAD_TOL / 10 of the float64 one."""
    from test_stft_loss import GRAD_TOL, LOSS_TOL, mrstft_ref
    EPS = eps
    res = ((256, 30, 150), (128, 13, 64))
    g = torch.Generator().manual_seed(0)
    y = torch.randn(rows, length, generator=g)
    x = y + 0.3 * torch.randn(rows, length, generator=g)
    xr = x.double().requires_grad_()
    ref = mrstft_ref(xr, y, res, 1.0, 1.0, 0.5, EPS)
    (dx_ref,) = torch.autograd.grad(ref, xr)
    x32 = x.clone().requires_grad_()
    (dx32,) = torch.autograd.grad(mrstft_ref(x32, y, res, 1.0, 1.0, 0.5, EPS, dtype=torch.float32), x32)
    assert rel_err(dx32, dx_ref) < GRAD_TOL / 10, "this input is ill conditioned: pick another for a placement test"
    gl = torch.tensor([0.7])
    arr = (ctypes.c_int64 * 6)(*[v for r in res for v in r])

    def run(P):
        L_ = _C.lib()
        s = stream()
        xd, yd, gd = P.inp("x", x), P.inp("y", y), P.inp("gloss", gl)
        loss, dx = P.out("loss", (1,)), P.out("dx", (rows, length))
        wsf = P.ws("ws_fwd", P.val(L_.adp_stft_loss_ws_bytes(rows, length, 2, arr, 0), "adp_stft_loss_ws_bytes"))
        wsb = P.ws("ws_bwd", P.val(L_.adp_stft_loss_ws_bytes(rows, length, 2, arr, 1), "adp_stft_loss_ws_bytes"))
        P.ok(L_.adp_stft_loss_fwd(p(xd), p(yd), rows, length, 2, arr, 1.0, 1.0, 0.5, EPS, p(loss), p(wsf), s), "adp_stft_loss_fwd")
        P.ok(L_.adp_stft_loss_bwd(p(xd), p(yd), p(gd), p(wsf), rows, length, 2, arr, 1.0, 1.0, 0.5, EPS, p(dx), p(wsb), s),
             "adp_stft_loss_bwd")
        return [("loss", loss, ref.detach().reshape(1), LOSS_TOL), ("dx", dx, 0.7 * dx_ref, GRAD_TOL)]
    return run


@case("adp_mel_spectrogram", [dict(n_fft=256, hop=64, win=256, sr=16000, n_mels=32, T=4096, norm=0, log=0),
                              dict(n_fft=64, hop=16, win=64, sr=8000, n_mels=8, T=2050, norm=1, log=1),
                              dict(n_fft=512, hop=128, win=400, sr=22050, n_mels=40, T=3001, norm=0, log=1)])
def mel(n_fft, hop, win, sr, n_mels, T, norm, log):
    from audio_diffusion_pytorch_amd import vocoder
    from test_vocoder import MARGIN, mel_ref, wave
    rows = 3
    x = wave((rows, T), seed=n_fft)
    want = mel_ref(x, n_fft, hop, win, sr, n_mels, bool(norm), bool(log))
    # the entry point's own bound: MARGIN x the error of the same restatement in float32 (test_mel_matches_restatement)
    yard = rel_err(mel_ref(x, n_fft, hop, win, sr, n_mels, bool(norm), bool(log), dtype=torch.float32), want)
    m = vocoder.MelSpectrogram(n_fft, hop, win, sr, n_mels)
    fb, rng = m.fb.detach().cpu().float(), m.fb_range.detach().cpu().to(torch.int32)

    def run(P):
        L_ = _C.lib()
        xd, fd, rd = P.inp("x", x), P.inp("fb", fb), P.inp("range", rng)
        frames = P.val(L_.adp_mel_frames(T, n_fft, hop), "adp_mel_frames")
        o = P.out("out", (rows, n_mels, frames))
        ws = P.ws("ws", L_.adp_mel_spectrogram_ws_bytes(rows, T, n_fft, hop, win, n_mels)) if norm else None
        P.ok(L_.adp_mel_spectrogram(p(xd), p(fd), p(rd), rows, T, n_fft, hop, win, n_mels, norm, log, p(o), p(ws), stream()),
             "adp_mel_spectrogram")
        return [("out", o, want, MARGIN * yard)]
    return run


@case(("adp_tflat_fwd", "adp_tflat_wgrad"), [dict(M=32, K=256, hop=64, L=40), dict(M=5, K=7, hop=3, L=45),
                                               dict(M=8, K=64, hop=16, L=131)])
def tflat(M, K, hop, L):
    from test_vocoder import MARGIN
    g = torch.Generator().manual_seed(M)
    N, pad = 3, (K - hop) // 2
    spec, w = torch.randn(N, M, L, generator=g), torch.randn(M, 1, K, generator=g) / math.sqrt(M)
    Lout = (L - 1) * hop - 2 * pad + K
    gout = torch.randn(N, 1, Lout, generator=g)

    def side(dtype):
        wd = w.to(dtype).requires_grad_(True)
        y = F.conv_transpose1d(spec.to(dtype), wd, stride=hop, padding=pad)
        y.backward(gout.to(dtype))
        return y.detach(), wd.grad

    (y64, dw64), (y32, dw32) = side(torch.float64), side(torch.float32)
    ty, tw = MARGIN * rel_err(y32, y64), MARGIN * rel_err(dw32, dw64)   # test_to_flat_forward_and_weight_gradient's bound

    def run(P):
        L_ = _C.lib()
        sd, wd, gd = P.inp("spec", spec), P.inp("w", w), P.inp("g", gout)
        o, dw = P.out("out", (N, 1, Lout)), P.out("dw", (M, 1, K))
        ws = P.ws("ws", P.val(L_.adp_tflat_wgrad_ws_bytes(N, M, L, K, hop) + 1, "adp_tflat_wgrad_ws_bytes") - 1)
        P.ok(L_.adp_tflat_fwd(p(sd), p(wd), N, M, L, K, hop, p(o), stream()), "adp_tflat_fwd")
        P.ok(L_.adp_tflat_wgrad(p(sd), p(gd), N, M, L, K, hop, p(dw), p(ws), stream()), "adp_tflat_wgrad")
        return [("out", o, y64, ty), ("dw", dw, dw64, tw)]
    return run


# ---------------------------------------------------------------------------------------------------- optimizer
@case(("adp_sqnorm_partials", "adp_adamw_step"), [dict(sizes=(1024, 64, 4096)), dict(sizes=(1027, 5, 333))])
def adamw(sizes):
    """The tensors themselves (p, g, m, v, ema) are the placed operands; the tables hold their placed addresses."""
    CH = 512
    T = len(sizes)
    ps = [rnd(n, seed=10 + i) for i, n in enumerate(sizes)]
    gs = [rnd(n, seed=20 + i) for i, n in enumerate(sizes)]
    ms = [rnd(n, seed=30 + i, scale=0.1) for i, n in enumerate(sizes)]
    vs = [rnd(n, seed=40 + i).abs() * 0.01 for i, n in enumerate(sizes)]
    es = [rnd(n, seed=50 + i) for i, n in enumerate(sizes)]
    chunks = torch.tensor([[i, a, min(CH, n - a)] for i, n in enumerate(sizes) for a in range(0, n, CH)], dtype=torch.int64)
    hp = dict(decay=1 - 1e-3 * 0.01, one_minus_beta1=0.1, beta2=0.999, one_minus_beta2=1e-3, inv_bc2_sqrt=(1 - 0.999 ** 3) ** -0.5,
              eps=1e-8, step_size=1e-3 / (1 - 0.9 ** 3), ema_weight=0.05)
    f = lambda k: float(torch.tensor(hp[k], dtype=torch.float32))  # noqa: E731  (the host's doubles rounded to float)
    max_norm = 1.0
    norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs))
    clip = min(1.0, max_norm / (norm + 1e-6))
    want = [refs.adamw(ps[i].double(), gs[i].double(), ms[i].double(), vs[i].double(), es[i].double(), clip=clip,
                       **{k: f(k) for k in hp}) for i in range(T)]
    # the bound of test_optim._check: MARGIN (4) x the error of the same recurrence in float32 torch, floored at one ulp
    norm32 = torch.sqrt(sum((g ** 2).sum() for g in gs))
    clip32 = torch.clamp(max_norm / (norm32 + 1e-6), max=1.0)
    f32 = [refs.adamw(ps[i], gs[i], ms[i], vs[i], es[i], clip=clip32, **{k: f(k) for k in hp}) for i in range(T)]
    bound = lambda a32, a64: 4.0 * max(rel_err(a32, a64), 2.0 ** -23)  # noqa: E731

    def run(P):
        L_ = _C.lib()
        s = stream()
        pd = [P.inout(f"p{i}", ps[i]) for i in range(T)]
        gd = [P.inp(f"g{i}", gs[i]) for i in range(T)]
        md = [P.inout(f"m{i}", ms[i]) for i in range(T)]
        vd = [P.inout(f"v{i}", vs[i]) for i in range(T)]
        ed = [P.inout(f"ema{i}", es[i]) for i in range(T)]
        ptrs = P.inp("grad_ptrs", torch.tensor([t.data_ptr() for t in gd], dtype=torch.int64))
        numels = P.inp("numels", torch.tensor(sizes, dtype=torch.int64))
        tab = P.inp("tensors", torch.tensor([[pd[i].data_ptr(), gd[i].data_ptr(), md[i].data_ptr(), vd[i].data_ptr(),
                                              ed[i].data_ptr(), sizes[i]] for i in range(T)], dtype=torch.int64))
        ch = P.inp("chunk_table", chunks)
        nch = chunks.shape[0]
        written = torch.zeros(1024, dtype=torch.bool)
        written[:min(nch, 1024)] = True
        part = P.out("partials", (1024,), dtype=torch.float64, written=written)
        gn = P.out("grad_norm", (1,))
        np_ = P.val(L_.adp_sqnorm_partials(p(ptrs), p(numels), T, p(ch), nch, p(part), s), "adp_sqnorm_partials")
        assert np_ == min(nch, 1024)
        P.ok(L_.adp_adamw_step(p(tab), p(ch), nch, f("decay"), f("one_minus_beta1"), f("beta2"), f("one_minus_beta2"),
                               f("inv_bc2_sqrt"), f("eps"), f("step_size"), f("ema_weight"), p(part), np_, max_norm, p(gn), s),
             "adp_adamw_step")
        n64 = torch.tensor([norm], dtype=torch.float64)
        out = [("sqnorm", part[:np_].cpu().sum().reshape(1), n64 * n64, bound(norm32.reshape(1) ** 2, n64 * n64)),
               ("grad_norm", gn, n64, bound(norm32.reshape(1), n64))]
        for i in range(T):
            out += [(f"{nm}{i}", dev_t[i], want[i][j], bound(f32[i][j], want[i][j]))
                    for j, (nm, dev_t) in enumerate((("p", pd), ("m", md), ("v", vd), ("ema", ed)))]
        return out
    return run


# =====================================================================================================================
# The harness
# =====================================================================================================================
CASE_IDS = [c[0] for c in CASES]
_BUILT = {}


def _built(cid):
    if cid not in _BUILT:
        _, _, fn, shape, _ = CASES[CASE_IDS.index(cid)]
        _BUILT[cid] = fn(**shape)
    return _BUILT[cid]


def _setenv(monkeypatch, cid):
    for k, v in CASES[CASE_IDS.index(cid)][4].items():
        monkeypatch.setenv(k, v)


def place_and_check(dev, cid, plan, what):
    """One placed call of case `cid`: returns the Placer (operand list, notes) after every check has passed."""
    run = _built(cid)
    P = Placer(dev, plan)
    P.notes["refused"] = False
    try:
        checks = run(P)
    except AlignRefused:
        P.arena.verify(refused=True)   # a refused call must not have touched anything, its outputs included
        P.notes["refused"] = True
        return P
    print(f"{cid} [{what}] kernels: {P.notes.get('kernels', '-')}")
    problems = []
    for label, got, want, bound in checks:
        err = rel_err(got, want)
        print(f"{cid} [{what}] {label}: rel err {err:.3e} (bound {bound:.1e})")
        if not err < bound:
            problems.append(f"{label}: rel err {err:.3e} >= {bound:.1e}")
    try:
        P.arena.verify()
    except PlacementError as e:
        problems.append(str(e))
    assert not problems, f"{cid}, placement {what} (kernels: {P.notes.get('kernels', '?')}):\n" + "\n".join(problems)
    return P


@pytest.mark.parametrize("kind", ["zero", "all1", "mixed"])
@pytest.mark.parametrize("cid", CASE_IDS)
def test_whole_call_placements(dev, cid, kind, monkeypatch):
    _setenv(monkeypatch, cid)
    P = place_and_check(dev, cid, PLANS[kind], kind)
    run = _built(cid)
    if kind == "zero" and hasattr(run, "want_tile"):
        assert P.notes["tile"] == run.want_tile, f"{cid}: the aligned placement must dispatch to {run.family}: {P.notes}"
        if run.want_ws:
            assert P.notes["ws"] > 0, f"{cid}: meant to take the cross-workgroup K split"
    if kind == "zero":
        for k in getattr(run, "want_kernels", []):
            assert k in P.notes["kernels"], f"{cid}: the aligned placement must launch {k}: {P.notes['kernels']}"
    if kind == "zero" and getattr(run, "want_partials", 0):
        assert P.notes["partials"] > 1, f"{cid}: meant to take the parked form"


def _single_placements(dev, cid, monkeypatch):
    """(operand, offset, Placer) for each single-operand placement of the case."""
    _setenv(monkeypatch, cid)
    base = place_and_check(dev, cid, PLANS["zero"], "zero")
    out = [(None, 0, base)]
    for name, role in base.operands:
        out.append((name, 1, place_and_check(dev, cid, single(name, 1), f"{name}@1")))
        if role in ("out", "inout", "ws", "res"):
            out.append((name, 2, place_and_check(dev, cid, single(name, 2), f"{name}@2")))
    return out


@pytest.mark.parametrize("cid", [c for c in CASE_IDS if c not in CONV_FAMILY])
def test_single_operand_placements(dev, cid, monkeypatch):
    _single_placements(dev, cid, monkeypatch)


# Which single-operand placements move an adp_conv1d call to another kernel, per case (recorded from the emulator build; the
# dispatch is host code, the same on the GPU): "moves" lists the operands whose offset 1 (4 bytes off) changes what
# adp_conv1d_tile reports -- another family of the chain, or another variant of conv_mm (its Winograd form wants 8 bytes on
# out / res / out_pre / ws: the code drops the 40000000 of that form) --, "moves@2" the output / residual / workspace
# operands that still do so at offset 2 (8 bytes off: the 16-byte clauses), "keeps" the operands whose offset 1 leaves the
# report alone (no eligibility clause looks at them; the kernels pick a scalar path themselves), "gnb_off" (data-gradient
# cases with the gnb_ab epilogue) the operands whose offset 1 makes adp_conv1d_gnb_entries answer 0: the launch then runs
# without that epilogue.  A change to an eligibility clause shows up here as a diff.
DISPATCH = {
    "conv1d-tile32-0": {"moves": ["bias", "out", "res", "x"],
        "moves@2": ["out", "res"],
        "keeps": ["gn_part", "w"]},
    "conv1d-tile32-1": {"moves": ["bias", "out", "res", "x"],
        "moves@2": ["out", "res"],
        "keeps": ["gn_part", "pro_beta", "pro_gamma", "pro_stats", "w"]},
    "conv1d-tile32-2": {"moves": ["out", "x"],
        "moves@2": ["out"],
        "keeps": ["gnb_ab", "gnb_beta", "gnb_gamma", "gnb_stats", "gnb_x", "w"],
        "gnb_off": ["gnb_beta", "gnb_gamma", "gnb_x", "out", "x"]},
    "conv1d-tilek-3": {"moves": ["out", "res", "w", "x"],
        "moves@2": ["out", "res"],
        "keeps": ["bias", "gn_part"]},
    "conv1d-tilek-4": {"moves": ["out", "res", "w", "x"],
        "moves@2": ["out", "res"],
        "keeps": ["gnb_ab", "gnb_beta", "gnb_gamma", "gnb_stats", "gnb_x"],
        "gnb_off": ["gnb_x", "out", "res", "w", "x"]},
    "conv1d-mm4-5": {"moves": ["out", "out_pre", "res", "w", "x"],
        "moves@2": ["out", "out_pre", "res"],
        "keeps": ["bias", "e_scale", "gn_part"]},
    "conv1d-mm4-6": {"moves": ["out", "out_pre", "res", "w", "x"],
        "moves@2": ["out", "out_pre", "res"],
        "keeps": ["bias", "e_scale", "gn_part"]},
    "conv1d-mm4-7": {"moves": ["out", "out_pre", "res", "w", "x"],
        "moves@2": ["out", "out_pre", "res"],
        "keeps": ["bias", "e_scale", "gn_part", "ws"]},
    "conv1d-mm4-8": {"moves": ["out", "w", "x"],
        "moves@2": ["out"],
        "keeps": ["gnb_ab", "gnb_beta", "gnb_gamma", "gnb_stats", "gnb_x"],
        "gnb_off": ["gnb_x", "out", "w", "x"]},
    "conv1d-tilek1-9": {"moves": ["out", "res", "w", "x"],
        "moves@2": ["out", "res"],
        "keeps": ["bias", "gn_part"]},
    "conv1d-tilek1-10": {"moves": ["out", "res", "w", "x"],
        "moves@2": ["out", "res"],
        "keeps": []},
    "conv1d-mm-11": {"moves": ["w", "x"],
        "moves@2": [],
        "keeps": ["bias", "e_scale", "gn_part", "out", "out_pre", "pro_beta", "pro_gamma", "pro_stats", "res"]},
    "conv1d-mm-12": {"moves": ["w", "x"],
        "moves@2": [],
        "keeps": ["bias", "e_scale", "gn_part", "out", "out_pre", "res"]},
    "conv1d-mm-wino-13": {"moves": ["out", "out_pre", "res", "w", "x"],
        "moves@2": [],
        "keeps": ["bias", "e_scale", "gn_part"]},
    "conv1d-mm-wino-wide-14": {"moves": ["out", "out_pre", "res", "w", "x"],
        "moves@2": [],
        "keeps": ["bias", "e_scale", "gn_part", "pro_beta", "pro_gamma", "pro_stats"]},
    "conv1d-mm-splitk-15": {"moves": ["out", "out_pre", "res", "w", "ws", "x"],
        "moves@2": [],
        "keeps": ["bias", "e_scale", "gn_part"]},
    "conv1d-mm-splitk-16": {"moves": ["out", "w", "ws", "x"],
        "moves@2": [],
        "keeps": ["gnb_ab", "gnb_beta", "gnb_gamma", "gnb_stats", "gnb_x"],
        "gnb_off": ["gnb_x", "out", "w", "ws", "x"]},
    "conv1d-direct-17": {"moves": ["out", "out_pre", "res", "x", "x2"],
        "moves@2": ["out", "out_pre", "res"],
        "keeps": ["bias", "e_scale", "pro_beta", "pro_gamma", "pro_stats", "w"]},
    "conv1d-direct-18": {"moves": ["out", "out_pre", "res", "x"],
        "moves@2": ["out", "out_pre", "res"],
        "keeps": ["bias", "e_scale", "w"]},
    "conv1d-direct-19": {"moves": ["out", "out_pre", "res", "x"],
        "moves@2": ["out", "out_pre", "res"],
        "keeps": ["bias", "e_scale", "w"]},
    "conv1d-generic-20": {"moves": [],
        "moves@2": [],
        "keeps": ["bias", "e_scale", "out", "out_pre", "pro_beta", "pro_gamma", "pro_stats", "res", "w", "x", "x2"]},
    "conv1d-generic-21": {"moves": [],
        "moves@2": [],
        "keeps": ["bias", "e_scale", "out", "out_pre", "res", "w", "x"]},
    "conv1d-generic-22": {"moves": [],
        "moves@2": [],
        "keeps": ["bias", "e_scale", "out", "out_pre", "pro_beta", "pro_gamma", "pro_stats", "res", "w", "x"]},
    "conv1d-generic-23": {"moves": [],
        "moves@2": [],
        "keeps": ["bias", "e_scale", "out", "out_pre", "res", "w", "x"]},
}


@pytest.mark.parametrize("cid", list(CONV_FAMILY))
def test_conv_single_operand_placements_and_dispatch(dev, cid, monkeypatch):
    runs = _single_placements(dev, cid, monkeypatch)
    base = runs[0][2].notes
    moves = sorted(n for n, k, P in runs if k == 1 and P.notes["tile"] != base["tile"])
    keeps = sorted(n for n, k, P in runs if k == 1 and P.notes["tile"] == base["tile"])
    moves2 = sorted(n for n, k, P in runs if k == 2 and P.notes["tile"] != base["tile"])
    # the gnb_ab epilogue: which offset-1 placements switch it off (adp_conv1d_gnb_entries answers 0), which are refused
    gnb_off = sorted(n for n, k, P in runs if k == 1 and base["gnb"] and not P.notes["gnb"])
    refused = sorted(f"{n}@{k}" for n, k, P in runs if P.notes["refused"])
    if base["gnb"]:
        assert "gnb_x" in gnb_off, f"{cid}: the epilogue reads gnb_x with 16-byte loads; a misaligned gnb_x must switch it off"
        assert refused == ["gnb_ab@1"], f"{cid}: adp.h wants gnb_ab 8-byte aligned (ADP_ERR_ALIGN): refused {refused}"
    else:
        assert not refused and not gnb_off
    report = "\n".join(f"  {n}@{k}: tile {P.notes['tile']} ws {P.notes['ws']} gn {P.notes['gn']} gnb {P.notes['gnb']} "
                       f"kernels {P.notes['kernels']}" for n, k, P in runs)
    print(f"{cid}: aligned tile {base['tile']}\n{report}")
    want = DISPATCH.get(cid)
    assert want is not None, f"{cid}: no DISPATCH entry; measured moves={moves} moves2={moves2} keeps={keeps} gnb_off={gnb_off}"
    assert (moves, moves2, keeps, gnb_off) == (sorted(want["moves"]), sorted(want["moves@2"]), sorted(want["keeps"]),
                                               sorted(want.get("gnb_off", []))), \
        f"{cid}: dispatch under single-operand placement changed:\nmoves {moves}\nmoves@2 {moves2}\nkeeps {keeps}\n" \
        f"gnb_off {gnb_off}\n{report}"


def test_every_conv_family_has_a_moving_and_a_keeping_operand():
    fams = {}
    for cid, fam in CONV_FAMILY.items():
        f = fams.setdefault(fam.split("-")[0], dict(moves=set(), keeps=set()))
        f["moves"] |= set(DISPATCH[cid]["moves"])
        f["keeps"] |= set(DISPATCH[cid]["keeps"])
    assert set(fams) == {"tile32", "tilek", "mm4", "tilek1", "mm", "direct", "generic"}
    for fam, f in fams.items():
        assert f["keeps"], f"{fam}: no operand whose misalignment keeps the family"
        if fam != "generic":   # the end of the chain: nothing to fall back to, every operand keeps it
            assert f["moves"], f"{fam}: no operand whose misalignment moves the call to another family"


def test_table_and_exclusions_cover_the_c_abi():
    covered = {e for c in CASES for e in c[1]}
    assert not covered & set(EXCLUDED), covered & set(EXCLUDED)
    assert all(isinstance(r, str) and r for r in EXCLUDED.values())
    missing = set(_C.ABI["adp.h"]) - covered - set(EXCLUDED)
    extra = (covered | set(EXCLUDED)) - set(_C.ABI["adp.h"])
    assert not missing and not extra, f"decide how to place: {sorted(missing)}; not in the C-ABI: {sorted(extra)}"


# =====================================================================================================================
# End to end through the Python API: parameters as odd-offset views of one flat buffer, input an odd-offset slice
# =====================================================================================================================
def test_unet_with_odd_offset_parameters_and_input(dev):
    """The tiny U-Net of test_unet_forward_backward_tiny with every parameter a view into ONE flat buffer at an odd float
    offset (what a flat-buffer optimizer or a checkpoint loader produces) and an input that is a contiguous slice at an
    odd offset: output, loss and every parameter gradient match the same net with ordinary parameters within the bound
    that test puts on the net against the oracle (and the relocated net still matches the oracle itself)."""
    from test_unet import TINY, TOL as UNET_TOL, build_pair, compare_grads
    B, L = 2, 256
    oracle, plain = build_pair(TINY, dev)
    _, moved = build_pair(TINY, dev)
    params = list(moved.parameters())
    total, offs = 1, []
    for q in params:
        total += total % 2 == 0            # every view starts at an odd float
        offs.append(total)
        total += q.numel()
    flat = torch.zeros(total + 1, device=dev)
    assert flat.data_ptr() % 16 == 0
    with torch.no_grad():
        for q, off in zip(params, offs):
            view = flat[off:off + q.numel()].view(q.shape)
            view.copy_(q)
            q.data = view
            assert q.data_ptr() % 8 == 4 and q.is_contiguous()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 2, L, generator=g)
    t = torch.linspace(0.3, 0.8, B)
    feats = 0.1 * torch.randn(B, TINY["modulation_features"], generator=g)
    gy = torch.randn(B, 2, L, generator=g)
    xbuf = torch.zeros(B * 2 * L + 1, device=dev)
    xbuf[1:].copy_(x.reshape(-1))
    x_odd = xbuf[1:].view(B, 2, L)
    assert x_odd.is_contiguous() and x_odd.data_ptr() % 16 == 4
    y_ref = oracle(x, t, features=feats)
    y0 = plain(x.to(dev), t.to(dev), features=feats.to(dev))
    y1 = moved(x_odd, t.to(dev), features=feats.to(dev))
    assert rel_err(y1, y0) < UNET_TOL and rel_err(y1, y_ref) < UNET_TOL
    loss0, loss1 = (y0 * gy.to(dev)).sum(), (y1 * gy.to(dev)).sum()
    assert abs(loss1.item() - loss0.item()) < UNET_TOL * max(abs(loss0.item()), 1.0)
    y_ref.backward(gy)
    loss0.backward()
    loss1.backward()
    g0 = {n: q.grad.detach().double().cpu() for n, q in plain.named_parameters()}
    gmax = max(v.abs().max().item() for v in g0.values())
    for n, q in moved.named_parameters():
        assert q.grad is not None, n
        e = (q.grad.detach().double().cpu() - g0[n]).abs().max().item() / max(g0[n].abs().max().item(), 1e-3 * gmax)
        assert e < UNET_TOL, (n, e)        # compare_grads' metric, against the ordinary net
    compare_grads(moved, oracle)


# =====================================================================================================================
# The harness itself, with pure-Python stand-ins for kernels (emulator side only; no kernel is made to misbehave)
# =====================================================================================================================
def test_guard_is_at_least_a_wave_row_of_16_byte_stores():
    assert GUARD_BYTES >= 1024 * 4 and GUARD_BYTES >= 64 * 16


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_verify_names_an_overrun(offset):
    a = Arena("cpu")
    x = a.input("x", torch.arange(10.0), offset)
    y = a.output("y", (10,), offset)
    y.copy_(x * 2)
    a.verify()
    y.as_strided((11,), (1,))[10] = 1.0   # a stand-in kernel that writes one float past its output
    with pytest.raises(PlacementError, match=r"operand 'y' .*guard after the payload touched, 1 int32 word\(s\), first index 0, last index 0"):
        a.verify()


def test_verify_names_an_underrun_and_a_changed_input():
    a = Arena("cpu")
    x = a.input("x", torch.arange(10.0), 2)
    y = a.output("y", (10,), 1)
    y.zero_()
    torch.as_strided(y, (1,), (1,), y.storage_offset() - 1)[0] = 0.0   # the offset gap in front of y
    x[3] = -1.0
    with pytest.raises(PlacementError) as e:
        a.verify()
    assert "operand 'y' (offset 1): guard before the payload touched, 1 int32 word(s), first index -1, last index -1" in str(e.value)
    assert "operand 'x' (offset 2): input payload changed, 1 int32 word(s), first index 3, last index 3" in str(e.value)


def test_verify_names_an_unwritten_element():
    a = Arena("cpu")
    y = a.output("y", (4, 5), 1)
    y.view(-1)[:19] = 1.0                  # a stand-in kernel that leaves the last element unwritten
    with pytest.raises(PlacementError, match=r"operand 'y' \(offset 1\): 1 output element\(s\) left unwritten, first index 19, last index 19"):
        a.verify()
    y.view(-1)[19] = float("nan")          # an ordinary NaN is a written value
    a.verify()


def test_verify_of_a_refused_call_wants_the_outputs_untouched():
    a = Arena("cpu")
    y = a.output("y", (8,), 1)
    a.verify(refused=True)
    y[2] = 1.0
    with pytest.raises(PlacementError, match=r"operand 'y' .*1 element\(s\) outside the promised output written, first index 2"):
        a.verify(refused=True)


def _stand_in(code, figures):
    def run(P):
        P.out("y", (4,)).fill_(1.0)   # a stand-in kernel that writes its whole output
        return code, figures
    return run


def test_place_and_check_names_a_refused_call():
    with pytest.raises(AssertionError, match=r"adp_stand_in \(case\) odd \[zero\] returned -3 \(misaligned pointer\)"):
        shared_place_and_check("cpu", "adp_stand_in", "(case) odd", _stand_in(-3, []), PLANS["zero"], "zero")
    assert shared_place_and_check("cpu", "adp_stand_in", "(case) odd", _stand_in(0, []), PLANS["all1"], "all1").operands == \
        [("y", "out")]

    def writes_nothing(P):
        P.out("y", (4,))
        return 0, []
    with pytest.raises(PlacementError, match=r"operand 'y' \(offset 0\): 4 output element\(s\) left unwritten"):
        shared_place_and_check("cpu", "adp_stand_in", "(case) odd", writes_nothing, PLANS["zero"], "zero")


@pytest.mark.parametrize("figure", [("edge", 1e-4, "<", 1e-4), ("edge", 1.1e-4, "<=", 1e-4), ("edge", float("nan"), "<=", 1.0),
                                    close("edge", torch.ones(3), torch.tensor([1.0, 1.0, 1.001]), 1e-4),
                                    exact("edge", torch.zeros(2), torch.tensor([0.0, 2.0 ** -149]))])
def test_place_and_check_names_a_figure_out_of_bound(figure):
    held = ("fine", 0.0, "<", 1e-4)
    shared_place_and_check("cpu", "adp_stand_in", "(case) odd", _stand_in(0, [held]), PLANS["zero"], "zero")
    with pytest.raises(AssertionError, match=r"adp_stand_in \(case\) odd, placement zero:\nedge: ") as e:
        shared_place_and_check("cpu", "adp_stand_in", "(case) odd", _stand_in(0, [held, figure]), PLANS["zero"], "zero")
    assert "fine" not in str(e.value)


def test_verify_respects_the_promised_elements_and_other_types():
    a = Arena("cpu")
    mask = strided_rows(2, 3, 5)
    y = a.output("y", (8,), 0, written=mask)
    d = a.output("d", (3,), 1, dtype=torch.float64)
    m = a.input("m", torch.tensor([1, 0, 1], dtype=torch.uint8), 3)
    t = a.input("t", torch.tensor([5, 6], dtype=torch.int64), 1)
    assert m.data_ptr() % 4 == 3 and d.data_ptr() % 16 == 8 and t.data_ptr() % 16 == 8
    y[:3] = 1.0
    y[5:] = 2.0
    d.fill_(3.0)
    a.verify()
    y[3] = 0.0                             # a write into the row-stride gap
    with pytest.raises(PlacementError, match=r"operand 'y' .*1 element\(s\) outside the promised output written, first index 3"):
        a.verify()
