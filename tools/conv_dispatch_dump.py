"""Dumps what the conv / weight-gradient dispatch of a library build decides, one line per descriptor of a fixed grid.

    python tools/conv_dispatch_dump.py [path/to/lib.so] > table.txt     (default: the SIMT-emulated test build)

Part 1 ("q" lines) only asks the query functions (adp_conv1d_tile / _ws_bytes / _gn_entries / _gnb_entries with and without
ws, adp_conv1d_wgrad_ws_bytes / _partials); they inspect pointer VALUES only, so the addresses are fabricated.  Part 2 ("l"
lines) launches small problems with the launch trace on and prints the kernel instantiations (emulator builds: CPU buffers).
The run fails if a kernel family of either dispatch table is never reached.  tests/test_conv_dispatch.py compares the output
of the current build with tests/golden/conv_dispatch.txt, recorded from the commit BEFORE a dispatch change.
"""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audio_diffusion_pytorch_amd._C import ABI, ConvDesc, WgradDesc  # noqa: E402

KNOBS = [
    {},
    {"ADP_CONV_WINO": "0"},
    {"ADP_CONV_WINO4": "0", "ADP_CONV_TILEK": "0", "ADP_CONV_TILEK1": "0"},
    {"ADP_MM_MIN_BLOCKS": "1", "ADP_MM4_MIN_BLOCKS": "1", "ADP_TILEK_MIN_R": "64", "ADP_TILEK_MIN_TILES": "1",
     "ADP_TILEK1_MIN_R": "64", "ADP_TILEK1_MIN_TILES": "1"},
    {"ADP_MM4_KS_MAX": "4", "ADP_CONV_TILEK": "0"},
]
# config 1 of bench.py / the README model: (channels, length) per depth and the resampling factor that leads to it
DEPTHS = [(8, 262144, 1), (32, 65536, 4), (64, 16384, 4), (128, 4096, 4), (256, 2048, 2), (512, 1024, 2), (512, 512, 2),
          (1024, 256, 2), (1024, 128, 2)]
A = 0x7f0000000000  # fabricated, 4 KiB-aligned operand addresses, 16 MiB apart


def bind(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in {**ABI["adp.h"], **ABI["adp_ar.h"]}.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def conv_desc(B, R, M, Lin, N, KT, stride=1, up=1, tr=0, pro=0, store=0, sp=0, mis=0, **kw):
    d = ConvDesc()
    for i, n in enumerate(("x", "w", "out")):
        setattr(d, n, A + (i << 24) + mis)
    d.B, d.R, d.R1, d.Lin, d.M, d.N, d.KT, d.stride, d.dil, d.pad, d.up = B, R, R, Lin, M, N, KT, stride, 1, (KT - 1) // 2 if stride == 1 else 0, up
    d.transposed, d.prologue, d.groups, d.store, d.sp = tr, pro, 8 if pro == 1 else 0, store, sp
    if pro:
        d.pro_stats, d.pro_gamma, d.pro_beta = A + (8 << 24), A + (9 << 24), A + (10 << 24)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def wgrad_desc(c):
    g = WgradDesc()
    g.x, g.dy, g.dw, g.ws = c.x, c.out, c.w, A + (5 << 24)
    for n in ("B", "R", "R1", "Lin", "M", "N", "KT", "stride", "dil", "pad", "up", "prologue", "groups"):
        setattr(g, n, getattr(c, n))
    g.pro_stats, g.pro_gamma, g.pro_beta = c.pro_stats, c.pro_gamma, c.pro_beta
    return g


def grid(thin=False):
    """(label, descriptor) of every grid point; thin: batch 4 only (knob sets that move no batch-1 decision on their own)"""
    out = []
    for B in (4,) if thin else (1, 4):
        prev = None
        for C, L, f in DEPTHS:
            for pro in (0, 1):
                out.append((f"k3 B{B} C{C} L{L} pro{pro}", conv_desc(B, C, C, L, L, 3, pro=pro)))
            out.append((f"k3 dgrad B{B} C{C} L{L}", conv_desc(B, C, C, L, L, 3, tr=1)))
            out.append((f"k1 B{B} C{C} L{L}", conv_desc(B, C, C, L, L, 1)))
            if prev:
                PC, PL = prev
                out.append((f"down B{B} {PC}->{C} L{PL}->{L}", conv_desc(B, PC, C, PL, L, f, stride=f)))
                out.append((f"up B{B} {C}->{PC} L{L}->{PL}", conv_desc(B, C, PC, L, PL, 3, up=f)))
                out.append((f"up dgrad B{B} {PC}->{C} L{PL} pooled", conv_desc(B, PC, C, PL, PL, 3, tr=1, store=2, sp=f)))
            prev = (C, L)
        out.append((f"k1 dgrad B{B} 512->1536 L512", conv_desc(B, 512, 1536, 512, 512, 1, tr=1)))
        out.append((f"k1 dgrad B{B} store1 512->512 L512", conv_desc(B, 512, 512, 512, 512, 1, tr=1, store=1, sp=8)))
    # small problems of the tests (they reach the families through the knobs), misaligned operands, odd extents
    for C, L in ((32, 256), (64, 256), (128, 512), (48, 100), (3, 64)):
        out.append((f"small k3 C{C} L{L}", conv_desc(2, C, C, L, L, 3)))
        out.append((f"small k3 dgrad C{C} L{L}", conv_desc(2, C, C, L, L, 3, tr=1)))
        out.append((f"small k1 C{C} L{L}", conv_desc(2, C, C, L, L, 1)))
        out.append((f"small k3 C{C} L{L} x+4", conv_desc(2, C, C, L, L, 3, mis=4)))
    out.append(("dil2 k3 C64", conv_desc(2, 64, 64, 256, 256, 3, dil=2, pad=2)))
    out.append(("x2 split C64", conv_desc(2, 64, 64, 256, 256, 3, R1=32, x2=A + (11 << 24))))
    out.append(("out+8 k3 C256", conv_desc(4, 256, 256, 2048, 2048, 3, out=A + (2 << 24) + 8)))
    # what the entry points refuse
    out.append(("err B0", conv_desc(0, 64, 64, 256, 256, 3)))
    out.append(("err N0", conv_desc(2, 64, 64, 256, 0, 3)))
    out.append(("err k5", conv_desc(2, 64, 64, 256, 256, 5)))
    out.append(("err k2 stride1", conv_desc(2, 64, 64, 256, 256, 2)))
    return out


CONV_CODES = {32064: "tile", 48000064: "tilek", 64032128: "mm4", 47000064: "tilek1", 8999: "direct", 32128: "generic",
              128128: "generic", 64064: "generic"}


def family_of(tile):
    """family behind an adp_conv1d_tile code; conv_mm's is [4]<K groups><32|64>0<64 * NSP>: winograd * 40000000 + kg * 1000000 + rows * 1000 + positions"""
    if tile < 0:
        return "error"
    if tile in CONV_CODES:
        return CONV_CODES[tile]
    if tile % 40000000 // 1000000 in (1, 2, 4) and tile % 1000000 // 1000 in (32, 64) and tile % 1000 in (64, 128, 256):
        return "mm"
    sys.exit(f"conv_dispatch_dump: adp_conv1d_tile returned the unknown code {tile}")


def queries(lib, hits):
    for ki, knobs in enumerate(KNOBS):
        os.environ.update(knobs)
        for label, d in grid(thin=ki in (1, 2, 4)):
            tile = lib.adp_conv1d_tile(ctypes.byref(d))
            hits[family_of(tile)] = True
            f = [tile, lib.adp_conv1d_ws_bytes(ctypes.byref(d))]
            for ws in (None, A + (6 << 24)):
                for gnb_x in (A + (7 << 24), A + (7 << 24) + 4):
                    d.ws, d.gnb_x = ws, gnb_x
                    f += [lib.adp_conv1d_gn_entries(ctypes.byref(d)), lib.adp_conv1d_gnb_entries(ctypes.byref(d))]
            d.ws, d.gnb_x, d.gnb_ab = A + (6 << 24), A + (7 << 24), A + (13 << 24)  # (as ops.conv1d has it at the launch of a data gradient)
            f += [lib.adp_conv1d_tile(ctypes.byref(d)), lib.adp_conv1d_gnb_entries(ctypes.byref(d))]
            d.gnb_ab, d.gn_part = None, A + (12 << 24)  # (the GroupNorm-forward partials exclude the gnb epilogue of conv_mm)
            f += [lib.adp_conv1d_tile(ctypes.byref(d)), lib.adp_conv1d_gnb_entries(ctypes.byref(d))]
            g = wgrad_desc(d)
            f += [lib.adp_conv1d_wgrad_ws_bytes(ctypes.byref(g)), lib.adp_conv1d_wgrad_partials(ctypes.byref(g))]
            g.x = g.x + 4 if g.x else 4
            f += [lib.adp_conv1d_wgrad_ws_bytes(ctypes.byref(g)), lib.adp_conv1d_wgrad_partials(ctypes.byref(g))]
            if min(f) < 0:
                hits["error"] = True
            print(f"q knobs{ki} {label}: " + " ".join(str(v) for v in f))
        for k in knobs:
            del os.environ[k]


# launch subset: (knobs, label, conv descriptor arguments [gn / gnb: with gn_part / the GroupNorm-backward operands, set the
# way ops.conv1d does, after the entry-count query; nows: the caller gives no scratch], also launch the weight gradient).  One row per family and per
# instantiation branch that tests/test_kernels.py and tests/test_operand_placement.py reach, with their knob settings.
SMALL = {"ADP_MM_MIN_BLOCKS": "1", "ADP_MM4_MIN_BLOCKS": "1"}
TK = {"ADP_TILEK_MIN_R": "256", "ADP_TILEK_MIN_TILES": "1"}
TK1 = {"ADP_TILEK1_MIN_R": "64", "ADP_TILEK1_MIN_TILES": "1"}
MM4 = {"ADP_MM4_MIN_BLOCKS": "1", "ADP_WINO4_MIN_R": "128", "ADP_MM4_VPRE": "0", "ADP_MM4_LIGHT_MIN_BLOCKS": "1000000", "ADP_CONV_TILEK": "0"}
NO4 = {"ADP_CONV_WINO4": "0", "ADP_CONV_TILEK": "0", "ADP_CONV_TILEK1": "0"}
K3 = dict(B=1, R=128, M=64, Lin=256, N=256, KT=3)
LAUNCHES = [
    ({}, "tile k3 32->32", dict(B=1, R=32, M=32, Lin=128, N=128, KT=3), True),
    ({}, "tile dgrad", dict(B=1, R=32, M=32, Lin=128, N=128, KT=3, tr=1), False),
    ({"ADP_TILE_NW": "1"}, "tile nw1 pro1 gn", dict(B=2, R=32, M=32, Lin=192, N=192, KT=3, pro=1, gn=1), False),
    ({"ADP_TILE_NW": "4"}, "tile nw4 dgrad gnb", dict(B=1, R=32, M=32, Lin=256, N=256, KT=3, tr=1, gnb=1), False),
    ({"ADP_TILE_NW": "16"}, "tile nw16", dict(B=1, R=32, M=32, Lin=1024, N=1024, KT=3), False),
    ({"ADP_TILE_NW": "16"}, "tile nw16 on 4 tiles", dict(B=1, R=32, M=32, Lin=256, N=256, KT=3), False),
    ({"ADP_TILEK_MIN_R": "64", "ADP_TILEK_MIN_TILES": "1"}, "tilek k3 256->32", dict(B=1, R=256, M=32, Lin=64, N=64, KT=3), False),
    (dict(TK, ADP_TILEK_RB="1"), "tilek rb1 gn", dict(B=1, R=256, M=32, Lin=64, N=64, KT=3, gn=1), False),
    (dict(TK, ADP_TILEK_RB="2"), "tilek rb2 dgrad gnb", dict(B=1, R=256, M=32, Lin=128, N=128, KT=3, tr=1, gnb=1), False),
    (dict(TK, ADP_TILEK_RB="1", ADP_TILEK_PF="4"), "tilek rb1 pf4", dict(B=1, R=512, M=64, Lin=64, N=64, KT=3), False),
    (TK1, "tilek1 k1 256->16", dict(B=1, R=256, M=16, Lin=64, N=64, KT=1), False),
    (dict(TK1, ADP_TILEK1_NKW="8"), "tilek1 nkw8 gn", dict(B=2, R=256, M=48, Lin=64, N=64, KT=1, gn=1), False),
    (dict(TK1, ADP_TILEK1_NKW="16"), "tilek1 nkw16", dict(B=2, R=512, M=48, Lin=64, N=64, KT=1), False),
    (dict(TK1, ADP_TILEK1_NKW="16"), "tilek1 nkw16 dgrad", dict(B=1, R=512, M=48, Lin=128, N=128, KT=1, tr=1), False),
    (TK1, "tilek1 dgrad store1", dict(B=1, R=256, M=64, Lin=64, N=64, KT=1, tr=1, store=1, sp=4), False),
    (SMALL, "mm4 k3 64->32", dict(B=1, R=64, M=32, Lin=128, N=128, KT=3), True),
    (dict(MM4, ADP_MM4_BKT="32"), "mm4 bkt32 gn", dict(K3, gn=1), False),
    (dict(MM4, ADP_MM4_BKT="64"), "mm4 bkt64 gn", dict(K3, gn=1), False),
    (dict(MM4, ADP_MM4_BKT="64"), "mm4 bkt64 dgrad gnb", dict(K3, tr=1, gnb=1), False),
    (dict(MM4, ADP_MM4_LIGHT_MIN_BLOCKS="1"), "mm4 light gn", dict(K3, gn=1), False),
    (dict(MM4, ADP_MM4_LIGHT_MIN_BLOCKS="1"), "mm4 light dgrad gnb", dict(K3, tr=1, gnb=1), False),
    (dict(MM4, ADP_MM4_NPG="3"), "mm4 npg3", K3, False),
    (dict(MM4, ADP_MM4_NPG="3"), "mm4 npg3 dgrad gnb", dict(K3, tr=1, gnb=1), False),
    (dict(MM4, ADP_MM4_VPRE="1"), "mm4 vpre64", K3, False),
    (dict(MM4, ADP_MM4_VPRE="1", ADP_MM4_LIGHT_MIN_BLOCKS="1"), "mm4 vprelight", K3, False),
    (dict(MM4, ADP_MM4_KS_MAX="2", ADP_MM4_MIN_BLOCKS="2"), "mm4 ksplit2 gn", dict(B=1, R=1024, M=32, Lin=128, N=128, KT=3, gn=1), False),
    (dict(MM4, ADP_MM4_KS_MAX="2", ADP_MM4_MIN_BLOCKS="2"), "mm4 ksplit2 dgrad", dict(B=1, R=1024, M=32, Lin=128, N=128, KT=3, tr=1), False),
    (dict(MM4, ADP_MM4_KS_MAX="2", ADP_MM4_MIN_BLOCKS="2"), "mm4 ksplit2, no scratch given", dict(B=1, R=1024, M=32, Lin=128, N=128, KT=3, nows=1), False),
    (dict(MM4, ADP_MM4_KS_MAX="4", ADP_MM4_MIN_BLOCKS="4"), "mm4 ksplit4 dgrad gnb", dict(B=1, R=1024, M=32, Lin=128, N=128, KT=3, tr=1, gnb=1), False),
    (dict(MM4, ADP_MM4_MIN_BLOCKS="1"), "mm4 pooled dgrad of up2", dict(B=1, R=128, M=64, Lin=128, N=128, KT=3, tr=1, store=2, sp=2), False),
    ({"ADP_CONV_WINO4": "0"}, "mm F(2,3) k3 64->64", dict(B=1, R=64, M=64, Lin=64, N=64, KT=3), True),
    ({"ADP_CONV_WINO": "0"}, "mm direct-form k3 64->32 pro1", dict(B=1, R=64, M=32, Lin=64, N=64, KT=3, pro=1), True),
    ({}, "mm k1 64->64", dict(B=1, R=64, M=64, Lin=64, N=64, KT=1), True),
    ({}, "mm down 32->64", dict(B=1, R=32, M=64, Lin=128, N=64, KT=2, stride=2), True),
    ({"ADP_CONV_WINO": "0"}, "mm up2 64->32", dict(B=1, R=64, M=32, Lin=32, N=64, KT=3, up=2), True),
    (dict(NO4, ADP_MM_MIN_BLOCKS="1", ADP_MM_NSP="2"), "mm F(2,3) nsp2 pro1 gn", dict(B=2, R=64, M=64, Lin=300, N=300, KT=3, pro=1, gn=1), False),
    (dict(NO4, ADP_MM_MIN_BLOCKS="1", ADP_MM_NSP="4"), "mm F(2,3) nsp4 64-row dgrad", dict(B=1, R=64, M=128, Lin=520, N=520, KT=3, tr=1), False),
    (dict(NO4, ADP_MM_MIN_BLOCKS="1", ADP_MM_NSP="2"), "mm k1 nsp2 dgrad", dict(B=2, R=64, M=128, Lin=300, N=300, KT=1, tr=1), False),
    (dict(NO4, ADP_CONV_WINO="0", ADP_MM_MIN_BLOCKS="1", ADP_MM_NSP="4"), "mm direct-form nsp4", dict(B=1, R=64, M=64, Lin=516, N=516, KT=3), False),
    (dict(NO4, ADP_MM_K1_BKT="32"), "mm k1 bkt32", dict(B=2, R=256, M=64, Lin=200, N=200, KT=1, nows=1), False),
    (dict(NO4, ADP_MM_K1_BKT="64"), "mm k1 bkt64", dict(B=2, R=256, M=64, Lin=200, N=200, KT=1, nows=1), False),
    (dict(NO4, ADP_MM_K1_BKT="64", ADP_MM_MIN_BLOCKS="1"), "mm k1 bkt64 wide dgrad", dict(B=2, R=256, M=128, Lin=260, N=260, KT=1, tr=1, nows=1), False),
    (dict(NO4, ADP_MM_PF="0"), "mm F(2,3) pf0", dict(B=1, R=64, M=64, Lin=64, N=64, KT=3), False),
    (NO4, "mm F(2,3) gn", dict(B=2, R=64, M=64, Lin=200, N=200, KT=3, gn=1), False),
    (NO4, "mm F(2,3) dgrad gnb", dict(B=2, R=128, M=128, Lin=256, N=256, KT=3, tr=1, gnb=1), False),
    (NO4, "mm split-K + reduce", dict(B=1, R=512, M=64, Lin=64, N=64, KT=3), False),
    (NO4, "mm split-K + reduce gn", dict(B=1, R=512, M=64, Lin=64, N=64, KT=3, gn=1), False),
    (NO4, "mm split-K + reduce dgrad gnb", dict(B=1, R=512, M=64, Lin=64, N=64, KT=3, tr=1, gnb=1), False),
    (dict(NO4, ADP_GNB_FAMILIES="0"), "mm dgrad gnb, families off", dict(B=2, R=128, M=128, Lin=256, N=256, KT=3, tr=1, gnb=1), False),
    ({}, "mm pooled dgrad of up4", dict(B=1, R=64, M=32, Lin=64, N=64, KT=3, tr=1, store=2, sp=4), False),
    ({}, "mm k1 dgrad store1", dict(B=1, R=64, M=64, Lin=64, N=64, KT=1, tr=1, store=1, sp=2), False),
    ({}, "direct k3 2->8", dict(B=1, R=2, M=8, Lin=64, N=64, KT=3), True),
    ({}, "direct down 8->32", dict(B=1, R=8, M=32, Lin=256, N=64, KT=4, stride=4), True),
    ({}, "generic s1 k3 48->48", dict(B=1, R=48, M=48, Lin=100, N=100, KT=3), True),
    ({}, "generic s1 k1 24->24", dict(B=1, R=24, M=24, Lin=100, N=100, KT=1), True),
    ({}, "generic down 24->48", dict(B=1, R=24, M=48, Lin=100, N=50, KT=2, stride=2), True),
    ({}, "generic dil2 k3 48->48", dict(B=1, R=48, M=48, Lin=100, N=100, KT=3, dil=2, pad=2), True),
]
W4 = {"ADP_WINO_WGRAD_MIN_R": "32", "ADP_WINO4_WGRAD_MIN_R": "32"}
# weight gradients alone: (knobs, label, conv descriptor arguments, accumulate)
WGRADS = [
    (dict(W4, ADP_CONV_WINO="0"), "direct form 64x64", dict(B=2, R=64, M=64, Lin=512, N=512, KT=3), 0),
    (dict(W4, ADP_WGRAD_WINO4="0"), "F(2,3) 64x64", dict(B=2, R=64, M=64, Lin=512, N=512, KT=3), 1),
    (dict(W4, ADP_WGRAD_WINO4="1"), "F(4,3) 32x32", dict(B=2, R=32, M=32, Lin=512, N=512, KT=3), 0),
    (dict(W4, ADP_WGRAD_WINO4="1"), "F(4,3) parked", dict(B=2, R=32, M=32, Lin=4096, N=4096, KT=3), 2),
    (dict(W4, ADP_WGRAD_WINO4_UP="0"), "up2, F(2,3)", dict(B=1, R=64, M=32, Lin=128, N=256, KT=3, up=2), 0),
    (W4, "up2, F(4,3)", dict(B=1, R=64, M=32, Lin=128, N=256, KT=3, up=2), 0),
    ({}, "narrow 8->8 pro1", dict(B=2, R=8, M=8, Lin=2304, N=2304, KT=3, pro=1), 0),
]
# adp_conv1d_wgrad_batch: (knobs, label, conv descriptor arguments, items)
BATCHES = [
    ({"ADP_WGRAD_BATCH_SPLIT": "1"}, "3 x 32 ch, batch split", dict(B=2, R=32, M=32, Lin=4096, N=4096, KT=3), 3),
    ({"ADP_WGRAD_BATCH_SPLIT": "0"}, "3 x 32 ch, lone split", dict(B=2, R=32, M=32, Lin=4096, N=4096, KT=3), 3),
    ({}, "10 x 64 ch (8 + 2)", dict(B=2, R=64, M=64, Lin=1024, N=1024, KT=3), 10),
    ({"ADP_WG_SOLO": "1"}, "2 x 64 ch, solo forced", dict(B=2, R=64, M=64, Lin=1024, N=1024, KT=3), 2),
    ({"ADP_WG_SOLO": "0"}, "2 x 64 ch, solo off", dict(B=2, R=64, M=64, Lin=1024, N=1024, KT=3), 2),
    ({}, "1 item", dict(B=2, R=32, M=32, Lin=2048, N=2048, KT=3), 1),
    ({}, "3 x narrow (one call per item)", dict(B=1, R=2, M=8, Lin=64, N=64, KT=3), 3),
    ({}, "3 x generic (one call per item)", dict(B=1, R=48, M=48, Lin=100, N=100, KT=3), 3),
    ({}, "refused: no items", dict(B=1, R=32, M=32, Lin=128, N=128, KT=3), 0),
]
WGRAD_KERNELS = {"wgrad_mm_kernel": "wgrad_mm", "wgrad_direct_kernel": "wgrad_direct", "wgrad_direct8_kernel": "wgrad_direct",
                 "wgrad_s1_kernel": "wgrad_s1", "wgrad_kernel": "wgrad_generic"}
NBUF, BUF_FLOATS = 16, 1 << 20  # 4 MiB each: every operand below is checked against it


def traced(lib, fn, *args):
    lib.adp_launch_trace(1, None, 0)
    rc = fn(*args, None)
    buf = ctypes.create_string_buffer(1 << 16)
    lib.adp_launch_trace(0, buf, 1 << 16)
    names = re.sub(r"; adp_\w+_desc = adp_\w+_desc", "", buf.value.decode())  # (a typedef __PRETTY_FUNCTION__ spells out)
    return f"rc={rc} " + " ; ".join(names.split("\n"))


def note_wgrad(t, hits):
    for k, fam in WGRAD_KERNELS.items():
        if k + "<" in t or k + "@" in t or "(" + k in t:
            hits[fam] = True
    return t


def launches(lib, hits):
    bufs = [np.zeros(BUF_FLOATS, dtype=np.float32) + 0.5 for _ in range(NBUF)]
    p = [b.ctypes.data + (-b.ctypes.data % 64) for b in bufs]
    room = 4 * BUF_FLOATS - 64

    def conv(args):
        args = dict(args)
        gn, gnb, nows = args.pop("gn", 0), args.pop("gnb", 0), args.pop("nows", 0)
        d = conv_desc(**args)
        d.x, d.w, d.out = p[0], p[1], p[2]
        assert 4 * max(d.B * d.R * d.Lin, d.M * d.R * d.KT, d.B * d.M * d.N) <= room
        if d.prologue:
            d.pro_stats, d.pro_gamma, d.pro_beta = p[3], p[4], p[5]
        ws = lib.adp_conv1d_ws_bytes(ctypes.byref(d))
        assert ws <= room
        if ws > 0 and not nows:
            d.ws = p[6]
        if gn:
            n = lib.adp_conv1d_gn_entries(ctypes.byref(d))
            assert 0 < n and 4 * d.B * d.M * n * 3 <= room, n
            d.gn_part = p[8]
        if gnb:
            d.gnb_x, d.gnb_stats, d.gnb_gamma, d.gnb_beta, d.gnb_groups = p[9], p[10], p[11], p[12], 8
            n = lib.adp_conv1d_gnb_entries(ctypes.byref(d))
            assert 4 * d.B * d.M * max(n, 0) * 2 <= room, n
            if n > 0:
                d.gnb_ab = p[13]
        return d

    def with_knobs(knobs, line):
        os.environ.update(knobs)
        print(line())
        for k in knobs:
            del os.environ[k]

    def wgrad(d, accumulate=0):
        g = wgrad_desc(d)
        g.dw, g.ws, g.accumulate = p[7], p[6], accumulate
        assert 0 < lib.adp_conv1d_wgrad_ws_bytes(ctypes.byref(g)) <= room
        return g

    def conv_lines(label, args, with_wgrad):
        d = conv(args)
        out = f"l conv {label}: " + traced(lib, lib.adp_conv1d, ctypes.byref(d))
        if with_wgrad:
            out += f"\nl wgrad {label}: " + note_wgrad(traced(lib, lib.adp_conv1d_wgrad, ctypes.byref(wgrad(d))), hits)
        return out

    def batch_line(label, args, n):
        ds = (WgradDesc * max(n, 1))()
        g = wgrad(conv(args))
        each = lib.adp_conv1d_wgrad_ws_bytes(ctypes.byref(g))
        each += -each % 64
        dw = 4 * g.M * g.R * g.KT
        dw += -dw % 64
        assert n * each <= room and n * dw <= room
        for i in range(n):
            ctypes.memmove(ctypes.byref(ds[i]), ctypes.byref(g), ctypes.sizeof(g))
            ds[i].ws, ds[i].dw = p[6] + i * each, p[7] + i * dw
        return f"l wgrad_batch {label}: " + note_wgrad(traced(lib, lib.adp_conv1d_wgrad_batch, ds, n), hits)

    for knobs, label, args, with_wgrad in LAUNCHES:
        with_knobs(knobs, lambda: conv_lines(label, args, with_wgrad))
    for knobs, label, args, acc in WGRADS:
        with_knobs(knobs, lambda: f"l wgrad {label}: " + note_wgrad(traced(lib, lib.adp_conv1d_wgrad, ctypes.byref(wgrad(conv(args), acc))), hits))
    for knobs, label, args, n in BATCHES:
        with_knobs(knobs, lambda: batch_line(label, args, n))


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "emul", "libadp_emul.so")
    lib = bind(path)
    hits = {}
    queries(lib, hits)
    launches(lib, hits)
    want = ["tile", "tilek", "mm4", "tilek1", "mm", "direct", "generic", "error", "wgrad_mm", "wgrad_direct", "wgrad_s1", "wgrad_generic"]
    missing = [f for f in want if f not in hits]
    if missing:
        sys.exit(f"conv_dispatch_dump: the grid never reached {missing}")


if __name__ == "__main__":
    main()
