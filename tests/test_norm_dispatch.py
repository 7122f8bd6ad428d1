"""The channel-LayerNorm and GroupNorm dispatch of csrc/norm.hip decides what it decided before: over a fixed grid of shapes,
operand placements and knob settings every entry point returns, and launches, exactly what tests/golden/norm_dispatch.txt
records, line for line (entry point, arguments, return value -- error code, tile count or bytes -- and the kernel instantiations
in the spelling of `_C._decode_trace`).  Host-only: the SIMT-emulated build of the kernel sources runs the launches on CPU buffers.

The table is recorded from the commit BEFORE a change of the dispatch, never from the code under test.  A deliberate policy
change regenerates it from a build of the new code and shows up as a readable diff of that file:

    python tests/emul/build_emul.py && python tests/test_norm_dispatch.py > tests/golden/norm_dispatch.txt

Run as a script (optional argument: the library) this file prints the table, and fails if the grid missed an instantiation.
"""
import ctypes
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# every (segment, threads, passes) the channel-LayerNorm kernels are instantiated for: 16-byte form, 4-byte form
VEC_TILES = [(64, 256, 2), (32, 256, 4), (16, 256, 4), (8, 256, 4), (8, 512, 4), (8, 1024, 2), (4, 512, 4), (2, 512, 2), (4, 512, 8),
             (2, 512, 4), (1, 512, 2), (4, 1024, 2), (2, 1024, 1), (4, 1024, 4), (2, 1024, 2), (1, 1024, 1)]
ROW_TILES = [(64, 256, 2), (64, 256, 8), (64, 256, 16), (32, 256, 16), (32, 1024, 8), (16, 1024, 16), (8, 1024, 8), (4, 1024, 4)]
WANT = [f"{k}<{a}, {b}, {c}>" for k in ("chan_lnv_fwd_kernel", "chan_lnv_bwd_kernel", "chan_lnv_bwd_chain_kernel") for a, b, c in VEC_TILES]
WANT += [f"{k}<{a}, {b}, {c}>" for k in ("chan_ln_fwd_kernel", "chan_ln_bwd_kernel") for a, b, c in ROW_TILES]
WANT += [f"{k}<{t}>" for k in ("gn_bwd_reduce_vec_kernel", "gn_bwd_apply_vec_kernel") for t in (16, 32, 64, 256)]
WANT += [f"gn_act_slab_kernel<{s}, {n}>" for s in (0, 1, 2) for n in (1, 4)]
WANT += ["gn_bwd_reduce_kernel", "gn_bwd_apply_kernel", "gn_act_kernel", "gn_finalize_act_kernel", "gn_apply_kernel"]

CHANNELS = [1, 8, 9, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024]
KNOBS = [{}, {"ADP_LNV_NT": "1024"}, {"ADP_LNV_NT_BWD": "1024"}]
# (B, L) of the deep layers (C > 256), one on each side of every narrowing threshold.  16-byte form: B * ceil(L / (4 * lpr)) < 32
# at lpr 4 and 2 -> lpr 4, 2, 1.  4-byte form (L % 4 != 0): B * ceil(L / 16) >= 192, B * ceil(L / 8) >= 192 -> 16, 8, 4 positions.
DEEP_VEC = [(4, 128), (1, 256), (1, 16)]
DEEP_ROW = [(4, 767), (4, 383), (1, 15)]
BUF_FLOATS = 1 << 20  # 4 MiB per operand: every operand below is checked against it
FWD = ["adp_modulation_fwd", "adp_modulation_ln_fwd", "adp_ln_stats", "adp_ln_affine_fwd"]
BWD = ["adp_modulation_bwd", "adp_modulation_bwd_partial", "adp_ln_bwd", "adp_modulation_ln_bwd_partial"]
LN_ALL = FWD + ["adp_chan_ln_bwd_ws_bytes"] + BWD
# the 192-workgroup launches of the 4-byte form's wide tiles are the emulator's slowest: one forward and one backward each
LN_WIDE = ["adp_ln_stats", "adp_chan_ln_bwd_ws_bytes", "adp_modulation_bwd_partial"]
LN_VEC_WIDE = LN_WIDE + ["adp_modulation_ln_bwd_partial"]


class Run:
    def __init__(self, path):
        import numpy as np
        sys.path.insert(0, ROOT)
        from audio_diffusion_pytorch_amd import _C
        self.decode = _C._decode_trace
        self.lib = ctypes.CDLL(path)
        for name, (res, args) in _C.ABI["adp.h"].items():
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = res, args
        self.bufs = {}
        self.np = np
        self.seen = set()

    def buf(self, name, floats, off=0):
        """address of the named operand (64-byte aligned + off bytes), with room for `floats` floats checked"""
        assert 4 * floats + off + 64 <= 4 * BUF_FLOATS, (name, floats)
        if name not in self.bufs:
            self.bufs[name] = self.np.full(BUF_FLOATS, 0.5, dtype=self.np.float32)
        a = self.bufs[name].ctypes.data
        return a + (-a % 64) + off

    def traced(self, name, *args):
        self.lib.adp_launch_trace(1, None, 0)
        rv = getattr(self.lib, name)(*args)
        out = ctypes.create_string_buffer(4096)
        self.lib.adp_launch_trace(0, out, 4096)
        kernels = self.decode(out.value.decode())
        self.seen.update(k for k in kernels.split(" + ") if k)
        return f"-> {rv} : {kernels}"

    def ln(self, name, B, C, L, off=None, null=None):
        """one LayerNorm entry point at (B, C, L); off: {operand: byte offset}; null: operand passed as a null pointer"""
        off = off or {}
        assert B <= 4 or B == 65536  # (B = 0 and B = 65536 are refused before an operand is touched)
        nb = min(max(B, 1), 4)
        A, st, cv, bs = nb * C * L, nb * L * 2, 2 * C, 2 * C

        def p(n, floats=A):
            return None if n == null else self.buf(n, floats, off.get(n, 0))

        if name == "adp_chan_ln_bwd_ws_bytes":
            return f"-> {self.lib.adp_chan_ln_bwd_ws_bytes(B, C, L)} :"
        ws = self.lib.adp_chan_ln_bwd_ws_bytes(nb, C, L) // 4
        if name == "adp_modulation_fwd":
            return self.traced(name, p("x"), p("ss", nb * bs), bs, B, C, L, 1e-5, p("y"), p("stats", st), None)
        if name == "adp_modulation_ln_fwd":
            return self.traced(name, p("x"), p("ss", nb * bs), bs, B, C, L, 1e-5, p("y"), p("stats", st), 1e-5, p("gamma", cv), p("beta", cv),
                               p("xn"), p("gamma2", cv), p("beta2", cv), p("xn2"), p("ln_stats", st), None)
        if name == "adp_ln_stats":
            return self.traced(name, p("x"), B, C, L, 1e-5, p("stats", st), None)
        if name == "adp_ln_affine_fwd":
            return self.traced(name, p("x"), B, C, L, 1e-5, p("gamma", cv), p("beta", cv), p("y"), p("gamma2", cv), p("beta2", cv), p("xn2"),
                               p("stats", st), None)
        if name == "adp_modulation_bwd":
            return self.traced(name, p("x"), p("dy"), p("ss", nb * bs), bs, p("stats", st), B, C, L, p("dx"), p("dss", nb * bs), bs, p("ws", ws), None)
        if name == "adp_modulation_bwd_partial":
            return self.traced(name, p("x"), p("dy"), p("ss", nb * bs), bs, p("stats", st), B, C, L, p("dx"), p("ws", ws), None)
        if name == "adp_ln_bwd":
            return self.traced(name, p("x"), p("dy"), p("stats", st), p("gamma", cv), p("dres"), B, C, L, 0, p("dx"), p("dgd", cv), p("ws", ws), None)
        assert name == "adp_modulation_ln_bwd_partial"
        return self.traced(name, p("x"), p("ss", nb * bs), bs, p("stats", st), p("y"), p("dy"), p("gamma", cv), p("ln_stats", st), p("dres"), B, C, L,
                           0, p("dx"), p("ws", ws), p("dgd", cv), p("ws_ln", ws), None)

    def gn(self, name, B, C, L, G, NS=1, off=None, E=2):
        off = off or {}
        A = B * C * L

        def p(n, floats=A):
            return self.buf(n, floats, off.get(n, 0))

        st, ab = B * G * 2, B * C * NS * 2
        if name == "adp_gn_silu_bwd_reduce":
            return self.traced(name, p("x"), p("dy"), p("stats", st), p("gamma", C), p("beta", C), B, C, L, G, NS, p("ab", ab), None)
        if name == "adp_gn_silu_bwd_apply_ab":
            return self.traced(name, p("x"), p("dy"), p("stats", st), p("gamma", C), p("beta", C), p("ab", ab), p("dres"), B, C, L, G, NS, NS, p("dx"),
                               p("dgamma", C), p("dbeta", C), 0, None)
        if name == "adp_gn_act":
            return self.traced(name, p("x"), p("stats", st), p("gamma", C), p("beta", C), B, C, L, G, p("y"), None)
        if name == "adp_gn_finalize_act":
            return self.traced(name, p("x"), p("part", B * (C // 4) * E * 3), B, C, L, E, G, 1e-5, p("gamma", C), p("beta", C), p("stats", st), p("y"), None)
        assert name == "adp_gn_stats_act"
        ws = self.lib.adp_gn_stats_ws_bytes(B, C, L, G) // 4
        return self.traced(name, p("x"), B, C, L, G, 1e-5, p("gamma", C), p("beta", C), p("stats", st), p("y"), p("ws", ws), None)


def layer_norm_lines(r):
    def emit(knobs, place, names, B, C, L, off=None, null=None):
        os.environ.update(knobs)
        for name in names:
            print(f"{name} B{B} C{C} L{L} {place} {' '.join(f'{k}={v}' for k, v in knobs.items()) or 'knobs-unset'} " + r.ln(name, B, C, L, off, null))
        for k in knobs:
            del os.environ[k]

    for C in CHANNELS:
        deep = C > 256
        # aligned operands: the 16-byte form; the knobs move the choice from 129 channels up
        for B, L in DEEP_VEC if deep else [(2, 80)]:
            if (B, L) in DEEP_VEC[:2] and C not in (512, 513):
                continue  # (the 32-workgroup launches: on both sides of the 512-channel boundary only)
            for knobs in KNOBS if C > 128 else KNOBS[:1]:
                # the deep layers' launches are the emulator's slow ones: there a knob runs with its own direction only, and the
                # 32-workgroup launches with one entry point per kernel
                names = LN_VEC_WIDE if (B, L) in DEEP_VEC[:2] else LN_ALL
                if deep and knobs:
                    names = [n for n in names if n not in (BWD if "ADP_LNV_NT" in knobs else FWD)]
                emit(knobs, "aligned", names, B, C, L)
        # x one float off, and a length that is no multiple of 4: the 4-byte form (it reads no knob: C = 257 shows that)
        B, L = (1, 16) if deep else (2, 80)
        if C not in (512, 513):
            emit({}, "x+4", LN_ALL, B, C, L, off={"x": 4})
        B, L = (1, 15) if deep else (2, 79)
        for knobs in KNOBS if C == 257 else KNOBS[:1]:
            emit(knobs, "L%4", LN_WIDE if knobs else LN_ALL, B, C, L)
    for B, L in DEEP_ROW[:2]:
        emit({}, "L%4", LN_WIDE, B, 257, L)
    # each operand of the chained forms one float off in turn: every one of them keeps the launch off the 16-byte form
    for n in ("y", "xn2", "stats", "xn", "ln_stats"):
        emit({}, n + "+4", ["adp_modulation_ln_fwd"], 2, 8, 80, off={n: 4})
    for n in ("dy", "dres", "dx", "stats", "ln_stats", "y"):
        emit({}, n + "+4", ["adp_modulation_ln_bwd_partial"], 2, 8, 80, off={n: 4})
    # what the entry points refuse
    for B, C, L, null in ((2, 1025, 80, None), (0, 8, 80, None), (65536, 8, 80, None), (2, 8, 80, "x"), (2, 1025, 80, "x"), (0, 1025, 80, None)):
        emit({}, "aligned" + (" null-x" if null else ""), LN_ALL, B, C, L, null=null)


def group_norm_lines(r):
    def emit(name, place, B, C, L, G, NS=1, off=None):
        print(f"{name} B{B} C{C} L{L} G{G} NS{NS} {place} " + r.gn(name, B, C, L, G, NS, off))

    # backward of SiLU(GroupNorm): segment lengths CL on both sides of 64, 128 and 1024, 16-byte and row form
    for name in ("adp_gn_silu_bwd_reduce", "adp_gn_silu_bwd_apply_ab"):
        for L, NS in ((64, 1), (68, 1), (128, 1), (132, 1), (1024, 1), (1028, 1), (136, 2), (2056, 2)):
            emit(name, "aligned", 2, 4, L, 2, NS)
            emit(name, "x+4", 2, 4, L, 2, NS, off={"x": 4})
        for L, NS in ((66, 1), (130, 1), (1026, 1), (134, 2)):
            emit(name, "L%4", 2, 4, L, 2, NS)
        for n in ("dy", "ab", "dres", "dx"):
            emit(name, n + "+4", 2, 4, 64, 2, off={n: 4})
        emit(name, "ab+8", 2, 4, 64, 2, off={"ab": 8})
    # SiLU(GroupNorm) materialised: slab form (4096 elements per workgroup from 1024 workgroups up), row form
    for name in ("adp_gn_act", "adp_gn_finalize_act", "adp_gn_stats_act"):
        emit(name, "aligned", 2, 8, 64, 2)
        emit(name, "aligned", 128, 32, 4, 8)
        emit(name, "x+4", 2, 8, 64, 2, off={"x": 4})
        emit(name, "y+4", 2, 8, 64, 2, off={"y": 4})
        emit(name, "L%4", 2, 8, 63, 2)


def main():
    r = Run(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "emul", "libadp_emul.so"))
    layer_norm_lines(r)
    group_norm_lines(r)
    missing = [k for k in WANT if k not in r.seen]
    if missing:
        sys.exit(f"test_norm_dispatch: the grid never reached {missing}")


def test_norm_dispatch_table_unchanged():
    sys.path.insert(0, os.path.join(HERE, "emul"))
    import build_emul
    lib = build_emul.build()
    env = {k: v for k, v in os.environ.items() if not k.startswith("ADP_")}  # the script sets every knob it wants itself
    run = subprocess.run([sys.executable, os.path.abspath(__file__), lib], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-2000:]  # (also: an instantiation that the grid never reached)
    with open(os.path.join(HERE, "golden", "norm_dispatch.txt")) as f:
        want = f.read().splitlines()
    got = run.stdout.splitlines()
    diff = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not diff, f"{len(diff)} lines differ; first: line {diff[0][0]}\n  recorded: {diff[0][1]}\n  now:      {diff[0][2]}"
    assert len(got) == len(want)


if __name__ == "__main__":
    main()
