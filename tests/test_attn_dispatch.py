"""The attention dispatch of csrc/attention.hip decides what it decided before: over a fixed grid of shapes, strides and knob
settings the four entry points return, launch and write exactly what tests/golden/attn_dispatch.txt records, line for line.
Host-only: the SIMT-emulated build of the kernel sources runs the launches on CPU buffers.

A size line is `ws_bytes B H D n m -> adp_attn_fwd_ws_bytes adp_attn_bwd_ws_bytes`.  A launching line holds the entry point,
(B, H, D, n, m), the two batch strides, whether a workspace was passed, the knobs set, a null operand if any, the return value, the
kernel instantiations in the spelling of `_C._decode_trace`, and the written runs of the workspace: it is filled with a NaN of a
fixed payload before the call, and afterwards every maximal run of floats whose bits changed is listed as `start+length`, equal
runs at a constant distance as `start+length*count/distance`.  Kernel names cannot show a split count or a region offset; the
runs show all of them (and whether delta goes through the workspace at all: the merged and few-keys forms compute their own).
The script also fails if a launch writes past the size its query returned, or leaves a NaN in a result.

The table is recorded from the commit BEFORE a change of the dispatch, never from the code under test.  A deliberate policy
change regenerates it from a build of the new code and shows up as a readable diff of that file:

    python tests/emul/build_emul.py && python tests/test_attn_dispatch.py > tests/golden/attn_dispatch.txt

Run as a script (optional argument: the library) this file prints the table, and fails if the grid missed a kernel.
"""
import ctypes
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

WANT = [f"{k}<{d}>" for k in ("attn_fwd_kernel", "attn_bwd_q_kernel", "attn_bwd_kv_kernel", "attn_bwd_merged_kernel") for d in ("true", "false")]
WANT += ["attn_fwd_fewkeys_kernel", "attn_fwd_combine_kernel", "attn_bwd_fewkeys_kernel", "attn_bwd_reduce_kernel", "attn_sum_splits_kernel",
         "attn_kv_reduce_kernel"]
FILL = 0x7FC0A5A5  # the workspace and the results before a call: a quiet NaN no kernel computes
GUARD = 64         # floats behind the workspace a call was promised: never written

# size queries: n and m on both sides of every limit of the two split counts (see size_lines)
SIZE_N = [1, 32, 33, 64, 128, 129, 1024, 1025, 1056, 4096, 4097, 32768, 32769, 100000]
SIZE_M = [1, 32, 64, 65, 96, 97, 128, 288, 544, 1024, 1025, 4096, 32768, 32769]
FWD, BWD = "adp_attn_fwd", "adp_attn_bwd"
PAD = 8  # floats between batch elements of an unpacked operand


class Run:
    def __init__(self, path):
        import numpy as np
        sys.path.insert(0, ROOT)
        from audio_diffusion_pytorch_amd import _C
        self.decode = _C._decode_trace
        self.lib = ctypes.CDLL(path)
        for name in (FWD, BWD, FWD + "_ws_bytes", BWD + "_ws_bytes"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _C.SIGNATURES[name]
        self.np = np
        self.seen = set()
        self.rng = np.random.default_rng(1234)

    def array(self, floats, fill=None):
        """(64-byte aligned float32 view, its address): uniform values in [-0.5, 0.5) or the NaN fill"""
        np = self.np
        raw = np.empty(floats + 16, dtype=np.float32)
        a = raw[(-raw.ctypes.data % 64) // 4:][:floats]
        if fill is None:
            a[:] = self.rng.random(floats, dtype=np.float32) - 0.5
        else:
            a.view(np.uint32)[:] = fill
        return a, a.ctypes.data

    def traced(self, name, *args):
        self.lib.adp_launch_trace(1, None, 0)
        rv = getattr(self.lib, name)(*args)
        out = ctypes.create_string_buffer(4096)
        self.lib.adp_launch_trace(0, out, 4096)
        kernels = self.decode(out.value.decode())
        self.seen.update(k for k in kernels.split(" + ") if k)
        return rv, kernels

    def written(self, ws, promised):
        """the runs of `ws` whose bits changed, compactly; nothing behind the `promised` floats may have"""
        np = self.np
        edge = np.diff(np.concatenate(([0], (ws.view(np.uint32) != FILL).astype(np.int8), [0])))
        start, end = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
        assert len(end) == 0 or end[-1] <= promised, f"written up to float {end[-1]} of a workspace of {promised}"
        out, i = [], 0
        while i < len(start):
            j, ln = i, end[i] - start[i]
            if i + 1 < len(start):
                step = start[i + 1] - start[i]
                while j + 1 < len(start) and start[j + 1] - start[j] == step and end[j + 1] - start[j + 1] == ln:
                    j += 1
            out.append(f"{start[i]}+{ln}" + (f"*{j - i + 1}/{step}" if j > i else ""))
            i = j + 1
        return " ".join(out) or "-"

    def launch(self, entry, B, H, D, n, m, qbs=None, kvbs=None, ws=True, knobs=None, null=None):
        """one call of adp_attn_fwd / adp_attn_bwd -> (its line of the table, its results).  qbs / kvbs: batch strides in floats
        (default: packed; a kvbs below 2*H*D*m means separate k and v); ws: pass a workspace; null: the operand passed as null"""
        np, knobs = self.np, knobs or {}
        qcnt, kvcnt = H * D * n, H * D * m
        qbs, kvbs = qbs or qcnt, kvbs or 2 * kvcnt
        assert qbs >= qcnt and (kvbs >= 2 * kvcnt or kvbs == kvcnt)
        bwd = entry == BWD
        promised = max(getattr(self.lib, entry + "_ws_bytes")(B, H, D, n, m), 0) // 4 if ws else 0
        ops, res = {}, {}
        for name in ("q",) + (("o", "dout") if bwd else ()):
            ops[name] = self.array(B * qbs)
        apart = kvbs < 2 * kvcnt  # k | v in one row per batch element (v = k + kvcnt), or all of v behind all of k
        for k, v, fill in (("k", "v", None),) + ((("dk", "dv", FILL),) if bwd else ()):
            a, p = self.array(B * kvbs * (2 if apart else 1), fill)
            off = B * kvbs if apart else kvcnt
            ops[k], ops[v] = (a, p), (a[off:], p + 4 * off)
        if bwd:
            ops["lse"] = self.array(B * H * n)
            ops["lse"][0][:] = 4.0  # (above every score of these operands: the probabilities stay finite)
            ops["dq"] = self.array(B * qbs, FILL)
        else:
            ops["o"], ops["lse"] = self.array(B * qbs, FILL), self.array(B * H * n, FILL)
        ops["ws"] = self.array(promised + GUARD, FILL) if ws else (None, None)
        ptr = {k: (None if k == null else v[1]) for k, v in ops.items()}
        os.environ.update(knobs)
        if bwd:
            rv, kernels = self.traced(entry, ptr["q"], ptr["k"], ptr["v"], ptr["o"], ptr["dout"], ptr["lse"], B, H, D, n, m, qbs, kvbs,
                                      ptr["dq"], ptr["dk"], ptr["dv"], ptr["ws"], None)
        else:
            rv, kernels = self.traced(entry, ptr["q"], ptr["k"], ptr["v"], B, H, D, n, m, qbs, kvbs, ptr["o"], ptr["lse"], ptr["ws"], None)
        for k in knobs:
            del os.environ[k]
        if rv == 0:  # the addressed part of every result: rows of qcnt (kvcnt) floats at the batch stride (o, dout and lse are packed)
            for name, cnt, bs in (("dq", qcnt, qbs), ("dk", kvcnt, kvbs), ("dv", kvcnt, kvbs)) if bwd else (("o", qcnt, qcnt), ("lse", H * n, H * n)):
                a = ops[name][0]
                res[name] = np.stack([a[b * bs:b * bs + cnt] for b in range(B)]).copy()
                assert not np.isnan(res[name]).any(), (entry, name, B, H, D, n, m)
        line = (f"{entry} B{B} H{H} D{D} n{n} m{m} qbs{qbs} kvbs{kvbs} ws={'yes' if ws else 'null'} "
                f"{' '.join(f'{k}={v}' for k, v in knobs.items()) or 'knobs-unset'}{' null-' + null if null else ''} -> {rv} : {kernels}")
        return line + (" | ws " + self.written(ops["ws"][0], promised) if ws else ""), res


def size_lines(r):
    """Both size queries.  The key split (forward, dq) is min(8, key tiles / 2, 1024 / (B*H*query tiles)), rounded so that every
    slice is non-empty (m = 288, 544): the cap needs m >= 512; B*H*query tiles = 128 | 129 (n = 4096 | 4097 at B*H = 1) falls
    below 8 and 1024 | 1025 (n = 32768 | 32769) to 0.  The query split (dk, dv) is min(32, query tiles, 1024 / (B*H*key tiles)):
    B*H*key tiles = 32 | 33 (m = 1024 | 1025) leaves the cap, 1024 | 1025 (m = 32768 | 32769) falls to 0."""
    def q(B, H, D, n, m):
        print(f"ws_bytes B{B} H{H} D{D} n{n} m{m} -> {r.lib.adp_attn_fwd_ws_bytes(B, H, D, n, m)} {r.lib.adp_attn_bwd_ws_bytes(B, H, D, n, m)}")

    for B in (1, 2, 9):
        for H in (1, 4, 8):
            for D in (2, 64):
                for n in SIZE_N:
                    for m in SIZE_M:
                        q(B, H, D, n, m)
    # what attn_shape_ok refuses, next to the nearest shape it accepts
    for D in (0, 1, 2, 3, 16, 63, 64, 65, 66):
        q(1, 1, D, 64, 64)
    for B, H in ((0, 1), (1, 0), (65535, 1), (65536, 1), (1, 65535), (1, 65536), (65535, 65535)):
        q(B, H, 2, 64, 64)
    for n, m in ((0, 64), (64, 0), (-1, 64), ((1 << 25) - 1, 64), (1 << 25, 64), (64, (1 << 25) - 1), (64, 1 << 25)):
        q(1, 1, 64, n, m)  # (D * n, D * m < 2^31)
    q(1, 1, 2, (1 << 30) - 1, 64)
    q(1, 1, 2, 1 << 30, 64)


def launch_cases():
    """(entry, B, H, D, n, m, keywords of Run.launch): at least one on each side of every decision the launchers make, at the
    smallest shapes that reach it -- D = 2 unless the decision needs D = 64, one key unless it needs keys."""
    both = (FWD, BWD)
    # few keys: D = 64 and m <= 64 (forward and backward), and with the form switched off
    for e in both:
        for D, m in ((64, 64), (32, 64), (64, 65), (64, 1)):
            yield e, 1, 1, D, 33, m, {}
        yield e, 1, 1, 64, 33, 64, {"knobs": {"ADP_ATTN_FEWKEYS": "0"}}
        yield e, 2, 3, 64, 33, 64, {}
    # few-keys backward: its query split ns4 = 1 (one query tile) | 2 | 3 of the 5 that the query split of dk | dv allows | 1 of 2 by the knob
    yield BWD, 1, 1, 64, 32, 1, {}
    yield BWD, 1, 1, 64, 160, 1, {}
    yield BWD, 1, 1, 64, 160, 1, {"knobs": {"ADP_ATTN_FK_SLICES": "3"}}
    yield BWD, 1, 1, 64, 33, 1, {"knobs": {"ADP_ATTN_FK_SLICES": "1"}}
    yield BWD, 1, 1, 64, 33, 1, {"knobs": {"ADP_ATTN_FK_SLICES": "-5"}}
    # ... and its work limit B * H * query tiles <= 512 at B * H > 8, <= 1024 up to 8 (the emulator's slowest launches)
    for H, n in ((9, 1792), (9, 1793), (8, 4096), (8, 4097)):
        yield BWD, 1, H, 64, n, 1, {}
    # merged | split by the default rule (workgroups of both passes * H * B * 4 <= 1024: 4 | 6 at H = 64), and forced
    for n in (256, 257):
        for knobs in ({}, {"ADP_ATTN_MERGE": "0"}, {"ADP_ATTN_MERGE": "1"}):
            yield BWD, 1, 64, 2, n, 1, {"knobs": knobs}
    # the four cases of (ns, nq) in {1, > 1}, merged and split; both forms at D = 64 and at 16
    for n, m in ((32, 1), (64, 1), (32, 128), (64, 128)):
        for knobs in ({"ADP_ATTN_MERGE": "1"}, {"ADP_ATTN_MERGE": "0"}):
            yield BWD, 1, 1, 2, n, m, {"knobs": knobs}
    for D in (64, 16):
        for knobs in ({}, {"ADP_ATTN_MERGE": "0"}):
            yield BWD, 2, 1, D, 64, 128, {"knobs": knobs}
    # key slices that would be empty are dropped: 9 key tiles in 4 slices -> 3 of 3; 17 in 8 -> 6 of 3
    for e in both:
        for m in (288, 544):
            yield e, 1, 1, 2, 32, m, {}
    # the forward's key split needs the workspace
    for D in (2, 64):
        yield FWD, 1, 1, D, 32, 128, {"ws": False}
        yield FWD, 1, 1, D, 32, 128, {}
    yield FWD, 2, 3, 16, 160, 200, {}
    # strides.  q unpacked: no key split of dq (packed: nq = 2).  kv unpacked: refused when dk | dv are split (before the few-keys
    # form is looked at), served when they are not.  k and v apart (kv_bstride = H*D*m): smaller partial copies
    for knobs in ({}, {"ADP_ATTN_MERGE": "0"}):
        yield BWD, 2, 1, 2, 64, 128, {"qbs": 2 * 64 + PAD, "knobs": knobs}
        yield BWD, 2, 1, 2, 64, 128, {"kvbs": 2 * 128, "knobs": knobs}
    yield BWD, 2, 1, 2, 64, 128, {"kvbs": 2 * 2 * 128 + PAD}
    yield BWD, 2, 1, 64, 64, 1, {"kvbs": 2 * 64 + PAD}
    yield BWD, 2, 1, 64, 64, 1, {"kvbs": 64}
    yield BWD, 2, 1, 2, 32, 128, {"qbs": 2 * 32 + PAD, "kvbs": 2 * 2 * 128 + PAD}
    yield BWD, 2, 1, 64, 32, 1, {"qbs": 64 * 32 + PAD, "kvbs": 2 * 64 + PAD}
    yield FWD, 2, 1, 2, 32, 128, {"qbs": 2 * 32 + PAD, "kvbs": 2 * 2 * 128 + PAD}
    yield FWD, 2, 1, 64, 32, 1, {"qbs": 64 * 32 + PAD, "kvbs": 2 * 64 + PAD}
    # refusals, in their order: a null operand, then the shape, then the strides
    for e in both:
        for null in ("q", "k", "v", "o", "lse") + (("dout", "dq", "dk", "dv", "ws") if e == BWD else ()):
            yield e, 1, 1, 2, 32, 1, {"null": null}
        yield e, 1, 1, 3, 32, 1, {"null": "q"}
        yield e, 1, 1, 3, 32, 1, {}
        yield e, 1, 1, 66, 32, 1, {}
    yield BWD, 2, 1, 3, 64, 1, {"kvbs": 2 * 3 * 1 + PAD}


def main():
    r = Run(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "emul", "libadp_emul.so"))
    size_lines(r)
    for entry, B, H, D, n, m, kw in launch_cases():
        print(r.launch(entry, B, H, D, n, m, **kw)[0], flush=True)
    missing = [k for k in WANT if k not in r.seen]
    if missing:
        sys.exit(f"test_attn_dispatch: the grid never reached {missing}")


def test_attn_dispatch_table_unchanged():
    sys.path.insert(0, os.path.join(HERE, "emul"))
    import build_emul
    lib = build_emul.build()
    env = {k: v for k, v in os.environ.items() if not k.startswith("ADP_")}  # the script sets every knob it wants itself
    run = subprocess.run([sys.executable, os.path.abspath(__file__), lib], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-2000:]  # (also: a kernel that the grid never reached)
    with open(os.path.join(HERE, "golden", "attn_dispatch.txt")) as f:
        want = f.read().splitlines()
    got = run.stdout.splitlines()
    diff = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not diff, f"{len(diff)} lines differ; first: line {diff[0][0]}\n  recorded: {diff[0][1]}\n  now:      {diff[0][2]}"
    assert len(got) == len(want)


if __name__ == "__main__":
    main()
