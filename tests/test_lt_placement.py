"""The entry points of include/adp_lt.h with misaligned operands and guard bands (tests/placement.py), as
tests/test_ar_placement.py does for include/adp_ar.h: every operand of a direct call through `_C.lib()` is placed by the test
at the zero / all1 / mixed / single1 / single2 placements.  A placed call returns ADP_OK, agrees with the float64 reference
within the kernels' own bound (1e-4, tests/test_lt.py) and leaves every guard, offset gap and input payload bit-identical.
Two geometries: the one on the 16-byte paths (which a misplaced pointer must leave) and the odd one."""
from audio_diffusion_pytorch_amd import _C, ops
from placement import close, p, single_operand_tests, whole_call_tests
from test_lt import TOL, case

GEOMS = ["vec16", "odd"]   # every 16-byte access available (which a misplaced pointer must leave); odd sizes


def _conv(xk, wk, mode, refk):
    def run(P, d):
        x, w = P.inp("x", d[xk]), P.inp("w", d[wk])
        B, C, T = d[xk].shape
        O, K = d[wk].shape[0], d[wk].shape[2]
        y = P.out("y", d[refk].shape)
        code = _C.lib().adp_lt_conv(p(x), p(w), B, C, T, O, K, d["s"], d["p"], mode, p(y), _C.stream())
        return code, [close("y", y, d[refk], TOL)]
    return run


def _convt(xk, wk, mode, refk):
    def run(P, d):
        x, w = P.inp("x", d[xk]), P.inp("w", d[wk])
        B, C, L = d[xk].shape
        O, K = d[wk].shape[1], d[wk].shape[2]
        out = P.out("out", d[refk].shape)
        code = _C.lib().adp_lt_convt(p(x), p(w), B, C, L, O, K, d["s"], d["p"], mode, d["T"], p(out), _C.stream())
        return code, [close("out", out, d[refk], TOL)]
    return run


def _wgrad(uk, vk, mode, refk):
    def run(P, d):
        u, v = P.inp("u", d[uk]), P.inp("v", d[vk])
        B, A, L = d[uk].shape
        Bc, T = d[vk].shape[1], d[vk].shape[2]
        K = d["W"]
        dw = P.out("dw", d[refk].shape)
        nbytes = _C.lib().adp_lt_wgrad_ws_bytes(B, A, Bc, L, K)
        assert nbytes > 0 and nbytes % 4 == 0
        ws = P.ws_numel("ws", nbytes // 4)
        code = _C.lib().adp_lt_wgrad(p(u), p(v), B, A, Bc, L, T, K, d["s"], d["p"], mode, p(dw), p(ws), _C.stream())
        return code, [close("dw", dw, d[refk], TOL)]
    return run


# case -> (placing function, the entry point it places); with QUERIES they must cover _C.ABI["adp_lt.h"]
CASES = {
    "encode_fwd": (_conv("x", "we", ops.LT_REFLECT, "y"), "adp_lt_conv"),
    "decode_dgrad": (_conv("go", "wd", ops.LT_ZERO, "dyin"), "adp_lt_conv"),
    "decode_fwd": (_convt("yin", "wd", ops.LT_PLAIN, "out"), "adp_lt_convt"),
    "encode_dgrad": (_convt("gy", "we", ops.LT_FOLD, "dx"), "adp_lt_convt"),
    "encode_wgrad": (_wgrad("gy", "x", ops.LT_REFLECT, "dwe"), "adp_lt_wgrad"),
    "decode_wgrad": (_wgrad("yin", "go", ops.LT_ZERO, "dwd"), "adp_lt_wgrad"),
}
QUERIES = {"adp_lt_conv_out_len": "length query, integers only", "adp_lt_convt_out_len": "length query, integers only",
           "adp_lt_wgrad_ws_bytes": "size query, integers only"}
ALL = [(n, g) for n in CASES for g in GEOMS]
test_whole_call_placements = whole_call_tests(CASES, ALL, case)
test_single_operand_placements = single_operand_tests(CASES, ALL, case)


def test_every_lt_entry_point_is_placed():
    assert {entry for _, entry in CASES.values()} | set(QUERIES) == set(_C.ABI["adp_lt.h"])
