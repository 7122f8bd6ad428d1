"""The entry points of include/adp_enc.h with misaligned operands and guard bands (tests/placement.py), as
tests/test_lt_placement.py does for include/adp_lt.h: every operand of a direct call through `_C.lib()` is placed by the test
at the zero / all1 / mixed / single1 / single2 placements.  A placed call returns ADP_OK, agrees with the float64 reference
within the kernels' own bound (1e-4, tests/test_encoder.py) and leaves every guard, offset gap and input payload bit-identical.
Two geometries: the one on the 16-byte paths (which a misplaced pointer must leave) and the odd one."""
from audio_diffusion_pytorch_amd import _C
from placement import close, p, single_operand_tests, whole_call_tests
from test_encoder import GEOMS, TOL, case


def _dims(d):
    return d["B"], d["R"], d["M"], d["L"], d["f"]


def _fwd(P, d):
    x, w, bias = P.inp("x", d["x"]), P.inp("w", d["w"]), P.inp("bias", d["bias"])
    y = P.out("y", d["y"].shape)
    code = _C.lib().adp_enc_down_fwd(p(x), p(w), p(bias), *_dims(d), p(y), _C.stream())
    return code, [close("y", y, d["y"], TOL)]


def _dgrad(P, d):
    dy, w = P.inp("dy", d["dy"]), P.inp("w", d["w"])
    dx = P.out("dx", d["dx"].shape)
    code = _C.lib().adp_enc_down_dgrad(p(dy), p(w), *_dims(d), p(dx), _C.stream())
    return code, [close("dx", dx, d["dx"], TOL)]


def _wgrad(P, d):
    x, dy = P.inp("x", d["x"]), P.inp("dy", d["dy"])
    dw, dbias = P.out("dw", d["dw"].shape), P.out("dbias", d["dbias"].shape)
    nbytes = _C.lib().adp_enc_down_wgrad_ws_bytes(*_dims(d))
    assert nbytes > 0 and nbytes % 4 == 0
    ws = P.ws_numel("ws", nbytes // 4)
    code = _C.lib().adp_enc_down_wgrad(p(x), p(dy), *_dims(d), p(dw), p(dbias), p(ws), _C.stream())
    return code, [close("dw", dw, d["dw"], TOL), close("dbias", dbias, d["dbias"], TOL)]


def _tanh_fwd(P, d):
    h = P.inp("h", d["h"])
    z = P.out("z", d["z"].shape)
    code = _C.lib().adp_enc_tanh_fwd(p(h), h.numel(), p(z), _C.stream())
    return code, [close("z", z, d["z"], TOL)]


def _tanh_bwd(P, d):
    z, dz = P.inp("z", d["zf"]), P.inp("dz", d["dz"])
    dh = P.out("dh", d["dh"].shape)
    code = _C.lib().adp_enc_tanh_bwd(p(z), p(dz), z.numel(), p(dh), _C.stream())
    return code, [close("dh", dh, d["dh"], TOL)]


# case -> (placing function, the entry point it places); with QUERIES they must cover _C.ABI["adp_enc.h"]
CASES = {
    "down_fwd": (_fwd, "adp_enc_down_fwd"),
    "down_dgrad": (_dgrad, "adp_enc_down_dgrad"),
    "down_wgrad": (_wgrad, "adp_enc_down_wgrad"),
    "tanh_fwd": (_tanh_fwd, "adp_enc_tanh_fwd"),
    "tanh_bwd": (_tanh_bwd, "adp_enc_tanh_bwd"),
}
QUERIES = {"adp_enc_down_out_len": "length query, integers only", "adp_enc_down_wgrad_ws_bytes": "size query, integers only"}
ALL = [(n, g) for n in CASES for g in GEOMS]
test_whole_call_placements = whole_call_tests(CASES, ALL, case)
test_single_operand_placements = single_operand_tests(CASES, ALL, case)


def test_every_enc_entry_point_is_placed():
    assert {entry for _, entry in CASES.values()} | set(QUERIES) == set(_C.ABI["adp_enc.h"])
