"""The entry points of include/adp_ar.h with misaligned operands and guard bands (tests/placement.py), as
tests/test_operand_placement.py does for include/adp.h: every operand of a direct call through `_C.lib()` is placed by the
test at the zero / all1 / mixed / single1 / single2 placements.  A placed call returns ADP_OK, agrees with the fp64 formula
within the kernels' own bound (1e-6, tests/test_ar.py) and leaves every guard, offset gap and input payload bit-identical."""
from audio_diffusion_pytorch_amd import _C
from placement import close, exact, p, single_operand_tests, whole_call_tests
from test_ar import KERNEL_TOL, case_data, noise_ref, per_position, step_ref

# (B, C, T, N): l a multiple of 4 (the 16-byte paths where the pointers allow them), l = 7, and one split
SHAPES = {"shape0": (2, 3, 2048, 8), "shape1": (3, 2, 35, 5), "shape2": (1, 2, 300, 1)}


def arv_noise(P, shape):
    B, C, T, N = shape
    x, v, sigma, _ = case_data(B, C, T, N, seed=3)
    xd, vd, sd = P.inp("x", x), P.inp("noise", v), P.inp("sigma", sigma)
    xn, vt, plane = P.out("x_noisy", (B, C, T)), P.out("v_target", (B, C, T)), P.out("sigma_plane", (B, T))
    code = _C.lib().adp_arv_noise(p(xd), p(vd), p(sd), B, C, T, N, p(xn), p(vt), p(plane), _C.stream())
    xn_ref, vt_ref, plane_ref = noise_ref(x, v, sigma)
    return code, [close("x_noisy", xn, xn_ref, KERNEL_TOL), close("v_target", vt, vt_ref, KERNEL_TOL),
                  exact("sigma_plane", plane, plane_ref[:, 0].float())]


def arv_step(P, shape):
    B, C, T, N = shape
    x, v, _, coef = case_data(B, C, T, N, seed=4)
    xd, vd, cd = P.inp("x", x), P.inp("v", v), P.inp("coef", coef)
    xo, plane = P.out("x_out", (B, C, T)), P.out("sigma_plane_out", (B, T))
    code = _C.lib().adp_arv_step(p(xd), p(vd), p(cd), B, C, T, N, p(xo), p(plane), _C.stream())
    out_ref, next_ref = step_ref(x, v, coef)
    l = T // N
    return code, [close("x_out", xo, out_ref, KERNEL_TOL), exact("sigma_plane_out", plane, next_ref.float().expand(B, T)),
                  exact("context split", xo[..., :l], x[..., :l])]


def arv_step_in_place(P, shape):
    """x_out = x and no plane: the form the captured sampler step's first operand takes."""
    B, C, T, N = shape
    x, v, _, coef = case_data(B, C, T, N, seed=5)
    xd, vd, cd = P.inout("x", x), P.inp("v", v), P.inp("coef", coef)
    code = _C.lib().adp_arv_step(p(xd), p(vd), p(cd), B, C, T, N, p(xd), None, _C.stream())
    l = T // N
    return code, [close("x", xd, step_ref(x, v, coef)[0], KERNEL_TOL), exact("context split", xd[..., :l], x[..., :l])]


def arv_plane(P, shape):
    B, C, T, N = shape
    sigma = case_data(B, C, T, N, seed=6)[2][0].contiguous()
    sd, plane = P.inp("sigma", sigma), P.out("sigma_plane", (B, T))
    code = _C.lib().adp_arv_plane(p(sd), B, T, N, p(plane), _C.stream())
    return code, [exact("sigma_plane", plane, per_position(sigma, T).expand(B, T))]


# case -> the entry point it places; together they must cover _C.ABI["adp_ar.h"]
CASES = {"arv_noise": (arv_noise, "adp_arv_noise"), "arv_step": (arv_step, "adp_arv_step"),
         "arv_step_in_place": (arv_step_in_place, "adp_arv_step"), "arv_plane": (arv_plane, "adp_arv_plane")}
ALL = [(n, s) for n in CASES for s in SHAPES]
test_whole_call_placements = whole_call_tests(CASES, ALL, SHAPES.get)
test_single_operand_placements = single_operand_tests(CASES, ALL, SHAPES.get)


def test_every_ar_entry_point_is_placed():
    assert {entry for _, entry in CASES.values()} == set(_C.ABI["adp_ar.h"])
