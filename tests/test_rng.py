"""include/adp_rng.h: the Philox4x32-10 generator, its normals and the inpainting step that draws them in registers.

The contract is the published algorithm, restated here in plain Python integers (`philox4x32_10`, checked first against the
Random123 known-answer vectors) and a float64 Box-Muller (`normals_ref`):

  group g of draw d under seed s : counter (lo32(g), hi32(g), d, 0), key (lo32(s), hi32(s))
  u = ((r >> 8) + 0.5) 2^-24 ; z_even = sqrt(-2 ln u_a) cos(2 pi u_b) ; z_odd = sqrt(-2 ln u_a) sin(2 pi u_b)

Bounds.  Words: exact.  Normals: 1e-5 absolute -- |z| <= sqrt(2 * 25 * ln 2) = 5.89, one ulp at that size is 4.8e-7, the
rounding of 2 pi u (up to 4.8e-7) is multiplied by the radius, and three library calls contribute a few ulp each.  Fused step:
1e-6 in the max norm, the bound tests/test_kernels.py::test_v_noise_mse_step and tests/test_operand_placement.py hold
adp_v_step / adp_v_inpaint_step to.
"""
import ctypes
import math

import pytest
import torch

from audio_diffusion_pytorch_amd import _C, ops
from conftest import rel_err

M32 = 0xFFFFFFFF
NORMAL_TOL = 1e-5
STEP_TOL = 1e-6
SEEDS = [0, 2 ** 64 - 1, 0x299F31D0A4093822]
DRAWS = [0, 1, 2 ** 32 - 1]


# ------------------------------------------------------------------ the restatement
def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def words_ref(seed, draw, n_words):
    out = []
    for g in range((n_words + 3) // 4):
        out.extend(philox4x32_10((g & M32, g >> 32, draw, 0), (seed & M32, seed >> 32)))
    return out[:n_words]


def normals_ref(words):
    """float64 Box-Muller on a whole number of groups of words (a torch.int64 tensor of values in [0, 2^32))."""
    u = ((words >> 8).double() + 0.5) * 2.0 ** -24
    ua, ub = u[0::2], u[1::2]
    radius = torch.sqrt(-2.0 * torch.log(ua))
    z = torch.stack([radius * torch.cos(2 * math.pi * ub), radius * torch.sin(2 * math.pi * ub)], dim=1)
    return z.reshape(-1)


def as_u32(t):
    """int32 bit patterns -> the uint32 values as int64."""
    return t.cpu().to(torch.int64) & M32


def row(seed, draw, dev):
    return ops.rng_rows(seed, [draw])[0].to(dev)


_REF = {}


def reference(seed, draw, n):
    """(words, normals) of the first n elements of a row's stream; computed once per row and length, never modified."""
    key = (seed, draw, n)
    if key not in _REF:
        words = torch.tensor(words_ref(seed, draw, (n + 3) // 4 * 4), dtype=torch.int64)
        _REF[key] = (words, normals_ref(words)[:n])
    return _REF[key]


def guarded(n, dtype, dev, guard=64):
    """A NaN / -1 prefilled buffer with guard bands on both sides and the payload view (16-byte aligned start)."""
    fill = float("nan") if dtype == torch.float32 else -1
    back = torch.full((guard + n + guard,), fill, dtype=dtype, device=dev)
    return back, back[guard:guard + n]


def guards_intact(back, n, guard=64):
    lo, hi = back[:guard].cpu(), back[guard + n:].cpu()
    if back.dtype == torch.float32:
        return bool(torch.isnan(lo).all() and torch.isnan(hi).all())
    return bool((lo == -1).all() and (hi == -1).all())


# ------------------------------------------------------------------ 1. the generator, exact
def test_restatement_reproduces_the_known_answer_vectors():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((M32,) * 4, (M32,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join(f"{w:08x}" for w in philox4x32_10(ctr, key)) == want


def test_rng_rows_layout():
    rows = ops.rng_rows(0x299F31D0A4093822, [0, 5, 2 ** 32 - 1])
    assert rows.dtype == torch.int32 and rows.shape == (3, 4)
    assert as_u32(rows).tolist() == [[0xA4093822, 0x299F31D0, 0, 0], [0xA4093822, 0x299F31D0, 5, 0],
                                    [0xA4093822, 0x299F31D0, M32, 0]]
    for bad in (dict(seed=-1, draws=[0]), dict(seed=2 ** 64, draws=[0]), dict(seed=0, draws=[2 ** 32])):
        with pytest.raises(ValueError):
            ops.rng_rows(**bad)


@pytest.mark.parametrize("draw", DRAWS)
@pytest.mark.parametrize("seed", SEEDS)
def test_philox_bits_equal_the_restatement(dev, seed, draw):
    r = row(seed, draw, dev)
    for n in (1, 3, 4, 5, 4 * 257 + 2):
        back, out = guarded(n, torch.int32, dev)
        assert ops.philox_bits(n, r, out=out) is out
        assert as_u32(out).tolist() == words_ref(seed, draw, n), (seed, draw, n)
        assert guards_intact(back, n)
    if seed == 0 and draw == 0:
        assert as_u32(ops.philox_bits(4, r)).tolist() == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    # the row's last word is reserved: the stream does not depend on it
    r2 = r.clone()
    r2[3] = 12345
    assert torch.equal(ops.philox_bits(9, r2), ops.philox_bits(9, r))


# ------------------------------------------------------------------ 2. normals
@pytest.mark.parametrize("seed,draw", [(0, 0), (2 ** 64 - 1, 2 ** 32 - 1), (0x299F31D0A4093822, 1)])
def test_randn_matches_float64_box_muller(dev, seed, draw):
    r = row(seed, draw, dev)
    worst = 0.0
    for n in (1, 3, 4, 5, 1023, 4096 + 3):
        back, out = guarded(n, torch.float32, dev)
        assert ops.randn((n,), r, out=out) is out
        dev_max = (out.cpu().double() - reference(seed, draw, n)[1]).abs().max().item()
        print(f"adp_randn seed={seed:#x} draw={draw} n={n}: max abs deviation {dev_max:.3e} (bound {NORMAL_TOL:.0e})")
        worst = max(worst, dev_max)
        assert guards_intact(back, n), n
        assert torch.equal(ops.randn((n,), r), out), "two calls with the same row differ"
    assert worst < NORMAL_TOL, worst


# (draw, group, first word of the pair) under seed 7 whose u_a = (k + 0.5) 2^-24 has k = 2^24 - 1 (twice) and k = 0 (twice):
# found by running the restatement over draws < 2^17 and groups < 256; the test re-derives each k before it relies on it
CORNERS = [(50328, 4, 0, 2 ** 24 - 1), (52329, 107, 2, 2 ** 24 - 1), (82433, 247, 0, 0), (29247, 244, 2, 0)]


@pytest.mark.parametrize("draw,group,lane,k", CORNERS)
def test_randn_where_u_is_next_to_one_or_zero(dev, draw, group, lane, k):
    """Box-Muller's corners.  k = 2^24 - 1: u_a = 1 - 2^-25 needs 25 bits, one more than a float holds, and the radius is
    sqrt(2^-24) = 2.4e-4 -- a u_a rounded to a float (1.0) would give 0, off by 24 times the bound.  k = 0: the radius is at
    its cap, sqrt(50 ln 2) = 5.89, where the angle's rounding weighs most."""
    seed, n = 7, 1024
    words, z = reference(seed, draw, n)
    assert int(words[4 * group + lane]) >> 8 == k
    out = ops.randn((n,), row(seed, draw, dev)).cpu().double()
    lo = 4 * group + lane
    radius = math.hypot(*z[lo:lo + 2].tolist())
    assert radius == pytest.approx(math.sqrt(-2 * math.log((k + 0.5) * 2.0 ** -24)), rel=1e-12)
    err = (out[lo:lo + 2] - z[lo:lo + 2]).abs().max().item()
    print(f"k = {k}: radius {radius:.6e}, z = {z[lo:lo + 2].tolist()}, deviation {err:.3e} (bound {NORMAL_TOL:.0e})")
    assert err < NORMAL_TOL
    assert (out - z).abs().max().item() < NORMAL_TOL


def test_randn_streams_are_distinct(dev):
    n = 4096
    base = ops.randn((n,), row(11, 5, dev))
    for other in (row(11, 6, dev), row(12, 5, dev), row(11 + 2 ** 32, 5, dev)):
        assert not (ops.randn((n,), other) == base).any()


def test_randn_moments(dev):
    n = 2 ** 20
    z = ops.randn((n,), row(2024, 1, dev)).cpu().double()
    mean, var = z.mean().item(), z.var(unbiased=True).item()
    print(f"n = 2^20: mean {mean:.3e} (bound {5 / math.sqrt(n):.3e}), var - 1 {var - 1:.3e} (bound {5 * math.sqrt(2 / n):.3e}), "
          f"max |z| {z.abs().max().item():.3f}")
    assert abs(mean) < 5 / math.sqrt(n)
    assert abs(var - 1) < 5 * math.sqrt(2 / n)
    assert z.abs().max().item() <= 5.9
    assert torch.isfinite(z).all()


def test_randn_shape_like_and_wrapper_errors(emul):
    r = row(1, 0, emul)
    like = torch.empty(2, 3, 5)
    out = ops.randn(like, r)
    assert out.shape == like.shape and torch.equal(out.reshape(-1), ops.randn((30,), r))
    with pytest.raises(ValueError, match="rng4"):
        ops.randn(like, r.to(torch.int64))
    with pytest.raises(ValueError, match="rng4"):
        ops.randn(like, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        ops.randn(like, r, out=torch.empty(30))
    with pytest.raises(ValueError, match="shape"):
        ops.v_inpaint_step_rng(like, like, like, torch.zeros(2, 3, 4, dtype=torch.uint8), torch.zeros(4), r)


# ------------------------------------------------------------------ 3. the fused step
def step_ref(x, v, src, z, mask, ab4):
    a0, b0, a1, b1 = (float(c) for c in ab4.double())
    x, v = x.double(), v.double()
    rotated = a1 * (a0 * x - b0 * v) + b1 * (b0 * x + a0 * v)
    return torch.where(mask.bool(), a1 * src.double() + b1 * z.double(), rotated)


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("mask_kind", ["all-true", "all-false", "random"])
@pytest.mark.parametrize("shape", [(2, 3, 5), (1, 2, 64), (3, 1, 1027)])
def test_fused_step_matches_formula_fed_by_randn(dev, shape, mask_kind, inplace):
    g = torch.Generator().manual_seed(sum(shape))
    x, v, src = [torch.randn(shape, generator=g) for _ in range(3)]
    mask = {"all-true": torch.ones(shape), "all-false": torch.zeros(shape),
            "random": (torch.rand(shape, generator=g) > 0.5)}[mask_kind].to(torch.uint8)
    ab4 = torch.tensor([0.3, 0.9, 0.5, 0.8])
    r = row(99, 4, dev)
    z = ops.randn(shape, r).cpu()
    want = step_ref(x, v, src, z, mask, ab4)
    dx, dv, dsrc, dmask, dab = [t.clone().to(dev) for t in (x, v, src, mask, ab4)]   # (on the CPU .to() is the tensor itself)
    n = x.numel()
    if inplace:
        out = ops.v_inpaint_step_rng(dx, dv, dsrc, dmask, dab, r, out=dx)
        assert out is dx
    else:
        back, view = guarded(n, torch.float32, dev)
        out = ops.v_inpaint_step_rng(dx, dv, dsrc, dmask, dab, r, out=view.view(shape))
        assert guards_intact(back, n) and torch.equal(dx.cpu(), x)
    assert torch.equal(dv.cpu(), v) and torch.equal(dsrc.cpu(), src) and torch.equal(dmask.cpu(), mask)
    err = rel_err(out, want)
    print(f"adp_v_inpaint_step_rng {shape} {mask_kind} inplace={inplace}: rel_err {err:.3e} (bound {STEP_TOL:.0e})")
    assert torch.isfinite(out).all() and err < STEP_TOL
    if mask_kind == "all-false":   # no element needs noise: the step is adp_v_step's rotation
        assert torch.equal(out.cpu(), ops.v_step(x.to(dev), dv, dab).cpu())


# ------------------------------------------------------------------ 4. C-ABI
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def test_c_abi_error_codes(dev):
    L = _C.lib()
    s = _C.stream()
    n = 8
    r = row(1, 2, dev)
    f = [torch.zeros(n + 4, device=dev) for _ in range(4)]
    x, v, src, out = f
    mask = torch.zeros(n + 4, dtype=torch.uint8, device=dev)
    ab4 = torch.tensor([0.3, 0.9, 0.5, 0.8], device=dev)
    words = torch.zeros(n + 4, dtype=torch.int32, device=dev)

    def off(t, nbytes):
        return ctypes.c_void_p(t.data_ptr() + nbytes)

    out.fill_(float("nan"))
    words.fill_(-1)
    # NULL pointers: -5
    assert L.adp_randn(None, n, _p(out), s) == -5 and L.adp_randn(_p(r), n, None, s) == -5
    assert L.adp_philox_bits(None, n, _p(words), s) == -5 and L.adp_philox_bits(_p(r), n, None, s) == -5
    good = [_p(x), _p(v), _p(src), _p(mask), _p(ab4), _p(r)]
    for i in range(6):
        args = list(good)
        args[i] = None
        assert L.adp_v_inpaint_step_rng(*args, n, _p(out), s) == -5, i
    assert L.adp_v_inpaint_step_rng(*good, n, None, s) == -5
    # a negative n: -1
    assert L.adp_randn(_p(r), -1, _p(out), s) == -1
    assert L.adp_philox_bits(_p(r), -1, _p(words), s) == -1
    assert L.adp_v_inpaint_step_rng(*good, -1, _p(out), s) == -1
    # pointers below their element's alignment: -3
    for nbytes in (1, 2, 3):
        assert L.adp_randn(off(r, nbytes), n, _p(out), s) == -3
        assert L.adp_randn(_p(r), n, off(out, nbytes), s) == -3
        assert L.adp_philox_bits(off(r, nbytes), n, _p(words), s) == -3
        assert L.adp_philox_bits(_p(r), n, off(words, nbytes), s) == -3
    for i in (0, 1, 2, 4, 5):   # (mask is bytes: any address)
        args = list(good)
        args[i] = off((x, v, src, mask, ab4, r)[i], 2)
        assert L.adp_v_inpaint_step_rng(*args, n, _p(out), s) == -3, i
    assert L.adp_v_inpaint_step_rng(*good, n, off(out, 2), s) == -3
    # n = 0 is fine and launches nothing
    assert L.adp_randn(_p(r), 0, _p(out), s) == 0 and L.adp_philox_bits(_p(r), 0, _p(words), s) == 0
    assert L.adp_v_inpaint_step_rng(*good, 0, _p(out), s) == 0
    # a refused call wrote nothing
    assert torch.isnan(out.cpu()).all() and (words.cpu() == -1).all()
    # float-aligned (not 16-byte aligned) operands and a byte-offset mask are served, with the same values
    assert L.adp_randn(_p(r), n, off(out, 4), s) == 0
    assert torch.equal(out[1:1 + n].cpu(), ops.randn((n,), r).cpu()) and torch.isnan(out[0].cpu()) and torch.isnan(out[n + 1:].cpu()).all()
    assert L.adp_v_inpaint_step_rng(_p(x), _p(v), _p(src), off(mask, 1), _p(ab4), _p(r), n, _p(out), s) == 0
    assert torch.isfinite(out[:n].cpu()).all()
