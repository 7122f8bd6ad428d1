"""Karras (EDM) diffusion: `KDiffusion`, `KSampler`, `KarrasSchedule`, `LogNormalDistribution` and the kernels of
include/adp_edm.h.

Nothing in the reference provides it, so the contract is the mathematics, restated here in float64 (`edm_table`,
`edm_step_ref`, `edm_sample_ref`, `edm_loss_ref`: plain Python over torch tensors).  `edm_sample_ref` and `edm_loss_ref` work
on the UNSCALED state x, as the paper writes it, so the product's scaled-state algebra is checked and not restated.  With
sd = sigma_data, r = sqrt(s^2 + sd^2):

  c_in = 1 / r ; c_skip = sd^2 / r^2 ; c_out = s sd / r ; D(x, s) = c_skip x + c_out F(c_in x, ln(s) / 4)
  training   loss = loss_fn(F(c_in (x + s n), ln(s) / 4), (x - c_skip (x + s n)) / c_out)
  sampling   D_i = D(x_i, s_i) ; nh_i = (x_i - D_i) / s_i ; x0c_i = D_i | clamp(D_i, -1, 1) | clamp(D_i, -q_r, q_r) / q_r
             up = min(s', eta sqrt(s'^2 (s^2 - s'^2) / s^2)) ; down = sqrt(s'^2 - up^2)           (s = s_i, s' = s_{i+1})
             x_{i+1} = x0c_i + down nh_i + up z_i + (1 - s' / s) (h_i / (2 h_{i-1})) (x0c_i - x0c_{i-1})
             h_i = ln(s_i / s_{i+1}); the last term for order 2, i > 0 and s' > 0 only (DPM-Solver++(2M))
  kernel     on xs = c_in(s_i) x_i:  x0 = a0 xs - b0 F ; nh = e0 xs + f0 F ; xs' = c1 x0c + d1 nh + cb (x0c - hist) + s1 z

Kernel errors are measured in the max norm relative to the largest INPUT magnitude A, not to the largest output: the bound
then follows from the coefficients alone, before any output is seen.

STEP_TOL.  The header fixes the kernel's sequence: b0 * F and the fused multiply-add behind it (2 roundings), the division by
the scale (1), the multiply-add with d1 nh (1) and the two closing multiply-adds (2): 6 float32 roundings on the longest path
(the path through x0c - hist has 6 as well), counted as at most 8 roundings of 2**-24 as tests/test_rf.py counts its own.  Every rounded value, times the coefficients it still passes through, is at most G * A with the row's
gain G = (|c1| + |cb|) (|a0| + |b0|) + |d1| (|e0| + |f0|) + |cb| + |s1| (the sum of the absolute values of every term of the
update for inputs of magnitude A; the clamps and the division by a scale >= 1 only shrink).  For sd = 0.5: |a0| + |b0| =
sd (sd + s) / r <= 0.71, |e0| + |f0| <= 1.42, c1 = g <= 1 / sd = 2, d1, s1 <= g s' <= 1 and |cb| <= g h_i / (2 h_{i-1}),
about 1.1 for the rows used here: G <= 5, which `_rows` asserts on the float64 rows before any kernel runs.
8 * 2**-24 * 5 = 2.4e-6; the bound is twice that, 4.8e-6, as STEP_TOL of tests/test_rf.py doubles its own count.

NOISE_TOL.  r = sqrt(fma(s, s, sd * sd)), a quotient or two, one product and the closing multiply-add: 6 roundings on the
longest path, counted as at most 8.  With x = sd * (unit data) and A = max(|x| / sd, |n|), both outputs are sums of two terms
whose coefficients satisfy c_in sd + c_n = (sd + s) / r <= 1.42 and t_x sd + t_n = (s + sd) / r <= 1.42: every rounded value
is at most 2 A.  8 * 2**-24 * 2 = 9.5e-7, doubled: 1.9e-6.
"""
import copy
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import audio_diffusion_pytorch_amd as adp
from audio_diffusion_pytorch_amd import diffusion, graphed, ops
from conftest import rel_err
from oracle import vdiffusion as ovd
from oracle.a_unet_restatement import AppendChannelsOracle, UNetV0Oracle
from test_multistep_sampler import PARITY_TOL, GaussianV
from test_threshold_sampler import OUT_GAIN, clip_ref
from test_unet import TINY, FixedSigmas, compare_grads
from test_unet import TOL as UNET_TOL

STEP_GAIN = 5.0
STEP_TOL = 2 * (8 * 2.0 ** -24 * STEP_GAIN)   # 4.8e-6 of the largest input (module docstring)
NOISE_TOL = 2 * (8 * 2.0 ** -24 * 2)          # 1.9e-6 of the largest input (module docstring)
LOOP_TOL = 1e-5                               # sampler against the restatement on the same net and backend (tests/test_inpaint_graph.py)
SD = 0.5
SEED = 0x2C91E5A70B3D48F6
assert STEP_TOL <= 5e-6


def err_in(got, want, *inputs) -> float:
    """||got - want||_inf over the largest input magnitude (module docstring)."""
    a = max(t.detach().double().abs().max().item() for t in inputs)
    return (got.detach().double().cpu() - want.detach().double().cpu()).abs().max().item() / a


# ------------------------------------------------------------------ float64 restatement of the contract
def edm_table(sigmas: torch.Tensor, sd: float = SD, order: int = 2, eta: float = 0.0) -> torch.Tensor:
    """Rows (a0, b0, e0, f0, c1, d1, s1, cb) in float64 for sigma_0..sigma_N."""
    s = [float(v) for v in sigmas.double()]
    n = len(s) - 1
    rows = []
    for i in range(n):
        s0, s1 = s[i], s[i + 1]
        r0 = math.sqrt(s0 * s0 + sd * sd)
        g = 1.0 if i == n - 1 else 1.0 / math.sqrt(s1 * s1 + sd * sd)
        up = min(s1, eta * math.sqrt(s1 * s1 * (s0 * s0 - s1 * s1) / (s0 * s0)))
        down = math.sqrt(max(s1 * s1 - up * up, 0.0))
        cb = 0.0
        if order == 2 and i > 0 and s1 > 0:
            cb = g * (1 - s1 / s0) * math.log(s0 / s1) / (2 * math.log(s[i - 1] / s0))
        rows.append([sd * sd / r0, -s0 * sd / r0, s0 / r0, -sd / r0, g, g * down, g * up, cb])
    return torch.tensor(rows, dtype=torch.float64).reshape(n, 8)


def edm_step_ref(xs, f, hist, row, z=None, clip=False, scale=None):
    """One kernel update in float64 on the scaled state: (xs_next, x0c).  `scale` [B] or None; clip without a scale is the
    static clamp.  nh comes from the raw f; the history is not used where cb = 0, z not where s1 = 0."""
    xs, f = xs.double(), f.double()
    a0, b0, e0, f0, c1, d1, s1, cb = [r.double() for r in row]
    x0, nh = a0 * xs - b0 * f, e0 * xs + f0 * f
    if clip and scale is not None:
        s = diffusion.pad_dims(scale.double(), xs.ndim - 1)
        x0 = x0.clamp(-s, s) / s
    elif clip:
        x0 = x0.clamp(-1.0, 1.0)
    xn = c1 * x0 + d1 * nh
    if cb != 0:
        xn = xn + cb * (x0 - hist.double())
    if s1 != 0:
        xn = xn + s1 * z.double()
    return xn, x0


def draw(seed, d, like):
    """Draw d of the seed in the shape of `like`, from the library's generator on `like`'s backend."""
    return ops.randn(like, ops.rng_rows(seed, [d])[0].to(like.device))


@torch.no_grad()
def edm_sample_ref(net, noise, sigmas, sd=SD, order=2, eta=0.0, seed=SEED, q=None, start=None, stats=None, **kw):
    """The sampler in float64 on the UNSCALED state, from start + sigma_0 noise.  `net` runs in float32 wherever `noise`
    lives and is given (c_in x, ln(sigma) / 4); the noise of step i is draw 1 + i from `ops.randn` there.  `q`: None, 0.0
    (static clamp) or a quantile; `stats`, a list, receives per step (scale row or None, max |D|)."""
    dev = noise.device
    s32 = sigmas.to(torch.float32)
    c_noise = torch.log(s32[:-1].to(dev)) * 0.25           # (the float32 values the product forms, on the same backend)
    s = [float(v) for v in s32.double()]
    n = len(s) - 1
    x = s[0] * noise.double() + (0.0 if start is None else start.double())
    old = None
    for i in range(n):
        s0, s1 = s[i], s[i + 1]
        r = math.sqrt(s0 * s0 + sd * sd)
        out = net((x / r).float(), c_noise[i].expand(x.shape[0]), **kw).double()
        d = (sd * sd / (r * r)) * x + (s0 * sd / r) * out
        nh = (x - d) / s0
        scale = None
        if q:
            scale = clip_ref(d.cpu(), q)[1].to(dev)
        if stats is not None:
            stats.append((None if scale is None else scale.cpu(), d.abs().max().item()))
        if q is not None:
            if scale is None:
                x0c = d.clamp(-1.0, 1.0)
            else:
                sc = diffusion.pad_dims(scale, x.ndim - 1)
                x0c = d.clamp(-sc, sc) / sc
        else:
            x0c = d
        up = min(s1, eta * math.sqrt(s1 * s1 * (s0 * s0 - s1 * s1) / (s0 * s0)))
        down = math.sqrt(max(s1 * s1 - up * up, 0.0))
        xn = x0c + down * nh
        if up != 0:
            xn = xn + up * draw(seed, 1 + i, x.float()).double()
        if order == 2 and i > 0 and s1 > 0:
            xn = xn + (1 - s1 / s0) * (math.log(s0 / s1) / (2 * math.log(s[i - 1] / s0))) * (x0c - old)
        x, old = xn, x0c
    return x


def edm_loss_ref(net, x, noise, sigma, sd=SD, loss_fn=F.mse_loss, **kw):
    """The training loss on a float32 net (the oracle), with the preconditioning done in float64 and rounded once."""
    s = diffusion.pad_dims(sigma.double(), x.ndim - 1)
    r2 = s * s + sd * sd
    xn = x.double() + s * noise.double()
    x_in = (xn / torch.sqrt(r2)).float()
    target = ((x.double() - (sd * sd / r2) * xn) / (s * sd / torch.sqrt(r2))).float()
    return loss_fn(net(x_in, torch.log(sigma.float()) * 0.25, **kw), target)


class GaussianF(nn.Module):
    """The optimal EDM net output for data that is elementwise N(0, c**2) (a plain module, not a U-Net): D(x, s) =
    c**2 / (c**2 + s**2) x, so F = (D - c_skip x) / c_out on x = r xs.  The probability-flow ODE dx/ds = (x - D) / s then has
    the exact solution x(s) = x(s_0) sqrt((c**2 + s**2) / (c**2 + s_0**2)): from s_0 noise to s = 0 it ends at
    s_0 c / sqrt(c**2 + s_0**2) noise."""

    def __init__(self, c: float, sd: float = SD):
        super().__init__()
        self.c, self.sd = c, sd

    def forward(self, xs, c_noise):
        s = torch.exp(4 * c_noise.double()).view(-1, *([1] * (xs.ndim - 1)))
        r2 = s * s + self.sd ** 2
        gain = (self.c ** 2 / (self.c ** 2 + s * s) - self.sd ** 2 / r2) * r2 / (s * self.sd)
        return (gain * xs.double()).float()

    def exact(self, noise, s0: float):
        return noise.double() * s0 * self.c / math.sqrt(self.c ** 2 + s0 ** 2)


# ------------------------------------------------------------------ 1. kernels against the restatement
ROWS = 2
PERS = [2048, 1001]
SIGMAS = torch.tensor([80.0, 0.5, 0.002, 0.0])    # three steps spanning the range; the last ends at the data (g = 1)
Q = 0.9


def _rows(order, eta):
    table = edm_table(SIGMAS, SD, order, eta)
    a0, b0, e0, f0, c1, d1, s1, cb = table.abs().unbind(1)
    gain = (c1 + cb) * (a0 + b0) + d1 * (e0 + f0) + cb + s1
    assert bool((gain <= STEP_GAIN).all()), gain          # the condition STEP_TOL was derived under (coefficients only)
    return table.to(torch.float32)                        # (the fp32 rows the kernel is given)


def _kernel_case(per, count):
    g = torch.Generator().manual_seed(per)
    return [torch.randn(ROWS, per, generator=g) for _ in range(count)]


def _rng(dev, d=3):
    return ops.rng_rows(SEED, [d])[0].to(dev)


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("variant", ["order1", "order2", "eta1"])
@pytest.mark.parametrize("mode", ["none", "static", "scale"])
@pytest.mark.parametrize("per", PERS)
def test_step_kernel_matches_restatement(dev, per, mode, variant, inplace):
    order, eta = (2 if variant == "order2" else 1), (1.0 if variant == "eta1" else 0.0)
    table = _rows(order, eta)
    assert table.shape == (3, 8) and bool((table[:, 6] == 0).all()) == (eta == 0.0)
    assert (table[1, 7] != 0) == (order == 2) and table[0, 7] == 0 and table[2, 7] == 0 and table[2, 4] == 1
    if eta:
        assert table[0, 6] > 0.1 and table[1, 6] > 1e-3 and table[2, 6] == 0   # two rows with noise, the last without
    xs, f, hist = _kernel_case(per, 3)
    assert 1001 % 4 != 0                  # at 1001 the second item starts inside a group of four
    for i, row in enumerate(table):
        dx, df, dh, drow, rng = xs.to(dev), f.to(dev), hist.to(dev), row.to(dev), _rng(dev, 1 + i)
        z = ops.randn(dx, rng).cpu()
        scale = None
        if mode == "scale":   # the restatement clamps with the scale the product's own select returned
            scale = ops.clip_scale(dx, Q, v=df, coef=drow, min_scale=1.0)
            assert scale.shape == (ROWS,) and bool((scale >= 1).all())
        want, want_h = edm_step_ref(xs, f, hist, row, z, clip=mode != "none", scale=None if scale is None else scale.cpu())
        kw = dict(scale=scale, clip=mode != "none", out=dx if inplace else None)
        if order == 1:
            out, got_h = ops.edm_step(dx, df, drow, rng, **kw), None
        else:
            out, got_h = ops.edm_step(dx, df, drow, rng, order=2, hist=dh, hist_out=dh if inplace else None, **kw)
            assert (got_h is dh) == inplace
        assert (out is dx) == inplace
        if not inplace:
            assert torch.equal(dx.cpu(), xs) and torch.equal(dh.cpu(), hist)
        assert torch.equal(df.cpu(), f) and torch.equal(drow.cpu(), row) and torch.equal(rng.cpu(), _rng("cpu", 1 + i))
        err = err_in(out, want, xs, f, hist, z)
        print(f"adp_edm_step per={per} {mode} {variant} row {i} inplace={inplace}: err {err:.3e} (bound {STEP_TOL:.2e})")
        assert out.shape == xs.shape and err <= STEP_TOL
        if got_h is not None:
            herr = err_in(got_h, want_h, xs, f, hist, z)
            print(f"  hist_out: err {herr:.3e}")
            assert herr <= STEP_TOL


@pytest.mark.parametrize("per", PERS)
def test_noise_kernel_matches_float64(dev, per):
    unit, n = _kernel_case(per, 2)
    for sd in (0.5, 1.0):
        x = sd * unit
        for sigma in (torch.tensor([0.002, 80.0]), torch.tensor([0.5, 0.002]), torch.tensor([80.0, 0.5])):
            s = sigma.double()[:, None]
            r = torch.sqrt(s * s + sd * sd)
            want_in = (x.double() + s * n.double()) / r
            want_t = (x.double() - (sd * sd / (r * r)) * (x.double() + s * n.double())) / (s * sd / r)
            x_in, target = ops.edm_noise(x.to(dev), n.to(dev), sigma.to(dev), sd)
            errs = (err_in(x_in, want_in, unit, n), err_in(target, want_t, unit, n))
            print(f"adp_edm_noise per={per} sd={sd} sigma={sigma.tolist()}: err x_in / target = {errs} (bound {NOISE_TOL:.2e})")
            assert x_in.shape == x.shape and all(e <= NOISE_TOL for e in errs)
            # what the net reads has unit variance for data of variance sd**2 (five standard deviations of a sample variance)
            assert abs(x_in.double().var().item() - 1) < 5 * math.sqrt(2 / (ROWS * per))


def test_noise_kernel_in_place(dev):
    x, n = _kernel_case(1001, 2)
    sigma = torch.tensor([0.7, 12.0]).to(dev)
    want = ops.edm_noise(x.to(dev), n.to(dev), sigma, SD)
    dx, dn = x.to(dev), n.to(dev)
    got = ops.edm_noise(dx, dn, sigma, SD, x_in_out=dx, target_out=dn)
    assert got[0] is dx and got[1] is dn and torch.equal(dx, want[0]) and torch.equal(dn, want[1])


@pytest.mark.parametrize("per", PERS)
def test_the_noise_is_randn_of_the_same_row(dev, per):
    zero = torch.zeros(ROWS, per, device=dev)
    only_noise = torch.tensor([0.3, 0.9, 0.5, 0.2, 1.0, 1.0, 1.0, 0.0], device=dev)   # xs = f = 0, s1 = 1
    rng = _rng(dev)
    want = ops.randn(zero, rng)
    assert torch.equal(ops.edm_step(zero, zero, only_noise, rng), want)
    assert not torch.equal(ops.edm_step(zero, zero, only_noise, _rng(dev, 4)), want)
    # noise asked for without a row: NaN, not a read through a null pointer
    assert torch.isnan(ops.edm_step(zero, zero, only_noise, None)).all()


def test_nan_stays_nan(dev):
    xs, f = _kernel_case(1001, 2)
    xs[1, 3] = float("nan")
    row = _rows(1, 0.0)[1]
    scale = torch.tensor([1.5, float("nan")])
    out = ops.edm_step(xs.to(dev), f.to(dev), row.to(dev), scale=scale.to(dev), clip=True).cpu()
    assert torch.isfinite(out[0]).all() and torch.isnan(out[1]).all()
    out = ops.edm_step(xs.to(dev), f.to(dev), row.to(dev), clip=True).cpu()
    assert torch.isnan(out[1, 3]) and int(torch.isnan(out).sum()) == 1


# ------------------------------------------------------------------ 2. bit equalities
@pytest.mark.parametrize("mode", ["none", "scale"])
@pytest.mark.parametrize("per", PERS)
def test_an_order_2_row_with_cb_zero_gives_the_bits_of_order_1(dev, per, mode):
    xs, f = _kernel_case(per, 2)
    row = _rows(2, 0.0)[1].clone()
    full = row.clone()
    row[7] = 0.0
    dx, df, drow = xs.to(dev), f.to(dev), row.to(dev)
    scale = ops.clip_scale(dx, Q, v=df, coef=drow, min_scale=1.0) if mode == "scale" else None
    nan = torch.full((ROWS, per), float("nan")).to(dev)
    first = ops.edm_step(dx, df, drow, scale=scale, clip=scale is not None)
    out, h = ops.edm_step(dx, df, drow, scale=scale, clip=scale is not None, order=2, hist=nan)
    assert torch.isfinite(out).all() and torch.isfinite(h).all() and torch.isnan(nan).all()
    assert torch.equal(out, first), "order 2 with cb = 0 must give the bits of order 1"
    # and with cb != 0 the history is read: the NaN arrives
    assert torch.isnan(ops.edm_step(dx, df, full.to(dev), order=2, hist=nan)[0]).all()


@pytest.mark.parametrize("per", PERS)
def test_a_row_without_noise_does_not_read_the_generator(dev, per):
    """s1 = 0: a NaN-filled generator row, or none at all, cannot reach xs."""
    xs, f = _kernel_case(per, 2)
    row = _rows(1, 0.0)[0]
    nan_row = torch.full((4,), 0x7FC00000, dtype=torch.int32)
    plain = ops.edm_step(xs.to(dev), f.to(dev), row.to(dev))
    assert torch.isfinite(plain).all()
    assert torch.equal(ops.edm_step(xs.to(dev), f.to(dev), row.to(dev), nan_row.to(dev)), plain)


class ViaWords(adp.KSampler):
    """An eta = 0 sampler whose rows take the int32 path of eta > 0 (coefficients next to a generator row)."""

    def _tables(self, num_steps, b, device):
        c_noise, coef = super()._tables(num_steps, b, device)
        assert coef.dtype == torch.float32 and coef.shape == (num_steps, 8)
        words = torch.cat([coef.cpu().view(torch.int32), ops.rng_rows(SEED, range(1, 1 + num_steps))], dim=1)
        return c_noise, words.contiguous().to(device)


def _noise(dev, seed=1, shape=(2, 2, 256)):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def test_eta_zero_through_the_word_table_gives_the_bits_of_the_float_table(dev):
    net, x = GaussianF(1.5), _noise(dev, shape=(2, 2, 1001))
    schedule = adp.KarrasSchedule(0.002, 80.0)
    for order in (1, 2):
        plain = adp.KSampler(net, schedule, order=order, use_graph=False)(x, num_steps=5)
        assert torch.equal(ViaWords(net, schedule, order=order, use_graph=False)(x, num_steps=5), plain)


# ------------------------------------------------------------------ 3. cross-check against the v-objective
class TanSchedule(adp.Schedule):
    """sigma = tan(pi t / 2) for LinearSchedule(0.95, 0)'s t: the noise levels at which the v-objective's path
    cos(phi) x + sin(phi) n is c_in (x + sigma n) for sigma_data = 1."""

    def forward(self, num_steps, device):
        t = torch.linspace(0.95, 0.0, num_steps).double()
        return torch.tan(t * (math.pi / 2)).to(torch.float32).to(device)


class MinusV(nn.Module):
    """-v(xs, t) of a v-objective net, read as an EDM net: t = atan(sigma) 2 / pi, sigma = exp(4 c_noise)."""

    def __init__(self, v):
        super().__init__()
        self.v = v

    def forward(self, xs, c_noise):
        t = torch.atan(torch.exp(4 * c_noise.double())) * (2 / math.pi)
        return -self.v(xs, t.float())


@pytest.mark.parametrize("per", PERS)
def test_noising_is_the_v_objectives_for_unit_sigma_data(dev, per):
    x, n = _kernel_case(per, 2)
    t = torch.tensor([0.3, 0.8])
    sigma = torch.tan(t.double() * (math.pi / 2)).to(torch.float32)
    x_noisy, v_target = ops.v_noise(x.to(dev), n.to(dev), t.to(dev))
    x_in, target = ops.edm_noise(x.to(dev), n.to(dev), sigma.to(dev), 1.0)
    errs = (rel_err(x_in, x_noisy), rel_err(target, -v_target))
    print(f"edm_noise against v_noise per={per}: rel_err x_in / target = {errs} (bound {LOOP_TOL:.0e})")
    assert all(e <= LOOP_TOL for e in errs)


def test_first_order_sampler_is_vsampler_for_unit_sigma_data(dev):
    v = GaussianV(1.5)
    noise = _noise(dev, shape=(2, 2, 1001))
    k = adp.KSampler(MinusV(v), TanSchedule(), sigma_data=1.0, order=1, eta=0.0)
    got = k(noise, num_steps=8)
    phi0 = 0.95 * math.pi / 2
    start = (math.sin(phi0) * noise.double()).float()       # c_in(sigma_0) sigma_0 noise: the v-path's state at t = 0.95
    want = adp.VSampler(v, adp.LinearSchedule(0.95, 0.0))(start, num_steps=8)
    err = rel_err(got, want)
    print(f"KSampler(order=1, sigma_data=1) against VSampler: rel_err {err:.3e} (bound {LOOP_TOL:.0e})")
    assert got.shape == noise.shape and err <= LOOP_TOL


# ------------------------------------------------------------------ 4. the table, the schedule, the distribution
def test_table_matches_restatement(emul):
    sigmas = adp.KarrasSchedule(0.002, 80.0)(41, "cpu")
    for order, eta in ((1, 0.0), (2, 0.0), (1, 1.0), (1, 0.4)):
        coef = ops.edm_table(sigmas, SD, order, eta)
        assert coef.shape == (40, 8) and coef.dtype == torch.float32 and coef.device.type == "cpu"
        # both are float64 values rounded to float32 once: at most one float32 ulp apart
        assert torch.allclose(coef, edm_table(sigmas, SD, order, eta).to(torch.float32), rtol=2 ** -23, atol=1e-30)
        assert coef[-1, 4] == 1 and coef[-1, 5] == 0 and coef[-1, 6] == 0 and coef[-1, 7] == 0   # the last step returns x0c
        assert coef[0, 7] == 0 and bool((coef[1:-1, 7] != 0).all()) == (order == 2)
        assert bool((coef[:-1, 6] > 0).all()) == (eta > 0) and bool((coef[:, 1] < 0).all()) and bool((coef[:, 3] < 0).all())
    # through the sampler: c_noise is ln(sigma) / 4 with a last row of 0, and eta > 0 appends the generator rows
    net = GaussianF(1.5)
    s = adp.KSampler(net, adp.KarrasSchedule(0.002, 80.0))
    c_noise, table = s._tables(40, 3, "cpu")
    assert c_noise.shape == (41, 3) and torch.equal(c_noise[:-1, 0], torch.log(sigmas[:-1]) * 0.25)
    assert bool((c_noise[-1] == 0).all()) and torch.equal(table, ops.edm_table(sigmas, SD, 2, 0.0))
    s = adp.KSampler(net, adp.KarrasSchedule(0.002, 80.0), order=1, eta=0.4)
    s._seed = SEED
    _, words = s._tables(40, 3, "cpu")
    assert words.shape == (40, 12) and words.dtype == torch.int32
    assert torch.equal(words[:, :8].contiguous().view(torch.float32), ops.edm_table(sigmas, SD, 1, 0.4))
    assert torch.equal(words[:, 8:], ops.rng_rows(SEED, range(1, 41)))
    assert s._step_key() == (1, True, None) and adp.KSampler(net, s.schedule, dynamic_threshold=0.9)._step_key() == (2, False, 0.9)


def test_karras_schedule():
    sched = adp.KarrasSchedule(0.002, 80.0)
    assert sched.rho == 7.0
    s = sched(11, "cpu")
    assert s.shape == (11,) and s.dtype == torch.float32 and s[-1] == 0
    assert s[0] == 80.0 and abs(s[-2].item() / 0.002 - 1) < 1e-6 and bool((s[1:] < s[:-1]).all())
    i = torch.arange(10, dtype=torch.float64) / 9
    want = (80.0 ** (1 / 7) + i * (0.002 ** (1 / 7) - 80.0 ** (1 / 7))) ** 7
    assert torch.allclose(s[:-1].double(), want, rtol=2 ** -23, atol=0)
    assert sched(2, "cpu").tolist() == [80.0, 0.0] and sched(1, "cpu").tolist() == [0.0]
    lin = adp.KarrasSchedule(1.0, 3.0, rho=1.0)(4, "cpu")
    assert torch.allclose(lin, torch.tensor([3.0, 2.0, 1.0, 0.0]), rtol=1e-6, atol=0)


@pytest.mark.parametrize("mean,std", [(-1.2, 1.2), (0.3, 0.5)])
def test_log_normal_distribution(mean, std):
    dist = adp.LogNormalDistribution(mean, std)
    s = dist(2 ** 16, device=torch.device("cpu"), generator=torch.Generator().manual_seed(5))
    assert s.shape == (2 ** 16,) and s.dtype == torch.float32 and bool((s > 0).all())
    log = torch.log(s.double())
    print(f"log-normal({mean}, {std}): log mean {log.mean().item():.4f}, std {log.std().item():.4f}")
    # 65536 draws: the mean of the logs has standard deviation std / 256, their std a relative one of 1 / 362: five of each
    assert abs(log.mean().item() - mean) <= 5 * std / 256 and abs(log.std().item() / std - 1) <= 5 / 362
    assert dist.graph_key() == ("log-normal", float(mean), float(std))
    assert adp.LogNormalDistribution().graph_key() == ("log-normal", -1.2, 1.2)
    torch.manual_seed(9)
    a = dist(8)
    torch.manual_seed(9)
    assert torch.equal(a, dist(8)) and not torch.equal(a, dist(8))


# ------------------------------------------------------------------ 5. order on a problem with a known answer
ORDER_N = (10, 20, 40)


def _assert_second_order_wins(e1, e2, what):
    ratios = [e1[n] / e2[n] for n in ORDER_N]
    print(f"{what}: order 1 {e1}; order 2 {e2}; ratios {ratios}")
    for n in ORDER_N:
        assert e2[n] < e1[n], (what, n, e2[n], e1[n])
    assert ratios[0] < ratios[1] < ratios[2], (what, ratios)


@pytest.mark.parametrize("c", [0.25, 1.5])
def test_restatement_second_order_beats_first(c):
    """The float64 loop of this file (the yardstick is itself the method)."""
    net, noise = GaussianF(c), _noise("cpu", seed=3, shape=(4, 2, 64))
    e1, e2 = {}, {}
    for n in ORDER_N:
        sigmas = adp.KarrasSchedule(0.002, 80.0)(n + 1, "cpu")
        exact = net.exact(noise, float(sigmas[0]))
        e1[n] = rel_err(edm_sample_ref(net, noise, sigmas, order=1), exact)
        e2[n] = rel_err(edm_sample_ref(net, noise, sigmas, order=2), exact)
    _assert_second_order_wins(e1, e2, f"float64 loop, c={c}")


@pytest.mark.parametrize("c", [0.25, 1.5])
def test_sampler_second_order_beats_first(dev, c):
    net, noise = GaussianF(c), _noise(dev, seed=3, shape=(4, 2, 64))
    schedule = adp.KarrasSchedule(0.002, 80.0)
    first, second = adp.KSampler(net, schedule, order=1), adp.KSampler(net, schedule, order=2)
    exact = net.exact(noise, 80.0)
    e1 = {n: rel_err(first(noise, num_steps=n), exact) for n in ORDER_N}
    e2 = {n: rel_err(second(noise, num_steps=n), exact) for n in ORDER_N}
    _assert_second_order_wins(e1, e2, f"KSampler, c={c}")
    # and the product is the restatement's method
    sigmas = schedule(21, "cpu")
    assert rel_err(second(noise, num_steps=20), edm_sample_ref(net, noise, sigmas)) <= LOOP_TOL


# ------------------------------------------------------------------ 6. sampler against the restatement through a U-Net
SHAPE, STEPS = (2, 2, 256), 6
SCHEDULE = adp.KarrasSchedule(0.002, 80.0)


def tiny_pair(dev, gain=1.0, seed=0):
    """(oracle, the product net with its weights); `gain` scales the output convolution, as tests/test_threshold_sampler.py
    does: a freshly initialised TINY net is close to the identity, and x0 = a0 xs - b0 F then rarely leaves [-1, 1]."""
    torch.manual_seed(seed)
    oracle = UNetV0Oracle(**TINY)
    with torch.no_grad():
        oracle.blocks[0].up.weight.mul_(gain)
        oracle.blocks[0].up.bias.mul_(gain)
    net = adp.UNetV0(dim=1, **TINY)
    net.load_oracle_state_dict(oracle.state_dict())
    return oracle, net.to(dev).eval()


class Counting(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net, self.calls = net, 0

    def forward(self, x, time, **kw):
        self.calls += 1
        return self.net(x, time, **kw)


# (orders 1 and 2, eta = 1, the static and the dynamic threshold: an emulated forward takes seconds, so four cases carry them)
CASES = [(1, 0.0, None), (2, 0.0, None), (1, 1.0, 0.0), (2, 0.0, 0.9)]
_OUTS = {}


@pytest.mark.parametrize("order,eta,q", CASES, ids=[f"order{o}-eta{e:g}-q{q}" for o, e, q in CASES])
def test_sampler_matches_restatement_through_a_unet(dev, order, eta, q):
    _, net = tiny_pair(dev, gain=1.0 if q is None else OUT_GAIN)
    x = _noise(dev, shape=SHAPE)
    counting = Counting(net)
    sampler = adp.KSampler(counting, SCHEDULE, order=order, eta=eta, dynamic_threshold=q, use_graph=False)
    kept = x.clone()
    out = sampler(x, num_steps=STEPS, seed=SEED)
    assert counting.calls == STEPS, "one net evaluation per step"
    assert torch.equal(x, kept)
    stats = []
    want = edm_sample_ref(net, x, SCHEDULE(STEPS + 1, "cpu"), order=order, eta=eta, seed=SEED, q=q, stats=stats)
    if q:   # the condition under which the thresholded case says anything: the clamp bites
        assert any(s > 1 for scale, _ in stats for s in scale.tolist()), stats
    elif q is not None:
        assert any(m > 1 for _, m in stats), stats
    err = rel_err(out, want)
    print(f"KSampler order={order} eta={eta} q={q}: rel_err vs float64 loop {err:.3e} (bound {LOOP_TOL:.0e})")
    assert out.shape == x.shape and err <= LOOP_TOL
    # the other cases of this threshold are other trajectories (the comparison is between the cases' kept results)
    for (d, o, e, qq), other in _OUTS.items():
        if d == dev.type and qq == q and (o, e) != (order, eta):
            assert rel_err(out, other) > 1e-3
    _OUTS[(dev.type, order, eta, q)] = out.cpu()


def test_start_shifts_the_run(dev):
    """start + sigma_0 noise: with a start the restatement's run begins there, and the result differs."""
    net = GaussianF(1.5)
    noise, start = _noise(dev, seed=2, shape=(2, 2, 64)), 0.5 * _noise(dev, seed=3, shape=(2, 2, 64))
    sampler = adp.KSampler(net, adp.KarrasSchedule(0.01, 1.0), use_graph=False)
    got = sampler(noise, num_steps=5, start=start)
    want = edm_sample_ref(net, noise, sampler.schedule(6, "cpu"), start=start)
    assert rel_err(got, want) <= LOOP_TOL and rel_err(got, sampler(noise, num_steps=5)) > 1e-2


def test_seed_governs_the_run(dev):
    net, x = GaussianF(1.5), _noise(dev, shape=(2, 2, 64))
    s = adp.KSampler(net, SCHEDULE, order=1, eta=1.0, use_graph=False)
    a = s(x, num_steps=3, seed=7)
    assert torch.equal(a, s(x, num_steps=3, seed=7)) and not torch.equal(a, s(x, num_steps=3, seed=8))
    torch.manual_seed(123)
    d1, d2 = s(x, num_steps=3), s(x, num_steps=3)
    torch.manual_seed(123)
    assert torch.equal(d1, s(x, num_steps=3)) and not torch.equal(d1, d2) and s._seed == 0
    # eta = 0 draws nothing: torch's generator is left alone
    state = torch.get_rng_state()
    adp.KSampler(net, SCHEDULE, use_graph=False)(x, num_steps=3)
    assert torch.equal(torch.get_rng_state(), state)


# ------------------------------------------------------------------ 7. replay
@pytest.mark.gpu
@pytest.mark.parametrize("order,eta,q", [(2, 0.0, None), (2, 0.0, 0.9), (1, 1.0, 0.9)], ids=["order2", "order2-q0.9", "eta1-q0.9"])
def test_replayed_sampling_equals_eager(hip, order, eta, q):
    _, net = tiny_pair(hip, gain=1.0 if q is None else OUT_GAIN)
    x = _noise(hip, shape=SHAPE)
    g = adp.KSampler(net, SCHEDULE, order=order, eta=eta, dynamic_threshold=q)
    e = adp.KSampler(net, SCHEDULE, order=order, eta=eta, dynamic_threshold=q, use_graph=False)
    out4, out9 = g(x, num_steps=4, seed=7), g(x, num_steps=9, seed=7)
    assert g.graph_captures == 1 and g.graph_replays == 2 and len(g._graph_cache) == 1 and e.graph_captures == 0
    assert torch.equal(out4, e(x, num_steps=4, seed=7)) and torch.equal(out9, e(x, num_steps=9, seed=7))
    assert not torch.equal(out4, out9)
    assert torch.equal(g(x, num_steps=4, seed=7), out4), "the previous run's history leaked into this one"
    if eta:
        other = g(x, num_steps=4, seed=8)
        assert torch.equal(other, e(x, num_steps=4, seed=8)) and not torch.equal(other, out4)
    entry = next(iter(g._graph_cache.values()))
    assert len(entry.bufs) == (2 if q else 0) + (1 if order == 2 else 0)
    assert entry.sab.shape == ((12,) if eta else (8,)) and entry.sab.dtype == (torch.int32 if eta else torch.float32)
    # a run from NaN leaves NaN in the entry's buffers; the next run must not see it
    assert torch.isnan(g(torch.full_like(x, float("nan")), num_steps=3, seed=7)).all()
    assert torch.equal(g(x, num_steps=9, seed=7), out9) and g.graph_captures == 1
    # order, eta > 0 and the clip mode are other steps
    g.order = e.order = 1
    g.eta = e.eta = 0.0
    first = g(x, num_steps=4)
    captures = g.graph_captures
    assert torch.equal(first, e(x, num_steps=4)) and captures == 2 and not torch.equal(first, out4)
    g.dynamic_threshold = e.dynamic_threshold = 0.0
    assert torch.equal(g(x, num_steps=4), e(x, num_steps=4)) and g.graph_captures == 3
    # a deep copy (an EMA copy) leaves the captured steps behind and captures its own
    g.order, g.eta, g.dynamic_threshold = order, eta, q
    cp = copy.deepcopy(g)
    assert len(cp._graph_cache) == 0 and cp.graph_captures == 0 and cp.order == order and cp.dynamic_threshold == q
    assert torch.equal(cp(x, num_steps=4, seed=7), out4) and cp.graph_captures == 1 and g.graph_captures == 3


# ------------------------------------------------------------------ 8. training step
def _train_pair(dev, loss_fn=F.mse_loss, dist=None, **extra):
    torch.manual_seed(0)
    model = adp.DiffusionModel(net_t=adp.UNetV0, diffusion_t=adp.KDiffusion, sampler_t=adp.KSampler, loss_fn=loss_fn,
                               diffusion_sigma_distribution=dist or FixedSigmas([0.3, 2.5]), sampler_schedule=SCHEDULE,
                               **extra, **TINY)
    oracle = UNetV0Oracle(**TINY)
    model.net.load_oracle_state_dict(oracle.state_dict())
    return oracle, model.to(dev)


def test_kdiffusion_loss_and_grads(dev):
    oracle, model = _train_pair(dev)
    assert type(model.diffusion) is adp.KDiffusion and type(model.sampler) is adp.KSampler
    assert model.diffusion.sigma_data == 0.5 and model.sampler.sigma_data == 0.5 and model.sampler.schedule is SCHEDULE
    g = torch.Generator().manual_seed(3)
    x, noise = SD * torch.randn(2, 2, 256, generator=g), torch.randn(2, 2, 256, generator=g)
    sigma = torch.tensor([0.3, 2.5])
    loss_ref = edm_loss_ref(oracle, x, noise, sigma)
    loss_ref.backward()
    loss = model(x.to(dev), noise=noise.to(dev))
    loss.backward()
    print(f"KDiffusion loss {loss.item():.6f} against {loss_ref.item():.6f}")
    assert abs(loss.item() - loss_ref.item()) < UNET_TOL * abs(loss_ref.item())
    compare_grads(model.net, oracle)
    # it is not the v-objective under another name
    v_ref = ovd.v_loss(oracle, x, noise, torch.tensor([0.3, 0.7]))
    assert abs(v_ref.item() - loss_ref.item()) > 1e-2 * abs(loss_ref.item())
    # sigma_data reaches the kernel
    oracle2, model2 = _train_pair(dev, diffusion_sigma_data=1.0)
    l2 = model2(x.to(dev), noise=noise.to(dev))
    l2_ref = edm_loss_ref(oracle2, x, noise, sigma, sd=1.0)
    assert abs(l2.item() - l2_ref.item()) < UNET_TOL * abs(l2_ref.item())
    assert abs(l2.item() - loss.item()) > 1e-2 * abs(loss.item())
    # a user loss_fn runs (autograd) and differs
    oracle1, model1 = _train_pair(dev, loss_fn=F.l1_loss)
    l1 = model1(x.to(dev), noise=noise.to(dev))
    l1.backward()
    l1_ref = edm_loss_ref(oracle1, x, noise, sigma, loss_fn=F.l1_loss)
    assert abs(l1.item() - l1_ref.item()) < UNET_TOL * abs(l1_ref.item())
    assert abs(l1.item() - loss.item()) > 1e-2 * abs(loss.item())
    assert all(p.grad is not None for p in model1.net.parameters())


def test_denoise_is_the_preconditioned_net(dev):
    oracle, model = _train_pair(dev)
    g = torch.Generator().manual_seed(4)
    x, sigma = torch.randn(2, 2, 256, generator=g) * 3, torch.tensor([0.3, 2.5])
    s = sigma.double()[:, None, None]
    r = torch.sqrt(s * s + SD * SD)
    with torch.no_grad():
        out = oracle((x.double() / r).float(), torch.log(sigma) * 0.25).double()
        got = model.diffusion.denoise(x.to(dev), sigma.to(dev))
    want = (SD * SD / (r * r)) * x.double() + (s * SD / r) * out
    assert got.shape == x.shape and rel_err(got, want) <= UNET_TOL


def _zero(m):
    for p in m.parameters():
        p.grad = None


def _three_steps(m, xs, seed=123, noise=None):
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    losses, grads = [], []
    for x in xs:
        _zero(m)
        loss = m(x) if noise is None else m(x, noise=noise)
        loss.backward()
        losses.append(loss.clone())
        grads.append([p.grad.clone() for p in m.parameters()])
    return losses, grads


class DeviceSigmas(adp.Distribution):
    """Fixed sigmas that already live on the device (a view of one tensor: nothing is copied under capture)."""

    def __init__(self, vals):
        self.vals = vals

    def __call__(self, num_samples, device=None):
        return self.vals[:num_samples]

    def graph_key(self):
        return ("device-sigmas",)


class KFixed(adp.KDiffusion):
    GRAPH_DISTRIBUTIONS = (DeviceSigmas,)


def _model(dev, diffusion_t, dist, **extra):
    torch.manual_seed(0)
    kw = {} if dist is None else dict(diffusion_sigma_distribution=dist)
    return adp.DiffusionModel(net_t=adp.UNetV0, diffusion_t=diffusion_t, **kw, **extra, **TINY).to(dev)


def _assert_same_steps(a, b):
    (la, ga), (lb, gb) = a, b
    for i in range(len(la)):
        assert torch.equal(la[i], lb[i]), (i, la, lb)
        assert all(torch.equal(p, q) for p, q in zip(ga[i], gb[i]))


@pytest.mark.gpu
def test_replayed_training_step_equals_eager(hip):
    make = lambda: adp.LogNormalDistribution(-0.4, 0.8)
    m_g, m_e = _model(hip, adp.KDiffusion, make()), _model(hip, adp.KDiffusion, make(), diffusion_use_graph=False)
    xs = [SD * torch.randn(2, 2, 1024, device=hip) for _ in range(3)]
    run_g, run_e = _three_steps(m_g, xs), _three_steps(m_e, xs)
    g = graphed.GRAPHS_OF[m_g.diffusion]
    assert g.captures == 1 and g.replays == 3 and graphed.GRAPHS_OF.get(m_e.diffusion) is None
    _assert_same_steps(run_g, run_e)
    assert len({round(v.item(), 9) for v in run_g[0]}) == 3, "every replay must draw fresh sigmas / noise"
    again, _ = _three_steps(m_g, xs)
    assert all(torch.equal(a, b) for a, b in zip(again, run_g[0])) and g.captures == 1 and g.replays == 6
    assert next(iter(g.cache))[-3:] == ("log-normal", -0.4, 0.8)
    # a deep copy (an EMA copy) after the capture: it works, leaves the graphs behind and captures its own
    cp = copy.deepcopy(m_g)
    assert graphed.GRAPHS_OF.get(cp.diffusion) is None and cp.diffusion.sigma_data == 0.5
    _assert_same_steps(_three_steps(cp, xs), run_e)
    assert graphed.GRAPHS_OF[cp.diffusion].captures == 1 and g.captures == 1


@pytest.mark.gpu
def test_replayed_step_under_injected_noise_and_fixed_sigmas(hip):
    """Nothing is drawn: the replayed and the eager step see the same numbers, and must give the same bits."""
    sig = torch.tensor([0.3, 2.5], device=hip)
    m_g, m_e = _model(hip, KFixed, DeviceSigmas(sig)), _model(hip, adp.KDiffusion, FixedSigmas([0.3, 2.5]))
    xs = [SD * torch.randn(2, 2, 1024, device=hip) for _ in range(3)]
    noise = torch.randn(2, 2, 1024, device=hip)
    run_g, run_e = _three_steps(m_g, xs, noise=noise), _three_steps(m_e, xs, noise=noise)
    g = graphed.GRAPHS_OF[m_g.diffusion]
    assert g.captures == 1 and g.replays == 3 and graphed.GRAPHS_OF.get(m_e.diffusion) is None
    _assert_same_steps(run_g, run_e)
    # the graph reads the sigma row at every replay
    sig.copy_(torch.tensor([1.0, 0.1], device=hip))
    m_e.diffusion.sigma_distribution = FixedSigmas([1.0, 0.1])
    moved_g, moved_e = _three_steps(m_g, xs[:1], noise=noise), _three_steps(m_e, xs[:1], noise=noise)
    _assert_same_steps(moved_g, moved_e)
    assert not torch.equal(moved_g[0][0], run_g[0][0]) and g.captures == 1


@pytest.mark.gpu
def test_other_distributions_run_eagerly(hip):
    """A distribution class that KDiffusion does not list is not captured: the eager step runs."""
    x = SD * torch.randn(2, 2, 1024, device=hip)
    for dist in (FixedSigmas([0.3, 2.5]), adp.UniformDistribution(0.1, 2.0), adp.LogitNormalDistribution()):
        m = _model(hip, adp.KDiffusion, dist)
        m(x).backward()
        assert graphed.GRAPHS_OF.get(m.diffusion) is None, type(dist)
    m = _model(hip, adp.KDiffusion, None)
    assert type(m.diffusion.sigma_distribution) is adp.LogNormalDistribution
    m(x).backward()
    assert graphed.GRAPHS_OF[m.diffusion].captures == 1
    # and the v-objective does not take the log-normal draw
    other = _model(hip, adp.VDiffusion, adp.LogNormalDistribution())
    other(x).backward()
    assert graphed.GRAPHS_OF.get(other.diffusion) is None


# ------------------------------------------------------------------ 9. wrappers
def _on_cpu(oracle):
    """The oracle net (CPU, float32) as a net of `edm_sample_ref` whose state lives on the GPU."""
    def net(x, t, **kw):
        return oracle(x.cpu(), t.cpu(), **kw).to(x.device)
    return net


@pytest.mark.gpu
def test_diffusion_model_with_sampler_t(hip):
    oracle, model = _train_pair(hip, dist=adp.LogNormalDistribution(), diffusion_sigma_data=0.4, sampler_sigma_data=0.4,
                                sampler_order=2)
    assert model.sampler.order == 2 and model.sampler.sigma_data == 0.4 and model.diffusion.sigma_data == 0.4
    noise = torch.randn(2, 2, 1024, generator=torch.Generator().manual_seed(4)).to(hip)
    out = model.sample(noise, num_steps=5)
    assert model.sampler.graph_captures == 1
    assert rel_err(out, edm_sample_ref(_on_cpu(oracle), noise, SCHEDULE(6, "cpu"), sd=0.4)) <= PARITY_TOL
    _, first = _train_pair(hip, sampler_order=1, sampler_eta=1.0)
    ref = edm_sample_ref(_on_cpu(oracle), noise, SCHEDULE(6, "cpu"), order=1, eta=1.0, seed=SEED)
    assert rel_err(first.sample(noise, num_steps=5, seed=SEED), ref) <= PARITY_TOL


@pytest.mark.gpu
def test_upsampler_sample(hip):
    torch.manual_seed(0)
    cfg = dict(TINY)
    cfg.pop("in_channels")
    up = adp.DiffusionUpsampler(net_t=adp.UNetV0, in_channels=2, upsample_factor=4, diffusion_t=adp.KDiffusion,
                                sampler_t=adp.KSampler, sampler_schedule=SCHEDULE, sampler_dynamic_threshold=0.9, **cfg)
    oracle = AppendChannelsOracle(lambda **kw: UNetV0Oracle(**kw), channels=2)(in_channels=2, **cfg)
    up.net.net.load_oracle_state_dict(oracle.net.state_dict())
    up = up.to(hip)
    low = torch.randn(2, 2, 256, generator=torch.Generator().manual_seed(9))
    cond = ovd.upsample(low, 4)
    torch.manual_seed(77)
    out = up.sample(low.to(hip), num_steps=5)
    torch.manual_seed(77)
    start = torch.randn(cond.shape).to(hip)
    ref = edm_sample_ref(_on_cpu(oracle), start, SCHEDULE(6, "cpu"), q=0.9, append_channels=cond)
    assert out.shape == (2, 2, 1024) and rel_err(out, ref) <= PARITY_TOL


@pytest.mark.gpu
def test_autoencoder_decode(hip):
    class Enc(adp.EncoderBase):
        def __init__(self):
            super().__init__()
            self.out_channels, self.downsample_factor = 3, 4
            self.conv = torch.nn.Conv1d(2, 3, kernel_size=4, stride=4)

        def forward(self, x, with_info=False):
            z = torch.tanh(self.conv(x))
            return (z, {"z": z}) if with_info else z

    torch.manual_seed(0)
    cfg = dict(channels=[8, 16], factors=[2, 2], items=[1, 1], modulation_features=32)
    ae = adp.DiffusionAE(net_t=adp.UNetV0, in_channels=2, encoder=Enc(), inject_depth=1, diffusion_t=adp.KDiffusion,
                         sampler_t=adp.KSampler, sampler_schedule=SCHEDULE, **cfg)
    oracle = UNetV0Oracle(in_channels=2, context_channels=[0, 3], **cfg)
    ae.net.load_oracle_state_dict(oracle.state_dict())
    ae = ae.to(hip)
    z = torch.tanh(torch.randn(2, 3, 256, generator=torch.Generator().manual_seed(6)))
    out = ae.decode(z.to(hip), num_steps=5, generator=torch.Generator(device=hip).manual_seed(5))
    start = torch.randn((2, 2, 1024), device=hip, dtype=z.dtype, generator=torch.Generator(device=hip).manual_seed(5))
    ref = edm_sample_ref(_on_cpu(oracle), start, SCHEDULE(6, "cpu"), channels=[None, z])
    assert out.shape == (2, 2, 1024) and rel_err(out, ref) <= PARITY_TOL
    # and it trains: the encoder's latent reaches the preconditioned net
    loss = ae(SD * torch.randn(2, 2, 1024, device=hip))
    loss.backward()
    assert torch.isfinite(loss) and all(p.grad is not None for p in ae.encoder.parameters())


# ------------------------------------------------------------------ 10. bad arguments
def test_wrappers_reject_bad_arguments(emul):
    x, row, sig, rng = torch.zeros(2, 8), torch.zeros(8), torch.ones(2), _rng("cpu")
    for call in (lambda: ops.edm_noise(x, torch.zeros(2, 7), sig),
                 lambda: ops.edm_noise(x, x, torch.ones(3)),
                 lambda: ops.edm_noise(x, x, sig.double()),
                 lambda: ops.edm_noise(x, x, sig, 0.0),
                 lambda: ops.edm_noise(x, x, sig, -1.0),
                 lambda: ops.edm_noise(x, x, sig, float("nan")),
                 lambda: ops.edm_noise(x, x, sig, x_in_out=torch.zeros(16)),
                 lambda: ops.edm_noise(torch.zeros(()), torch.zeros(()), sig),
                 lambda: ops.edm_step(x, torch.zeros(2, 7), row),
                 lambda: ops.edm_step(x, x, torch.zeros(6)),
                 lambda: ops.edm_step(x, x, row.double()),
                 lambda: ops.edm_step(x, x, row, rng.float()),
                 lambda: ops.edm_step(x, x, row, rng[:3]),
                 lambda: ops.edm_step(x, x, row, scale=torch.ones(2)),               # a scale without clip
                 lambda: ops.edm_step(x, x, row, scale=torch.ones(3), clip=True),
                 lambda: ops.edm_step(x, x, row, clip=1),
                 lambda: ops.edm_step(x, x, row, order=3),
                 lambda: ops.edm_step(x, x, row, order=2),                           # no history
                 lambda: ops.edm_step(x, x, row, order=1, hist=x),
                 lambda: ops.edm_step(x, x, row, out=torch.zeros(16)),
                 lambda: ops.edm_table(torch.tensor([1.0, 0.5, 0.5, 0.0])),          # not strictly decreasing
                 lambda: ops.edm_table(torch.tensor([1.0, 0.5, 0.7, 0.0])),
                 lambda: ops.edm_table(torch.tensor([1.0, 0.0, 0.0])),               # a non-final sigma <= 0
                 lambda: ops.edm_table(torch.tensor([1.0, 0.5, -0.1])),              # a final sigma < 0
                 lambda: ops.edm_table(torch.tensor([1.0, 0.0]), sigma_data=0.0),
                 lambda: ops.edm_table(torch.tensor([1.0, 0.0]), order=3),
                 lambda: ops.edm_table(torch.tensor([1.0, 0.0]), order=1, eta=1.5),
                 lambda: ops.edm_table(torch.tensor([1.0, 0.0]), order=2, eta=0.5)):
        with pytest.raises(ValueError):
            call()
    assert torch.equal(x, torch.zeros(2, 8))
    assert ops.edm_table(torch.tensor([1.0, 0.5, 0.0])).shape == (2, 8)     # a final sigma of 0 is the usual end
    assert ops.edm_table(torch.tensor([1.0, 0.5, 0.1])).shape == (2, 8)     # ... and a positive one is allowed


def test_bad_arguments_raise(emul):
    net = GaussianF(1.5)
    for bad in (0, 3, "2", None, True, 1.5):
        with pytest.raises(ValueError, match="order"):
            adp.KSampler(net, SCHEDULE, order=bad)
    for bad in (-0.1, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="eta"):
            adp.KSampler(net, SCHEDULE, order=1, eta=bad)
    with pytest.raises(ValueError, match="eta"):
        adp.KSampler(net, SCHEDULE, order=2, eta=0.5)
    for bad in (-0.1, 1.5, float("nan"), "0.9", True):
        with pytest.raises(ValueError, match="dynamic_threshold"):
            adp.KSampler(net, SCHEDULE, dynamic_threshold=bad)
    for bad in (0.0, -0.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="sigma_data"):
            adp.KSampler(net, SCHEDULE, sigma_data=bad)
        with pytest.raises(ValueError, match="sigma_data"):
            adp.KDiffusion(net, sigma_data=bad)
    s = adp.KSampler(net, SCHEDULE)
    assert s.order == 2 and s.eta == 0.0 and s.sigma_data == 0.5 and s.dynamic_threshold is None and s.use_graph
    d = adp.KDiffusion(net)
    assert d.sigma_data == 0.5 and type(d.sigma_distribution) is adp.LogNormalDistribution and d.loss_fn is F.mse_loss
    assert d.use_graph and adp.KDiffusion.GRAPH_DISTRIBUTIONS == (adp.LogNormalDistribution,)
    assert adp.KSampler.diffusion_types == [adp.KDiffusion]
    for name in ("KDiffusion", "KSampler", "KarrasSchedule", "LogNormalDistribution"):
        assert name in adp.__all__ and hasattr(adp, name)
    assert issubclass(adp.KSampler, adp.VSampler) and issubclass(adp.KDiffusion, adp.VDiffusion)
    assert issubclass(adp.KarrasSchedule, adp.Schedule) and issubclass(adp.LogNormalDistribution, adp.Distribution)
    with pytest.raises(ValueError, match="start"):
        s(torch.randn(1, 2, 8), num_steps=2, start=torch.randn(1, 2, 9))
    assert s._seed == 0

    class Repeats(adp.Schedule):
        def forward(self, num_steps, device):
            t = torch.linspace(1.0, 0.0, num_steps, device=device)
            t[2] = t[1]
            return t

    with pytest.raises(ValueError, match="schedule"):
        adp.KSampler(net, Repeats(), use_graph=False)(torch.randn(1, 2, 8), num_steps=5)
    with pytest.raises(ValueError, match="schedule"):   # LinearSchedule(1, 0) under order 1 is fine; rising is not
        adp.KSampler(net, adp.LinearSchedule(0.0, 1.0), order=1, use_graph=False)(torch.randn(1, 2, 8), num_steps=5)
    adp.KSampler(net, adp.LinearSchedule(), order=1, use_graph=False)(torch.randn(1, 2, 8), num_steps=5)
    for bad in (0.0, -1.0, "1", True, float("nan")):
        with pytest.raises(ValueError, match="std"):
            adp.LogNormalDistribution(std=bad)
    with pytest.raises(ValueError, match="mean"):
        adp.LogNormalDistribution(mean="0")
    for kw in (dict(sigma_min=0.0, sigma_max=1.0), dict(sigma_min=-1.0, sigma_max=1.0), dict(sigma_min=1.0, sigma_max=1.0),
               dict(sigma_min=1.0, sigma_max=0.5), dict(sigma_min=0.1, sigma_max=1.0, rho=0.0),
               dict(sigma_min="0.1", sigma_max=1.0), dict(sigma_min=0.1, sigma_max=True)):
        with pytest.raises(ValueError, match="KarrasSchedule"):
            adp.KarrasSchedule(**kw)
    with pytest.raises(ValueError, match="num_steps"):
        SCHEDULE(0, "cpu")
