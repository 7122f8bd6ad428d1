"""RePaint inpainting: `VRepainter`, `RFRepainter`, `KRepainter` and the kernels of include/adp_repaint.h.

Nothing in the reference provides the scheme (its `VInpainter` re-noises the known region only), so the contract is the
mathematics, restated here in float64.  A level is x_l = a_l x0 + b_l n with (a, b) = (cos, sin)(sigma pi / 2) | (1 - t, t) |
(1, sigma) for "v" | "rf" | "k".  From a_0 (mask ? source : 0) + b_0 n0, for step i and resample r:

    p = net(state, level_i) ;  (x0, eps) = the objective's predictions ;  y = a_{i+1} clip(x0) + b_{i+1} eps
    r < R - 1:  y <- A y + S z,  A = a_i / a_{i+1},  S = sqrt(b_i^2 - (A b_{i+1})^2),  j = i ;   r = R - 1:  j = i + 1
    state = mask ? a_j source + b_j z : y

`repaint_ref` is that loop on the UNSCALED state for all three objectives (for "k" it knows nothing of the scaled state or
of the folded coefficients); `repaint_step_ref` is one kernel call on the row the kernel is given.

KERNEL_TOL.  Kernel errors are measured in the max norm relative to the largest INPUT magnitude M (x, p, source, z), as
tests/test_edm.py measures its own: the bound then follows from the coefficients alone.  The objective's step is at most 6
float32 roundings on its longest path (tests/test_rf.py and tests/test_edm.py count theirs, and count them as 8); the jump
adds two (A * y and the multiply-add with S z), the known region is two on its own: 10 roundings of 2**-24.  Every rounded
value, times the coefficients it still passes through, is at most G M with the row's gain G = max(|A| G_step + |S|,
|P| + |Q|), G_step the sum of the absolute values of every term of the step for unit inputs (the clamps and the division by
a scale >= 1 only shrink).  For the rows used here G <= 4, which `_rows` asserts on the float64 rows before any kernel
runs: v and rf steps have G_step <= 2 with A < 1 and S < 1; for sd = 0.5 the K step has G_step <= 2 * 0.71 + 1 * 1.42 = 2.84
(tests/test_edm.py), A = r_{i+1} / r_i < 1, S < 1, P <= 2 and Q <= 1.  10 * 2**-24 * 4 = 2.4e-6; the bound is twice that,
4.8e-6, as the STEP_TOLs of those files double their own counts.
"""
import copy
import math

import pytest
import torch
import torch.nn as nn

import audio_diffusion_pytorch_amd as adp
from audio_diffusion_pytorch_amd import diffusion, ops
from conftest import rel_err
from test_edm import GaussianF, edm_step_ref, edm_table, err_in
from test_multistep_sampler import GaussianV
from test_rf import GaussianU, rf_step_ref, rf_table
from test_stochastic_sampler import STAT_TOL
from test_threshold_sampler import clip_ref, threshold_step_ref

KERNEL_GAIN = 4.0
KERNEL_TOL = 2 * (10 * 2.0 ** -24 * KERNEL_GAIN)   # 4.8e-6 of the largest input (module docstring)
LOOP_TOL = 1e-5                                    # a loop against its restatement on the same net and backend (tests/test_inpaint_graph.py)
SD = 0.5
SEED = 0x51C0FFEE9A3B7D21
OBJECTIVES = ("v", "rf", "k")
WORDS = {"v": 4, "rf": 6, "k": 8}
assert KERNEL_TOL <= 5e-6


# ------------------------------------------------------------------ float64 restatement of the contract
def ab_of(obj, levels):
    l = levels.double()
    if obj == "v":
        return torch.cos(l * (math.pi / 2)), torch.sin(l * (math.pi / 2))
    return (1 - l, l) if obj == "rf" else (torch.ones_like(l), l)


def step_table(obj, levels, sd=SD):
    """The objective's own first-order rows in float64."""
    if obj == "v":
        a, b = ab_of(obj, levels)
        return torch.stack([a[:-1], b[:-1], a[1:], b[1:]], dim=1)
    return rf_table(levels, order=1) if obj == "rf" else edm_table(levels, sd, order=1, eta=0.0)


def table_ref(obj, levels, R, sd=SD):
    """Rows (step row, A, S, P, Q) in float64, [N R, W + 4] in loop order; for "k" with the scale factors folded in."""
    a, b = ab_of(obj, levels)
    l = levels.double()
    n = l.numel() - 1
    step = step_table(obj, levels, sd)
    c_in = 1 / torch.sqrt(l * l + sd * sd) if obj == "k" else torch.ones_like(l)
    rows = []
    for i in range(n):
        A = a[i] / a[i + 1]
        S = torch.sqrt((b[i] ** 2 - (A * b[i + 1]) ** 2).clamp_min(0.0))
        g = 1.0 if (obj != "k" or i == n - 1) else c_in[i + 1]      # the factor the step row applied
        for r in range(R):
            if r < R - 1:
                tail = [c_in[i] * A / g, c_in[i] * S, c_in[i] * a[i], c_in[i] * b[i]]
            elif obj == "k" and i == n - 1:
                tail = [1.0, 0.0, 1.0, 0.0]
            else:
                tail = [1.0, 0.0, c_in[i + 1] * a[i + 1], c_in[i + 1] * b[i + 1]]
            rows.append(torch.cat([step[i], torch.tensor([float(t) for t in tail], dtype=torch.float64)]))
    return torch.stack(rows) if rows else torch.zeros(0, WORDS[obj] + 4, dtype=torch.float64)


def repaint_step_ref(obj, x, p, src, mask, row, z, clip=False, scale=None):
    """One kernel call in float64 on the row the kernel is given.  `scale` [B] or None; clip without a scale is the static
    clamp.  z is used where S != 0 and, in the known region, where Q != 0."""
    w = WORDS[obj]
    step = row[:w].double().clone()
    A, S, P, Q = [float(c) for c in row[w:].double()]
    if obj == "v":
        if clip:
            y = threshold_step_ref(x, p, None, None, step, scale)[0]
        else:
            a0, b0, a1, b1 = step
            xd, pd = x.double(), p.double()
            y = a1 * (a0 * xd - b0 * pd) + b1 * (b0 * xd + a0 * pd)
    elif obj == "rf":
        step[5] = 0.0
        y = rf_step_ref(x, p, None, step, clip=clip, scale=scale)[0]
    else:
        step[6] = step[7] = 0.0
        y = edm_step_ref(x, p, None, step, None, clip=clip, scale=scale)[0]
    if S != 0:
        y = A * y + S * z.double()
    elif A != 1:
        y = A * y
    k = P * src.double()
    if Q != 0:
        k = k + Q * z.double()
    return torch.where(mask.bool(), k, y)


def draw(seed, d, like):
    """Draw d of the seed in the shape of `like`, from the library's generator on `like`'s backend."""
    return ops.randn(like, ops.rng_rows(seed, [d])[0].to(like.device))


def predict(obj, x, p, level, sd=SD):
    """(x0, eps) from the UNSCALED state x at `level` and the net's output p, float64."""
    if obj == "v":
        a, b = math.cos(level * math.pi / 2), math.sin(level * math.pi / 2)
        return a * x - b * p, b * x + a * p
    if obj == "rf":
        return x - level * p, x + (1 - level) * p
    r = math.sqrt(level * level + sd * sd)
    d = (sd * sd / (r * r)) * x + (level * sd / r) * p
    return d, (x - d) / level


def net_input(obj, x, level, sd=SD):
    return x / math.sqrt(level * level + sd * sd) if obj == "k" else x


def net_arg(obj, l32, i, dev):
    """What the net is given at level i: the float32 value the product forms, on the same backend."""
    lv = l32[i].to(dev)
    return torch.log(lv) * 0.25 if obj == "k" else lv


def default_levels(obj, n):
    sched = adp.KarrasSchedule(0.002, 80.0) if obj == "k" else adp.LinearSchedule()
    return sched(n + 1, device="cpu").to(torch.float32)


@torch.no_grad()
def repaint_ref(obj, net, source, mask, num_steps, num_resamples, seed, q=None, x_noisy=None, levels=None, sd=SD,
                scales=None, **kw):
    """The scheme of the module docstring in float64 on the unscaled state.  `net` runs in float32 wherever `source` lives;
    the draws are `ops.randn`'s there.  `q`: None, 0.0 (static clamp) or a quantile; `scales`, a list, receives each
    resample's scale row."""
    dev = source.device
    l32 = default_levels(obj, num_steps) if levels is None else levels.to(torch.float32).cpu()
    l = [float(v) for v in l32.double()]
    a, b = [[float(v) for v in t] for t in ab_of(obj, l32)]
    src = source.double()
    n0 = draw(seed, 0, source) if x_noisy is None else x_noisy
    x = a[0] * torch.where(mask, src, torch.zeros_like(src)) + b[0] * n0.double()
    for i in range(num_steps):
        for r in range(num_resamples):
            p = net(net_input(obj, x, l[i], sd).float(), net_arg(obj, l32, i, dev).expand(x.shape[0]), **kw).double()
            x0, eps = predict(obj, x, p, l[i], sd)
            if q:
                scale = clip_ref(x0.cpu(), q)[1].to(dev)
                if scales is not None:
                    scales.append(scale.cpu())
                s = diffusion.pad_dims(scale, x.ndim - 1)
                x0 = x0.clamp(-s, s) / s
            elif q is not None:
                x0 = x0.clamp(-1.0, 1.0)
            y = a[i + 1] * x0 + b[i + 1] * eps
            z = draw(seed, 1 + i * num_resamples + r, source).double()
            j = i + 1
            if r < num_resamples - 1:
                A = a[i] / a[i + 1]
                y = A * y + math.sqrt(max(b[i] ** 2 - (A * b[i + 1]) ** 2, 0.0)) * z
                j = i
            x = torch.where(mask, a[j] * src + b[j] * z, y)
    return x


def make(obj, net, **kw):
    if obj == "v":
        return adp.VRepainter(net, **kw)
    if obj == "rf":
        return adp.RFRepainter(net, **kw)
    return adp.KRepainter(net, adp.KarrasSchedule(0.002, 80.0), sigma_data=SD, **kw)


class Counting(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net, self.calls = net, 0

    def forward(self, x, time, **kw):
        self.calls += 1
        return self.net(x, time, **kw)


# ------------------------------------------------------------------ 1. the kernel against the restatement
KERNEL_LEVELS = {"v": torch.tensor([0.62, 0.3, 0.0]), "rf": torch.tensor([0.62, 0.3, 0.0]), "k": torch.tensor([3.0, 0.5, 0.0])}
KIND_ROW = {"jump": 0, "last": 1, "final": 3}      # of the table for R = 2: (0, jump), (0, last), (1, jump), (1, last = final)
SHAPES = [(1, 1, 1), (1, 1, 7), (3, 1, 5), (2, 2, 1025), (2, 3, 4099)]
MASKS = ("none", "all", "random", "single")
Q = 0.9


def _step_gain(obj, row):
    r = row.abs()
    if obj == "v":
        return (r[2] + r[3]) * (r[0] + r[1])
    if obj == "rf":
        return r[4] * (r[0] + r[1]) + r[3] * (1 + r[2])
    return r[4] * (r[0] + r[1]) + r[5] * (r[2] + r[3])


def _rows(obj):
    """The float32 rows the kernel is given, by kind; the gain KERNEL_TOL was derived under is asserted on the float64 rows."""
    table = table_ref(obj, KERNEL_LEVELS[obj], 2)
    w = WORDS[obj]
    for row in table:
        A, S, P, Q_ = row[w:].abs()
        assert max(A * _step_gain(obj, row) + S, P + Q_) <= KERNEL_GAIN, row
    given = ops.repaint_table(obj, KERNEL_LEVELS[obj], 2, SD)
    rows = {kind: given[i] for kind, i in KIND_ROW.items()}
    w4 = rows["jump"][w:], rows["last"][w:], rows["final"][w:]
    assert w4[0][1] > 0.1 and w4[0][3] > 0.1                       # the jump draws everywhere
    assert w4[1][0] == 1 and w4[1][1] == 0 and w4[1][3] > 0.1       # the last resample of a step moves on; the known region draws
    assert w4[2][0] == 1 and w4[2][1] == 0 and w4[2][2] == 1 and w4[2][3] == 0
    return rows


def _mask(kind, shape, g):
    if kind == "none":
        return torch.zeros(shape, dtype=torch.bool)
    if kind == "all":
        return torch.ones(shape, dtype=torch.bool)
    if kind == "random":
        return torch.rand(shape, generator=g) > 0.5
    m = torch.zeros(shape, dtype=torch.bool)      # a single True, inside a group of four where the tensor has one
    m.view(-1)[min(6, m.numel() - 1)] = True
    return m


def _kernel_case(shape, mask_kind):
    g = torch.Generator().manual_seed(shape[0] * 100003 + shape[-1])
    x, p, src = [torch.randn(shape, generator=g) * 1.5 for _ in range(3)]
    return x, p, src, _mask(mask_kind, shape, g)


def _rng(dev, d=3):
    return ops.rng_rows(SEED, [d])[0].to(dev)


def _check_kernel(dev, obj, mode, kind, inplace, shape, mask_kind):
    row = _rows(obj)[kind]
    x, p, src, mask = _kernel_case(shape, mask_kind)
    dx, dp, ds, dm, drow, rng = x.to(dev), p.to(dev), src.to(dev), mask.to(torch.uint8).to(dev), row.to(dev), _rng(dev)
    z = ops.randn(dx, rng).cpu()
    scale = None
    if mode == "scale":   # the restatement clamps with the scale the product's own select returned
        scale = ops.clip_scale(dx, Q, v=dp, coef=drow, min_scale=1.0)
        assert scale.shape == (shape[0],) and bool((scale >= 1).all())
    want = repaint_step_ref(obj, x, p, src, mask, row, z, clip=mode != "none", scale=None if scale is None else scale.cpu())
    out = ops.repaint_step(obj, dx, dp, ds, dm, drow, rng, scale=scale, clip=mode != "none", out=dx if inplace else None)
    assert (out is dx) == inplace and out.shape == x.shape
    if not inplace:
        assert torch.equal(dx.cpu(), x)
    assert torch.equal(dp.cpu(), p) and torch.equal(ds.cpu(), src) and torch.equal(dm.cpu().bool(), mask)
    assert torch.equal(drow.cpu(), row) and torch.equal(rng.cpu(), _rng("cpu"))
    err = err_in(out, want, x, p, src, z)
    print(f"adp_repaint_{obj}_step {shape} {mode} {kind} mask={mask_kind} inplace={inplace}: err {err:.3e} "
          f"(bound {KERNEL_TOL:.2e})")
    assert err <= KERNEL_TOL
    return out


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("kind", list(KIND_ROW))
@pytest.mark.parametrize("mode", ["none", "static", "scale"])
@pytest.mark.parametrize("obj", OBJECTIVES)
def test_kernel_matches_restatement(dev, obj, mode, kind, inplace):
    assert 5 % 4 != 0   # at (3, 1, 5) a group of four straddles two items
    for shape in SHAPES:
        for mask_kind in MASKS:
            _check_kernel(dev, obj, mode, kind, inplace, shape, mask_kind)


@pytest.mark.gpu
@pytest.mark.parametrize("obj", OBJECTIVES)
def test_kernel_beyond_one_pass_of_the_grid(hip, obj):
    """4096 workgroups of 256 threads own four elements each per pass: this case needs a second pass, and a tail."""
    shape = (1, 2, 2 ** 21 + 3)
    assert 2 * (2 ** 21 + 3) > 4096 * 256 * 4
    _check_kernel(hip, obj, "scale", "jump", True, shape, "random")


def test_the_known_region_and_the_jump_use_randn_of_the_same_row(dev):
    """With x = p = 0 and source = 0 the output is S z where the mask is clear and Q z where it is set: the normals of
    `ops.randn` for the same row, element by element."""
    shape = (2, 1, 1001)
    row = _rows("rf")["jump"]
    S, Q_ = row[7].item(), row[9].item()
    zero = torch.zeros(shape).to(dev)
    mask = _mask("random", shape, torch.Generator().manual_seed(2))
    rng = _rng(dev, 11)
    z = ops.randn(zero, rng).cpu()
    out = ops.repaint_step("rf", zero, zero, zero, mask.to(torch.uint8).to(dev), row.to(dev), rng).cpu()
    assert torch.equal(out, torch.where(mask, Q_ * z, S * z))


# ------------------------------------------------------------------ 2. bit equalities
@pytest.mark.parametrize("mode", ["none", "static", "scale"])
@pytest.mark.parametrize("obj", OBJECTIVES)
def test_a_row_without_noise_does_not_read_the_generator(dev, obj, mode):
    rows = _rows(obj)
    x, p, src, mask = _kernel_case((2, 3, 4099), "random")
    dx, dp, ds, dm = x.to(dev), p.to(dev), src.to(dev), mask.to(torch.uint8).to(dev)
    row = rows["final"].to(dev)
    scale = ops.clip_scale(dx, Q, v=dp, coef=row, min_scale=1.0) if mode == "scale" else None
    kw = dict(scale=scale, clip=mode != "none")
    with_row = ops.repaint_step(obj, dx, dp, ds, dm, row, _rng(dev), **kw)
    without = ops.repaint_step(obj, dx, dp, ds, dm, row, None, **kw)
    assert torch.isfinite(without).all() and torch.equal(with_row, without)
    assert torch.equal(without.cpu()[mask], src[mask]), "P = 1, Q = 0: the source itself"
    # a row that needs a normal and has no generator row is loud: NaN where z is used, nothing dereferenced
    none = torch.zeros_like(dm)
    assert torch.isnan(ops.repaint_step(obj, dx, dp, ds, none, rows["jump"].to(dev), None, **kw)).all()
    last = ops.repaint_step(obj, dx, dp, ds, dm, rows["last"].to(dev), None, **kw).cpu()
    assert torch.isnan(last[mask]).all() and torch.isfinite(last[~mask]).all()
    # ... and with nothing known the last resample of a step draws nothing at all
    assert torch.isfinite(ops.repaint_step(obj, dx, dp, ds, none, rows["last"].to(dev), None, **kw)).all()


WIDE = 2.0   # data N(0, 2**2): the predicted clean value leaves [-1, 1], so the thresholds act


def gaussian_net(obj, s=WIDE):
    return GaussianV(s) if obj == "v" else GaussianU(s) if obj == "rf" else GaussianF(s, SD)


def first_order_sampler(obj, net, q):
    if obj == "v":
        return adp.VSampler(net) if q is None else adp.VThresholdSampler(net, dynamic_threshold=q, order=1)
    if obj == "rf":
        return adp.RFSampler(net, order=1, dynamic_threshold=q)
    return adp.KSampler(net, adp.KarrasSchedule(0.002, 80.0), sigma_data=SD, order=1, eta=0.0, dynamic_threshold=q)


EQ_SHAPE, EQ_STEPS = (2, 2, 261), 5


def _eq_case(dev):
    g = torch.Generator().manual_seed(4)
    source, n0 = torch.randn(EQ_SHAPE, generator=g), torch.randn(EQ_SHAPE, generator=g)
    return source.to(dev), n0.to(dev), (torch.rand(EQ_SHAPE, generator=g) > 0.5).to(dev)


@pytest.mark.parametrize("q", [None, 0.0, 0.9], ids=["none", "static", "q0.9"])
@pytest.mark.parametrize("obj", OBJECTIVES)
def test_nothing_known_and_one_resample_is_the_first_order_sampler(dev, obj, q):
    source, n0, _ = _eq_case(dev)
    net = gaussian_net(obj)
    nothing = torch.zeros(EQ_SHAPE, dtype=torch.bool, device=dev)
    out = make(obj, net, dynamic_threshold=q)(source, nothing, num_steps=EQ_STEPS, num_resamples=1, x_noisy=n0, seed=SEED)
    sampler = first_order_sampler(obj, net, q)
    if obj == "k":
        want = sampler(n0, num_steps=EQ_STEPS)              # (forms 0 + sigma_0 n0, scaled, by the same kernel)
    else:
        first = default_levels(obj, EQ_STEPS)[0].expand(EQ_SHAPE[0]).contiguous().to(dev)
        noised = ops.v_noise if obj == "v" else ops.rf_noise
        want = sampler(noised(torch.zeros_like(n0), n0, first)[0], num_steps=EQ_STEPS)
    assert torch.isfinite(out).all() and torch.equal(out, want)
    if q is not None:   # the condition under which the thresholded case says anything
        plain = make(obj, net)(source, nothing, num_steps=EQ_STEPS, num_resamples=1, x_noisy=n0, seed=SEED)
        assert not torch.equal(out, plain)


@pytest.mark.parametrize("obj", OBJECTIVES)
def test_the_known_region_ends_as_the_source(dev, obj):
    """The schedules end at level 0: the last row has P = 1, Q = 0."""
    source, _, mask = _eq_case(dev)
    rp = make(obj, gaussian_net(obj))
    out = rp(source, mask, num_steps=4, num_resamples=2, seed=SEED)
    assert torch.isfinite(out).all()
    assert torch.equal(out[mask], source[mask]) and not torch.equal(out[~mask], source[~mask])
    assert torch.equal(rp(source, torch.ones_like(mask), num_steps=3, num_resamples=2, seed=SEED), source)
    # a mask that broadcasts: the second half of every item
    half = torch.zeros(1, 1, EQ_SHAPE[2], dtype=torch.bool, device=dev)
    half[..., EQ_SHAPE[2] // 2:] = True
    out = rp(source, half, num_steps=3, num_resamples=2, seed=SEED)
    assert torch.equal(out[..., EQ_SHAPE[2] // 2:], source[..., EQ_SHAPE[2] // 2:])


# ------------------------------------------------------------------ 3. the table
@pytest.mark.parametrize("obj", OBJECTIVES)
def test_table_matches_restatement(emul, obj):
    levels = default_levels(obj, 12)
    for R in (1, 3):
        got = ops.repaint_table(obj, levels, R, SD)
        w = WORDS[obj]
        assert got.shape == (12 * R, w + 4) and got.dtype == torch.float32 and got.device.type == "cpu"
        want = table_ref(obj, levels, R)
        # both are float64 values rounded to float32 once; the v step row is formed in float32 (VSampler's own): cos and sin
        # of a float32 angle, 2**-24 of pi / 2 off
        assert torch.allclose(got[:, w:], want[:, w:].to(torch.float32), rtol=2 ** -23, atol=0)
        assert torch.allclose(got[:, :w], want[:, :w].to(torch.float32), rtol=2 ** -23, atol=2 ** -22 if obj == "v" else 0)
        moves = got[R - 1::R, w:]
        assert bool((moves[:, 0] == 1).all()) and bool((moves[:, 1] == 0).all())
        assert moves[-1, 2] == 1 and moves[-1, 3] == 0
        if R > 1:
            assert bool((got[0::R, w + 1] > 0).all())
    # the step rows are the samplers' own, bit for bit
    n = 12
    if obj == "v":
        own = adp.VSampler(GaussianV(0.5))._tables(n, 1, "cpu")[1]
    elif obj == "rf":
        own = adp.RFSampler(GaussianU(0.5), order=1)._tables(n, 1, "cpu")[1]
    else:
        own = adp.KSampler(GaussianF(0.5), adp.KarrasSchedule(0.002, 80.0), sigma_data=SD, order=1)._tables(n, 1, "cpu")[1]
    assert torch.equal(ops.repaint_table(obj, levels, 1, SD)[:, :WORDS[obj]], own)


def test_the_run_table_holds_the_draws(emul):
    rp = adp.RFRepainter(GaussianU(0.5))
    table = rp._table(default_levels("rf", 3), 2, 5 + (9 << 32))
    assert table.shape == (6, 6 + 4 + 4) and table.dtype == torch.int32
    assert table[:, 10:].tolist() == [[5, 9, 1 + k, 0] for k in range(6)]
    assert torch.equal(table[:, :10].view(torch.float32), ops.repaint_table("rf", default_levels("rf", 3), 2))


# ------------------------------------------------------------------ 4. the loop against the restatement through a net
SHAPE, STEPS = (2, 2, 32), 2
# a time-conditioned UNetV0 of two levels: an emulated forward of it takes well under a second
SMALL = dict(in_channels=2, channels=[8, 16], factors=[1, 2], items=[1, 1], modulation_features=32)
_RUNS = {}


def tiny_net(dev, seed=0):
    torch.manual_seed(seed)
    return adp.UNetV0(dim=1, **SMALL).to(dev).eval()


def _case(dev, seed=5, gain=3.0):   # (wide enough for the predicted clean value to leave [-1, 1])
    g = torch.Generator().manual_seed(seed)
    source = gain * torch.randn(SHAPE, generator=g)
    mask = torch.rand(SHAPE, generator=g) > 0.5
    return source.to(dev), mask.to(dev)


def _run(dev, obj, R, q, monkeypatch):
    """(net, source, mask, result) of the eager run with SEED, once per backend and case (an emulated U-Net forward takes
    a moment) and never modified.  While it runs, torch.randn_like raises and the net's calls are counted."""
    key = (dev.type, obj, R, q)
    if key not in _RUNS:
        net = tiny_net(dev)
        source, mask = _case(dev)
        counting = Counting(net)

        def forbidden(*a, **kw):
            raise AssertionError("torch's generator on the philox path")

        with monkeypatch.context() as m:
            m.setattr(torch, "randn_like", forbidden)
            kept = source.clone()
            out = make(obj, counting, dynamic_threshold=q, use_graph=False)(source, mask, num_steps=STEPS, num_resamples=R,
                                                                            seed=SEED)
        assert counting.calls == STEPS * R, "one net evaluation per resample"
        assert torch.equal(source, kept)
        _RUNS[key] = (net, source, mask, out)
    return _RUNS[key]


@pytest.mark.parametrize("q", [None, 0.9], ids=["none", "q0.9"])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("obj", OBJECTIVES)
def test_loop_matches_restatement_through_a_unet(dev, monkeypatch, obj, R, q):
    net, source, mask, out = _run(dev, obj, R, q, monkeypatch)
    assert out.shape == source.shape and torch.isfinite(out).all() and torch.equal(out[mask], source[mask])
    scales = []
    want = repaint_ref(obj, net, source, mask, STEPS, R, SEED, q=q, scales=scales)
    if q:   # the condition under which the thresholded case says anything
        assert len(scales) == STEPS * R and any(s > 1 for row in scales for s in row.tolist()), scales
    err = rel_err(out, want)
    print(f"{obj} repainter R={R} q={q}: rel_err vs float64 loop {err:.3e} (bound {LOOP_TOL:.0e})")
    assert err <= LOOP_TOL
    if R > 1:           # resampling is another trajectory
        once = _RUNS.get((dev.type, obj, 1, q))
        assert once is None or rel_err(out, once[3]) > 1e-3


@pytest.mark.parametrize("obj", OBJECTIVES)
def test_seed_and_start(dev, obj):
    """The same seed gives the same bits, another seed another result; a given x_noisy replaces draw 0 and nothing else; a
    missing seed comes from torch's default CPU generator (so torch.manual_seed governs it)."""
    source, _, mask = _eq_case(dev)
    rp = make(obj, gaussian_net(obj))
    run = lambda **kw: rp(source, mask, num_steps=2, num_resamples=2, **kw)
    a = run(seed=SEED)
    other = run(seed=SEED + 1)
    assert torch.equal(a, run(seed=SEED)) and not torch.equal(a, other) and torch.equal(other[mask], source[mask])
    start = draw(SEED, 0, source)
    kept = start.clone()
    assert torch.equal(a, run(seed=SEED, x_noisy=start)) and torch.equal(start, kept)
    # the draws behind the start noise follow the seed as well
    assert not torch.equal(a, run(seed=SEED + 1, x_noisy=start))
    # (from level 1 the first jump back forgets the start: another start noise shows where no resample jumps)
    straight = lambda n0: rp(source, mask, num_steps=2, num_resamples=1, seed=SEED, x_noisy=n0)
    assert not torch.equal(straight(start), straight(draw(SEED, 99, source)))
    torch.manual_seed(123)
    d1, d2 = run(), run()
    torch.manual_seed(123)
    assert torch.equal(d1, run()) and not torch.equal(d1, d2)


def test_one_resample_agrees_with_vinpainter(dev, monkeypatch):
    """At R = 1 both schemes step and re-noise the known region at the next level with the same draw; they differ only in
    how the known region's sum is rounded (and that is overwritten by the source at the end)."""
    net, source, mask, out = _run(dev, "v", 1, None, monkeypatch)
    want = adp.VInpainter(net, noise="philox")(source, mask, num_steps=STEPS, num_resamples=1, seed=SEED)
    err = rel_err(out, want)
    print(f"VRepainter vs VInpainter(philox) at R = 1: rel_err {err:.3e} (bound {LOOP_TOL:.0e})")
    assert err <= LOOP_TOL


def test_kwargs_reach_the_net(dev):
    class Shifted(nn.Module):
        def forward(self, x, t, shift=None):
            return GaussianU(0.5)(x, t) + (0.0 if shift is None else shift)

        def prepare_sampling_kwargs(self, x, kwargs):
            kwargs = dict(kwargs)
            kwargs["shift"] = kwargs.pop("amount") * torch.ones_like(x)
            return kwargs

    source, _, mask = _eq_case(dev)
    rp = adp.RFRepainter(Shifted())
    a, b = (rp(source, mask, num_steps=3, num_resamples=2, seed=SEED, amount=v) for v in (0.0, 0.5))
    assert torch.equal(a, adp.RFRepainter(GaussianU(0.5))(source, mask, num_steps=3, num_resamples=2, seed=SEED))
    assert not torch.equal(a, b)


# ------------------------------------------------------------------ 5. the jump is variance-consistent
STAT_S, STAT_N, STAT_R, STAT_SHAPE = 0.3, 10, 3, (1, 1, 65536)


def analytic_variance(obj, R, jump_noise=True, s=STAT_S, n=STAT_N):
    """Elementwise variance of the scheme's output with nothing known, for x ~ N(0, b_0**2) and the optimal predictor of
    N(0, s**2) data, which is linear in x: a step multiplies the variance by its linear gain squared, a jump maps
    v -> A**2 v + S**2."""
    l32 = default_levels(obj, n)
    l = [float(v) for v in l32.double()]
    a, b = [[float(v) for v in t] for t in ab_of(obj, l32)]
    net = gaussian_net(obj, s)
    one = torch.ones(1, 1, 1, dtype=torch.float64)
    var = b[0] ** 2
    for i in range(n):
        p = net(net_input(obj, one, l[i]), net_arg(obj, l32, i, "cpu").expand(1)).double()
        x0, eps = predict(obj, one, p, l[i])
        gain = (a[i + 1] * x0 + b[i + 1] * eps).item()
        A = a[i] / a[i + 1]
        S2 = max(b[i] ** 2 - (A * b[i + 1]) ** 2, 0.0)
        for r in range(R):
            var = gain * gain * var
            if r < R - 1:
                var = A * A * var + (S2 if jump_noise else 0.0)
    return var


@pytest.mark.parametrize("obj", OBJECTIVES)
def test_output_variance_is_the_schemes_own(dev, obj):
    want, silent = analytic_variance(obj, STAT_R), analytic_variance(obj, STAT_R, jump_noise=False)
    assert abs(silent / want - 1) > 2 * STAT_TOL     # the test can tell a jump without its noise apart
    source = torch.zeros(STAT_SHAPE).to(dev)
    nothing = torch.zeros(STAT_SHAPE, dtype=torch.bool).to(dev)
    out = make(obj, gaussian_net(obj, STAT_S))(source, nothing, num_steps=STAT_N, num_resamples=STAT_R, seed=SEED)
    got = out.double().var().item()
    print(f"{obj}: variance analytic {want:.5f} (jumps without noise: {silent:.3e}), product {got:.5f}; data {STAT_S ** 2:.5f}; "
          f"bound {STAT_TOL:.4f} relative")
    assert abs(got / want - 1) <= STAT_TOL


# ------------------------------------------------------------------ 6. resampling harmonises
class Consensus(nn.Module):
    """The closed-form optimal denoiser for data x0 = g 1 over an item's n positions, g ~ N(0, 1), in the objective's
    parametrisation (a plain module, not a U-Net): from x = a g 1 + b noise the posterior mean of g is
    a sum(x) / (b**2 + n a**2)."""

    def __init__(self, obj, sd=SD):
        super().__init__()
        self.obj, self.sd = obj, sd

    def forward(self, x, arg):
        x = x.double()
        lv = arg.double().view(-1, *([1] * (x.ndim - 1)))
        if self.obj == "v":
            a, b = torch.cos(lv * (math.pi / 2)), torch.sin(lv * (math.pi / 2))
        elif self.obj == "rf":
            a, b = 1 - lv, lv
        else:
            b = torch.exp(4 * lv)
            a = torch.ones_like(b)
            r = torch.sqrt(b * b + self.sd ** 2)
            x = r * x
        n = x[0].numel()
        x0 = a * x.flatten(1).sum(dim=1).view_as(lv) / (b * b + n * a * a) * torch.ones_like(x)
        if self.obj == "v":
            p = (a * x - x0) / b
        elif self.obj == "rf":
            p = (x - x0) / b
        else:
            p = (x0 - (self.sd ** 2 / (r * r)) * x) / (b * self.sd / r)
        return p.float()


HARM_SHAPE, HARM_N, HARM_G = (512, 1, 64), 10, 1.5


def _harmony_error(inpainter, dev, R):
    """RMS over the items of (mean of the generated half - g), the first half known with g = 1.5."""
    source = torch.full(HARM_SHAPE, HARM_G).to(dev)
    mask = torch.zeros(HARM_SHAPE, dtype=torch.bool)
    mask[..., :HARM_SHAPE[2] // 2] = True
    out = inpainter(source, mask.to(dev), num_steps=HARM_N, num_resamples=R, seed=SEED).double().cpu()
    assert torch.isfinite(out).all()
    return (out[..., HARM_SHAPE[2] // 2:].mean(dim=-1) - HARM_G).pow(2).mean().sqrt().item()


@pytest.mark.parametrize("obj", OBJECTIVES)
def test_resampling_harmonises(dev, obj):
    """What the feature is for: the generated half is pulled towards the known one by the resamples.  The float64
    restatement gives ratios 0.11 (v), 0.09 (rf) and 0.005 (k) between R = 4 and R = 1."""
    rp = make(obj, Consensus(obj))
    e1, e4 = _harmony_error(rp, dev, 1), _harmony_error(rp, dev, 4)
    print(f"{obj} repainter: RMS error of the generated half R=1 {e1:.4f}, R=4 {e4:.4f}, ratio {e4 / e1:.3f} (bound 0.5)")
    assert e4 <= 0.5 * e1


def test_vinpainter_resampling_does_not(dev):
    """The reference's scheme on the same problem: its resamples leave the generated region where it was (the float64
    restatement gives 0.98)."""
    inp = adp.VInpainter(Consensus("v"), noise="philox")
    e1, e4 = _harmony_error(inp, dev, 1), _harmony_error(inp, dev, 4)
    print(f"VInpainter: RMS error of the generated half R=1 {e1:.4f}, R=4 {e4:.4f}, ratio {e4 / e1:.3f} (bound > 0.8)")
    assert e4 > 0.8 * e1


# ------------------------------------------------------------------ 7. the replayed resample
@pytest.mark.gpu
@pytest.mark.parametrize("q", [None, 0.9], ids=["none", "q0.9"])
@pytest.mark.parametrize("obj", OBJECTIVES)
def test_replay_equals_eager(hip, obj, q):
    net = tiny_net(hip)
    source, mask = _case(hip)
    g, e = make(obj, net, dynamic_threshold=q), make(obj, net, dynamic_threshold=q, use_graph=False)
    assert g.use_graph
    out = g(source, mask, num_steps=STEPS, num_resamples=2, seed=7)
    assert torch.equal(out, e(source, mask, num_steps=STEPS, num_resamples=2, seed=7))
    assert torch.equal(out[mask], source[mask])
    out2 = g(source, mask, num_steps=5, num_resamples=3, seed=8)
    assert torch.equal(out2, e(source, mask, num_steps=5, num_resamples=3, seed=8)) and not torch.equal(out, out2)
    assert g.graph_captures == 1 and g.graph_replays == 2 and len(g._graph_cache) == 1 and e.graph_captures == 0
    entry = next(iter(g._graph_cache.values()))
    assert len(entry.bufs) == (2 if q else 0) and entry.srow.shape == (WORDS[obj] + 8,)
    # other source / mask / start through the same entry; the caller's tensors are not touched
    source2, mask2 = _case(hip, seed=6)
    start = torch.randn(SHAPE, generator=torch.Generator().manual_seed(9)).to(hip)
    kept = start.clone()
    out3 = g(source2, mask2, num_steps=STEPS, num_resamples=2, seed=7, x_noisy=start)
    assert torch.equal(out3, e(source2, mask2, num_steps=STEPS, num_resamples=2, seed=7, x_noisy=start))
    assert torch.equal(start, kept) and g.graph_captures == 1
    # show_progress is served eagerly
    assert torch.equal(g(source, mask, num_steps=STEPS, num_resamples=2, seed=7, show_progress=True), out)
    assert g.graph_replays == 3
    # the clip mode is another step
    g.dynamic_threshold = e.dynamic_threshold = 0.0
    assert torch.equal(g(source, mask, num_steps=2, num_resamples=2, seed=7), e(source, mask, num_steps=2, num_resamples=2, seed=7))
    assert g.graph_captures == 2


@pytest.mark.gpu
@pytest.mark.parametrize("obj", OBJECTIVES)
def test_recapture_after_parameters_moved_and_deepcopy(hip, obj):
    net = tiny_net(hip)
    source, mask = _case(hip)
    g = make(obj, net, dynamic_threshold=0.9)
    out = g(source, mask, num_steps=STEPS, num_resamples=2, seed=7)
    cp = copy.deepcopy(g)
    assert len(cp._graph_cache) == 0 and cp.graph_captures == 0 and cp.graph_replays == 0
    assert cp.dynamic_threshold == 0.9 and cp.use_graph
    assert torch.equal(cp(source, mask, num_steps=STEPS, num_resamples=2, seed=7), out)
    assert cp.graph_captures == 1 and g.graph_captures == 1
    # new weights in fresh storage (allocated while the old storage is alive): the old graph holds dead addresses
    gen = torch.Generator().manual_seed(4)
    sd = {k: v + 0.05 * v.abs().mean() * torch.randn(v.shape, generator=gen).to(v.device) for k, v in net.state_dict().items()}
    net.load_state_dict(sd, assign=True)
    out_new = g(source, mask, num_steps=STEPS, num_resamples=2, seed=7)
    assert g.graph_captures == 2 and len(g._graph_cache) == 1, "the stale entry was not recaptured"
    eager = make(obj, net, dynamic_threshold=0.9, use_graph=False)(source, mask, num_steps=STEPS, num_resamples=2, seed=7)
    assert torch.equal(out_new, eager) and not torch.equal(out_new, out)


# ------------------------------------------------------------------ 8. arguments
class Rising(adp.Schedule):
    def forward(self, num_steps, device):
        return torch.linspace(0.1, 0.9, num_steps, device=device)


class Flat(adp.Schedule):
    def forward(self, num_steps, device):
        return torch.tensor([0.9, 0.5, 0.5, 0.0][:num_steps], device=device)


def test_bad_arguments_raise(emul):
    net = GaussianU(0.5)
    karras = adp.KarrasSchedule(0.002, 80.0)
    for bad in (-0.1, 1.5, "0.9", True):
        with pytest.raises(ValueError, match="dynamic_threshold"):
            adp.VRepainter(net, dynamic_threshold=bad)
        with pytest.raises(ValueError, match="dynamic_threshold"):
            adp.RFRepainter(net, dynamic_threshold=bad)
        with pytest.raises(ValueError, match="dynamic_threshold"):
            adp.KRepainter(net, karras, dynamic_threshold=bad)
    for bad in (0.0, -1.0, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="sigma_data"):
            adp.KRepainter(net, karras, sigma_data=bad)
    source, mask = torch.zeros(2, 2, 16), torch.zeros(2, 2, 16, dtype=torch.bool)
    for cls in (adp.VRepainter, adp.RFRepainter):
        for sched in (Rising(), Flat()):
            with pytest.raises(ValueError, match="schedule"):
                cls(net, schedule=sched)(source, mask, num_steps=3, num_resamples=2, seed=1)
    for sched in (Rising(), Flat(), adp.LinearSchedule(1.0, -1.0)):
        with pytest.raises(ValueError, match="schedule"):
            adp.KRepainter(net, sched)(source, mask, num_steps=3, num_resamples=2, seed=1)
    for rp in (adp.VRepainter(net), adp.RFRepainter(net), adp.KRepainter(net, karras)):
        for bad in (0, -1, 1.5, True):
            with pytest.raises(ValueError, match="num_resamples"):
                rp(source, mask, num_steps=2, num_resamples=bad, seed=1)
        with pytest.raises(ValueError, match="mask"):
            rp(source, torch.zeros(2, 2, 15, dtype=torch.bool), num_steps=2, num_resamples=1, seed=1)
        with pytest.raises(ValueError, match="mask"):
            rp(source, torch.zeros(2, 2, 16), num_steps=2, num_resamples=1, seed=1)       # a soft mask
        with pytest.raises(ValueError, match="source"):
            rp(source.double(), mask, num_steps=2, num_resamples=1, seed=1)
        with pytest.raises(ValueError, match="x_noisy"):
            rp(source, mask, num_steps=2, num_resamples=1, seed=1, x_noisy=torch.zeros(2, 2, 8))
        assert isinstance(rp, adp.diffusion.Inpainter)
    assert {"VRepainter", "RFRepainter", "KRepainter"} <= set(adp.__all__)


def test_wrappers_reject_bad_arguments(emul):
    x, m, row = torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.uint8), torch.zeros(10)
    for call in (lambda: ops.repaint_step("ddpm", x, x, x, m, row),
                 lambda: ops.repaint_step("rf", x, torch.zeros(2, 7), x, m, row),
                 lambda: ops.repaint_step("rf", x, x, torch.zeros(2, 7), m, row),
                 lambda: ops.repaint_step("rf", x, x, x, torch.zeros(16, dtype=torch.uint8), row),
                 lambda: ops.repaint_step("rf", x, x, x, m, torch.zeros(8)),            # the v row
                 lambda: ops.repaint_step("v", x, x, x, m, row),
                 lambda: ops.repaint_step("k", x, x, x, m, row),
                 lambda: ops.repaint_step("rf", x, x, x, m, row.double()),
                 lambda: ops.repaint_step("rf", x, x, x, m, row, torch.zeros(3, dtype=torch.int32)),
                 lambda: ops.repaint_step("rf", x, x, x, m, row, scale=torch.ones(2)),  # a scale without clip
                 lambda: ops.repaint_step("rf", x, x, x, m, row, scale=torch.ones(3), clip=True),
                 lambda: ops.repaint_step("rf", x, x, x, m, row, clip=1),
                 lambda: ops.repaint_step("rf", x, x, x, m, row, out=torch.zeros(16)),
                 lambda: ops.repaint_table("ddpm", torch.tensor([1.0, 0.0]), 1),
                 lambda: ops.repaint_table("rf", torch.tensor([1.0, 0.5, 0.5, 0.0]), 1),   # a repeated level
                 lambda: ops.repaint_table("rf", torch.tensor([0.0, 0.5, 1.0]), 1),        # rising
                 lambda: ops.repaint_table("v", torch.tensor([1.5, 0.5, 0.0]), 1),         # beyond the objective's range
                 lambda: ops.repaint_table("k", torch.tensor([1.0, 0.5, -0.1]), 1),
                 lambda: ops.repaint_table("k", torch.tensor([float("inf"), 0.5, 0.0]), 1),
                 lambda: ops.repaint_table("k", torch.tensor([1.0, 0.0]), 1, sigma_data=0.0),
                 lambda: ops.repaint_table("rf", torch.tensor([1.0, 0.0]), 0),
                 lambda: ops.repaint_table("rf", torch.tensor([1.0, 0.0]), 1.0),
                 lambda: ops.repaint_table("rf", torch.tensor([]), 1)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        ops.repaint_step("rf", x, x, x, m.to(torch.float32), row)
    assert torch.equal(x, torch.zeros(2, 8))
