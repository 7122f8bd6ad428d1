"""optim.AdamW: the fused AdamW + gradient-clipping + EMA step (adp_sqnorm_partials / adp_adamw_step).

Parity rule (every comparison with torch below): the reference is torch.optim.AdamW (+ clip_grad_norm_, + lerp_ for the EMA)
run in float64 on the CPU from the same initial values and the same gradient sequence; the yardstick is torch's own float32
run of that sequence.  Per tensor:  rel_err(native, f64) <= 4 * max(rel_err(torch_f32, f64), 2**-23)  with conftest.rel_err
(the factor 4 allows another, equally valid fp32 evaluation order: fused multiply-adds, the clip coefficient applied when the
gradient is read instead of stored).  Every figure is printed before it is asserted (pytest -s); the largest ratio
native / max(torch_f32, 2**-23) seen over all cases here is 1.07 on the emulator and 1.48 on the MI355X (the end-to-end test)."""
import copy

import pytest
import torch
import torch.nn as nn

import audio_diffusion_pytorch_amd as adp
from audio_diffusion_pytorch_amd import AdamW, graphed
from audio_diffusion_pytorch_amd.optim import CHUNK
from conftest import rel_err

SIZES = [1, 7, 8, 1023, 4096 + 3, 20000]   # 20000 = three chunks
SPLIT = 3                                  # parameters [0, 3) are group 0, the rest group 1
TRAINER = dict(lr=1e-4, betas=(0.95, 0.999), eps=1e-6, weight_decay=1e-3)
DEFAULTS = dict()
GROUP1 = dict(lr=3e-3, weight_decay=0.1)   # the second group's own values
STEPS = 20
EPS32 = 2.0 ** -23


def _grads(gen, sizes=SIZES):
    """|g| in [1e-3, 1] (log-uniform), random sign: sqrt(v) stays far from underflow, the quotient well conditioned."""
    return [(10.0 ** (-3.0 * torch.rand(n, generator=gen))) * (torch.randint(0, 2, (n,), generator=gen) * 2.0 - 1.0)
            for n in sizes]


def _init(seed=0, sizes=SIZES):
    gen = torch.Generator().manual_seed(seed)
    return [0.5 * torch.randn(n, generator=gen) for n in sizes]


def _groups(params, hp, emas=None):
    a = {"params": params[:SPLIT]}
    b = {"params": params[SPLIT:], **GROUP1}
    if emas is not None:
        a["ema_params"], b["ema_params"] = emas[:SPLIT], emas[SPLIT:]
    return [a, b], hp


def _torch_run(dtype, init, grad_seq, hp, max_norm=None, ema_decay=None, opt_state=None):
    """torch.optim.AdamW + clip_grad_norm_ + lerp_ on the CPU in `dtype`; returns (params, optimizer, emas, norms)."""
    params = [nn.Parameter(t.to(dtype).clone()) for t in init]
    groups, kw = _groups(params, hp)
    opt = torch.optim.AdamW(groups, **kw)
    if opt_state is not None:
        opt.load_state_dict(opt_state)
    emas = [p.detach().clone() for p in params]
    norms = []
    for grads in grad_seq:
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.to(dtype).clone()
        if max_norm is not None:
            norms.append(torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2).detach().clone())
        opt.step()
        if ema_decay is not None:
            with torch.no_grad():
                for e, p in zip(emas, params):
                    e.lerp_(p, 1.0 - ema_decay)
    return params, opt, emas, norms


class _Native:
    """The native optimizer over tensors on `dev`; gradients either separate tensors or views of ONE flat buffer that starts
    at an odd element offset (what the U-Net backward hands out)."""

    def __init__(self, dev, init, hp, max_norm=None, ema_decay=None, flat=False):
        self.dev = dev
        self.params = [nn.Parameter(t.clone().to(dev)) for t in init]
        self.emas = [p.detach().clone() for p in self.params] if ema_decay is not None else None
        groups, kw = _groups(self.params, hp, self.emas)
        self.opt = AdamW(groups, max_grad_norm=max_norm, ema_decay=ema_decay, **kw)
        self.norms = []
        self.views = None
        if flat:
            self.flat = torch.zeros(1 + sum(t.numel() for t in init), device=dev)
            self.views, off = [], 1
            for t in init:
                self.views.append(self.flat[off:off + t.numel()])
                off += t.numel()

    def set_grads(self, grads):
        for i, (p, g) in enumerate(zip(self.params, grads)):
            if g is None:
                p.grad = None
            elif self.views is not None:
                self.views[i].copy_(g)
                p.grad = self.views[i]
            else:
                p.grad = g.clone().to(self.dev)

    def run(self, grad_seq):
        for grads in grad_seq:
            self.set_grads(grads)
            self.opt.step()
            if self.opt.max_grad_norm is not None:
                self.norms.append(self.opt.grad_norm.detach().cpu().clone())
        return self


def _check(name, native, t32, t64, report):
    e32, en = rel_err(t32, t64), rel_err(native, t64)
    bound = 4.0 * max(e32, EPS32)
    report.append(f"{name}: native {en:.3e} torch_f32 {e32:.3e} ratio {en / max(e32, EPS32):.2f}")
    print(report[-1])
    return en <= bound


def _check_all(nat, r32, r64, report, ema=False, norms=False):
    """Parameters, both moments, EMA tensors and the gradient norms of a native run against the two torch runs."""
    ok = True
    p32, o32, e32, n32 = r32
    p64, o64, e64, n64 = r64
    for i, p in enumerate(nat.params):
        ok &= _check(f"p[{i}]", p, p32[i], p64[i], report)
        st = nat.opt.state.get(p, {})
        if p64[i] in o64.state:
            for key in ("exp_avg", "exp_avg_sq"):
                ok &= _check(f"{key}[{i}]", st[key], o32.state[p32[i]][key], o64.state[p64[i]][key], report)
            assert float(st["step"]) == float(o64.state[p64[i]]["step"])
        else:
            assert len(st) == 0
        if ema:
            ok &= _check(f"ema[{i}]", nat.emas[i], e32[i], e64[i], report)
    if norms:
        assert len(nat.norms) == len(n64)
        for k, (a, b, c) in enumerate(zip(nat.norms, n32, n64)):
            ok &= _check(f"grad_norm[step {k}]", a, b, c, report)
    assert ok, "\n".join(report)


def _yardstick_is_sound(r32):
    """The float32 torch run itself must be finite and non-degenerate for the chosen inputs."""
    p32, o32, e32, _ = r32
    for p in p32:
        assert torch.isfinite(p).all()
        if p in o32.state:
            v = o32.state[p]["exp_avg_sq"]
            assert torch.isfinite(v).all() and v.min().item() > 1e-30, "sqrt(v) near underflow: ill-conditioned quotient"
    for e in e32:
        assert torch.isfinite(e).all()


CASES = {
    "plain": dict(),
    "clip_inactive": dict(max_norm=1e9),
    "clip_active": dict(max_norm=0.5),
    "ema": dict(ema_decay=0.999),
    "all": dict(max_norm=0.5, ema_decay=0.999),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("hp", [TRAINER, DEFAULTS], ids=["trainer", "defaults"])
def test_parity_with_torch(dev, hp, case):
    kw = CASES[case]
    gen = torch.Generator().manual_seed(1234)
    init = _init()
    grad_seq = [_grads(gen) for _ in range(STEPS)]
    r64 = _torch_run(torch.float64, init, grad_seq, hp, **kw)
    r32 = _torch_run(torch.float32, init, grad_seq, hp, **kw)
    _yardstick_is_sound(r32)
    if case == "clip_active":
        assert all(n.item() > 2 * kw["max_norm"] for n in r64[3]), "the clip is meant to be active"
    nat = _Native(dev, init, hp, flat=True, **kw).run(grad_seq)
    _check_all(nat, r32, r64, [], ema="ema_decay" in kw, norms="max_norm" in kw)
    assert nat.opt.table_builds == 1


def test_flat_views_and_separate_tensors_agree_and_grad_is_untouched(dev):
    """Gradients as odd-offset slices of one buffer and as separate tensors: the update is the same element by element
    (torch.equal without clipping: 16-byte and scalar paths round alike), both satisfy the parity rule with clipping, and .grad
    is bit-identical before and after a clipped step (the coefficient is applied at load)."""
    gen = torch.Generator().manual_seed(7)
    init = _init(1)
    grad_seq = [_grads(gen) for _ in range(STEPS)]
    a = _Native(dev, init, TRAINER, ema_decay=0.99, flat=True).run(grad_seq)
    b = _Native(dev, init, TRAINER, ema_decay=0.99, flat=False).run(grad_seq)
    for x, y in zip(a.params + a.emas, b.params + b.emas):
        assert torch.equal(x, y)
    kw = dict(max_norm=0.5, ema_decay=0.99)
    r64 = _torch_run(torch.float64, init, grad_seq, TRAINER, **kw)
    r32 = _torch_run(torch.float32, init, grad_seq, TRAINER, **kw)
    for flat in (True, False):
        nat = _Native(dev, init, TRAINER, flat=flat, **kw)
        nat.run(grad_seq[:-1])
        nat.set_grads(grad_seq[-1])
        before = [p.grad.clone() for p in nat.params]
        nat.opt.step()
        nat.norms.append(nat.opt.grad_norm.detach().cpu().clone())
        for p, g0 in zip(nat.params, before):
            assert torch.equal(p.grad, g0), "step() scaled .grad"
        assert nat.norms[-1].item() > 1.0  # the clip was active
        _check_all(nat, r32, r64, [], ema=True, norms=True)


def test_misaligned_parameters_and_state(dev):
    """Parameters / moments / EMA tensors that are themselves odd-offset views: with a common 16-byte phase the kernel peels
    a scalar head, with different phases it takes the scalar path; both equal the aligned run bit for bit."""
    gen = torch.Generator().manual_seed(3)
    sizes = [5, 1023, CHUNK + 4099]
    init = _init(2, sizes)
    grad_seq = [_grads(gen, sizes) for _ in range(4)]

    def run(p_off, s_off):
        params, emas, grads = [], [], []
        for t in init:
            n = t.numel()
            buf = torch.zeros(n + 8, device=dev)
            buf[p_off:p_off + n].copy_(t)
            params.append(nn.Parameter(buf[p_off:p_off + n]))
            ebuf = torch.zeros(n + 8, device=dev)
            ebuf[s_off:s_off + n].copy_(t)
            emas.append(ebuf[s_off:s_off + n])
            grads.append(torch.zeros(n + 8, device=dev)[3:3 + n])
        opt = AdamW(params, max_grad_norm=0.5, ema_params=emas, ema_decay=0.9, **TRAINER)
        for p in params:
            n = p.numel()
            opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.zeros(n + 8, device=dev)[s_off:s_off + n],
                            "exp_avg_sq": torch.zeros(n + 8, device=dev)[s_off:s_off + n]}
        for gs in grad_seq:
            for p, gv, g in zip(params, grads, gs):
                gv.copy_(g)
                p.grad = gv
            opt.step()
        return [p.detach().clone() for p in params] + [e.clone() for e in emas] + \
               [opt.state[p][k].clone() for p in params for k in ("exp_avg", "exp_avg_sq")]

    aligned = run(0, 0)
    for offs in ((1, 1), (3, 3), (1, 2), (0, 3)):
        for x, y in zip(run(*offs), aligned):
            assert torch.equal(x, y), offs


def test_parameters_without_gradient_are_skipped(dev):
    """grad is None: no state, no step; once the gradient shows up the parameter gets its OWN bias corrections."""
    gen = torch.Generator().manual_seed(5)
    init = _init(3)
    grad_seq = [_grads(gen) for _ in range(STEPS)]
    for k in range(8):            # parameters 1 and 4 join late, parameter 5 pauses
        grad_seq[k][1] = None
    for k in range(3):
        grad_seq[k][4] = None
    for k in range(5, 9):
        grad_seq[k][5] = None
    r64 = _torch_run(torch.float64, init, grad_seq, TRAINER, max_norm=0.5)
    r32 = _torch_run(torch.float32, init, grad_seq, TRAINER, max_norm=0.5)
    nat = _Native(dev, init, TRAINER, max_norm=0.5, flat=True)
    nat.run(grad_seq[:2])
    assert len(nat.opt.state.get(nat.params[1], {})) == 0 and float(nat.opt.state[nat.params[0]]["step"]) == 2
    nat.run(grad_seq[2:])
    assert float(nat.opt.state[nat.params[1]]["step"]) == STEPS - 8
    assert float(nat.opt.state[nat.params[5]]["step"]) == STEPS - 4
    _check_all(nat, r32, r64, [], norms=True)
    assert nat.opt.table_builds == 5  # the first step, then 4 joins, 5 leaves, 1 joins, 5 returns


def test_state_dict_interchange_with_torch(dev):
    gen = torch.Generator().manual_seed(9)
    init = _init(4)
    grad_seq = [_grads(gen) for _ in range(STEPS + 1)]
    head, last = grad_seq[:STEPS], grad_seq[STEPS:]
    # torch -> native
    t32 = _torch_run(torch.float32, init, head, TRAINER)
    nat = _Native(dev, [p.detach() for p in t32[0]], TRAINER, flat=True)
    sd = copy.deepcopy(t32[1].state_dict())
    nat.opt.load_state_dict(sd)
    assert float(nat.opt.state[nat.params[0]]["step"]) == STEPS
    nat.run(last)
    # (the float64 reference continues from ITS OWN state: the comparison covers all STEPS + 1 steps)
    r64 = _torch_run(torch.float64, init, grad_seq, TRAINER)
    r32 = _torch_run(torch.float32, init, grad_seq, TRAINER)
    _check_all(nat, r32, r64, [])
    # native -> torch: same keys, and torch continues from it
    nat2 = _Native(dev, init, TRAINER, flat=True).run(head)
    sd2 = nat2.opt.state_dict()
    assert set(sd2["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert set(sd2["param_groups"][0]) == set(t32[1].state_dict()["param_groups"][0])
    sd2 = {"state": {k: {n: v.detach().cpu().clone() for n, v in s.items()} for k, s in sd2["state"].items()},
           "param_groups": copy.deepcopy(sd2["param_groups"])}
    cont = _torch_run(torch.float32, [p.detach().cpu() for p in nat2.params], last, TRAINER, opt_state=sd2)
    for i in range(len(init)):
        assert float(cont[1].state[cont[0][i]]["step"]) == STEPS + 1
        assert _check(f"p[{i}] torch continues", cont[0][i], r32[0][i], r64[0][i], [])


def test_two_runs_from_equal_state_are_bit_identical(dev):
    gen = torch.Generator().manual_seed(11)
    init = _init(5)
    grad_seq = [_grads(gen) for _ in range(6)]
    kw = dict(max_norm=0.5, ema_decay=0.99)
    for flat in (True, False):
        a = _Native(dev, init, TRAINER, flat=flat, **kw).run(grad_seq)
        b = _Native(dev, init, TRAINER, flat=flat, **kw).run(grad_seq)
        for x, y in zip(a.params + a.emas + a.norms, b.params + b.emas + b.norms):
            assert torch.equal(x, y)
        for p, q in zip(a.params, b.params):
            assert torch.equal(a.opt.state[p]["exp_avg_sq"], b.opt.state[q]["exp_avg_sq"])


def test_tables_are_built_once_and_rebuilt_when_something_moves(dev):
    gen = torch.Generator().manual_seed(13)
    init = _init(6)
    nat = _Native(dev, init, TRAINER, max_norm=1.0, ema_decay=0.99, flat=True)
    assert nat.opt.table_builds == 0
    nat.run([_grads(gen) for _ in range(4)])
    assert nat.opt.table_builds == 1
    nat.opt.zero_grad()                       # set_to_none: the gradients are gone ...
    nat.run([_grads(gen) for _ in range(2)])  # ... and come back at the same addresses, as a replayed backward hands them out
    assert nat.opt.table_builds == 1
    nat.params[2].grad = nat.params[2].grad.clone()  # a gradient moved
    nat.opt.step()
    assert nat.opt.table_builds == 2
    nat.opt.step()
    assert nat.opt.table_builds == 2
    nat.params[3].data = nat.params[3].data.clone()  # a parameter's storage was replaced
    nat.opt.step()
    assert nat.opt.table_builds == 3
    for g in nat.opt.param_groups:                    # a scheduler writing group["lr"] needs no rebuild and is picked up
        g["lr"] = 0.0
        g["weight_decay"] = 0.0
    before = [p.detach().clone() for p in nat.params]
    nat.opt.step()
    assert nat.opt.table_builds == 3
    for p, q in zip(nat.params, before):
        assert torch.equal(p, q)


def test_lr_scheduler_and_closure(dev):
    gen = torch.Generator().manual_seed(17)
    init = _init(7)
    grad_seq = [_grads(gen) for _ in range(STEPS)]

    def sched(opt):
        return torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=0.5)

    def ref(dtype):
        params = [nn.Parameter(t.to(dtype).clone()) for t in init]
        groups, kw = _groups(params, TRAINER)
        opt = torch.optim.AdamW(groups, **kw)
        s = sched(opt)
        for grads in grad_seq:
            for p, g in zip(params, grads):
                p.grad = g.to(dtype).clone()
            opt.step()
            s.step()
        return params

    nat = _Native(dev, init, TRAINER, flat=True)
    s = sched(nat.opt)
    for grads in grad_seq:
        nat.set_grads(grads)
        seen = []

        def closure():
            assert torch.is_grad_enabled()
            seen.append(1)
            return torch.tensor(3.0)

        assert nat.opt.step(closure).item() == 3.0 and seen == [1]
        s.step()
    p32, p64 = ref(torch.float32), ref(torch.float64)
    report = []
    assert all([_check(f"p[{i}]", p, p32[i], p64[i], report) for i, p in enumerate(nat.params)]), "\n".join(report)


@pytest.mark.parametrize("option", [dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(foreach=True),
                                    dict(foreach=False), dict(fused=True), dict(fused=False), dict(differentiable=True)],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_unsupported_options_raise_and_name_the_option(option):
    p = [nn.Parameter(torch.zeros(4))]
    with pytest.raises(NotImplementedError, match=next(iter(option))):
        AdamW(p, **option)


def test_ema_arguments_are_validated():
    p = [nn.Parameter(torch.zeros(4)), nn.Parameter(torch.zeros(3))]
    e = [torch.zeros(4), torch.zeros(3)]
    with pytest.raises(ValueError, match="ema_decay"):
        AdamW(p, ema_params=e)
    with pytest.raises(ValueError, match="ema_decay"):
        AdamW(p, ema_decay=0.99)
    with pytest.raises(ValueError, match="ema_params"):
        AdamW(p, ema_params=e[:1], ema_decay=0.99)
    with pytest.raises(ValueError, match="shape"):
        AdamW(p, ema_params=[torch.zeros(4), torch.zeros(5)], ema_decay=0.99)
    with pytest.raises(ValueError, match="ema_params"):
        AdamW([{"params": p[:1], "ema_params": e[:1]}, {"params": p[1:]}], ema_decay=0.99)
    with pytest.raises(ValueError, match="IS its parameter"):
        AdamW(p, ema_params=p, ema_decay=0.99)
    opt = AdamW([{"params": p[:1], "ema_params": e[:1]}, {"params": p[1:], "ema_params": e[1:]}], ema_decay=0.99)
    assert "ema_params" not in opt.param_groups[0] and "ema_params" not in opt.state_dict()["param_groups"][0]


def test_unsupported_tensors_raise_with_the_parameter_index(dev):
    good = nn.Parameter(torch.zeros(4, device=dev))
    good.grad = torch.ones(4, device=dev)
    bad = nn.Parameter(torch.zeros(4, dtype=torch.float64, device=dev))
    bad.grad = torch.ones(4, dtype=torch.float64, device=dev)
    with pytest.raises(TypeError, match="parameter 1"):
        AdamW([good, bad]).step()
    strided = nn.Parameter(torch.zeros(4, 4, device=dev).t())
    strided.grad = torch.ones(4, 4, device=dev)
    with pytest.raises(TypeError, match="parameter 1"):
        AdamW([good, strided]).step()
    sparse = nn.Parameter(torch.zeros(4, 2, device=dev))
    sparse.grad = torch.sparse_coo_tensor(torch.tensor([[0, 2]]), torch.ones(2, 2), (4, 2)).to(dev)
    with pytest.raises(RuntimeError, match="parameter 1.*sparse|sparse.*parameter 1"):
        AdamW([good, sparse]).step()
    assert torch.equal(good.detach().cpu(), torch.zeros(4)), "a refused step must not have updated anything"


def test_kernels_refuse_cpu_tensors_without_the_emulator():
    """No fallback: off the emulator a CPU parameter is an error, not an eager update."""
    from audio_diffusion_pytorch_amd import _C
    _C._testing_use_library(None, allow_cpu=False)
    p = nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError):
        AdamW([p]).step()


# ---------------------------------------------------------------------------------------------- on the MI355X only
TINY = dict(in_channels=2, channels=[8, 32, 64], factors=[1, 4, 4], items=[1, 2, 2], modulation_features=128)
E2E = dict(lr=1e-4, betas=(0.95, 0.999), eps=1e-6, weight_decay=1e-3)


def _model(dev, seed=0, **extra):
    torch.manual_seed(seed)
    return adp.DiffusionModel(net_t=adp.UNetV0, **TINY, **extra).to(dev)


@pytest.mark.gpu
def test_readme_loop_with_native_adamw_and_ema_model(hip):
    """Five README-loop steps (replayed training step + native AdamW with clipping and an EMA model) against torch.optim.AdamW
    fed the recorded gradients in float64 / float32 on the CPU; the EMA model, whose sampler graph was captured BEFORE the
    training, samples with the current EMA weights and equals an eager sample of a model loaded with them."""
    xs = [torch.randn(2, 2, 4096, device=hip) for _ in range(5)]
    noise = torch.randn(1, 2, 4096, device=hip)
    model = _model(hip, seed=3)
    init = [p.detach().cpu().clone() for p in model.parameters()]
    ema_model = copy.deepcopy(model)
    first = ema_model.sample(noise, num_steps=2)
    assert ema_model.sampler.graph_captures == 1
    opt = AdamW(model.parameters(), max_grad_norm=1.0, ema_params=ema_model.parameters(), ema_decay=0.9, **E2E)
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    recorded, losses, norms = [], [], []
    for x in xs:
        opt.zero_grad()
        loss = model(x)
        loss.backward()
        recorded.append([p.grad.detach().cpu().clone() for p in model.parameters()])
        opt.step()
        losses.append(loss.item())
        norms.append(opt.grad_norm.item())
    g = graphed.GRAPHS_OF[model.diffusion]
    assert g.captures == 1 and g.replays == 5
    assert opt.table_builds == 1, "the replayed backward hands out the same addresses: one table"

    def replay(dtype):
        params = [nn.Parameter(t.to(dtype).clone()) for t in init]
        ref = torch.optim.AdamW(params, **E2E)
        emas = [p.detach().clone() for p in params]
        ns = []
        for grads in recorded:
            for p, gr in zip(params, grads):
                p.grad = gr.to(dtype).clone()
            ns.append(torch.nn.utils.clip_grad_norm_(params, 1.0).item())
            ref.step()
            with torch.no_grad():
                for e, p in zip(emas, params):
                    e.lerp_(p, 0.1)
        return params, emas, ns

    p64, e64, n64 = replay(torch.float64)
    p32, e32, n32 = replay(torch.float32)
    report, ok = [], True
    for i, (p, e) in enumerate(zip(model.parameters(), ema_model.parameters())):
        ok &= _check(f"p[{i}]", p, p32[i], p64[i], report)
        ok &= _check(f"ema[{i}]", e, e32[i], e64[i], report)
    for k in range(5):
        ok &= _check(f"grad_norm[{k}]", *(torch.tensor(v, dtype=torch.float64) for v in (norms[k], n32[k], n64[k])), report)
    assert ok, "\n".join(r for r in report)

    # the same loop with torch.optim.AdamW (+ clip_grad_norm_): same seeds, so the first loss is the same number and the
    # trajectories stay within the project's 1e-3 parity contract over five small steps
    twin = _model(hip, seed=3)
    topt = torch.optim.AdamW(twin.parameters(), **E2E)
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    tl = []
    for x in xs:
        topt.zero_grad()
        loss = twin(x)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(twin.parameters(), 1.0)
        topt.step()
        tl.append(loss.item())
    assert tl[0] == losses[0]
    assert all(abs(a - b) <= 1e-3 * abs(b) for a, b in zip(losses, tl)), (losses, tl)

    # EMA weights are in place: same sampler graph, new numbers, equal to an eager sample from the same tensors
    s_g = ema_model.sample(noise, num_steps=2)
    assert ema_model.sampler.graph_captures == 1 and not torch.equal(s_g, first)
    eager = _model(hip, seed=5, sampler_use_graph=False)
    eager.load_state_dict(ema_model.state_dict())
    assert torch.equal(s_g, eager.sample(noise, num_steps=2))


@pytest.mark.gpu
def test_step_never_synchronises(hip):
    gen = torch.Generator().manual_seed(19)
    init = _init(8)
    nat = _Native(hip, init, TRAINER, max_norm=0.5, ema_decay=0.99, flat=True)
    nat.run([_grads(gen) for _ in range(2)])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            nat.opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert nat.opt.table_builds == 1 and torch.isfinite(nat.opt.grad_norm).item()
