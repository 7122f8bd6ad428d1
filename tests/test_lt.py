"""The learned-transform front end (audio_diffusion_pytorch_amd.lt, csrc/lt.hip, include/adp_lt.h): the three kernels against
float64 torch, call-to-call determinism, C-ABI return codes, the module contract of `LTPlugin`, and the plugin end to end
against the CPU composition (torch convolutions around the oracle U-Net).

Reference of the kernels: F.conv1d(F.pad(x, (p, p), mode="reflect"), w, stride=s) and F.conv_transpose1d(y, w, stride=s,
padding=p) in float64 and their float64 autograd gradients from random output gradients.  Bound: 1e-4 (test_kernels.TOL,
the project's bound for single ops) on conftest.rel_err.  End to end: 1e-3, the project's parity contract.
"""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import audio_diffusion_pytorch_amd as adp
from audio_diffusion_pytorch_amd import _C, lt, ops
from audio_diffusion_pytorch_amd.components import _AppendChannelsNet
from conftest import rel_err
from oracle import vdiffusion as ovd
from oracle.a_unet_restatement import UNetV0Oracle
from test_unet import FixedSigmas

TOL = 1e-4        # tests/test_kernels.py TOL
PARITY_TOL = 1e-3  # tests/test_unet.py TOL

# (B, C, F, W, s, T, Cout).  The tiled kernels cut the frame axis into tiles of 128 (lt_conv: frames, lt_convt: q) and
# the weight gradient into segments that are multiples of 32 frames; they take layers with at least 8 transform channels.
GEOMETRIES = {
    "vec16": (2, 2, 4, 8, 4, 64, 2),          # 16-byte paths
    "odd": (1, 3, 5, 7, 3, 45, 3),            # odd everything; C F = 15 is below one MFMA tile
    "nooverlap": (2, 1, 16, 16, 16, 256, 1),  # W = s, p = 0
    "overlap4": (1, 2, 24, 32, 8, 320, 2),    # four overlapping windows; C F = 48 spans tiles, no multiple of 32
    "borders": (1, 2, 4, 32, 8, 16, 2),       # T = p + 4: the reflected borders cover almost the whole signal, L = 2
    "cout": (2, 2, 8, 8, 4, 64, 3),           # decode to a different channel count
    "long": (1, 2, 8, 8, 4, 1160, 2),         # L = 290: three frame tiles of 128, the last one partial (34)
    "oddsplit": (1, 3, 6, 7, 3, 99, 3),       # odd stride and window, C F = 18: a second, partial reduction chunk per channel
}
# Dispatch, checked by hand against csrc/lt.hip's conditions and asserted below from the launch trace: a tiled kernel needs
# at least 8 rows / columns of its fragment filled -- lt_conv: O = C F; lt_convt: O s (C s for the encode data gradient,
# Cout s for the decode forward); lt_wgrad: A = C F -- and a segment within the LDS plan (every geometry here: a few hundred
# floats of 12288).  The smallest values above are 8 (vec16, borders, cout, long), so EVERY kernel of EVERY geometry is the
# tiled one.  16-byte staging (lt_conv_tile_kernel<true>) needs s, T multiples of 4 (p = 2 only shifts the segment): all but odd and oddsplit;
# 16-byte weight loads (lt_convt_tile_kernel<true>) need s, W multiples of 4: the same set.
VEC_GEOMETRIES = {"vec16", "nooverlap", "overlap4", "borders", "cout", "long"}


def launched(fn):
    """(result of fn(), names of the kernels it launched) from the library's launch trace."""
    _C.PROFILE = []
    try:
        out = fn()
    finally:
        recs = _C.profile_collect()
    return out, [k for _, k, _, _ in recs]


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs (float32) and the float64 reference of one geometry; computed once, shared, never modified."""
    B, C, Fn, W, s, T, Cout = GEOMETRIES[name]
    p = W // 2 - s // 2
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    r = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    L = (T + 2 * p - W) // s + 1
    d = dict(B=B, C=C, W=W, s=s, T=T, p=p, L=L, Cout=Cout)
    d["x"], d["we"], d["gy"] = r(B, C, T), r(C * Fn, C, W) / (C * W) ** 0.5, r(B, C * Fn, L)
    d["yin"], d["wd"], d["go"] = r(B, Cout * Fn, L), r(Cout * Fn, Cout, W) / (Cout * Fn) ** 0.5, r(B, Cout, T)
    x, we = d["x"].double().requires_grad_(), d["we"].double().requires_grad_()
    y = F.conv1d(F.pad(x, (p, p), mode="reflect") if p else x, we, stride=s)
    d["y"] = y.detach()
    d["dx"], d["dwe"] = torch.autograd.grad(y, (x, we), d["gy"].double())
    yin, wd = d["yin"].double().requires_grad_(), d["wd"].double().requires_grad_()
    out = F.conv_transpose1d(yin, wd, stride=s, padding=p)
    assert out.shape[-1] == T and y.shape[-1] == L
    d["out"] = out.detach()
    d["dyin"], d["dwd"] = torch.autograd.grad(out, (yin, wd), d["go"].double())
    return d


def run_all(d, dev):
    """The six operations of one geometry on the kernels."""
    t = lambda k: d[k].to(dev)  # noqa: E731
    s, p, W = d["s"], d["p"], d["W"]
    return dict(
        y=ops.lt_conv(t("x"), t("we"), s, p, ops.LT_REFLECT),
        out=ops.lt_convt(t("yin"), t("wd"), s, p, ops.LT_PLAIN),
        dx=ops.lt_convt(t("gy"), t("we"), s, p, ops.LT_FOLD, T=d["T"]),
        dyin=ops.lt_conv(t("go"), t("wd"), s, p, ops.LT_ZERO),
        dwe=ops.lt_wgrad(t("gy"), t("x"), W, s, p, ops.LT_REFLECT),
        dwd=ops.lt_wgrad(t("yin"), t("go"), W, s, p, ops.LT_ZERO))


# ------------------------------------------------------------------ 1. kernel parity
@pytest.mark.parametrize("path", ["tiled", "per_output"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_kernels_match_float64_torch(dev, name, path, monkeypatch):
    """Both layers and their four gradients; `per_output` sends every call to the kernels behind the tiled ones."""
    if path == "per_output":
        monkeypatch.setenv("ADP_LT_TILED", "0")
    d = case(name)
    got, kernels = launched(lambda: run_all(d, dev))
    print(f"lt {name} [{path}] kernels: {sorted(set(kernels))}")
    if path == "tiled":
        vec = "true" if name in VEC_GEOMETRIES else "false"
        want = {f"lt_conv_tile_kernel<{vec}>": 2, f"lt_convt_tile_kernel<{vec}>": 2, "lt_wgrad_tile_kernel": 2,
                "lt_wgrad_sum_kernel": 2, "lt_convt_fold_kernel": 1 if d["p"] else 0}
    else:
        want = {"lt_conv_plain_kernel": 2, "lt_convt_plain_kernel": 2, "lt_wgrad_plain_kernel": 2, "lt_wgrad_sum_kernel": 2}
    assert {k: kernels.count(k) for k in set(kernels)} == {k: n for k, n in want.items() if n}, kernels
    bad = []
    for k, v in got.items():
        assert v.shape == d[k].shape and v.dtype == torch.float32, k
        err = rel_err(v, d[k])
        print(f"lt {name} [{path}] {k}: rel err {err:.3e} (bound {TOL:.0e})")
        if not err < TOL:
            bad.append((k, err))
    assert not bad, bad


# ------------------------------------------------------------------ 2. determinism
@pytest.mark.parametrize("name", ["overlap4", "odd", "long"])
def test_weight_gradients_are_written_and_deterministic(dev, name):
    d = case(name)
    a, b = run_all(d, dev), run_all(d, dev)
    import os
    assert os.environ.get("ADP_DEBUG_POISON") == "1"   # conftest.py: every output below was NaN-filled before its launch
    for k in ("dwe", "dwd", "y", "out", "dx", "dyin"):
        assert torch.isfinite(a[k]).all(), f"{k}: an element was left unwritten"
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ["borders", "odd"])
def test_per_output_kernels_write_every_element(dev, name, monkeypatch):
    monkeypatch.setenv("ADP_LT_TILED", "0")
    for k, v in run_all(case(name), dev).items():
        assert torch.isfinite(v).all(), f"{k}: an element was left unwritten"


# ------------------------------------------------------------------ 3. C-ABI
def test_c_abi_return_codes(dev):
    lib, st = _C.lib(), _C.stream()
    ERR_SHAPE, ERR_UNSUPPORTED, ERR_NULL = -1, -2, -5
    B, C, O, K, s, p, T = 2, 2, 8, 8, 4, 2, 64
    L = (T + 2 * p - K) // s + 1
    SENTINEL = 7.5
    x, w = torch.randn(B, C, T).to(dev), torch.randn(O, C, K).to(dev)
    y = torch.full((B, O, L), SENTINEL).to(dev)
    xo = torch.full((B, C, T), SENTINEL).to(dev)
    dw = torch.full((O, C, K), SENTINEL).to(dev)
    ws_bytes = lib.adp_lt_wgrad_ws_bytes(B, O, C, L, K)
    assert ws_bytes >= 4 * O * C * K
    ws = torch.empty(ws_bytes // 4).to(dev)
    P = lambda t: t.data_ptr()  # noqa: E731

    def conv(**kw):
        a = dict(x=P(x), w=P(w), B=B, C=C, T=T, O=O, K=K, s=s, p=p, mode=1, y=P(y))
        a.update(kw)
        return lib.adp_lt_conv(*a.values(), st)

    def convt(**kw):   # (the encode data gradient: [B, O, L] -> [B, C, T])
        a = dict(x=P(y), w=P(w), B=B, C=O, L=L, O=C, K=K, s=s, p=p, mode=1, T=T, out=P(xo))
        a.update(kw)
        return lib.adp_lt_convt(*a.values(), st)

    def wgrad(**kw):
        a = dict(u=P(y), v=P(x), B=B, A=O, Bc=C, L=L, T=T, K=K, s=s, p=p, mode=1, dw=P(dw), ws=P(ws))
        a.update(kw)
        return lib.adp_lt_wgrad(*a.values(), st)

    untouched = lambda: all(bool((t == SENTINEL).all()) for t in (y, xo, dw))  # noqa: E731
    for fn, ptrs, sizes in ((conv, ("x", "w", "y"), ("B", "C", "T", "O", "K", "s")),
                            (convt, ("x", "w", "out"), ("B", "C", "L", "O", "K", "s", "T")),
                            (wgrad, ("u", "v", "dw", "ws"), ("B", "A", "Bc", "L", "T", "K", "s"))):
        for k in ptrs:
            assert fn(**{k: None}) == ERR_NULL, (fn.__name__, k)
        for k in sizes:
            for bad in (0, -3):
                assert fn(**{k: bad}) == ERR_SHAPE, (fn.__name__, k, bad)
        assert fn(p=-1) == ERR_UNSUPPORTED, fn.__name__          # a negative padding
        assert fn(mode=2) == ERR_UNSUPPORTED, fn.__name__
    # a reflection needs pad < T
    assert conv(T=3, p=3, K=8) == ERR_SHAPE and conv(T=3, p=4, K=8) == ERR_SHAPE
    assert convt(T=2, p=2, L=1, K=4, s=4) == ERR_SHAPE
    assert wgrad(T=3, p=3, K=8, L=1) == ERR_SHAPE
    assert convt(T=T + 1, mode=0) == ERR_SHAPE and convt(L=L + 1) == ERR_SHAPE and wgrad(L=L + 1) == ERR_SHAPE
    assert lib.adp_lt_conv_out_len(T, K, s, p) == L and lib.adp_lt_convt_out_len(L, K, s, p) == T
    assert lib.adp_lt_conv_out_len(T, K, s, -1) == ERR_UNSUPPORTED and lib.adp_lt_convt_out_len(L, K, s, -1) == ERR_UNSUPPORTED
    assert lib.adp_lt_conv_out_len(0, K, s, p) == ERR_SHAPE and lib.adp_lt_conv_out_len(3, K, s, 1) == ERR_SHAPE
    assert lib.adp_lt_convt_out_len(0, K, s, p) == ERR_SHAPE and lib.adp_lt_convt_out_len(1, 2, 1, 3) == ERR_SHAPE
    assert lib.adp_lt_wgrad_ws_bytes(0, O, C, L, K) == ERR_SHAPE and lib.adp_lt_wgrad_ws_bytes(B, O, C, 0, K) == ERR_SHAPE
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert untouched(), "a refused call wrote to an output"
    assert conv() == 0 and convt() == 0 and wgrad() == 0
    assert not untouched()


# ------------------------------------------------------------------ 4. module contract
NET = dict(channels=[8, 32, 64], factors=[1, 4, 4], items=[1, 2, 2], modulation_features=128)


def test_module_contract():
    net = lt.LTPlugin(adp.UNetV0, num_filters=4, window_length=8, stride=4)(dim=1, in_channels=2, **NET)
    named = list(net.named_parameters())
    assert [n for n, _ in named[:2]] == ["encode.weight", "decode.weight"]
    assert all(n.startswith("net.") for n, _ in named[2:]) and len(named) > 2
    assert tuple(net.encode.weight.shape) == (8, 2, 8) and tuple(net.decode.weight.shape) == (8, 2, 8)
    assert isinstance(net.encode, nn.Conv1d) and isinstance(net.decode, nn.ConvTranspose1d)
    assert net.encode.padding_mode == "reflect" and net.encode.bias is None and net.decode.bias is None
    other = lt.LTPlugin(adp.UNetV0, num_filters=4, window_length=8, stride=4)(dim=1, in_channels=2, out_channels=3, **NET)
    assert tuple(other.decode.weight.shape) == (12, 3, 8)
    with pytest.raises(NotImplementedError, match="dim"):
        lt.LTPlugin(adp.UNetV0, num_filters=4, window_length=8, stride=4)(dim=2, in_channels=2, **NET)
    with pytest.raises(ValueError, match="negative"):
        lt.LTPlugin(adp.UNetV0, num_filters=4, window_length=2, stride=8)
    with pytest.raises(NotImplementedError, match="audio_diffusion_pytorch_amd.lt.LTPlugin"):
        adp.LTPlugin(adp.UNetV0, num_filters=4, window_length=8, stride=4)


def test_forward_checks_the_length(dev):
    net = lt.LTPlugin(adp.UNetV0, num_filters=4, window_length=8, stride=4)(dim=1, in_channels=2, **NET).to(dev)
    with pytest.raises(ValueError, match="does not survive"):
        net(torch.randn(1, 2, 4098).to(dev), torch.tensor([0.5]).to(dev))
    far = lt.LTPlugin(adp.UNetV0, num_filters=2, window_length=64, stride=8)(dim=1, in_channels=2, **NET).to(dev)
    with pytest.raises(ValueError, match="exceed"):
        far(torch.randn(1, 2, 24).to(dev), torch.tensor([0.5]).to(dev))
    with pytest.raises(ValueError, match="must be"):
        net(torch.randn(1, 3, 4096).to(dev), torch.tensor([0.5]).to(dev))


def test_plugin_nesting_with_append_channels():
    """LT(Append(UNetV0)): the appended tensor lives in the transformed domain and the U-Net reads it through its second
    pointer; Append(LT(UNetV0)): the LT module is no UNetV0Net, so the concat is the strided-copy pair."""
    inner = lt.LTPlugin(adp.AppendChannelsPlugin(adp.UNetV0, 3), num_filters=4, window_length=8, stride=4)(
        dim=1, in_channels=2, **NET)
    assert isinstance(inner.net, _AppendChannelsNet) and inner.net.two_pointer
    assert tuple(inner.encode.weight.shape) == (8, 2, 8)
    outer = adp.AppendChannelsPlugin(lt.LTPlugin(adp.UNetV0, num_filters=4, window_length=8, stride=4), 3)(
        dim=1, in_channels=2, **NET)
    assert isinstance(outer.net, lt.LTNet) and not outer.two_pointer
    assert tuple(outer.net.encode.weight.shape) == (20, 5, 8) and tuple(outer.net.decode.weight.shape) == (8, 2, 8)


# ------------------------------------------------------------------ 5. end to end against the CPU composition
class Composition(nn.Module):
    """The reference's module on CPU torch: Conv1d(reflect) -> oracle U-Net -> ConvTranspose1d."""

    def __init__(self, encode, decode, net):
        super().__init__()
        self.encode, self.decode, self.net = encode, decode, net

    def forward(self, x, *args, **kwargs):
        return self.decode(self.net(self.encode(x), *args, **kwargs))


@functools.lru_cache(maxsize=None)
def composition():
    """The CPU side of the end-to-end tests, computed once: module, inputs, loss, gradients, two sampler steps."""
    torch.manual_seed(0)
    oracle = UNetV0Oracle(in_channels=8, out_channels=8, **NET)
    encode = nn.Conv1d(2, 8, 8, stride=4, padding=2, padding_mode="reflect", bias=False)
    decode = nn.ConvTranspose1d(8, 2, 8, stride=4, padding=2, bias=False)
    ref = Composition(encode, decode, oracle)
    x, noise = torch.randn(2, 2, 4096), torch.randn(2, 2, 4096)
    sigmas = torch.tensor([0.25, 0.75])
    loss = ovd.v_loss(ref, x, noise, sigmas)
    loss.backward()
    sample = ovd.v_sample(ref, noise[:1], 2)
    return dict(ref=ref, x=x, noise=noise, sigmas=sigmas, loss=loss.detach(), sample=sample)


def build_model(c, dev, **kw):
    model = adp.DiffusionModel(net_t=lt.LTPlugin(adp.UNetV0, num_filters=4, window_length=8, stride=4), in_channels=2,
                               diffusion_sigma_distribution=FixedSigmas(c["sigmas"].tolist()), **NET, **kw)
    model.net.net.load_oracle_state_dict(c["ref"].net.state_dict())
    with torch.no_grad():
        model.net.encode.weight.copy_(c["ref"].encode.weight)
        model.net.decode.weight.copy_(c["ref"].decode.weight)
    return model.to(dev)


def grad_err(own, ref, gmax):
    """smoke()'s normalisation: the denominator is floored at 1e-3 x the largest gradient magnitude of the model."""
    return (own.detach().double().cpu() - ref.double()).abs().max().item() / max(ref.abs().max().item(), 1e-3 * gmax)


def test_training_step_and_sampler_match_the_composition(dev):
    c = composition()
    ref = c["ref"]
    model = build_model(c, dev)
    loss = model(c["x"].to(dev), noise=c["noise"].to(dev))
    loss.backward()
    rel = abs(loss.item() - c["loss"].item()) / abs(c["loss"].item())
    print(f"lt end to end: loss {loss.item():.6f} (composition {c['loss'].item():.6f}) rel {rel:.2e}")
    assert rel < PARITY_TOL
    gmax = max(p.grad.abs().max().item() for p in ref.parameters())
    errs = {"encode.weight": grad_err(model.net.encode.weight.grad, ref.encode.weight.grad, gmax),
            "decode.weight": grad_err(model.net.decode.weight.grad, ref.decode.weight.grad, gmax)}
    own = model.net.net.oracle_named_grads({n: p.grad for n, p in model.net.net.named_parameters()})
    for n, p in ref.net.named_parameters():
        errs["net." + n] = grad_err(own[n], p.grad, gmax)
    worst = max(errs, key=errs.get)
    print(f"lt end to end: encode {errs['encode.weight']:.2e} decode {errs['decode.weight']:.2e} worst {worst} {errs[worst]:.2e}")
    assert errs[worst] < PARITY_TOL, (worst, errs[worst])
    s = model.sample(c["noise"][:1].to(dev), num_steps=2)
    err = rel_err(s, c["sample"])
    print(f"lt end to end: two VSampler steps rel err {err:.2e}")
    assert err < PARITY_TOL


# ------------------------------------------------------------------ 6. input gradient
def test_input_gradient_matches_the_composition(dev):
    c = composition()
    ref = c["ref"]
    model = build_model(c, dev)
    g = torch.Generator().manual_seed(5)
    x, gout = torch.randn(2, 2, 256, generator=g), torch.randn(2, 2, 256, generator=g)
    xr = x.clone().requires_grad_()
    (ref(xr, c["sigmas"]) * gout).sum().backward()
    xd = x.to(dev).requires_grad_()
    (model.net(xd, c["sigmas"].to(dev)) * gout.to(dev)).sum().backward()
    err = rel_err(xd.grad, xr.grad)
    print(f"lt input gradient: rel err {err:.2e}")
    assert err < PARITY_TOL


def test_encode_data_gradient_is_not_launched_without_need(dev, monkeypatch):
    """In diffusion training the noised input does not require grad: no lt_convt(fold) launch in that backward."""
    calls = []
    real = ops.lt_convt
    monkeypatch.setattr(ops, "lt_convt", lambda *a, **k: (calls.append(a[4]), real(*a, **k))[1])
    conv = nn.Conv1d(2, 8, 8, stride=4, padding=2, padding_mode="reflect", bias=False).to(dev)
    x = torch.randn(1, 2, 64).to(dev)
    lt.lt_encode(x, conv).sum().backward()
    assert calls == [] and conv.weight.grad is not None
    lt.lt_encode(x.requires_grad_(), conv).sum().backward()
    assert calls == [ops.LT_FOLD] and x.grad is not None


# ------------------------------------------------------------------ 7. nesting with AppendChannelsPlugin, the wrappers
SMALL = dict(channels=[8, 16], factors=[2, 2], items=[1, 1], modulation_features=24)


def _tensors(seed, *shapes):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) for s in shapes]


def test_lt_around_append_channels_runs_in_the_transformed_domain(dev):
    """LTPlugin(AppendChannelsPlugin(UNetV0, 3)): forward and backward; the appended tensor has the frame length and reaches
    the U-Net through its second input pointer."""
    from oracle.a_unet_restatement import AppendChannelsOracle
    from test_unet import compare_grads
    torch.manual_seed(0)
    wrap = AppendChannelsOracle(lambda **kw: UNetV0Oracle(**kw), channels=3)(in_channels=8, out_channels=8, **SMALL)
    encode = nn.Conv1d(2, 8, 8, stride=4, padding=2, padding_mode="reflect", bias=False)
    decode = nn.ConvTranspose1d(8, 2, 8, stride=4, padding=2, bias=False)
    net = lt.LTPlugin(adp.AppendChannelsPlugin(adp.UNetV0, 3), num_filters=4, window_length=8, stride=4)(
        dim=1, in_channels=2, **SMALL)
    net.net.net.load_oracle_state_dict(wrap.net.state_dict())
    net.encode.load_state_dict(encode.state_dict())
    net.decode.load_state_dict(decode.state_dict())
    net = net.to(dev)
    x, extra, gout = _tensors(11, (2, 2, 256), (2, 3, 64), (2, 2, 256))
    t = torch.tensor([0.3, 0.8])
    ref = decode(wrap(encode(x), t, append_channels=extra))
    (ref * gout).sum().backward()
    out = net(x.to(dev), t.to(dev), append_channels=extra.to(dev))
    (out * gout.to(dev)).sum().backward()
    assert rel_err(out, ref) < PARITY_TOL
    assert rel_err(net.encode.weight.grad, encode.weight.grad) < PARITY_TOL
    assert rel_err(net.decode.weight.grad, decode.weight.grad) < PARITY_TOL
    compare_grads(net.net.net, wrap.net)
    with pytest.raises(ValueError, match="transformed domain"):   # an appended tensor of the SIGNAL's length
        net(x.to(dev), t.to(dev), append_channels=torch.randn(2, 3, 256).to(dev))


def test_upsampler_puts_append_channels_around_the_lt_module(dev):
    """DiffusionUpsampler(net_t=LTPlugin(UNetV0, ...)) = AppendChannelsPlugin(LTPlugin(UNetV0)): the concat is the strided
    copy pair in front of encode; the training loss and the transform's gradients against the CPU composition."""
    torch.manual_seed(0)
    oracle = UNetV0Oracle(in_channels=16, out_channels=8, **SMALL)
    encode = nn.Conv1d(4, 16, 8, stride=4, padding=2, padding_mode="reflect", bias=False)
    decode = nn.ConvTranspose1d(8, 2, 8, stride=4, padding=2, bias=False)
    ref = Composition(encode, decode, oracle)
    up = adp.DiffusionUpsampler(net_t=lt.LTPlugin(adp.UNetV0, num_filters=4, window_length=8, stride=4), in_channels=2,
                                upsample_factor=4, diffusion_sigma_distribution=FixedSigmas([0.4, 0.6]), **SMALL)
    assert isinstance(up.net, _AppendChannelsNet) and isinstance(up.net.net, lt.LTNet) and not up.net.two_pointer
    up.net.net.net.load_oracle_state_dict(oracle.state_dict())
    up.net.net.encode.load_state_dict(encode.state_dict())
    up.net.net.decode.load_state_dict(decode.state_dict())
    up = up.to(dev)
    x, noise = _tensors(5, (2, 2, 256), (2, 2, 256))
    low = ovd.upsample(ovd.downsample(x.clone(), 4), 4)
    loss_ref = ovd.v_loss(lambda xn, sg: ref(torch.cat([xn, low], dim=1), sg), x, noise, torch.tensor([0.4, 0.6]))
    loss_ref.backward()
    loss = up(x.to(dev), noise=noise.to(dev))
    loss.backward()
    assert abs(loss.item() - loss_ref.item()) < PARITY_TOL * abs(loss_ref.item())
    gmax = max(p.grad.abs().max().item() for p in ref.parameters())
    assert grad_err(up.net.net.encode.weight.grad, encode.weight.grad, gmax) < PARITY_TOL
    assert grad_err(up.net.net.decode.weight.grad, decode.weight.grad, gmax) < PARITY_TOL


def test_inpainter_runs_the_lt_module(dev):
    """VInpainter over an LT net: on the CPU build the seeded run equals the oracle's loop; on every device the kept region
    ends on the source (the last level is sigma = 0) and the result is finite."""
    torch.manual_seed(0)
    oracle = UNetV0Oracle(in_channels=8, out_channels=8, **SMALL)
    encode = nn.Conv1d(2, 8, 8, stride=4, padding=2, padding_mode="reflect", bias=False)
    decode = nn.ConvTranspose1d(8, 2, 8, stride=4, padding=2, bias=False)
    ref = Composition(encode, decode, oracle)
    net = lt.LTPlugin(adp.UNetV0, num_filters=4, window_length=8, stride=4)(dim=1, in_channels=2, **SMALL)
    net.net.load_oracle_state_dict(oracle.state_dict())
    net.encode.load_state_dict(encode.state_dict())
    net.decode.load_state_dict(decode.state_dict())
    net = net.to(dev)
    source, start = _tensors(9, (1, 2, 256), (1, 2, 256))
    mask = torch.zeros(1, 2, 256, dtype=torch.bool)
    mask[..., :128] = True
    torch.manual_seed(21)
    out = adp.VInpainter(net=net)(source.to(dev), mask.to(dev), num_steps=2, num_resamples=2, x_noisy=start.to(dev))
    assert out.shape == source.shape and torch.isfinite(out).all()
    assert rel_err(out[..., :128], source[..., :128]) < 1e-5
    if dev.type == "cpu":   # (the noise draws are torch's, per device)
        torch.manual_seed(21)
        want = ovd.v_inpaint(ref, source, mask, 2, 2, x_noisy=start)
        assert rel_err(out, want) < PARITY_TOL


# ------------------------------------------------------------------ 8. reference checkpoints
def test_reference_checkpoint_loader_accepts_the_lt_module():
    """components.load_reference_state_dict: the plugin's two tensors come first and are shape-checked, the rest goes down
    the positional path (UNVERIFIED offline like that loader: a_unet is not installable here)."""
    from audio_diffusion_pytorch_amd.components import load_reference_state_dict
    small = dict(channels=[8, 16], factors=[2, 2], items=[1, 1], modulation_features=24)
    torch.manual_seed(4)
    make = lambda: lt.LTPlugin(adp.UNetV0, num_filters=4, window_length=8, stride=4)(dim=1, in_channels=2, **small)  # noqa: E731
    dst, src = make(), make()
    core, order = src.net, src.net.a_unet_key_order()
    own = core.oracle_named_grads({n: p.detach() for n, p in core.named_parameters()})  # (name mapping only)
    key = lambda i, k: f"blocks.2.blocks.{i}." + ("weights" if k == "time_weights" else k.rsplit(".", 1)[-1])  # noqa: E731
    ckpt = dict([("blocks.0.weight", src.encode.weight.detach().clone()), ("blocks.1.weight", src.decode.weight.detach().clone())]
                + [(key(i, k), own[k].clone()) for i, k in enumerate(order)])
    keymap = load_reference_state_dict(dst, ckpt)
    assert keymap["blocks.0.weight"] == "encode.weight" and keymap["blocks.1.weight"] == "decode.weight"
    for (n, a), (_, b) in zip(dst.named_parameters(), src.named_parameters()):
        assert torch.equal(a, b), n
    wrong = dict(ckpt)
    wrong["blocks.1.weight"] = torch.zeros(8, 3, 8)
    with pytest.raises(ValueError, match="decode.weight"):
        load_reference_state_dict(make(), wrong)
    inside = adp.components.TextConditioningNet(make(), torch.nn.Identity())
    with pytest.raises(TypeError, match="around the whole UNetV0"):
        load_reference_state_dict(inside, ckpt)
