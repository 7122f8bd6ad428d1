"""Multi-resolution STFT loss on the GPU (default resolutions at [4, 2, 2**18]): the native loss (adp_stft_loss_*) against
the same contract written with torch.stft (hipFFT), and the replayed training step of the bench model with F.mse_loss,
with the native loss and with the torch.stft loss (whether graphed.py captures that one).  Prints one JSON object.
--mode stereo measures the losses of spectral.py at the same shape instead: (a) the sum/difference loss in one native call
against the two-call form (torch sum and difference, then losses.MultiResolutionSTFTLoss twice), alternating the two in one
process, forward, backward and the replayed step; (b) the mel loss, and mel + A-weighting + sum/difference, against the same
loss on torch.stft.
usage: python tools/stft_loss_bench.py [--steps K] [--mode default|stereo]"""
import argparse
import json
import os
import sys
import time
import warnings

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_diffusion_pytorch_amd as adp  # noqa: E402
from audio_diffusion_pytorch_amd import graphed, ops  # noqa: E402
from audio_diffusion_pytorch_amd import spectral  # noqa: E402
from audio_diffusion_pytorch_amd.losses import MultiResolutionSTFTLoss  # noqa: E402

SHAPE = (4, 2, 2 ** 18)
CHANNELS = [8, 32, 64, 128, 256, 512, 512, 1024, 1024]  # bench.py's model
FACTORS = [1, 4, 4, 4, 2, 2, 2, 2, 2]
ITEMS = [1, 2, 2, 2, 2, 2, 2, 4, 4]


class TorchSTFTLoss(torch.nn.Module):
    """The losses.py contract on torch.stft: what a user brings when auraloss is absent."""

    def __init__(self, res=((1024, 120, 600), (2048, 240, 1200), (512, 50, 240)), eps=1e-8):
        super().__init__()
        self.res, self.eps = res, eps

    def forward(self, x, y):
        L = x.shape[-1]
        x, y = x.reshape(-1, L), y.reshape(-1, L)
        total = 0.0
        for N, h, W in self.res:
            win = torch.hann_window(W, device=x.device)
            mx, my = (torch.sqrt(torch.clamp(s.real ** 2 + s.imag ** 2, min=self.eps)) for s in
                      (torch.stft(v, N, h, W, win, center=True, pad_mode="reflect", return_complex=True) for v in (x, y)))
            total = total + torch.linalg.vector_norm(my - mx) / torch.linalg.vector_norm(my) + \
                (torch.log(mx) - torch.log(my)).abs().mean()
        return total / len(self.res)


class TwoCallSumDiff(torch.nn.Module):
    """Sum/difference without spectral.py: torch forms the two tensors, the native loss runs twice."""

    def __init__(self):
        super().__init__()
        self.loss = MultiResolutionSTFTLoss()

    def forward(self, x, y):
        xs, xd, ys, yd = x[:, :1] + x[:, 1:], x[:, :1] - x[:, 1:], y[:, :1] + y[:, 1:], y[:, :1] - y[:, 1:]
        return (self.loss(xs, ys) + self.loss(xd, yd)) / 2


class TorchSpectralLoss(torch.nn.Module):
    """The spectral.py contract on torch.stft: mel filterbank, optional FIR pre-filter, optional sum/difference."""

    def __init__(self, sample_rate, n_bins, taps=None, pair=False, res=TorchSTFTLoss().res, eps=1e-8):
        super().__init__()
        self.res, self.eps, self.pair = res, eps, pair
        for i, (N, _, _) in enumerate(res):
            self.register_buffer(f"fb{i}", spectral.mel_filterbank(sample_rate, N, n_bins).float())
        self.register_buffer("taps", None if taps is None else taps.view(1, 1, -1))

    def forward(self, x, y):
        L = x.shape[-1]

        def groups(v):
            gs = [v[:, 0] + v[:, 1], v[:, 0] - v[:, 1]] if self.pair else [v.reshape(-1, L)]
            if self.taps is not None:
                gs = [F.conv1d(g[:, None], self.taps, padding=self.taps.shape[-1] // 2)[:, 0] for g in gs]
            return gs
        values = []
        for xg, yg in zip(groups(x), groups(y)):
            total = 0.0
            for i, (N, h, W) in enumerate(self.res):
                win = torch.hann_window(W, device=x.device)
                fb = getattr(self, f"fb{i}")
                mx, my = (fb @ torch.sqrt(torch.clamp(s.real ** 2 + s.imag ** 2, min=self.eps)) for s in
                          (torch.stft(v, N, h, W, win, center=True, pad_mode="reflect", return_complex=True)
                           for v in (xg, yg)))
                total = total + torch.linalg.vector_norm(my - mx) / torch.linalg.vector_norm(my) + \
                    (torch.log(mx) - torch.log(my)).abs().mean()
            values.append(total / len(self.res))
        return sum(values) / len(values)


def cuda_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def loss_times(crit, x, y, reps):
    """(forward us, backward us) of crit at x, y."""
    xg = x.clone().requires_grad_(True)
    with torch.no_grad():
        fwd = cuda_ms(lambda: crit(x, y), reps)

    def step():
        xg.grad = None
        crit(xg, y).backward()
    return fwd * 1e3, (cuda_ms(step, reps) - fwd) * 1e3


def step_ms(loss_fn, steps, dev):
    torch.manual_seed(0)
    model = adp.DiffusionModel(net_t=adp.UNetV0, in_channels=2, channels=CHANNELS, factors=FACTORS, items=ITEMS,
                               loss_fn=loss_fn).to(dev)
    x = torch.randn(*SHAPE, device=dev)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in range(3):
            model(x).backward()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            model(x).backward()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
    g = graphed.GRAPHS_OF.get(model.diffusion)
    out = {"step_ms": round(ms, 3), "captures": g.captures if g else 0, "replays": g.replays if g else 0,
           "eager_only": bool(g and g.eager_only)}
    warn = [str(w.message) for w in caught if "graph capture" in str(w.message)]
    if warn:
        out["capture_warning"] = warn[0][:300]
    del model
    torch.cuda.empty_cache()
    return out


def stereo(args, dev, x, y):
    """(a) one native sum/difference call against the two-call form, alternating, medians of `rounds`; (b) mel modes."""
    res = {"shape": list(SHAPE), "mode": "stereo", "sample_rate": 44100, "n_bins": 64}
    one, two = spectral.SumAndDifferenceSTFTLoss().to(dev), TwoCallSumDiff().to(dev)
    la, lb = one(x, y).item(), two(x, y).item()
    res["loss_one_call"], res["loss_two_calls"] = la, lb
    times = {"one_call": [], "two_calls": []}
    for _ in range(args.rounds):
        for name, crit in (("one_call", one), ("two_calls", two)):
            times[name].append(loss_times(crit, x, y, args.reps))
    med = lambda v: sorted(v)[len(v) // 2]
    for name, t in times.items():
        f, b = med([a for a, _ in t]), med([c for _, c in t])
        res[f"sumdiff_{name}_us"] = {"fwd": round(f, 1), "bwd": round(b, 1), "fwd_bwd": round(f + b, 1),
                                     "fwd_bwd_min_max": [round(min(a + c for a, c in t), 1), round(max(a + c for a, c in t), 1)]}
    kw = dict(scale="mel", sample_rate=44100, n_bins=64)
    taps = spectral.a_weighting_fir(44100)
    for name, native, ref in (("mel", spectral.MultiResolutionSTFTLoss(**kw), TorchSpectralLoss(44100, 64)),
                              ("mel_aw_sumdiff", spectral.SumAndDifferenceSTFTLoss(perceptual_weighting=True, **kw),
                               TorchSpectralLoss(44100, 64, taps, True))):
        native, ref = native.to(dev), ref.to(dev)
        nf, nb = loss_times(native, x, y, args.reps)
        tf, tb = loss_times(ref, x, y, max(2, args.reps // 4))
        res[f"{name}_native_us"] = {"fwd": round(nf, 1), "bwd": round(nb, 1), "fwd_bwd": round(nf + nb, 1)}
        res[f"{name}_torch_stft_us"] = {"fwd": round(tf, 1), "bwd": round(tb, 1), "fwd_bwd": round(tf + tb, 1)}
        res[f"loss_{name}_native"], res[f"loss_{name}_torch_stft"] = native(x, y).item(), ref(x, y).item()
    del one, two, native, ref
    torch.cuda.empty_cache()
    steps = {"step_sumdiff_one_call": [], "step_sumdiff_two_calls": []}
    for _ in range(2):   # alternating
        steps["step_sumdiff_one_call"].append(step_ms(spectral.SumAndDifferenceSTFTLoss(), args.steps, dev))
        steps["step_sumdiff_two_calls"].append(step_ms(TwoCallSumDiff(), args.steps, dev))
    for name, runs in steps.items():
        res[name] = dict(runs[-1], step_ms=min(r["step_ms"] for r in runs), step_ms_runs=[r["step_ms"] for r in runs])
    res["step_mel_aw_sumdiff"] = step_ms(spectral.SumAndDifferenceSTFTLoss(perceptual_weighting=True, **kw), args.steps, dev)
    res["step_mse"] = step_ms(F.mse_loss, args.steps, dev)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mode", choices=("default", "stereo"), default="default")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.randn(*SHAPE, device=dev, generator=g)
    x = y + 0.3 * torch.randn(*SHAPE, device=dev, generator=g)
    if args.mode == "stereo":
        return stereo(args, dev, x, y)
    native, ref = MultiResolutionSTFTLoss(), TorchSTFTLoss()
    res = {"shape": list(SHAPE), "resolutions": [list(r) for r in native.resolutions]}
    nf, nb = loss_times(native, x, y, args.reps)
    tf, tb = loss_times(ref, x, y, args.reps)
    res["native_us"] = {"fwd": round(nf, 1), "bwd": round(nb, 1), "fwd_bwd": round(nf + nb, 1)}
    res["torch_stft_us"] = {"fwd": round(tf, 1), "bwd": round(tb, 1), "fwd_bwd": round(tf + tb, 1)}
    res["loss_native"], res["loss_torch_stft"] = native(x, y).item(), ref(x, y).item()
    loss, ws = ops.stft_loss_fwd(x, y, native.resolutions, 1.0, 1.0, 0.0, 1e-8)
    loss2, _ = ops.stft_loss_fwd(x, y, native.resolutions, 1.0, 1.0, 0.0, 1e-8)
    res["deterministic_fwd"] = bool(torch.equal(loss, loss2))
    res["step_mse"] = step_ms(F.mse_loss, args.steps, dev)
    res["step_native_stft"] = step_ms(MultiResolutionSTFTLoss(), args.steps, dev)
    res["step_torch_stft"] = step_ms(TorchSTFTLoss(), args.steps, dev)
    res["native_minus_mse_ms"] = round(res["step_native_stft"]["step_ms"] - res["step_mse"]["step_ms"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
