"""Multi-resolution STFT loss on the GPU (default resolutions at [4, 2, 2**18]): the native loss (adp_stft_loss_*) against
the same contract written with torch.stft (hipFFT), and the replayed training step of the bench model with F.mse_loss,
with the native loss and with the torch.stft loss (whether graphed.py captures that one).  Prints one JSON object.
usage: python tools/stft_loss_bench.py [--steps K]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.randn(*SHAPE, device=dev, generator=g)
    x = y + 0.3 * torch.randn(*SHAPE, device=dev, generator=g)
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
