"""Autoregressive diffusion (ar.DiffusionAR) on the README U-Net layout at [B, 2, 2**18], num_splits = 8: ms per sampler step
(1 step = 1 U-Net forward + the update) and ms per training step (forward + backward), each three ways:

  replayed   the package's path, steps replayed from hipGraphs
  eager      the same kernels launched call by call (use_graph=False)
  baseline   what a user had to write before ar.py existed: the same native UNetV0 fed by torch.cat, with the reference's
             torch elementwise arithmetic around it (diffusion.py:118-130, :223-296 without its per-step host read),
             launched eagerly

The three are timed alternately, `--repeats` times each after a warm-up of every variant; the median and the extremes are
reported.  One JSON line on stdout; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time
from math import pi

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

SPLITS = 8


def baseline_sample(sampler, net, num_items, num_chunks, num_steps):
    """ARVSampler.forward as the reference writes it, on torch ops; `sampler` only supplies get_sigmas_ladder."""
    b, c, t, n, l = num_items, sampler.in_channels, sampler.length, sampler.num_splits, sampler.split_length
    dev = sampler.device

    def loop(current, sigmas):
        angle = sigmas * pi / 2
        alphas, betas = torch.cos(angle), torch.sin(angle)
        for i in range(sigmas.shape[0] - 1):
            v_pred = net(torch.cat([current, sigmas[i]], dim=1))
            x_pred = alphas[i] * current - betas[i] * v_pred
            noise_pred = betas[i] * current + alphas[i] * v_pred
            current = alphas[i + 1] * x_pred + betas[i + 1] * noise_pred
        return current

    with torch.no_grad():
        sigmas = torch.linspace(1, 0, num_steps + 1, device=dev)[:, None, None, None].expand(-1, b, 1, t)
        start = loop(torch.randn((b, c, t), device=dev) * sigmas[0], sigmas)
        if num_chunks == n:
            return start
        sigmas = sampler.get_sigmas_ladder(num_items=b, num_steps_per_split=num_steps // n)
        angle = sigmas[0] * pi / 2
        start = torch.cos(angle) * start + torch.sin(angle) * torch.randn_like(start)
        chunks = list(start.chunk(chunks=n, dim=-1))
        for _ in range(num_chunks):
            updated = loop(torch.cat(chunks[-n:], dim=-1), sigmas)
            chunks[-n:] = list(updated.chunk(chunks=n, dim=-1))
            chunks += [torch.randn((b, c, l), device=dev)]
        return torch.cat(chunks[:num_chunks], dim=-1)


def baseline_loss(net, x, n):
    """ARVDiffusion.forward as the reference writes it, on torch ops around the native net."""
    b, _, t = x.shape
    sigmas = torch.rand((b, 1, n), device=x.device, dtype=x.dtype).repeat_interleave(t // n, dim=-1)
    noise = torch.randn_like(x)
    angle = sigmas * pi / 2
    alphas, betas = torch.cos(angle), torch.sin(angle)
    x_noisy = alphas * x + betas * noise
    v_target = alphas * noise - betas * x
    return F.mse_loss(net(torch.cat([x_noisy, sigmas], dim=1)), v_target)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(ms, per):
    v = sorted(m / per for m in ms)
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4), "runs": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--num-steps", type=int, default=16)
    ap.add_argument("--num-chunks", type=int, default=12)
    ap.add_argument("--train-steps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--length", type=int, default=bench.LENGTH)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from audio_diffusion_pytorch_amd import UNetV0
    from audio_diffusion_pytorch_amd.ar import DiffusionAR
    assert torch.cuda.is_available(), "ar_bench measures on the MI355X only"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = DiffusionAR(net_t=UNetV0, in_channels=2, length=a.length, num_splits=SPLITS, channels=bench.CHANNELS,
                        factors=bench.FACTORS, items=bench.ITEMS).to(dev)
    evals = a.num_steps + (a.num_chunks * (a.num_steps // SPLITS) if a.num_chunks > SPLITS else 0)
    result = {"metric": "DiffusionAR, README U-Net layout", "length": a.length, "num_splits": SPLITS,
              "num_steps": a.num_steps, "num_chunks": a.num_chunks, "net_evaluations_per_sample_call": evals,
              "train_steps_per_run": a.train_steps, "batches": {}}

    def set_graph(flag):
        model.sampler.use_graph = model.diffusion.use_graph = flag

    for b in a.batches:
        x = torch.randn(b, 2, a.length, device=dev)

        def sample(flag):
            set_graph(flag)
            return model.sample(num_items=b, num_chunks=a.num_chunks, num_steps=a.num_steps)

        def train(flag, loss_of=None):
            set_graph(flag)
            for _ in range(a.train_steps):
                for p in model.parameters():
                    p.grad = None
                (model(x) if loss_of is None else loss_of()).backward()

        variants = {
            "sampler_replayed": (lambda: sample(True), evals),
            "sampler_eager": (lambda: sample(False), evals),
            "sampler_baseline": (lambda: baseline_sample(model.sampler, model.net, b, a.num_chunks, a.num_steps), evals),
            "train_replayed": (lambda: train(True), a.train_steps),
            "train_eager": (lambda: train(False), a.train_steps),
            "train_baseline": (lambda: train(False, lambda: baseline_loss(model.net, x, SPLITS)), a.train_steps),
        }
        for fn, _ in variants.values():  # warm-up of every variant: captures, allocator pools, code objects
            fn()
        times = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, (fn, _) in variants.items():
                times[k].append(timed(fn))
        out = {k: summary(times[k], variants[k][1]) for k in variants}
        out["sampler_graph_captures"] = model.sampler.graph_captures
        out["train_graph_captures"] = model.diffusion.train_graphs().captures
        out["finite"] = bool(torch.isfinite(sample(True)).all())
        result["batches"][str(b)] = out
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
