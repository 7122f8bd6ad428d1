"""The learned-transform front end on the GPU at [4, 2, 2**18], num_filters=128, window_length=64, stride=32: each of the five
launches of a training step (encode forward, decode forward, decode data gradient, both weight gradients) against
F.pad(reflect) + F.conv1d / F.conv_transpose1d and their autograd in the same process, and the replayed training step of an LT
model next to the plain model whose U-Net has the same inner shape ([4, 256, 8192]; its own first and last convs take the
place of the transform).  Medians over --reps repeats with the min-max spread.  Prints one JSON object.
usage: python tools/lt_bench.py [--steps K] [--reps R]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import audio_diffusion_pytorch_amd as adp  # noqa: E402
from audio_diffusion_pytorch_amd import ops  # noqa: E402
from audio_diffusion_pytorch_amd.lt import LTPlugin  # noqa: E402
from vocoder_bench import cuda_us, step_ms  # noqa: E402

SHAPE = (4, 2, 2 ** 18)
LT = dict(num_filters=128, window_length=64, stride=32)
NET = dict(channels=[256, 512, 512, 1024, 1024], factors=[1, 2, 2, 2, 2], items=[2, 2, 2, 4, 4])  # the README example
F32_MFMA_PEAK_TFLOPS = 157.3   # MI355X: 256 CUs x 256 flop / clock (v_mfma_f32_32x32x2_f32) x 2.4 GHz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    B, C, T = SHAPE
    Fn, W, s = LT["num_filters"], LT["window_length"], LT["stride"]
    p = W // 2 - s // 2
    L = (T + 2 * p - W) // s + 1
    x, we, wd = r(B, C, T), r(C * Fn, C, W) / (C * W) ** 0.5, r(C * Fn, C, W) / (C * Fn) ** 0.5
    y, gy, go = r(B, C * Fn, L), r(B, C * Fn, L), r(B, C, T)
    res = {"shape": list(SHAPE), **LT, "frames": L}

    native = {
        "encode_fwd": lambda: ops.lt_conv(x, we, s, p, ops.LT_REFLECT),
        "decode_fwd": lambda: ops.lt_convt(y, wd, s, p, ops.LT_PLAIN),
        "decode_dgrad": lambda: ops.lt_conv(go, wd, s, p, ops.LT_ZERO),
        "encode_wgrad": lambda: ops.lt_wgrad(gy, x, W, s, p, ops.LT_REFLECT),
        "decode_wgrad": lambda: ops.lt_wgrad(y, go, W, s, p, ops.LT_ZERO),
    }
    weg, wdg, yg = we.clone().requires_grad_(), wd.clone().requires_grad_(), y.clone().requires_grad_()
    enc_out = F.conv1d(F.pad(x, (p, p), mode="reflect"), weg, stride=s)
    dec_out = F.conv_transpose1d(yg, wdg, stride=s, padding=p)
    stock = {
        "encode_fwd": lambda: F.conv1d(F.pad(x, (p, p), mode="reflect"), we, stride=s),
        "decode_fwd": lambda: F.conv_transpose1d(y, wd, stride=s, padding=p),
        "decode_dgrad": lambda: torch.autograd.grad(dec_out, yg, go, retain_graph=True),
        "encode_wgrad": lambda: torch.autograd.grad(enc_out, weg, gy, retain_graph=True),
        "decode_wgrad": lambda: torch.autograd.grad(dec_out, wdg, go, retain_graph=True),
    }
    unwrap = lambda v: v[0] if isinstance(v, tuple) else v  # noqa: E731
    for name in native:
        a, b = native[name](), unwrap(stock[name]())
        res[name + "_rel_diff_vs_torch"] = float((a - b).abs().max() / b.abs().max())
        res[name + "_native_us"] = cuda_us(native[name], args.reps)
        res[name + "_torch_us"] = cuda_us(stock[name], args.reps)
    flops = 2.0 * B * L * (C * Fn) * (C * W)
    res["encode_fwd_tflops"] = round(flops / res["encode_fwd_native_us"]["median"] * 1e-6, 2)
    res["encode_fwd_fraction_of_f32_mfma_peak"] = round(res["encode_fwd_tflops"] / F32_MFMA_PEAK_TFLOPS, 4)
    del enc_out, dec_out

    torch.manual_seed(0)
    model = adp.DiffusionModel(net_t=LTPlugin(adp.UNetV0, **LT), in_channels=C, **NET).to(dev)
    res["lt_step_replayed_ms"] = step_ms(model, x, args.steps, args.reps)
    tg = model.diffusion.train_graphs()
    res["captures"], res["replays"] = tg.captures, tg.replays
    del model
    torch.cuda.empty_cache()
    torch.manual_seed(0)
    plain = adp.DiffusionModel(net_t=adp.UNetV0, in_channels=C * Fn, **NET).to(dev)
    res["plain_step_replayed_ms"] = step_ms(plain, r(B, C * Fn, L), args.steps, args.reps)
    res["lt_minus_plain_us"] = round((res["lt_step_replayed_ms"]["median"] - res["plain_step_replayed_ms"]["median"]) * 1e3, 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
