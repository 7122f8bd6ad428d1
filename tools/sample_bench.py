"""BASELINE config 3: VSampler.sample, num_steps=50, noise [B, 2, 2**18], inference only, one hipGraph-captured step
replayed per iteration.  Prints sampler steps/s (1 step = 1 U-Net forward + the rotation kernel).
--sampler multistep runs the same loop through VMultistepSampler (1 step = 1 U-Net forward + adp_v_step2).
--sampler threshold [--threshold q] [--order n] runs it through VThresholdSampler (1 step = 1 U-Net forward + the quantile
select of adp_clip_scale, five launches, for q > 0 + adp_clip_step).  --repeats N times the run N times in one process and
reports the median (every run is listed)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--graph", type=int, default=1)
    ap.add_argument("--sampler", choices=["v", "multistep", "threshold"], default="v")
    ap.add_argument("--threshold", type=float, default=0.995, help="--sampler threshold: dynamic_threshold (0 = static clamp)")
    ap.add_argument("--order", type=int, default=None, help="--sampler multistep / threshold: order (their default if unset)")
    ap.add_argument("--repeats", type=int, default=1)
    a = ap.parse_args()
    import audio_diffusion_pytorch_amd as adp
    sampler_t = {"v": adp.VSampler, "multistep": adp.VMultistepSampler, "threshold": adp.VThresholdSampler}[a.sampler]
    sampler_kw = {}
    if a.sampler == "threshold":
        sampler_kw["sampler_dynamic_threshold"] = a.threshold
    if a.order is not None and a.sampler != "v":
        sampler_kw["sampler_order"] = a.order
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = adp.DiffusionModel(net_t=adp.UNetV0, in_channels=2, channels=bench.CHANNELS, factors=bench.FACTORS,
                               items=bench.ITEMS, sampler_t=sampler_t, sampler_use_graph=bool(a.graph), **sampler_kw).to(dev)
    noise = torch.randn(a.batch, 2, bench.LENGTH).to(dev)
    model.sample(noise, num_steps=2)  # warm-up + graph capture
    times = []
    for _ in range(max(1, a.repeats)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.sample(noise, num_steps=a.steps)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    dt = sorted(times)[len(times) // 2]
    res = {"metric": f"sampler steps/s ({sampler_t.__name__}, UNetV0 forward only)",
           "value": round(a.steps / dt, 2),
           "ms_per_step": round(dt / a.steps * 1e3, 3), "batch": a.batch, "num_steps": a.steps,
           "launch": "hipGraph replay" if a.graph else "eager", "finite": bool(torch.isfinite(out).all())}
    if a.sampler != "v":
        res["sampler_kwargs"] = {k[len("sampler_"):]: v for k, v in sampler_kw.items()}
    if a.repeats > 1:
        res["ms_per_step_runs"] = [round(t / a.steps * 1e3, 3) for t in times]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
