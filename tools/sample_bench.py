"""BASELINE config 3: VSampler.sample, num_steps=50, noise [B, 2, 2**18], inference only, one hipGraph-captured step
replayed per iteration.  Prints sampler steps/s (1 step = 1 U-Net forward + the rotation kernel).
--sampler multistep runs the same loop through VMultistepSampler (1 step = 1 U-Net forward + adp_v_step2).
--sampler threshold [--threshold q] [--order n] runs it through VThresholdSampler (1 step = 1 U-Net forward + the quantile
select of adp_clip_scale, five launches, for q > 0 + adp_clip_step).  --sampler stochastic --eta E [--threshold q] runs it
through VStochasticSampler (1 step = 1 U-Net forward + adp_v_step_eta, its noise formed in the kernel; --threshold as for
`threshold`, none if unset) with a fixed seed.  --repeats N times the run N times in one process and reports the median
(every run is listed).  --also NAME ... measures further samplers on the same net in the same process, interleaved with the
first per repeat, one result line each (an A/B on one box: numbers of different boxes differ by a few percent)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


SAMPLERS = ["v", "multistep", "threshold", "stochastic"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--graph", type=int, default=1)
    ap.add_argument("--sampler", choices=SAMPLERS, default="v")
    ap.add_argument("--also", choices=SAMPLERS, nargs="*", default=[], help="further samplers, same net, same process")
    ap.add_argument("--threshold", type=float, default=None,
                    help="--sampler threshold / stochastic: dynamic_threshold (0 = static clamp; threshold's default 0.995)")
    ap.add_argument("--eta", type=float, default=1.0, help="--sampler stochastic: eta in [0, 1]")
    ap.add_argument("--order", type=int, default=None, help="--sampler multistep / threshold: order (their default if unset)")
    ap.add_argument("--repeats", type=int, default=1)
    a = ap.parse_args()
    import audio_diffusion_pytorch_amd as adp
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = adp.UNetV0(dim=1, in_channels=2, channels=bench.CHANNELS, factors=bench.FACTORS, items=bench.ITEMS).to(dev)
    noise = torch.randn(a.batch, 2, bench.LENGTH).to(dev)
    names = [a.sampler] + list(a.also)
    samplers, kwargs, run_kw = [], [], []
    for name in names:
        sampler_t = {"v": adp.VSampler, "multistep": adp.VMultistepSampler, "threshold": adp.VThresholdSampler,
                     "stochastic": adp.VStochasticSampler}[name]
        kw = {}
        if name == "threshold":
            kw["dynamic_threshold"] = 0.995 if a.threshold is None else a.threshold
        if name == "stochastic":
            kw["eta"] = a.eta
            if a.threshold is not None:
                kw["dynamic_threshold"] = a.threshold
        if a.order is not None and name in ("multistep", "threshold"):
            kw["order"] = a.order
        samplers.append(sampler_t(net=net, use_graph=bool(a.graph), **kw))
        kwargs.append(kw)
        run_kw.append({"seed": 0} if name == "stochastic" else {})
    with torch.no_grad():
        for s, rk in zip(samplers, run_kw):
            s(noise, num_steps=2, **rk)  # warm-up + graph capture
        times = [[] for _ in samplers]
        outs = [None] * len(samplers)
        for _ in range(max(1, a.repeats)):
            for k, (s, rk) in enumerate(zip(samplers, run_kw)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[k] = s(noise, num_steps=a.steps, **rk)
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
    for name, s, kw, ts, out in zip(names, samplers, kwargs, times, outs):
        dt = sorted(ts)[len(ts) // 2]
        res = {"metric": f"sampler steps/s ({type(s).__name__}, UNetV0 forward only)",
               "value": round(a.steps / dt, 2),
               "ms_per_step": round(dt / a.steps * 1e3, 3), "batch": a.batch, "num_steps": a.steps,
               "launch": "hipGraph replay" if a.graph else "eager", "finite": bool(torch.isfinite(out).all())}
        if name != "v":
            res["sampler_kwargs"] = kw
        if a.repeats > 1:
            res["ms_per_step_runs"] = [round(t / a.steps * 1e3, 3) for t in ts]
        print(json.dumps(res))


if __name__ == "__main__":
    main()
