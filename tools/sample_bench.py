"""BASELINE config 3: VSampler.sample, num_steps=50, noise [B, 2, 2**18], inference only, one hipGraph-captured step
replayed per iteration.  Prints sampler steps/s (1 step = 1 U-Net forward + the rotation kernel).
--sampler multistep runs the same loop through VMultistepSampler (1 step = 1 U-Net forward + adp_v_step2).
--sampler threshold [--threshold q] [--order n] runs it through VThresholdSampler (1 step = 1 U-Net forward + the quantile
select of adp_clip_scale, five launches, for q > 0 + adp_clip_step).  --sampler stochastic --eta E [--threshold q] runs it
through VStochasticSampler (1 step = 1 U-Net forward + adp_v_step_eta, its noise formed in the kernel; --threshold as for
`threshold`, none if unset) with a fixed seed.  --repeats N times the run N times in one process and reports the median
(every run is listed).  --also NAME ... measures further samplers on the same net in the same process, interleaved with the
first per repeat, one result line each (an A/B on one box: numbers of different boxes differ by a few percent).
--sampler rf [--order n] [--threshold q] runs it through RFSampler (rectified flow: 1 step = 1 U-Net forward + adp_rf_step,
behind the quantile select for q > 0); `vsampler` is another name of `v`.  --train N times the replayed training step instead:
RFDiffusion against VDiffusion on the same net shape, N steps each per repeat, interleaved.  --kernels N times the update
kernels alone (adp_rf_step order 1 / 2 against adp_v_step / adp_v_step2, adp_rf_noise against adp_v_noise) from the library's
own per-launch event pairs, N launches each, median.
--sampler k [--order n] [--k-eta E] [--threshold q] runs it through KSampler (Karras / EDM: 1 step = 1 U-Net forward +
adp_edm_step, behind the quantile select for q > 0) on KarrasSchedule(0.002, 80); --train and --kernels list KDiffusion and
the adp_edm_* kernels next to the others.
--sampler repaint-v | repaint-rf | repaint-k [--resamples R] [--threshold q] runs the RePaint inpainters (VRepainter,
RFRepainter, KRepainter: 1 resample = 1 U-Net forward + adp_repaint_*_step, behind the quantile select for q > 0) on a
continuation mask (the first half known), --steps steps of R resamples each, and reports ms per resample; `inpaint` is
VInpainter(noise="philox", use_graph=True) on the same problem, for an A/B through --also.  --kernels lists the
adp_repaint_*_step kernels next to adp_v_inpaint_step_rng."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


INPAINTERS = ["repaint-v", "repaint-rf", "repaint-k", "inpaint"]
SAMPLERS = ["v", "vsampler", "multistep", "threshold", "stochastic", "rf", "k"] + INPAINTERS


def train_bench(a, adp, dev):
    """Replayed training steps (loss = model(x); loss.backward()) of RFDiffusion, KDiffusion and VDiffusion, interleaved per
    repeat."""
    models = {}
    for name, diffusion_t in (("RFDiffusion", adp.RFDiffusion), ("KDiffusion", adp.KDiffusion), ("VDiffusion", adp.VDiffusion)):
        torch.manual_seed(0)
        models[name] = adp.DiffusionModel(net_t=adp.UNetV0, in_channels=2, channels=bench.CHANNELS, factors=bench.FACTORS,
                                          items=bench.ITEMS, diffusion_t=diffusion_t).to(dev)
    x = torch.randn(a.batch, 2, bench.LENGTH, device=dev)

    def steps(m, n):
        for _ in range(n):
            for p in m.parameters():
                p.grad = None
            m(x).backward()

    for m in models.values():
        steps(m, 3)  # warm-up + capture
    times = {name: [] for name in models}
    for _ in range(max(1, a.repeats)):
        for name, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(m, a.train)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.train)
    for name, m in models.items():
        ts = times[name]
        graphs = m.diffusion.train_graphs()
        print(json.dumps({"metric": f"training step ms ({name}, replayed)", "value": round(sorted(ts)[len(ts) // 2] * 1e3, 3),
                          "batch": a.batch, "steps": a.train, "captures": graphs.captures, "replays": graphs.replays,
                          "ms_per_step_runs": [round(t * 1e3, 3) for t in ts]}))


def kernel_bench(a, adp, dev):
    """The update kernels alone, from the event pair the library records around each launch while profiling."""
    from audio_diffusion_pytorch_amd import _C, ops
    g = torch.Generator().manual_seed(0)
    x, u, h1, h2 = [torch.randn(a.batch, 2, bench.LENGTH, generator=g).to(dev) for _ in range(4)]
    out, o1, o2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    t = torch.rand(a.batch, generator=g).to(dev)
    row6 = ops.rf_table(torch.tensor([0.62, 0.55, 0.5]))[1].to(dev)
    ab4, ab6 = torch.rand(4, generator=g).to(dev), torch.rand(6, generator=g).to(dev)
    k2, k_eta = ops.edm_table([80.0, 0.5, 0.002, 0.0])[1].to(dev), ops.edm_table([80.0, 0.5, 0.002, 0.0], order=1, eta=1.0)[1].to(dev)
    rng, sigma = ops.rng_rows(0, [1])[0].to(dev), torch.rand(a.batch, generator=g).to(dev) + 0.1
    half = torch.zeros(a.batch, 2, bench.LENGTH, dtype=torch.uint8, device=dev)
    half[..., :bench.LENGTH // 2] = 1   # (continuation: the first half keeps the source)
    calls = {
        "adp_rf_step order 1": lambda: ops.rf_step(x, u, row6, out=out),
        "adp_v_step": lambda: ops.v_step(x, u, ab4, out=out),
        "adp_rf_step order 2": lambda: ops.rf_step(x, u, row6, order=2, hist=h1, out=out, hist_out=o1),
        "adp_v_step2": lambda: ops.v_step2(x, u, h1, h2, ab6, out=out, hist_x0_out=o1, hist_eps_out=o2),
        "adp_rf_step order 1 static clamp": lambda: ops.rf_step(x, u, row6, clip=True, out=out),
        "adp_rf_noise": lambda: ops.rf_noise(x, u, t, x_t_out=o1, u_out=o2),
        "adp_v_noise": lambda: ops.v_noise(x, u, t),
        "adp_edm_step order 1": lambda: ops.edm_step(x, u, k2, out=out),
        "adp_edm_step order 2": lambda: ops.edm_step(x, u, k2, order=2, hist=h1, out=out, hist_out=o1),
        "adp_edm_step order 1 eta 1": lambda: ops.edm_step(x, u, k_eta, rng, out=out),
        "adp_v_step_eta": lambda: ops.v_step_eta(x, u, ab6[:5], rng, out=out),
        "adp_edm_noise": lambda: ops.edm_noise(x, u, sigma, 0.5, x_in_out=o1, target_out=o2),
        "adp_v_inpaint_step_rng": lambda: ops.v_inpaint_step_rng(x, u, h1, half, ab4, rng, out=out),
    }
    for obj, levels in (("v", [0.62, 0.55, 0.5]), ("rf", [0.62, 0.55, 0.5]), ("k", [80.0, 0.5, 0.002])):
        table = ops.repaint_table(obj, torch.tensor(levels), 2).to(dev)
        for kind, row in (("jump", table[0]), ("move on", table[1])):
            calls[f"adp_repaint_{obj}_step {kind}"] = lambda obj=obj, row=row: ops.repaint_step(obj, x, u, h1, half, row, rng, out=out)
    static_row = ops.repaint_table("v", torch.tensor([0.62, 0.55]), 2)[0].to(dev)
    calls["adp_repaint_v_step jump static clamp"] = lambda: ops.repaint_step("v", x, u, h1, half, static_row, rng, clip=True, out=out)
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(a.kernels):
        for name, fn in calls.items():
            _C.PROFILE = []
            fn()
            times[name] += [ms for _, _, _, ms in _C.profile_collect()]
    for name, ts in times.items():
        ts = sorted(ts)
        print(json.dumps({"metric": f"kernel us ({name})", "value": round(ts[len(ts) // 2] * 1e3, 2),
                          "min": round(ts[0] * 1e3, 2), "launches": len(ts), "shape": [a.batch, 2, bench.LENGTH]}))


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
    ap.add_argument("--k-eta", type=float, default=0.0, help="--sampler k: eta in [0, 1] (eta > 0 needs --order 1)")
    ap.add_argument("--order", type=int, default=None,
                    help="--sampler multistep / threshold / rf / k: order (their default if unset)")
    ap.add_argument("--resamples", type=int, default=4, help="--sampler repaint-* / inpaint: num_resamples")
    ap.add_argument("--train", type=int, default=0,
                    help="time N replayed training steps of RFDiffusion, KDiffusion and VDiffusion instead")
    ap.add_argument("--kernels", type=int, default=0, help="time N launches of each update kernel alone instead")
    ap.add_argument("--repeats", type=int, default=1)
    a = ap.parse_args()
    import audio_diffusion_pytorch_amd as adp
    dev = torch.device("cuda:0")
    if a.train or a.kernels:
        return (train_bench if a.train else kernel_bench)(a, adp, dev)
    torch.manual_seed(0)
    net = adp.UNetV0(dim=1, in_channels=2, channels=bench.CHANNELS, factors=bench.FACTORS, items=bench.ITEMS).to(dev)
    noise = torch.randn(a.batch, 2, bench.LENGTH).to(dev)
    names = [a.sampler] + list(a.also)
    samplers, kwargs, run_kw = [], [], []
    for name in names:
        if name in INPAINTERS:
            kw = {} if a.threshold is None or name == "inpaint" else {"dynamic_threshold": a.threshold}
            if name == "inpaint":
                samplers.append(adp.VInpainter(net=net, noise="philox", use_graph=bool(a.graph)))
            elif name == "repaint-k":
                samplers.append(adp.KRepainter(net=net, schedule=adp.KarrasSchedule(0.002, 80.0), use_graph=bool(a.graph), **kw))
            else:
                cls = adp.VRepainter if name == "repaint-v" else adp.RFRepainter
                samplers.append(cls(net=net, use_graph=bool(a.graph), **kw))
            kwargs.append(kw)
            run_kw.append({"seed": 0})
            continue
        sampler_t = {"v": adp.VSampler, "vsampler": adp.VSampler, "multistep": adp.VMultistepSampler,
                     "threshold": adp.VThresholdSampler, "stochastic": adp.VStochasticSampler, "rf": adp.RFSampler, "k": adp.KSampler}[name]
        kw = {}
        if name == "threshold":
            kw["dynamic_threshold"] = 0.995 if a.threshold is None else a.threshold
        if name == "stochastic":
            kw["eta"] = a.eta
            if a.threshold is not None:
                kw["dynamic_threshold"] = a.threshold
        if name in ("rf", "k") and a.threshold is not None:
            kw["dynamic_threshold"] = a.threshold
        if name == "k":
            kw.update(schedule=adp.KarrasSchedule(0.002, 80.0), eta=a.k_eta)
        if a.order is not None and name in ("multistep", "threshold", "rf", "k"):
            kw["order"] = a.order
        samplers.append(sampler_t(net=net, use_graph=bool(a.graph), **kw))
        kwargs.append(kw)
        run_kw.append({"seed": 0} if name in ("stochastic", "k") else {})
    known = torch.zeros(a.batch, 2, bench.LENGTH, dtype=torch.bool, device=dev)
    known[..., :bench.LENGTH // 2] = True   # (continuation of a clip: the first half keeps the source)

    def run(name, s, steps, rk):
        if name in INPAINTERS:
            return s(noise, known, num_steps=steps, num_resamples=a.resamples, **rk)
        return s(noise, num_steps=steps, **rk)

    with torch.no_grad():
        for name, s, rk in zip(names, samplers, run_kw):
            run(name, s, 2, rk)  # warm-up + graph capture
        times = [[] for _ in samplers]
        outs = [None] * len(samplers)
        for _ in range(max(1, a.repeats)):
            for k, (name, s, rk) in enumerate(zip(names, samplers, run_kw)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[k] = run(name, s, a.steps, rk)
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
    for name, s, kw, ts, out in zip(names, samplers, kwargs, times, outs):
        dt = sorted(ts)[len(ts) // 2]
        if name in INPAINTERS:
            n = a.steps * a.resamples
            res = {"metric": f"inpainter resamples/s ({type(s).__name__}, UNetV0 forward only)", "value": round(n / dt, 2),
                   "ms_per_resample": round(dt / n * 1e3, 3), "batch": a.batch, "num_steps": a.steps,
                   "num_resamples": a.resamples, "launch": "hipGraph replay" if a.graph else "eager",
                   "finite": bool(torch.isfinite(out).all()), "inpainter_kwargs": kw}
            if a.repeats > 1:
                res["ms_per_resample_runs"] = [round(t / n * 1e3, 3) for t in ts]
            print(json.dumps(res))
            continue
        res = {"metric": f"sampler steps/s ({type(s).__name__}, UNetV0 forward only)",
               "value": round(a.steps / dt, 2),
               "ms_per_step": round(dt / a.steps * 1e3, 3), "batch": a.batch, "num_steps": a.steps,
               "launch": "hipGraph replay" if a.graph else "eager", "finite": bool(torch.isfinite(out).all())}
        if name not in ("v", "vsampler"):
            res["sampler_kwargs"] = {k: v for k, v in kw.items() if k != "schedule"}
        if a.repeats > 1:
            res["ms_per_step_runs"] = [round(t / a.steps * 1e3, 3) for t in ts]
        print(json.dumps(res))


if __name__ == "__main__":
    main()
