"""What the tail of a training step costs on the headline net: torch's clip_grad_norm_ + AdamW + EMA lerp against the
fused optim.AdamW (adp_sqnorm_partials + adp_adamw_step), and the README loop with either.

    python tools/optim_bench.py [--reps 30] [--out profiles/optim_bench.json]

One process, bench.py's headline configuration ([4,2,2**18], 176 M parameters), gradients produced by one real (replayed)
backward so that they are the slices of the flat gradient buffer the optimizer sees in training.  Every leg is warmed up,
timed with device events over `--reps` repetitions in three windows (the median window is reported, all three are kept),
and runs under its own alarm (`--leg-timeout` seconds).  Prints ONE JSON line and writes it to `--out`.

  torch_A      clip_grad_norm_ + torch.optim.AdamW(fused=True) + torch._foreach_lerp_ into an EMA copy   (52 B / parameter)
  torch_B      the same with torch.optim.AdamW at its defaults (what the README snippet constructs)
  native       AdamW(max_grad_norm, ema_params, ema_decay)                                              (40 B / parameter)
  native_*     without clipping (36 B), without EMA (32 B), plain (28 B)
  loop_*       zero_grad / model(x) / backward / step: steps per second with torch_B, with native, and without a step
"""
import argparse
import json
import os
import signal
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HP = dict(lr=1e-4, betas=(0.95, 0.999), eps=1e-6, weight_decay=1e-3)
MAX_NORM, EMA_DECAY = 1.0, 0.999


class _LegTimeout(Exception):
    pass


def _alarm(signum, frame):
    raise _LegTimeout()


def _windows(fn, reps, warmup, windows=3):
    """[(device ms per call, host ms per call to ISSUE it)] for `windows` windows of `reps` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        host = (time.perf_counter() - t0) * 1e3 / reps
        torch.cuda.synchronize()
        out.append((a.elapsed_time(b) / reps, host))
    return out


def _leg(result, name, make, reps, warmup, timeout, bytes_per_call=None, copy_gbps=None):
    """Runs one leg under its own alarm; a leg that fails or times out is reported and ends the run (nothing more is started
    on the device after a failure)."""
    signal.alarm(timeout)
    try:
        fn, cleanup = make()
        win = _windows(fn, reps, warmup)
        torch.cuda.synchronize()
        cleanup()
    except _LegTimeout:
        result[name] = {"error": f"timed out after {timeout} s"}
        raise
    finally:
        signal.alarm(0)
    ms = sorted(w[0] for w in win)[len(win) // 2]
    rec = {"ms": round(ms, 4), "windows_ms": [round(w[0], 4) for w in win], "host_issue_ms": round(min(w[1] for w in win), 4)}
    if bytes_per_call:
        rec["bytes"] = bytes_per_call
        rec["gbps"] = round(bytes_per_call / ms / 1e6, 1)
        if copy_gbps:
            rec["fraction_of_copy"] = round(rec["gbps"] / copy_gbps, 3)
    result[name] = rec
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--leg-timeout", type=int, default=120)
    ap.add_argument("--tiny", action="store_true", help="a small net instead of the headline one (checks the script itself)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    args = ap.parse_args()

    import bench
    import audio_diffusion_pytorch_amd as adp
    from audio_diffusion_pytorch_amd import _C
    from audio_diffusion_pytorch_amd._C import ptr

    signal.signal(signal.SIGALRM, _alarm)
    dev = torch.device("cuda:0")
    length = bench.LENGTH
    if args.tiny:
        torch.manual_seed(0)
        model = adp.DiffusionModel(net_t=adp.UNetV0, in_channels=2, channels=[8, 32, 64], factors=[1, 4, 4],
                                   items=[1, 2, 2], modulation_features=128).to(dev)
        length = 4096
    else:
        model = bench.build_model(dev)
    x = torch.randn(args.batch, 2, length, device=dev)
    params = [p for p in model.parameters() if p.requires_grad]
    n = sum(p.numel() for p in params)
    res = {"tool": "tools/optim_bench.py", "workload": f"[{args.batch},2,{length}] UNetV0, {n} parameters in {len(params)} tensors",
           "hyper_parameters": {**HP, "max_grad_norm": MAX_NORM, "ema_decay": EMA_DECAY}, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__}

    def fwd_bwd():
        for p in params:
            p.grad = None
        loss = model(x)
        loss.backward()

    try:
        signal.alarm(args.leg_timeout)
        for _ in range(3):   # the first call captures the step, the others replay it
            fwd_bwd()
        torch.cuda.synchronize()
        signal.alarm(0)
        grads = [p.grad for p in params]   # the views of the flat gradient buffer: kept for every optimizer-only leg

        # copy bandwidth of THIS box, as bench.py --full's calibration measures it (256 MB, 16-byte accesses)
        nc = 64 << 20
        src, dst = torch.randn(nc, device=dev), torch.empty(nc, device=dev)
        r = _leg(res, "copy_256MB", lambda: ((lambda: _C.call("adp_probe_copy", ptr(src), ptr(dst), nc, _C.stream())),
                                              (lambda: None)), 10, 5, args.leg_timeout, bytes_per_call=8 * nc)
        copy = r["gbps"]
        del src, dst

        def torch_leg(**kw):
            def make():
                opt = torch.optim.AdamW(params, **HP, **kw)
                ema = [p.detach().clone() for p in params]

                def fn():
                    torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                    opt.step()
                    with torch.no_grad():
                        torch._foreach_lerp_(ema, params, 1.0 - EMA_DECAY)
                return fn, (lambda: None)
            return make

        def native_leg(clip=True, ema=True):
            def make():
                emas = [p.detach().clone() for p in params] if ema else None
                opt = adp.AdamW(params, **HP, max_grad_norm=MAX_NORM if clip else None, ema_params=emas,
                                ema_decay=EMA_DECAY if ema else None)

                def cleanup():
                    assert opt.table_builds == 1, opt.table_builds
                return opt.step, cleanup
            return make

        legs = [("torch_A", torch_leg(fused=True), 52), ("torch_B", torch_leg(), 52), ("native", native_leg(), 40),
                ("native_no_clip", native_leg(clip=False), 36), ("native_no_ema", native_leg(ema=False), 32),
                ("native_plain", native_leg(clip=False, ema=False), 28)]
        for name, make, bpp in legs:
            _leg(res, name, make, args.reps, args.warmup, args.leg_timeout, bytes_per_call=bpp * n, copy_gbps=copy)
            torch.cuda.empty_cache()

        def loop_torch():
            opt = torch.optim.AdamW(params, **HP)
            ema = [p.detach().clone() for p in params]

            def fn():
                opt.zero_grad()
                loss = model(x)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                opt.step()
                with torch.no_grad():
                    torch._foreach_lerp_(ema, params, 1.0 - EMA_DECAY)
            return fn, (lambda: None)

        def loop_native():
            emas = [p.detach().clone() for p in params]
            opt = adp.AdamW(params, **HP, max_grad_norm=MAX_NORM, ema_params=emas, ema_decay=EMA_DECAY)

            def fn():
                opt.zero_grad()
                loss = model(x)
                loss.backward()
                opt.step()

            def cleanup():
                assert opt.table_builds == 1, opt.table_builds
            return fn, cleanup

        for name, make in (("loop_fwd_bwd_only", lambda: (fwd_bwd, lambda: None)), ("loop_torch_B", loop_torch),
                           ("loop_native", loop_native)):
            r = _leg(res, name, make, args.reps, args.warmup, args.leg_timeout)
            r["steps_per_s"] = round(1e3 / r["ms"], 3)
            torch.cuda.empty_cache()
        res["native_over_torch_A"] = round(res["native"]["ms"] / res["torch_A"]["ms"], 3)
        res["native_over_torch_B"] = round(res["native"]["ms"] / res["torch_B"]["ms"], 3)
    except _LegTimeout:
        res["aborted"] = "a leg timed out; nothing was started after it"
    except Exception as e:  # reported in the line; nothing is started after a failure
        res["aborted"] = f"{type(e).__name__}: {e}"
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 1 if "aborted" in res else 0


if __name__ == "__main__":
    sys.exit(main())
