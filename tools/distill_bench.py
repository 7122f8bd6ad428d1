"""What a progressive-distillation step costs on the headline net, against what it is made of.

    python tools/distill_bench.py [--reps 20] [--num-steps 32] [--out profiles/distill_bench.json]

One process, bench.py's headline configuration ([4,2,2**18], the README net), three legs:

  distill_step   `loss = distiller(x); loss.backward()`   the replayed VDistillation step (graph F: index and noise draws,
                                                          two teacher forwards, two adp_distill_comb launches, the student
                                                          forward, the weighted loss; graph B: the student's backward)
  plain_step     `loss = model(x); loss.backward()`       the replayed VDiffusion step of the same model
  forward        one U-Net forward under torch.no_grad(), replayed from a hipGraph of its own (as the teacher's forwards run
                 inside graph F)

The expectation is distill_step = plain_step + 2 forward; `ratio` is distill_step over that sum.  Every leg is warmed up,
timed with device events over `--reps` repetitions in three windows (the median window is reported, all three are kept) and
runs under its own alarm (`--leg-timeout` seconds); nothing is started on the device after a leg that failed.  Prints ONE
JSON line and writes it to `--out`.
"""
import argparse
import json
import os
import signal
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _LegTimeout(Exception):
    pass


def _alarm(signum, frame):
    raise _LegTimeout()


def _windows(fn, reps, warmup, windows=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return out


def _leg(result, name, fn, reps, warmup, timeout):
    signal.alarm(timeout)
    try:
        win = _windows(fn, reps, warmup)
    except _LegTimeout:
        result[name] = {"error": f"timed out after {timeout} s"}
        raise
    finally:
        signal.alarm(0)
    result[name] = {"ms": round(sorted(win)[len(win) // 2], 4), "windows_ms": [round(w, 4) for w in win]}
    return result[name]["ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--num-steps", type=int, default=32)
    ap.add_argument("--leg-timeout", type=int, default=120)
    ap.add_argument("--tiny", action="store_true", help="a small net instead of the headline one (checks the script itself)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_bench.json"))
    args = ap.parse_args()

    import bench
    import audio_diffusion_pytorch_amd as adp
    from audio_diffusion_pytorch_amd import graphed

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
    distiller = adp.Distiller(model, args.num_steps).to(dev)
    x = torch.randn(args.batch, 2, length, device=dev)
    params = distiller.student_parameters()
    res = {"tool": "tools/distill_bench.py", "num_steps": args.num_steps, "reps": args.reps,
           "workload": f"[{args.batch},2,{length}] UNetV0, {sum(p.numel() for p in params)} student parameters",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__}

    def step_of(module):
        def fn():
            for p in params:
                p.grad = None
            module(x).backward()
        return fn

    try:
        distill = _leg(res, "distill_step", step_of(distiller), args.reps, args.warmup, args.leg_timeout)
        g = graphed.GRAPHS_OF.get(distiller.diffusion)
        res["distill_step"]["captures"], res["distill_step"]["replays"] = (g.captures, g.replays) if g else (0, 0)
        plain = _leg(res, "plain_step", step_of(model), args.reps, args.warmup, args.leg_timeout)
        g = graphed.GRAPHS_OF.get(model.diffusion)
        res["plain_step"]["captures"], res["plain_step"]["replays"] = (g.captures, g.replays) if g else (0, 0)

        signal.alarm(args.leg_timeout)
        sigma = torch.full((args.batch,), 0.5, device=dev)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                distiller.teacher(x, sigma)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(graph):
            distiller.teacher(x, sigma)
        signal.alarm(0)
        forward = _leg(res, "forward", graph.replay, args.reps, args.warmup, args.leg_timeout)
        res["expected_ms"] = round(plain + 2 * forward, 4)
        res["ratio"] = round(distill / (plain + 2 * forward), 4)
    except _LegTimeout:
        res["aborted"] = "a leg timed out; nothing was started after it"
    except Exception as e:  # reported in the line; nothing is started after a failure
        res["aborted"] = f"{type(e).__name__}: {e}"
    finally:
        signal.alarm(0)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 1 if "aborted" in res else 0


if __name__ == "__main__":
    sys.exit(main())
