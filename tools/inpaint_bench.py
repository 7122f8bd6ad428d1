"""VInpainter on the README U-Net layout (BASELINE config 3's net) at [1, 2, 2**18]: ms per resample (1 resample = 1 U-Net
forward + the update) of a run of 8 steps x 4 resamples, three ways:

  torch_eager    VInpainter(net): torch.randn_like + adp_v_inpaint_step, every kernel launched call by call (the default)
  philox_eager   noise="philox": adp_v_inpaint_step_rng forms the noise in registers, launched call by call
  philox_graph   noise="philox", use_graph=True: one captured resample replayed behind a copy of its table row

One process per variant and run (a fresh child each time: its own allocator pools, code objects and captures), the variants
alternating, `--repeats` runs each.  A child warms up with one whole run, then times the next one.  The spread of a variant
is max - min over its runs.  One JSON line on stdout; it is also written to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {"torch_eager": dict(), "philox_eager": dict(noise="philox"), "philox_graph": dict(noise="philox", use_graph=True)}


def child(variant: str, steps: int, resamples: int, length: int) -> None:
    import torch
    import bench
    import audio_diffusion_pytorch_amd as adp
    assert torch.cuda.is_available(), "inpaint_bench measures on the MI355X only"
    dev = torch.device("cuda:0")
    net = bench.build_model(dev).net
    inp = adp.VInpainter(net, **VARIANTS[variant])
    g = torch.Generator().manual_seed(1)
    source = torch.randn(1, 2, length, generator=g).to(dev)
    mask = torch.zeros(1, 2, length, dtype=torch.bool, device=dev)
    mask[..., : length // 2] = True   # continuation: the first half is known
    kw = dict(seed=3) if variant != "torch_eager" else {}

    def run():
        return inp(source, mask, num_steps=steps, num_resamples=resamples, **kw)

    torch.manual_seed(2)
    run()  # warm-up: capture, allocator pools, code objects
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"variant": variant, "ms_per_resample": ms / (steps * resamples), "finite": bool(torch.isfinite(out).all()),
                      "known_region_exact": bool(torch.equal(out[mask], source[mask])),
                      "graph_captures": inp.graph_captures}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, choices=list(VARIANTS))
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--resamples", type=int, default=4)
    ap.add_argument("--length", type=int, default=2 ** 18)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inpaint_bench.json"))
    a = ap.parse_args()
    if a.child:
        child(a.child, a.steps, a.resamples, a.length)
        return
    runs = {v: [] for v in VARIANTS}
    for _ in range(a.repeats):
        for v in VARIANTS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", v, "--steps", str(a.steps), "--resamples",
                   str(a.resamples), "--length", str(a.length)]
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            if done.returncode != 0:   # nothing more is started on the device after a child that failed
                sys.stderr.write(done.stdout + done.stderr)
                raise SystemExit(f"inpaint_bench: the {v} child ended with status {done.returncode}")
            runs[v].append(json.loads(done.stdout.strip().splitlines()[-1]))
    result = {"metric": "VInpainter ms per resample, README U-Net layout", "shape": [1, 2, a.length], "num_steps": a.steps,
              "num_resamples": a.resamples, "runs_per_variant": a.repeats, "variants": {}}
    for v, recs in runs.items():
        ms = sorted(r["ms_per_resample"] for r in recs)
        result["variants"][v] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4),
                                 "max_ms": round(ms[-1], 4), "spread_ms": round(ms[-1] - ms[0], 4),
                                 "finite": all(r["finite"] for r in recs),
                                 "known_region_exact": all(r["known_region_exact"] for r in recs),
                                 "graph_captures": recs[-1]["graph_captures"]}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
