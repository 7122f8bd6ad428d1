"""The mel encoder on the GPU at the README autoencoder shape: MelE1d(in_channels=2, channels=512, multipliers=[1, 1],
factors=[2], num_blocks=[12], out_channels=32, 80 mel channels, n_fft 1024, hop 256, tanh bottleneck) on x = [4, 2, 2**18].
Times forward + backward (every parameter gradient) of two subjects in one process, interleaved repeat by repeat:

    native   the module as it is (csrc/encoder.hip + the conv / norm kernels of include/adp.h)
    torch    the same module's own torch.nn submodules called directly (MIOpen / rocBLAS) behind the same native mel front end

Medians over --reps repeats with the min-max spread, then ONE profiled native pass (a HIP event pair per launch) for the
per-kernel split and the share of the new downsample kernels.  Writes one JSON object to --out and prints it.  The
measurement runs in a child process under --timeout seconds; this process never opens the GPU.
usage: python tools/encoder_bench.py [--reps R] [--inner I] [--timeout S] [--out profiles/encoder_bench.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (4, 2, 2 ** 18)
ENCODER = dict(in_channels=2, channels=512, multipliers=[1, 1], factors=[2], num_blocks=[12], out_channels=32, mel_channels=80,
               mel_sample_rate=48000, mel_n_fft=1024, mel_hop_length=256, mel_normalize_log=True)


def worker(args):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from audio_diffusion_pytorch_amd import _C
    from audio_diffusion_pytorch_amd.encoders import MelE1d, TanhBottleneck

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = MelE1d(**ENCODER, bottleneck=TanhBottleneck()).to(dev)
    params = list(enc.parameters())
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(*SHAPE, device=dev, generator=g)

    def torch_stack(mel):
        h = enc.to_in(mel)
        for stage in enc.downsample:
            h = stage.down(h)
            for b in stage.blocks:
                h = h + b.conv2(F.silu(b.norm2(b.conv1(F.silu(b.norm1(h))))))
        return torch.tanh(enc.to_out(h))

    def mel_of(x):
        with torch.no_grad():
            m = enc.mel(x)
        return m.view(x.shape[0], -1, m.shape[3])

    dz = torch.randn(enc(x).shape, device=dev, generator=g)
    subjects = {
        "native": lambda: torch.autograd.grad(enc(x), params, dz),
        "torch": lambda: torch.autograd.grad(torch_stack(mel_of(x)), params, dz),
    }
    ga, gb = subjects["native"](), subjects["torch"]()
    res = {"shape": list(SHAPE), "encoder": ENCODER, "latent": list(dz.shape), "reps": args.reps, "inner": args.inner,
           "max_grad_rel_diff_vs_torch": max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(ga, gb))}
    del ga, gb
    for fn in subjects.values():   # warm-up: code objects, MIOpen's algorithm search
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in subjects}
    for _ in range(args.reps):     # interleaved: native, torch, native, torch, ...
        for name, fn in subjects.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / args.inner)
    for name, t in times.items():
        res[name + "_fwd_bwd_ms"] = {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    res["native_over_torch"] = round(res["native_fwd_bwd_ms"]["median"] / res["torch_fwd_bwd_ms"]["median"], 3)

    _C.PROFILE = []                # one profiled pass: the events slow the host, so this is a split, not a step time
    try:
        subjects["native"]()
    finally:
        recs = _C.profile_collect()
    split, total, down = {}, 0.0, 0.0
    for call, kernel, meta, ms in recs:
        key = kernel.split("<")[0].split("::")[-1]
        e = split.setdefault(key, {"launches": 0, "ms": 0.0})
        e["launches"] += 1
        e["ms"] += ms
        total += ms
        if call.startswith("adp_enc_down"):
            down += ms
    res["native_kernel_split_ms"] = {k: {"launches": v["launches"], "ms": round(v["ms"], 4)}
                                     for k, v in sorted(split.items(), key=lambda kv: -kv[1]["ms"])}
    res["native_kernel_sum_ms"] = round(total, 3)
    res["down_kernels_ms"] = round(down, 4)
    res["down_kernels_share"] = round(down / total, 4) if total > 0 else None
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_bench.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(args.reps), "--inner", str(args.inner),
           "--out", args.out]
    try:
        sys.exit(subprocess.run(cmd, timeout=args.timeout).returncode)
    except subprocess.TimeoutExpired:
        sys.exit(f"encoder_bench: the measurement did not finish in {args.timeout} s")


if __name__ == "__main__":
    main()
