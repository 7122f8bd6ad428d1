"""One text encode on the GPU, random weights, m = 64 tokens, B = 1 and B = 4, at the geometry --ff names:

    relu         t5-base       vocab 32128, d_model 768, 12 heads of 64, d_ff 3072, 12 blocks    text.T5Encoder
    gated-gelu   flan-t5-base  vocab 32128, d_model 768, 12 heads of 64, d_ff 2048, 12 blocks    text.T5GatedEncoder

Subjects, timed in one process and interleaved repeat by repeat:

    native_eager   the native encoder, one Python call per kernel launch
    native_graph   the same forward captured once and replayed from a hipGraph
    torch_eager    transformers.T5EncoderModel with the SAME weights on the same GPU (library GEMMs); only where
                   transformers is importable -- what a user has without the native encoder

Medians over --reps repeats with the min-max spread; launches per encode (native: counted from one profiled pass; the weight
bytes an encode must stream over the replayed time as GB/s); then ONE profiled native pass per batch size (a HIP event pair
per launch) for the per-kernel split.  Writes one JSON object to --out and prints it.  The measurement runs in a child
process under --timeout seconds; this process never opens the GPU.
--out holds one object per --ff: a run replaces its own entry and keeps the other.
usage: python tools/t5_bench.py [--ff relu|gated-gelu] [--reps R] [--inner I] [--timeout S] [--out profiles/t5_bench.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMS = {"relu": dict(vocab_size=32128, d_model=768, d_kv=64, d_ff=3072, num_layers=12, num_heads=12),
         "gated-gelu": dict(vocab_size=32128, d_model=768, d_kv=64, d_ff=2048, num_layers=12, num_heads=12)}
TOKENS = 64


def worker(args):
    import torch
    sys.path.insert(0, ROOT)
    from audio_diffusion_pytorch_amd import _C
    from audio_diffusion_pytorch_amd.text import T5Encoder, T5GatedEncoder

    GEOM = GEOMS[args.ff]
    Encoder = {"relu": T5Encoder, "gated-gelu": T5GatedEncoder}[args.ff]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = Encoder(**GEOM).to(dev)
    hf = None
    try:
        import transformers
        hf = transformers.T5EncoderModel(transformers.T5Config(**GEOM, feed_forward_proj=args.ff, dropout_rate=0.0)).eval()
        enc_cpu = Encoder(**GEOM)
        enc_cpu.load_hf_state_dict(hf.state_dict())   # the same weights on both sides
        enc = enc_cpu.to(dev)
        hf = hf.to(dev)
    except ImportError:
        pass
    inner = GEOM["num_heads"] * GEOM["d_kv"]
    # what an encode must read once: every block's matrices (the embedding rows and norm weights are noise next to them)
    ff_mats = 3 if args.ff == "gated-gelu" else 2
    weight_bytes = 4 * GEOM["num_layers"] * (4 * inner * GEOM["d_model"] + ff_mats * GEOM["d_model"] * GEOM["d_ff"])
    res = {"feed_forward_proj": args.ff, "geometry": GEOM, "tokens": TOKENS, "reps": args.reps, "inner": args.inner, "weight_bytes": weight_bytes,
           "transformers": None if hf is None else transformers.__version__, "batches": {}}
    for B in (1, 4):
        g = torch.Generator().manual_seed(B)
        ids = torch.randint(0, GEOM["vocab_size"], (B, TOKENS), generator=g).to(dev)
        mask = (torch.arange(TOKENS)[None, :] < torch.tensor([TOKENS, 20, 9, 40][:B])[:, None]).to(torch.int64).to(dev)
        want = enc(ids, mask).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            enc(ids, mask)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = enc(ids, mask)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), "the replayed encode differs from the eager one"
        subjects = {"native_eager": lambda: enc(ids, mask), "native_graph": graph.replay}
        r = {}
        if hf is not None:
            def torch_eager():
                with torch.no_grad():
                    return hf(input_ids=ids, attention_mask=mask).last_hidden_state
            subjects["torch_eager"] = torch_eager
            ref = torch_eager()
            r["max_rel_diff_vs_torch"] = float((want - ref).abs().max() / ref.abs().max())
        for fn in subjects.values():   # warm-up: code objects, the GEMM library's algorithm choice
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in subjects}
        for _ in range(args.reps):     # interleaved
            for name, fn in subjects.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.inner):
                    fn()
                b.record()
                torch.cuda.synchronize()
                times[name].append(a.elapsed_time(b) / args.inner)
        for name, t in times.items():
            r[name + "_ms"] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
        r["native_graph_weight_GBps"] = round(weight_bytes / (r["native_graph_ms"]["median"] * 1e-3) / 1e9, 1)
        if hf is not None:
            r["native_graph_over_torch_eager"] = round(r["native_graph_ms"]["median"] / r["torch_eager_ms"]["median"], 3)
            try:   # kernel launches of one torch encode, from torch's own profiler; None where it cannot trace here
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    torch_eager()
                    torch.cuda.synchronize()
                r["torch_eager_launches"] = sum(e.count for e in prof.key_averages() if e.device_type.name != "CPU") or None
            except Exception as e:
                r["torch_eager_launches"] = None
                r["torch_eager_launches_error"] = repr(e)[:200]
        _C.PROFILE = []                # one profiled pass: the events slow the host, so this is a split, not an encode time
        try:
            enc(ids, mask)
        finally:
            recs = _C.profile_collect()
        split, total = {}, 0.0
        for call, kernel, meta, ms in recs:
            key = kernel.split("::")[-1]
            e = split.setdefault(key, {"launches": 0, "ms": 0.0})
            e["launches"] += 1
            e["ms"] += ms
            total += ms
        r["native_launches"] = len(recs)
        r["native_kernel_split_ms"] = {k: {"launches": v["launches"], "ms": round(v["ms"], 4)}
                                       for k, v in sorted(split.items(), key=lambda kv: -kv[1]["ms"])}
        r["native_kernel_sum_ms"] = round(total, 4)
        res["batches"][f"B{B}"] = r
    both = {}
    if os.path.exists(args.out):   # one entry per --ff; a file of the earlier single-object layout is a ReLU run
        with open(args.out) as f:
            old = json.load(f)
        both = {"relu": old} if "batches" in old else old
    both[args.ff] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(both) + "\n")
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ff", choices=sorted(GEOMS), default="relu", help="the feed-forward, and with it the geometry")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t5_bench.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--ff", args.ff, "--reps", str(args.reps), "--inner", str(args.inner),
           "--out", args.out]
    try:
        sys.exit(subprocess.run(cmd, timeout=args.timeout).returncode)
    except subprocess.TimeoutExpired:
        sys.exit(f"t5_bench: the measurement did not finish in {args.timeout} s")


if __name__ == "__main__":
    main()
