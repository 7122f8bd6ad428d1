"""Generates tests/golden/clip_golden.pt from the LIVE reference's `clip` (diffusion.py:41-54, loaded by
oracle/reference_loader.py): inputs and the reference's outputs for the static clamp and for dynamic thresholds, on a
[B, C, T] and a [B, T] batch.  Run where the reference is present:  python tests/golden/make_clip_golden.py

The inputs are Gaussians scaled so that some items exceed [-1, 1] at the chosen quantile and some do not (the reference
clamps the scale to a minimum of 1)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.reference_loader import load_reference  # noqa: E402

THRESHOLDS = (0.0, 0.3, 0.5, 0.9, 0.995, 1.0)
SHAPES = {"bct": (3, 2, 257), "bt": (4, 100)}


def main():
    D, _ = load_reference()
    g = torch.Generator().manual_seed(4321)
    out = {"thresholds": torch.tensor(THRESHOLDS, dtype=torch.float64)}
    for name, shape in SHAPES.items():
        gain = torch.tensor([0.2, 1.0, 3.0, 0.7][:shape[0]]).view(-1, *([1] * (len(shape) - 1)))
        x = torch.randn(shape, generator=g) * gain
        out[f"{name}/x"] = x
        for q in THRESHOLDS:
            out[f"{name}/clip/{q}"] = D.clip(x.clone(), dynamic_threshold=q)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "clip_golden.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
