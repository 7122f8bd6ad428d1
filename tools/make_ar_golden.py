"""Generates tests/golden/ar_golden.pt from the LIVE reference's ARVDiffusion / ARVSampler
(/root/reference/audio_diffusion_pytorch/diffusion.py:98-130, :193-296, loaded by oracle/reference_loader.py) driven through a
tiny UNetV0Oracle with the autoregressive flags (one extra input channel, no modulation, no time conditioning).
Runs only where the reference checkout exists:  python tools/make_ar_golden.py

The fixture holds data only: the net's configuration and state dict, one training case (x, the sigmas and the noise the
reference drew, x_noisy, v_target, loss, parameter gradients), sigma ladders, and seeded sampler runs (seed, arguments, output).
The reference exposes neither its draws nor x_noisy / v_target: the net's input and the loss function's arguments are
recorded while it runs, and the draws are recovered by re-seeding and repeating them in the reference's order -- asserted to
reproduce the recorded x_noisy exactly."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.a_unet_restatement import UNetV0Oracle  # noqa: E402
from oracle.reference_loader import load_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ar_golden.pt")
C, LENGTH, SPLITS = 2, 64, 4
CFG = dict(in_channels=C + 1, out_channels=C, channels=[8, 16], factors=[2, 2], items=[1, 1], resnet_groups=4,
           use_modulation=False, use_time_conditioning=False)
TRAIN_SEED = 31
LADDERS = [(4, 2), (8, 1), (6, 3), (2, 5)]          # (num_splits, steps per split) at length 48
SAMPLER_RUNS = [dict(seed=5, num_items=2, num_chunks=4, num_steps=5),     # num_chunks == num_splits: the start alone
                dict(seed=7, num_items=2, num_chunks=6, num_steps=8)]     # shifts: 8 + 6 * 2 = 20 net evaluations


class Recording(torch.nn.Module):
    """The net, keeping the last input it was given."""

    def __init__(self, net):
        super().__init__()
        self.net, self.seen = net, None

    def forward(self, channels, **kwargs):
        self.seen = channels.detach().clone()
        return self.net(channels, **kwargs)


def main():
    D, _ = load_reference()
    torch.manual_seed(0)
    net = UNetV0Oracle(**CFG)
    with torch.no_grad():  # non-trivial norms and biases
        for name, p in net.named_parameters():
            if name.endswith("bias") or "gn" in name:
                p.add_(0.1 * torch.randn_like(p))
    out = {"cfg": CFG, "in_channels": C, "length": LENGTH, "num_splits": SPLITS,
           "state_dict": {k: v.clone() for k, v in net.state_dict().items()}}

    # ---- training case
    x = torch.randn(3, C, LENGTH, generator=torch.Generator().manual_seed(11))
    rec, targets = Recording(net), {}

    def loss_fn(v_pred, v_target):
        targets["v_target"] = v_target.detach().clone()
        return F.mse_loss(v_pred, v_target)

    diffusion = D.ARVDiffusion(rec, length=LENGTH, num_splits=SPLITS, loss_fn=loss_fn)
    torch.manual_seed(TRAIN_SEED)
    loss = diffusion(x)
    loss.backward()
    torch.manual_seed(TRAIN_SEED)  # the reference's draws, in its order (diffusion.py:118, :121)
    sigmas = torch.rand((x.shape[0], 1, SPLITS))
    noise = torch.randn_like(x)
    full = sigmas.repeat_interleave(LENGTH // SPLITS, dim=-1)
    alphas, betas = diffusion.get_alpha_beta(full)
    x_noisy, plane = rec.seen[:, :C], rec.seen[:, C:]
    assert torch.equal(alphas * x + betas * noise, x_noisy), "the recovered draws do not reproduce the reference's x_noisy"
    assert torch.equal(plane, full)
    assert torch.equal(alphas * noise - betas * x, targets["v_target"])
    out["train"] = dict(seed=TRAIN_SEED, x=x, sigmas=sigmas, noise=noise, x_noisy=x_noisy.clone(),
                        v_target=targets["v_target"], loss=loss.detach().clone(),
                        grads={k: p.grad.clone() for k, p in net.named_parameters()})
    net.zero_grad()

    # ---- ladders
    out["ladders"] = []
    for n, i in LADDERS:
        sampler = D.ARVSampler(net, in_channels=C, length=48, num_splits=n)
        out["ladders"].append(dict(num_splits=n, length=48, num_items=2, num_steps_per_split=i,
                                   sigmas=sampler.get_sigmas_ladder(num_items=2, num_steps_per_split=i)))

    # ---- seeded sampler runs (the reference draws from the global generator)
    sampler = D.ARVSampler(net, in_channels=C, length=LENGTH, num_splits=SPLITS)
    out["samples"] = []
    for run in SAMPLER_RUNS:
        args = {k: v for k, v in run.items() if k != "seed"}
        torch.manual_seed(run["seed"])
        y = sampler(**args)
        assert y.shape == (args["num_items"], C, args["num_chunks"] * (LENGTH // SPLITS)) and torch.isfinite(y).all()
        out["samples"].append(dict(run, output=y.clone()))

    torch.save(out, OUT)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
