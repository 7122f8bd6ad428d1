"""Progressive distillation (Salimans & Ho 2022) of a v-objective model on the gfx950 kernels of include/adp_distill.h:
`VDistillation` (the training loss of one stage) and `Distiller` (the stages: train, `halve()`, train, ...).  Not in the
reference; DESIGN.md section 6, "Progressive distillation".

A student learns to do in ONE DDIM step what its teacher does in TWO.  With phi = sigma pi / 2 a DDIM step of the v-objective
is a rotation, x' = cos(d) x - sin(d) v with d = phi - phi', so on the teacher grid `schedule(2N + 1)` (the student's N + 1
levels are its even entries) the two teacher steps d1, d2 from level 2i and the inversion of the one student step
D = d1 + d2 collapse to

    x_mid    = cos(d1) x_t - sin(d1) v1                      v1 = teacher(x_t,   sigma_{2i})
    v_target = c_x x_t + c_1 v1 + c_2 v2                     v2 = teacher(x_mid, sigma_{2i+1})
    c_x = -sin(d1) sin(d2) / sin(D)    c_1 = cos(d2) sin(d1) / sin(D)    c_2 = sin(d2) / sin(D)

in which the data never appears.  (The textbook form (cos(D) x_t - x_end) / sin(D) divides a cancelling difference by
sin(D) ~ pi / (2N): in float32, at the first step (sigma = 1, where the target is small), its relative error is 8e-3 at
N = 64 and above 1 at N = 1024, where the three-term form stays at 1e-6.)  The coefficients are one small host table per
`num_steps` (`ops.distill_table`, float64 rounded once); both combinations are launches of ONE kernel (adp_distill_comb),
the loss is the per-item weighted squared error (adp_distill_wmse_fwd / _bwd).

The step replays where `VDiffusion`'s does (graphed.py): graph F holds the index draw, the noise draw, both teacher forwards,
the two combinations, the student forward and the loss; graph B the student's backward only.
"""
import copy
from typing import Any, Dict, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from . import ops
from .capture import kwarg_structure
from .diffusion import (Distribution, LinearSchedule, Schedule, VDiffusion, VSampler, _is_number, _on_device_of, _VNoise)
from .models import DiffusionModel

WEIGHTINGS = ("truncated-snr", "uniform")


def _check_steps(what: str, num_steps) -> int:
    if not _is_number(num_steps) or int(num_steps) != num_steps or num_steps < 1:
        raise ValueError(f"{what}: num_steps must be a positive integer; got {num_steps!r}")
    return int(num_steps)


class DistillSteps(Distribution):
    """The draw of one distillation stage: a uniform student step index i in [0, N), i.e. the noise level `levels[2 i]` of
    the teacher grid.  `VDistillation` draws the INDEX itself (it gathers the whole coefficient row by it); this object is
    what the replayed step is keyed on."""

    def __init__(self, num_steps: int, levels: Tensor, weighting: str):
        super().__init__()
        self.num_steps, self.weighting = num_steps, weighting
        self.levels = levels.detach().to("cpu", torch.float32)  # the 2N + 1 teacher levels
        self.start, self.end = float(self.levels[0]), float(self.levels[-1])

    def __call__(self, num_samples: int, device: torch.device = torch.device("cpu")):
        idx = torch.randint(0, self.num_steps, (num_samples,), device=device)
        return self.levels.to(device)[2 * idx]

    def graph_key(self) -> Tuple:
        """What a captured training step bakes in of this stage (graphed.py)."""
        return ("distill", self.num_steps, self.start, self.end, self.weighting)


class _WMSE(torch.autograd.Function):
    """mean(w_r (v_pred - v_target)^2), one weight per item (None: ones), with a fused backward; the target is not
    differentiated."""

    @staticmethod
    def forward(ctx, v_pred, v_target, w):
        v_pred, v_target = v_pred.contiguous(), v_target.contiguous()
        ctx.save_for_backward(v_pred, v_target, w)
        return ops.distill_wmse_fwd(v_pred, v_target, w)

    @staticmethod
    def backward(ctx, gloss):
        v_pred, v_target, w = ctx.saved_tensors
        return ops.distill_wmse_bwd(v_pred, v_target, w, gloss.contiguous()), None, None


class VDistillation(VDiffusion):
    """The loss of one progressive-distillation stage: `net` (the student) learns, at a uniformly drawn student level, the
    v that makes ONE DDIM step of `num_steps` equal TWO DDIM steps of `teacher` on `schedule(2 * num_steps + 1)`.

    `teacher` is a submodule (`.to()` moves it), frozen, kept in eval mode and called under `torch.no_grad()`.
    `weighting`: "truncated-snr" weighs item r by max(cos^2 phi_r, sin^2 phi_r) -- max(SNR, 1) on the x error, written on
    the v error -- and "uniform" not at all.  A `loss_fn` other than `F.mse_loss` is called as `loss_fn(v_pred, v_target)`
    and needs weighting="uniform".  `teacher_kwargs` (fixed at construction) are merged over the call's kwargs for the two
    teacher calls only: `dict(embedding_scale=5.0)` makes the student learn the guided prediction in one unguided forward.
    `forward(x, noise=None, step_index=None, **kwargs)`: `step_index` [B] injects the draw as `noise` does (such a call
    runs eagerly).  The schedule is read when a table is built (once per `num_steps` and device)."""

    GRAPH_DISTRIBUTIONS = (DistillSteps,)

    def __init__(self, net: nn.Module, teacher: nn.Module, num_steps: int, schedule: Schedule = LinearSchedule(),
                 weighting: str = "truncated-snr", teacher_kwargs: Optional[Dict[str, Any]] = None,
                 loss_fn: Any = F.mse_loss, use_graph: bool = True):
        if weighting not in WEIGHTINGS:
            raise ValueError(f"VDistillation: weighting must be one of {WEIGHTINGS}; got {weighting!r}")
        if loss_fn is not F.mse_loss and weighting != "uniform":
            raise ValueError("VDistillation: the per-item weights are part of the fused squared error; a loss_fn other than "
                             "F.mse_loss needs weighting='uniform'")
        if teacher is net:
            raise ValueError("VDistillation: the teacher must be a copy of the student, not the same module")
        super().__init__(net=net, sigma_distribution=None, loss_fn=loss_fn, use_graph=use_graph)
        self.teacher = teacher.requires_grad_(False).eval()
        self.schedule = schedule
        self.weighting = weighting
        self.teacher_kwargs = dict(teacher_kwargs or {})
        self._tables: Dict[Any, Tensor] = {}  # (num_steps, device) -> [8, N]; kept for the module's lifetime (graphs read them)
        self.num_steps = num_steps

    # ---- the stage
    @property
    def num_steps(self) -> int:
        return self.sigma_distribution.num_steps

    @num_steps.setter
    def num_steps(self, value: int) -> None:
        n = _check_steps("VDistillation", value)
        levels = self.schedule(2 * n + 1, device="cpu").to(torch.float32)
        ops.distill_table(levels)  # (refuses levels that do not fall strictly inside [0, 1])
        self.sigma_distribution = DistillSteps(n, levels, self.weighting)

    def train(self, mode: bool = True):
        super().train(mode)
        self.teacher.eval()
        return self

    def table(self, device) -> Tensor:
        """`ops.distill_table` of this stage's teacher levels [8, N], on `device`."""
        key = (self.num_steps, torch.device(device))
        table = self._tables.get(key)
        if table is None:
            table = self._tables[key] = ops.distill_table(self.sigma_distribution.levels).to(device)
        return table

    # ---- the step
    def forward(self, x: Tensor, noise: Optional[Tensor] = None, step_index=None, **kwargs) -> Tensor:
        with _on_device_of(x):
            self.table(x.device)  # (a host-to-device copy: in front of a capture, never inside one)
        if step_index is None and self._graph_path_ok(x, noise) and self._teacher_kwargs_static():
            with _on_device_of(x):
                loss = self.train_graphs().run(x, noise, kwargs)
            if loss is not None:
                return loss
        return self._forward_eager(x, noise, step_index, **kwargs)

    def _teacher_kwargs_static(self) -> bool:
        """Whether a captured step may bake the teacher's own kwargs in (capture.kwarg_structure's rules)."""
        return kwarg_structure(self.teacher_kwargs, lambda t: t.is_cuda and not t.requires_grad) is not None

    def _step_rows(self, x: Tensor, step_index) -> Tensor:
        """The coefficient rows [8, B] of the drawn (or injected) student steps, gathered on the device."""
        n, b = self.num_steps, x.shape[0]
        if step_index is None:
            idx = torch.randint(0, n, (b,), device=x.device)
        else:
            idx = torch.as_tensor(step_index).detach().to("cpu", torch.long).reshape(-1)
            if idx.numel() != b or bool(((idx < 0) | (idx >= n)).any()):
                raise ValueError(f"VDistillation: step_index holds one student step in [0, {n}) per item ({b}); got "
                                 f"{idx.tolist()}")
            idx = idx.to(x.device)
        return self.table(x.device).index_select(1, idx)

    def _forward_eager(self, x: Tensor, noise: Optional[Tensor] = None, step_index=None, **kwargs) -> Tensor:
        with _on_device_of(x):
            rows = self._step_rows(x, step_index)
            if noise is None:
                noise = torch.randn_like(x)
            sigma, sigma_mid = rows[0], rows[1]
            x_t, _ = _VNoise.apply(x, noise, sigma)
            teacher_kwargs = {**kwargs, **self.teacher_kwargs}
            with torch.no_grad():
                v1 = self.teacher(x_t, sigma, **teacher_kwargs).contiguous()
                x_mid = ops.distill_comb(x_t, v1, rows[2:4])
                v2 = self.teacher(x_mid, sigma_mid, **teacher_kwargs).contiguous()
                v_target = ops.distill_comb(x_t, v1, rows[4:7], q=v2, out=x_mid)
            v_pred = self.net(x_t, sigma, **kwargs)
            if self.loss_fn is F.mse_loss:
                return _WMSE.apply(v_pred, v_target, rows[7] if self.weighting == "truncated-snr" else None)
            return self.loss_fn(v_pred, v_target)


class Distiller(nn.Module):
    """Progressive distillation of a trained `DiffusionModel` (v-objective): `Distiller(model, num_steps, **options)`, the
    options being `VDistillation`'s (schedule, weighting, teacher_kwargs, loss_fn, use_graph).

        distiller = Distiller(model, num_steps=32)              # the teacher samples in 64 steps
        opt = AdamW(distiller.student_parameters(), lr=1e-4)
        for audio in loader: distiller(audio).backward(); opt.step(); opt.zero_grad()
        distiller.halve()                                       # student -> teacher, num_steps 32 -> 16; train again
        sample = distiller.sample(noise)                        # VSampler over the student at distiller.num_steps

    `.student` is `model.net`, trained in place; `.teacher` is a deep copy of it.  `halve()` copies the student's weights
    into the teacher IN PLACE, so no address changes and no captured graph is invalidated by the copy (the next step is
    captured once more because the stage's `num_steps` is part of its key).  `state_dict()` carries `num_steps`."""

    def __init__(self, model: DiffusionModel, num_steps: int, schedule: Schedule = LinearSchedule(), **options):
        super().__init__()
        if not isinstance(model, DiffusionModel) or type(getattr(model, "diffusion", None)) is not VDiffusion:
            trained = type(model.diffusion).__name__ if isinstance(model, DiffusionModel) else None
            raise TypeError("Distiller: model must be a DiffusionModel trained with VDiffusion; got "
                            f"{type(model).__name__}" + (f" with {trained}" if trained else ""))
        self.diffusion = VDistillation(net=model.net, teacher=copy.deepcopy(model.net), num_steps=num_steps,
                                       schedule=schedule, **options)
        self.sampler = VSampler(net=model.net, schedule=schedule)

    @property
    def student(self) -> nn.Module:
        return self.diffusion.net

    @property
    def teacher(self) -> nn.Module:
        return self.diffusion.teacher

    @property
    def num_steps(self) -> int:
        return self.diffusion.num_steps

    @num_steps.setter
    def num_steps(self, value: int) -> None:
        self.diffusion.num_steps = value

    def student_parameters(self):
        """What to give the optimizer: the student's parameters (the teacher's are frozen)."""
        return [p for p in self.student.parameters() if p.requires_grad]

    def forward(self, x: Tensor, **kwargs) -> Tensor:
        return self.diffusion(x, **kwargs)

    def halve(self) -> int:
        """The student becomes the next stage's teacher: its weights (and buffers) are copied into the teacher in place and
        `num_steps` is halved.  Returns the new `num_steps`."""
        n = self.num_steps
        if n < 2 or n % 2:
            raise ValueError(f"Distiller.halve: num_steps must be even to be halved; got {n}")
        with torch.no_grad():
            for mine, theirs in ((self.teacher.parameters(), self.student.parameters()),
                                 (self.teacher.buffers(), self.student.buffers())):
                for dst, src in zip(mine, theirs):
                    dst.copy_(src)
        self.num_steps = n // 2
        return self.num_steps

    @torch.no_grad()
    def sample(self, noise: Tensor, num_steps: Optional[int] = None, **kwargs) -> Tensor:
        """`VSampler` over the student, by default at this stage's `num_steps`."""
        return self.sampler(noise, num_steps=self.num_steps if num_steps is None else num_steps, **kwargs)

    def get_extra_state(self):
        return {"num_steps": self.num_steps}

    def set_extra_state(self, state) -> None:
        self.num_steps = state["num_steps"]
