"""The tail of a training step as two launches: `AdamW` = torch.optim.AdamW + clip_grad_norm_ + an EMA copy of the weights.

    ema_model = copy.deepcopy(model)
    opt = AdamW(model.parameters(), lr=1e-4, betas=(0.95, 0.999), eps=1e-6, weight_decay=1e-3,
                max_grad_norm=1.0, ema_params=ema_model.parameters(), ema_decay=0.999)
    for x in loader:
        opt.zero_grad(); loss = model(x); loss.backward(); opt.step()

`step()` issues one reduction over the gradients (adp_sqnorm_partials; only with `max_grad_norm`) and one fused update per
class of parameters that share every scalar (adp_adamw_step; normally one per param group): p, g, m, v and the EMA tensor
are read once and p, m, v, EMA written once, 36 B + 4 B per parameter against 52 B for torch's three best-case passes.

The arithmetic is torch.optim.AdamW's: hyper-parameters and bias corrections are computed on the host in double from
`group["lr"]` etc. at every step (LR schedulers keep working) and handed to the kernel as arguments.

Differences from the torch calls it replaces, all deliberate:
  * clipping is applied when the update kernel READS the gradient: `.grad` itself is left unscaled (clip_grad_norm_ scales it
    in place).  The norm of the last step is `opt.grad_norm`, a 0-dim device tensor; reading it is the caller's sync.
  * the EMA tensors are updated in place: the EMA model samples with current weights, and its captured sampler graphs
    stay valid because no address moves.
  * the kernels work from DEVICE tables of pointers and chunks, built at the first step and rebuilt only when a parameter, a
    gradient or an EMA tensor moved, or the set of parameters with a gradient changed (`opt.table_builds` counts).  The
    replayed training step hands back gradients at the same addresses every step, so in the steady state `step()` allocates
    nothing, copies nothing between host and device and never synchronises.  An eager loop whose gradients are re-allocated
    every step (zero_grad(set_to_none=True)) rebuilds the tables every step: correct, but it pays a small upload each time.

fp32 contiguous dense parameters on one device only; no amsgrad / maximize / capturable / foreach / fused / differentiable.
"""
import math
from typing import Any, Dict, Iterable, List, Optional

import torch
from torch import Tensor

from . import ops

CHUNK = 8192  # elements of one unit of work (one workgroup trip): 32 KB per stream

# option -> the only accepted value (torch.optim.AdamW's default)
_UNSUPPORTED = (("amsgrad", False), ("maximize", False), ("foreach", None), ("capturable", False),
                ("differentiable", False), ("fused", None), ("decoupled_weight_decay", True))


class _Class:
    """Parameters that share every scalar of the update: one param group, one step count -> one launch."""
    __slots__ = ("group", "step", "chunks")


class AdamW(torch.optim.Optimizer):
    """Drop-in for torch.optim.AdamW (same positional / keyword names, defaults, state-dict keys) running as fused gfx950
    kernels, with optional global-norm gradient clipping (`max_grad_norm`, clip_grad_norm_(params, max_grad_norm, 2.0)
    semantics over ALL parameters of ALL groups) and an optional in-place EMA copy (`ema_params` one to one with `params`,
    `ema_decay`; with several param groups put `ema_params` into each group dict).  See the module docstring."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, *, maximize: bool = False, foreach: Optional[bool] = None,
                 capturable: bool = False, differentiable: bool = False, fused: Optional[bool] = None,
                 max_grad_norm: Optional[float] = None, ema_params: Optional[Iterable[Tensor]] = None,
                 ema_decay: Optional[float] = None):
        if isinstance(lr, Tensor):
            raise NotImplementedError("AdamW: a tensor `lr` is not supported (hyper-parameters are host scalars passed as "
                                      "kernel arguments); pass a float")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        if ema_decay is not None and not 0.0 <= ema_decay <= 1.0:
            raise ValueError(f"Invalid ema_decay: {ema_decay}")
        params = list(params)
        grouped = len(params) > 0 and isinstance(params[0], dict)
        if grouped:
            if ema_params is not None:
                raise ValueError("AdamW: with param groups, pass `ema_params` inside each group dict")
            has_ema = any("ema_params" in g for g in params)
        else:
            has_ema = ema_params is not None
            if has_ema:
                params = [{"params": params, "ema_params": ema_params}]
        if has_ema != (ema_decay is not None):
            raise ValueError("AdamW: `ema_params` and `ema_decay` go together (got one without the other)")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.grad_norm: Optional[Tensor] = None   # 0-dim device tensor: the global L2 gradient norm of the last step
        self.table_builds = 0                     # how many times the device tables were (re)built
        self._ema_groups: List[Optional[List[Tensor]]] = []
        self._sig = None
        self._classes: List[_Class] = []
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=True)
        self._check_options(defaults)
        super().__init__(params, defaults)

    # ------------------------------------------------------------------ construction / validation
    @staticmethod
    def _check_options(group: Dict[str, Any]) -> None:
        for name, only in _UNSUPPORTED:
            value = group.get(name, only)
            if (value is not only) if only is None else (bool(value) != only):
                raise NotImplementedError(f"AdamW: {name}={value!r} is not supported by the fused gfx950 step "
                                          f"(only {name}={only!r})")

    def add_param_group(self, param_group: Dict[str, Any]) -> None:
        param_group = dict(param_group)
        ema = param_group.pop("ema_params", None)
        if (ema is not None) != (self.ema_decay is not None):
            raise ValueError("AdamW: every param group carries `ema_params` when `ema_decay` is given, and none otherwise")
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._check_options(group)
            if ema is not None:
                ema = [ema] if isinstance(ema, Tensor) else list(ema)
                ps = group["params"]
                if len(ema) != len(ps):
                    raise ValueError(f"AdamW: {len(ema)} ema_params for {len(ps)} params")
                for i, (e, p) in enumerate(zip(ema, ps)):
                    if e.shape != p.shape:
                        raise ValueError(f"AdamW: ema_params[{i}] has shape {tuple(e.shape)}, its parameter "
                                         f"{tuple(p.shape)}")
                    if e is p or (e.numel() and e.data_ptr() == p.data_ptr()):
                        raise ValueError(f"AdamW: ema_params[{i}] IS its parameter (use a copy.deepcopy of the model)")
        except Exception:
            self.param_groups.pop()
            raise
        self._ema_groups.append(ema)
        self._sig = None

    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        super().load_state_dict(state_dict)
        self._sig = None  # moments and step counts were replaced: the tables name the old ones

    # ------------------------------------------------------------------ device tables
    def _signature(self) -> tuple:
        """What the device tables assume: addresses of every parameter, its gradient (0: none) and its EMA tensor."""
        sig = []
        for group, emas in zip(self.param_groups, self._ema_groups):
            for p in group["params"]:
                g = p.grad
                sig.append(p.data_ptr())
                sig.append(0 if g is None else g.data_ptr())
            if emas is not None:
                sig.extend(e.data_ptr() for e in emas)
        return tuple(sig)

    @staticmethod
    def _check_tensor(t: Tensor, what: str, index: int, device) -> None:
        if t.layout != torch.strided:
            raise RuntimeError(f"AdamW: {what} of parameter {index} is {t.layout} (sparse gradients are not supported)")
        if t.dtype != torch.float32:
            raise TypeError(f"AdamW: {what} of parameter {index} is {t.dtype}; the fused step is fp32 only")
        if not t.is_contiguous():
            raise TypeError(f"AdamW: {what} of parameter {index} is not contiguous")
        if t.device != device:
            raise RuntimeError(f"AdamW: {what} of parameter {index} is on {t.device}, parameter 0 on {device}")

    def _build(self) -> None:
        """Walks params / grads / state once and uploads the tables (the only host-to-device copy this class makes)."""
        rows: Dict[Any, list] = {}      # (group index, step count) -> [(p, g, m, v, ema)]
        grads: List[Tensor] = []
        steps: List[Tensor] = []
        device, index = None, -1
        for gi, (group, emas) in enumerate(zip(self.param_groups, self._ema_groups)):
            self._check_options(group)
            for pi, p in enumerate(group["params"]):
                index += 1
                g = p.grad
                if g is None:
                    continue
                if device is None:
                    device = p.device
                self._check_tensor(p, "the data", index, device)
                self._check_tensor(g, "the gradient", index, device)
                if g.shape != p.shape:
                    raise RuntimeError(f"AdamW: the gradient of parameter {index} has shape {tuple(g.shape)}")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if st["step"].device.type != "cpu":  # (a checkpoint of a capturable / fused torch optimizer)
                    st["step"] = st["step"].detach().to("cpu", torch.float32)
                self._check_tensor(st["exp_avg"], "exp_avg", index, device)
                self._check_tensor(st["exp_avg_sq"], "exp_avg_sq", index, device)
                e = None
                if emas is not None:
                    e = emas[pi]
                    self._check_tensor(e, "the EMA tensor", index, device)
                steps.append(st["step"])
                if p.numel() == 0:
                    continue
                grads.append(g)
                rows.setdefault((gi, int(st["step"].item())), []).append((p, g, st["exp_avg"], st["exp_avg_sq"], e))
        self._classes, self._steps, self._keep = [], steps, rows
        if not rows:
            return
        tensors, chunks, spans = [], [], []
        for (gi, step), members in rows.items():
            first = len(chunks)
            for p, g, m, v, e in members:
                t, n = len(tensors), p.numel()
                tensors.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0 if e is None else e.data_ptr(), n))
                chunks.extend((t, s, min(CHUNK, n - s)) for s in range(0, n, CHUNK))
            spans.append((gi, step, first, len(chunks)))
        # the norm pass sees consecutive slices of ONE buffer (the U-Net's flat gradient) as one tensor; tensors with storage
        # of their own are never merged, whatever their addresses, so the summation order depends on the program alone
        runs: List[list] = []  # [address, numel, storage address]
        for g in grads:
            store = g.untyped_storage().data_ptr()
            if runs and runs[-1][2] == store and runs[-1][0] + 4 * runs[-1][1] == g.data_ptr():
                runs[-1][1] += g.numel()
            else:
                runs.append([g.data_ptr(), g.numel(), store])
        nchunks = [(t, s, min(CHUNK, n - s)) for t, (_, n, _) in enumerate(runs) for s in range(0, n, CHUNK)]
        host = torch.tensor([x for row in tensors for x in row] + [x for row in chunks for x in row]
                            + [r[0] for r in runs] + [r[1] for r in runs] + [x for row in nchunks for x in row],
                            dtype=torch.int64)
        tab = host.to(device)
        a = 6 * len(tensors)
        b = a + 3 * len(chunks)
        c = b + len(runs)
        d = c + len(runs)
        self._tensors = tab[:a].view(-1, 6)
        all_chunks = tab[a:b].view(-1, 3)
        self._norm_ptrs, self._norm_numels, self._norm_chunks = tab[b:c], tab[c:d], tab[d:].view(-1, 3)
        for gi, step, first, last in spans:
            cls = _Class()
            cls.group, cls.step, cls.chunks = self.param_groups[gi], step, all_chunks[first:last]
            self._classes.append(cls)
        if self.max_grad_norm is not None:
            if self.grad_norm is None or self.grad_norm.device != device:
                self.grad_norm = torch.zeros((), dtype=torch.float32, device=device)
                self._partials = torch.zeros(1024, dtype=torch.float64, device=device)
        self.table_builds += 1

    # ------------------------------------------------------------------ the step
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        try:
            sig = self._signature()
        except RuntimeError:  # (a sparse gradient has no data pointer)
            sig = None
        if sig is None or sig != self._sig:
            self._build()
            self._sig = self._signature()
        if not self._classes:
            return loss
        partials, n_partials, max_norm = None, 0, 0.0
        if self.max_grad_norm is not None:
            partials, max_norm = self._partials, self.max_grad_norm
            n_partials = ops.sqnorm_partials(self._norm_ptrs, self._norm_numels, self._norm_chunks, partials)
        ema_w = 0.0 if self.ema_decay is None else 1.0 - self.ema_decay
        norm_out = self.grad_norm
        for cls in self._classes:
            group = cls.group
            cls.step += 1
            lr, (beta1, beta2) = float(group["lr"]), group["betas"]
            beta1, beta2 = float(beta1), float(beta2)
            bc1 = 1.0 - beta1 ** cls.step
            bc2 = 1.0 - beta2 ** cls.step
            ops.adamw_step(self._tensors, cls.chunks, decay=1.0 - lr * float(group["weight_decay"]),
                           one_minus_beta1=1.0 - beta1, beta2=beta2, one_minus_beta2=1.0 - beta2,
                           inv_bc2_sqrt=1.0 / math.sqrt(bc2), eps=float(group["eps"]), step_size=lr / bc1, ema_weight=ema_w,
                           partials=partials, n_partials=n_partials, max_grad_norm=max_norm, grad_norm_out=norm_out)
            norm_out = None  # (one writer is enough)
        torch._foreach_add_(self._steps, 1)
        return loss
