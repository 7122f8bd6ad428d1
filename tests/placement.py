"""Operand placement for C-ABI tests: every operand is a view into a backing buffer of its own,

    [ guard | offset elements | payload | guard ]

so that a test chooses each pointer's alignment (offset 0-3 elements of the operand's own type from a 64-byte
aligned base) and sees everything a kernel touches outside its operands.  Guards and the offset gap hold one fixed NaN
bit pattern; input payloads hold the case's data; output and workspace payloads hold a second NaN pattern, so an
element the entry point promised to write and did not is caught as well.  `Arena.verify()` compares bit patterns
(int32 words; bytes for one-byte types), never floats: a NaN compares unequal to itself.

A guard is at least 1024 floats (4 KiB).  That is a condition, not a tuned value: an overrun by a whole wave row of
16-byte stores (64 lanes x 16 B = 1 KiB), before or behind the payload, still lands inside memory the test owns -- a
defect is observed and reported, it never becomes a GPU fault.

Below `Arena`, the harness the placement test files share: `Placer` (the operands of one call in declaration order, each at
the offset a plan gives it), the plans, `place_and_check` and the two parametrized tests every header's file instantiates.
"""
import ctypes

import pytest
import torch

from audio_diffusion_pytorch_amd import _C
from conftest import rel_err

GUARD_BYTES = 4096
assert GUARD_BYTES >= 1024 * 4 and GUARD_BYTES >= 4 * 64 * 16
GUARD_WORD = 0x7FC0DEAD          # quiet NaN, payload 0xDEAD: guards and offset gaps
UNWRITTEN_WORD = 0x7FC0BEEF      # quiet NaN, payload 0xBEEF: outputs and workspaces before the call
UNWRITTEN_F64 = 0x7FF8BEEF7FC0BEEF  # a NaN double whose two int32 halves are NaNs / the float pattern (low word)
MAX_OFFSET = 3


class PlacementError(AssertionError):
    pass


class _Operand:
    __slots__ = ("name", "role", "offset", "backing", "snapshot", "lo", "hi", "view", "written")


def _words(t: torch.Tensor) -> torch.Tensor:
    """The bits of a 1-D uint8 tensor as int32 words where its length and start allow, else as bytes."""
    if t.numel() % 4 == 0 and t.storage_offset() % 4 == 0:
        return t.view(torch.int32)
    return t


class Arena:
    """Hands out operands of one C-ABI call; `verify()` after the call (it synchronises by reading the buffers)."""

    def __init__(self, dev):
        self.dev = torch.device(dev)
        self.ops = {}

    # ---- placing
    def _place(self, name: str, role: str, shape, dtype, offset: int, data=None, written=None) -> torch.Tensor:
        if name in self.ops:
            raise ValueError(f"operand {name!r} placed twice")
        if not 0 <= offset <= MAX_OFFSET:
            raise ValueError(f"offset {offset} outside 0..{MAX_OFFSET}")
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        item = torch.empty((), dtype=dtype).element_size()
        lo = GUARD_BYTES + offset * item
        hi = lo + numel * item
        total = (hi + GUARD_BYTES + 63) // 64 * 64
        host = torch.empty(total, dtype=torch.uint8)
        assert host.data_ptr() % 4 == 0
        host.view(torch.int32).fill_(GUARD_WORD)
        payload = host[lo:hi]
        if data is not None:
            src = data.detach().to("cpu", dtype).contiguous()
            if tuple(src.shape) != shape:
                raise ValueError(f"{name}: data of shape {tuple(src.shape)} for an operand of shape {shape}")
            payload.copy_(src.reshape(-1).view(torch.uint8))
        elif dtype == torch.float64:
            payload.view(torch.int64).fill_(UNWRITTEN_F64)
        elif item == 4:
            payload.view(torch.int32).fill_(UNWRITTEN_WORD)
        else:
            raise ValueError(f"{name}: no 'unwritten' pattern for outputs of type {dtype}")
        op = _Operand()
        op.name, op.role, op.offset, op.lo, op.hi = name, role, offset, lo, hi
        op.backing = host.to(self.dev)
        assert op.backing.data_ptr() % 64 == 0, "backing buffers are expected to start 64-byte aligned"
        op.snapshot = host.clone()   # (.to() of a CPU tensor to the CPU is the tensor itself)
        op.view = op.backing[lo:hi].view(dtype).view(shape)
        if written is not None:
            written = written.to("cpu", torch.bool).reshape(-1)
            assert written.numel() == numel
        op.written = written
        self.ops[name] = op
        return op.view

    def input(self, name: str, data: torch.Tensor, offset: int = 0, dtype=None) -> torch.Tensor:
        """A read-only operand: verify() wants its payload bit-identical afterwards."""
        return self._place(name, "in", data.shape, dtype or data.dtype, offset, data=data)

    def inout(self, name: str, data: torch.Tensor, offset: int = 0) -> torch.Tensor:
        """An operand the call reads and rewrites (accumulated gradients, state): only its surroundings are checked."""
        return self._place(name, "inout", data.shape, data.dtype, offset, data=data)

    def output(self, name: str, shape, offset: int = 0, dtype=torch.float32, written=None) -> torch.Tensor:
        """An operand the call must write.  `written`: bool mask (same shape) of the elements the entry point promises to
        write -- default all; the others (row-stride gaps) must keep the 'unwritten' pattern."""
        return self._place(name, "out", shape, dtype, offset, written=written)

    def workspace(self, name: str, numel: int, offset: int = 0, dtype=torch.float32) -> torch.Tensor:
        """Scratch: the call may write any part of it."""
        return self._place(name, "ws", (numel,), dtype, offset)

    # ---- checking
    @staticmethod
    def _span(bad: torch.Tensor):
        idx = bad.nonzero().reshape(-1)
        return int(idx[0]), int(idx[-1]), int(idx.numel())

    def verify(self, refused: bool = False) -> None:
        """`refused`: the call answered an error code, so it must have written nothing at all -- outputs included."""
        problems = []
        for op in self.ops.values():
            now = op.backing.cpu()
            was = op.snapshot
            unit = "int32 word" if (op.lo % 4 == 0 and op.hi % 4 == 0) else "byte"
            for side, a, b in (("before", 0, op.lo), ("after", op.hi, now.numel())):
                n, w = _words(now[a:b]), _words(was[a:b])
                if unit == "byte":
                    n, w = now[a:b], was[a:b]
                bad = n != w
                if bad.any():
                    first, last, cnt = self._span(bad)
                    if side == "before":  # count back from the payload's first element
                        total = bad.numel()
                        first, last = first - total, last - total
                    problems.append(f"operand {op.name!r} (offset {op.offset}): guard {side} the payload touched, {cnt} "
                                    f"{unit}(s), first index {first}, last index {last} relative to the payload's "
                                    f"{'start' if side == 'before' else 'end'}")
            pn, pw = now[op.lo:op.hi], was[op.lo:op.hi]
            item = op.view.element_size()
            if op.role == "in":
                bad = _words(pn) != _words(pw) if unit != "byte" else pn != pw
                if bad.any():
                    first, last, cnt = self._span(bad)
                    problems.append(f"operand {op.name!r} (offset {op.offset}): input payload changed, {cnt} {unit}(s), "
                                    f"first index {first}, last index {last}")
            elif op.role == "out":
                # per element: does it still hold the 'unwritten' pattern?
                if item == 8:
                    still = pn.view(torch.int64) == UNWRITTEN_F64
                else:
                    still = pn.view(torch.int32) == UNWRITTEN_WORD
                must = op.written if op.written is not None else torch.ones_like(still)
                if refused:
                    must = torch.zeros_like(still)
                bad = still & must
                if bad.any():
                    first, last, cnt = self._span(bad)
                    problems.append(f"operand {op.name!r} (offset {op.offset}): {cnt} output element(s) left unwritten, "
                                    f"first index {first}, last index {last}")
                bad = ~still & ~must
                if bad.any():
                    first, last, cnt = self._span(bad)
                    problems.append(f"operand {op.name!r} (offset {op.offset}): {cnt} element(s) outside the promised "
                                    f"output written, first index {first}, last index {last}")
        if problems:
            raise PlacementError("\n".join(problems))


# =====================================================================================================================
# The harness of the placement test files
# =====================================================================================================================
ERR_ALIGN = -3
OUTPUT_ROLES = ("out", "inout")
# (entry point, operand) -> bytes: the alignment requirements the headers state.  A placed call may answer ADP_ERR_ALIGN when
# one of these operands is placed off that boundary, and only then; every other pointer takes the alignment of its type.
ALIGN_DOCUMENTED = {("adp_conv1d", "gnb_ab"): 8}

# the whole-call plans: `plan(i, name, role)` gives operand i of the call its offset in elements of its own type
PLANS = {"zero": lambda i, n, r: 0, "all1": lambda i, n, r: 1, "mixed": lambda i, n, r: 1 + i % 3}


def single(target, k):
    return lambda i, n, r: k if n == target else 0


def single_plans(operands):
    """(plan, label) of the single-operand placements: each pointer operand alone at offset 1, each output alone at offset 2
    (the 8-byte phase)."""
    for name, role in operands:
        yield single(name, 1), f"{name}@1"
        if role in OUTPUT_ROLES:
            yield single(name, 2), f"{name}@2"


def p(t):
    return None if t is None else _C.ptr(t, t.dtype)


class AlignRefused(Exception):
    pass


class Placer:
    """Places the operands of one call in declaration order; `plan(i, name, role)` gives operand i its offset."""

    def __init__(self, dev, plan):
        self.arena, self.plan, self.operands, self.notes = Arena(dev), plan, [], {}

    def _off(self, name, role):
        i = len(self.operands)
        self.operands.append((name, role))
        return self.plan(i, name, role)

    def inp(self, name, data, res=False):
        return self.arena.input(name, data, self._off(name, "res" if res else "in"))

    def inout(self, name, data):
        return self.arena.inout(name, data, self._off(name, "inout"))

    def out(self, name, shape, dtype=torch.float32, written=None):
        return self.arena.output(name, shape, self._off(name, "out"), dtype, written)

    def ws(self, name, nbytes, dtype=torch.float32):
        """A workspace of `nbytes` BYTES, as a *_ws_bytes query answers (rounded up to whole elements, at least one)."""
        item = torch.empty((), dtype=dtype).element_size()
        return self.ws_numel(name, max(1, (nbytes + item - 1) // item), dtype)

    def ws_numel(self, name, numel, dtype=torch.float32):
        """A workspace of `numel` ELEMENTS."""
        return self.arena.workspace(name, numel, self._off(name, "ws"), dtype)

    def off_boundary(self, entry):
        """The placed operands of `entry` whose documented alignment (ALIGN_DOCUMENTED) this placement violates."""
        return [o for (e, o), nbytes in ALIGN_DOCUMENTED.items()
                if e == entry and o in self.arena.ops and self.arena.ops[o].view.data_ptr() % nbytes]

    def ok(self, code, entry, launched=None):
        bad = self.off_boundary(entry)
        if bad:  # the header names the requirement on these operands: the call must refuse, not run a misaligned access
            assert code == ERR_ALIGN, f"{entry} returned {code} with {bad} off the boundary adp.h documents"
            assert not launched, f"{entry} refused the call and still launched {launched}"
            raise AlignRefused(f"{entry}: {bad}")
        assert code == 0, f"{entry} returned {code} ({_C.ERRORS.get(code, '?')})"

    def call(self, entry, fn):
        """`ok(fn(), entry)` with the kernel instantiations the call launched recorded in notes["kernels"] (adp_launch_trace;
        the names rocprofv3 reports)."""
        lib = _C.lib()
        lib.adp_launch_trace(1, None, 0)
        try:
            code = fn()
        finally:
            buf = ctypes.create_string_buffer(4096)
            lib.adp_launch_trace(0, buf, 4096)
            lib.adp_launch_times(None, 0)   # (drops the events the trace recorded)
        names = _C._decode_trace(buf.value.decode())
        self.notes["kernels"] = (self.notes.get("kernels", "") + " | " + names).strip(" |")
        self.ok(code, entry, names)

    def val(self, v, entry):
        assert v > 0, f"{entry} returned {v} ({_C.ERRORS.get(v, '?')})"
        return int(v)


# A case function `run(P)` places its operands, makes the call and returns (code, figures); a figure is
# (label, err, op, bound) with op "<" or "<=", made by one of:
def close(label, got, want, bound):
    """rel_err(got, want) < bound"""
    return label, rel_err(got, want), "<", bound


def exact(label, got, want):
    """got and want bit-identical"""
    return label, 0.0 if torch.equal(got.cpu(), want.cpu()) else float("inf"), "<=", 0.0


def place_and_check(dev, entry, label, run, plan, what):
    """One placed call: it must return ADP_OK, every figure must hold and verify() must find nothing; returns the Placer."""
    P = Placer(dev, plan)
    code, figures = run(P)
    assert code == 0, f"{entry} {label} [{what}] returned {code} ({_C.ERRORS.get(code, '?')})"
    problems = []
    for name, err, op, bound in figures:
        print(f"{entry} {label} [{what}] {name}: {err:.3e} (bound: {op} {bound:.3e})")
        assert op in ("<", "<=")
        if not (err < bound if op == "<" else err <= bound):
            problems.append(f"{name}: {err:.3e} is not {op} {bound:.3e}")
    P.arena.verify()   # raises PlacementError naming the operand and the span
    assert not problems, f"{entry} {label}, placement {what}:\n" + "\n".join(problems)
    return P


# What a header's file instantiates.  `cases`: case name -> (run(P, x), the entry point it places); `pairs`: the (case name,
# key) combinations to run, `arg(key)` being the x of that key (a geometry, a shape, a length: the file's parameter axis).
def _placed(cases, arg, dev, name, where, plan, what):
    run, entry = cases[name]
    return place_and_check(dev, entry, f"({name}) {where}", lambda P: run(P, arg(where)), plan, what)


def _ids(pairs):
    return [f"{name}-{where}" for name, where in pairs]


def whole_call_tests(cases, pairs, arg):
    @pytest.mark.parametrize("kind", list(PLANS))
    @pytest.mark.parametrize("name,where", pairs, ids=_ids(pairs))
    def test_whole_call_placements(dev, name, where, kind):
        _placed(cases, arg, dev, name, where, PLANS[kind], kind)
    return test_whole_call_placements


def single_operand_tests(cases, pairs, arg):
    @pytest.mark.parametrize("name,where", pairs, ids=_ids(pairs))
    def test_single_operand_placements(dev, name, where):
        """single1: each pointer operand alone at offset 1; single2: each output alone at offset 2 (the 8-byte phase)."""
        base = _placed(cases, arg, dev, name, where, PLANS["zero"], "zero")
        for plan, what in single_plans(base.operands):
            _placed(cases, arg, dev, name, where, plan, what)
    return test_single_operand_placements
