"""What the hipGraph-replayed steps share -- the training step (graphed.py), the samplers and the inpainter (diffusion.py,
ar.py), the data-parallel step (parallel.py) -- so that each rule lives once: a step is captured per call STRUCTURE and owns
static copies of its kwarg tensors; a graph holds the parameters' addresses, so an entry whose parameters moved is dropped,
never replayed, and it keeps the context-bank tables it was captured with alive; entries own their activations, so the caches
are LRU-bounded; a step runs eagerly on a side stream before it is captured.  The cache keys, what an entry holds besides
`CapturedStep`'s fields and the capture itself (error mode, pool, generator state) stay with the owners, which differ there.
Imports none of the modules that use it."""
from collections import OrderedDict
from typing import Any, Callable, Dict, List

import torch
import torch.nn as nn
from torch import Tensor


def kw_spec(value, tensors: List[Tensor]):
    """Hashable structure of a forward kwarg (names / shapes / dtypes / python scalars -- never object identity);
    the tensors it holds are appended to `tensors` in traversal order.  None when it cannot be made static."""
    if isinstance(value, Tensor):
        tensors.append(value)
        return ("T", tuple(value.shape), value.dtype, value.device)
    if value is None or isinstance(value, (bool, int, float)):
        return ("S", type(value).__name__, value)
    # (strings are NOT static: a net that takes text runs a host-side tokenizer + H2D copy per call, which is illegal
    # inside stream capture; our own TextConditioningNet resolves text to a tensor before the loop instead)
    if isinstance(value, (list, tuple)):
        items = tuple(kw_spec(v, tensors) for v in value)
        return None if any(i is None for i in items) else ("L", type(value).__name__, items)
    return None


def kw_rebuild(value, it):
    """The same structure with every tensor replaced by the next one from `it` (the cache entry's static copy)."""
    if isinstance(value, Tensor):
        return next(it)
    if isinstance(value, (list, tuple)):
        return type(value)(kw_rebuild(v, it) for v in value)
    return value


def kwarg_structure(kwargs: Dict[str, Any], accept: Callable[[Tensor], bool]):
    """None (the caller runs eagerly) when a kwarg cannot be made static or holds a tensor that `accept` refuses, else
    (names, live, specs): the sorted kwarg names, the caller's kwarg tensors in traversal order, and the hashable
    (name, kw_spec) pairs that the owner builds its cache key from."""
    names = sorted(kwargs)
    live: List[Tensor] = []
    specs = tuple((k, kw_spec(kwargs[k], live)) for k in names)
    if any(sp is None for _, sp in specs) or not all(accept(t) for t in live):
        return None
    return names, live, specs


def static_kwargs(kwargs: Dict[str, Any], names, live: List[Tensor]):
    """Static copies of the kwarg tensors (filled with the caller's values) and the kwargs rebuilt around them."""
    statics = [t.detach().clone(memory_format=torch.contiguous_format) for t in live]
    it = iter(statics)
    return statics, {k: kw_rebuild(kwargs[k], it) for k in names}


def tracked_parameters(module: nn.Module) -> List[nn.Parameter]:
    """`list(module.parameters())` without the module-tree walk (1-2 ms for ~600 parameters) on every call: the list is cached
    on the module together with where each entry is registered and re-validated by identity per call (~30 us); replaced
    Parameter objects (load_state_dict(assign=True), to_empty, ...) or a changed parameter count rebuild it."""
    cache = module.__dict__.get("_adp_param_cache")
    if cache is not None:
        params, holders = cache
        for p, (d, leaf) in zip(params, holders):
            if d.get(leaf) is not p:
                cache = None
                break
    if cache is None:
        params, holders, seen = [], [], set()
        for mod in module.modules():
            for leaf, p in mod._parameters.items():
                if p is not None and id(p) not in seen:
                    seen.add(id(p))
                    params.append(p)
                    holders.append((mod._parameters, leaf))
        module.__dict__["_adp_param_cache"] = (params, holders)
    return params


def param_signature(params) -> tuple:
    """What a captured graph assumes about the parameters: their addresses and whether they are differentiated."""
    return tuple((p.data_ptr(), p.requires_grad) for p in params)


def ctx_tables_under(module: nn.Module) -> list:
    """The context-bank pointer tables (attention.CtxBank) of every net under `module`.  A graph captured over such a net reads
    them by address, so every captured entry holds the ones it was captured with: a net rebuilds its tables when its
    parameters move, and the old ones must outlive every graph that still points at them."""
    return [t for m in module.modules() if (t := m.__dict__.get("_ctx_tables")) is not None]


class StepCache(OrderedDict):
    """Captured steps by call-structure key, least recently used first.  An entry is any object with a `.psig`, the
    parameter signature it was captured under."""

    def fetch(self, key, psig):
        """The entry under `key`, made the most recently used one, or None.  An entry captured under another parameter
        signature is dropped here (its graph holds stale addresses): never replayed."""
        entry = self.get(key)
        if entry is not None and entry.psig != psig:
            del self[key]
            return None
        if entry is not None:
            self.move_to_end(key)
        return entry

    def store(self, key, entry, bound: int) -> None:
        """`entry` as the most recently used of at most `bound`: the least recently used graphs go, with their buffers."""
        self[key] = entry
        while len(self) > bound:
            self.popitem(last=False)


class CapturedStep:
    """A sampler's cache entry: the graph of one step in place on the static x `sx`, the static kwarg tensors, the
    parameter signature and the context-bank tables at capture (held, not read), and the owner's own static tensors by name."""

    def __init__(self, graph, sx: Tensor, statics: List[Tensor], psig: tuple, tables: list, **own):
        self.graph, self.sx, self.statics, self.psig, self.tables = graph, sx, statics, psig, tables
        self.__dict__.update(own)


def warm_up(fn: Callable[[], Any], device=None) -> None:
    """Runs `fn()` on a fresh side stream of `device` (None = the current device) behind that device's current stream, then
    makes the current stream wait for it: the eager run in front of a capture (allocator pools, lazily built tables,
    communicators), kept off the stream that is about to be captured."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(device).wait_stream(side)
