"""The rules every replayed step shares (audio_diffusion_pytorch_amd/capture.py), on the host: the LRU cache of captured steps
and the call structure of forward kwargs.  No kernel library, no GPU."""
import torch

from audio_diffusion_pytorch_amd.capture import StepCache, kw_rebuild, kw_spec, kwarg_structure, static_kwargs


class _Stub:
    def __init__(self, psig):
        self.psig = psig


def test_step_cache_hit_is_most_recent():
    cache = StepCache()
    a, b = _Stub("p"), _Stub("p")
    cache.store((1,), a, 4)
    cache.store((2,), b, 4)
    assert list(cache) == [(1,), (2,)]
    assert cache.fetch((1,), "p") is a
    assert list(cache) == [(2,), (1,)]
    assert cache.fetch((3,), "p") is None and list(cache) == [(2,), (1,)]


def test_step_cache_drops_an_entry_of_another_signature():
    cache = StepCache()
    cache.store((1,), _Stub("old"), 4)
    cache.store((2,), _Stub("old"), 4)
    assert cache.fetch((1,), "new") is None
    assert (1,) not in cache and list(cache) == [(2,)]


def test_step_cache_evicts_the_least_recently_used():
    cache = StepCache()
    entries = [_Stub("p") for _ in range(5)]
    for i in range(4):
        cache.store((i,), entries[i], 4)
    assert cache.fetch((1,), "p") is entries[1]   # just fetched: not the one to go
    cache.store((4,), entries[4], 4)
    assert len(cache) == 4 and (0,) not in cache, "the first stored entry goes"
    assert list(cache) == [(2,), (3,), (1,), (4,)]


def _accept(t):
    return True


def test_nested_kwarg_round_trips_through_static_copies():
    t0, t1, t2 = torch.arange(6.0).view(2, 3), torch.arange(4).view(4, 1).expand(4, 2), torch.ones(1)
    kwargs = {"channels": [t0, (t1, 3), None], "scale": 2.5, "embedding": t2}
    names, live, specs = kwarg_structure(kwargs, _accept)
    assert names == ["channels", "embedding", "scale"] and [k for k, _ in specs] == names
    assert len(live) == 3 and live[0] is t0 and live[1] is t1 and live[2] is t2   # traversal order over sorted names
    hash(specs)
    statics, skw = static_kwargs(kwargs, names, live)
    assert all(s is not t and torch.equal(s, t) and s.is_contiguous() for s, t in zip(statics, live))
    assert list(skw) == names and skw["scale"] == 2.5 and type(skw["scale"]) is float
    ch = skw["channels"]
    assert type(ch) is list and type(ch[1]) is tuple and ch[1][1] == 3 and type(ch[1][1]) is int and ch[2] is None
    assert ch[0] is statics[0] and ch[1][0] is statics[1] and skw["embedding"] is statics[2]
    assert kw_spec(skw["channels"], []) == kw_spec(kwargs["channels"], [])
    # kw_rebuild alone: the same containers around whatever the iterator yields
    assert kw_rebuild([t0, (t1, 3), None], iter(["a", "b"])) == ["a", ("b", 3), None]


def test_strings_cannot_be_made_static():
    assert kwarg_structure({"text": "abc"}, _accept) is None
    assert kwarg_structure({"x": torch.ones(2), "text": [torch.ones(1), "abc"]}, _accept) is None
    assert kw_spec("abc", []) is None and kw_spec(["a", "b"], []) is None


def test_refused_tensor_gives_none():
    assert kwarg_structure({"x": [torch.ones(2)]}, lambda t: t.is_cuda) is None
    assert kwarg_structure({"x": 3}, lambda t: t.is_cuda) is not None   # (no tensor: nothing to refuse)


def test_specs_follow_structure_not_values():
    def specs(**kw):
        return kwarg_structure(kw, _accept)[2]
    assert specs(c=[torch.zeros(2, 3), (torch.ones(4), 3)]) == specs(c=[torch.randn(2, 3), (torch.full((4,), 7.0), 3)])
    assert specs(c=[torch.zeros(2, 3), (torch.ones(4), 3)]) != specs(c=[torch.zeros(2, 3), (torch.ones(4), 4)])
    assert specs(c=torch.zeros(2, 3)) != specs(c=torch.zeros(3, 2))
    assert specs(c=torch.zeros(2)) != specs(c=torch.zeros(2, dtype=torch.float64))
    assert specs(s=1) != specs(s=1.0) and specs(s=1) != specs(s=True)
