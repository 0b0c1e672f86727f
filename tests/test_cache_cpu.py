"""The staleness rule of the host-side table caches (scaleprotoseg_amd/_cache.py), on the helper alone: hits return the stored
object, every kind of edit of a source or an extra misses, and an entry keeps its sources alive."""
import gc
import weakref

import torch

from scaleprotoseg_amd._cache import cached


class _Holder:
    pass


class _Counted:
    """A build() that counts its calls and returns a fresh object every time."""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return object()


def test_a_hit_returns_the_stored_object_without_building():
    h, build, t = _Holder(), _Counted(), torch.zeros(2, 2)
    v = cached(h, "_c", (t,), (3, "cpu"), build)
    assert cached(h, "_c", (t,), (3, "cpu"), build) is v and build.calls == 1
    assert cached(h, "_other", (t,), (3, "cpu"), build) is not v and build.calls == 2      # slots are independent


def test_every_kind_of_edit_misses():
    h, build, t = _Holder(), _Counted(), torch.zeros(2, 2)
    v = cached(h, "_c", (t, None), (1,), build)
    t[0, 0] = 1                                                    # in place: the version counter moves
    v1 = cached(h, "_c", (t, None), (1,), build)
    assert v1 is not v and build.calls == 2
    c = t.clone()                                                  # equal values, another object
    v2 = cached(h, "_c", (c, None), (1,), build)
    assert v2 is not v1 and build.calls == 3
    v3 = cached(h, "_c", (c, None), (2,), build)                   # a changed extra
    assert v3 is not v2 and build.calls == 4
    v4 = cached(h, "_c", (c, torch.zeros(1)), (2,), build)         # None turning into a tensor
    assert v4 is not v3 and build.calls == 5
    assert cached(h, "_c", (c, None), (2,), build) is not v3 and build.calls == 6          # one way: v3's entry was replaced


def test_an_entry_keeps_its_source_alive_until_it_is_replaced():
    h, build = _Holder(), _Counted()
    t = torch.zeros(3)
    ref = weakref.ref(t)
    cached(h, "_c", (t,), (), build)
    del t
    gc.collect()
    assert ref() is not None                                       # neither its id nor its address can be handed out again
    assert cached(h, "_c", (ref(),), (), build) is not None and build.calls == 1
    cached(h, "_c", (torch.zeros(3),), (), build)                  # a miss on another source overwrites the slot
    gc.collect()
    assert ref() is None and build.calls == 2


def test_ways_keep_the_most_recently_used_entries():
    h, build = _Holder(), _Counted()
    ts = [torch.zeros(1) for _ in range(5)]
    vs = [cached(h, "_c", (t,), (), build, ways=4) for t in ts[:4]]
    assert [cached(h, "_c", (t,), (), build, ways=4) for t in ts[:4]] == vs and build.calls == 4
    cached(h, "_c", (ts[1],), (), build, ways=4)                   # use order, oldest first: 0 2 3 1
    v4 = cached(h, "_c", (ts[4],), (), build, ways=4)              # evicts 0 and no other
    assert build.calls == 5
    assert [cached(h, "_c", (t,), (), build, ways=4) for t in (ts[2], ts[3], ts[1], ts[4])] == [vs[2], vs[3], vs[1], v4]
    assert build.calls == 5
    assert cached(h, "_c", (ts[0],), (), build, ways=4) is not vs[0] and build.calls == 6


def test_an_unversioned_source_hits_by_identity():
    h, build = _Holder(), _Counted()
    a, b = _Holder(), _Holder()
    v = cached(h, "_c", (a,), (), build)
    assert cached(h, "_c", (a,), (), build) is v and build.calls == 1
    assert cached(h, "_c", (b,), (), build) is not v and build.calls == 2


def test_a_module_holder_registers_nothing():
    m, t = torch.nn.Linear(2, 2), torch.nn.Parameter(torch.zeros(2))
    n = len(list(m.parameters()))
    v = cached(m, "_c", (t,), (), lambda: torch.nn.Linear(1, 1))
    assert cached(m, "_c", (t,), (), lambda: None) is v
    assert len(list(m.parameters())) == n and len(list(m.children())) == 0 and "_c" not in m.state_dict()
