"""The staleness rule of the host-side table caches, stated once.

A derived table (slot tables, pair masks, index tables, device copies, kernel specs) is kept on the object that uses it, next
to what it was derived from.  An entry HOLDS its sources, so neither an ``id`` nor a device address can be handed out again
while it lives; sources are compared by identity and by the ``_version`` they had when the entry was made (an object without a
version counter, such as ``GroupTables``, by identity alone), everything else (``extras``) by value.
"""
from __future__ import annotations


def cached(holder, slot: str, sources: tuple, extras: tuple, build, ways: int = 1):
    """The value ``build()`` made for these ``sources`` (tensors or plain objects, ``None`` allowed) and ``extras``, kept in
    ``holder.<slot>``: the stored object itself on a hit, else a fresh one, stored in front of the ``ways - 1`` most recently
    used other entries."""
    entries = getattr(holder, slot, None) or ()
    for i, (held, versions, kept, value) in enumerate(entries):
        if kept == extras and len(held) == len(sources):
            for h, v, s in zip(held, versions, sources):
                if h is not s or v != getattr(s, "_version", None):
                    break
            else:
                if i:
                    object.__setattr__(holder, slot, (entries[i],) + entries[:i] + entries[i + 1:])
                return value
    versions = tuple(getattr(s, "_version", None) for s in sources)
    value = build()
    # (object.__setattr__: an nn.Module holder must not try to register what the entry holds)
    object.__setattr__(holder, slot, ((tuple(sources), versions, extras, value),) + entries[:ways - 1])
    return value
