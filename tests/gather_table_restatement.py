"""Loop restatement of ``scaleprotoseg_amd.functional.class_gather_table``, prototype by prototype - the definition its vectorised
form is held to, bit for bit, rows with several ones included.

    class of p   the argmax of row p of the identity [P, K]; none when the row's sum is not positive
    slot of p    the number of earlier prototypes of the same class
    table[c, j]  the prototype of (class c, slot j), -1 where the class has fewer; J = the largest count, at least 1
    keys         per panel of the plan, in its padded row order (32 npb rows a panel): (class << 16) | slot of the row's
                 prototype, -1 for a prototype without class and for padding; int32
"""
from __future__ import annotations

import torch


def class_gather_table(plan, prototype_class_identity: torch.Tensor):
    """(keys int32, J, table int64 [K, J]) on the host for the panel plan ``plan`` (``BankLayout.plan()``)."""
    ident = prototype_class_identity.detach().cpu()
    P, K = ident.shape
    has = ident.sum(dim=1) > 0
    cls = torch.where(has, ident.argmax(dim=1), torch.full((P,), -1, dtype=torch.long))
    slot = torch.zeros(P, dtype=torch.long)
    counts = [0] * K
    for p in range(P):
        c = int(cls[p])
        if c >= 0:
            slot[p] = counts[c]
            counts[c] += 1
    J = max(1, max(counts) if counts else 1)
    table = torch.full((K, J), -1, dtype=torch.long)
    for p in range(P):
        if int(cls[p]) >= 0:
            table[int(cls[p]), int(slot[p])] = p
    rows = plan.npb * 32
    keys = torch.full((plan.npanels * rows,), -1, dtype=torch.int64)
    for q in range(plan.npanels):
        p0, n = plan.panel_p0[q], plan.panel_np[q]
        for r_ in range(n):
            p = p0 + r_
            if int(cls[p]) >= 0:
                keys[q * rows + r_] = (int(cls[p]) << 16) | int(slot[p])
    keys = torch.where(keys < 0, torch.full_like(keys, 0xFFFFFFFF), keys)
    keys32 = (keys & 0xFFFFFFFF).to(torch.int64)
    keys32 = torch.where(keys32 >= 2**31, keys32 - 2**32, keys32).to(torch.int32)   # same bits as uint32
    return keys32, J, table
