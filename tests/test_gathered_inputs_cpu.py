"""The input layer of the class-gathered losses (scaleprotoseg_amd/_gathered.py) on the CPU, where everything it produces is exact:
the two slot rules, the four constructors of ``Gathered``, the walk hint and the one domain check.  Family: B = 2, grid 4 x 5,
K = 3, P = 7; class 1 has no prototypes, prototype 4 has no class; the label map holds 0 (void), K, K + 1, 255 and (int64) -3."""
import pytest
import torch

import scaleprotoseg_amd as spx
from oracle import ppnet_oracle as O
from scaleprotoseg_amd import _gathered as G
from scaleprotoseg_amd.loss import ActivationRegularizers, ClassDistances, KLDLoss, KLDLossGroup

from gather_table_restatement import class_gather_table as gather_table_loops

B, H, W, K, P, NG = 2, 4, 5, 3, 7, 2
HW = H * W
CLASS_OF = [0, 2, 0, 2, -1, 0, 2]


def _ident():
    ident = torch.zeros(P, K)
    for p, c in enumerate(CLASS_OF):
        if c >= 0:
            ident[p, c] = 1
    return ident


def _target(dtype=torch.int64):
    t = torch.tensor([[1, 3, 0, 1, 2], [3, 3, 1, 0, K + 1], [2, 1, 255, 3, 1], [0, 0, 3, 1, 3]], dtype=torch.int64)
    t = torch.stack([t, t.flip(0).roll(2, dims=1)])
    if dtype == torch.int64:
        t[1, 0, 0] = -3
    return t.to(dtype)


def _map():
    return torch.rand(B, P, H, W, generator=torch.Generator().manual_seed(5))


TABLE = torch.tensor([[0, 2, 5], [-1, -1, -1], [1, 3, 6]])


# ---- tables ------------------------------------------------------------------------------------------------------------
def _layouts():
    even = lambda P_, S: tuple((s * (P_ // S), (s + 1) * (P_ // S)) for s in range(S))
    yield "family", spx.BankLayout(P, K, 1, 64, ((0, P),)), _ident()
    for P_, K_, S in ((228, 19, 4), (1800, 150, 4)):
        yield f"{P_}", spx.BankLayout(P_, K_, S, 64, even(P_, S)), O.default_class_identity(P_, K_, S)


def _two_hot(ident):
    ident = ident.clone()
    ident[3, (int(ident[3].argmax()) + 1) % ident.shape[1]] = 1
    return ident


def _rows_zeroed(ident):
    ident = ident.clone()
    ident[[0, 5]] = 0
    return ident


TABLE_CASES = [(f"{name}-{vname}", lay, variant(ident)) for name, lay, ident in _layouts()
               for vname, variant in (("as_built", lambda i: i), ("rows_0_5_zero", _rows_zeroed), ("row_3_two_hot", _two_hot))]


def test_class_slot_table_is_the_oracles():
    assert torch.equal(G.class_slot_table(_ident()), TABLE)
    for _, _, ident in TABLE_CASES:
        assert torch.equal(G.class_slot_table(ident), O.class_slot_table(ident))
    assert spx.loss.class_slot_table is G.class_slot_table and spx.ClassDistances is G.ClassDistances


@pytest.mark.parametrize("case", TABLE_CASES, ids=[c[0] for c in TABLE_CASES])
def test_class_gather_table_is_the_loop_restatement(case):
    name, layout, ident = case
    keys, J, table = spx.class_gather_table(layout, ident, "cpu")
    rkeys, rJ, rtable = gather_table_loops(layout.plan(), ident)
    assert J == rJ and keys.dtype == rkeys.dtype and table.dtype == rtable.dtype
    assert torch.equal(keys, rkeys) and torch.equal(table, rtable)
    if name.startswith("1800"):
        assert layout.plan().npanels == 12
    column_wise = G.class_slot_table(ident)
    if "two_hot" not in name:                                    # one-hot or all-zero rows: the two rules agree exactly
        assert torch.equal(table, column_wise)
    else:                                                        # prototype 3 takes a slot in both classes column-wise
        assert not torch.equal(table, column_wise) and (column_wise == 3).sum() == 2 and (table == 3).sum() == 1
        if name.startswith("228"):
            assert (J, column_wise.shape[1]) == (12, 13)


# ---- the constructors --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.uint8])
def test_distance_map_constructor(dtype):
    d, t = _map(), _target(dtype)
    g = G.from_distance_map(d, t, TABLE)
    assert torch.equal(g.labels0, t.reshape(B, HW).long() - 1) and g.table is TABLE and g.poison is None
    want = O.gather_class_distances(d, t.reshape(B, HW).long() - 1, _ident()).permute(0, 2, 1)
    assert g.planes.is_contiguous() and g.planes.shape == (B, 3, HW) and torch.equal(g.planes, want)
    classed = ((g.labels0 >= 0) & (g.labels0 < K)).unsqueeze(1) & (TABLE[g.labels0.clamp(0, K - 1)] >= 0).permute(0, 2, 1)
    assert (g.planes[~classed] == 0).all() and (g.planes[classed] > 0).all()
    with pytest.raises(spx.SpxError):
        G.from_distance_map(d, t.reshape(B, HW)[:, :-1], TABLE)


@pytest.mark.parametrize("shape", ["[M, P]", "[B, HW, P]"])
def test_activation_constructor_leaves_unused_entries_unmasked(shape):
    d, t = _map(), _target()
    act = d.reshape(B, P, HW).permute(0, 2, 1).contiguous()                        # [B, HW, P], all entries > 0
    g = G.from_activations(act.reshape(-1, P) if shape == "[M, P]" else act, t, TABLE)
    lab = (t.reshape(B, HW) - 1).tolist()
    want = torch.empty(B, 3, HW)
    used = torch.zeros(B, 3, HW, dtype=torch.bool)
    for b in range(B):
        for px in range(HW):
            c = min(max(lab[b][px], 0), K - 1)                                    # what the clamped index reads
            for j in range(3):
                want[b, j, px] = act[b, px, max(int(TABLE[c, j]), 0)]
                used[b, j, px] = 0 <= lab[b][px] < K and int(TABLE[c, j]) >= 0
    assert g.planes.is_contiguous() and torch.equal(g.planes, want) and torch.equal(g.labels0, t.reshape(B, HW) - 1)
    oracle = O.gather_class_distances(d, t.reshape(B, HW) - 1, _ident()).permute(0, 2, 1)
    assert torch.equal(g.planes[used], oracle[used])
    assert (~used).any() and (g.planes[~used] != 0).all()                          # no ``where``: the kernels mask these entries
    with pytest.raises(spx.SpxError):
        G.from_activations(act[:, :-1], t, TABLE)


def test_group_constructor_list_and_concatenated():
    ident, t = _ident(), _target()
    gci = torch.zeros(2 * NG, K)                                                   # projection 0 serves class 0, projection 1 class 2
    gci[:NG, 0] = 1
    gci[NG:, 2] = 1
    proj, table = G.group_class_tables(ident, gci, NG)
    assert proj.tolist() == [0, -1, 1] and table.tolist() == [[0, 1], [-1, -1], [0, 1]]
    gen = torch.Generator().manual_seed(7)
    acts = [torch.rand(B * HW, NG, generator=gen) for _ in range(2)]
    g = G.from_groups(acts, t, proj, table)
    gc = G.from_groups(torch.cat(acts, dim=1), t, proj, table)
    assert torch.equal(g.planes, gc.planes) and torch.equal(g.labels0, gc.labels0) and g.planes.is_contiguous()
    assert torch.equal(g.labels0, t.reshape(B, HW) - 1) and g.table is table and (g.walk_w, gc.walk_w) == (W, W)
    lab, seen = (t.reshape(B, HW) - 1).tolist(), 0
    for b in range(B):
        for px in range(HW):
            c = lab[b][px]
            if 0 <= c < K and int(proj[c]) >= 0:
                assert torch.equal(g.planes[b, :, px], acts[int(proj[c])][b * HW + px])
                seen += 1
    assert seen > 0.5 * B * HW
    m = KLDLossGroup(ident, gci, NG)
    assert torch.equal(m._gathered(acts, t).planes, g.planes)
    with pytest.raises(spx.SpxError):
        G.from_groups(acts, t.reshape(B, HW)[:, :-1], proj, table)


def _cd(t, grid=(H, W)):
    planes = O.gather_class_distances(_map(), t.reshape(B, HW).long() - 1, _ident()).permute(0, 2, 1).contiguous()
    return ClassDistances(planes, (t.reshape(B, HW) - 1).int(), TABLE, grid, t, t._version)


def test_class_distances_constructor():
    t = _target()
    cd = _cd(t)
    g = G.from_class_distances(cd, t)
    assert g.planes is cd.values and g.labels0 is cd.labels and g.table is TABLE and g.poison is None and g.walk_w == W
    g = G.from_class_distances(cd, t.clone())
    assert g.planes is cd.values and torch.equal(g.labels0, t.reshape(B, HW) - 1) and g.poison.item() == 1
    other_void = t.clone()
    assert (other_void == K + 1).any() and (other_void == 255).any()
    other_void[other_void == K + 1] = 255                                          # another value for "no class"
    assert G.from_class_distances(cd, other_void).poison.item() == 1
    assert G.from_class_distances(cd, t.to(torch.int32)).poison.item() == 1
    t[0, 0, 0] = 2                                                                 # in place: class 0 -> class 1 at one pixel
    assert cd.target is t and torch.isnan(G.from_class_distances(cd, t).poison).item()
    with pytest.raises(spx.SpxError):
        G.from_class_distances(cd, t.reshape(B, HW)[:, :-1])
    on_dev = TABLE.clone()
    assert G.from_class_distances(cd, t, on_dev).table is on_dev                   # the caller's device copy


def test_walk_hint():
    assert [G.walk_width(w, 20) for w in (5, 0, 3, 20, 1)] == [5, 0, 0, 20, 1]
    t = _target()
    assert [G.from_class_distances(_cd(t, grid), t).walk_w for grid in ((H, W), (H, 0), (H, 3))] == [W, 0, 0]
    d = _map()
    assert G.from_distance_map(d, t, TABLE).walk_w == W and G.from_distance_map(d.reshape(B, P, HW), t, TABLE).walk_w == HW
    assert G.from_distance_map(d.reshape(B, P, 2, 10), t, TABLE).walk_w == 10
    act = d.reshape(B, P, HW).permute(0, 2, 1)
    assert G.from_activations(act, t, TABLE).walk_w == W and G.from_activations(act, t.reshape(B, HW), TABLE).walk_w == 0
    assert G.from_activations(act, t.reshape(B, 1, HW), TABLE).walk_w == HW and G.from_activations(act, t.reshape(1, B * H, W), TABLE).walk_w == W
    acts = [torch.zeros(B * HW, NG)] * 2
    proj, table = torch.tensor([0, -1, 1]), torch.tensor([[0, 1], [-1, -1], [0, 1]])
    assert G.from_groups(acts, t, proj, table).walk_w == W and G.from_groups(acts, t.reshape(B, HW), proj, table).walk_w == 0


# ---- the domain check ----------------------------------------------------------------------------------------------------
def _blocks(K_, J):
    """Identity with J prototypes for each of K_ classes, class-major."""
    return torch.eye(K_).repeat_interleave(J, dim=0)


def _consumers(K_, J, dtype):
    """(operator name, call) of the three consumers on a 2 x 2 image of class 1 with J slots per class, by the reference's
    argument names."""
    ident, t = _blocks(K_, J), torch.ones(1, 2, 2, dtype=torch.long)
    ranges = {0: (0, K_ * J)}
    yield "KLD loss", lambda: KLDLoss(ident, 1, ranges)(prototype_distances=torch.rand(1, K_ * J, 2, 2).to(dtype), target_labels=t)
    yield "activation losses", lambda: ActivationRegularizers(ident, 1, ranges, 1.0, 1.0, 1.0)(prototype_activations=torch.rand(4, K_ * J).to(dtype),
                                                                                           target_labels=t)
    gci = _blocks(K_, J)                                                            # projection c serves class c, J groups each
    yield "KLD loss", lambda: KLDLossGroup(torch.eye(K_), gci, J)(list_group_activation=[torch.rand(4, J).to(dtype) for _ in range(K_)], target_labels=t)


@pytest.mark.parametrize("why,K_,J,dtype", [("17 slots", 1, 17, torch.float32), ("fp64", 2, 2, torch.float64),
                                            ("LDS bound", 400, 16, torch.float32), ("CPU planes", 2, 2, torch.float32)])
def test_one_domain_check_refuses_for_all_three_consumers(why, K_, J, dtype):
    assert (K_ * J * 12 + K_ * 4 + 8 > 60 * 1024) == (why == "LDS bound")
    for op, call in _consumers(K_, J, dtype):
        with pytest.raises(spx.SpxError) as e:
            call()
        msg = str(e.value)
        assert msg.startswith(op + ": ") and "no other backend" in msg and f"(K={K_}, J={J})" in msg and str(dtype) in msg
    with pytest.raises(spx.SpxError, match="^segment_pair_sums: .*no other backend"):
        spx.loss.segment_pair_sums(torch.zeros(1, J, 4, dtype=dtype), torch.zeros(1, 4, dtype=torch.long), K_)
