"""The routing of ``forward_from_conv_features`` of the prototype-phase and the group-phase ``PPNetMultiScale``, on the CPU: the
operator calls the two model files make are replaced by stand-ins that log what they were asked for and return zero tensors of
the documented shapes (``proto_head_forward`` with its 3/4/5-entry return), as tests/test_nearest_cpu.py does for its kernels.

1. the call log of every path equals a literal table (``CALLS`` below);
2. for the same bank and flags the packed forward's log is the single-map forward's log but for the operand shapes: a
   ``PackedMaps`` takes the head branch its list form takes;
3. tuple lengths and shapes in the three tuple modes;
4. the attachments (``spx_group``, ``spx_group_wd``, ``spx_packed``, ``spx_ce``) and the ``ClassDistances`` fields, by identity
   against the tensors the stand-ins returned; per-segment outputs are views of them;
5. every refusal of the packed, ``scale_head`` and callable-similarity paths, message for message, and which fires first.

Shapes: P = 40, K = 5, S = 4, Cs = 16 (G = 3: 15 units), B = 2, grids (3, 4) and (2, 3) - the smallest at which a segment offset
and a branch can be wrong.  The ``target_labels`` paths build the class table through the host-only plan of the built library."""
import pytest
import torch

from support import group_net, proto_net

import scaleprotoseg_amd.functional as FN
import scaleprotoseg_amd.model_multiscale as MM
import scaleprotoseg_amd.model_multiscale_group as MG
from scaleprotoseg_amd.functional import FusedCrossEntropy, SpxError
from scaleprotoseg_amd.loss import ClassDistances
from scaleprotoseg_amd.msc import PackedLayout, PackedMaps

P, K, S, CS, G = 40, 5, 4, 16, 3
U, J = G * K, P // K                 # group units; slots per class of the class-gathered distances
B, GRIDS = 2, ((3, 4), (2, 3))
MODES = (dict(), dict(return_activations=True), dict(return_activations=True, return_distances=True))
WANT = ((True, False), (False, True), (True, True))      # (distances, activations) a tuple mode returns
WHO = "forward_from_conv_features(PackedMaps)"
T, F = True, False


# ---- the stand-ins -------------------------------------------------------------------------------------------------------------
class Ops:
    """``log``: one record per call - (name, operand shape, ...); ``out``: what each call returned, in step with ``log``."""

    NAMES = ("proto_head_forward", "wide_linear", "wide_group_tail", "group_exp", "cross_entropy_from_logits", "shifted_labels_i32")

    def __init__(self, monkeypatch, net):
        self.log, self.out, self.gather = [], [], None
        self._shift = FN.shifted_labels_i32
        for mod in (MM, MG):
            for name in self.NAMES:
                if hasattr(mod, name):
                    monkeypatch.setattr(mod, name, getattr(self, name))
        if hasattr(net, "_dense_group_matrix"):
            dense = net._dense_group_matrix
            monkeypatch.setattr(net, "_dense_group_matrix", lambda: self._add(("_dense_group_matrix", None), dense()))

    def _add(self, record, out):
        self.log.append(record)
        self.out.append(out)
        return out

    def proto_head_forward(self, x, bank, head, layout, *, want_distances=True, want_activations=False, epsilon=1e-4,
                           activation="log", class_gather=None, group_tail=None, ce_labels=None):
        Bx, _, H, W = x.shape
        M = Bx * H * W
        assert layout.num_prototypes == P and epsilon == 1e-4
        top = group_tail if group_tail is not None else head
        logits = torch.zeros(M, top.shape[0]) if top is not None else None
        dist = torch.zeros(Bx, P, H, W) if want_distances else None
        if class_gather is not None:
            self.gather = class_gather
            dist = torch.zeros(Bx, class_gather.width, H * W)
        out = (logits, dist, torch.zeros(M, P) if want_activations else None)
        if ce_labels is not None:
            out += (FusedCrossEntropy(torch.zeros(()), torch.zeros(M, dtype=torch.int32), ce_labels),)
        if group_tail is not None:
            out += (torch.zeros(M, head.shape[0]),)
        return self._add(("proto_head_forward", tuple(x.shape), head is not None, group_tail is not None, class_gather is not None,
                          ce_labels is not None, layout.num_classes, want_distances, want_activations, activation), out)

    def wide_linear(self, a, w):
        return self._add(("wide_linear", tuple(a.shape), w.shape[0]), torch.zeros(a.shape[0], w.shape[0]))

    def wide_group_tail(self, units, wg):
        return self._add(("wide_group_tail", tuple(units.shape), wg.shape[0]), torch.zeros(units.shape[0], wg.shape[0]))

    def group_exp(self, units):
        return self._add(("group_exp", tuple(units.shape)), torch.zeros_like(units))

    def cross_entropy_from_logits(self, logits, labels0):
        ce = FusedCrossEntropy(torch.zeros(()), torch.zeros(logits.shape[0], dtype=torch.int32), labels0)
        return self._add(("cross_entropy_from_logits", tuple(logits.shape)), ce)

    def shifted_labels_i32(self, labels, device):
        return self._add(("shifted_labels_i32", tuple(labels.shape)), self._shift(labels, device))

    def of(self, name):
        return [o for r, o in zip(self.log, self.out) if r[0] == name]

    @property
    def kernel(self):                   # the one distance launch's return
        (out,) = self.of("proto_head_forward")
        return out

    @property
    def flat_logits(self):              # [M, K]: the last product's output
        for r, o in zip(self.log[::-1], self.out[::-1]):
            if r[0] in ("wide_linear", "wide_group_tail"):
                return o
            if r[0] == "proto_head_forward":
                return o[0]

    def shapeless(self):
        return [r[:1] + r[2:] for r in self.log]


def ph(head, tail, gather, ce, rows, wd, wa, activation="log"):
    return ("proto_head_forward", head, tail, gather, ce, rows, wd, wa, activation)


DENSE = ("_dense_group_matrix",)
HEAD, UNITS, TAIL, CE = ("wide_linear", P, K), ("wide_linear", P, U), ("wide_group_tail", U, K), ("cross_entropy_from_logits", K)
LABELS = ("shifted_labels_i32",)
# (class, branch, extra) -> the calls of one forward that returns (distances: wd, activations: wa); rows without the operand shapes
CALLS = {
    ("proto", "narrow", None): lambda wd, wa: [ph(T, F, F, F, K, wd, wa)],
    ("proto", "wide", None): lambda wd, wa: [ph(F, F, F, F, 1, wd, T), HEAD],
    ("proto", "narrow", "ce"): lambda wd, wa: [LABELS, ph(T, F, F, T, K, wd, wa)],
    ("proto", "wide", "ce"): lambda wd, wa: [LABELS, ph(F, F, F, F, 1, wd, T), HEAD, CE],
    # the class-gathered distances replace the P-wide map: asked for only where distances are returned
    ("proto", "narrow", "gather"): lambda wd, wa: [LABELS] * wd + [ph(T, F, wd, F, K, F, wa)],
    ("proto", "wide", "gather"): lambda wd, wa: [LABELS] * wd + [ph(F, F, wd, F, 1, F, T), HEAD],
    ("proto", "callable", None): lambda wd, wa: [ph(F, F, F, F, 1, T, F), HEAD],
    ("proto", "scale_head", None): lambda wd, wa: [HEAD],
    ("group", "fused", None): lambda wd, wa: [DENSE, ph(T, T, F, F, U, wd, wa)],
    ("group", "wide_tail", None): lambda wd, wa: [DENSE, ph(T, F, F, F, U, wd, wa), TAIL],
    ("group", "product", None): lambda wd, wa: [DENSE, ph(F, F, F, F, 1, wd, T), UNITS, TAIL],
    ("group", "fused", "ce"): lambda wd, wa: [DENSE, LABELS, ph(T, T, F, T, U, wd, wa)],
    ("group", "wide_tail", "ce"): lambda wd, wa: [DENSE, LABELS, ph(T, F, F, F, U, wd, wa), TAIL, CE],
    ("group", "product", "ce"): lambda wd, wa: [DENSE, LABELS, ph(F, F, F, F, 1, wd, T), UNITS, TAIL, CE],
    ("group", "callable", None): lambda wd, wa: [DENSE, ph(F, F, F, F, 1, T, F), UNITS, TAIL],
    ("group", "scale_head", None): lambda wd, wa: [DENSE, UNITS, TAIL],
}
BRANCHES = {"proto": ("narrow", "wide"), "group": ("fused", "wide_tail", "product")}
CASES = [(kind, branch) for kind in BRANCHES for branch in BRANCHES[kind]]


def expected(key, mode, xshape):
    """The table's rows with the operand shapes of a forward on ``xshape`` filled in."""
    M = xshape[0] * xshape[2] * xshape[3]
    rows = []
    for r in CALLS[key](*WANT[mode]):
        shape = {"proto_head_forward": xshape, "_dense_group_matrix": None, "shifted_labels_i32": (xshape[0], M // xshape[0])}
        rows.append((r[0], shape[r[0]] if r[0] in shape else (M, r[1])) + r[(1 if r[0] in shape else 2):])
    return rows


def make(kind, branch, monkeypatch, **kw):
    """A module of ``kind`` whose width limits put it on ``branch``, and the stand-ins around it."""
    net = proto_net(P, K, S, CS, seed=0, **kw) if kind == "proto" else group_net(P, K, S, CS, G, seed=0, **kw)
    if branch == "wide":
        monkeypatch.setattr(MM, "MAX_FUSED_HEAD_ROWS", K - 1)
    if branch == "wide_tail":
        monkeypatch.setattr(MG, "MAX_FUSED_TAIL_CLASSES", K - 1)
    if branch == "product":
        monkeypatch.setattr(MG, "MAX_FUSED_HEAD_ROWS", U - 1)
    return net, Ops(monkeypatch, net)


def single_map():
    return torch.rand(B, S * CS, *GRIDS[0])


def packed_pair():
    lay = PackedLayout(B, GRIDS)
    return PackedMaps(features=torch.rand(1, S * CS, 1, lay.M), layout=lay, index=None)


def labels(grid, seed=0):
    return torch.randint(0, K + 1, (B,) + tuple(grid), generator=torch.Generator().manual_seed(seed))


def is_view(t, base, offset, shape, stride):
    return (t.data_ptr() == base.data_ptr() + offset * base.element_size() and tuple(t.shape) == tuple(shape)
            and tuple(t.stride()) == tuple(stride))


def check_group_tags(kind, branch, net, ops, logits, act):
    """``spx_group`` on the activations (one of units / exp(units), per branch) and ``spx_group_wd`` on the logits."""
    if kind != "group":
        return
    (wd,) = ops.of("_dense_group_matrix")
    tag = logits.spx_group_wd
    assert tag[0] is wd and tag[1] is net and tag[2] == tuple(gp.weight._version for gp in net.group_projection)
    if act is not None:
        units = {"fused": None, "wide_tail": ops.kernel[0], "product": ops.of("wide_linear")[0] if branch == "product" else None}
        version, u, g = act.spx_group
        assert version == act._version and u is units[branch]
        assert g is (ops.kernel[-1] if branch == "fused" else None)


def unpack(result, mode):
    assert type(result) is tuple and len(result) == (3 if mode == 2 else 2)
    wd, wa = WANT[mode]
    return result[0], result[1] if wd else None, result[-1] if wa else None


# ---- 1.-4. the single map ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", range(3))
@pytest.mark.parametrize("kind,branch", CASES)
def test_single_map(kind, branch, mode, monkeypatch):
    net, ops = make(kind, branch, monkeypatch)
    x = single_map()
    logits, dist, act = unpack(net.forward_from_conv_features(x, **MODES[mode]), mode)
    assert ops.log == expected((kind, branch, None), mode, tuple(x.shape))
    h, w = GRIDS[0]
    assert is_view(logits, ops.flat_logits, 0, (B, h, w, K), (h * w * K, w * K, K, 1))
    assert dist is (ops.kernel[1] if WANT[mode][0] else None) and act is (ops.kernel[2] if WANT[mode][1] else None)
    assert dist is None or tuple(dist.shape) == (B, P, h, w)
    assert act is None or tuple(act.shape) == (B * h * w, P)
    assert not hasattr(logits, "spx_ce") and not hasattr(logits, "spx_packed")
    check_group_tags(kind, branch, net, ops, logits, act)


@pytest.mark.parametrize("mode", range(3))
@pytest.mark.parametrize("kind,branch", CASES)
def test_single_map_with_ce_target(kind, branch, mode, monkeypatch):
    net, ops = make(kind, branch, monkeypatch)
    x, target = single_map(), labels(GRIDS[0])
    logits, dist, act = unpack(net.forward_from_conv_features(x, ce_target=target, **MODES[mode]), mode)
    assert ops.log == expected((kind, branch, "ce"), mode, tuple(x.shape))
    fused = branch in ("narrow", "fused")
    ce = ops.kernel[3] if fused else ops.of("cross_entropy_from_logits")[0]
    assert logits.spx_ce is ce and ce.target is target and ce.target_version == target._version
    (shifted,) = ops.of("shifted_labels_i32")
    assert ce.labels is shifted and shifted.dtype == torch.int32 and torch.equal(shifted, target.reshape(B, -1).int() - 1)
    check_group_tags(kind, branch, net, ops, logits, act)


@pytest.mark.parametrize("mode", range(3))
@pytest.mark.parametrize("branch", BRANCHES["proto"])
def test_single_map_with_target_labels(branch, mode, monkeypatch):
    net, ops = make("proto", branch, monkeypatch)
    x, target = single_map(), labels(GRIDS[0])
    logits, dist, act = unpack(net.forward_from_conv_features(x, target_labels=target, **MODES[mode]), mode)
    assert ops.log == expected(("proto", branch, "gather"), mode, tuple(x.shape))
    if WANT[mode][0]:
        g = ops.gather
        assert type(dist) is ClassDistances and dist.values is ops.kernel[1] and tuple(dist.values.shape) == (B, J, 12)
        assert dist.labels is g.labels and g.labels is ops.of("shifted_labels_i32")[0] and dist.table is g.table
        assert g.width == J and dist.grid == GRIDS[0] and dist.target is target and dist.target_version == target._version
    else:
        assert ops.gather is None
    assert act is (ops.kernel[2] if WANT[mode][1] else None)


# ---- 1.-4. the packed pair -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", range(3))
@pytest.mark.parametrize("kind,branch", CASES)
def test_packed_pair(kind, branch, mode, monkeypatch):
    net, ops = make(kind, branch, monkeypatch)
    pk = packed_pair()
    lay, M = pk.layout, pk.layout.M
    out = net.forward_from_conv_features(pk, **MODES[mode])
    assert ops.log == expected((kind, branch, None), mode, tuple(pk.features.shape))
    assert type(out) is list and len(out) == len(GRIDS)
    flat, kernel = ops.flat_logits, ops.kernel
    wd = ops.of("_dense_group_matrix")[0] if kind == "group" else None
    for k, (o, (h, w)) in enumerate(zip(lay.offsets, GRIDS)):
        logits, dist, act = unpack(out[k], mode)
        assert is_view(logits, flat, o * K, (B, h, w, K), (h * w * K, w * K, K, 1))
        tag = logits.spx_packed
        assert tag[0] is flat and tag[1] is lay and tag[2:] == (k, flat._version) and not hasattr(logits, "spx_ce")
        assert dist is None or is_view(dist, kernel[1], o, (B, P, h, w), (h * w, M, w, 1))
        assert act is None or is_view(act, kernel[2], o * P, (B * h * w, P), (P, 1))
        if kind == "group":
            assert logits.spx_group_wd[0] is wd and logits.spx_group_wd[1] is net
            assert logits.spx_group_wd[2] == tuple(gp.weight._version for gp in net.group_projection)
        if kind == "group" and act is not None:
            units = {"fused": None, "wide_tail": kernel[0], "product": ops.of("wide_linear")[0] if branch == "product" else None}[branch]
            version, u, g = act.spx_group
            assert version == act._version and (u is None) == (units is None) and (g is None) == (branch != "fused")
            assert u is None or is_view(u, units, o * U, (B * h * w, U), (U, 1))
            assert g is None or is_view(g, kernel[-1], o * U, (B * h * w, U), (U, 1))

    # 2. the branch the single map takes
    net1, ops1 = make(kind, branch, monkeypatch)
    net1.forward_from_conv_features(single_map(), **MODES[mode])
    assert ops.shapeless() == ops1.shapeless()


@pytest.mark.parametrize("mode", range(3))
@pytest.mark.parametrize("branch", BRANCHES["proto"])
def test_packed_pair_with_target_labels(branch, mode, monkeypatch):
    net, ops = make("proto", branch, monkeypatch)
    pk = packed_pair()
    lay = pk.layout
    targets = [labels(g, seed=k) for k, g in enumerate(GRIDS)]
    out = net.forward_from_conv_features(pk, target_labels=targets, **MODES[mode])
    assert ops.log == expected(("proto", branch, "gather"), mode, tuple(pk.features.shape))
    g = ops.gather
    assert (g is not None) == WANT[mode][0]
    for k, (o, (h, w)) in enumerate(zip(lay.offsets, GRIDS)):
        logits, dist, act = unpack(out[k], mode)
        assert logits.spx_packed[0] is ops.flat_logits and logits.spx_packed[2] == k
        if g is not None:
            assert type(dist) is ClassDistances and dist.table is g.table and dist.grid == (h, w)
            assert is_view(dist.values, ops.kernel[1], o, (B, J, h * w), (h * w, lay.M, 1))
            assert is_view(dist.labels, g.labels, o, (B, h * w), (h * w, 1))
            assert torch.equal(dist.labels, targets[k].reshape(B, -1).int() - 1)
            assert dist.target is targets[k] and dist.target_version == targets[k]._version

    net1, ops1 = make("proto", branch, monkeypatch)
    net1.forward_from_conv_features(single_map(), target_labels=labels(GRIDS[0]), **MODES[mode])
    assert ops.shapeless() == ops1.shapeless()


# ---- the callable similarity, the scale_head's tuple, compute_group ----------------------------------------------------------
@pytest.mark.parametrize("mode", range(3))
@pytest.mark.parametrize("kind", ["proto", "group"])
def test_callable_similarity(kind, mode, monkeypatch):
    seen = []
    net, ops = make(kind, None, monkeypatch, prototype_activation_function=lambda d: seen.append(d) or -d)
    x = single_map()
    h, w = GRIDS[0]
    logits, dist, act = unpack(net.forward_from_conv_features(x, **MODES[mode]), mode)
    assert ops.log == expected((kind, "callable", None), mode, tuple(x.shape))
    assert seen[0] is ops.kernel[1] and len(seen) == 1
    assert is_view(logits, ops.flat_logits, 0, (B, h, w, K), (h * w * K, w * K, K, 1))
    assert dist is (ops.kernel[1] if WANT[mode][0] else None)
    assert act is None or tuple(act.shape) == (B * h * w, P)
    if kind == "group" and act is not None:
        assert act.spx_group[0] == act._version and act.spx_group[1] is ops.of("wide_linear")[0] and act.spx_group[2] is None
    assert not hasattr(logits, "spx_group_wd")


@pytest.mark.parametrize("mode", range(3))
@pytest.mark.parametrize("kind", ["proto", "group"])
def test_scale_head_tuple(kind, mode, monkeypatch):
    """The chain of launches under a scale_head is tests/test_gpu_scale_head.py's; here: what follows it."""
    net, ops = make(kind, None, monkeypatch, scale_head_type="sum")
    h, w = GRIDS[0]
    chain = torch.zeros(B, P, h, w)
    monkeypatch.setattr(net, "_scale_head_chain", lambda x: chain)
    logits, dist, act = unpack(net.forward_from_conv_features(single_map(), **MODES[mode]), mode)
    assert ops.log == expected((kind, "scale_head", None), mode, (B, S * CS, h, w))
    assert is_view(logits, ops.flat_logits, 0, (B, h, w, K), (h * w * K, w * K, K, 1))
    assert dist is (chain if WANT[mode][0] else None) and (act is None or tuple(act.shape) == (B * h * w, P))


@pytest.mark.parametrize("branch", BRANCHES["group"])
def test_compute_group_reads_the_forwards_tag(branch, monkeypatch):
    net, ops = make("group", branch, monkeypatch)
    sizes = [G] * K
    _, act = net.forward_from_conv_features(single_map(), return_activations=True)
    n = len(ops.log)
    groups = net.compute_group(act)
    src = ops.kernel[-1] if branch == "fused" else ops.of("group_exp")[0]
    assert ops.log[n:] == ([] if branch == "fused" else [("group_exp", (24, U))])
    assert [tuple(g.shape) for g in groups] == [(24, s) for s in sizes]
    assert all(is_view(g, src, j * G, (24, G), (U, 1)) for j, g in enumerate(groups))
    (_, a0), (_, a1) = net.forward_from_conv_features(packed_pair(), return_activations=True)
    n = len(ops.log)
    groups = net.compute_group(a1)
    assert ops.log[n:] == ([] if branch == "fused" else [("group_exp", (12, U))])
    if branch == "fused":
        g_all = ops.of("proto_head_forward")[-1][-1]
        assert all(is_view(g, g_all, 24 * U + j * G, (12, G), (U, 1)) for j, g in enumerate(groups))


# ---- 5. the refusals -----------------------------------------------------------------------------------------------------------
CE_HINT = {
    "proto": "launch, the objective one per segment (module_multiscale.py:273); call PixelWiseCrossEntropyLoss on "
             "each segment's logits",
    "group": "launch, the objective one per segment (module_multiscale_group_train.py:232-310); call "
             "SegmentedCrossEntropy on the segments' logits",
}
PACKED_CE = {k: f"{WHO}: ce_target is refused - the fused cross entropy has one mean and one backward coefficient per " + v
             for k, v in CE_HINT.items()}
PACKED_SCALE_HEAD = f"{WHO}: a scale_head chains launches per scale and has no packed form"
PACKED_CALLABLE = f"{WHO}: a callable similarity has no packed form ('log' or 'linear')"
ORIGINAL = "Original Prototype Network Implementation"
SCALE_HEAD_EXTRAS = {
    "proto": "target_labels / ce_target live in the fused distance kernel's epilogues, which do not carry a scale_head",
    "group": "ce_target lives in the fused distance kernel's epilogue, which does not carry a scale_head",
}
CALLABLE_EXTRAS = {
    "proto": "target_labels / ce_target need a built-in similarity ('log' or 'linear')",
    "group": "ce_target needs a built-in similarity ('log' or 'linear')",
}


def refused(exc, message, call, ops):
    with pytest.raises(Exception) as e:
        call()
    assert type(e.value) is exc and str(e.value) == message
    assert not ops.of("proto_head_forward")            # refused before the launch


@pytest.mark.parametrize("kind", ["proto", "group"])
def test_packed_refusals(kind, monkeypatch):
    pk, target = packed_pair(), labels(GRIDS[0])
    fwd = lambda net, **kw: lambda: net.forward_from_conv_features(pk, **kw)
    net, ops = make(kind, None, monkeypatch)
    refused(SpxError, PACKED_CE[kind], fwd(net, ce_target=target), ops)
    net.patch_classification = False
    refused(Exception, ORIGINAL, fwd(net, ce_target=target), ops)              # the guard comes first
    refused(Exception, ORIGINAL, lambda: net.forward_from_conv_features(single_map()), ops)
    net, ops = make(kind, None, monkeypatch, scale_head_type="sum", prototype_activation_function=lambda d: -d)
    refused(SpxError, PACKED_CE[kind], fwd(net, ce_target=target), ops)        # ce_target, scale_head, callable: in this order
    refused(SpxError, PACKED_SCALE_HEAD, fwd(net), ops)
    net, ops = make(kind, None, monkeypatch, prototype_activation_function=lambda d: -d)
    refused(SpxError, PACKED_CALLABLE, fwd(net), ops)
    net, ops = make(kind, None, monkeypatch)
    net.prototype_vectors = torch.nn.Parameter(torch.rand(P, CS, 2, 2))
    refused(SpxError, "only 1x1 prototypes are supported (all reference configs)", fwd(net), ops)


def test_packed_target_labels_are_checked_before_any_launch(monkeypatch):
    pk = packed_pair()
    net, ops = make("proto", "narrow", monkeypatch)
    good = [labels(g) for g in GRIDS]
    refused(SpxError, f"{WHO}: target_labels: a list with one label map per segment (2), got a tensor",
            lambda: net.forward_from_conv_features(pk, target_labels=good[0]), ops)
    refused(SpxError, f"{WHO}: target_labels[1] must be [2, 2, 3] (the segment's grid), got (2, 3, 4)",
            lambda: net.forward_from_conv_features(pk, return_activations=True, target_labels=[good[0], good[0]]), ops)
    assert ops.log == []


@pytest.mark.parametrize("kind", ["proto", "group"])
def test_single_map_refusals(kind, monkeypatch):
    x, target = single_map(), labels(GRIDS[0])
    wrong = labels(GRIDS[1])
    net, ops = make(kind, None, monkeypatch, scale_head_type="sum", prototype_activation_function=lambda d: -d)
    refused(SpxError, SCALE_HEAD_EXTRAS[kind], lambda: net.forward_from_conv_features(x, ce_target=target), ops)     # before the callable's
    net, ops = make(kind, None, monkeypatch, prototype_activation_function=lambda d: -d)
    refused(SpxError, CALLABLE_EXTRAS[kind], lambda: net.forward_from_conv_features(x, ce_target=target), ops)
    net, ops = make(kind, None, monkeypatch)
    refused(SpxError, "ce_target must be [2, 3, 4] (latent grid), got (2, 2, 3)",
            lambda: net.forward_from_conv_features(x, ce_target=wrong), ops)
    if kind == "proto":
        refused(SpxError, "target_labels must be [2, 3, 4] (latent grid), got (2, 2, 3)",
                lambda: net.forward_from_conv_features(x, target_labels=wrong), ops)
        assert ops.log == []
        net, ops = make(kind, None, monkeypatch, scale_head_type="sum")
        refused(SpxError, SCALE_HEAD_EXTRAS[kind], lambda: net.forward_from_conv_features(x, target_labels=target), ops)
        net, ops = make(kind, None, monkeypatch, prototype_activation_function=lambda d: -d)
        refused(SpxError, CALLABLE_EXTRAS[kind], lambda: net.forward_from_conv_features(x, target_labels=target), ops)


@pytest.mark.parametrize("kind", ["proto", "group"])
def test_a_list_drops_the_flags(kind, monkeypatch):
    net, ops = make(kind, None, monkeypatch)
    out = net.forward_from_conv_features([single_map(), torch.rand(B, S * CS, *GRIDS[1])], return_activations=True, return_distances=True)
    assert [len(o) for o in out] == [2, 2] and [tuple(o[1].shape) for o in out] == [(B, P, 3, 4), (B, P, 2, 3)]
