"""Coherence of the host-side caches that sit between the caller and the kernels: the pack cache
(``functional._cached_packs``), every table cache that goes through ``scaleprotoseg_amd/_cache.py`` (the modules' gather, push-key
and group-index tables, the losses' slot / pair / device / class tables, the regularisers' kernel spec), the ``spx_group`` tag and
the ``target`` / ``target_version`` attachment of ``ClassDistances``.

Every result that follows an edit is held against the CPU oracle (oracle/ppnet_oracle.py, the float64 restatements of the
loss tests) evaluated on the values AS THEY ARE NOW, with the bounds the suite already states:
  forward      ``assert_fwd`` of tests/parity_cases.py (distances 1e-4 (1 + d), activations 2e-4 (1 + |a|), logits 1e-4)
  gradients    ``GRAD_TOL`` = 1e-3 of max|g|, ``BF16_DX_TOL`` = 4e-3 for dX returned in bf16 (tests/support.py)
  KLD          1e-4 max(1, |ref|)      (tests/test_gpu_parity.py::test_kld_through_the_module)
  activation   1e-5 max(1, |ref|)      (tests/activation_loss_cases.py::check_against_reference64)
  regularisers 1e-6                    (tests/regularizer_cases.py::check_against_f64)
  push / prune bit for bit on the same distance map
and every case first asserts, with the oracle alone, that the reference before the edit and after it differ by at least
100x the bound used at the maximum element: a stale result cannot pass."""
import gc

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from oracle import ppnet_oracle as O
from activation_loss_cases import W3, log_activation
from activation_loss_cases import restate as act_restate
from parity_cases import assert_fwd, close_fwd
from push_cases import push_problem
from regularizer_cases import check_against_f64
from regularizer_cases import restate as reg_restate
from support import BF16_DX_TOL, GRAD_TOL, gpu_device, grad_close, group_net, proto_net

KLD_TOL = 1e-4           # tests/test_gpu_parity.py::test_kld_through_the_module
ACT_TOL = 1e-5           # tests/activation_loss_cases.py::check_against_reference64
REG_TOL = 1e-6           # tests/regularizer_cases.py::check_against_f64
GROUP_ACT_TOL = 2e-4     # tests/test_gpu_modules.py: |g - ref| <= 2e-4 (1 + |ref|) for compute_group's list

# the smallest problem that still runs every cached consumer of the prototype-phase module: two scales, 4 prototypes per
# (class, scale), a 128-pixel grid (one tile per image, two images)
B, S, Cs, P, K, H, W = 2, 2, 32, 40, 5, 8, 16
# the group module: P = 60, K = 6, G = 2 on a ragged 9 x 11 grid
GS, GCs, GP, GK, GG, GH, GW = 2, 16, 60, 6, 2, 9, 11


@pytest.fixture(autouse=True)
def _fresh_pack_cache():
    from scaleprotoseg_amd import functional as F

    F.invalidate_pack_cache()
    F.PACK_CACHE_STATS["hits"] = F.PACK_CACHE_STATS["misses"] = 0
    yield


def _stats():
    from scaleprotoseg_amd.functional import PACK_CACHE_STATS

    return PACK_CACHE_STATS["misses"], PACK_CACHE_STATS["hits"]


def _gen(seed):
    return torch.Generator().manual_seed(20241017 + seed)


_memo = {}


def _once(key, make):
    """Inputs and cotangents are made once and shared (never edited)."""
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _conv(group=False):
    shape = (B, GS * GCs, GH, GW) if group else (B, S * Cs, H, W)
    return _once(("conv", group), lambda: O.bf16_representable(torch.sigmoid(torch.randn(*shape, generator=_gen(0)))))


def _bank(seed, rows=P, cs=Cs):
    return O.bf16_representable(torch.rand(rows, cs, 1, 1, generator=_gen(seed)))


def _head(seed, ident):
    return O.last_layer_init(ident) + 0.3 * torch.randn(ident.shape[1], ident.shape[0], generator=_gen(100 + seed))


def _cotangents(rows, group=False):
    def make():
        g = _gen(7)
        h, w, k = (GH, GW, GK) if group else (H, W, K)
        # (the cotangents of the distances and activations are kept a tenth of the logits': the share of dX and dPrototypes
        # that passes through the head then moves them far enough for a head-only edit to be told apart)
        return (torch.randn(B, h, w, k, generator=g) * 1e-3, torch.randn(B, rows, h, w, generator=g) * 1e-4,
                torch.randn(B * h * w, rows, generator=g) * 1e-4)

    return _once(("cot", rows, group), make)


# (local: memoised 2 x 4 label patches of this module's two grids; parity_cases.gather_labels draws per pixel)
def _labels(seed=0, group=False):
    """[B, H, W] in the reference's convention (0 = void, 1..K): 2 x 4 patches of one label, so that every segment has pixels."""
    def make():
        h, w, k = (GH, GW, GK) if group else (H, W, K)
        t = torch.randint(0, k + 1, (B, (h + 1) // 2, (w + 3) // 4), generator=_gen(50 + seed))
        return t.repeat_interleave(2, 1).repeat_interleave(4, 2)[:, :h, :w].contiguous()

    return _once(("labels", seed, group), make)


def _net(dev, seed=1):
    def init(net):
        net.prototype_vectors.copy_(_bank(seed))
        net.last_layer.weight.copy_(_head(seed, net.prototype_class_identity))

    # (an empty add-on: conv_features(x) = x, so push_min_distances sees the features as they are)
    return proto_net(P, K, S, Cs, add_on=nn.Sequential(), init=init, device=dev)


def _ranges(net):
    return {s: tuple(int(v) for v in net.scale_num_prototypes[s]) for s in range(net.num_scales)}


def _oracle(net):
    """The oracle on the module's parameters and tables AS THEY ARE NOW (the bank rounded to bf16, as the kernels take it):
    forward, the gradients of sum(logits gl) + sum(distances gd), the class-masked push minimum.  CPU only."""
    bank = O.bf16_representable(net.prototype_vectors.detach().float().cpu())
    head = net.last_layer.weight.detach().float().cpu().clone()
    ident = net.prototype_class_identity.detach().cpu().clone()
    gl, gd, _ = _cotangents(bank.shape[0])
    logits, dist, act, dx, dp, dw = O.fwd_bwd_reference(_conv(), bank, _ranges(net), S, head, gl, gd)
    _, push = O.push_masked_argmin(dist, _labels(), ident, K, void_class=0)
    return dict(logits=logits, dist=dist, act=act, dx=dx, dp=dp, dw=dw, push=push, ident=ident)


def _bound(kind, ref, dx_tol=GRAD_TOL):
    """The largest the suite's bound for ``kind`` gets over the elements of ``ref``."""
    top = ref.abs().max().item()
    if kind in ("dist", "gathered"):
        return 1e-4 * (1 + top)
    if kind in ("act", "groups"):
        return 2e-4 * (1 + top)
    if kind == "logits":
        return 1.1e-4 * 1.2 * max(1.0, top)             # the per-element bound of assert_fwd at the largest element
    if kind in ("push", "wd"):
        return 0.0                                       # bit for bit
    return (dx_tol if kind == "dx" else GRAD_TOL) * top  # gradients: max-normalised


def _assert_discriminates(before, after, kinds, dx_tol=GRAD_TOL):
    """Oracle alone: the references before and after the edit differ by >= 100x the bound at the maximum element."""
    for kind in kinds:
        a, b = before[kind], after[kind]
        assert a.shape == b.shape, kind
        diff = (a - b).abs().max().item()
        need = 100 * max(_bound(kind, a, dx_tol), _bound(kind, b, dx_tol))
        print(f"discriminates: {kind} differs by {diff:.3g}, 100 x bound = {need:.3g}")
        assert diff > 0 and diff >= need, f"the edit does not move {kind} enough: {diff:.3g} < {need:.3g}"


def _check_consumers(net, dev, ref, x_dtype=torch.float32):
    """Every consumer of the pack cache through the module, against ``ref`` = _oracle(net)."""
    from scaleprotoseg_amd.functional import prune_nearest_from_features, prune_nearest_from_map

    rows = net.num_prototypes
    x0 = _conv().to(dev, x_dtype)
    with torch.no_grad():
        logits, dist = net.forward_from_conv_features(x0)
    assert_fwd(logits, dist, None, ref["logits"], ref["dist"], None)
    gl, gd, _ = _cotangents(rows)
    net.zero_grad(set_to_none=True)
    x = _conv().to(dev, x_dtype).requires_grad_(True)
    lg, d = net.forward_from_conv_features(x)
    torch.autograd.backward([lg, d], [gl.to(dev), gd.to(dev)])
    assert_fwd(lg.detach(), d.detach(), None, ref["logits"], ref["dist"], None)
    assert x.grad.dtype == x_dtype
    grad_close(x.grad, ref["dx"], "dX", tol=GRAD_TOL if x_dtype == torch.float32 else BF16_DX_TOL)
    grad_close(net.prototype_vectors.grad, ref["dp"], "dPrototypes")
    grad_close(net.last_layer.weight.grad, ref["dw"], "dLastLayer")
    net.zero_grad(set_to_none=True)
    del lg, d, x
    # the fused push minimum and the fused prune search: bit for bit what the two-step forms give on the map just verified
    lab = _labels()
    out = net.push_min_distances(x0, lambda hw: lab.to(dev), void_class=0)
    assert out is not None
    ridx, rval = O.push_masked_argmin(dist.cpu(), lab, ref["ident"], K, void_class=0)
    assert torch.equal(out[0].cpu(), ridx) and torch.equal(out[1].cpu(), rval), "push_min_distances"
    plab = (lab - 1).to(dev)
    keys = prune_nearest_from_features(x0, net.prototype_vectors, net._layout(1), plab)
    assert torch.equal(keys, prune_nearest_from_map(dist, plab)), "prune_nearest_from_features"


# ------------------------------------------------------------------------------------------------------------------
# A. the pack cache serves an unchanged bank
# ------------------------------------------------------------------------------------------------------------------
def _plain_problem(dev, grad=False):
    from scaleprotoseg_amd.functional import BankLayout

    ident = O.default_class_identity(P, K, S)
    ranges = O.default_scale_ranges(P, S)
    lay = lambda k: BankLayout(P, k, S, Cs, tuple(ranges[s] for s in range(S)))
    pv, w = _bank(1).to(dev).requires_grad_(grad), _head(1, ident).to(dev).requires_grad_(grad)
    return _conv().to(dev), pv, w, lay, ident, ranges


def test_untouched_parameters_are_served_from_the_cache():
    dev = gpu_device()
    net = _net(dev)
    ref = _oracle(net)
    x = _conv().to(dev)
    n = 5
    for _ in range(n):
        with torch.no_grad():
            logits, dist = net.forward_from_conv_features(x)
    assert _stats() == (1, n - 1)
    assert_fwd(logits, dist, None, ref["logits"], ref["dist"], None)


def test_packs_with_and_without_the_transposed_operands_are_separate_entries():
    from scaleprotoseg_amd.functional import proto_head_forward

    dev = gpu_device()
    x, pv, w, lay, ident, ranges = _plain_problem(dev)
    rl, rd, _ = O.forward_from_conv_features(_conv(), _bank(1), ranges, S, _head(1, ident))
    for grad in (False, True, False, True):
        pv.requires_grad_(grad)
        w.requires_grad_(grad)
        logits, dist, _ = proto_head_forward(x, pv, w, lay(K))
        assert_fwd(logits, dist, None, rl, rd, None)
    assert _stats() == (2, 2)
    (logits.sum() + dist.sum()).backward()                  # the entry served to a differentiable forward carries bank^T / head^T
    assert torch.isfinite(pv.grad).all() and torch.isfinite(w.grad).all()


def test_push_and_prune_share_the_distance_only_packs():
    """``push_min_from_features``, ``prune_nearest_from_features`` and a distance-only forward of a frozen bank key their packs
    alike (the bank, no head, no tail, no transposed operands, the same plan): one miss, then hits.  The head's plan is
    another entry."""
    from scaleprotoseg_amd.functional import proto_head_forward, prune_nearest_from_features, push_min_from_features

    dev = gpu_device()
    x, pv, w, lay, ident, ranges = _plain_problem(dev)
    lab = _labels().to(dev)
    idx, val = push_min_from_features(x, pv, lay(1), lab, ident, void_class=0)
    assert _stats() == (1, 0)
    keys = prune_nearest_from_features(x, pv, lay(1), lab - 1)
    assert _stats() == (1, 1)
    _, dist, _ = proto_head_forward(x, pv, None, lay(1))
    assert _stats() == (1, 2)
    proto_head_forward(x, pv, w, lay(K))
    assert _stats() == (2, 2)
    rd = O.scale_l2_convolution(_conv(), _bank(1), ranges, S)
    assert_fwd(None, dist, None, None, rd, None)
    ridx, rval = O.push_masked_argmin(dist.cpu(), _labels(), ident, K, void_class=0)
    assert torch.equal(idx.cpu(), ridx) and torch.equal(val.cpu(), rval)


def test_nothing_is_cached_during_stream_capture():
    """The warm-up's eager forward is the one miss; the captured forward neither reads nor fills the cache (its pack kernels are
    part of the graph), so a replay after an in-place edit of the bank computes with the bank as it is then."""
    from scaleprotoseg_amd import functional as F
    from scaleprotoseg_amd.graphs import capture_step

    dev = gpu_device()
    x, pv, w, lay, ident, ranges = _plain_problem(dev)

    def step():
        with torch.no_grad():
            logits, dist, _ = F.proto_head_forward(x, pv, w, lay(K))
        return logits, dist

    graph, (logits, dist) = capture_step(step, warmup=1)
    assert _stats() == (1, 0) and len(F._PACK_CACHE) == 0
    before = O.forward_from_conv_features(_conv(), _bank(1), ranges, S, _head(1, ident))
    after = O.forward_from_conv_features(_conv(), _bank(2), ranges, S, _head(1, ident))
    _assert_discriminates(dict(logits=before[0], dist=before[1]), dict(logits=after[0], dist=after[1]), ("logits", "dist"))
    graph.replay()
    torch.cuda.synchronize()
    assert_fwd(logits, dist, None, before[0], before[1], None)
    with torch.no_grad():
        pv.copy_(_bank(2).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    assert_fwd(logits, dist, None, after[0], after[1], None)
    assert _stats() == (1, 0) and len(F._PACK_CACHE) == 0


def test_the_cache_holds_a_bounded_number_of_entries():
    from scaleprotoseg_amd import functional as F

    dev = gpu_device()
    x, pv, w, lay, ident, ranges = _plain_problem(dev)
    heads = [_head(10 + i, ident).to(dev) for i in range(F._PACK_CACHE_MAX + 3)]       # all alive: distinct objects and addresses
    for h in heads:
        F.proto_head_forward(x, pv, h, lay(K))
    assert _stats() == (len(heads), 0)
    assert 1 <= len(F._PACK_CACHE) <= F._PACK_CACHE_MAX
    logits, dist, _ = F.proto_head_forward(x, pv, heads[-1], lay(K))              # the most recent entry is still there ...
    assert _stats() == (len(heads), 1)
    F.proto_head_forward(x, pv, heads[0], lay(K))                                 # ... the oldest was dropped
    assert _stats() == (len(heads) + 1, 1)
    rl, rd, _ = O.forward_from_conv_features(_conv(), _bank(1), ranges, S, heads[-1].cpu())
    assert_fwd(logits, dist, None, rl, rd, None)


# ------------------------------------------------------------------------------------------------------------------
# B. every kind of parameter edit x every consumer
# ------------------------------------------------------------------------------------------------------------------
ALL = ("logits", "dist", "dx", "dp", "dw", "push")
HEAD_ONLY = ("logits", "dx", "dp")                   # dW = dLogits^T . act and the distances do not read the head


def _new_values(net, seed=2):
    return _bank(seed, net.num_prototypes), _head(seed, net.prototype_class_identity.cpu())


def _edit_sgd(net, dev):
    b2, h2 = _new_values(net)
    pv, w = net.prototype_vectors, net.last_layer.weight
    opt = torch.optim.SGD([pv, w], lr=1.0)
    pv.grad, w.grad = pv.detach() - b2.to(dev), w.detach() - h2.to(dev)       # one step of lr 1 lands (nearly) on the new values
    opt.step()
    return ALL


def _edit_adam_foreach(net, dev):
    """This file's references are stated for a bf16-representable bank (off that grid the gradient's reference is the per-site
    restatement of DESIGN.md 4 "operand sites", held by tests/test_gpu_offgrid.py, not plain autograd): as with SGD
    the step is made to land on the new values.  The first Adam step moves an element by lr g / (|g| + eps); with eps = 1
    a move of r lr, |r| < 1/2, takes g = r / (1 - |r|).  In fp32 that lands within a few 1e-7 of the target."""
    b2, h2 = _new_values(net)
    pv, w = net.prototype_vectors, net.last_layer.weight
    lr, eps = 4.0, 1.0
    opt = torch.optim.Adam([pv, w], lr=lr, eps=eps, foreach=True)
    for p, new in ((pv, b2), (w, h2)):
        r = (p.detach().double() - new.to(dev).double()) / lr
        assert r.abs().max().item() < 0.5
        p.grad = (eps * r / (1 - r.abs())).float()
    opt.step()
    assert (pv.detach() - b2.to(dev)).abs().max().item() <= 1e-6 and (w.detach() - h2.to(dev)).abs().max().item() <= 1e-6
    return ALL


def _edit_no_grad_copy_add(net, dev):
    b2, h2 = _new_values(net)
    with torch.no_grad():
        net.prototype_vectors.copy_(b2.to(dev))
        net.last_layer.weight.add_(h2.to(dev) - net.last_layer.weight)
    return ALL


def _new_state_dict(net, dev=None):
    b2, h2 = _new_values(net)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    sd["prototype_vectors"], sd["last_layer.weight"] = b2, h2
    return {k: v.to(dev) for k, v in sd.items()} if dev is not None else sd


def _edit_load_state_dict(net, dev):
    net.load_state_dict(_new_state_dict(net))
    return ALL


def _edit_load_state_dict_assign(net, dev):
    old = net.prototype_vectors
    net.load_state_dict(_new_state_dict(net, dev), assign=True)
    assert net.prototype_vectors is not old and net.prototype_vectors.requires_grad
    return ALL


def _edit_data_assign(net, dev):
    b2, h2 = _new_values(net)
    net.prototype_vectors.data = b2.to(dev)
    net.last_layer.weight.data = h2.to(dev)
    return ALL


def _edit_cpu_round_trip(net, dev):
    b2, h2 = _new_values(net)
    net.cpu()
    with torch.no_grad():
        net.prototype_vectors.copy_(b2)
        net.last_layer.weight.copy_(h2)
    net.to(dev)
    return ALL


def _edit_prune(net, dev):
    net.prune_prototypes([1, 7, 22, 39])
    return ("logits", "dx")                         # (the kept rows' distances and gradients do not move; their shapes do)


def _edit_incorrect_connection(net, dev):
    net.set_last_layer_incorrect_connection(-2.0)
    return HEAD_ONLY


def _edit_initialize_weights(net, dev):
    net._initialize_weights()                       # takes the 0.3 randn off the head: too little for dX to move by 100 bounds
    return ("logits", "dp")


def _edit_commit_push(net, dev):
    from scaleprotoseg_amd.push import commit_push

    b2, _ = _new_values(net)
    dup = commit_push(net, [r.numpy().reshape(-1, 1, 1) for r in b2], log=lambda *_: None)
    assert dup == []
    return ("logits", "dist", "dx", "dp", "dw", "push")


def _edit_foreign_data_copy_then_invalidate(net, dev):
    from scaleprotoseg_amd.functional import invalidate_pack_cache

    b2, h2 = _new_values(net)
    net.prototype_vectors.data.copy_(b2.to(dev))
    net.last_layer.weight.data.copy_(h2.to(dev))
    invalidate_pack_cache()                         # the documented duty of foreign code that writes through .data
    return ALL


EDITS = {f.__name__[len("_edit_"):]: f for f in (
    _edit_sgd, _edit_adam_foreach, _edit_no_grad_copy_add, _edit_load_state_dict, _edit_load_state_dict_assign, _edit_data_assign,
    _edit_cpu_round_trip, _edit_prune, _edit_incorrect_connection, _edit_initialize_weights, _edit_commit_push,
    _edit_foreign_data_copy_then_invalidate)}
BF16_EDITS = ("sgd", "data_assign", "prune")        # bf16 features: dX through the transposed packs, returned in bf16


@pytest.mark.parametrize("edit,x_dtype", [(e, torch.float32) for e in EDITS] + [(e, torch.bfloat16) for e in BF16_EDITS],
                         ids=[e + "-fp32" for e in EDITS] + [e + "-bf16" for e in BF16_EDITS])
def test_every_consumer_sees_the_edit(edit, x_dtype):
    dev = gpu_device()
    dx_tol = GRAD_TOL if x_dtype == torch.float32 else BF16_DX_TOL
    net = _net(dev)
    before = _oracle(net)
    _check_consumers(net, dev, before, x_dtype)             # fills every cache with the first values
    assert _stats()[0] >= 2
    kinds = EDITS[edit](net, dev)
    after = _oracle(net)
    if edit == "prune":
        assert after["dist"].shape[1] == P - 4
    _assert_discriminates(before, after, kinds, dx_tol)
    _check_consumers(net, dev, after, x_dtype)
    _check_consumers(net, dev, after, x_dtype)              # ... and again, now from whatever the first round cached


def test_the_push_commit_reaches_every_consumer(tmp_path):
    """``push_prototypes_multiscale`` end to end (the problem of tests/push_cases.py) on a module whose packs are
    cached: the push's own forwards cache the old bank, the commit writes through ``.data`` and prunes the duplicate."""
    from scaleprotoseg_amd.push import push_prototypes_multiscale

    dev = gpu_device()
    S_, K_ = 4, 5
    net, data, _ = push_problem(dev, S=S_, K=K_)
    with torch.no_grad():
        conv = net.conv_features(data[0][0].unsqueeze(0).to(dev))

    def oracle():
        return O.forward_from_conv_features(conv.cpu(), O.bf16_representable(net.prototype_vectors.detach().cpu()), _ranges(net), S_,
                                            net.last_layer.weight.detach().cpu())

    def check(ref):
        with torch.no_grad():
            logits, dist = net.forward_from_conv_features(conv)
        close_fwd(dist, ref[1], "distances")
        close_fwd(logits, ref[0], "logits")

    before = oracle()
    check(before)
    check(before)
    assert _stats() == (1, 1)
    rows_before = net.num_prototypes
    push_prototypes_multiscale(data, net, root_dir_for_saving_prototypes=str(tmp_path), log=lambda *_: None)
    assert net.num_prototypes < rows_before                                    # the duplicates are dropped
    after = oracle()
    _assert_discriminates(dict(logits=before[0]), dict(logits=after[0]), ("logits",))
    check(after)
    check(after)


# ---- the group module: the cached tail (last_layer_group.weight) and the per-forward dense matrix wd ---------------------
def _group_net(dev, seed=1):
    from scaleprotoseg_amd.utils import projection_simplex_sort

    g = _gen(200 + seed)

    def init(net):
        net.prototype_vectors.copy_(_bank(seed, GP, GCs))
        for gp in net.group_projection:
            gp.weight.copy_(projection_simplex_sort(torch.rand(gp.weight.shape, generator=g)))
        net.last_layer_group.weight.add_(0.3 * torch.randn(net.last_layer_group.weight.shape, generator=g))

    return group_net(GP, GK, GS, GCs, GG, add_on=nn.Sequential(), init=init, device=dev)


def _group_oracle(net):
    bank = O.bf16_representable(net.prototype_vectors.detach().float().cpu()).requires_grad_(True)
    gws = [gp.weight.detach().float().cpu().clone().requires_grad_(True) for gp in net.group_projection]
    tail = net.last_layer_group.weight.detach().float().cpu().clone().requires_grad_(True)
    ident = net.prototype_class_identity.detach().cpu().clone()
    x = _conv(group=True).clone().requires_grad_(True)
    gl, gd, ga = _cotangents(bank.shape[0], group=True)
    logits, dist, act = O.forward_from_conv_features(x, bank, _ranges(net), GS, None, class_identity=ident, group_weights=gws,
                                                     last_layer_group_weight=tail)
    ((logits * gl).sum() + (dist * gd).sum() + (act * ga).sum()).backward()
    return dict(logits=logits.detach(), dist=dist.detach(), act=act.detach(), dx=x.grad, dp=bank.grad, dtail=tail.grad,
                dgw=torch.cat([w.grad.reshape(-1) for w in gws]), ident=ident,
                groups=torch.cat(O.compute_group(act.detach(), ident, [w.detach() for w in gws]), dim=-1))


def _check_group_consumers(net, dev, ref):
    gl, gd, ga = _cotangents(net.num_prototypes, group=True)
    net.zero_grad(set_to_none=True)
    x = _conv(group=True).to(dev).requires_grad_(True)
    logits, dist, act = net.forward_from_conv_features(x, return_activations=True, return_distances=True)
    assert_fwd(logits.detach(), dist.detach(), act.detach(), ref["logits"], ref["dist"], ref["act"])
    for a in (act, act.detach().clone()):                   # the forward's own tag, and the product kernels on foreign activations
        groups = torch.cat(net.compute_group(a), dim=-1).detach().cpu()
        assert ((groups - ref["groups"]).abs() <= GROUP_ACT_TOL * (1 + ref["groups"].abs())).all(), "compute_group"
    torch.autograd.backward([logits, dist, act], [gl.to(dev), gd.to(dev), ga.to(dev)])
    grad_close(x.grad, ref["dx"], "dX")
    grad_close(net.prototype_vectors.grad, ref["dp"], "dPrototypes")
    grad_close(net.last_layer_group.weight.grad, ref["dtail"], "dLastLayerGroup")
    grad_close(torch.cat([gp.weight.grad.reshape(-1) for gp in net.group_projection]), ref["dgw"], "dGroupProjection")
    net.zero_grad(set_to_none=True)


def _group_new(net, dev, seed=2):
    from scaleprotoseg_amd.utils import projection_simplex_sort

    g = _gen(300 + seed)
    gws = [projection_simplex_sort(torch.rand(gp.weight.shape, generator=g)).to(dev) for gp in net.group_projection]
    tail = (O.last_layer_init(net.group_class_identity.cpu()) + 0.3 * torch.randn(net.last_layer_group.weight.shape, generator=g)).to(dev)
    return _bank(seed, net.num_prototypes, GCs).to(dev), gws, tail


def _gedit_sgd(net, dev):
    bank, gws, tail = _group_new(net, dev)
    params = [net.prototype_vectors, net.last_layer_group.weight] + [gp.weight for gp in net.group_projection]
    opt = torch.optim.SGD(params, lr=1.0)
    for p, new in zip(params, [bank, tail] + gws):
        p.grad = p.detach() - new
    opt.step()
    return ("logits", "dist", "act", "groups", "dx", "dp", "dtail", "dgw")


def _gedit_simplex_rebind(net, dev):
    """What ``DataParallelStep`` and ``_initialize_weights`` do after a step: ``weight.data = projection_simplex_sort(...)``."""
    from scaleprotoseg_amd.utils import projection_simplex_sort

    g = _gen(5)
    for gp in net.group_projection:
        gp.weight.data = projection_simplex_sort(gp.weight.data + torch.rand(gp.weight.shape, generator=g).to(dev))
    return ("logits", "groups", "dx", "dp", "dtail")


def _gedit_tail_data_assign(net, dev):
    net.last_layer_group.weight.data = _group_new(net, dev)[2]
    return ("logits", "dx", "dp", "dgw")


def _gedit_tail_no_grad_copy(net, dev):
    with torch.no_grad():
        net.last_layer_group.weight.copy_(_group_new(net, dev)[2])
    return ("logits", "dx", "dp", "dgw")


def _gedit_bank_data_assign(net, dev):
    net.prototype_vectors.data = _group_new(net, dev)[0]
    return ("logits", "dist", "act", "groups", "dx", "dp", "dtail", "dgw")


def _gedit_initialize_weights(net, dev):
    net._initialize_weights()                       # rebinds every group weight (simplex) and fills the tail through .data
    return ("logits", "dx", "dp", "dgw")


GROUP_EDITS = {f.__name__[len("_gedit_"):]: f for f in (_gedit_sgd, _gedit_simplex_rebind, _gedit_tail_data_assign,
                                                         _gedit_tail_no_grad_copy, _gedit_bank_data_assign, _gedit_initialize_weights)}


@pytest.mark.parametrize("edit", list(GROUP_EDITS))
def test_the_group_module_sees_the_edit(edit):
    dev = gpu_device()
    net = _group_net(dev)
    before = _group_oracle(net)
    _check_group_consumers(net, dev, before)
    kinds = GROUP_EDITS[edit](net, dev)
    after = _group_oracle(net)
    _assert_discriminates(before, after, kinds)
    _check_group_consumers(net, dev, after)
    _check_group_consumers(net, dev, after)


# ------------------------------------------------------------------------------------------------------------------
# C. storage rebinding onto a recycled address
# ------------------------------------------------------------------------------------------------------------------
def _forward_checked(net, dev, what):
    ref = _oracle(net)
    with torch.no_grad():
        logits, dist = net.forward_from_conv_features(_conv().to(dev))
    torch.cuda.synchronize()
    try:
        assert_fwd(logits, dist, None, ref["logits"], ref["dist"], None)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None
    return ref


@pytest.mark.parametrize("which", ["bank", "head"])
def test_rebinding_onto_a_recycled_address_never_hits(which):
    """``p.data = new`` leaves ``p._version`` alone, and the caching allocator hands a freed block to the next request of its
    size: the third value of a parameter sits where the first did, under the same (object, version, address).  Every forward
    is held against the oracle on the value of that moment.

    How the recycle is made deterministic: the new tensor is the ONLY allocation of a rebind (``empty_like`` while the old
    storage is still held, filled by a host copy), the old storage is released only after the forward that follows (so that
    forward's own buffers cannot take its block), and nothing else is allocated in between: the one free block of exactly the
    parameter's size is then the block of the value before the last.  The test asserts that precondition - some rebind within
    six lands on an address an earlier, different value was packed from - and fails, not skips, when the allocator does not
    comply (the cache holds 8 entries: six rebinds stay below that)."""
    dev = gpu_device()
    net = _net(dev)
    p = net.prototype_vectors if which == "bank" else net.last_layer.weight
    torch.cuda.synchronize()
    seen = {p.data_ptr(): 1}
    refs = [_forward_checked(net, dev, "value 1")]
    recycled = None
    for i in range(2, 8):                                    # values 2..7: six rebinds
        value = _bank(i) if which == "bank" else _head(i, net.prototype_class_identity)
        new = torch.empty_like(p.data)
        new.copy_(value)
        old = p.data
        version = p._version
        p.data = new
        assert p._version == version and p.data_ptr() != old.data_ptr()
        del new
        refs.append(_forward_checked(net, dev, f"value {i} at {p.data_ptr():#x} (addresses so far: {seen})"))
        _assert_discriminates(refs[-2], refs[-1], ("logits",) if which == "head" else ("logits", "dist"))
        del old                                              # only now may the previous block be reissued
        if p.data_ptr() in seen and recycled is None:
            recycled = (i, seen[p.data_ptr()])
        seen[p.data_ptr()] = i
        if recycled is not None and i >= recycled[0] + 1:
            break
    print(f"{which}: value -> address {seen}; first recycle: {recycled}")
    assert recycled is not None, ("precondition not met: within six rebinds the allocator never placed a new value of the "
                                  f"{which} at an address an earlier value was packed from ({seen})")


@pytest.mark.parametrize("which", ["bank", "head"])
def test_two_rebinds_without_a_forward_in_between(which):
    """v1 is packed; the parameter is rebound to v2 and at once to v3 - where the block v1 lived in is the natural candidate.
    (While an entry packed from v1's storage is alive that block must not be reissued at all; either way the forward computes
    with v3.)"""
    dev = gpu_device()
    net = _net(dev)
    p = net.prototype_vectors if which == "bank" else net.last_layer.weight
    first = _forward_checked(net, dev, "value 1")
    addrs = [p.data_ptr()]
    for i in (2, 3):
        value = _bank(i) if which == "bank" else _head(i, net.prototype_class_identity)
        new = torch.empty_like(p.data)
        new.copy_(value)
        p.data = new
        del new
        addrs.append(p.data_ptr())
    print(f"{which}: addresses {[hex(a) for a in addrs]}")
    _assert_discriminates(first, _oracle(net), ("logits",) if which == "head" else ("logits", "dist"))
    _forward_checked(net, dev, f"value 3 at {addrs[2]:#x} after value 1 at {addrs[0]:#x}")


def test_cpu_round_trips_onto_recycled_addresses_never_hit():
    """``net.cpu()``, ``p.data = new``, ``net.to(dev)``: ``Module._apply`` rebinds every parameter (same object, same version)
    and the allocator serves the same sizes in the same order, so a parameter comes back to an address it had.  Precondition
    asserted as above: within six round trips some value lands where an earlier one was packed from."""
    dev = gpu_device()
    net = _net(dev)
    pv, w = net.prototype_vectors, net.last_layer.weight
    seen = {(pv.data_ptr(), w.data_ptr()): 1}
    refs = [_forward_checked(net, dev, "value 1")]
    recycled = None
    for i in range(2, 8):
        version = pv._version
        net.cpu()
        pv.data, w.data = _bank(i), _head(i, net.prototype_class_identity)
        net.to(dev)
        assert net.prototype_vectors is pv and pv._version == version and pv.is_cuda
        key = (pv.data_ptr(), w.data_ptr())
        refs.append(_forward_checked(net, dev, f"value {i} at {key} (addresses so far: {seen})"))
        _assert_discriminates(refs[-2], refs[-1], ("logits", "dist"))
        if recycled is None and any(key[0] == k[0] or key[1] == k[1] for k in seen):
            recycled = i
        seen[key] = i
        if recycled is not None and i >= recycled + 1:
            break
    print(f"round trips: (bank, head) addresses -> value {seen}; first recycle at value {recycled}")
    assert recycled is not None, f"precondition not met: no address recurred within six round trips ({seen})"


def test_a_new_model_on_a_recycled_parameter_is_not_served_the_old_packs():
    """Models built and dropped in sequence: a new Parameter may land on the ``id`` and the address of a dead one, at the same
    version.  The entry's weak reference tells them apart.  (Whether ids and addresses do recur is up to the interpreter and the
    allocator; the recurrences are printed, the results are held to the oracle either way.)"""
    dev = gpu_device()
    seen, prev = {}, None
    for i in range(1, 6):
        net = _net(dev, seed=i)
        key = (id(net.prototype_vectors), net.prototype_vectors.data_ptr(), net.prototype_vectors._version)
        ref = _forward_checked(net, dev, f"model {i}, (id, address, version) {key}; earlier: {seen}")
        if prev is not None:
            _assert_discriminates(prev, ref, ("logits", "dist"))
        print(f"model {i}: bank (id, address, version) {key}" + (f" - as model {seen[key]}" if key in seen else ""))
        seen[key] = i
        prev = ref
        del net
        gc.collect()


# ------------------------------------------------------------------------------------------------------------------
# D. table caches: prototype_class_identity and scale_num_prototypes
# ------------------------------------------------------------------------------------------------------------------
def _tedit_reassign(net):
    net.prototype_class_identity = net.prototype_class_identity.roll(1, dims=1)      # every class takes its neighbour's prototypes


def _tedit_rows_in_place(net):
    ident = net.prototype_class_identity
    for p in list(range(0, 8)) + list(range(20, 26)):        # classes 0 and 1 lose prototypes of both scales to classes 2 and 3
        ident[p] = torch.nn.functional.one_hot(torch.tensor(2 + p % 2), ident.shape[1]).to(ident)


def _tedit_prune(net):
    net.prune_prototypes([0, 1, 2, 4, 5, 6, 8, 9, 10, 21, 22, 25, 26, 30, 33, 34, 38])


def _tedit_scale_item(net):
    net.scale_num_prototypes[0] = (0, 8)                     # the boundary between the scales moves by three class blocks
    net.scale_num_prototypes[1] = (8, 40)


TABLE_EDITS = {f.__name__[len("_tedit_"):]: f for f in (_tedit_reassign, _tedit_rows_in_place, _tedit_prune, _tedit_scale_item)}


def _loss_oracle(net, dist, target):
    """float64 restatements of the losses on the distance map ``dist`` [B, P, H, W] under the module's tables as they are now."""
    ident = net.prototype_class_identity.detach().cpu().clone()
    ranges = _ranges(net)
    d64 = dist.double()
    kld = O.kld_loss(d64, target, ident, net.num_scales, ranges).item()
    a64 = log_activation(d64.reshape(d64.shape[0], d64.shape[1], -1).permute(0, 2, 1).reshape(-1, d64.shape[1]))
    vals, counts = act_restate(a64, target, ident, [ranges[s] for s in range(net.num_scales)], norm_type="l1")
    assert all(n > 0 for n in counts.values())
    terms = torch.stack([vals["spat"], vals["sampl"], vals["norm"]])
    w64 = net.last_layer.weight.detach().cpu().double()
    l1 = (w64 * (1 - ident.double().t())).abs().sum().item()
    return dict(kld=torch.tensor(kld), act_terms=terms, act_total=(terms * torch.tensor(W3, dtype=torch.float64)).sum(), l1=torch.tensor(l1),
                gathered=O.gather_class_distances(dist, target.reshape(target.shape[0], -1) - 1, ident), table=O.class_slot_table(ident))


def _scalar_close(got, ref, tol, what):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).double()
    err = (got - ref).abs()
    print(f"{what}: got {got.tolist()} ref {ref.tolist()}")
    assert torch.isfinite(got).all() and (err <= tol * ref.abs().clamp_min(1.0)).all(), f"{what}: {got.tolist()} vs {ref.tolist()}"


LOSS_TOL = {"kld": KLD_TOL, "act_terms": ACT_TOL, "l1": REG_TOL}


def _assert_losses_discriminate(before, after, keys=("kld", "act_terms", "l1")):
    for key in keys:
        tol = LOSS_TOL[key]
        a, b = before[key].double(), after[key].double()
        diff = (a - b).abs().max().item()
        need = 100 * tol * max(1.0, a.abs().max().item(), b.abs().max().item())
        print(f"discriminates: {key} differs by {diff:.3g}, 100 x bound = {need:.3g}")
        assert diff >= need, f"the edit does not move {key} enough: {diff:.3g} < {need:.3g}"


def _check_table_consumers(net, dev, losses, target):
    """The consumers of the class / scale tables through the module and through long-lived loss modules (``losses``: built
    once, BEFORE the edit, so their caches have seen the old tables)."""
    import scaleprotoseg_amd as spx

    ref = _oracle(net)
    lref = _loss_oracle(net, ref["dist"], target)
    x = _conv().to(dev)
    tgt = target.to(dev)
    with torch.no_grad():
        logits, cd = net.forward_from_conv_features(x, target_labels=tgt)
        _, dist, act = net.forward_from_conv_features(x, return_activations=True, return_distances=True)
    assert_fwd(logits, dist, act, ref["logits"], ref["dist"], ref["act"])
    assert isinstance(cd, spx.ClassDistances) and torch.equal(cd.table.cpu(), lref["table"])
    got = cd.values.cpu().permute(0, 2, 1)
    assert got.shape == lref["gathered"].shape
    assert ((got - lref["gathered"]).abs() <= 1e-4 * (1 + lref["gathered"])).all() and (got[lref["gathered"] == 0] == 0).all()
    out = net.push_min_distances(x, lambda hw: _labels().to(dev), void_class=0)
    ridx, rval = O.push_masked_argmin(dist.cpu(), _labels(), ref["ident"], K, void_class=0)
    assert out is not None and torch.equal(out[0].cpu(), ridx) and torch.equal(out[1].cpu(), rval), "push_min_distances"
    kld, reg = losses
    _scalar_close(kld(cd, tgt), lref["kld"], KLD_TOL, "KLD of the ClassDistances")
    _scalar_close(kld(dist, tgt), lref["kld"], KLD_TOL, "KLD of the full map")
    for form, inp in (("ClassDistances", cd), ("activations", act)):
        tot, terms = reg(inp, tgt)
        _scalar_close(terms, lref["act_terms"], ACT_TOL, f"activation terms of the {form}")
        _scalar_close(tot, lref["act_total"], ACT_TOL, f"activation total of the {form}")
    _scalar_close(spx.head_l1(net), lref["l1"], REG_TOL, "head L1")
    return dict(gathered=lref["gathered"], **ref), lref


@pytest.mark.parametrize("edit", list(TABLE_EDITS))
def test_table_caches_follow_the_edit(edit):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    net = _net(dev)
    target = _labels(1)
    kld = spx.KLDLoss(net.prototype_class_identity, S, net.scale_num_prototypes)
    reg = spx.ActivationRegularizers(net.prototype_class_identity, S, net.scale_num_prototypes, *W3, epsilon=net.epsilon)
    before, lbefore = _check_table_consumers(net, dev, (kld, reg), target)
    TABLE_EDITS[edit](net)
    # the losses hold the identity TENSOR and the scale DICT of the module: an in-place edit reaches them, a re-assignment on
    # the module (prune_prototypes re-assigns too) has to be repeated on them
    kld.prototype_class_identity = reg.prototype_class_identity = net.prototype_class_identity
    after, lafter = _check_table_consumers(net, dev, (kld, reg), target)
    if edit == "scale_item":
        _assert_discriminates(before, after, ("dist", "logits"))
    elif edit != "prune":
        assert before["gathered"].shape != after["gathered"].shape or (before["gathered"] != after["gathered"]).any()
        _assert_discriminates(before, after, ("push",))
    _assert_losses_discriminate(lbefore, lafter, ("kld", "act_terms") if edit == "scale_item" else ("kld", "act_terms", "l1"))
    _check_table_consumers(net, dev, (kld, reg), target)


def _dense_reference(net):
    """The index_put form of the dense group matrix (model_multiscale_group.py:283-303 in dense form)."""
    ident = net.prototype_class_identity.cpu()
    idxs = O.class_prototype_index(ident)
    ws = [gp.weight.detach().cpu() for gp in net.group_projection]
    wd = torch.zeros(sum(w.shape[0] for w in ws), ident.shape[0])
    r0 = 0
    for idx, w in zip(idxs, ws):
        wd[r0:r0 + w.shape[0]].index_put_((torch.arange(w.shape[0]).unsqueeze(1), idx.unsqueeze(0)), w)
        r0 += w.shape[0]
    return wd


def _gtedit_reassign(net):
    net.prototype_class_identity = net.prototype_class_identity.roll(1, dims=1)


def _gtedit_swap_rows_in_place(net):
    ident = net.prototype_class_identity
    for p, q in ((0, 5), (1, 36), (31, 47)):                 # the classes keep their counts (the projections their shapes)
        row = ident[p].clone()
        ident[p] = ident[q]
        ident[q] = row


def _gtedit_prune(net):
    net.prune_prototypes([0, 1, 7, 33, 59])
    net._initialize_weights()


def _gtedit_scale_item(net):
    net.scale_num_prototypes[0] = (0, 25)
    net.scale_num_prototypes[1] = (25, 60)


GROUP_TABLE_EDITS = {f.__name__[len("_gtedit_"):]: f for f in (_gtedit_reassign, _gtedit_swap_rows_in_place, _gtedit_prune,
                                                              _gtedit_scale_item)}
REG_WEIGHTS = (0.25, 0.1, 0.3, 1e-3)


def _check_group_tables(net, dev, reg):
    wd_ref = _dense_reference(net)
    assert torch.equal(net._dense_group_matrix().detach().cpu(), wd_ref), "_dense_group_matrix"
    act = torch.rand(37, net.num_prototypes, generator=_gen(9)) * 3.0
    ref = torch.cat(O.compute_group(act, net.prototype_class_identity.cpu(), [gp.weight.detach().cpu() for gp in net.group_projection]), dim=-1)
    got = torch.cat(net.compute_group(act.to(dev)), dim=-1).detach().cpu()
    assert ((got - ref).abs() <= GROUP_ACT_TOL * (1 + ref.abs())).all(), "compute_group"
    check_against_f64(net, reg, REG_WEIGHTS, 1e-5)
    return dict(wd=wd_ref, groups=ref)


def _reg_reference(net):
    ident = net.prototype_class_identity.cpu()
    hg = net.last_layer_group.weight.detach().cpu().numpy()
    w = torch.cat([gp.weight.detach().reshape(-1) for gp in net.group_projection]).cpu().numpy()
    r = reg_restate(ident, net.scale_num_prototypes, net.num_groups, 1e-5, w, hg, np.zeros((ident.shape[1], ident.shape[0]), np.float32))
    return torch.stack([r["ent"], r["ceg"], r["sm"], r["l1_group"]])


@pytest.mark.parametrize("edit", list(GROUP_TABLE_EDITS))
def test_group_table_caches_follow_the_edit(edit):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    net = _group_net(dev)
    reg = spx.GroupRegularizers(net, group_ent=REG_WEIGHTS[0], crs_ent_group=REG_WEIGHTS[1], scale_max=REG_WEIGHTS[2], l1=REG_WEIGHTS[3],
                                epsilon=1e-5)
    before, rbefore = _check_group_tables(net, dev, reg), _reg_reference(net)
    GROUP_TABLE_EDITS[edit](net)
    after_ref = _reg_reference(net)
    if edit == "scale_item":                                 # only ScaleMax reads the scale ranges
        diff = (after_ref[2] - rbefore[2]).abs().item()
        assert diff >= 100 * REG_TOL * max(1.0, after_ref[2].abs().item()), f"ScaleMax moves by {diff:.3g} only"
    elif edit != "prune":
        _assert_discriminates(before, dict(wd=_dense_reference(net), groups=before["groups"]), ("wd",))
    _check_group_tables(net, dev, reg)
    _check_group_tables(net, dev, reg)


def _group_acts():
    """Group activations [B * GH * GW, GG] of every projection, made so that the class -> projection table decides the value: the
    groups of projection j nearly agree on the pixels of class j and disagree elsewhere, so a class that is served another
    class's projection loses most of its term."""
    def make():
        g = _gen(11)
        lab = _labels(0, group=True).reshape(-1, 1)
        acts = []
        for j in range(GK):
            base, noise = torch.randn(lab.numel(), 1, generator=g), torch.randn(lab.numel(), GG, generator=g)
            acts.append(base + torch.where(lab == j + 1, 0.3 * noise, 3.0 * noise))
        return acts

    return _once("group_acts", make)


def test_the_group_kld_tables_follow_the_group_identity():
    """A long-lived ``KLDLossGroup`` after an in-place swap of two classes' row blocks of ``group_class_identity`` and after a
    re-assignment to such a swapped copy (finetune_wandb_group.py:77-78 re-assigns it)."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    net = _group_net(dev)
    target, acts = _labels(0, group=True), _group_acts()
    tgt, dacts = target.to(dev), [a.to(dev) for a in acts]
    kld = spx.KLDLossGroup(net.prototype_class_identity, net.group_class_identity, GG)

    def check(what):
        ref = O.kld_loss_group([a.double() for a in acts], target, kld.prototype_class_identity.cpu(), kld.group_class_identity.cpu(), GG)
        _scalar_close(kld(dacts, tgt), ref, KLD_TOL, f"group KLD {what}")
        return dict(kld=ref)

    def swapped(a, b):
        rows = list(range(GG * GK))
        rows[a * GG:(a + 1) * GG], rows[b * GG:(b + 1) * GG] = rows[b * GG:(b + 1) * GG], rows[a * GG:(a + 1) * GG]
        return rows

    first = check("as built")
    kld.group_class_identity[swapped(0, 1)] = kld.group_class_identity.clone()          # in place
    second = check("after the in-place swap")
    _assert_losses_discriminate(first, second, ("kld",))
    kld.group_class_identity = kld.group_class_identity[swapped(2, 3)]                   # re-assigned
    third = check("after the re-assignment")
    _assert_losses_discriminate(second, third, ("kld",))
    check("once more")


def test_an_in_place_edit_of_the_returned_activations_voids_the_group_tag():
    """``compute_group(act)`` takes the group activations the forward left on ``act`` (``spx_group``) only while ``act`` is as the
    forward returned it: after an in-place edit it recomputes from the edited values."""
    dev = gpu_device()
    net = _group_net(dev)
    ref = _group_oracle(net)
    with torch.no_grad():
        _, act = net.forward_from_conv_features(_conv(group=True).to(dev), return_activations=True)
        tagged = torch.cat(net.compute_group(act), dim=-1).cpu()
        assert ((tagged - ref["groups"]).abs() <= GROUP_ACT_TOL * (1 + ref["groups"].abs())).all()
        act.mul_(0.5)
        edited = O.compute_group(act.cpu(), ref["ident"], [gp.weight.detach().cpu() for gp in net.group_projection])
        edited = torch.cat(edited, dim=-1)
        _assert_discriminates(dict(groups=ref["groups"]), dict(groups=edited), ("groups",))
        got = torch.cat(net.compute_group(act), dim=-1).cpu()
    assert ((got - edited).abs() <= GROUP_ACT_TOL * (1 + edited.abs())).all()


# ------------------------------------------------------------------------------------------------------------------
# E. the label attachment of ClassDistances
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["same_tensor", "clone", "edited_in_place", "other_labels"])
def test_losses_given_class_distances_and_labels(variant):
    """The planes of a ``ClassDistances`` were gathered under the labels of its forward.  Handed those labels - the very tensor
    or an equal one - the losses give the reference value; handed labels under which some pixel has another class they must
    not give a finite number (the planes cannot be re-gathered): the loss is NaN."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    net = _net(dev)
    target = _labels(1)
    ref = _oracle(net)
    lref = _loss_oracle(net, ref["dist"], target)
    changed = (target + 1) % (K + 1)                         # every class moves to the next one, the last to void, void to class 1
    _assert_losses_discriminate(lref, _loss_oracle(net, ref["dist"], changed), ("kld", "act_terms"))
    kld = spx.KLDLoss(net.prototype_class_identity, S, net.scale_num_prototypes)
    reg = spx.ActivationRegularizers(net.prototype_class_identity, S, net.scale_num_prototypes, *W3, epsilon=net.epsilon)
    tgt = target.to(dev)
    x = _conv().to(dev).requires_grad_(True)
    _, cd = net.forward_from_conv_features(x, target_labels=tgt)
    if variant == "same_tensor":
        given = tgt
    elif variant == "clone":
        given = tgt.clone()
    elif variant == "edited_in_place":
        tgt.copy_(changed.to(dev))
        given = tgt
    else:
        given = changed.to(dev)
    k = kld(cd, given)
    tot, terms = reg(cd, given)
    (k + tot).backward()
    torch.cuda.synchronize()
    if variant in ("same_tensor", "clone"):
        _scalar_close(k, lref["kld"], KLD_TOL, "KLD")
        _scalar_close(terms, lref["act_terms"], ACT_TOL, "activation terms")
        _scalar_close(tot, lref["act_total"], ACT_TOL, "activation total")
        assert torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    else:
        print(f"{variant}: KLD {k.item()}, activation total {tot.item()}, terms {terms.tolist()}")
        assert torch.isnan(k).item(), f"KLD of planes gathered under other labels is {k.item()}"
        assert torch.isnan(tot).item() and torch.isnan(terms).all(), f"activation losses: {tot.item()}, {terms.tolist()}"


def test_the_label_check_does_not_synchronise():
    """The mismatch path (labels that are not the forward's tensor) decides on the device: no host read-back, for equal labels
    and for changed ones."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    net = _net(dev)
    tgt = _labels(1).to(dev)
    equal, other = tgt.clone(), (tgt % K + 1)
    kld = spx.KLDLoss(net.prototype_class_identity, S, net.scale_num_prototypes)
    reg = spx.ActivationRegularizers(net.prototype_class_identity, S, net.scale_num_prototypes, *W3, epsilon=net.epsilon)
    x = _conv().to(dev)

    def step():
        with torch.no_grad():
            _, cd = net.forward_from_conv_features(x, target_labels=tgt)
            return [kld(cd, t) for t in (tgt, equal, other)] + [reg(cd, t)[0] for t in (tgt, equal, other)]

    step()
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
        out = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    vals = [v.item() for v in out]
    assert all(np.isfinite(v) for v in vals[:2] + vals[3:5]) and np.isnan(vals[2]) and np.isnan(vals[5]), vals
    assert vals[0] == vals[1] and vals[3] == vals[4]
