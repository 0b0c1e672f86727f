"""SegmentationMetrics on the GPU (segmentation/eval_valid_multiscale.py:229-275): every integer counter held EXACTLY to
the reference's NumPy counting (restated below with its line numbers) on the pinned bilinear arithmetic
(oracle::upsample_bilinear_restated, the arithmetic spx_upsample_argext and the fused kernels share), and to counters
built with torch from spx_upsample_argext's full-resolution maps."""
import numpy as np
import pytest
import torch

from oracle import ppnet_oracle as O
from support import gpu_device, group_net, Guarded, proto_net
from support import release_cached_blocks  # noqa: F401  (a module-scoped autouse fixture, taken by importing its name)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------
# the reference's counting, restated
# ------------------------------------------------------------------------------------------------------------------
def _restated_maps(src_nchw, size, largest, samples=None, chunk=4):
    """(arg map int64 [N, H, W], values at the sample pixels [N, S, C] or None) of the pinned bilinear map, computed a
    few channels at a time (the float64 restatement of a whole 1024 x 2048 map would not fit in memory)."""
    N, C = src_nchw.shape[:2]
    best = arg = None
    picked = []
    for c0 in range(0, C, chunk):
        up = O.upsample_bilinear_restated(src_nchw[:, c0:c0 + chunk], size)
        for j in range(up.shape[1]):
            v = up[:, j]
            if best is None:
                best, arg = v.clone(), torch.zeros(v.shape, dtype=torch.int64)
            else:
                better = v > best if largest else v < best     # strict: the lowest channel wins a tie
                best = torch.where(better, v, best)
                arg[better] = c0 + j
        if samples is not None:
            n = torch.arange(N)[:, None]
            picked.append(up.permute(0, 2, 3, 1)[n, samples[..., 0].long(), samples[..., 1].long()])
    return arg, (torch.cat(picked, dim=2) if samples is not None else None)


def _reference_counts(pred, ann, K, near=None, cls=None, samp_d=None, samples=None):
    """eval_valid_multiscale.py:236-269 image by image, with the confusion matrix the contract defines beside it."""
    pred, ann = pred.numpy(), ann.numpy().astype(np.int64)
    P = 0 if cls is None else len(cls)
    correct = total = 0
    CLS_I, CLS_U = np.zeros(K, np.int64), np.zeros(K, np.int64)
    counts, topk = np.zeros(P, np.int64), np.zeros(P, np.int64)
    conf = np.zeros((K + 1) * K, np.int64)
    cls2protos = {c: [p for p in range(P) if cls[p] == c] for c in range(K)}       # :107-112
    for n in range(pred.shape[0]):
        pr_n, a = pred[n], ann[n]
        correct += np.sum(((pr_n + 1) == a) & (a != 0))                              # :236
        total += np.sum(a != 0)                                                      # :237
        for c in range(K):                                                           # :239-243
            pr, gt = pr_n == c, a == c + 1
            CLS_I[c] += np.sum(pr & gt)
            CLS_U[c] += np.sum((pr | gt) & (a != 0))
        row = np.where((a >= 1) & (a <= K), a - 1, K)
        conf += np.bincount((row * K + pr_n)[a != 0], minlength=(K + 1) * K)
        if near is not None:                                                         # :245-253
            nr = near[n].numpy()
            near_cls = cls[nr]
            for c in range(K):
                is_class_proto = (pr_n == c) & (near_cls == c)
                for p in cls2protos[c]:
                    counts[p] += np.sum(is_class_proto & (nr == p))
        if samp_d is not None:                                                       # :255-269, stable order
            sd = samp_d[n].numpy()                                                   # [S, P]
            sp = pr_n[samples[n, :, 0].numpy(), samples[n, :, 1].numpy()]
            order = np.argsort(sd, axis=1, kind="stable")
            hit = cls[order] == sp[:, None]
            topk += np.cumsum(hit, axis=1).sum(axis=0)
    return dict(conf=conf.reshape(K + 1, K), I=CLS_I, U=CLS_U, correct=int(correct), total=int(total), hits=counts, topk=topk)


def _check_against_reference(m, ref, K, S_total=None):
    res = m.compute()
    conf = res.confusion.numpy()
    np.testing.assert_array_equal(conf, ref["conf"])
    # everything the reference reports follows from the confusion matrix exactly
    np.testing.assert_array_equal(np.diagonal(conf[:K]), ref["I"])
    np.testing.assert_array_equal(conf[:K].sum(1) + conf.sum(0) - np.diagonal(conf[:K]), ref["U"])
    assert int(np.trace(conf[:K])) == ref["correct"] and int(conf.sum()) == ref["total"]
    if ref["hits"].size:
        np.testing.assert_array_equal(res.prototype_counts.numpy(), ref["hits"])
    if S_total is not None:
        np.testing.assert_array_equal(m.topk.cpu().numpy(), ref["topk"])
        assert res.samples_seen == S_total
    iou = {c: ref["I"][c] * 100 / u for c, u in enumerate(ref["U"]) if u > 0}                  # :272-274
    assert set(res.class_iou) == set(iou)
    for c, v in iou.items():
        assert res.class_iou[c] == pytest.approx(v, rel=1e-12)
    assert res.mean_iou == pytest.approx(float(np.mean(list(iou.values()))), rel=1e-12)
    assert res.pixel_accuracy == pytest.approx(ref["correct"] / ref["total"] * 100, rel=1e-12)
    return res


# (local: labels with values beyond K from the caller's generator; parity_cases.gather_labels draws 0..K from a seed)
def _labels(g, N, H, W, K):
    """Random labels with void (0), every class, and values > K (non-void, no class)."""
    return torch.randint(0, K + 4, (N, H, W), generator=g)


def _samples(g, N, H, W, S=100):
    s = torch.stack([torch.randint(0, H, (N, S), generator=g), torch.randint(0, W, (N, S), generator=g)], dim=2)
    s[:, S - 10:] = s[:, :10]                   # duplicates, as np.random.randint draws them
    return s


def _ident(g, P, K):
    cls = torch.randint(0, K, (P,), generator=g)
    cls[:K] = torch.arange(min(P, K))[:P]       # every class has a prototype where P >= K
    return torch.nn.functional.one_hot(cls, K).float(), cls.numpy()


def _run_restated(N, K, P, h, w, H, W, seed):
    from scaleprotoseg_amd import SegmentationMetrics

    dev = gpu_device()
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(N, h, w, K, generator=g) * 3
    dist = torch.rand(N, P, h, w, generator=g) * 10
    ident, cls = _ident(g, P, K)
    ann = _labels(g, N, H, W, K)
    smp = _samples(g, N, H, W)
    pred, _ = _restated_maps(logits.permute(0, 3, 1, 2), (H, W), True)
    near, samp_d = _restated_maps(dist, (H, W), False, samples=smp)
    ref = _reference_counts(pred, ann, K, near, cls, samp_d, smp)
    m = SegmentationMetrics(K, ident, dev)
    m.update(logits.to(dev), ann.to(dev), dist.to(dev), smp.to(dev))
    res = _check_against_reference(m, ref, K, S_total=N * smp.shape[1])
    k1 = np.arange(1, P + 1)
    np.testing.assert_allclose(res.mean_top_k.numpy(), 100 * ref["topk"] / (k1 * N * smp.shape[1]), rtol=1e-12)
    return res


# (1) the reference's evaluation shapes with a channel subset, ragged and down-sampling maps, wide heads on small maps
@pytest.mark.parametrize("case", [(1, 19, 24, 129, 257, 1024, 2048), (2, 21, 42, 65, 65, 513, 513), (2, 5, 7, 9, 11, 70, 90),
                                  (1, 4, 6, 33, 65, 17, 20), (3, 3, 5, 4, 5, 4, 5), (1, 7, 9, 1, 1, 3, 5),
                                  (1, 150, 300, 12, 14, 50, 61), (1, 182, 364, 9, 9, 40, 44)])
def test_counters_match_restated_reference(case):
    _run_restated(*case, seed=sum(case))


def _torch_counters(pred, near, ann, cls, K, P):
    """Counters from full-resolution maps with torch on the device (the composition a user writes today)."""
    a = ann.long()
    row = torch.where((a >= 1) & (a <= K), a - 1, torch.full_like(a, K))
    nv = a != 0
    conf = torch.bincount((row * K + pred)[nv], minlength=(K + 1) * K).view(K + 1, K)
    hits = None
    if near is not None:
        ok = cls[near] == pred
        hits = torch.bincount(near[ok], minlength=P)
    return conf, hits


def _run_against_argext(N, K, P, h, w, H, W, seed, diag_frac=0.0):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(N, h, w, K, generator=g) * 3).to(dev)
    dist = (torch.rand(N, P, h, w, generator=g) * 10).to(dev)
    ident, cls = _ident(g, P, K)
    pred, _ = spx.upsample_argext(logits.permute(0, 3, 1, 2), (H, W), largest=True)
    near, _ = spx.upsample_argext(dist, (H, W), largest=False)
    ann = _labels(g, N, H, W, K).to(dev)
    if diag_frac:        # a trained model's confusion is heavily diagonal: put most labels on the prediction
        on = torch.rand(N, H, W, generator=g).to(dev) < diag_frac
        ann = torch.where(on, pred + 1, ann)
    m = spx.SegmentationMetrics(K, ident, dev)
    m.update(logits, ann, dist)
    conf, hits = _torch_counters(pred, near, ann, torch.from_numpy(cls).to(dev), K, P)
    assert torch.equal(m.conf, conf)
    assert torch.equal(m.hits, hits)
    return m


# (2) the full Cityscapes shape
def test_cityscapes_full_bank_against_upsample_argext():
    _run_against_argext(1, 19, 228, 129, 257, 1024, 2048, seed=3, diag_frac=0.8)


# (3) wide heads: the confusion matrix no longer fits in LDS whole
@pytest.mark.parametrize("case", [(1, 150, 1800, 64, 64, 512, 512, 0.7), (2, 182, 364, 40, 52, 320, 416, 0.7),
                                  (1, 150, 1800, 64, 64, 512, 512, 0.0)])
def test_wide_heads_against_upsample_argext(case):
    *shape, frac = case
    _run_against_argext(*shape, seed=11, diag_frac=frac)


# (4) layout and accumulation
def _net(kind, dev, P=40, K=10, S=4, Cs=64, G=6):
    import scaleprotoseg_amd as spx

    torch.manual_seed(5)
    if kind == "ppnet":
        net = proto_net(P, K, 1, Cs, cls=spx.PPNet)
        S = 1
    elif kind == "group":
        net = group_net(P, K, S, Cs, G)
    else:
        net = proto_net(P, K, S, Cs)
    net = net.to(dev).eval()
    g = torch.Generator().manual_seed(9)
    conv = torch.randn(2, S * Cs, 17, 23, generator=g).to(dev)
    with torch.no_grad():
        logits, dist = net.forward_from_conv_features(conv)
    return net, logits, dist


def test_strided_logits_equal_contiguous():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    net, logits, dist = _net("ms", dev)
    N, h, w, K = logits.shape
    g = torch.Generator().manual_seed(1)
    ann = _labels(g, N, 129, 181, K).to(dev)
    smp = _samples(g, N, 129, 181).to(dev)
    padded = torch.zeros(N, h, w, K + 3, device=dev)[..., 1:K + 1]
    padded.copy_(logits)
    nchw_storage = logits.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    dist_strided = torch.zeros(N, dist.shape[1], h, w + 5, device=dev)[..., 2:w + 2]
    dist_strided.copy_(dist)
    outs = []
    for lg, d in ((logits, dist), (logits.contiguous(), dist.contiguous()), (padded, dist_strided), (nchw_storage, dist)):
        m = spx.SegmentationMetrics.for_model(net)
        m.update(lg, ann, d, smp)
        outs.append(m._buf.clone())
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    assert not padded.is_contiguous() and not dist_strided.is_contiguous() and not nchw_storage.is_contiguous()


def test_updates_accumulate_and_label_dtypes_agree():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    g = torch.Generator().manual_seed(21)
    N, K, P, h, w, H, W = 6, 12, 36, 11, 13, 87, 101
    logits = torch.randn(N, h, w, K, generator=g).to(dev)
    dist = torch.rand(N, P, h, w, generator=g).to(dev)
    ident, _ = _ident(g, P, K)
    ann = torch.randint(0, 200, (N, H, W), generator=g).to(dev)        # fits uint8; > K values included
    ann[:, :5] = 0
    smp = _samples(g, N, H, W).to(dev)
    one = spx.SegmentationMetrics(K, ident, dev)
    one.update(logits, ann, dist, smp)
    three = spx.SegmentationMetrics(K, ident, dev)
    for sl in (slice(0, 1), slice(1, 4), slice(4, 6)):
        three.update(logits[sl], ann[sl], dist[sl], smp[sl])
    assert torch.equal(one._buf, three._buf)
    for dt in (torch.uint8, torch.int32):
        m = spx.SegmentationMetrics(K, ident, dev)
        m.update(logits, ann.to(dt), dist, smp)
        assert torch.equal(m._buf, one._buf), dt
    conf_only = spx.SegmentationMetrics(K, ident, dev)
    conf_only.update(logits, ann, None)
    assert torch.equal(conf_only.conf, one.conf)
    assert int(conf_only.hits.abs().sum()) == 0
    assert conf_only.compute().mean_top_k is None


# (5) ties
def test_ties_resolve_to_the_lowest_index():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    g = torch.Generator().manual_seed(4)
    N, K, P, h, w, H, W = 1, 6, 8, 7, 9, 30, 40
    logits = torch.full((N, h, w, K), 0.25)                       # constant planes: pred = 0 everywhere
    dist = torch.rand(N, P, h, w, generator=g) + 1
    dist[:, 2] = 0.5                                              # prototypes 2 and 5 are identical and
    dist[:, 5] = 0.5                                              # everyone's nearest
    ident = torch.zeros(P, K)
    ident[torch.arange(P), torch.tensor([0, 1, 0, 2, 3, 0, 4, 5])] = 1
    ann = _labels(g, N, H, W, K)
    smp = _samples(g, N, H, W)
    m = spx.SegmentationMetrics(K, ident, dev)
    m.update(logits.to(dev), ann.to(dev), dist.to(dev), smp.to(dev))
    res = m.compute()
    assert int(res.confusion[:, 1:].sum()) == 0 and int(res.confusion.sum()) == int((ann != 0).sum())
    assert int(res.prototype_counts[2]) == N * H * W and int(res.prototype_counts[5]) == 0
    near, samp_d = _restated_maps(dist, (H, W), False, samples=smp)
    ref = _reference_counts(torch.zeros(N, H, W, dtype=torch.int64), ann, K, near, ident.argmax(1).numpy(), samp_d, smp)
    _check_against_reference(m, ref, K, S_total=N * smp.shape[1])
    # stable order: 2 then 5 are the first two for every sample; both are of class 0 = pred
    assert int(m.topk[0]) == 100 and int(m.topk[1]) == 200


# (6) end to end through the modules
@pytest.mark.parametrize("kind", ["group", "ppnet", "ms"])
def test_module_forward_to_compute(kind):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    net, logits, dist = _net(kind, dev)
    N, h, w, K = logits.shape
    H, W = 120, 150
    g = torch.Generator().manual_seed(8)
    ann = _labels(g, N, H, W, K)
    smp = _samples(g, N, H, W)
    m = spx.SegmentationMetrics.for_model(net)
    m.update(logits, ann.to(dev), dist, smp.to(dev))
    cls = net.prototype_class_identity.cpu().argmax(1).numpy()
    pred, _ = _restated_maps(logits.cpu().permute(0, 3, 1, 2), (H, W), True)
    near, samp_d = _restated_maps(dist.cpu(), (H, W), False, samples=smp)
    ref = _reference_counts(pred, ann, K, near, cls, samp_d, smp)
    res = _check_against_reference(m, ref, K, S_total=N * smp.shape[1])
    ref_counts = res.class_prototype_counts()
    for c in range(K):
        protos = [p for p in range(len(cls)) if cls[p] == c]
        assert [ref_counts[c][i] for i in range(len(protos))] == [int(ref["hits"][p]) for p in protos]


# (7) update never waits for the device: it captures into a graph, and (where torch honours it) raises nothing under
# the sync debug mode
def test_update_does_not_synchronise():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    g = torch.Generator().manual_seed(13)
    N, K, P, h, w, H, W = 2, 9, 27, 10, 12, 80, 96
    logits = torch.randn(N, h, w, K, generator=g).to(dev)
    dist = torch.rand(N, P, h, w, generator=g).to(dev)
    ident, _ = _ident(g, P, K)
    ann = _labels(g, N, H, W, K).to(dev)
    smp = _samples(g, N, H, W).to(dev).to(torch.int32)
    ref = spx.SegmentationMetrics(K, ident, dev)
    ref.update(logits, ann, dist, smp)
    m = spx.SegmentationMetrics(K, ident, dev)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.update(logits, ann, dist, smp)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(m._buf, ref._buf)
    m.reset()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            m.update(logits, ann, dist, smp)
    torch.cuda.current_stream().wait_stream(s)
    m.reset()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(m._buf, 2 * ref._buf)


# (8) nothing lands outside the counter buffers
@pytest.mark.parametrize("case", [(1, 3, 5, 3, 4, 5, 7), (2, 19, 37, 9, 13, 65, 67), (1, 150, 1800, 5, 6, 33, 45),
                                  (3, 182, 364, 7, 3, 19, 100), (1, 91, 91, 4, 4, 4, 4)])
def test_no_write_outside_the_counters(case):
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd.metrics import eval_accumulate, eval_topk

    dev = gpu_device()
    N, K, P, h, w, H, W = case
    g = torch.Generator().manual_seed(sum(case))
    logits = torch.randn(N, h, w, K, generator=g).to(dev)
    dist = torch.rand(N, P, h, w, generator=g).to(dev)
    ident, _ = _ident(g, P, K)
    ann = _labels(g, N, H, W, K).to(dev)
    smp = _samples(g, N, H, W).to(dev)
    ref = spx.SegmentationMetrics(K, ident, dev)
    ref.update(logits, ann, dist, smp)
    guarded = [Guarded(8 * n, dev) for n in ((K + 1) * K, P, P, 1)]
    conf, hits, topk, seen = (g.body(torch.int64).zero_() for g in guarded)          # zeroed int64 counters between the bands
    eval_accumulate(logits, ann, conf, dist, ref.proto_class, hits)
    eval_topk(logits, dist, ref.proto_class, smp, (H, W), topk, seen)
    torch.cuda.synchronize()
    assert all(g.intact() for g in guarded)
    assert torch.equal(conf.view(K + 1, K), ref.conf) and torch.equal(hits, ref.hits)
    assert torch.equal(topk, ref.topk) and torch.equal(seen, ref.samples_seen)
