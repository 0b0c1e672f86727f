"""CPU checks of the evaluation metrics: the float64 finalisation from hand-built counters, the host-side argument checks
of the C entries (no GPU is touched), the refusal of CPU tensors, and the sum of two ranks' counters over gloo."""
import ctypes as C
import math
import os

import pytest
import torch

from support import run_gloo


@pytest.fixture(scope="module")
def lib():
    from scaleprotoseg_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        from scaleprotoseg_amd.build import build

        build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------------
# finalisation (eval_valid_multiscale.py:272-275)
# ------------------------------------------------------------------------------------------------------------------
def test_finalize_iou_accuracy_and_other_label_row():
    from scaleprotoseg_amd.metrics import finalize

    K = 4
    conf = torch.zeros(K + 1, K, dtype=torch.int64)
    conf[0, 0], conf[0, 1] = 6, 2          # class 0: 6 right, 2 predicted as 1
    conf[1, 1] = 3
    conf[2, 0] = 1                         # class 2 never predicted right: I = 0, U = 1
    conf[K, 1] = 5                         # "other label" pixels predicted as class 1
    # class 3: no label, never predicted -> U = 0, left out
    res = finalize(conf)
    assert res.pixel_accuracy == pytest.approx(100.0 * 9 / 17)      # the other-label row counts into total
    # U_0 = 8 + 7 - 6 = 9; U_1 = 3 + (2 + 3 + 5) - 3 = 10 (other-label row in class 1's union, not its intersection)
    assert set(res.class_iou) == {0, 1, 2}
    assert res.class_iou[0] == pytest.approx(100.0 * 6 / 9)
    assert res.class_iou[1] == pytest.approx(100.0 * 3 / 10)
    assert res.class_iou[2] == 0.0
    assert res.mean_iou == pytest.approx((100.0 * 6 / 9 + 100.0 * 3 / 10 + 0.0) / 3)
    assert res.mean_top_k is None and res.prototype_counts is None


def test_finalize_nothing_seen():
    from scaleprotoseg_amd.metrics import finalize

    res = finalize(torch.zeros(3, 2, dtype=torch.int64))
    assert res.class_iou == {} and math.isnan(res.mean_iou) and math.isnan(res.pixel_accuracy)


def test_mean_top_k_denominator():
    from scaleprotoseg_amd.metrics import finalize

    topk = torch.tensor([3, 7, 9], dtype=torch.int64)
    res = finalize(torch.zeros(3, 2, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), topk, samples_seen=5)
    # 100 * topk[k] / ((k + 1) * samples actually seen)
    assert res.mean_top_k.tolist() == pytest.approx([100 * 3 / 5, 100 * 7 / 10, 100 * 9 / 15])
    assert finalize(torch.zeros(3, 2, dtype=torch.int64), None, topk, samples_seen=0).mean_top_k is None


def test_prototype_class_is_the_first_argmax():
    from scaleprotoseg_amd.metrics import finalize, prototype_classes

    ident = torch.tensor([[0.0, 1.0, 1.0], [0.5, 0.5, 0.0], [0.0, 0.0, 1.0], [0.2, 0.9, 0.9], [1.0, 0.0, 0.0]])
    cls = prototype_classes(ident)
    assert cls.dtype == torch.int32 and cls.tolist() == [1, 0, 2, 1, 0]
    hits = torch.tensor([4, 1, 2, 8, 3], dtype=torch.int64)
    res = finalize(torch.zeros(4, 3, dtype=torch.int64), hits, None, 0, cls)
    # the reference's {class: Counter({index among the class's prototypes: count})} (:98, :107-112, :245-253)
    per = res.class_prototype_counts()
    assert per[0] == {0: 1, 1: 3} and per[1] == {0: 4, 1: 8} and per[2] == {0: 2}


# ------------------------------------------------------------------------------------------------------------------
# host-side validation of the C entries: nothing reaches a device
# ------------------------------------------------------------------------------------------------------------------
FAKE = 0x1000          # never dereferenced: every call below fails its argument checks first


def _st(*v):
    return (C.c_int64 * 4)(*v)


def _acc(lib, **kw):
    a = dict(logits=FAKE, lst=_st(1, 1, 1, 1), dist=FAKE, dst=_st(1, 1, 1, 1), cls=FAKE, labels=FAKE, lb=8, N=1, K=19, P=228,
             h=4, w=4, H=8, W=8, conf=FAKE, hits=FAKE)
    a.update(kw)
    return lib.spx_eval_accumulate(a["logits"], a["lst"], a["dist"], a["dst"], a["cls"], a["labels"], a["lb"], a["N"], a["K"],
                                   a["P"], a["h"], a["w"], a["H"], a["W"], a["conf"], a["hits"], None)


def _topk(lib, **kw):
    a = dict(logits=FAKE, lst=_st(1, 1, 1, 1), dist=FAKE, dst=_st(1, 1, 1, 1), cls=FAKE, samples=FAKE, sb=8, N=1, S=100, K=19,
             P=228, h=4, w=4, H=8, W=8, topk=FAKE, seen=FAKE)
    a.update(kw)
    return lib.spx_eval_topk(a["logits"], a["lst"], a["dist"], a["dst"], a["cls"], a["samples"], a["sb"], a["N"], a["S"], a["K"], a["P"],
                             a["h"], a["w"], a["H"], a["W"], a["topk"], a["seen"], None)


@pytest.mark.parametrize("kw,msg", [
    (dict(logits=None), "NULL"), (dict(labels=None), "NULL"), (dict(conf=None), "NULL"), (dict(lst=None), "NULL"),
    (dict(hits=None), "hit counters"), (dict(cls=None), "prototype classes"), (dict(dst=None), "NULL distance strides"),
    (dict(lb=2), "label byte code"), (dict(lb=0), "label byte code"), (dict(N=0), "empty"), (dict(K=0), "empty"),
    (dict(H=0), "empty"), (dict(w=-1), "empty"), (dict(K=1025), "classes"), (dict(P=0), "prototypes"), (dict(P=4097), "prototypes"),
    (dict(N=4, H=32768, W=32768), "too large"), (dict(lst=_st(1, -1, 1, 1)), "negative"), (dict(dst=_st(1, 1, -4, 1)), "negative"),
])
def test_accumulate_rejects_bad_arguments(lib, kw, msg):
    assert _acc(lib, **kw) != 0
    assert msg in lib.spx_last_error().decode()
    assert lib.spx_last_error().decode().startswith("spx_eval_accumulate")


@pytest.mark.parametrize("kw,msg", [
    (dict(dist=None), "NULL"), (dict(samples=None), "NULL"), (dict(topk=None), "NULL"), (dict(cls=None), "NULL"),
    (dict(logits=None), "NULL"), (dict(S=0), "sample count"), (dict(N=1 << 12, S=1 << 12), "sample count"), (dict(sb=2), "sample byte code"),
    (dict(P=5000), "prototypes"), (dict(K=2000), "classes"), (dict(h=0), "empty"),
])
def test_topk_rejects_bad_arguments(lib, kw, msg):
    assert _topk(lib, **kw) != 0
    assert msg in lib.spx_last_error().decode()
    assert lib.spx_last_error().decode().startswith("spx_eval_topk")


def test_class_table_check(lib):
    ok = (C.c_int32 * 4)(0, 2, 1, 2)
    assert lib.spx_eval_check_classes(ok, 4, 3) == 0
    bad = (C.c_int32 * 4)(0, 3, 1, 2)
    assert lib.spx_eval_check_classes(bad, 4, 3) != 0
    assert "prototype 1 has class 3 outside [0, 3)" in lib.spx_last_error().decode()
    neg = (C.c_int32 * 2)(0, -1)
    assert lib.spx_eval_check_classes(neg, 2, 3) != 0
    assert lib.spx_eval_check_classes(None, 2, 3) != 0
    assert lib.spx_eval_check_classes(ok, 0, 3) != 0


def test_cpu_tensors_are_refused(lib):
    from scaleprotoseg_amd import SegmentationMetrics, SpxError
    from scaleprotoseg_amd.metrics import eval_accumulate, eval_topk

    with pytest.raises(SpxError, match="GPU only"):
        SegmentationMetrics(3, torch.eye(3), "cpu")
    logits, labels = torch.zeros(1, 2, 2, 3), torch.zeros(1, 4, 4, dtype=torch.int64)
    dist, cls = torch.zeros(1, 3, 2, 2), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(SpxError, match="no CPU fallback"):
        eval_accumulate(logits, labels, torch.zeros(12, dtype=torch.int64), dist, cls, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(SpxError, match="no CPU fallback"):
        eval_topk(logits, dist, cls, torch.zeros(1, 5, 2, dtype=torch.int64), (4, 4), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(SpxError, match="int32 or int64"):
        eval_topk(logits, dist, cls, torch.zeros(1, 5, 2, dtype=torch.int16), (4, 4), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(SpxError, match="uint8, int32 or int64"):
        eval_accumulate(logits, labels.to(torch.int16), torch.zeros(12, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------------------------
# all_reduce over gloo, world size 2 (the same code runs over RCCL)
# ------------------------------------------------------------------------------------------------------------------
class _HostMetrics:
    """SegmentationMetrics' counter buffer and finalisation on the host (no kernel is involved in the exchange)."""

    def __init__(self, K, ident, buf):
        from scaleprotoseg_amd.metrics import SegmentationMetrics

        m = SegmentationMetrics.__new__(SegmentationMetrics)
        m.num_classes, m.num_prototypes = K, ident.shape[0]
        m.prototype_class_host = torch.argmax(ident, 1).to(torch.int32)
        m._buf = buf
        self.m = m


def _counters(rank, K, P):
    g = torch.Generator().manual_seed(40 + rank)
    n = (K + 1) * K
    buf = torch.zeros(n + 2 * P + 1, dtype=torch.int64)
    buf[:n] = torch.randint(0, 50, (n,), generator=g)
    buf[n:n + 2 * P] = torch.randint(0, 30, (2 * P,), generator=g)
    buf[-1] = 7 + rank
    return buf


def _all_reduce_case(rank, world):
    K, P = 5, 10
    hm = _HostMetrics(K, torch.eye(K).repeat(2, 1), _counters(rank, K, P))
    hm.m.all_reduce()
    return hm.m._buf


def test_all_reduce_sums_two_ranks(tmp_path):
    bufs = run_gloo(_all_reduce_case, tmp_path)
    K, P = 5, 10
    total = _counters(0, K, P) + _counters(1, K, P)
    assert torch.equal(bufs[0], total) and torch.equal(bufs[1], total)
    a = _HostMetrics(K, torch.eye(K).repeat(2, 1), bufs[0]).m.compute()
    b = _HostMetrics(K, torch.eye(K).repeat(2, 1), total).m.compute()
    assert a.class_iou == b.class_iou and a.mean_iou == b.mean_iou and a.pixel_accuracy == b.pixel_accuracy
    assert torch.equal(a.confusion, b.confusion) and torch.equal(a.prototype_counts, b.prototype_counts)
    assert torch.equal(a.mean_top_k, b.mean_top_k) and a.samples_seen == b.samples_seen == 15
