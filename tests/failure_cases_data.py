"""The reference-recorded failure cases (tools/gen_failure_golden.py -> tests/golden/failure_cases.npz), shared by the CPU and
GPU tests, with what the tests read off a case.  Fields of a case: ``kind`` (proto / group), ``threshold``, ``logits``
[N, h, w, K], ``labels`` [N, H, W] in 0..K, ``cases`` [F, 3] = (n, a, miss), ``logged_iou`` [F] (the reference's "%.4f") and ``counts`` [F, 2] (its CLS_I and CLS_U),
``table``, the planes' source (``distances`` + ``ident``, or ``activations`` + ``head``), and per kind ``<kind>_rows`` [R, 4],
``<kind>_heat`` [R, H, W], ``<kind>_ranges`` [Q, 2], ``<kind>_flagged`` (where the reference's conversion is undefined; zeros
are recorded there).  The proto case also holds eval_test.py's ``test_logits``, ``test_lut`` and ``test_pred``."""
import numpy as np
import torch

from support import group_net, load_cases, planes_of, proto_net

CASES = load_cases("failure_cases")
activations_of = planes_of


def net_tables(case, device=None):
    """(a real module whose tables are the case's, make(cls, net, threshold, **kw) -> the FailureCases of the case's kind)."""
    K = int(case["table"].shape[0])
    if str(case["kind"]) == "proto":
        ident = torch.from_numpy(case["ident"])
        net = proto_net(ident.shape[0], K, 2, 16, seed=3, device=device).eval()
        assert tuple(net.prototype_class_identity.shape) == tuple(ident.shape)
        net.prototype_class_identity.data.copy_(ident)
        return net, lambda cls, n, thr, **kw: cls.for_prototypes(n, thr, **kw)
    G = int(case["table"].shape[1])
    net = group_net(12, K, 2, 16, G, seed=3, device=device).eval()
    assert tuple(net.last_layer_group.weight.shape) == tuple(case["head"].shape)
    return net, lambda cls, n, thr, **kw: cls.for_groups(n, thr, **kw)


def as_batch(case, BatchFailures, fr):
    """The restatement's BatchFailures of a case, host tensors: what ``rows_for`` takes without a device."""
    K = int(case["table"].shape[0])
    k_star = fr.argmax_map(case["logits"], case["labels"].shape[1:])
    conf = fr.confusion(k_star, case["labels"], K)
    iou, miss, fail = fr.failure_table(conf, float(case["threshold"]))
    return BatchFailures(torch.from_numpy(k_star.astype(np.uint8)), torch.from_numpy(conf), torch.from_numpy(iou), torch.from_numpy(miss),
                         torch.from_numpy(fail))
