"""Push problems shared by the CPU rehearsals and the GPU suites: the pooled-backbone problem of tests/test_gpu_modules.py,
the feature-image problem of the single-pass push's CPU tests with its oracle-based device steps, and the comparison of the
model state two pushes leave behind."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import push_merge_restatement as R
from oracle import ppnet_oracle as O
from support import RoundBf16, proto_net


class PushDataset:
    """len / [i] -> (image [3,h,w] float, target [h,w] int with 0 = void, 1..K); see scaleprotoseg_amd/push.py."""

    convert_targets = None

    def __init__(self, n, h, w, K, absent, seed):
        gen = torch.Generator().manual_seed(seed)
        self.items = []
        for i in range(n):
            img = torch.randn(3, h, w, generator=gen)
            t = torch.randint(0, K + 1, (h // 8, w // 8), generator=gen).repeat_interleave(8, 0).repeat_interleave(8, 1)
            t[t == absent + 1] = 0                          # class `absent` never appears anywhere
            self.items.append((img, t.numpy().astype(np.int64)))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def bf16_bank_with_a_duplicate(net):
    """``init`` of a push problem: a bf16-representable bank whose prototypes 0 and 1 (same class, same scale) start equal, so
    that both win the same pixel - a forced duplicate."""
    net.prototype_vectors.copy_(O.bf16_representable(net.prototype_vectors.data))
    net.prototype_vectors[1].copy_(net.prototype_vectors[0])


def push_problem(dev, S=4, Cs=16, K=5, per=2, n_img=6, seed=3):
    """(net on a pooling backbone, images of 40 x 56 with class 3 absent, P)"""
    P = S * K * per
    net = proto_net(P, K, S, Cs, seed=seed, backbone="pool", add_on=nn.Sequential(nn.Sigmoid(), RoundBf16()),
                    init=bf16_bank_with_a_duplicate, device=dev)
    return net, PushDataset(n_img, 40, 56, K, absent=3, seed=seed + 1), P


def patch_kernels_with_oracle(S):
    """compute_distances / argmin_over_images on the CPU oracle (tests may use it; the product path never does)."""
    from scaleprotoseg_amd import push as push_mod

    def compute_distances(ppnet, dataset, img, target, num_classes, max_dist=1e10, device=None, void_class=None):
        conv = ppnet.conv_features(img.unsqueeze(0))
        ranges = {s: tuple(ppnet.scale_num_prototypes[s]) for s in range(S)}
        d = O.scale_l2_convolution(conv, ppnet.prototype_vectors.detach(), ranges, S)
        lab = O.resize_label(target, (d.shape[3], d.shape[2])).unsqueeze(0)
        return O.push_masked_argmin(d, lab, ppnet.prototype_class_identity, num_classes, max_dist, void_class)

    push_mod.compute_distances = compute_distances
    push_mod.argmin_over_images = lambda v: v.argmin(dim=0)


QUIET = dict(log=lambda *_: None, device="cpu")


class FeatureData:
    """Feature "images" of the given latent (h, w) sizes in order; targets at four times that size, one label per latent
    pixel, class ``absent`` never appears."""

    convert_targets = None

    def __init__(self, sizes, K, absent, seed, channels=None):
        g = torch.Generator().manual_seed(seed)
        self.items = []
        for h, w in sizes:
            img = torch.rand(channels or S_ * CS_, h, w, generator=g)
            t = torch.randint(0, K + 1, (h, w), generator=g).repeat_interleave(4, 0).repeat_interleave(4, 1)
            t[t == absent + 1] = 0
            self.items.append((img, t.numpy()))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


S_, CS_, K_, PER_ = 2, 16, 3, 2
SAME = [(6, 8)] * 7
MIXED = [(6, 8)] * 2 + [(8, 10)] * 3 + [(6, 8)] + [(8, 6)]                # runs break at 2, 5 and 6


def feature_problem(sizes):
    """(CPU net on the identity backbone with a forced duplicate, feature images of ``sizes`` with class 2 absent)"""
    net = proto_net(S_ * K_ * PER_, K_, S_, CS_, seed=11, add_on=nn.Identity(),
                    init=lambda net: net.prototype_vectors[1].copy_(net.prototype_vectors[0]))
    return net, FeatureData(sizes, K_, absent=2, seed=12)


def replace_device_steps():
    """push_run_minima / push_run_merge on the oracle and the restatement (tests only; the product path never does)."""
    from scaleprotoseg_amd import push as push_mod

    def minima(net, conv, labels, void_class, max_dist=1e10):
        ranges = {s: tuple(net.scale_num_prototypes[s]) for s in range(net.num_scales)}
        d = O.scale_l2_convolution(conv, net.prototype_vectors.detach(), ranges, net.num_scales)
        return O.push_masked_argmin(d, labels, net.prototype_class_identity, net.num_classes, max_dist, void_class)

    def merge(table, idx, val, conv, proto_scale, image0):
        B = table.check(idx, val, conv, proto_scale, image0)
        R.merge(dict(best_value=table.best_value, best_image=table.best_image, best_flat=table.best_flat,
                     best_patch=table.best_patch), idx, val, conv, proto_scale, image0)
        table.next_image = int(image0) + B

    push_mod.push_run_minima = minima
    push_mod.push_run_merge = merge


@pytest.fixture
def steps(monkeypatch):
    """Both paths on the CPU for one test: today's compute_distances / argmin_over_images as ``patch_kernels_with_oracle`` replaces
    them, and the single pass's two device steps; everything is put back afterwards."""
    from scaleprotoseg_amd import push as push_mod

    for name in ("compute_distances", "argmin_over_images", "push_run_minima", "push_run_merge"):
        monkeypatch.setattr(push_mod, name, getattr(push_mod, name))        # registers the restore
    patch_kernels_with_oracle(S_)
    replace_device_steps()


def push_state(net, root=None):
    """What a push leaves behind, as CPU copies: bank, scale ranges, head, class identity and, with ``root``, the saved json."""
    out = dict(bank=net.prototype_vectors.detach().cpu().clone(),
               ranges={s: tuple(net.scale_num_prototypes[s]) for s in range(net.num_scales)},
               last=net.last_layer.weight.detach().cpu().clone(), ident=net.prototype_class_identity.cpu().clone())
    if root is not None:
        out["json"] = json.load(open(os.path.join(root, "unique_prototypes.json")))
    return out


def same_push_state(a, b):
    for k in ("bank", "last", "ident"):
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    assert a["ranges"] == b["ranges"] and a.get("json") == b.get("json"), (a["ranges"], b["ranges"])
