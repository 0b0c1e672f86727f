"""Record the reference's ``PPNetMultiScale.forward`` in TRAINING mode on MSC's four maps (model_multiscale.py:332-388), on the CPU:

    SPX_REFERENCE=<reference checkout> python tools/gen_msc_packed_golden.py

builds the reference's REAL class (stub modules of oracle/gen_golden.py for the packages the checkout imports, as
tools/gen_scale_head_golden.py does), replaces its ``conv_features`` by a recorded list of four bf16-representable maps - what
``MSC`` hands out in training, ``[full] + pyramid + [max]``: the ``odd`` grids of tools/gen_msc_golden.py, 7 x 9, 4 x 5, 6 x 7, and a
fourth map on the first grid - and calls ``forward(x, **flags)`` in the three tuple modes.  It writes data only:
tests/golden/msc_packed_forward.npz with "case__field" keys (tests/support.py::load_cases), one case ``train``:

    conv0 .. conv3       the maps, float32 [B, S Cs, h_k, w_k], bf16-representable
    bank, head           prototype_vectors [P, Cs, 1, 1] (bf16-representable) and last_layer.weight [K, P]
    identity, scale_ranges, shape = (B, S, Cs, P, K)
    grids                the (h_k, w_k) in list order
    logits0.., distances0.., activations0..     the entries of the segments' tuples
    tuple_lengths        per mode (default, return_activations, return_activations + return_distances) the length of every tuple

The three modes return the same tensors at the positions the reference states (:378-385): asserted here, so each is stored once."""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import gen_golden as GG  # noqa: E402

SEED = 20261021
B, S, Cs, P, K = 2, 2, 16, 12, 3
GRIDS = ((7, 9), (4, 5), (6, 7), (7, 9))


def main():
    GG._install_stubs()
    ref = os.environ.get("SPX_REFERENCE")
    if not ref:
        sys.exit("set SPX_REFERENCE to the reference checkout")
    sys.path.insert(0, ref)
    import segmentation.model.model_multiscale as ms

    torch.set_num_threads(1)
    torch.manual_seed(SEED)
    net = ms.PPNetMultiScale(features=GG._Backbone(Cs * S), img_size=64, prototype_shape=(P, Cs, 1, 1), proto_layer_rf_info=[],
                             num_classes=K, init_weights=True, add_on_layers_type="deeplab_simple", patch_classification=True,
                             num_scales=S)
    with torch.no_grad():
        net.prototype_vectors.copy_(GG._bf16r(net.prototype_vectors))
        net.last_layer.weight.add_(0.05 * torch.randn_like(net.last_layer.weight))
    maps = [GG._bf16r(torch.sigmoid(torch.randn(B, S * Cs, h, w))) for h, w in GRIDS]
    net.conv_features = lambda x: list(maps)
    net.train()
    x = torch.zeros(B, 3, 8, 8)                      # never read
    with torch.no_grad():
        default = net(x)
        acts = net(x, return_activations=True)
        full = net(x, return_activations=True, return_distances=True)
    assert isinstance(full, list) and len(default) == len(acts) == len(full) == len(GRIDS)
    out = {"train__shape": np.array((B, S, Cs, P, K), dtype=np.int64), "train__grids": np.array(GRIDS, dtype=np.int64),
           "train__bank": GG._np(net.prototype_vectors), "train__head": GG._np(net.last_layer.weight),
           "train__identity": GG._np(net.prototype_class_identity),
           "train__scale_ranges": np.array([net.scale_num_prototypes[s] for s in range(S)], dtype=np.int64),
           "train__tuple_lengths": np.array([[len(t) for t in mode] for mode in (default, acts, full)], dtype=np.int64)}
    for k, (m, d, a, f) in enumerate(zip(maps, default, acts, full)):
        logits, dist, act = f
        assert len(d) == 2 and torch.equal(d[0], logits) and torch.equal(d[1], dist)
        assert len(a) == 2 and torch.equal(a[0], logits) and torch.equal(a[1], act)
        h, w = GRIDS[k]
        assert tuple(logits.shape) == (B, h, w, K) and tuple(dist.shape) == (B, P, h, w) and tuple(act.shape) == (B * h * w, P)
        out[f"train__conv{k}"] = GG._np(m)
        out[f"train__logits{k}"] = GG._np(logits)
        out[f"train__distances{k}"] = GG._np(dist)
        out[f"train__activations{k}"] = GG._np(act)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "..", "tests", "golden", "msc_packed_forward.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
