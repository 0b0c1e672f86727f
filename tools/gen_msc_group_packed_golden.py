"""Record the reference's group-phase TRAINING step on MSC's four maps (model_multiscale_group.py:396-452, trainer loop
module_multiscale_group_train.py:232-310), on the CPU:

    SPX_REFERENCE=<reference checkout> python tools/gen_msc_group_packed_golden.py

builds the reference's REAL group class (stub modules of oracle/gen_golden.py for the packages the checkout imports) on the net of
``case_group_train_step``, replaces its ``conv_features`` by four bf16-representable maps on the grids of
tools/gen_msc_packed_golden.py (7 x 9, 4 x 5, 6 x 7, 7 x 9), calls ``net(x, return_activations=True, return_distances=True)`` in
training mode and walks the trainer's loop: per segment ``compute_group``, the targets resized with the reference's
``resize_label``, ``PixelWiseCrossEntropyLoss(ignore_index=-1, return_correct=True)``, ``KLDLossGroup`` and a linear term on the
distances (standing in for the other distance-side losses); the loss is the mean over the segments.  It writes data only:
tests/golden/msc_group_packed_step.npz with "case__field" keys (tests/support.py::load_cases), one case ``step``:

    conv0 .. conv3, bank, last_layer_group, group_w_i, identity, group_identity, scale_ranges, shape = (B, S, Cs, P, K, G)
    grids, target (the full-size label map), target0 .. target3 (resized), g_dist0 .., w_kld
    logits0.., distances0.., activations0.., group_cat0..            the segments' outputs and cat(compute_group)
    ce [4], n_correct [4], n_valid [4], kld [4], loss []             the trainer's per-segment values and the mean loss
    d_conv0 .. d_conv3, d_bank, d_last_layer_group, d_group_w_i      every gradient of ``loss``"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import gen_golden as GG  # noqa: E402

B, S, Cs, K, P, G = 2, 4, 16, 5, 40, 3          # the net of oracle/gen_golden.py::case_group_train_step
GRIDS = ((7, 9), (4, 5), (6, 7), (7, 9))
TARGET_HW = (28, 36)
W_KLD = 0.25


def main():
    GG._install_stubs()
    ref = os.environ.get("SPX_REFERENCE")
    if not ref:
        sys.exit("set SPX_REFERENCE to the reference checkout")
    sys.path.insert(0, ref)
    import segmentation.model.model_multiscale as ms
    import segmentation.model.model_multiscale_group as msg
    import segmentation.model.loss as lossmod
    from segmentation.data.dataset import resize_label

    torch.set_num_threads(1)
    torch.manual_seed(GG.SEED + 5)
    old = GG._make_proto_phase(ms, P=P, Cs=Cs, S=S, K=K)
    net = msg.PPNetMultiScale(
        features=GG._Backbone(Cs * S), img_size=64, prototype_shape=(P, Cs, 1, 1), proto_layer_rf_info=[], num_classes=K,
        init_weights=True, add_on_layers_type="deeplab_simple", patch_classification=True, num_scales=S, num_groups=G,
    )
    net.load_state_dict(old.state_dict(), strict=False)
    with torch.no_grad():
        net.last_layer_group.weight.add_(0.05 * torch.randn_like(net.last_layer_group.weight))
    maps = [GG._bf16r(torch.sigmoid(torch.randn(B, S * Cs, h, w))).requires_grad_(True) for h, w in GRIDS]
    mcs_target = torch.randint(0, K + 1, (B,) + TARGET_HW).numpy().astype(np.float32)
    g_dists = [torch.randn(B, P, h, w) * 1e-3 for h, w in GRIDS]
    net.conv_features = lambda x: list(maps)
    net.train()
    outs = net(torch.zeros(B, 3, 8, 8), return_activations=True, return_distances=True)
    assert isinstance(outs, list) and len(outs) == len(GRIDS)
    ce_fn = lossmod.PixelWiseCrossEntropyLoss(ignore_index=-1, return_correct=True)
    kld_fn = lossmod.KLDLossGroup(net.prototype_class_identity, net.group_class_identity, G)
    out = {"step__shape": np.array((B, S, Cs, P, K, G), dtype=np.int64), "step__grids": np.array(GRIDS, dtype=np.int64),
           "step__bank": GG._np(net.prototype_vectors), "step__last_layer_group": GG._np(net.last_layer_group.weight),
           "step__identity": GG._np(net.prototype_class_identity), "step__group_identity": GG._np(net.group_class_identity),
           "step__scale_ranges": np.array([net.scale_num_prototypes[s] for s in range(S)], dtype=np.int64),
           "step__target": mcs_target.astype(np.int64), "step__w_kld": np.float32(W_KLD)}
    mcs_loss, ces, klds, n_correct, n_valid = 0.0, [], [], [], []
    for k, outputs in enumerate(outs):                                   # module_multiscale_group_train.py:232-310
        output, prototype_distances, prototype_activations = outputs
        groups = net.compute_group(prototype_activations)
        target = torch.stack([resize_label(t, size=(output.shape[2], output.shape[1])) for t in mcs_target], dim=0)
        assert bool((target > 0).any()), f"segment {k} has no valid pixel"
        cross_entropy, correct = ce_fn(predicted_logits=output, target_labels=target)
        kld_loss = kld_fn(list_group_activation=groups, target_labels=target)
        loss = cross_entropy + W_KLD * kld_loss + (prototype_distances * g_dists[k]).sum()
        mcs_loss = mcs_loss + loss / len(outs)
        ces.append(cross_entropy.item())
        klds.append(kld_loss.item())
        n_correct.append(int(torch.sum(correct)))
        n_valid.append(int(correct.shape[0]))
        h, w = GRIDS[k]
        assert tuple(output.shape) == (B, h, w, K) and tuple(prototype_distances.shape) == (B, P, h, w)
        out[f"step__target{k}"] = target.numpy().astype(np.int64)
        out[f"step__g_dist{k}"] = GG._np(g_dists[k])
        out[f"step__logits{k}"] = GG._np(output)
        out[f"step__distances{k}"] = GG._np(prototype_distances)
        out[f"step__activations{k}"] = GG._np(prototype_activations)
        out[f"step__group_cat{k}"] = GG._np(torch.cat(groups, dim=-1))
    net.zero_grad()
    mcs_loss.backward()
    out.update({"step__ce": np.array(ces, dtype=np.float32), "step__kld": np.array(klds, dtype=np.float32),
                "step__n_correct": np.array(n_correct, dtype=np.int64), "step__n_valid": np.array(n_valid, dtype=np.int64),
                "step__loss": GG._np(mcs_loss), "step__d_bank": GG._np(net.prototype_vectors.grad),
                "step__d_last_layer_group": GG._np(net.last_layer_group.weight.grad)})
    for k, m in enumerate(maps):
        out[f"step__conv{k}"] = GG._np(m)
        out[f"step__d_conv{k}"] = GG._np(m.grad)
    for i, gp in enumerate(net.group_projection):
        out[f"step__group_w_{i}"] = GG._np(gp.weight)
        out[f"step__d_group_w_{i}"] = GG._np(gp.weight.grad)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "..", "tests", "golden", "msc_group_packed_step.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "ce", ces, "kld", klds, "correct", n_correct, "valid", n_valid)
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
