"""Record the reference's PPNetMultiScale with a scale head (scale_head_type "sum" / "mult" / "concat"), both phases, on the CPU:

    SPX_REFERENCE=<reference checkout> python tools/gen_scale_head_golden.py

builds the reference's REAL classes (stub modules of oracle/gen_golden.py for the packages the checkout imports) and writes data
only: tests/golden/scale_head.npz (shape G1) and tests/golden/scale_head_g2_<head>.npz (shape G2, one file per head type so that
every file stays below 1 MiB).  Keys are "case__field" (tests/support.py::load_cases):

    <G>                  conv, g_logits, g_dist, g_act, scale_ranges, shape = (B, S, Cs, P, K, H, W, groups)
    <G>_<head>           distances, activations of forward_from_conv_features (identical in both phases: asserted here; the
                         two-entry tuple modes return the same tensors: asserted here)
    <G>_<head>_<phase>   logits, the gradients d.<name> of the loss of oracle/gen_golden.py::case_proto_phase, the state dict
                         sd.<key> (features.* left out) and its key list state_keys

Conv features and bank are bf16-representable, as in the other fixtures; the upstream gradients are multiples of 2^-20 (they
compress).  The group-phase module starts from the prototype-phase module's state dict (finetune_wandb_group.py:74-83)."""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import gen_golden as GG  # noqa: E402

SEED = 20261020
SHAPES = {
    # id: B, S, Cs, P, K, H, W, groups
    "G1": (2, 3, 16, 24, 4, 5, 7, 3),
    "G2": (1, 4, 64, 228, 19, 9, 13, 3),
}
HEADS = ("sum", "mult", "concat")


def _coarse(t, scale=1e-3):
    return torch.round(t * scale * 2.0 ** 20) / 2.0 ** 20


def _net(cls, shape, head, **kw):
    B, S, Cs, P, K, H, W, G = shape
    return cls(features=GG._Backbone(Cs * S), img_size=64, prototype_shape=(P, Cs, 1, 1), proto_layer_rf_info=[], num_classes=K,
               init_weights=True, add_on_layers_type="deeplab_simple", patch_classification=True, num_scales=S,
               scale_head_type=head, **kw)


def _record(net, conv, g, head_params):
    with torch.no_grad():
        o_default = net.forward_from_conv_features(conv)
        o_act = net.forward_from_conv_features(conv, return_activations=True)
    x = conv.clone().requires_grad_(True)
    logits, dist, act = net.forward_from_conv_features(x, return_activations=True, return_distances=True)
    assert len(o_default) == 2 and len(o_act) == 2
    assert torch.equal(o_default[0], logits) and torch.equal(o_default[1], dist)
    assert torch.equal(o_act[0], logits) and torch.equal(o_act[1], act)
    loss = (logits * g["g_logits"]).sum() + (dist * g["g_dist"]).sum() + (act * g["g_act"]).sum()
    net.zero_grad()
    loss.backward()
    out = {"logits": GG._np(logits), "d.conv": GG._np(x.grad)}
    for name, p in head_params(net):
        out["d." + name] = GG._np(p.grad)
    sd = {k: v for k, v in net.state_dict().items() if not k.startswith("features.")}
    out["state_keys"] = np.array(list(sd))
    for k, v in sd.items():
        out["sd." + k] = GG._np(v)
    return out, dist.detach(), act.detach()


def _proto_params(net):
    yield "prototype_vectors", net.prototype_vectors
    yield "last_layer.weight", net.last_layer.weight
    for k, p in net.scale_head.named_parameters():
        yield "scale_head." + k, p


def _group_params(net):
    yield "prototype_vectors", net.prototype_vectors
    yield "last_layer_group.weight", net.last_layer_group.weight
    for i, gp in enumerate(net.group_projection):
        yield f"group_projection.{i}.weight", gp.weight
    for k, p in net.scale_head.named_parameters():
        yield "scale_head." + k, p


def cases_of(ms, msg, gid):
    shape = SHAPES[gid]
    B, S, Cs, P, K, H, W, G = shape
    torch.manual_seed(SEED + ord(gid[1]))
    conv = GG._bf16r(torch.sigmoid(torch.randn(B, S * Cs, H, W)))
    g = dict(g_logits=_coarse(torch.randn(B, H, W, K)), g_dist=_coarse(torch.randn(B, P, H, W)), g_act=_coarse(torch.randn(B * H * W, P)))
    shared = {f"{gid}__conv": GG._np(conv), f"{gid}__shape": np.array(shape, dtype=np.int64)}
    shared.update({f"{gid}__{k}": GG._np(v) for k, v in g.items()})
    per_head = {}
    for head in HEADS:
        torch.manual_seed(SEED + 7 * HEADS.index(head) + ord(gid[1]))
        net = _net(ms.PPNetMultiScale, shape, head)
        with torch.no_grad():
            net.prototype_vectors.copy_(GG._bf16r(net.prototype_vectors))
            net.last_layer.weight.add_(0.05 * torch.randn_like(net.last_layer.weight))
        grp = _net(msg.PPNetMultiScale, shape, head, num_groups=G)
        grp.load_state_dict(net.state_dict(), strict=False)
        with torch.no_grad():
            grp.last_layer_group.weight.add_(0.05 * torch.randn_like(grp.last_layer_group.weight))
        shared[f"{gid}__scale_ranges"] = np.array([net.scale_num_prototypes[s] for s in range(S)], dtype=np.int64)
        out = {}
        rec_p, dist, act = _record(net, conv, g, _proto_params)
        rec_g, dist_g, act_g = _record(grp, conv, g, _group_params)
        assert torch.equal(dist, dist_g) and torch.equal(act, act_g)
        out[f"{gid}_{head}__distances"] = GG._np(dist)
        out[f"{gid}_{head}__activations"] = GG._np(act)
        out.update({f"{gid}_{head}_proto__{k}": v for k, v in rec_p.items()})
        out.update({f"{gid}_{head}_group__{k}": v for k, v in rec_g.items()})
        per_head[head] = out
    return shared, per_head


def main():
    GG._install_stubs()
    ref = os.environ.get("SPX_REFERENCE")
    if not ref:
        sys.exit("set SPX_REFERENCE to the reference checkout")
    sys.path.insert(0, ref)
    import segmentation.model.model_multiscale as ms
    import segmentation.model.model_multiscale_group as msg

    torch.set_num_threads(1)
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "..", "tests", "golden")
    shared, per_head = cases_of(ms, msg, "G1")
    for out in per_head.values():
        shared.update(out)
    files = {"scale_head.npz": shared}
    shared2, per_head2 = cases_of(ms, msg, "G2")
    for head, out in per_head2.items():
        files[f"scale_head_g2_{head}.npz"] = dict(shared2, **out)
    for name, blob in files.items():
        path = os.path.join(out_dir, name)
        np.savez_compressed(path, **blob)
        print(name, os.path.getsize(path))
        assert os.path.getsize(path) < 1 << 20, name


if __name__ == "__main__":
    main()
