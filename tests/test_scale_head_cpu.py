"""CPU checks of the scale head (no device):

* tests/scale_head_restatement.py reproduces what the reference's REAL classes recorded (tests/golden/scale_head*.npz,
  tools/gen_scale_head_golden.py): distances within 1e-4 (1 + d), activations within 2e-4 (1 + |a|), logits within assert_fwd's
  bound, gradients by grad_close (GRAD_TOL) - both phases, three head types, shapes G1 and G2;
* with the distance kernels' bf16 rounding of every distance input, the worst |d - fixture| / (1e-4 (1 + d)) per scale is
  printed and written to profiles/scale_head_summary.md.  That number is information, not a bound: a chained scale's input x'
  is off the bf16 grid, so the kernels answer at bf16(x') and differ from the unrounded reference by the same order as the
  "oracle at (x,p) vs (x~,p~)" column of profiles/offgrid_summary.md.  It is why tests/test_gpu_scale_head.py holds the kernels
  to the restatement link by link and only the LAST scale (whose input is the bf16-representable fixture feature) to the fixture;
* the module surface: constructors, state-dict keys, the unknown type, the checkpoint helpers."""
import os

import numpy as np
import pytest
import torch

import offgrid_restatement as R
import scale_head_restatement as SH
from support import GRAD_TOL, HERE, ROOT, grad_close, group_net, proto_net

GOLDEN = os.path.join(HERE, "golden")
CASES = [(g, h, p) for g in ("G1", "G2") for h in SH.HEADS for p in SH.PHASES]
SUMMARY = os.path.join(ROOT, "profiles", "scale_head_summary.md")
BEGIN, END = "<!-- rounding-hook:begin -->", "<!-- rounding-hook:end -->"


def _leaves(fx):
    conv = fx["conv"].double().requires_grad_(True)
    bank = fx["sd.prototype_vectors"].double().requires_grad_(True)
    lin = None if fx["linear"] is None else tuple(t.double().requires_grad_(True) for t in fx["linear"])
    return conv, bank, lin


@pytest.mark.parametrize("gid,head,phase", CASES)
def test_restatement_matches_the_reference(gid, head, phase):
    fx = SH.fixture(gid, head, phase, GOLDEN)
    d = fx["dims"]
    conv, bank, lin = _leaves(fx)
    params = SH.head_params(fx, phase)
    dist, _ = SH.chain(conv, bank, fx["ranges"], d.S, head, linear=lin)
    loss, logits, act = SH.head_loss(fx, phase, dist, params)
    ref_d, ref_a, ref_l = fx["distances"].double(), fx["activations"].double(), fx["logits"].double()
    assert dist.shape == ref_d.shape and act.shape == ref_a.shape and logits.shape == ref_l.shape
    assert ((dist - ref_d).abs() <= 1e-4 * (1 + ref_d)).all(), f"distance err {(dist - ref_d).abs().max().item()}"
    assert ((act - ref_a).abs() <= 2e-4 * (1 + ref_a.abs())).all(), f"activation err {(act - ref_a).abs().max().item()}"
    assert (logits - ref_l).abs().max().item() <= 1e-4 * max(1.0, ref_l.abs().max().item())
    loss.backward()
    grad_close(conv.grad, fx["d.conv"], "d conv")
    grad_close(bank.grad, fx["d.prototype_vectors"], "d prototype_vectors")
    for k, p in params.items():
        if k != "ident":
            grad_close(p.grad, fx["d." + k], "d " + k)
    if lin is not None:
        grad_close(lin[0].grad, fx["d.scale_head.output_layer.linear_block.0.weight"], "d concat weight")
        grad_close(lin[1].grad, fx["d.scale_head.output_layer.linear_block.0.bias"], "d concat bias")


def test_chain_gradients_equal_autograd_without_rounding():
    """The composed gradient (site formula + autograd of the aggregation link) IS the chain's gradient when nothing is rounded."""
    for head in SH.HEADS:
        fx = SH.fixture("G1", head, "proto", GOLDEN)
        d = fx["dims"]
        conv, bank, lin = _leaves(fx)
        params = SH.head_params(fx, "proto")
        dist, _ = SH.chain(conv, bank, fx["ranges"], d.S, head, linear=lin)
        SH.head_loss(fx, "proto", dist, params)[0].backward()
        got = SH.chain_gradients(fx["conv"], fx["sd.prototype_vectors"], fx["ranges"], d.S, head,
                                 lambda dd: SH.head_loss(fx, "proto", dd, SH.head_params(fx, "proto"))[0], linear=fx["linear"],
                                 rounding=None)
        # (the sites c / b hold fp16_rtz(bf16(x')) / bf16(p): with x' off the grid they differ from x' by up to 2^-8 relative,
        # which reaches the bank gradient at that order - the kernels' own, held by test_gpu_scale_head.py)
        grad_close(got.conv, conv.grad, f"{head}: d conv", tol=2.0 ** -7)
        grad_close(got.bank, bank.grad, f"{head}: d bank", tol=2.0 ** -7)
        if lin is not None:
            grad_close(got.linear[0], lin[0].grad, "d concat weight", tol=2.0 ** -7)


def _write_summary(lines):
    try:
        text = open(SUMMARY).read() if os.path.exists(SUMMARY) else ""
    except OSError:
        return
    block = BEGIN + "\n" + "\n".join(lines) + "\n" + END
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN)] + block + text[text.index(END) + len(END):]
    else:
        text = text + ("\n" if text and not text.endswith("\n") else "") + block + "\n"
    try:
        with open(SUMMARY, "w") as f:
            f.write(text)
    except OSError:
        pass


def test_rounding_hook_ratio_per_scale():
    """Information, not a bound (module docstring): the chained scales sit tens of tolerances from the unrounded fixture, the
    last scale (bf16-representable input) at ~0."""
    lines = ["| case | " + " | ".join(f"scale {s}" for s in range(4)) + " |", "|---|---|---|---|---|"]
    for gid in ("G1", "G2"):
        for head in SH.HEADS:
            fx = SH.fixture(gid, head, "proto", GOLDEN)
            d = fx["dims"]
            dist, _ = SH.chain(fx["conv"], fx["sd.prototype_vectors"], fx["ranges"], d.S, head, linear=fx["linear"], rounding=R.bf16_rne)
            ratios = []
            for s in range(d.S):
                lo, hi = fx["ranges"][s]
                ratios.append(R.distance_ratio(dist[:, lo:hi], fx["distances"][:, lo:hi]))
            print(f"rounding hook {gid} {head}: worst |d - fixture| / (1e-4 (1 + d)) per scale " + " ".join(f"{r:.2f}" for r in ratios))
            lines.append(f"| {gid} {head} | " + " | ".join([f"{r:.2f}" for r in ratios] + ["-"] * (4 - d.S)) + " |")
            assert ratios[-1] <= 1.0, "the last scale's inputs are on the bf16 grid: it must meet the fixture"
            assert all(np.isfinite(r) for r in ratios)
    _write_summary(lines)


# ---- module surface -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", SH.PHASES)
@pytest.mark.parametrize("head", SH.HEADS)
def test_constructor_builds_the_head_with_the_reference_keys(head, phase):
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import scale_head as M

    fx = SH.fixture("G1", head, phase, GOLDEN)
    d = fx["dims"]
    net = (proto_net(d.P, d.K, d.S, d.Cs, scale_head_type=head) if phase == "proto"
           else group_net(d.P, d.K, d.S, d.Cs, d.G, scale_head_type=head))
    assert isinstance(net.scale_head, spx.WeightedAgg)
    assert type(net.scale_head.output_layer) is {"sum": M.OutSum, "mult": M.OutMult, "concat": M.OutConcat}[head]
    sd = net.state_dict()
    keys = [k for k in sd if not k.startswith("features.")]
    assert keys == fx["state_keys"]
    for k in keys:
        assert tuple(sd[k].shape) == tuple(fx["sd." + k].shape), k
    has = [k for k in keys if k.startswith("scale_head.")]
    assert has == (["scale_head.output_layer.linear_block.0.weight", "scale_head.output_layer.linear_block.0.bias"] if head == "concat" else [])


def test_unknown_type_raises_not_implemented():
    import scaleprotoseg_amd as spx

    with pytest.raises(NotImplementedError, match="Unknown output type"):
        proto_net(24, 4, 3, 16, scale_head_type="max")
    with pytest.raises(NotImplementedError):
        group_net(24, 4, 3, 16, 3, scale_head_type="max")
    with pytest.raises(NotImplementedError):
        spx.factory_output_layer("avg", channel_dim=16)
    assert isinstance(spx.factory_output_layer("concat", channel_dim=16).linear_block[0], torch.nn.Linear)


def test_no_head_is_unchanged(golden):
    net = proto_net(40, 5, 4, 16)
    assert net.scale_head is None
    keys = [k for k in net.state_dict() if not k.startswith("features.")]
    assert keys == [str(k) for k in golden("proto_ms_small")["state_keys"]]
    grp = group_net(40, 5, 4, 16, 3)
    assert grp.scale_head is None
    assert [k for k in grp.state_dict() if not k.startswith("features.")] == [str(k) for k in golden("group_ms_small")["state_keys"]]


@pytest.mark.parametrize("phase", SH.PHASES)
def test_checkpoint_helpers_carry_the_head(phase):
    import scaleprotoseg_amd as spx

    fx = SH.fixture("G1", "concat", phase, GOLDEN)
    d = fx["dims"]
    build = (lambda **kw: proto_net(d.P, d.K, d.S, d.Cs, **kw)) if phase == "proto" else (lambda **kw: group_net(d.P, d.K, d.S, d.Cs, d.G, **kw))
    sd = {k: fx["sd." + k] for k in fx["state_keys"]}
    net = build(scale_head_type="concat")
    res = spx.load_reference_state_dict(net, sd)
    assert not res.unexpected_keys and all(k.startswith("features.") for k in res.missing_keys)
    lin = net.scale_head.output_layer.linear_block[0]
    assert torch.equal(lin.weight.detach(), fx["linear"][0]) and torch.equal(lin.bias.detach(), fx["linear"][1])
    blob = spx.export_state(net)
    assert "scale_head.output_layer.linear_block.0.weight" in blob["state_dict"]
    other = build(scale_head_type="concat")
    spx.import_state(other, blob)
    lin2 = other.scale_head.output_layer.linear_block[0]
    assert torch.equal(lin2.weight.detach(), fx["linear"][0]) and torch.equal(lin2.bias.detach(), fx["linear"][1])
    # a head the checkpoint does not match is refused, not dropped in silence under strict=False
    for wrong in (None, "sum"):
        with pytest.raises(ValueError, match="scale_head"):
            spx.load_reference_state_dict(build(scale_head_type=wrong), sd)
        with pytest.raises(ValueError, match="scale_head"):
            spx.import_state(build(scale_head_type=wrong), blob)
    with pytest.raises(ValueError, match="scale_head"):
        spx.load_reference_state_dict(build(scale_head_type="concat"), {k: v for k, v in sd.items() if not k.startswith("scale_head.")})


def test_host_checks_come_before_any_launch():
    import scaleprotoseg_amd as spx

    x, src, p = torch.rand(1, 16, 3, 3), torch.rand(1, 5, 3, 3), torch.rand(5, 16)
    with pytest.raises(spx.SpxError, match="unknown mode"):
        spx.scale_aggregate(x, src, p, mode="max")
    with pytest.raises(spx.SpxError, match="source_kind"):
        spx.scale_aggregate(x, src, p, mode="sum", source_kind="logits")
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.scale_aggregate(x, src, p, mode="sum")
    net = proto_net(24, 4, 3, 16, scale_head_type="sum")
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        net._scale_l2_convolution(torch.rand(1, 48, 3, 3))
