"""The in-place simplex projection on the GPU (csrc/spx_simplex.hip, utils.projection_simplex_sort_): bit-exact against the
stock formula on a CPU copy of the input, in place (storage kept, version bumped, nothing written outside the rows), chunked
past 192 tensors, capturable, seen by the module's caches, and selectable in DataParallelStep."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from simplex_restatement import case_rows
from support import bits_equal, gpu_device, group_net, run_gloo

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 12, 63, 64, 65, 257, 1024)
_REF = {}


def _formula(v: torch.Tensor, z: float = 1.0) -> torch.Tensor:
    from scaleprotoseg_amd.utils import projection_simplex_sort

    return projection_simplex_sort(v.detach().cpu(), z)


def _ragged_inputs():
    """24 CPU matrices: G in {1, 3, 5} at every n of SIZES, together every row kind of case_rows at every n."""
    if "in" not in _REF:
        ws = []
        for n in SIZES:
            rows = torch.from_numpy(case_rows(n, 100 + n))
            ws += [rows[0:1].clone(), rows[1:4].clone(), rows[4:9].clone()]
        _REF["in"] = ws
    return _REF["in"]


def _ragged_reference(z):
    if z not in _REF:
        _REF[z] = [_formula(w, z) for w in _ragged_inputs()]
    return _REF[z]


def _theta64(row: np.ndarray, z: float) -> float:
    """theta of the projection in float64 (the exact formula, for the size of its rounding error only)."""
    u = np.sort(row.astype(np.float64))[::-1]
    css = np.cumsum(u) - z
    k = np.arange(1, len(u) + 1)
    rho = k[u - css / k > 0].max()
    return float(css[rho - 1] / rho)


@pytest.mark.parametrize("z", [1.0, 0.5])
def test_one_launch_over_a_ragged_list_is_bit_exact(z):
    """Row sums: w_i = fl(v_i - theta) on the support, each within 2^-24 relative, so sum w = sum_support v - |support| theta up
    to 2^-24 |z|; theta = fl(fl(fl(S) - z) / rho) carries three fp32 roundings (the sum's, the subtraction's, the division's) on
    magnitudes <= |theta| + |z| / rho, |theta|, |theta|: |d theta| <= 2^-24 (3 |theta| + |z| / rho), and it enters the sum at
    most n times.  Total <= n 2^-23 max(1, |z|) (which covers n 2^-24 |z| + 2^-24 |z|) + n 2^-23 1.5 |theta|."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    ws = [w.to(dev) for w in _ragged_inputs()]
    assert sorted({w.shape[0] for w in ws}) == [1, 3, 5] and sorted({w.shape[1] for w in ws}) == list(SIZES)
    spx.projection_simplex_sort_(ws, z)
    for w, v, ref in zip(ws, _ragged_inputs(), _ragged_reference(z)):
        got = w.cpu()
        assert bits_equal(got, ref), f"[{v.shape[0]}, {v.shape[1]}] z={z}: {(got - ref).abs().max().item()}"
        assert (got >= 0).all()
        n = v.shape[1]
        for g in range(v.shape[0]):
            tol = n * 2.0 ** -23 * max(1.0, abs(z)) + n * 2.0 ** -23 * 1.5 * abs(_theta64(v[g].numpy(), z))
            s = float(got[g].double().sum())
            assert abs(s - z) <= tol, f"[{v.shape[0]}, {n}] row {g}: sum {s} (z={z}, tol {tol})"


def test_193_tensors_are_chunked():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    g = torch.Generator().manual_seed(193)
    cpu = [torch.randn(3, 12, generator=g) * (0.1 + 0.05 * i) for i in range(193)]
    ws = [w.to(dev) for w in cpu]
    spx.projection_simplex_sort_(ws)
    ref = _formula(torch.cat(cpu, dim=0)).reshape(193, 3, 12)             # (the formula is row-wise)
    for i in (0, 191, 192):
        assert bits_equal(ws[i], ref[i]), i
    assert bits_equal(torch.stack([w.cpu() for w in ws]), ref)


def test_the_edit_is_in_place():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    g = torch.Generator().manual_seed(7)
    before = torch.full((64,), 5.0, device=dev)
    ws = [nn.Parameter(torch.randn(G, n, generator=g).to(dev)) for G, n in ((3, 12), (1, 65), (5, 7), (3, 12))]
    canary = torch.full((64,), 7.0, device=dev)                             # allocated directly after the last weight
    ptrs, versions = [w.data_ptr() for w in ws], [w._version for w in ws]
    cpu = [w.detach().cpu() for w in ws]
    spx.projection_simplex_sort_(ws)
    torch.cuda.synchronize()
    assert [w.data_ptr() for w in ws] == ptrs
    assert all(w._version > v for w, v in zip(ws, versions))
    assert all(w.grad_fn is None and w.requires_grad and w.is_leaf for w in ws)       # no autograd node on the parameters
    assert (canary == 7.0).all() and (before == 5.0).all()
    for w, v in zip(ws, cpu):
        assert bits_equal(w, _formula(v))
    with pytest.raises(spx.SpxError, match="listed twice"):
        spx.projection_simplex_sort_([ws[0], ws[1], ws[0]])
    with pytest.raises(spx.SpxError, match="fp32"):
        spx.projection_simplex_sort_([ws[0].detach().double()])


def test_rows_longer_than_the_kernel_takes_fall_back_in_place():
    """n > 1024 in any tensor: the whole call is the stock formula on the device, copied back into the same storages."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    g = torch.Generator().manual_seed(1025)
    ws = [nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in ((2, 1025), (3, 12))]
    want = [spx.projection_simplex_sort(w.detach().clone()) for w in ws]
    cpu = [_formula(w) for w in ws]
    ptrs, versions = [w.data_ptr() for w in ws], [w._version for w in ws]
    spx.projection_simplex_sort_(ws)
    assert [w.data_ptr() for w in ws] == ptrs and all(w._version > v for w, v in zip(ws, versions))
    for w, ref, c in zip(ws, want, cpu):
        assert torch.equal(w.detach(), ref)
        # against the CPU: the device's fp32 prefix sums round differently; theta is a mean of a few values of magnitude <= 5
        assert (w.detach().cpu() - c).abs().max().item() <= 1e-5


def test_a_nan_row_comes_back_nan_and_its_neighbours_exact():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    g = torch.Generator().manual_seed(11)
    a, b = torch.randn(3, 12, generator=g), torch.randn(2, 70, generator=g)
    a[1, 5] = float("nan")
    b[0, 69] = float("nan")
    wa, wb, wc = a.to(dev), b.to(dev), torch.randn(3, 12, generator=g).to(dev)
    c = wc.cpu()
    spx.projection_simplex_sort_([wa, wb, wc])
    assert torch.isnan(wa[1]).all() and torch.isnan(wb[0]).all()
    assert torch.isnan(_formula(a)[1]).all()                                # ... as the formula has it
    assert bits_equal(wa[[0, 2]], _formula(a[[0, 2]])) and bits_equal(wb[1:], _formula(b[1:])) and bits_equal(wc, _formula(c))


def _group_net(dev, seed=1):
    return group_net(40, 5, 4, 16, 3, seed=seed, add_on=nn.Sequential(), device=dev)


def _consumers(net, x):
    logits, _, act = net.forward_from_conv_features(x, return_activations=True, return_distances=True)
    tagged = torch.cat(net.compute_group(act), dim=-1)                      # the forward's own group activations
    foreign = torch.cat(net.compute_group(act.detach().clone()), dim=-1)    # the dense matrix + the product kernels
    return logits.detach().clone(), tagged.detach().clone(), foreign.detach().clone()


def test_the_module_caches_see_the_projection():
    dev = gpu_device()
    net = _group_net(dev)
    x = torch.sigmoid(torch.randn(2, 64, 9, 11, generator=torch.Generator().manual_seed(3))).to(dev)
    first = _consumers(net, x)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for gp in net.group_projection:
            gp.weight.add_((0.3 * torch.randn(gp.weight.shape, generator=g)).to(dev))
    noisy = _consumers(net, x)                                              # whatever this leaves cached is stale next
    ptrs = [gp.weight.data_ptr() for gp in net.group_projection]
    net.project_group_simplex_()
    assert [gp.weight.data_ptr() for gp in net.group_projection] == ptrs
    for gp in net.group_projection:
        w = gp.weight.detach()
        assert (w >= 0).all() and torch.allclose(w.sum(1), torch.ones(w.shape[0], device=dev), atol=1e-5)
    second = _consumers(net, x)

    fresh = _group_net(dev, seed=2)                                         # same shapes, other initial values
    with torch.no_grad():
        fresh.prototype_vectors.copy_(net.prototype_vectors)
        fresh.last_layer_group.weight.copy_(net.last_layer_group.weight)
        for a, b in zip(fresh.group_projection, net.group_projection):
            a.weight.copy_(b.weight)
    want = _consumers(fresh, x)
    for got, ref, old, mid, what in zip(second, want, first, noisy, ("logits", "group activations", "group activations (dense)")):
        assert torch.equal(got, ref), what
        assert not torch.equal(got, old) and not torch.equal(got, mid), what


def test_the_projection_is_capturable():
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import graphs

    dev = gpu_device()
    g = torch.Generator().manual_seed(21)
    shapes = ((3, 12), (3, 5), (2, 65))
    cpu = [spx.projection_simplex_sort(torch.rand(s, generator=g)) for s in shapes]
    deltas_cpu = [0.05 * torch.randn(s, generator=g) for s in shapes]
    ws, deltas = [w.to(dev) for w in cpu], [d.to(dev) for d in deltas_cpu]
    ptrs = [w.data_ptr() for w in ws]

    def step():
        for w, d in zip(ws, deltas):
            w.add_(d)
        spx.projection_simplex_sort_(ws)

    warmup, replays = 3, 4
    graph, _ = graphs.capture_step(step, warmup=warmup)
    for _ in range(replays):
        graph.replay()
    torch.cuda.synchronize()
    for _ in range(warmup + replays):                                       # (the capture itself runs nothing)
        cpu = [_formula(w + d) for w, d in zip(cpu, deltas_cpu)]
    assert [w.data_ptr() for w in ws] == ptrs
    for w, ref in zip(ws, cpu):
        assert bits_equal(w, ref)


# (what one rank runs in this file's data-parallel test; support.run_gloo spawns it)
def _dp_case(rank, world):
    """Two identical group modules through identical steps: the default re-projection (formula per class, rebound) and the fused
    one.  Plain SGD: the update is linear in the gradient, so the two paths stay a rounding error apart."""
    from scaleprotoseg_amd.dp import DataParallelStep

    dev = torch.device("cuda:0")
    K = 5
    out = {}
    for name, fused in (("default", False), ("fused", True)):
        net = _group_net(dev, seed=21)
        params = [net.prototype_vectors] + [gp.weight for gp in net.group_projection] + [net.last_layer_group.weight]
        stepper = DataParallelStep(net, torch.optim.SGD(params, lr=0.5), iter_size=1, fused_projection=fused)
        g = torch.Generator().manual_seed(100)
        ptrs = [[gp.weight.data_ptr() for gp in net.group_projection]]
        for _ in range(3):
            conv = torch.sigmoid(torch.randn(2, 64, 9, 11, generator=g)).to(dev)
            tgt = torch.randint(0, K, (2 * 9 * 11,), generator=g).to(dev)
            logits, dist_map = net.forward_from_conv_features(conv)
            loss = torch.nn.functional.cross_entropy(logits.reshape(-1, K), tgt) + 1e-3 * dist_map.mean()
            assert stepper.backward(loss)
            ptrs.append([gp.weight.data_ptr() for gp in net.group_projection])
        out[name] = ([gp.weight.detach().cpu() for gp in net.group_projection], ptrs)
    out["initial"] = [gp.weight.detach().cpu() for gp in _group_net(dev, seed=21).group_projection]
    return out


def test_data_parallel_step_with_the_fused_projection(tmp_path):
    gpu_device()
    (res,) = run_gloo(_dp_case, tmp_path, world=1, gpu=True)
    (wd, pd), (wf, pf) = res["default"], res["fused"]
    for a, b, w0 in zip(wd, wf, res["initial"]):
        assert (a - b).abs().max().item() <= 1e-6
        assert (b >= 0).all() and torch.allclose(b.sum(1), torch.ones(b.shape[0]), atol=1e-5)
        assert (b - w0).abs().max().item() > 1e-4                           # the steps moved the weights
    assert all(step == pf[0] for step in pf[1:])                            # fused: no storage moved
    for prev, cur in zip(pd[:-1], pd[1:]):                                  # default: every step rebinds every projection
        assert all(p != c for p, c in zip(prev, cur))
