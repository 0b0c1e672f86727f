"""Scaffolding the test files share: the device gate, the backbone stand-in, net builders, the two-rank gloo runner, the
allocator fixture and a few small checkers.  Test files import this module and the ``*_cases.py`` / ``*_restatement.py``
modules beside it, never each other.  Nothing here touches a device at import time."""
import functools
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# tolerances several suites share (stated in tests/test_gpu_parity.py's docstring)
GRAD_TOL = 1e-3        # gradients rel 1e-3 (max-normalised)
BF16_DX_TOL = 4e-3     # dX returned in bf16 (bf16 features): ONE output rounding is half a bf16 ulp = 2^-8 of the element
EPS = 1e-4             # the log activation's epsilon, as the reference's scripts use it


def gpu_device(required=False):
    """cuda:0; without a GPU the calling test is skipped, or fails if ``required`` (tests/test_gpu_regularizers.py)."""
    if not torch.cuda.is_available():
        (pytest.fail if required else pytest.skip)("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def release_cached_blocks():
    """Hand the blocks a module's tests cached back to the device, so the modules that follow see the caching allocator in a
    state that does not depend on these tests.  A module takes it by importing the name."""
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ---- stand-ins -----------------------------------------------------------------------------------------------------------
class RoundBf16(nn.Module):
    """Makes the add-on output bf16-representable (SURVEY.md 8d 'identical inputs')."""

    def forward(self, x):
        return x.to(torch.bfloat16).to(torch.float32)


class Backbone(nn.Module):
    """Stand-in for the DeepLab backbone (out of scope): ``str()`` starts with MSC and ``.base`` holds two Conv2d, which
    is all model_multiscale.py:153-171 asks of it.  ``mode``: identity (the "images" ARE the features, so an image's features
    do not depend on its batch mates), pool (image -> features for the push tests) or list (MSC training output: a list of
    feature maps).  Every mode draws the same two convolutions from the global generator."""

    def __init__(self, ch, mode="identity", stride=4):
        super().__init__()
        self.base = nn.Sequential(nn.Conv2d(3, ch, 1), nn.Conv2d(ch, ch, 1))
        self.pool = nn.AvgPool2d(stride)
        self.mode = mode

    def __repr__(self):
        return "MSC(standin)"

    def forward(self, x):
        if self.mode == "identity":
            return x
        if self.mode == "list":
            return [x, x[..., ::2, ::2].contiguous()]
        return self.base(self.pool(x))


class ListData(list):
    """A data set for the push and the pruning search: a list of (image, target) items."""

    convert_targets = None

    @property
    def items(self):                # the name the hand-written data sets of other suites keep their list under
        return self


def _build(cls, P, K, S, Cs, single, seed, add_on, init, device, backbone, stride, kw):
    if seed is not None:
        torch.manual_seed(seed)
    if not single:
        kw = dict(num_scales=S, **kw)
    net = cls(Backbone(Cs if single else S * Cs, backbone, stride), 64, (P, Cs, 1, 1), [], K, add_on_layers_type="deeplab_simple",
              patch_classification=True, **kw)
    if add_on is not None:
        net.add_on_layers = add_on
    if init is not None:
        with torch.no_grad():
            init(net)
    return net if device is None else net.to(device)


def proto_net(P, K, S, Cs, *, cls=None, seed=None, add_on=None, init=None, device=None, backbone="identity", stride=4, **kw):
    """A prototype-phase module (``cls``: PPNetMultiScale, or the single-scale PPNet, which takes no ``S``) on the stand-in
    backbone.  In this order: ``seed`` seeds the global generator, the backbone and the module are built, ``add_on`` replaces
    add_on_layers, ``init(net)`` runs under no_grad, the module moves to ``device``; what is None is left out."""
    import scaleprotoseg_amd as spx

    cls = cls or spx.PPNetMultiScale
    return _build(cls, P, K, S, Cs, cls is spx.PPNet, seed, add_on, init, device, backbone, stride, kw)


def group_net(P, K, S, Cs, G, *, seed=None, add_on=None, init=None, device=None, **kw):
    """A group-phase module; the arguments and their order of effect are ``proto_net``'s.  ``init`` is where a caller sets
    the group projections (fixture weights, a simplex projection of random rows, ...)."""
    import scaleprotoseg_amd as spx

    return _build(spx.PPNetMultiScaleGroup, P, K, S, Cs, False, seed, add_on, init, device, "identity", 4, dict(num_groups=G, **kw))


# ---- two ranks over gloo -------------------------------------------------------------------------------------------------
def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def gloo_worker(rank, world, port, fn, out, gpu):
    import torch.distributed as dist

    sys.path.insert(0, ROOT)
    if gpu:                                                     # both ranks share cuda:0
        sys.path.insert(0, HERE)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(0)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = fn(rank, world)
        torch.save(res, os.path.join(out, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def run_gloo(fn, tmp_path, world=2, gpu=False):
    """``fn(rank, world)`` (a module-level function) in ``world`` spawned processes joined by gloo: the list of its results."""
    import torch.multiprocessing as mp

    mp.spawn(gloo_worker, args=(world, free_port(), fn, str(tmp_path), gpu), nprocs=world, join=True)
    return [torch.load(os.path.join(tmp_path, f"r{r}.pt")) for r in range(world)]


# ---- small checkers ------------------------------------------------------------------------------------------------------
def bits_equal(a, b):
    """Same dtype, shape and bits of two float32 tensors on any device."""
    return (a.dtype == b.dtype and a.shape == b.shape
            and torch.equal(a.detach().cpu().contiguous().view(torch.int32), b.detach().cpu().contiguous().view(torch.int32)))


def grad_close(got, ref, what, tol=GRAD_TOL, report=None):
    """max|got - ref| <= tol * max|ref| on tensors of one shape; ``report`` prints the measured ratio under that label."""
    got, ref = got.detach().float().cpu(), torch.as_tensor(ref).detach().float().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    if report:
        print(f"{report} {what}: against the oracle {err / scale:.3e} of the maximum (bound {tol:.0e})")
    assert err <= tol * scale, f"{what}: err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.2e})"


class Guarded:
    """A device buffer with guard bands on both sides: kernels get a pointer into the middle, the bands must stay intact."""
    GUARD = 64 * 1024          # bytes each side

    def __init__(self, nbytes, dev):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * self.GUARD,), 0xA5, dtype=torch.uint8, device=dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.GUARD

    def body(self, dtype):
        return self.buf[self.GUARD:self.GUARD + self.n].view(dtype)

    def intact(self):
        g = self.GUARD
        return bool((self.buf[:g] == 0xA5).all()) and bool((self.buf[g + self.n:] == 0xA5).all())


# ---- reference-recorded map fixtures (tests/golden/*.npz with "case__field" keys) ------------------------------------------
@functools.lru_cache(maxsize=None)
def load_cases(fixture):
    z = np.load(os.path.join(HERE, "golden", fixture + ".npz"))
    cases = {}
    for key in z.files:
        name, field = key.split("__")
        cases.setdefault(name, {})[field] = z[key]
    return cases


def planes_of(case):
    """The float32 activation planes [N, C, h, w] the reference upsampled, by the case's ``kind``: the log activation of its
    distances (sample_activations_prototype.py:85, prototype_overlap.py:60, push_multiscale_optimization.py:447 on float32),
    the linear one (:449 with max_dist = 4), or the recorded activations."""
    kind = str(case["kind"])
    if kind in ("proto", "log"):
        d = case["distances"]
        return np.log((d + 1) / (d + EPS))
    if kind == "linear":
        return np.float32(4.0) - case["distances"]
    return case["activations"]
