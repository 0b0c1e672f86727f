"""GPU training-batch preparation (scaleprotoseg_amd/batch.py, csrc/spx_batch.hip) against tests/batch_restatement.py and what
tools/gen_batch_golden.py recorded from the reference's own data set class (tests/golden/batch_prepare.npz).

Labels, latent labels, the shifted int32 form and the uint8 image are compared bit for bit.  The fp32 image is held to
``batch_restatement.image_bound`` of the float64 normalisation of the same byte: 2^-23 (1 + |mean_c|) / std_c + 2^-23 |ref|, the
three fp32 roundings of r / 255, - mean and / std - derived, not measured (fp32 division is correctly rounded in this build).
Shapes: a 33 x 41 window (1353 pixels: five full workgroups of 256 and a ragged sixth, every row boundary inside a workgroup) over
three sources of different sizes, and a 3 x 300 window whose rows cross the workgroup edges at pixels 256, 512 and 768."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import batch_restatement as BR  # noqa: E402
from support import gpu_device  # noqa: E402
from support import release_cached_blocks  # noqa: E402,F401  (a module-scoped autouse fixture, taken by importing its name)

pytestmark = pytest.mark.gpu

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
WINDOW = (33, 41)
GRIDS = [(5, 6), (9, 11), (33, 41)]
ID_MAP = np.array([3, 0, 5, 1, 4, 2, 0, 6, 1, 2], np.int64)           # raw 0..9; the samples hold 10 and 11 as well
DTYPES = {"u8": torch.uint8, "i16": torch.int16, "i32": torch.int32, "i64": torch.int64}
POISON_I, POISON_F = -7777, 0x7FC12345


def mixed_samples():
    """Three sources: (37, 53) scaled by 1.45 and cropped, (23, 31) scaled by 0.6 and padded in both directions, (40, 40) at scale 1.0
    read through a margin view; both flip values."""
    g = np.random.default_rng(20240301)
    out = []
    for (h, w), f, m, origin, flip in (((37, 53), 1.45, 0, (11, 30), True), ((23, 31), 0.6, 0, (0, 0), False),
                                       ((40, 40), 1.0, 3, (5, 0), True)):
        full = g.integers(0, 256, (h + 2 * m, w + 2 * m, 3)).astype(np.uint8)
        blocks = g.integers(0, 12, (h // 4 + 1, w // 5 + 1))
        label = np.kron(blocks, np.ones((4, 5), np.int64))[:h, :w]
        out.append(dict(full=full, margin=m, label=label, scaled=(int(h * f), int(w * f)), origin=origin, flip=flip))
    return out


def tile_sample():
    g = np.random.default_rng(5)
    return dict(full=g.integers(0, 256, (5, 310, 3)).astype(np.uint8), margin=0, label=g.integers(0, 12, (5, 310)),
                scaled=(5, 310), origin=(1, 7), flip=True)


def inner(s):
    m = s["margin"]
    return s["full"][m:s["full"].shape[0] - m, m:s["full"].shape[1] - m] if m else s["full"]


def restate(samples, window, grids, id_map, flips=None):
    """The restatement of a batch, computed once per module: labels, latent labels, bytes, fp32 and float64 images."""
    ref = dict(labels=[], latent=[[] for _ in grids], u8=[], f32=[], f64=[], raw32=[], raw64=[], inside=[])
    for n, s in enumerate(samples):
        flip = s["flip"] if flips is None else flips[n]
        lab = BR.window_label(s["label"], id_map, s["scaled"], s["origin"], flip, window)
        ref["labels"].append(lab)
        for k, lat in enumerate(BR.latent_labels(lab, grids)):
            ref["latent"][k].append(lat)
        a = (inner(s), s["scaled"], s["origin"], flip, window)
        ref["u8"].append(BR.window_image_u8(*a, MEAN))
        ref["f32"].append(BR.window_image_f32(*a, MEAN, STD))
        ref["f64"].append(BR.window_image_f64(*a, MEAN, STD))
        ref["raw32"].append(BR.window_image_f32(*a, MEAN, STD, normalize=False))
        ref["raw64"].append(BR.window_image_f64(*a, MEAN, STD, normalize=False))
        ref["inside"].append(BR.window_bytes(*a)[1])
    return {k: (np.stack(v) if k != "latent" else [np.stack(x) for x in v]) for k, v in ref.items()}


@pytest.fixture(scope="module")
def mixed():
    samples = mixed_samples()
    return samples, restate(samples, WINDOW, GRIDS, ID_MAP)


def upload(samples, dev, label_dtype):
    images, labels = [], []
    for s in samples:
        m = s["margin"]
        full = torch.from_numpy(s["full"]).to(dev)
        images.append(full[m:full.shape[0] - m, m:full.shape[1] - m] if m else full)         # a strided view, read in place
        labels.append(torch.from_numpy(s["label"]).to(label_dtype).to(dev))
    return images, labels


def params_of(samples, flips=None):
    import scaleprotoseg_amd as spx

    return [spx.AugmentParams(s["scaled"], s["origin"], s["flip"] if flips is None else flips[n]) for n, s in enumerate(samples)]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().cpu()


def check_labels(batch, ref):
    from scaleprotoseg_amd.functional import shifted_labels_i32

    assert batch.labels.dtype == torch.int64 and np.array_equal(batch.labels.cpu().numpy(), ref["labels"])
    for k, want in enumerate(ref["latent"]):
        got, got0 = batch.latent[k], batch.latent0[k]
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), k
        assert got0.dtype == torch.int32 and np.array_equal(got0.cpu().numpy(), BR.shifted_i32(want)), k
        assert torch.equal(got0, shifted_labels_i32(got, got.device)), k


def check_fp32(image, ref, normalize=True):
    got = image.cpu().numpy()
    assert got.dtype == np.float32
    ref64 = ref["f64" if normalize else "raw64"]
    err = np.abs(got.astype(np.float64) - ref64)
    bound = np.stack([BR.image_bound(r, MEAN, STD, normalize) for r in ref64])
    print("fp32 image: max error", err.max(), "max error / bound", (err / bound).max())
    assert (err <= bound).all()
    # the float32 restatement, operation by operation, is the kernel bit for bit
    assert np.array_equal(got.view(np.int32), ref["f32" if normalize else "raw32"].view(np.int32))
    pad = ~ref["inside"]
    assert pad.any() and (~pad).any()
    for c in range(3):
        want = np.float32(0.0) if normalize else np.float32(MEAN[c])
        assert (got[:, c][pad].view(np.int32) == want.view(np.int32)).all()         # exactly 0 (+0.0), or exactly mean_c


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_mixed_batch(mixed, dtype_name):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    samples, ref = mixed
    images, labels = upload(samples, dev, DTYPES[dtype_name])
    kw = dict(window=WINDOW, mean=MEAN, std=STD, grids=GRIDS, id_map=ID_MAP)
    batch = spx.prepare_batch(images, labels, params_of(samples), **kw)
    assert tuple(batch.image.shape) == (3, 3) + WINDOW
    check_labels(batch, ref)
    check_fp32(batch.image, ref)
    again = spx.prepare_batch(images, labels, params_of(samples), **kw)                 # repeatability
    for a, b in zip([batch.image, batch.labels, *batch.latent, *batch.latent0], [again.image, again.labels, *again.latent, *again.latent0]):
        assert torch.equal(bits(a), bits(b))


def test_mixed_batch_other_outputs_and_flips(mixed):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    samples, ref = mixed
    images, labels = upload(samples, dev, torch.int32)
    kw = dict(window=WINDOW, mean=MEAN, std=STD, grids=GRIDS, id_map=ID_MAP)
    u8 = spx.prepare_batch(images, labels, params_of(samples), dtype=torch.uint8, **kw)
    assert u8.image.dtype == torch.uint8 and np.array_equal(u8.image.cpu().numpy(), ref["u8"])
    check_labels(u8, ref)
    raw = spx.prepare_batch(images, labels, params_of(samples), normalize=False, shifted=False, want_labels=False, **kw)
    assert raw.labels is None and raw.latent0 is None
    check_fp32(raw.image, ref, normalize=False)
    # every flip inverted: the other branch on every sample
    flips = [not s["flip"] for s in samples]
    ref2 = restate(samples, WINDOW, GRIDS[:1], ID_MAP, flips)
    inv = spx.prepare_batch(images, labels, params_of(samples, flips), window=WINDOW, mean=MEAN, std=STD, grids=GRIDS[:1], id_map=ID_MAP)
    check_labels(inv, ref2)
    check_fp32(inv.image, ref2)
    # one stacked tensor of equal sizes, no id table, no grid
    stack_i = torch.from_numpy(np.stack([samples[0]["full"]] * 2)).to(dev)
    stack_l = torch.from_numpy(np.stack([samples[0]["label"]] * 2)).to(dev)
    two = spx.prepare_batch(stack_i, stack_l, params_of(samples[:1]) * 2, window=WINDOW, mean=MEAN, std=STD)
    ref3 = restate(samples[:1], WINDOW, [], None)
    assert two.latent == [] and np.array_equal(two.labels.cpu().numpy(), np.concatenate([ref3["labels"]] * 2))
    assert np.array_equal(two.image.cpu().numpy().view(np.int32), np.concatenate([ref3["f32"]] * 2).view(np.int32))


def test_raw_values_outside_the_tables():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    lab = np.array([[-3, 0, 9, 10], [2 ** 40, 5, 2 ** 32 + 3, -2 ** 31]], np.int64)
    img = torch.zeros(2, 4, 3, dtype=torch.uint8, device=dev)
    p = [spx.AugmentParams((2, 4), (0, 0), False)]
    kw = dict(window=(2, 4), mean=MEAN, std=STD, grids=[(2, 4)])
    mapped = spx.prepare_batch([img], [torch.from_numpy(lab).to(dev)], p, id_map=ID_MAP, **kw)
    assert np.array_equal(mapped.labels.cpu().numpy()[0], BR.convert(lab, ID_MAP))
    assert mapped.labels.cpu().numpy()[0].tolist() == [[0, 3, 2, 0], [0, 2, 0, 0]]
    plain = spx.prepare_batch([img], [torch.from_numpy(lab).to(dev)], p, **kw)
    assert np.array_equal(plain.latent[0].cpu().numpy()[0], lab)
    assert np.array_equal(plain.latent0[0].cpu().numpy()[0], BR.shifted_i32(lab))          # beyond int32: no class


def test_tile_edges():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    samples = [tile_sample()]
    grids = [(3, 300), (2, 37)]
    ref = restate(samples, (3, 300), grids, None)
    images, labels = upload(samples, dev, torch.int64)
    batch = spx.prepare_batch(images, labels, params_of(samples), window=(3, 300), mean=MEAN, std=STD, grids=grids)
    check_labels(batch, ref)
    got = batch.image.cpu().numpy()
    assert np.array_equal(got.view(np.int32), ref["f32"].view(np.int32))
    assert (np.abs(got.astype(np.float64) - ref["f64"]) <= np.stack([BR.image_bound(r, MEAN, STD) for r in ref["f64"]])).all()
    u8 = spx.prepare_batch(images, labels, params_of(samples), window=(3, 300), mean=MEAN, std=STD, dtype=torch.uint8, want_labels=False)
    assert np.array_equal(u8.image.cpu().numpy(), ref["u8"])


def test_fixture_cases_are_the_references(golden):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    fx = golden("batch_prepare")
    n_images = 0
    for name in (str(n) for n in fx["cases"]):
        m, Hc, Wc, hs, ws, y0, x0, flip, has_image, has_ids = (int(v) for v in fx[f"meta__{name}"])
        full = torch.from_numpy(fx[f"image__{name}"]).to(dev)
        image = full[m:full.shape[0] - m, m:full.shape[1] - m] if m else full
        label = torch.from_numpy(fx[f"label__{name}"]).to(dev)
        mean, std = fx[f"mean_std__{name}"]
        grids = [tuple(g) for g in fx[f"grids__{name}"].tolist()]
        batch = spx.prepare_batch([image], [label], [spx.AugmentParams((hs, ws), (y0, x0), bool(flip))], window=(Hc, Wc), mean=mean,
                                  std=std, grids=grids, id_map=fx[f"id_map__{name}"] if has_ids else None)
        assert np.array_equal(batch.labels.cpu().numpy()[0], fx[f"out_label__{name}"]), name
        for k in range(len(grids)):
            want = fx[f"latent{k}__{name}"]
            assert np.array_equal(batch.latent[k].cpu().numpy()[0], want), (name, k)
            assert np.array_equal(batch.latent0[k].cpu().numpy()[0], BR.shifted_i32(want)), (name, k)
        if has_image:
            ref64 = fx[f"out_image__{name}"]
            err = np.abs(batch.image.cpu().numpy()[0].astype(np.float64) - ref64)
            assert (err <= BR.image_bound(ref64, mean, std)).all(), (name, err.max())
            n_images += 1
    assert n_images >= 3


def test_resize_labels_equals_the_host_loop():
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd.utils import resize_label

    dev = gpu_device()
    g = np.random.default_rng(9)
    pairs = [((40, 52), (40, 52)), ((513, 513), (65, 65)), ((129, 257), (17, 33))]
    while len(pairs) < 20:
        pairs.append(((int(g.integers(1, 80)), int(g.integers(1, 80))), (int(g.integers(1, 90)), int(g.integers(1, 90)))))
    dtypes = list(DTYPES.values())
    for i, ((H, W), (h, w)) in enumerate(pairs):
        lab = g.integers(0, 120, (2, H, W))
        want = torch.stack([resize_label(l, (w, h)) for l in lab])
        dt = dtypes[i % 4]
        got = spx.resize_labels(torch.from_numpy(lab).to(dt).to(dev), grids=[(h, w)])
        assert len(got) == 1 and got[0].dtype == torch.int64 and torch.equal(got[0].cpu(), want), ((H, W), (h, w))
    # several grids, the id table and the shifted form in one launch; a sequence of equal shapes
    lab = g.integers(0, 12, (3, 65, 47))
    dev_lab = torch.from_numpy(lab).to(dev)
    grids = [(65, 47), (9, 6), (33, 24), (1, 1)]
    got = spx.resize_labels(list(dev_lab.unbind(0)), grids=grids, id_map=ID_MAP, shifted=True)
    for (h, w), t in zip(grids, got):
        want = torch.stack([resize_label(BR.convert(l, ID_MAP), (w, h)) for l in lab])
        assert t.dtype == torch.int32 and np.array_equal(t.cpu().numpy(), BR.shifted_i32(want.numpy())), (h, w)


def guarded(shape, dtype, dev, guard=96):
    """(flat buffer, the output inside it): ``guard`` poisoned elements on both sides."""
    n = int(np.prod(shape))
    flat = torch.empty(n + 2 * guard, dtype=torch.int32 if dtype == torch.float32 else dtype, device=dev)
    flat.fill_(POISON_F if dtype == torch.float32 else (POISON_I if dtype != torch.uint8 else 0xA5))
    view = flat.view(dtype) if dtype == torch.float32 else flat
    return flat, view[guard:guard + n].view(shape), guard


def assert_written(flat, guard, poison, all_written=True):
    f = flat.cpu()
    assert (f[:guard] == poison).all() and (f[-guard:] == poison).all(), "a write outside the output"
    if all_written:
        assert not (f[guard:-guard] == poison).any(), "an element left unwritten"


def test_no_stray_writes(mixed):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    samples, ref = mixed
    images, labels = upload(samples, dev, torch.int16)
    B = len(samples)
    img = guarded((B, 3) + WINDOW, torch.float32, dev)
    win = guarded((B,) + WINDOW, torch.int64, dev)
    lat = [guarded((B,) + g, torch.int64, dev) for g in GRIDS]
    lat0 = [guarded((B,) + g, torch.int32, dev) for g in GRIDS]
    out = spx.PreparedBatch(img[1], win[1], [t[1] for t in lat], [t[1] for t in lat0])
    batch = spx.prepare_batch(images, labels, params_of(samples), window=WINDOW, mean=MEAN, std=STD, grids=GRIDS, id_map=ID_MAP, out=out)
    assert batch.image is img[1] and batch.latent[0] is lat[0][1]
    check_labels(batch, ref)
    assert_written(img[0], img[2], POISON_F)
    for flat, _, guard in [win] + lat + lat0:
        assert_written(flat, guard, POISON_I)
    # the uint8 image: 0xA5 is a legal byte, so only the guard band is read
    img8 = guarded((B, 3) + WINDOW, torch.uint8, dev)
    spx.prepare_batch(images, labels, params_of(samples), window=WINDOW, mean=MEAN, std=STD, dtype=torch.uint8, want_labels=False,
                      out=spx.PreparedBatch(img8[1], None, [], None))
    assert_written(img8[0], img8[2], 0xA5, all_written=False)
    assert np.array_equal(img8[1].cpu().numpy(), ref["u8"])
    res = guarded((B, 9, 11), torch.int64, dev)
    spx.resize_labels(torch.from_numpy(ref["labels"]).to(dev), grids=[(9, 11)], out=[res[1]])
    assert_written(res[0], res[2], POISON_I)
    assert np.array_equal(res[1].cpu().numpy(), ref["latent"][1])


def test_prepare_and_cross_entropy_replay_from_a_graph(mixed):
    """The captured step returns only the loss and what the test compares; the caller's table outlives it.  A refill of the table
    between replays gives the next replay new flips."""
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import graphs

    dev = gpu_device()
    samples, ref = mixed
    images, labels = upload(samples, dev, torch.uint8)
    K, (h, w) = 6, GRIDS[1]
    logits = torch.randn(len(samples), h, w, K, generator=torch.Generator().manual_seed(1)).to(dev)
    ce = spx.PixelWiseCrossEntropyLoss(ignore_index=-1)
    params = params_of(samples)
    kw = dict(window=WINDOW, grids=GRIDS[1:2], id_map=ID_MAP)
    table = spx.BatchTable(dev, batch=len(samples), index_entries=2048)
    with pytest.raises(spx.SpxError, match="do not fit"):
        spx.prepare_batch(images, labels, params, mean=MEAN, std=STD, table=spx.BatchTable(dev, batch=2, index_entries=2048), **kw)

    def step():
        batch = spx.prepare_batch(images, labels, params, mean=MEAN, std=STD, table=table, **kw)
        assert batch.table is table
        return batch.image, batch.labels, batch.latent[0], ce(logits, batch.latent[0])

    want = [t.clone() for t in step()]
    torch.cuda.synchronize()
    graph, out = graphs.capture_step(step, warmup=1)
    for t in out:
        t.zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, want):
        assert torch.equal(bits(a), bits(b))
    assert np.array_equal(out[2].cpu().numpy(), ref["latent"][1])
    labels0 = torch.from_numpy(ref["latent"][1]).reshape(-1) - 1
    keep = labels0 >= 0
    host = torch.nn.functional.cross_entropy(logits.cpu().reshape(-1, K)[keep].double(), labels0[keep])
    assert abs(out[3].item() - host.item()) <= 1e-5 * max(1.0, abs(host.item()))

    # the next replay with every flip inverted: the table is refilled, the graph is the same
    flips = [not s["flip"] for s in samples]
    ref2 = restate(samples, WINDOW, GRIDS[1:2], ID_MAP, flips)
    spx.fill_batch_table(table, images, labels, params_of(samples, flips), **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out[1].cpu().numpy(), ref2["labels"]) and np.array_equal(out[2].cpu().numpy(), ref2["latent"][0])
    assert np.array_equal(out[0].cpu().numpy().view(np.int32), ref2["f32"].view(np.int32))
    assert not np.array_equal(ref2["labels"], ref["labels"])
    with pytest.raises(spx.SpxError, match="fill_batch_table needs"):
        spx.fill_batch_table(table, images, labels, params, window=WINDOW, grids=GRIDS[:1], id_map=ID_MAP)


def test_a_captured_call_without_a_table_is_refused(mixed):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    lab = torch.zeros(1, 8, 8, dtype=torch.int64, device=dev)
    table = spx.BatchTable(dev, batch=1, index_entries=64)
    want = spx.resize_labels(lab + 3, grids=[(2, 3)], table=table)[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        src = lab + 3
        spx.resize_labels(src, grids=[(2, 3)], table=table)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    refused = []
    with torch.cuda.graph(g, stream=s):
        try:
            spx.resize_labels(src, grids=[(2, 3)])
        except spx.SpxError as e:
            refused.append(str(e))
        got = spx.resize_labels(src, grids=[(2, 3)], table=table)[0]
    got.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert refused and "BatchTable" in refused[0] and torch.equal(got, want)
