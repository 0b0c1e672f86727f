"""The shared input layer of the full-resolution map operators (scaleprotoseg_amd/_maps.py), through the four entry points that
can be reached without a GPU: one wording of the label rule, shape and type checks before anything asks for a device."""
import pytest
import torch

import scaleprotoseg_amd as spx
from scaleprotoseg_amd import _maps
from scaleprotoseg_amd.metrics import eval_accumulate

N, C, h, w, H, W = 2, 4, 3, 5, 6, 10
TABLE = torch.tensor([[0, 1], [2, 3]])
PLANES = torch.zeros(N, C, h, w)


def _eval(planes, labels):
    eval_accumulate(planes.permute(0, 2, 3, 1), labels, torch.zeros((C + 1) * C, dtype=torch.int64))       # logits [N, h, w, K]


CALLS = {
    "eval_accumulate": (_eval, "logits"),
    "push_bounding_boxes": (lambda p, lab: spx.push_bounding_boxes(p, lab, torch.tensor([[0, 1, 0, 2]])), "activations"),
    "activation_heat_maps": (lambda p, lab: spx.activation_heat_maps(p, lab, [[0, 1, 1]], TABLE), "activations"),
    "dominant_slot_maps": (lambda p, lab: spx.dominant_slot_maps(p, lab, [[1, 0]], TABLE), "activations"),
}


@pytest.fixture(params=sorted(CALLS))
def entry(request):
    return CALLS[request.param]


def test_label_type_and_rank_share_one_sentence(entry):
    call, _ = entry
    cases = ((torch.zeros(N, H, W), "torch.float32 (2, 6, 10)"), (torch.zeros(N, H * W, dtype=torch.long), "torch.int64 (2, 60)"))
    for labels, got in cases:
        with pytest.raises(spx.SpxError) as e:
            call(PLANES, labels)
        assert str(e.value) == f"labels must be uint8, int32 or int64 [N, H, W] (got {got})"


def test_label_batch_count(entry):
    call, what = entry
    with pytest.raises(spx.SpxError) as e:
        call(PLANES, torch.zeros(3, H, W, dtype=torch.long))
    assert str(e.value) == f"labels hold 3 images, {what} 2"


def test_well_formed_cpu_inputs_only_lack_the_device(entry):
    call, _ = entry
    for dtype in (torch.uint8, torch.int32, torch.int64):
        with pytest.raises(spx.SpxError, match="no CPU fallback"):
            call(PLANES, torch.zeros(N, H, W, dtype=dtype))


def test_pixel_major_planes():
    t = torch.arange(N * h * w * C, dtype=torch.float32).reshape(N * h * w, C)
    want = t.view(N, h, w, C).permute(0, 3, 1, 2)
    got = _maps.planes(t, (h, w), "activations")
    assert got.shape == want.shape and got.stride() == want.stride() and torch.equal(got, want)
    assert got.data_ptr() == t.data_ptr()
    assert list(_maps.strides(got)) == list(want.stride())
    assert list(_maps.strides(t.view(N, h, w, C), (0, 3, 1, 2))) == list(want.stride())
    with pytest.raises(spx.SpxError, match="not a multiple of the grid"):
        _maps.planes(t, (h, w + 1), "activations")
    with pytest.raises(spx.SpxError, match="grid="):
        _maps.planes(t, None, "activations")


def test_slot_table():
    got = _maps.slot_table([[0, 1, -1], [2, 3, 4]])
    assert got.dtype == torch.int32 and got.is_contiguous() and got.tolist() == [[0, 1, -1], [2, 3, 4]]
    assert _maps.slot_table(torch.zeros(2, _maps.MAX_SLOTS, dtype=torch.long)).shape == (2, 32)
    with pytest.raises(spx.SpxError, match="33 slots per class \\(at most 32\\)"):
        _maps.slot_table(torch.zeros(2, 33, dtype=torch.long))
    with pytest.raises(spx.SpxError, match="slot_table must be integer"):
        _maps.slot_table(torch.zeros(2, 3))
    with pytest.raises(spx.SpxError, match="slot_table must be integer"):
        _maps.slot_table(torch.zeros(6, dtype=torch.long))
