"""BinaryMaskList on the host (structures/segmentation_mask.py): construction from arrays, RLE dicts and another list, what it
refuses, that use without a GPU raises, that RLE-built ground truth passes through the evaluator's host path unchanged, and that
BoxList's field mapping reaches it -- shown with a stub device: the three launches it would make are replaced by the host
restatement of tests/bitmask_formulation.py.  No GPU."""
import numpy as np
import pytest
import torch

import bitmask_formulation as bf
from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle, pap_eval
from maskrcnn_benchmark.structures.bounding_box import BoxList
from maskrcnn_benchmark.structures.segmentation_mask import (BinaryMaskList, SegmentationMask, mask_window, FLIP_LEFT_RIGHT,
                                                             FLIP_TOP_BOTTOM)

H, W = 37, 53


def _masks(g=4, seed=0, h=H, w=W):
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand((g, h, w), generator=gen) < 0.4).to(torch.uint8)


def test_construction_len_size_repr():
    m = _masks()
    for src in (m, m.bool(), m.numpy(), m.numpy().astype(bool)):
        b = BinaryMaskList(src, (W, H))
        assert len(b) == 4 and tuple(b.size) == (W, H)
        assert repr(b) == "BinaryMaskList(num_instances=4, image_width=53, image_height=37)"
    one = BinaryMaskList(m[0], (W, H))
    assert len(one) == 1
    rles = [mask_rle.encode(x.numpy()) for x in m]
    r = BinaryMaskList(rles, (W, H))
    assert len(r) == 4 and tuple(r.size) == (W, H) and r.source_rles() == rles
    text = BinaryMaskList([dict(x, counts=x["counts"].decode("ascii")) for x in rles], (W, H))
    assert len(text) == 4
    again = BinaryMaskList(r, (W, H))
    assert len(again) == 4 and tuple(again.size) == (W, H) and again.source_rles() == rles
    for empty in (BinaryMaskList([], (W, H)), BinaryMaskList(torch.zeros((0, H, W), dtype=torch.uint8), (W, H))):
        assert len(empty) == 0 and list(empty) == [] and "num_instances=0" in repr(empty)
    assert b.to("cpu") is b


def test_refusals():
    m = _masks()
    with pytest.raises(ValueError):
        BinaryMaskList(m, (H, W))                                  # (w, h) the wrong way round
    with pytest.raises(ValueError):
        BinaryMaskList(m[0, :, :-1], (W, H))
    with pytest.raises(ValueError):
        BinaryMaskList(m.float(), (W, H))
    with pytest.raises(ValueError):
        BinaryMaskList(m[None], (W, H))
    with pytest.raises(ValueError):
        BinaryMaskList([mask_rle.encode(m[0].numpy()[:, :-1])], (W, H))
    with pytest.raises(ValueError):
        BinaryMaskList([[0.0, 0.0, 4.0, 0.0, 4.0, 4.0]], (W, H))   # polygons are SegmentationMask's
    with pytest.raises(ValueError):
        BinaryMaskList(BinaryMaskList(m, (W, H)), (W + 1, H))
    with pytest.raises(ValueError):
        BinaryMaskList("masks.png", (W, H))
    b = BinaryMaskList(m, (W, H))
    with pytest.raises(NotImplementedError):
        b.transpose(2)
    with pytest.raises(ValueError):
        b.crop([0.0, float("nan"), 5.0, 5.0])
    with pytest.raises(IndexError):
        b[4]
    with pytest.raises(IndexError):
        b[torch.tensor([True, False])]


def test_use_without_a_gpu_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    b = BinaryMaskList(_masks(), (W, H))
    with pytest.raises(RuntimeError) as want:
        SegmentationMask._device(None)
    for use in (b.mask_words, lambda: b.decode(H, W), b.get_mask_tensor, b.rles, lambda: b.resize((20, 10)).mask_words(),
                lambda: b[1:3].mask_words(), lambda: b.transpose(0).rles()):
        with pytest.raises(RuntimeError) as got:
            use()
        assert str(got.value) == str(want.value)
    with pytest.raises(ValueError):
        b.decode(W, H)                                             # the size is checked first, as SegmentationMask does


def test_host_window_is_the_formulation():
    rng = np.random.RandomState(0)
    boxes = rng.uniform(-30, 90, (200, 4)).astype(np.float32)
    boxes[::3] = np.round(boxes[::3] * 2) / 2                      # half-integers
    for b in boxes:
        assert mask_window(b, W, H) == bf.window(b, W, H)
    assert mask_window([float("inf"), 0, 1, 1], W, H) is None


class _Dataset(object):
    maxWS = W
    id_to_img_map = {0: "a"}
    contiguous_category_id_to_json_id = {1: 7}

    def __init__(self, target):
        self.target = target

    def get_ground_truth(self, original_id):
        return self.target


def test_rle_ground_truth_passes_through_the_evaluator_unchanged(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    m = torch.zeros((3, W, W), dtype=torch.uint8)
    m[0, 3:9, 4:11] = m[1, 20:30, 20:25] = m[2, 0, :] = 1
    rles = [mask_rle.encode(x.numpy()) for x in m]
    for r in rles:
        r["counts"] = r["counts"].decode("ascii")
    keep = [dict(r) for r in rles]
    target = BoxList(torch.tensor([[4., 3., 10., 8.], [20., 20., 24., 29.], [0., 0., 52., 0.]]), (W, W))
    target.add_field("labels", torch.tensor([1, 1, 1]))
    target.add_field("masks", BinaryMaskList(rles, (W, W)))
    pred = BoxList(torch.tensor([[4., 3., 10., 8.]]), (W, W))
    pred.add_field("mask", m[:1, None])
    pred.add_field("scores", torch.tensor([0.9]))
    pred.add_field("labels", torch.tensor([1]))
    gts, dts = pap_eval.prepare_for_pap_segmentation({0: pred}, _Dataset(target), on_device=False)
    assert [g["segmentation"] for g in gts] == keep and rles == keep
    assert all(g["segmentation"] is r for g, r in zip(gts, rles))
    assert [g["category_id"] for g in gts] == [7, 7, 7] and len(dts) == 1
    assert dts[0]["segmentation"]["counts"] == keep[0]["counts"]


# ---- the stub device: words on the host
def _unpack(words, h, w):
    bits = (words[:, :, None] >> torch.arange(64, dtype=torch.int64)) & 1
    return bits.reshape(words.shape[0], -1)[:, :h * w].reshape(-1, w, h).transpose(1, 2).to(torch.uint8).contiguous()


@pytest.fixture
def stub(monkeypatch):
    from maskrcnn_benchmark import _hip
    calls = []

    def pack(masks):
        calls.append("pack")
        return bf.pack(masks)

    def resample(words, h, w, window, flip, oh, ow):
        calls.append(("resample", tuple(window), flip, oh, ow))
        return bf.pack(bf.resample(_unpack(words, h, w), tuple(window), oh, ow, flip))

    monkeypatch.setattr(_hip, "mask_pack", pack)
    monkeypatch.setattr(_hip, "mask_words_resample", resample)
    monkeypatch.setattr(SegmentationMask, "_device", staticmethod(lambda device=None: torch.device("cpu")))
    return calls


def _bytes(b):
    return _unpack(b.mask_words()[0], b.size[1], b.size[0])


def test_boxlist_field_mapping_reaches_the_list(stub):
    m = _masks()
    t = BoxList(torch.tensor([[1., 2., 30., 20.], [5., 5., 50., 35.], [0., 0., 10., 10.], [20., 3., 40., 30.]]), (W, H))
    t.add_field("labels", torch.tensor([1, 2, 1, 2]))
    t.add_field("masks", BinaryMaskList(m, (W, H)))

    r = t.resize((106, 74))
    f = r.get_field("masks")
    assert isinstance(f, BinaryMaskList) and tuple(f.size) == (106, 74) and len(f) == 4 and stub == []   # recorded, not run
    assert torch.equal(_bytes(f), bf.resample(m, (0, 0, W, H), 74, 106))
    assert stub == ["pack", ("resample", (0, 0, W, H), 0, 74, 106)]
    assert torch.equal(_bytes(t.resize((40, 30)).get_field("masks")), bf.resample(m, (0, 0, W, H), 30, 40))

    for method, flip in ((FLIP_LEFT_RIGHT, 1), (FLIP_TOP_BOTTOM, 2)):
        f = t.transpose(method).get_field("masks")
        assert isinstance(f, BinaryMaskList) and tuple(f.size) == (W, H)
        assert torch.equal(_bytes(f), m.flip(2 if flip == 1 else 1))
        assert torch.equal(_bytes(f.transpose(method)), m)

    c = t.crop([3, 4, 43, 29])
    f = c.get_field("masks")
    assert isinstance(f, BinaryMaskList) and tuple(f.size) == (40, 25) == tuple(c.size)
    assert torch.equal(_bytes(f), m[:, 4:29, 3:43])

    for item, rows in ((1, [1]), (slice(1, 3), [1, 2]), ([3, 0], [3, 0]), (torch.tensor([2, 2, 1]), [2, 2, 1]),
                       (torch.tensor([True, False, True, True]), [0, 2, 3])):
        f = (t[item] if not isinstance(item, int) else t[[item]]).get_field("masks")
        assert isinstance(f, BinaryMaskList) and len(f) == len(rows)
        assert torch.equal(_bytes(f), m[rows])
    assert torch.equal(_bytes(BinaryMaskList(m, (W, H))[-1]), m[3:])
    assert [len(x) for x in BinaryMaskList(m, (W, H))] == [1, 1, 1, 1]
    assert t.to("cpu").get_field("masks") is t.get_field("masks")

    # the input pipeline's order: resize, then flip
    f = t.resize((80, 56)).transpose(FLIP_LEFT_RIGHT).get_field("masks")
    assert torch.equal(_bytes(f), bf.resample(m, (0, 0, W, H), 56, 80).flip(2))


def test_words_are_cached(stub):
    b = BinaryMaskList(_masks(), (W, H))
    first = b.mask_words()
    assert b.mask_words() is first and stub == ["pack"]
    assert BinaryMaskList(b, (W, H)).mask_words() is first and stub == ["pack"]
