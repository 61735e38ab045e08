"""Polygon ground truth in the run-length codec, host side (no GPU): `mask_rle.frPolygons` against the oracle's rleFrPoly
restatement (oracle.native.poly_mask) on every instance of tests/polygon_image_inputs.py, byte for byte; and the refusals of the
new host-visible interfaces (SegmentationMask.decode / Polygons.convert, the `_hip` bindings)."""
import numpy as np
import pytest
import torch

import polygon_image_inputs as pi
from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle
from maskrcnn_benchmark.structures.segmentation_mask import Polygons, SegmentationMask

ALL_SIZES = pi.SIZES + [pi.BIG]


@pytest.mark.parametrize("size", ALL_SIZES, ids=lambda s: "%dx%d" % s)
def test_host_strings_equal_the_encoded_oracle_masks(size):
    H, W = size
    c, want = pi.cases(size), pi.oracle_masks(size)
    got = mask_rle.frPolygons(pi.segm_of(c), H, W)
    assert len(got) == len(want) > 0
    for g, r in enumerate(got):
        e = mask_rle.encode(want[g])
        assert r["size"] == [H, W] and isinstance(r["counts"], bytes)
        assert r["counts"] == e["counts"], (size, g, c["cls"][g])
    if H * W > 1:
        assert len({r["counts"] for r in got}) > len(got) // 2        # (not one string many times)


@pytest.mark.parametrize("size", pi.SIZES, ids=lambda s: "%dx%d" % s)
def test_decode_round_trips(size):
    H, W = size
    want = pi.oracle_masks(size)
    got = mask_rle.frPolygons(pi.segm_of(pi.cases(size)), H, W)
    dec = mask_rle.decode(got)
    assert dec.shape == (H, W, len(want)) and np.array_equal(dec.transpose(2, 0, 1), want)
    assert [mask_rle.encode(dec[:, :, g])["counts"] for g in range(len(got))] == [r["counts"] for r in got]
    assert np.array_equal(mask_rle.area(got), want.reshape(len(want), -1).sum(1))


def test_frPolygons_takes_a_segmentation_mask_and_flat_lists():
    size = (37, 53)
    c = pi.cases(size)
    segm = pi.segm_of(c)
    full = [s for s in segm if s]
    sm = SegmentationMask([[torch.from_numpy(p) for p in inst] for inst in full], (size[1], size[0]), mode="poly")
    want = mask_rle.frPolygons(full, *size)
    assert mask_rle.frPolygons(sm, *size) == want
    assert mask_rle.frPolygons([[p.tolist() for p in inst] for inst in full], *size) == want
    assert mask_rle.frPolygons([], *size) == []
    assert mask_rle.area(mask_rle.frPolygons([[]], *size)[0]) == 0     # no polygon: an empty mask


def test_convert_refuses_other_modes():
    p = Polygons([[1.0, 1.0, 5.0, 1.0, 5.0, 5.0]], (8, 8), mode="poly")
    for mode in ("poly", "rle", None):
        with pytest.raises(NotImplementedError):
            p.convert(mode)


def test_decode_refuses_another_size():
    sm = SegmentationMask([[[1.0, 1.0, 5.0, 1.0, 5.0, 5.0]]], (8, 6), mode="poly")     # size is (w, h)
    for h, w in ((8, 6), (6, 9), (800, 800)):
        with pytest.raises(ValueError):
            sm.decode(h, w)


def test_bindings_refuse_host_tensors():
    from maskrcnn_benchmark import _hip
    xy, off, rng = torch.zeros(6), torch.tensor([0, 3], dtype=torch.int32), torch.tensor([[0, 1]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        _hip.polygon_mask_words(xy, off, rng, 8, 8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        _hip.mask_words_integral(torch.zeros((1, 1), dtype=torch.int64), [0, 1], 8, 8)


def test_evaluator_takes_polygon_ground_truth():
    """prepare_for_pap_segmentation with a ground-truth `masks` field that is a SegmentationMask: the same RLEs (str counts, like the
    detections') as a field that already holds frPolygons' dicts"""
    from maskrcnn_benchmark.data.datasets.evaluation.pap.pap_eval import prepare_for_pap_segmentation
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    size = (64, 64)
    c = pi.cases(size)
    full = [s for s in pi.segm_of(c) if s][:6]
    want = mask_rle.frPolygons(full, *size)

    class DS(object):
        maxWS = 64
        id_to_img_map = {0: {"file_name": "a", "location": (0, 0), "id": 1}}
        contiguous_category_id_to_json_id = {1: 1, 2: 2}

        def __init__(self, polygons):
            self.polygons = polygons

        def get_ground_truth(self, original_id):
            b = BoxList(torch.zeros((len(full), 4)), (64, 64), "xyxy")
            b.add_field("labels", torch.tensor([1 + g % 2 for g in range(len(full))], dtype=torch.int64))
            if self.polygons:
                b.add_field("masks", SegmentationMask([[torch.from_numpy(p) for p in inst] for inst in full], (64, 64), mode="poly"))
            else:
                b.add_field("masks", [dict(r, counts=r["counts"].decode("utf-8")) for r in want])
            return b

    pred = BoxList(torch.tensor([[4.0, 4.0, 20.0, 20.0]]), (64, 64), "xyxy")
    m = torch.zeros((1, 1, 64, 64), dtype=torch.uint8)
    m[0, 0, 4:21, 4:21] = 1
    pred.add_field("mask", m)
    pred.add_field("scores", torch.tensor([0.9], dtype=torch.float64))
    pred.add_field("labels", torch.tensor([1], dtype=torch.int64))
    g_poly, d_poly = prepare_for_pap_segmentation({0: pred}, DS(True))
    g_rle, d_rle = prepare_for_pap_segmentation({0: pred}, DS(False))
    assert g_poly == g_rle and d_poly == d_rle and len(g_poly) == len(full)
    for g, r in zip(g_poly, want):
        assert isinstance(g["segmentation"]["counts"], str) and g["segmentation"]["counts"] == r["counts"].decode("utf-8")
        assert g["segmentation"]["size"] == [64, 64]
