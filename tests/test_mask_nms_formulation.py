"""The plain formulation of mask NMS (tests/mask_nms_formulation.py) against keep lists written out by hand, and the
quantisation of the threshold as the host wrapper forms it (no GPU)."""
import numpy as np
import pytest

import mask_nms_formulation as F


@pytest.mark.parametrize("size", F.SIZES, ids=["%dx%d" % s for s in F.SIZES])
def test_named_cases_give_their_hand_written_keep_lists(size):
    H, W = size
    cases = F.named_cases(H, W)
    assert len(cases) >= 15
    for name, c in cases.items():
        got = F.reference(c["masks"], c["scores"], c["labels"], c["thresh"], c["measure"], c["class_agnostic"])
        assert got.dtype == np.uint8 and got.tolist() == c["expect"].tolist(), (name, got.tolist())


def test_the_cases_have_the_areas_and_intersections_they_are_named_for():
    for H, W in F.SIZES:
        c = F.named_cases(H, W)
        a, b = c["exact_threshold"]["masks"]
        assert (a.sum(), b.sum(), (a & b).sum()) == (3, 3, 2)
        a, b = c["just_below"]["masks"]
        assert (a.sum(), b.sum(), (a & b).sum()) == (4, 4, 2)
        a, b = c["nested_iou"]["masks"]
        assert (a & b).sum() == b.sum() == 2 and a.sum() == 8
        a, b = c["boxes_overlap_pixels_do_not"]["masks"]
        assert (a & b).sum() == 0
        for m in (a, b):   # equal 3 x 3 boxes
            ys, xs = np.nonzero(m)
            assert (ys.min(), ys.max(), xs.min(), xs.max()) == (0, 2, 0, 2)
        m = c["last_partial_word"]["masks"][0]
        ks = sorted(int(x) * H + int(y) for y, x in zip(*np.nonzero(m)))
        assert ks == [H * W - 3, H * W - 2, H * W - 1]
        assert c["empty_among_full"]["masks"][0].sum() == 0
    # at the sizes with more than one word the shifted cases straddle words 0 and 1 of the column-major flattening
    m = F.named_cases(37, 53)["chain"]["masks"][1]
    ks = [int(x) * 37 + int(y) for y, x in zip(*np.nonzero(m))]
    assert min(ks) < 64 <= max(ks)


def test_quantisation():
    assert F.quantise(0.3) == 314573 and F.quantise(0.5) == 1 << 19 and F.quantise(1.0) == 1 << 20
    assert F.quantise(1.0 / 3.0) == 349525 and F.quantise(2.0 ** -20) == 1
    from maskrcnn_benchmark import _hip as H
    for t in (0.3, 0.5, 1.0, 1.0 / 3.0, 2.0 ** -20, 0.7, 0.123456789):
        assert H.mask_nms_threshold_q20(t) == F.quantise(t)
    for t in (0.0, -0.1, 1.0000001, 2.0 ** -22):
        with pytest.raises(RuntimeError):
            H.mask_nms_threshold_q20(t)


def test_the_binding_declares_the_two_entry_points():
    import ctypes
    from maskrcnn_benchmark import _hip as H
    assert {"mmt_mask_nms", "mmt_mask_nms_workspace"} <= set(H.exported_symbols())
    sig = H._SIGS["mmt_mask_nms"]
    assert len(sig) == 15 and sig[11] is ctypes.c_int64
    assert H.MASK_NMS_MEASURES == {"iou": 0, "iomin": 1} and H.MASK_NMS_MAX == 1024
    # the query launches nothing and needs no GPU
    n = ctypes.c_int64(-1)
    L = ctypes.CDLL(H.LIB_PATH)
    assert L.mmt_mask_nms_workspace(200, ctypes.byref(n)) == 0 and n.value == 200 * 200
    assert L.mmt_mask_nms_workspace(1025, ctypes.byref(n)) == -22 and L.mmt_mask_nms_workspace(-1, ctypes.byref(n)) == -22
    assert L.mmt_mask_nms_workspace(0, ctypes.byref(n)) == 0 and n.value == 0


def test_random_blobs_overlap_tie_and_hold_empty_masks():
    masks, scores, labels = F.random_blobs(200, 100, 120, seed=5)
    assert masks.shape == (200, 100, 120) and len(np.unique(scores)) < 200 and set(labels.tolist()) == {1, 2, 3}
    assert (masks.reshape(200, -1).sum(1) == 0).sum() >= 5
    kept = [int(F.reference(masks, scores, labels, 0.5, m, a).sum()) for m in ("iou", "iomin") for a in (False, True)]
    # suppression happens in every mode, and the modes differ (a greedy sweep is not monotone in its relation: no order is asserted)
    assert all(0 < k < 200 for k in kept) and len(set(kept)) > 1, kept
