"""The inputs of tests/test_mask_geometry_gpu.py against the oracle alone (no GPU): a class of rasteriser cases whose targets
came out all ones or all zeros would compare equal whatever the kernel did inside the box."""
import numpy as np
import pytest

import mask_geometry_inputs as mg


@pytest.fixture(scope="module")
def cases():
    return mg.raster_cases()


def test_rasteriser_classes_are_all_there(cases):
    assert 380 <= len(cases["boxes"]) <= 420
    for c in mg.CLASSES:
        assert (cases["cls"] == c).sum() == mg.PER_CLASS, c
    n = cases["roi_poly"][:, 1] - cases["roi_poly"][:, 0]
    assert set(n[cases["cls"] != "h"]) == {1, 2, 3}
    assert (n[cases["cls"] == "h"] == 0).sum() >= 5                                   # empty ranges
    rp = cases["roi_poly"][cases["cls"] == "h"]
    assert len({tuple(r) for r in rp if r[1] > r[0]}) < (rp[:, 1] > rp[:, 0]).sum()    # shared ranges
    b = cases["boxes"][cases["cls"] == "a"]
    assert (np.minimum(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]) < 1).all()
    nv = np.diff(cases["poly_off"])
    assert (nv > 128).any() and (nv > 64).sum() >= 5                                  # more than one and two passes of 64 edges


@pytest.mark.parametrize("M", mg.RASTER_M)
def test_every_rasteriser_class_reaches_inside_its_box(cases, M):
    want = mg.oracle_targets(cases, M)
    assert set(np.unique(want)) == {0.0, 1.0}
    for c in mg.CLASSES:
        share = want[cases["cls"] == c].mean()
        print("M=%d class %s: share of ones %.3f" % (M, c, share))
        assert 0.02 < share < 0.98, (c, share)
    assert (want[cases["roi_poly"][:, 1] == cases["roi_poly"][:, 0]] == 0).all()


def test_only_the_comb_is_beyond_the_old_crossing_cap(cases):
    M = 28
    most = max(n for _, _, n in mg.crossing_counts(cases, M))
    comb = [n for _, _, n in mg.crossing_counts(mg.comb(), M)]
    long_comb = [n for _, _, n in mg.crossing_counts(mg.comb(130), M)]
    print("crossings at M=28: comb %s, comb of 130 edges %s, most of any other polygon %d" % (comb, long_comb, most))
    assert len(comb) == 1 and comb[0] > mg.OLD_CAP
    assert long_comb[0] > mg.OLD_CAP
    assert most < mg.OLD_CAP
    assert 0.02 < mg.oracle_targets(mg.comb(), M).mean() < 0.98


@pytest.mark.parametrize("M", mg.RASTER_M)
def test_the_restated_walk_is_the_oracles(cases, M):
    """the count above is of the right thing: the parity of the restated crossings at or below every pixel is the oracle's target,
    on every case and on both combs"""
    for c in (cases, mg.comb(), mg.comb(130)):
        np.testing.assert_array_equal(mg.parity_targets(c, M), mg.oracle_targets(c, M))


def test_paste_cases_cover_their_ranges():
    ih, iw = mg.CANVAS
    pc = mg.paste_cases()
    assert sorted(pc) == list(mg.PASTE_M) and 190 <= sum(len(b) for _, b in pc.values()) <= 210
    for M, (prob, boxes) in pc.items():
        assert prob.shape == (len(boxes), M, M) and prob.min() >= 0 and prob.max() <= 1
        w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
        assert (w == 0).any() and (h == 0).any() and (w > iw).any() and (h > ih).any()
        assert (boxes[:, 0] < -5).any() and (boxes[:, 1] < -5).any() and (boxes[:, 2] > iw + 5).any() and (boxes[:, 3] > ih + 5).any()
        assert (boxes != np.round(boxes)).mean() > 0.9
    for M in mg.PASTE_M:
        assert all(mg.clipped_area(b, M, ih, iw) == 0 for b in mg.outside_boxes())


@pytest.mark.parametrize("M", [14, 28])
def test_integral_paste_leaves_out_almost_nothing(M):
    logits, labels, boxes, img = mg.integral_case(M)
    assert set(labels) == {1, 2} and set(img) == {-1, 0, 1}
    want, left, n_left, n_cov = mg.integral_reference(logits, labels, boxes, img)
    print("M=%d: %d of %d covered (detection, pixel) pairs within %g of the threshold; map maximum %d" % (M, n_left, n_cov, mg.NEAR,
                                                                                                     want.max()))
    assert n_cov > 50000 and want.max() >= 3
    assert n_left <= mg.LEFT_OUT_CAP * n_cov
    assert left.sum() <= n_left


def test_fp64_paste_values_threshold_to_the_oracles_paste():
    """the helper that finds the near-threshold pixels follows the oracle's paste: away from the threshold its values, thresholded,
    are the oracle's mask"""
    import torch
    from oracle import model as om
    ih, iw = mg.CANVAS
    for M, (prob, boxes) in mg.paste_cases().items():
        for pr, b in zip(prob, boxes):
            val, cov = mg.paste_values64(pr, b, ih, iw)
            want = om.paste_mask(torch.from_numpy(pr), torch.from_numpy(b), ih, iw, mg.PASTE_THRESH).numpy().astype(bool)
            far = np.abs(val - mg.PASTE_THRESH) >= mg.NEAR
            assert cov.sum() == mg.clipped_area(b, M, ih, iw) and not want[~cov].any()
            np.testing.assert_array_equal((val > mg.PASTE_THRESH)[far], want[far])
