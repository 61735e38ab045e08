"""The plain Soft-NMS formulation (tests/soft_nms_formulation.py) on cases worked out by hand, and the conditions under which
the GPU tests may compare pick orders: the oracle is only an oracle if it is right, and a pick order is only comparable
where no decision hangs on the last bits (no GPU)."""
import math

import numpy as np
import pytest

import soft_nms_formulation as F

# 100 x 100 (area 10000 with the +1), its upper half (area 5000, inside A: IoU 5000 / 10000 = 0.5), and a box far away
A, B, C = [0, 0, 99, 99], [0, 0, 99, 49], [200, 200, 299, 299]
THREE = (np.asarray([A, B, C], np.float32), np.asarray([0.9, 0.8, 0.7], np.float32))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_three_boxes_by_hand(dtype):
    # linear, thr 0.5: A is picked, B (IoU exactly 0.5, and >= counts) falls to 0.8 * 0.5 = 0.4 and C overtakes it
    p, s = F.soft_nms(*THREE, "linear", 0.5, 0.5, 0.001, dtype)
    assert p.tolist() == [0, 2, 1] and s.dtype == dtype
    np.testing.assert_allclose(s, [0.9, 0.4, 0.7], rtol=1e-6)
    # thr just above the overlap: nothing decays
    p, s = F.soft_nms(*THREE, "linear", 0.51, 0.5, 0.001, dtype)
    assert p.tolist() == [0, 1, 2] and s.astype(np.float32).tolist() == THREE[1].tolist()
    # gaussian, sigma 0.5: B falls to 0.8 * exp(-0.25 / 0.5) = 0.4852, whatever the threshold; IoU 0 decays nothing
    for thr in (0.5, 0.9):
        p, s = F.soft_nms(*THREE, "gaussian", thr, 0.5, 0.001, dtype)
        assert p.tolist() == [0, 2, 1]
        np.testing.assert_allclose(s, [0.9, 0.8 * math.exp(-0.5), 0.7], rtol=1e-6)
    # a wider sigma decays less: 0.8 * exp(-0.25 / 2) = 0.706 stays ahead of C
    p, s = F.soft_nms(*THREE, "gaussian", 0.5, 2.0, 0.001, dtype)
    assert p.tolist() == [0, 1, 2]
    np.testing.assert_allclose(s, [0.9, 0.8 * math.exp(-0.125), 0.7], rtol=1e-6)


def test_chain_where_the_middle_box_is_overtaken():
    boxes, _ = F.chain(3)
    scores = np.asarray([0.9, 0.8, 0.7], np.float32)
    ov = F.iou(boxes[0], boxes[1:], np.float64)
    np.testing.assert_allclose(ov, [71.0 / 131.0, 41.0 / 161.0], rtol=1e-12)
    # A decays B (0.54 >= 0.5) but not C (0.25); C is picked next and decays B again; B comes last with 0.8 * (60 / 131)^2
    p, s = F.soft_nms(boxes, scores, "linear", 0.5, 0.5, 0.001, np.float64)
    assert p.tolist() == [0, 2, 1]
    np.testing.assert_allclose(s, [0.9, np.float32(0.8) * (60.0 / 131.0) ** 2, 0.7], rtol=1e-6)
    # the greedy NMS would have dropped B: with soft-NMS every box of the chain comes out
    for n in (2, 17, 64):
        p, s = F.soft_nms(*F.chain(n), "linear", 0.5, 0.5, 0.001)
        assert sorted(p.tolist()) == list(range(n))
        assert (np.diff(s[p]) <= 0).all()            # pick order is descending final score


def test_equal_scores_go_by_position():
    boxes, _ = F.disjoint(5)
    p, s = F.soft_nms(boxes, np.full(5, 0.5, np.float32), "linear", 0.5, 0.5, 0.001)
    assert p.tolist() == [0, 1, 2, 3, 4] and s.tolist() == [0.5] * 5
    # A and its half B at one score: A (position 0) is picked and halves B
    p, s = F.soft_nms(np.asarray([A, B, C], np.float32), np.full(3, 0.5, np.float32), "linear", 0.5, 0.5, 0.001)
    assert p.tolist() == [0, 2, 1] and s.tolist() == [0.5, 0.25, 0.5]
    p, s = F.soft_nms(np.asarray([B, A, C], np.float32), np.full(3, 0.5, np.float32), "linear", 0.5, 0.5, 0.001)
    assert p.tolist() == [0, 2, 1] and s.tolist() == [0.5, 0.25, 0.5]


def test_stop_at_min_score():
    # the same box three times: the first pick multiplies the others by 1 - 1 = 0, and 0 < MIN_SCORE ends it
    p, s = F.soft_nms(*F.all_equal(3), "linear", 0.5, 0.5, 0.001)
    assert p.tolist() == [0] and s.tolist() == [np.float32(0.9), 0.0, 0.0]
    # B's 0.4 is below MIN_SCORE 0.45: it is not picked and keeps the decayed score; at exactly 0.4 it is (the stop is `<`)
    p, s = F.soft_nms(*THREE, "linear", 0.5, 0.5, 0.45)
    assert p.tolist() == [0, 2]
    np.testing.assert_allclose(s, [0.9, 0.4, 0.7], rtol=1e-6)
    p, s = F.soft_nms(*THREE, "linear", 0.5, 0.5, float(s[1]))
    assert p.tolist() == [0, 2, 1]
    # nothing qualifies / nothing is there
    p, s = F.soft_nms(*THREE, "gaussian", 0.5, 0.5, 0.95)
    assert p.tolist() == [] and s.tolist() == THREE[1].tolist()
    p, s = F.soft_nms(np.zeros((0, 4), np.float32), np.zeros((0,), np.float32), "linear", 0.5, 0.5, 0.001)
    assert p.tolist() == [] and s.shape == (0,)


def test_overlaps_that_are_not_numbers_decay_nothing():
    boxes = np.asarray([A, [np.nan] * 4, B], np.float32)
    for method in F.METHODS:
        p, s = F.soft_nms(boxes, np.asarray([0.9, 0.8, 0.7], np.float32), method, 0.5, 0.5, 0.001)
        assert p.tolist()[:2] == [0, 1] and s[1] == np.float32(0.8) and s[2] < np.float32(0.7)


def test_filter_results_soft_by_hand():
    # one image, two foreground classes; class 1 sees A, B, C (rows 2, 0, 1 by score), class 2 only row 3
    prob = np.asarray([[0.1, 0.8, 0.01], [0.1, 0.7, 0.02], [0.0, 0.9, 0.03], [0.2, 0.04, 0.4]], np.float32)
    box = {0: B, 1: C, 2: A, 3: C}
    dec = np.zeros((4, 12), np.float32)
    for r in range(4):
        dec[r, 4:8] = dec[r, 8:12] = box[r]
    (bb, sc, lb), = F.filter_results_soft(prob, dec, [4], 0.05, 0.5, 0, "linear", 0.5, 0.001)
    assert lb.tolist() == [1, 1, 1, 2]                       # ascending row inside a class, classes concatenated
    assert sc.tolist() == [np.float32(0.8) * np.float32(0.5), np.float32(0.7), np.float32(0.9), np.float32(0.4)]
    assert bb.tolist() == [list(map(float, b)) for b in (B, C, A, C)]
    # the cut keeps `score >= kthvalue`: D = 3 has the two 0.4 tie at the cut and keeps all four, D = 2 keeps two
    (_, sc3, _), = F.filter_results_soft(prob, dec, [4], 0.05, 0.5, 3, "linear", 0.5, 0.001)
    assert len(sc3) == 4
    (_, sc2, lb2), = F.filter_results_soft(prob, dec, [4], 0.05, 0.5, 2, "linear", 0.5, 0.001)
    assert sc2.tolist() == [np.float32(0.7), np.float32(0.9)] and lb2.tolist() == [1, 1]


def test_generator():
    b, s = F.clustered(2048, 0)
    assert b.shape == (2048, 4) and b.dtype == np.float32 and s.dtype == np.float32
    assert (np.diff(s) <= 0).all() and s.min() > 0.05 and s.max() < 1.0
    assert (b[:, 2] > b[:, 0]).all() and (b[:, 3] > b[:, 1]).all() and b.min() >= 0 and b.max() <= 999
    side = np.concatenate([b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]])
    assert side.max() <= 132.0 + 1e-3
    # crowded: most boxes have a neighbour at IoU >= 0.5
    crowded = sum((F.iou(b[i], np.delete(b, i, 0), np.float32) >= 0.5).any() for i in range(0, 2048, 16))
    assert crowded > 96
    # the other kinds do what their names say
    bd, _ = F.disjoint(257)
    assert max(F.iou(bd[i], np.delete(bd, i, 0), np.float32).max() for i in range(257)) == 0.0
    be, _ = F.all_equal(5)
    assert (F.iou(be[0], be, np.float32) == 1.0).all()


def test_the_gaussian_comparison_is_well_conditioned():
    """what tests/test_soft_nms_gpu.py relies on: at every pick of the gaussian inputs the best current score leads the second
    best by at least 100 tolerances (in fp64), and no final score lies within a tolerance of MIN_SCORE -- so arithmetic that
    stays inside the tolerance cannot change a decision"""
    tol = F.gaussian_tolerance()
    print("gaussian tolerance (4 x fp32-vs-fp64 deviation of the restatement): %.3e" % tol)
    # an fp32 chain of at most 64 decays, each a handful of roundings of 2^-24: far below the gaps, and not zero
    assert 0.0 < tol <= 4 * 64 * 4 * 2.0 ** -24
    smallest = 1.0
    for n, seed in F.GAUSS_INPUTS:
        b, s = F.clustered(n, seed)
        gaps = []
        p, final = F.soft_nms(b, s, "gaussian", dtype=np.float64, gaps=gaps, **F.GAUSS)
        assert len(p) > 0
        if gaps:
            smallest = min(smallest, min(gaps))
        assert (np.abs(final - F.GAUSS["min_score"]) / F.GAUSS["min_score"] > tol).all()
    print("smallest relative gap between the best and the second-best score: %.3e" % smallest)
    assert smallest >= 100 * tol


def test_fp32_restatement_stays_close_at_2048():
    b, s = F.clustered(2048, 0)
    p64, s64 = F.soft_nms(b, s, "gaussian", dtype=np.float64, **F.GAUSS)
    p32, s32 = F.soft_nms(b, s, "gaussian", dtype=np.float32, **F.GAUSS)
    agree = min(len(p32), len(p64))
    first = next((i for i in range(agree) if p32[i] != p64[i]), agree)
    print("n = 2048: %d picks, first differing pick %d, deviation of the scores %.3e" % (len(p64), first, F.rel_dev(s32, s64)))
    assert F.rel_dev(s32, s64) < 1e-5
