"""Mask NMS at inference ("Mask NMS at inference"): the plain formulation and the inputs that
tests/test_mask_nms_formulation.py (CPU), tests/test_mask_nms_gpu.py and tests/test_mask_nms_model_gpu.py share.

reference() is numpy loops and a stable argsort with the integer test of the definition -- no floating point decides anything:
    order     score descending, equal scores in row order
    sweep     j is dropped when an earlier, still kept i has the same label (any label when class-agnostic) and overlaps it
    overlaps  inter = |mask_i & mask_j| > 0  and  inter * 2^20 >= tq * den,  den = a_i + a_j - inter ("iou") or min(a_i, a_j) ("iomin")
    tq        round(t * 2^20), halves up; t * 2^20 is exact in binary floating point, so 0.3 acts as 314573 / 2^20

The named cases are written as lists of positions k of the codec's column-major flattening (pixel y = k % H, x = k / H), shifted
so that, wherever the image has more than one word, the pixels straddle the boundary between words 0 and 1.  Every case fits the
15 pixels of a 5 x 3 image."""
import math

import numpy as np

Q = 1 << 20
SIZES = ((37, 53), (64, 64), (5, 3))   # (H, W): H * W = 1961 is no multiple of 64 and columns straddle words; whole words; one word


def quantise(thresh):
    assert 0.0 < thresh <= 1.0
    return int(math.floor(thresh * Q + 0.5))


def reference(masks, scores, labels, thresh, measure="iou", class_agnostic=False):
    """masks bool (D, H, W) -> keep uint8 (D,) in row order"""
    masks = np.asarray(masks).astype(bool)
    D = masks.shape[0]
    flat = masks.reshape(D, -1)
    area = [int(np.count_nonzero(flat[i])) for i in range(D)]
    labels = [int(v) for v in np.asarray(labels).reshape(-1)]
    order = np.argsort(-np.asarray(scores).reshape(-1), kind="stable")
    tq = quantise(thresh)
    assert measure in ("iou", "iomin")
    keep = np.zeros((D,), dtype=np.uint8)
    kept = []
    for j in order:
        j = int(j)
        dropped = False
        for i in kept:
            if not class_agnostic and labels[i] != labels[j]:
                continue
            inter = int(np.count_nonzero(flat[i] & flat[j]))
            den = area[i] + area[j] - inter if measure == "iou" else min(area[i], area[j])
            if inter > 0 and inter * Q >= tq * den:
                dropped = True
                break
        if not dropped:
            kept.append(j)
            keep[j] = 1
    return keep


def masks_from_positions(H, W, sets):
    """sets: per mask a list of column-major positions k -> bool (D, H, W)"""
    out = np.zeros((len(sets), H, W), dtype=bool)
    for d, ks in enumerate(sets):
        for k in ks:
            assert 0 <= k < H * W, (k, H, W)
            out[d, k % H, k // H] = True
    return out


def _base(H, W):
    return 60 if H * W >= 128 else 0   # positions 60 .. 74 straddle the boundary between words 0 and 1


def _case(H, W, sets, scores, labels, expect, thresh=0.5, measure="iou", class_agnostic=False, shift=True):
    b = _base(H, W) if shift else 0
    return dict(masks=masks_from_positions(H, W, [[b + k for k in ks] for ks in sets]), scores=np.asarray(scores, dtype=np.float32),
                labels=np.asarray(labels, dtype=np.int64), thresh=thresh, measure=measure, class_agnostic=class_agnostic,
                expect=np.asarray(expect, dtype=np.uint8))


def named_cases(H, W):
    """name -> dict(masks, scores, labels, thresh, measure, class_agnostic, expect): the keep flags written out by hand"""
    assert H >= 3 and W >= 3 and H * W >= 15
    r = range
    c = {}
    c["identical"] = _case(H, W, [r(0, 6), r(0, 6)], [0.9, 0.8], [1, 1], [1, 0])
    # A & B = 4 of a union of 8 (0.5), B & C alike, A & C = 2 of 10: A drops B, and B, dropped, does not drop C
    c["chain"] = _case(H, W, [r(0, 6), r(2, 8), r(4, 10)], [0.9, 0.8, 0.7], [1, 1, 1], [1, 0, 1])
    # the same chain met in another row order: the order is by score, the flags are by row
    c["chain_rows_permuted"] = _case(H, W, [r(4, 10), r(0, 6), r(2, 8)], [0.7, 0.9, 0.8], [1, 1, 1], [1, 1, 0])
    # rows 0 and 2 are one mask with one score: the lower row comes first
    c["equal_scores"] = _case(H, W, [r(0, 5), r(8, 12), r(0, 5)], [0.5, 0.9, 0.5], [1, 1, 1], [1, 1, 0])
    c["all_scores_equal"] = _case(H, W, [r(0, 5), r(0, 5), r(0, 5)], [0.5, 0.5, 0.5], [2, 2, 2], [1, 0, 0])
    c["different_labels"] = _case(H, W, [r(0, 6), r(0, 6)], [0.9, 0.8], [1, 2], [1, 1])
    c["different_labels_agnostic"] = _case(H, W, [r(0, 6), r(0, 6)], [0.9, 0.8], [1, 2], [1, 0], class_agnostic=True)
    # areas 3 and 3, intersection 2: 2 / 4 is the threshold itself (>= suppresses)
    c["exact_threshold"] = _case(H, W, [r(0, 3), r(1, 4)], [0.9, 0.8], [1, 1], [1, 0])
    # areas 4 and 4, intersection 2: 2 / 6
    c["just_below"] = _case(H, W, [r(0, 4), r(2, 6)], [0.9, 0.8], [1, 1], [1, 1])
    # 2 / 6 against 0.3 = 314573 / 2^20 and against 1 / 3 rounded to 349525 / 2^20 (just below 1 / 3: still suppressed)
    c["third_at_0.3"] = _case(H, W, [r(0, 4), r(2, 6)], [0.9, 0.8], [1, 1], [1, 0], thresh=0.3)
    c["third_at_a_third"] = _case(H, W, [r(0, 4), r(2, 6)], [0.9, 0.8], [1, 1], [1, 0], thresh=1.0 / 3.0)
    c["threshold_one"] = _case(H, W, [r(0, 4), r(0, 4), r(0, 3)], [0.9, 0.8, 0.7], [1, 1, 1], [1, 0, 1], thresh=1.0)
    # 2 pixels inside 8: 2 / 8 of the union, 2 / 2 of the smaller
    c["nested_iou"] = _case(H, W, [r(0, 8), r(2, 4)], [0.9, 0.8], [1, 1], [1, 1])
    c["nested_iomin"] = _case(H, W, [r(0, 8), r(2, 4)], [0.9, 0.8], [1, 1], [1, 0], measure="iomin")
    c["nested_iomin_small_first"] = _case(H, W, [r(0, 8), r(2, 4)], [0.8, 0.9], [1, 1], [0, 1], measure="iomin")
    # empty masks neither suppress nor are suppressed, wherever they stand in the order
    c["empty_among_full"] = _case(H, W, [[], r(0, 6), [], r(0, 6), []], [0.95, 0.9, 0.85, 0.8, 0.1], [1, 1, 1, 1, 1], [1, 1, 1, 0, 1])
    c["empty_among_full_iomin"] = _case(H, W, [[], r(0, 6), [], r(0, 6)], [0.95, 0.9, 0.85, 0.8], [1, 1, 1, 1], [1, 1, 1, 0],
                                        measure="iomin")
    # two diagonals of one 3 x 3 window: equal boxes, no common pixel
    d1, d2 = [0 * H + 0, 2 * H + 2], [0 * H + 2, 2 * H + 0]
    c["boxes_overlap_pixels_do_not"] = _case(H, W, [d1, d2], [0.9, 0.8], [1, 1], [1, 1], thresh=2.0 ** -20, shift=False)
    # the last pixels of the image: the last, partial word (the only word at 5 x 3)
    n = H * W
    c["last_partial_word"] = _case(H, W, [r(n - 3, n), r(n - 3, n), r(0, 3)], [0.9, 0.8, 0.7], [1, 1, 1], [1, 0, 1], shift=False)
    return c


def random_blobs(D, H, W, seed, n_labels=3):
    """D seeded ellipses around a few centres, so that many overlap; scores on a grid of 0.01, so that some tie; a few are empty
    -> (masks bool (D, H, W), scores float32, labels int64)"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    nc = max(D // 6, 1)
    cy, cx = g.uniform(0, H, nc), g.uniform(0, W, nc)
    masks = np.zeros((D, H, W), dtype=bool)
    for d in range(D):
        k = int(g.integers(nc))
        y0, x0 = cy[k] + g.normal(0, H / 40.0), cx[k] + g.normal(0, W / 40.0)
        ry, rx = g.uniform(H / 16.0, H / 6.0), g.uniform(W / 16.0, W / 6.0)
        if d % 29 != 7:   # (those rows stay empty)
            masks[d] = ((yy - y0) / ry) ** 2 + ((xx - x0) / rx) ** 2 <= 1.0
    scores = (g.integers(5, 100, D) / 100.0).astype(np.float32)
    labels = g.integers(1, n_labels + 1, D).astype(np.int64)
    return masks, scores, labels
