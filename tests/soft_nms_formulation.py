"""Soft-NMS as INTEGRATION.md ("Soft-NMS in the box head") defines it, in plain numpy loops: the expected values of
tests/test_soft_nms_gpu.py and tests/test_soft_nms_model_gpu.py.  Nothing here is the product's code.

`soft_nms` runs in the dtype it is given: float32 restates the kernel's arithmetic operation for operation (the linear method
is then compared by equality), float64 is the oracle the gaussian method is held against."""
import numpy as np

METHODS = ("linear", "gaussian")


def iou(a, b, dtype):
    """IoU of box a (4,) with boxes b (n, 4): the expression of csrc/nms.hip::iou_ge ("+1" areas), every operation in `dtype`"""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype).reshape(-1, 4)
    one, zero = dtype(1), dtype(0)
    aa = (a[2] - a[0] + one) * (a[3] - a[1] + one)
    ab = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    xx1, yy1 = np.fmax(a[0], b[:, 0]), np.fmax(a[1], b[:, 1])
    xx2, yy2 = np.fmin(a[2], b[:, 2]), np.fmin(a[3], b[:, 3])
    w, h = np.fmax(zero, xx2 - xx1 + one), np.fmax(zero, yy2 - yy1 + one)
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (aa + ab - inter)


def soft_nms(boxes, scores, method, thr, sigma, min_score, dtype=np.float32, gaps=None):
    """One pre-sorted segment.  -> (picked: positions in pick order, scores: every candidate's score when the loop stops).
    `gaps`: a list that receives, per pick, the relative gap between the best and the second-best current score."""
    assert method in METHODS
    dtype = np.dtype(dtype).type
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4).astype(dtype)
    s = np.asarray(scores, dtype=np.float32).astype(dtype).copy()
    thr, sigma, min_score, one = dtype(thr), dtype(sigma), dtype(min_score), dtype(1)
    alive = np.ones(len(s), dtype=bool)
    picked = []
    while alive.any():
        cand = np.flatnonzero(alive)
        i = int(cand[np.argmax(s[cand])])          # the first of equal scores: the smaller position
        if s[i] < min_score:
            break
        if gaps is not None and len(cand) > 1:
            second = np.sort(s[cand])[-2]
            gaps.append(float((s[i] - second) / s[i]))
        picked.append(i)
        alive[i] = False
        rest = np.flatnonzero(alive)
        if len(rest) == 0:
            break
        ov = iou(b[i], b[rest], dtype)
        if method == "linear":
            with np.errstate(invalid="ignore"):
                hit = ov >= thr                     # (False where ov is not a number)
            s[rest[hit]] = s[rest[hit]] * (one - ov[hit])
        else:
            ok = ov == ov
            s[rest[ok]] = s[rest[ok]] * np.exp(-(ov[ok] * ov[ok]) / sigma).astype(dtype)
    return np.asarray(picked, dtype=np.int32), s


def filter_results_soft(prob, dec, per, score_thresh, nms_thresh, detections_per_img, method, sigma, min_score, dtype=np.float32):
    """PostProcessor.filter_results with `soft_nms` in the place of the NMS.  prob (R, nc), dec (R, nc * 4), per = rows per
    image -> per image (boxes (n, 4) float32, scores (n,) `dtype`, labels (n,) int64)"""
    prob, dec = np.asarray(prob, dtype=np.float32), np.asarray(dec, dtype=np.float32)
    nc = prob.shape[1]
    out, lo = [], 0
    for R in per:
        pr, bx = prob[lo:lo + R], dec[lo:lo + R]
        lo += R
        bb, sc, lb = [], [], []
        for j in range(1, nc):
            rows = np.flatnonzero(pr[:, j] > np.float32(score_thresh))
            order = rows[np.argsort(-pr[rows, j], kind="stable")]
            picked, s = soft_nms(bx[order, 4 * j:4 * j + 4], pr[order, j], method, nms_thresh, sigma, min_score, dtype)
            pos = picked[np.argsort(order[picked], kind="stable")]      # ascending original row
            bb.append(bx[order[pos], 4 * j:4 * j + 4])
            sc.append(s[pos])
            lb.append(np.full(len(pos), j, dtype=np.int64))
        out.append((np.concatenate(bb), np.concatenate(sc), np.concatenate(lb)))
    return cut_detections(out, detections_per_img)


def cut_detections(results, detections_per_img):
    """the DETECTIONS_PER_IMG cut of filter_results on per-image (boxes, scores, labels): `score >= kthvalue(scores, n - D + 1)`,
    ties kept, list order kept; D <= 0 cuts nothing"""
    out = []
    for bb, sc, lb in results:
        n = len(sc)
        if n > detections_per_img > 0:
            kth = np.sort(sc)[n - detections_per_img]
            k = np.flatnonzero(sc >= kth)
            bb, sc, lb = bb[k], sc[k], lb[k]
        out.append((bb, sc, lb))
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs
def sort_stably(boxes, scores):
    order = np.argsort(-scores, kind="stable")
    return np.ascontiguousarray(boxes[order]), np.ascontiguousarray(scores[order])


def clustered(n, seed, size=1000.0):
    """n boxes around max(n // 10, 1) centres in a size x size image, centre jitter sigma = 8 px, sides 30-120 px, scores uniform
    in (0.05, 1), sorted stably by descending score -> boxes (n, 4) float32, scores (n,) float32"""
    rng = np.random.RandomState(seed)
    c = max(n // 10, 1)
    centres = rng.uniform(60.0, size - 60.0, size=(c, 2))
    sides = rng.uniform(30.0, 120.0, size=(c, 2))
    which = rng.randint(0, c, size=n)
    ctr = centres[which] + rng.normal(0.0, 8.0, size=(n, 2))
    wh = sides[which] * rng.uniform(0.9, 1.1, size=(n, 2))
    boxes = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).clip(0.0, size - 1.0).astype(np.float32)
    scores = rng.uniform(0.05, 1.0, size=n).astype(np.float32)
    return sort_stably(boxes, scores)


def chain(n):
    """a suppression chain: 101-px boxes 30 px apart, so that neighbours overlap at 71 / 131 = 0.54 and second neighbours at
    41 / 161 = 0.25; scores fall along the chain"""
    x = 30.0 * np.arange(n, dtype=np.float32)
    boxes = np.stack([x, np.full(n, 10, np.float32), x + 100, np.full(n, 110, np.float32)], 1).astype(np.float32)
    return boxes, np.linspace(0.95, 0.06, n).astype(np.float32) if n > 1 else np.full(n, 0.95, np.float32)


def all_equal(n):
    """the same box n times: the first pick decays every other score (to 0 when linear)"""
    return np.tile(np.asarray([[20, 30, 120, 90]], np.float32), (n, 1)), (np.linspace(0.9, 0.1, n).astype(np.float32) if n > 1
                                                                         else np.full(n, 0.9, np.float32))


def disjoint(n):
    """a grid of boxes that do not touch: nothing decays"""
    i = np.arange(n, dtype=np.float32)
    x, y = (i % 64) * 15, (i // 64) * 15
    return np.stack([x, y, x + 9, y + 9], 1).astype(np.float32), (np.linspace(0.99, 0.06, n).astype(np.float32) if n > 1
                                                                   else np.full(n, 0.99, np.float32))


def equal_scores(n, seed):
    """the clustered boxes with one score throughout: ties go by position until the decays tell them apart"""
    return clustered(n, seed)[0], np.full(n, 0.5, np.float32)


KINDS = {"clustered": lambda n: clustered(n, seed=n), "chain": chain, "all-equal": all_equal, "disjoint": disjoint,
         "equal-scores": lambda n: equal_scores(n, seed=n + 7)}


def rel_dev(a, b):
    """largest relative deviation of a from b (b the reference, nowhere 0)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b))) if len(b) else 0.0


GAUSS = dict(thr=0.5, sigma=0.5, min_score=0.001)
GAUSS_INPUTS = [(64, 0), (64, 1), (64, 2), (33, 3), (1, 4)]     # (n, seed) of the gaussian GPU test


def gaussian_tolerance():
    """4 x the largest relative deviation of the float32 restatement from the float64 oracle on GAUSS_INPUTS: the factor is for
    an expf and a division that may each round differently from numpy's"""
    worst = 0.0
    for n, seed in GAUSS_INPUTS:
        b, s = clustered(n, seed)
        p64, s64 = soft_nms(b, s, "gaussian", dtype=np.float64, **GAUSS)
        p32, s32 = soft_nms(b, s, "gaussian", dtype=np.float32, **GAUSS)
        assert p32.tolist() == p64.tolist()
        worst = max(worst, rel_dev(s32, s64))
    return 4.0 * worst
