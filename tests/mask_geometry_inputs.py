"""Seeded inputs for the mask geometry kernels of csrc/masks.hip (the polygon rasteriser and the two paste forms), shared by
tests/test_mask_geometry_gpu.py (kernel vs oracle) and tests/test_mask_geometry_inputs.py (the inputs vs the oracle alone: every
class reaches inside its box, the comb is beyond the old crossing cap, the integral paste leaves out almost nothing).  Plain numpy
/ torch on the CPU.

Rasteriser classes, about 50 ROIs each, one to three polygons per ROI:
  a  a box below 1 px in width and / or height (the max(w, 1) path)
  b  boxes of 1-4 px
  c  a polygon 20-50 times the size of its box, whose boundary runs through the box
  d  a polygon centred hundreds of pixels away that reaches into the box
  e  integer boxes, vertices on multiples of 0.5 and 0.1 (the `+ .5` rounding ties of the x5 walk)
  f  every vertex repeated (zero-length edges) and collinear runs
  g  ordinary instances, boxes jittered by a few pixels, up to 200 vertices (more than one pass of 64 edges)
  h  ROIs that share instances of 1-3 overlapping polygons through `roi_poly`, in shuffled order, some with an empty range"""
import math

import numpy as np
import torch
import torch.nn.functional as F

CLASSES = "abcdefgh"
PER_CLASS = 50
RASTER_M = (14, 28, 32)
OLD_CAP = 1536           # crossings the rasteriser kept per polygon before it walked in passes

CANVAS = (128, 150)      # (IH, IW) of the paste cases
PASTE_M = (7, 14, 28)
PASTE_THRESH = 0.5
NEAR = 2e-6              # |fp64 bilinear value - thresh| below which the device sigmoid (a few 1e-7 off the host's) may decide
LEFT_OUT_CAP = 1e-4


# ------------------------------------------------------------------------------------------ rasteriser
def _blob(rng, cx, cy, rx, ry, nv, rough=0.4):
    """star polygon: nv vertices at sorted angles, radii in [1 - rough, 1] of (rx, ry) -> float64 (nv, 2)"""
    th = np.sort(rng.uniform(0, 2 * math.pi, nv))
    r = 1.0 - rough * rng.uniform(0, 1, nv)
    return np.stack([cx + rx * r * np.cos(th), cy + ry * r * np.sin(th)], 1)


def _inside(rng, box, n):
    """n overlapping blobs in the effective box (sides at least 1 px, as the crop scales them)"""
    x0, y0 = box[0], box[1]
    ew, eh = max(box[2] - box[0], 1.0), max(box[3] - box[1], 1.0)
    out = []
    for _ in range(n):
        cx, cy = x0 + ew * rng.uniform(0.35, 0.65), y0 + eh * rng.uniform(0.35, 0.65)
        out.append(_blob(rng, cx, cy, ew * rng.uniform(0.3, 0.5), eh * rng.uniform(0.3, 0.5), int(rng.randint(3, 24))))
    return out


def _class_a(rng, i):
    x0, y0 = rng.uniform(5, 900, 2)
    w, h = [(rng.uniform(0, 1), rng.uniform(0, 1)), (rng.uniform(0, 1), rng.uniform(1, 6)), (rng.uniform(1, 6), rng.uniform(0, 1)),
            (0.0, 0.0)][i % 4]
    box = [x0, y0, x0 + w, y0 + h]
    return box, _inside(rng, box, 1 + i % 3)


def _class_b(rng, i):
    x0, y0 = rng.uniform(5, 900, 2)
    box = [x0, y0, x0 + rng.uniform(1, 4), y0 + rng.uniform(1, 4)]
    return box, _inside(rng, box, 1 + i % 3)


def _class_c(rng, i):
    x0, y0 = rng.uniform(200, 800, 2)
    w, h = rng.uniform(5, 40, 2)
    box = [x0, y0, x0 + w, y0 + h]
    polys = []
    for _ in range(1 + i % 2):
        R = rng.uniform(20, 50) * max(w, h)
        nv = int(rng.randint(12, 40))
        a = rng.uniform(0, 2 * math.pi)
        # the box centre lies near the boundary: about the apothem away from the polygon's centre
        d = R * math.cos(math.pi / nv) + rng.uniform(-0.3, 0.3) * min(w, h)
        cx, cy = x0 + w / 2 + d * math.cos(a), y0 + h / 2 + d * math.sin(a)
        # regular nv-gon with the middle of one side turned towards the box
        th = a + math.pi + 2 * math.pi * (np.arange(nv) + 0.5) / nv
        polys.append(np.stack([cx + R * np.cos(th), cy + R * np.sin(th)], 1))
    return box, polys


def _class_d(rng, i):
    x0, y0 = rng.uniform(300, 700, 2)
    w, h = rng.uniform(8, 60, 2)
    box = [x0, y0, x0 + w, y0 + h]
    polys = []
    for _ in range(1 + i % 2):
        a = rng.uniform(0, 2 * math.pi)
        L = rng.uniform(400, 1200)            # a bar of length L from inside the box outwards: its centre is L / 2 away
        hw = rng.uniform(0.15, 0.4) * min(w, h)
        sx, sy = x0 + w * rng.uniform(0.3, 0.7), y0 + h * rng.uniform(0.3, 0.7)
        ux, uy = math.cos(a), math.sin(a)
        p = np.array([[sx - uy * hw, sy + ux * hw], [sx + uy * hw, sy - ux * hw],
                      [sx + uy * hw + ux * L, sy - ux * hw + uy * L], [sx - uy * hw + ux * L, sy + ux * hw + uy * L]])
        polys.append(p)
    return box, polys


def _class_e(rng, i):
    x0, y0 = np.floor(rng.uniform(5, 900, 2))
    w, h = rng.choice([7, 10, 14, 16, 20, 28, 32, 56], 2)
    box = [x0, y0, x0 + w, y0 + h]
    step = 0.5 if i % 2 == 0 else 0.1
    polys = [np.round(p / step) * step for p in _inside(rng, box, 1 + i % 3)]
    return box, polys


def _class_f(rng, i):
    x0, y0 = rng.uniform(5, 900, 2)
    w, h = rng.uniform(10, 80, 2)
    box = [x0, y0, x0 + w, y0 + h]
    polys = []
    for j, p in enumerate(_inside(rng, box, 1 + i % 3)):
        if (i + j) % 2 == 0:
            # an axis-aligned rectangle with several vertices along every side: exactly collinear runs
            lo, hi = p.min(0), p.max(0)
            t = np.linspace(0, 1, 5)[:-1, None]
            c = [np.array(lo), np.array([hi[0], lo[1]]), np.array(hi), np.array([lo[0], hi[1]])]
            p = np.concatenate([c[s] + t * (c[(s + 1) % 4] - c[s]) for s in range(4)], 0)
        else:
            # thirds of every edge (collinear up to fp32 rounding)
            nxt = np.roll(p, -1, 0)
            p = np.stack([p, p + (nxt - p) / 3, p + (nxt - p) * 2 / 3], 1).reshape(-1, 2)
        polys.append(np.repeat(p, 2, 0))   # every vertex twice
    return box, polys


def _instance(rng, n, nv_max):
    cx, cy = rng.uniform(100, 800, 2)
    rx, ry = rng.uniform(8, 90, 2)
    polys = []
    for _ in range(n):
        polys.append(_blob(rng, cx + rng.uniform(-0.4, 0.4) * rx, cy + rng.uniform(-0.4, 0.4) * ry,
                           rx * rng.uniform(0.5, 1), ry * rng.uniform(0.5, 1), int(rng.randint(3, nv_max)), rough=0.6))
    return polys


def _jittered_box(rng, polys, amp):
    a = np.concatenate(polys, 0)
    lo, hi = a.min(0), a.max(0)
    j = rng.uniform(-amp, amp, 4)
    return [lo[0] + j[0], lo[1] + j[1], hi[0] + j[2], hi[1] + j[3]]


def _class_g(rng, i):
    polys = _instance(rng, 1 + i % 3, 200 if i % 5 == 0 else 40)
    return _jittered_box(rng, polys, 3.0), polys


def raster_cases(seed=0):
    """-> dict: poly_xy float32 (V, 2) all vertices, poly_off int32 (NP + 1,), roi_poly int32 (P, 2), boxes float32 (P, 4),
    cls (P,) array of class letters"""
    rng = np.random.RandomState(seed)
    polys, ranges, boxes, cls = [], [], [], []

    def own(box, ps, c):
        ranges.append((len(polys), len(polys) + len(ps)))
        polys.extend(ps)
        boxes.append(box)
        cls.append(c)

    for c, fn in zip("abcdefg", (_class_a, _class_b, _class_c, _class_d, _class_e, _class_f, _class_g)):
        for i in range(PER_CLASS):
            box, ps = fn(rng, i)
            own(box, ps, c)
    # h: 16 instances laid down first, then ROIs that point into them in shuffled order; every fifth range is empty
    inst = []
    for i in range(16):
        ps = _instance(rng, 1 + i % 3, 40)
        inst.append((len(polys), len(polys) + len(ps), ps))
        polys.extend(ps)
    for i, k in enumerate(rng.permutation(PER_CLASS) % 16):
        s, e, ps = inst[k]
        if i % 5 == 4:
            s = e = int(rng.randint(0, len(polys) + 1))
        ranges.append((s, e))
        boxes.append(_jittered_box(rng, ps, 5.0))
        cls.append("h")
    order = rng.permutation(len(boxes))     # classes interleaved over the launch
    return {"poly_xy": np.concatenate(polys, 0).astype(np.float32),
            "poly_off": np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int32),
            "roi_poly": np.asarray(ranges, np.int32)[order], "boxes": np.asarray(boxes, np.float32)[order],
            "cls": np.asarray(cls)[order]}


def comb(edges=60, box=(100.0, 60.0, 156.0, 116.0)):
    """one ROI, one polygon: a zig-zag of `edges` edges that alternate between the box's left and right side (2 px beyond
    each) while y rises from the top of the box to its bottom; the last edge closes it.  Same dict as raster_cases()."""
    x0, y0, x1, y1 = box
    xy = np.stack([np.where(np.arange(edges) % 2 == 0, x0 - 2, x1 + 2), np.linspace(y0, y1, edges)], 1)
    return {"poly_xy": xy.astype(np.float32), "poly_off": np.asarray([0, edges], np.int32),
            "roi_poly": np.asarray([[0, 1]], np.int32), "boxes": np.asarray([box], np.float32), "cls": np.asarray(["comb"])}


def oracle_targets(cases, M):
    """oracle.model.project_masks_on_boxes over the cases -> float32 (P, M, M); a ROI with an empty range is all zero (the
    oracle, like the reference, is never asked for one: the mask head's non-positives)"""
    from oracle import model as om
    xy, off = torch.from_numpy(cases["poly_xy"]), cases["poly_off"]
    boxes = torch.from_numpy(cases["boxes"])
    out = torch.zeros((len(boxes), M, M), dtype=torch.float32)
    full = [p for p, (s, e) in enumerate(cases["roi_poly"]) if e > s]
    inst = [[xy[off[i]:off[i + 1]].reshape(-1).clone() for i in range(*cases["roi_poly"][p])] for p in full]
    if full:
        out[full] = om.project_masks_on_boxes(inst, boxes[full], M)
    return out.numpy()


def crossings(cases, M):
    """host restatement of the rasteriser's boundary walk (csrc/masks.hip, rleFrPoly): the column crossings a = x * M + y it
    records for every (ROI, polygon of its range) -> [(roi, polygon, int array)]"""
    f32 = np.float32
    xy, off = cases["poly_xy"], cases["poly_off"]
    out = []
    for p, (s, e) in enumerate(cases["roi_poly"]):
        b = cases["boxes"][p]
        bw, bh = b[2] - b[0], b[3] - b[1]
        bw = bw if bw >= 1 else f32(1)
        bh = bh if bh >= 1 else f32(1)
        rw, rh = f32(float(M) / float(bw)), f32(float(M) / float(bh))
        for pi in range(s, e):
            v = xy[off[pi]:off[pi + 1]]
            fx, fy = (v[:, 0] - b[0]) * rw, (v[:, 1] - b[1]) * rh                 # float32
            X = np.trunc(5.0 * fx.astype(np.float64) + .5).astype(np.int64)
            Y = np.trunc(5.0 * fy.astype(np.float64) + .5).astype(np.int64)
            found = [np.zeros(0, np.int64)]
            for j in range(len(v)):
                xs, ys, xe, ye = X[j], Y[j], X[(j + 1) % len(v)], Y[(j + 1) % len(v)]
                dx, dy = abs(xe - xs), abs(ys - ye)
                if dx == 0:
                    continue                                   # the column never changes
                flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
                if flip:
                    xs, xe, ys, ye = xe, xs, ye, ys
                t = np.arange(max(dx, dy) + 1, dtype=np.float64)
                if flip:
                    t = t[::-1]
                if dx >= dy:
                    u, w = t + xs, np.trunc(ys + (float(ye - ys) / dx) * t + .5)
                else:
                    u, w = np.trunc(xs + (float(xe - xs) / dy) * t + .5), t + ys
                ch = u[1:] != u[:-1]
                xd = np.where(u[1:] < u[:-1], u[1:], u[1:] - 1)[ch]
                xd = (xd + .5) / 5.0 - .5
                ok = (np.floor(xd) == xd) & (xd >= 0) & (xd <= M - 1)
                yd = np.ceil(np.clip((np.minimum(w[1:], w[:-1])[ch][ok] + .5) / 5.0 - .5, 0, M))
                found.append((xd[ok] * M + yd).astype(np.int64))
            out.append((p, pi, np.concatenate(found)))
    return out


def crossing_counts(cases, M):
    return [(p, pi, len(a)) for p, pi, a in crossings(cases, M)]


def parity_targets(cases, M):
    """the targets as the kernel forms them from crossings(): pixel q = x * M + y of a polygon is the parity of its crossings at or
    below q; a ROI is the union of its polygons -> float32 (P, M, M)"""
    out = np.zeros((len(cases["boxes"]), M * M), bool)
    for p, _, a in crossings(cases, M):
        out[p] |= (np.cumsum(np.bincount(a, minlength=M * M + 1)[:M * M]) % 2).astype(bool)
    return out.reshape(-1, M, M).transpose(0, 2, 1).astype(np.float32)


# ------------------------------------------------------------------------------------------ paste
def expanded_box(box, M):
    """the integer box a detection is pasted into (mask_head/inference.py:120-135: expand by (M + 2) / M in fp32, truncate)
    -> x0, y0, x1, y1 (inclusive)"""
    f32 = np.float32
    b = np.asarray(box, f32)
    scale = f32(float(M + 2) / M)
    wh, hh = (b[2] - b[0]) * f32(.5) * scale, (b[3] - b[1]) * f32(.5) * scale
    xc, yc = (b[2] + b[0]) * f32(.5), (b[3] + b[1]) * f32(.5)
    return tuple(int(np.trunc(v)) for v in (xc - wh, yc - hh, xc + wh, yc + hh))


def clipped_area(box, M, im_h, im_w):
    x0, y0, x1, y1 = expanded_box(box, M)
    return max(min(x1 + 1, im_w) - max(x0, 0), 0) * max(min(y1 + 1, im_h) - max(y0, 0), 0)


def _field(rng, M):
    """a smooth random field on (M, M), roughly N(0, 1): low-resolution noise resized"""
    k = max(2, M // 4)
    z = torch.from_numpy(rng.randn(1, 1, k, k))
    return F.interpolate(z, size=(M, M), mode="bicubic", align_corners=False)[0, 0].numpy()


def _boxes(rng, n, im_h, im_w):
    """fractional boxes from zero area to larger than the canvas, hanging over every border by up to about 10 px; all of them
    reach the canvas"""
    out = []
    for i in range(n):
        kind = i % 8
        if kind == 0:      # degenerate: zero width, zero height or both
            x0, y0 = rng.uniform(2, im_w - 3), rng.uniform(2, im_h - 3)
            w, h = [(0.0, rng.uniform(0, 30)), (rng.uniform(0, 30), 0.0), (0.0, 0.0)][(i // 8) % 3]
        elif kind == 1:    # larger than the canvas
            x0, y0 = rng.uniform(-10, 0), rng.uniform(-10, 0)
            w, h = im_w + rng.uniform(0, 20), im_h + rng.uniform(0, 20)
        elif kind == 2:    # over the left / top border
            w, h = rng.uniform(14, 60, 2)
            x0, y0 = rng.uniform(-10, 0), rng.uniform(-10, 0)
        elif kind == 3:    # over the right / bottom border
            w, h = rng.uniform(14, 60, 2)
            x0, y0 = im_w - w + rng.uniform(0, 10), im_h - h + rng.uniform(0, 10)
        elif kind == 4:    # tiny
            w, h = rng.uniform(0.1, 3, 2)
            x0, y0 = rng.uniform(0, im_w - 4), rng.uniform(0, im_h - 4)
        else:              # ordinary
            w, h = rng.uniform(8, 100, 2)
            x0, y0 = rng.uniform(-5, im_w - w + 5), rng.uniform(-5, im_h - h + 5)
        out.append([x0, y0, x0 + w, y0 + h])
    return np.asarray(out, np.float32)


def paste_cases(seed=0, per_m=67):
    """-> {M: (prob float32 (D, M, M) in [0, 1], boxes float32 (D, 4))} for M in PASTE_M, about 200 pairs in all"""
    rng = np.random.RandomState(1000 + seed)
    out = {}
    for M in PASTE_M:
        boxes = _boxes(rng, per_m, *CANVAS)
        assert all(clipped_area(b, M, *CANVAS) > 0 for b in boxes)
        prob = np.stack([1 / (1 + np.exp(-3 * _field(rng, M))) if i % 4 else rng.uniform(0, 1, (M, M)) for i in range(per_m)])
        out[M] = (prob.astype(np.float32), boxes)
    return out


def outside_boxes():
    """boxes that lie wholly outside the CANVAS (the oracle, like the reference, raises for them): beyond each border, by a
    fraction of a pixel and by a lot"""
    ih, iw = CANVAS
    return np.asarray([[-40.5, 10, -9.25, 50], [10, -60.25, 70, -12.5], [iw + 8.5, 10, iw + 40.0, 60], [20, ih + 7.5, 90, ih + 33.25],
                       [-300, -300, -200, -250], [iw + 200, ih + 100, iw + 260.5, ih + 140], [-8.5, -8.5, -2.5, -2.5],
                       [iw + 1.25, 40, iw + 7.25, 46], [40, ih + 1.25, 46, ih + 7.25]], np.float32)


def integral_case(M, seed=0, D=64, NC=3):
    """-> logits float32 (D, NC, M, M), labels int32 (D,) in {1, 2}, boxes float32 (D, 4), img int32 (D,) in {-1, 0, 1}:
    detections of two images in one fixed-capacity list, every fifth row behind its image's count (img = -1: no vote)"""
    rng = np.random.RandomState(2000 + seed + M)
    logits = np.stack([np.stack([4 * _field(rng, M) for _ in range(NC)]) for _ in range(D)]).astype(np.float32)
    labels = rng.randint(1, 3, D).astype(np.int32)
    img = rng.randint(0, 2, D).astype(np.int32)
    img[4::5] = -1
    return logits, labels, _boxes(rng, D, *CANVAS), img


def paste_values64(prob, box, im_h, im_w):
    """the paste of oracle.model.paste_mask (mask_head/inference.py:169-206) with the resize in fp64 and no threshold
    -> (values float64 (im_h, im_w), covered bool (im_h, im_w)): the bilinear value at every canvas pixel of the expanded box"""
    M = prob.shape[-1]
    x0, y0, x1, y1 = expanded_box(box, M)
    w, h = max(x1 - x0 + 1, 1), max(y1 - y0 + 1, 1)
    pm = torch.zeros((1, 1, M + 2, M + 2), dtype=torch.float64)
    pm[0, 0, 1:-1, 1:-1] = torch.as_tensor(prob, dtype=torch.float64)
    m = F.interpolate(pm, size=(h, w), mode="bilinear", align_corners=False)[0, 0].numpy()
    val = np.zeros((im_h, im_w))
    cov = np.zeros((im_h, im_w), bool)
    cx0, cx1, cy0, cy1 = max(x0, 0), min(x1 + 1, im_w), max(y0, 0), min(y1 + 1, im_h)
    if cx1 > cx0 and cy1 > cy0:
        val[cy0:cy1, cx0:cx1] = m[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0]
        cov[cy0:cy1, cx0:cx1] = True
    return val, cov


def integral_reference(logits, labels, boxes, img, n_img=2, thresh=PASTE_THRESH):
    """-> (want int32 (n_img, IH, IW): per image the sum of oracle pastes of sigmoid(logit of the label),
           left_out bool (n_img, IH, IW): pixels where some detection's fp64 bilinear value lies within NEAR of the threshold,
           pairs_left_out, pairs_covered: (detection, pixel) counts over the expanded boxes)"""
    from oracle import model as om
    ih, iw = CANVAS
    want = np.zeros((n_img, ih, iw), np.int32)
    left = np.zeros((n_img, ih, iw), bool)
    n_left = n_cov = 0
    lg = torch.from_numpy(logits)
    for d in range(len(labels)):
        if img[d] < 0:
            continue
        z = lg[d, int(labels[d])]
        want[img[d]] += om.paste_mask(z.sigmoid(), torch.from_numpy(boxes[d]), ih, iw, thresh).numpy().astype(np.int32)
        val, cov = paste_values64(z.double().sigmoid().numpy(), boxes[d], ih, iw)
        near = cov & (np.abs(val - thresh) < NEAR)
        left[img[d]] |= near
        n_left += int(near.sum())
        n_cov += int(cov.sum())
    return want, left, n_left, n_cov
