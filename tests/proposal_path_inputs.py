"""Constructed inputs and plain references for the kernels between the RPN and the heads: ROIAlign (csrc/roi_align.hip), the
target matcher, box decode and the level mapper (csrc/targets.hip), and the two detection losses (csrc/losses.hip).  numpy on
the CPU, nothing from the product.

ROIAlign: the geometry (scaled ROI, bin size, grid counts, sample coordinates, the emptiness test, the clamps and the four
weights) is computed in numpy.float32 in the expression order of `roi_bin`, so the reference and the kernel take the same side
of every boundary; the accumulation is float64, and every function also returns the sum of the absolute values of the terms it
added (S_abs), which the tolerances are derived from.  Everything else is a float64 formulation of the tensor code.

tests/test_proposal_path_inputs.py checks on the CPU that every builder reaches the edge it names and that the references
agree with the CPU oracle and the fp32 tensor modules; tests/test_proposal_path_edges_gpu.py runs the kernels on the same
inputs."""
import functools
import math

import numpy as np

f32 = np.float32
U = 2.0 ** -24   # unit roundoff of fp32


def ro(a):
    a.setflags(write=False)
    return a


# ============================================================================================================== ROIAlign
ROI_LEVELS = ((9, 11, 0.5), (5, 6, 0.25))   # (H, W, scale): no multiple of the 8-pixel tile; 2 x 2 tiles and one partial tile
ROI_N = 2
ROI_CS = (4, 6, 64, 260)
ROI_POOLS = ((1, 1), (2, 3), (7, 7))
ROI_SRS = (0, 1, 2, 3)


def axis_taps(start, size, P, p, sr, L):
    """the samples of bin p along one axis of length L, in fp32 in the order of `roi_bin` / `bilin`
    -> grid count g, then per sample: coordinate, empty, low index, high index, low weight h, high weight l"""
    start, size = f32(start), f32(size)
    b = size / f32(P)
    g = sr if sr > 0 else int(math.ceil(size / f32(P)))
    out = []
    for i in range(g):
        v = start + f32(p) * b + f32(i + 0.5) * b / f32(g)
        coord = v
        if v < f32(-1.0) or v > f32(L):
            out.append((coord, True, 0, 0, f32(0), f32(0)))
            continue
        if v <= 0:
            v = f32(0)
        lo = int(v)
        if lo >= L - 1:
            hi = lo = L - 1
            v = f32(lo)
        else:
            hi = lo + 1
        l = v - f32(lo)
        h = f32(1) - l
        out.append((coord, False, lo, hi, h, l))
    return g, out


def roi_extent(roi, scale):
    """-> rsw, rsh, rw, rh in fp32 (sizes clamp to 1)"""
    s = f32(scale)
    rsw, rsh, rew, reh = f32(roi[1]) * s, f32(roi[2]) * s, f32(roi[3]) * s, f32(roi[4]) * s
    return rsw, rsh, max(rew - rsw, f32(1)), max(reh - rsh, f32(1))


def roi_samples(roi, scale, PH, PW, sr, H, W):
    """every sample coordinate of an ROI per axis -> (ys, y_empty, xs, x_empty) fp32 / bool arrays over (bin, sample)"""
    rsw, rsh, rw, rh = roi_extent(roi, scale)
    ys = [t for p in range(PH) for t in axis_taps(rsh, rh, PH, p, sr, H)[1]]
    xs = [t for p in range(PW) for t in axis_taps(rsw, rw, PW, p, sr, W)[1]]
    return (np.asarray([t[0] for t in ys], f32), np.asarray([t[1] for t in ys], bool),
            np.asarray([t[0] for t in xs], f32), np.asarray([t[1] for t in xs], bool))


def _bin_taps(ty, tx):
    """one bin's product grid -> valid [gh, gw], the four index pairs and the four fp32 weights (hy * hx, hy * lx, ly * hx, ly * lx)"""
    ey = np.asarray([t[1] for t in ty], bool)
    ex = np.asarray([t[1] for t in tx], bool)
    yl, yh = np.asarray([t[2] for t in ty]), np.asarray([t[3] for t in ty])
    xl, xh = np.asarray([t[2] for t in tx]), np.asarray([t[3] for t in tx])
    hy, ly = np.asarray([t[4] for t in ty], f32), np.asarray([t[5] for t in ty], f32)
    hx, lx = np.asarray([t[4] for t in tx], f32), np.asarray([t[5] for t in tx], f32)
    valid = ~ey[:, None] & ~ex[None, :]
    ws = (hy[:, None] * hx[None, :], hy[:, None] * lx[None, :], ly[:, None] * hx[None, :], ly[:, None] * lx[None, :])
    assert all(w.dtype == f32 for w in ws)
    idx = ((yl, xl), (yl, xh), (yh, xl), (yh, xh))
    return valid, idx, ws


def roi_align_reference(feat, rois, scale, PH, PW, sr):
    """feat [N, C, H, W], rois [K, 5] = (image, x1, y1, x2, y2) -> out [K, C, PH, PW] float64, S_abs like out (the sum of
    |weight * texel| over the samples that were added), grid [K, 2] = (gh, gw).  An empty sample adds nothing and reads nothing."""
    feat = np.asarray(feat)
    N, C, H, W = feat.shape
    f64 = feat.astype(np.float64)
    K = len(rois)
    out, sabs, grid = np.zeros((K, C, PH, PW)), np.zeros((K, C, PH, PW)), np.zeros((K, 2), np.int64)
    for k in range(K):
        b = int(rois[k][0])
        rsw, rsh, rw, rh = roi_extent(rois[k], scale)
        ytaps = [axis_taps(rsh, rh, PH, p, sr, H) for p in range(PH)]
        xtaps = [axis_taps(rsw, rw, PW, p, sr, W) for p in range(PW)]
        gh, gw = ytaps[0][0], xtaps[0][0]
        grid[k] = gh, gw
        count = float(gh * gw)
        for ph in range(PH):
            for pw in range(PW):
                valid, idx, ws = _bin_taps(ytaps[ph][1], xtaps[pw][1])
                acc, ab = np.zeros(C), np.zeros(C)
                for (iy, ix), w in zip(idx, ws):
                    t = f64[b][:, iy[:, None], ix[None, :]] * w.astype(np.float64)[None]     # [C, gh, gw]
                    t = t[:, valid]
                    acc += t.sum(1)
                    ab += np.abs(t).sum(1)
                out[k, :, ph, pw] = acc / count
                sabs[k, :, ph, pw] = ab
    return out, sabs, grid


def roi_align_backward_reference(gout, rois, scale, PH, PW, sr, shape):
    """gout [K, C, PH, PW] -> grad [N, C, H, W] float64, S_abs like grad, T [N, H, W] = the number of non-zero-weight
    contributions a texel received (per channel)"""
    gout = np.asarray(gout, np.float64)
    N, C, H, W = shape
    grad, sabs, T = np.zeros(shape), np.zeros(shape), np.zeros((N, H, W), np.int64)
    for k in range(len(rois)):
        b = int(rois[k][0])
        rsw, rsh, rw, rh = roi_extent(rois[k], scale)
        ytaps = [axis_taps(rsh, rh, PH, p, sr, H) for p in range(PH)]
        xtaps = [axis_taps(rsw, rw, PW, p, sr, W) for p in range(PW)]
        count = float(ytaps[0][0] * xtaps[0][0])
        for ph in range(PH):
            for pw in range(PW):
                valid, idx, ws = _bin_taps(ytaps[ph][1], xtaps[pw][1])
                g = gout[k, :, ph, pw]
                for (iy, ix), w in zip(idx, ws):
                    Y, X = np.broadcast_arrays(iy[:, None], ix[None, :])
                    Y, X, wv = Y[valid], X[valid], w[valid].astype(np.float64)
                    t = g[:, None] * wv[None, :] / count
                    np.add.at(grad[b], (slice(None), Y, X), t)
                    np.add.at(sabs[b], (slice(None), Y, X), np.abs(t))
                    np.add.at(T[b], (Y, X), (wv != 0).astype(np.int64))
    return grad, sabs, T


def roi_forward_bound(sabs, grid):
    """(8 gh gw + 2) u S_abs / count per element: one rounding per product and per add of the kernel's chain, and the division"""
    cnt = (grid[:, 0] * grid[:, 1]).astype(np.float64)[:, None, None, None]
    return (8.0 * cnt + 2.0) * U * sabs / cnt


def roi_backward_bound(sabs, T):
    """(T + 3) u S_abs per texel: the order of the additions is free, so the bound is on the sum of magnitudes"""
    return (T[:, None].astype(np.float64) + 3.0) * U * sabs


def roi_features(C, seed=0):
    """one [N, C, H, W] fp32 map per level"""
    rng = np.random.RandomState(1000 * seed + C)
    return [ro(rng.standard_normal((ROI_N, C, H, W)).astype(f32)) for H, W, _ in ROI_LEVELS]


def _step_until(roi, j, direction, pred):
    """the ROI with coordinate j moved in `direction` by the smallest amount for which pred(roi) holds: bisection down to two
    neighbouring fp32 values, the nearer one without and the farther one with the property"""
    lo, hi = np.array(roi, f32), np.array(roi, f32)
    hi[j] = lo[j] + f32(direction)
    assert not pred(lo) and pred(hi)
    while True:
        mid = lo.copy()
        mid[j] = f32((np.float64(lo[j]) + np.float64(hi[j])) / 2)
        if mid[j] == lo[j] or mid[j] == hi[j]:
            return hi
        if pred(mid):
            hi = mid
        else:
            lo = mid


def _edge_roi(PH, PW, sr, lvl, axis, edge):
    """an ROI (in image coordinates) whose first sample along `axis` (0 = y, 1 = x) lies at exactly -1.0 (edge "lo"), or whose
    last sample lies at exactly the map's size (edge "hi").  Bin size 2 sr with sr samples (adaptive: bin size 2, 2 samples):
    consecutive samples are 2 (1) apart and the first one lies 1 (0.5) behind the ROI's start -- all exact in fp32."""
    H, W, s = ROI_LEVELS[lvl]
    L, P = (H, PH) if axis == 0 else (W, PW)
    b, first = (2.0 * sr, 1.0) if sr > 0 else (2.0, 0.5)
    step = 2.0 if sr > 0 else 1.0
    g = sr if sr > 0 else 2
    if edge == "lo":
        start = -1.0 - first
    else:
        start = L - ((P - 1) * b + first + (g - 1) * step)
    lo, hi = start / s, (start + b * P) / s
    other = (1.0 / s, 3.5 / s)   # well inside along the other axis
    return (other[0], lo, other[1], hi) if axis == 0 else (lo, other[0], hi, other[1])


def roi_list(PH, PW, sr):
    """-> names, rois [K, 5] fp32, levels [K] int32: every named ROI on image 0 and on image 1, the level alternating.  The
    boundary ROIs depend on the pooling parameters (their samples must land exactly on -1, H and W)."""
    names, rois, levels = [], [], []

    def add(name, img, lvl, box):
        names.append("%s/i%d/l%d" % (name, img, lvl))
        rois.append([float(img)] + [float(f32(v)) for v in box])
        levels.append(lvl)

    def in_map(lvl, x1, y1, x2, y2):   # level-0 map coordinates -> image coordinates of the ROI at `lvl` (same relative place)
        H, W, s = ROI_LEVELS[lvl]
        fy, fx = H / 9.0, W / 11.0
        return (x1 * fx / s, y1 * fy / s, x2 * fx / s, y2 * fy / s)

    plain = [("inside", (2.25, 1.5, 7.75, 6.0)),
             ("zero_size", (3.5, 4.25, 3.5, 4.25)),                 # x2 == x1 and y2 == y1: the size clamps to 1
             ("inverted", (6.0, 2.0, 3.0, 5.0)),                    # x2 < x1
             ("sub_pixel", (4.125, 3.25, 4.375, 3.3125)),
             ("left_of_map", (-30.0, 2.0, -5.0, 6.0)),              # every sample empty along x
             ("above_map", (2.0, -30.0, 6.0, -5.0)),                # every sample empty along y
             ("beyond_far_corner", (40.0, 40.0, 60.0, 60.0)),       # every sample empty
             ("straddles_top_left", (-6.0, -5.0, 4.0, 3.0)),        # some samples empty, some clamped, some plain
             ("last_row_and_column", None),
             ("tile_seam", (7.25, 7.25, 9.5, 8.75)),                # starts in row / column 7: the last one of tile 0
             ("ends_before_seam", (1.0, 3.0, 7.9375, 7.9375)),      # ends in row / column 7, its last samples reach into 8
             ("wide_400", None)]
    n = 0
    for name, box in plain:
        for img in range(ROI_N):
            lvl = (n + img) % 2
            if name == "wide_400":   # 400 pixels wide, covers the whole map
                add(name, img, lvl, (-180.0, -4.0, 220.0, 44.0))
            elif name == "last_row_and_column":   # one pixel in size (a smaller one clamps to 1 and leaves the map)
                H, W, s = ROI_LEVELS[lvl]
                add(name, img, lvl, ((W - 1) / s, (H - 1) / s, W / s, H / s))
            else:
                add(name, img, lvl, in_map(lvl, *box))
        n += 1
    for axis, edge, tag in ((0, "lo", "y_at_minus_1"), (1, "lo", "x_at_minus_1"), (0, "hi", "y_at_H"), (1, "hi", "x_at_W")):
        for img in range(ROI_N):
            lvl = (n + img) % 2
            H, W, s = ROI_LEVELS[lvl]
            box = _edge_roi(PH, PW, sr, lvl, axis, edge)
            add(tag, img, lvl, box)
            j = 2 if axis == 0 else 1     # move the ROI's start (y1 or x1): every sample moves with it, the grid stays
            on = np.array([float(img)] + list(box), f32)

            def beyond(r, axis=axis, edge=edge, s=s, H=H, W=W):
                ys, ye, xs, xe = roi_samples(r, s, PH, PW, sr, H, W)
                e = ye if axis == 0 else xe
                return bool(e[0] if edge == "lo" else e[-1])
            tw = _step_until(on, j, -1 if edge == "lo" else 1, beyond)
            add(tag + "_beyond", img, lvl, tw[1:])
        n += 1
    for rep in range(3):   # the same ROI four times: colliding atomics and tile sums
        names.append("inside_again%d/i0/l0" % rep)
        rois.append(list(rois[0]))
        levels.append(levels[0])
    return names, ro(np.asarray(rois, f32)), ro(np.asarray(levels, np.int32))


def roi_many(K=300):
    """K copies and near-copies of one ROI on image 1, level 0 (the tile kernel's ROI list loop takes a second pass over k)"""
    rng = np.random.RandomState(7)
    base = np.asarray([1.0, 3.0, 2.0, 15.0, 13.0], f32)
    rois = np.tile(base, (K, 1))
    jit = (rng.randint(-8, 9, size=(K, 4)) / 8.0).astype(f32)
    jit[::3] = 0          # every third one is an exact copy
    rois[:, 1:] += jit
    return ro(rois.astype(f32)), ro(np.zeros(K, np.int32))


def roi_gout(K, C, PH, PW, seed=3):
    return ro(np.random.RandomState(seed + K + C).standard_normal((K, C, PH, PW)).astype(f32))


def bf16_round(a):
    """fp32 -> the nearest bf16 (ties to even), as fp32"""
    u = np.asarray(a, f32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(f32)


@functools.lru_cache(maxsize=None)
def roi_forward_case(C, PH, PW, sr, bf16=False, many=False):
    """-> feats, rois, levels, names, then per level the ROI indices, reference, S_abs and grid (computed once, read-only)"""
    feats = roi_features(C)
    if bf16:
        feats = [ro(bf16_round(f)) for f in feats]
    if many:
        rois, levels = roi_many()
        names = ["copy%d" % i for i in range(len(rois))]
    else:
        names, rois, levels = roi_list(PH, PW, sr)
    per = []
    for l, (H, W, s) in enumerate(ROI_LEVELS):
        idx = np.nonzero(levels == l)[0]
        out, sabs, grid = roi_align_reference(feats[l], rois[idx], s, PH, PW, sr)
        per.append((idx, ro(out), ro(sabs), ro(grid)))
    return feats, rois, levels, names, per


@functools.lru_cache(maxsize=None)
def roi_backward_case(C, PH, PW, sr, many=False):
    """-> gout, rois, levels, then per level the reference gradient, S_abs and T"""
    if many:
        rois, levels = roi_many()
    else:
        _, rois, levels = roi_list(PH, PW, sr)
    gout = roi_gout(len(rois), C, PH, PW)
    per = []
    for l, (H, W, s) in enumerate(ROI_LEVELS):
        idx = np.nonzero(levels == l)[0]
        g, sabs, T = roi_align_backward_reference(gout[idx], rois[idx], s, PH, PW, sr, (ROI_N, C, H, W))
        per.append((ro(g), ro(sabs), ro(T)))
    return gout, rois, levels, per


def roi_shapes(C):
    return [(ROI_N, C, H, W) for H, W, _ in ROI_LEVELS]


ROI_SCALES = [s for _, _, s in ROI_LEVELS]


# ======================================================================================================= IoU, Matcher, coder
def iou64(gt, cand):
    """[G, 4] x [A, 4] -> [G, A] float64, "+1" convention: inter / (area_g + area_c - inter)"""
    g, c = np.asarray(gt, np.float64).reshape(-1, 4), np.asarray(cand, np.float64).reshape(-1, 4)
    ag = (g[:, 2] - g[:, 0] + 1) * (g[:, 3] - g[:, 1] + 1)
    ac = (c[:, 2] - c[:, 0] + 1) * (c[:, 3] - c[:, 1] + 1)
    w = np.maximum(np.minimum(g[:, None, 2], c[None, :, 2]) - np.maximum(g[:, None, 0], c[None, :, 0]) + 1, 0)
    h = np.maximum(np.minimum(g[:, None, 3], c[None, :, 3]) - np.maximum(g[:, None, 1], c[None, :, 1]) + 1, 0)
    inter = w * h
    return inter / (ag[:, None] + ac[None, :] - inter)


def matcher64(q, high, low, allow_low_quality):
    """the Matcher's rules on a [G, A] quality matrix, plain loops: first maximal ground truth; -1 below `low`, -2 in
    [low, high); with allow_low_quality every candidate that is some ground truth's (tied) best keeps its arg-max.
    G == 0 (the library's contract for an image without ground truth): everything is -1."""
    G, A = q.shape
    out = np.full(A, -1, np.int64)
    if G == 0:
        return out
    top = [max(q[g]) if A else 0.0 for g in range(G)]
    for a in range(A):
        best, arg = -1.0, 0
        for g in range(G):
            if q[g, a] > best:
                best, arg = q[g, a], g
        m = arg
        if best < low:
            m = -1
        elif best < high:
            m = -2
        if allow_low_quality and any(q[g, a] == top[g] for g in range(G)):
            m = arg
        out[a] = m
    return out


def encode64(gt, cand, weights):
    """BoxCoder.encode in float64: [A, 4] matched boxes, [A, 4] candidates"""
    g, c = np.asarray(gt, np.float64), np.asarray(cand, np.float64)
    pw, ph = c[:, 2] - c[:, 0] + 1, c[:, 3] - c[:, 1] + 1
    px, py = c[:, 0] + 0.5 * pw, c[:, 1] + 0.5 * ph
    gw, gh = g[:, 2] - g[:, 0] + 1, g[:, 3] - g[:, 1] + 1
    gx, gy = g[:, 0] + 0.5 * gw, g[:, 1] + 0.5 * gh
    wx, wy, ww, wh = weights
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([wx * (gx - px) / pw, wy * (gy - py) / ph, ww * np.log(gw / pw), wh * np.log(gh / ph)], 1)


def decode64(codes, boxes, weights, clip, row_off=None, lim=None):
    """BoxCoder.decode in float64 (+ clip_to_image per image when row_off / lim are given): codes [R, 4 ncls], boxes [R, 4]"""
    c, b = np.asarray(codes, np.float64), np.asarray(boxes, np.float64)
    w, h = (b[:, 2] - b[:, 0] + 1)[:, None], (b[:, 3] - b[:, 1] + 1)[:, None]
    cx, cy = b[:, 0, None] + 0.5 * w, b[:, 1, None] + 0.5 * h
    wx, wy, ww, wh = weights
    dx, dy = c[:, 0::4] / wx, c[:, 1::4] / wy
    dw, dh = np.minimum(c[:, 2::4] / ww, clip), np.minimum(c[:, 3::4] / wh, clip)
    pcx, pcy = dx * w + cx, dy * h + cy
    pw, ph = np.exp(dw) * w, np.exp(dh) * h
    out = np.zeros_like(c)
    out[:, 0::4], out[:, 1::4] = pcx - 0.5 * pw, pcy - 0.5 * ph
    out[:, 2::4], out[:, 3::4] = pcx + 0.5 * pw - 1, pcy + 0.5 * ph - 1
    if lim is not None:
        for i in range(len(lim)):
            a, e = int(row_off[i]), int(row_off[i + 1])
            l4 = np.tile(np.asarray([lim[i][0], lim[i][1]] * 2, np.float64), c.shape[1] // 4)
            out[a:e] = np.minimum(np.maximum(out[a:e], 0.0), l4)
    return out


MATCH_THRESHOLDS = ((0.5, 0.5), (0.7, 0.3))
MATCH_CAND_COUNTS = (3, 0, 300, 5)
MATCH_GT_COUNTS = (2, 1, 4, 0)
MATCH_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
G_DOUBLE, G_COVERED, G_UNCOVERED = (10, 10, 29, 29), (100, 100, 119, 139), (400, 400, 420, 420)
# image 2's constructed candidates (index: meaning)
C_HALF, C_07, C_03, C_EQUAL, C_AREA0, C_TWIN = 0, 1, 2, 3, 4, 5


def match_inputs():
    """-> cands (per image [n, 4] fp32), gts (per image [g, 4] fp32), gt labels (per image int64); integer coordinates, so every
    IoU is an exact rational.
    image 0: three candidates at IoU 0.5, 0.3 and 0.7 to its two boxes (a real low-quality restore: the 0.3 one is the second
             box's best)
    image 1: one ground-truth box, no candidate
    image 2: two identical boxes, a box equal to a candidate, a box nothing overlaps; candidates at IoU exactly 0.5, 0.7, 0.3,
             1, an area-0 box (x2 == x1 - 1), a repeated candidate, and 294 more on a 200-pixel field
    image 3: five candidates, no ground truth"""
    gts = [np.asarray([(0, 0, 9, 9), (20, 0, 29, 9)], f32), np.asarray([(0, 0, 9, 9)], f32),
           np.asarray([G_DOUBLE, G_DOUBLE, G_COVERED, G_UNCOVERED], f32), np.zeros((0, 4), f32)]
    labels = [np.asarray([1, 2], np.int64), np.asarray([3], np.int64), np.asarray([1, 2, 3, 1], np.int64), np.zeros(0, np.int64)]
    c0 = np.asarray([(0, 0, 9, 4), (20, 0, 29, 2), (0, 0, 9, 6)], f32)
    special = [(10, 10, 29, 19),     # 200 of 400 pixels of the doubled box: IoU 0.5
               (10, 10, 29, 23),     # 280 of 400: 0.7
               (10, 10, 29, 15),     # 120 of 400: 0.3
               G_COVERED,            # IoU 1
               (15, 15, 14, 20),     # x2 == x1 - 1: area 0
               (10, 10, 29, 23)]     # the 0.7 candidate again
    rng = np.random.RandomState(11)
    xy = rng.randint(0, 200, size=(294, 2))
    wh = rng.randint(1, 60, size=(294, 2))
    c2 = np.concatenate([np.asarray(special, f32), np.concatenate([xy, xy + wh], 1).astype(f32)], 0)
    c3 = np.asarray([(0, 0, 9, 9), (5, 5, 30, 40), (100, 100, 119, 139), (7, 7, 6, 9), (300, 2, 310, 8)], f32)
    cands = [c0, np.zeros((0, 4), f32), c2, c3]
    assert tuple(len(c) for c in cands) == MATCH_CAND_COUNTS and tuple(len(g) for g in gts) == MATCH_GT_COUNTS
    return [ro(c) for c in cands], [ro(g) for g in gts], [ro(l) for l in labels]


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def match_expected(cands, gts, labels, high, low, lowq, weights, visible=None):
    """per image: matches, RPN labels (1 matched, 0 background, -1 between / not visible), box labels (class, 0 background, -1
    between), regression targets (encode of the matched box, box 0 for the unmatched; zeros where the image has no ground truth)"""
    out = []
    for c, g, gl in zip(cands, gts, labels):
        m = matcher64(iou64(g, c), high, low, lowq)
        lf = (m >= 0).astype(np.float64)
        if visible is not None:
            lf[~np.asarray(visible, bool)[:len(c)]] = -1.0
        lf[m == -2] = -1.0
        if len(g):
            li = gl[np.maximum(m, 0)].copy()
            li[m == -1], li[m == -2] = 0, -1
            reg = encode64(g[np.maximum(m, 0)], c, weights)
        else:
            li, reg = np.zeros(len(c), np.int64), np.zeros((len(c), 4))
        out.append((m, lf, li, reg))
    return out


# ENCODE_REL: the largest relative error of the fp32 tensor formulation of BoxCoder.encode (CPU) against encode64 on the matcher
# inputs, measured by tests/test_proposal_path_inputs.py::test_encode_fp32_margin, which asserts that it does not exceed this
# figure; the kernel is allowed twice as much (logf of another math library).  Zero targets are exact.
ENCODE_REL = 2.28e-6


def rel_err(got, ref):
    """max |got - ref| / |ref| over ref != 0; where ref == 0, got must be 0 (returns inf otherwise)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    z = ref == 0
    if (got[z] != 0).any():
        return np.inf
    return float((np.abs(got[~z] - ref[~z]) / np.abs(ref[~z])).max()) if (~z).any() else 0.0


# ============================================================================================================ level mapper
LEVEL_S0, LEVEL_LVL0, LEVEL_EPS, LEVEL_KMIN, LEVEL_KMAX = 224.0, 4.0, 1e-6, 2, 5


def level_boxes():
    """-> names, boxes [n, 4] fp32.  sqrt(area) exactly 56 .. 896 (sqrt(area) / s0 a power of two: log2 is an integer and the
    floor sits on it), each with the integer box of the next smaller area; boxes a few fp32 steps BELOW such a square, where
    sqrt(area) / s0 + eps is back on the upper side (eps decides the level); 1 x 1, area 0, and a 4000-pixel box."""
    names, boxes = [], []
    for s in (56, 112, 224, 448, 896):
        names.append("sqrt_area_%d" % s)
        boxes.append((3.0, 5.0, 3.0 + s - 1, 5.0 + s - 1))
        names.append("below_%d" % s)
        boxes.append((3.0, 5.0, 3.0 + s - 1, 5.0 + s - 2))
    for s in (112, 224):
        # s (1 - 4 * 2^-23): sqrt(area) / s0 lies 4.8e-7 (relative) below 2^k, eps = 1e-6 is 2e-6 / 1e-6 of it: above sqrtf's
        # rounding, and large enough that lvl0 + log2(.) without eps does not round back up to the integer
        side = f32(s) * (f32(1) - f32(4 * 2.0 ** -23))
        names.append("eps_decides_%d" % s)
        boxes.append((0.0, 0.0, float(side - f32(1)), float(side - f32(1))))
    names += ["one_pixel", "area_0", "clamp_4000"]
    boxes += [(7.0, 9.0, 7.0, 9.0), (7.0, 9.0, 6.0, 20.0), (0.0, 0.0, 3999.0, 3999.0)]
    return names, ro(np.asarray(boxes, f32))


def level_ref(boxes, dtype=np.float64, eps=LEVEL_EPS):
    """floor(lvl0 + log2(sqrt(area) / s0 + eps)) clamped to [k_min, k_max], minus k_min, evaluated in `dtype`"""
    b = np.asarray(boxes).astype(dtype)
    one = dtype(1)
    area = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    with np.errstate(divide="ignore"):
        lv = np.floor(dtype(LEVEL_LVL0) + np.log2(np.sqrt(area) / dtype(LEVEL_S0) + dtype(eps)))
    return (np.clip(lv, LEVEL_KMIN, LEVEL_KMAX) - LEVEL_KMIN).astype(np.int64)


# ============================================================================================================== box decode
DECODE_CLIP = math.log(1000.0 / 16)
DECODE_WEIGHTS = ((1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0))


def code_for(target, w):
    """an fp32 code with fl32(code / w) == target exactly"""
    target, w = f32(target), f32(w)
    c = target * w
    for _ in range(8):
        q = c / w
        if q == target:
            return c
        c = np.nextafter(c, f32(np.inf) if q < target else f32(-np.inf))
    raise AssertionError("no fp32 code divides to the target")


def decode_inputs(R, ncls, weights):
    """-> codes [R, 4 ncls], boxes [R, 4], row_off [5] (an empty first and an empty last image), lim [4, 2].
    The size codes (dw, dh) walk through: code / w exactly the clip, one fp32 step above it, -40 (exp underflows against the
    width: x2 == x1 - 1), and 0 -- dw and dh out of step with each other.  Rows 2 and 3 (R > 3) lie wholly outside their image's
    limits (beyond the far corner / at negative coordinates): all four corners clamp."""
    clip = f32(DECODE_CLIP)
    ww, wh = weights[2], weights[3]
    rng = np.random.RandomState(R + ncls)
    codes = np.zeros((R, 4 * ncls), f32)
    for r in range(R):
        for k in range(ncls):
            i = r + k
            sw = (code_for(clip, ww), code_for(np.nextafter(clip, f32(np.inf)), ww), f32(-40.0 * ww), f32(0))[i % 4]
            sh = (f32(-40.0 * wh), code_for(clip, wh), f32(0), code_for(np.nextafter(clip, f32(np.inf)), wh))[(i // 4 + i) % 4]
            codes[r, 4 * k:4 * k + 4] = (f32(rng.randint(-16, 17) / 8.0 * weights[0]), f32(rng.randint(-16, 17) / 8.0 * weights[1]), sw, sh)
    xy = rng.randint(0, 600, size=(R, 2)).astype(f32)
    wh_ = rng.randint(0, 120, size=(R, 2)).astype(f32)
    boxes = np.concatenate([xy, xy + wh_], 1).astype(f32)
    if R > 3:
        boxes[2] = (5000.0, 4000.0, 5010.0, 4020.0)
        boxes[3] = (-900.0, -800.0, -890.0, -780.0)
        codes[2:4] = 0
    first = 100 if R > 100 else R
    row_off = np.asarray([0, 0, first, R, R], np.int32)
    lim = np.asarray([[63.0, 47.0], [999.0, 799.0], [511.0, 639.0], [31.0, 15.0]], f32)
    return ro(codes), ro(boxes), ro(row_off), ro(lim)


# ================================================================================================================== losses
def rpn_loss64(obj, reg, labels, regt, pos, neg, beta):
    """-> (objectness loss, box loss), d objectness / d obj [R], d box / d reg [R, 4] in float64"""
    x, t = np.asarray(obj, np.float64), np.maximum(np.asarray(labels, np.float64), 0.0)
    pos, s = np.asarray(pos, bool), np.asarray(pos, bool) | np.asarray(neg, bool)
    n = max(int(s.sum()), 1)
    bce = (1.0 - t) * x + np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x)))
    e = np.asarray(reg, np.float64) - np.asarray(regt, np.float64)
    d = np.abs(e)
    sl1 = np.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta)
    with np.errstate(over="ignore"):
        dobj = np.where(s, 1.0 / (1.0 + np.exp(-x)) - t, 0.0) / n
    dreg = np.where(pos[:, None], np.where(d < beta, e / beta, np.sign(e)), 0.0) / n
    return (float(bce[s].sum() / n), float(sl1[pos].sum() / n)), dobj, dreg


RPN_BETAS = (1.0 / 9, 0.125)


def rpn_loss_inputs(R, beta, kind="mixed"):
    """obj [R], reg / regt [R, 4], labels [R] (-1 on unsampled anchors), pos / neg [R] bool.  kind: mixed / none / pos / neg.
    The differences reg - regt walk through exactly beta (as fp32), one fp32 step below it, exactly 0, their negatives, and
    plain values on both sides; the logits through +-100, 0 and plain values."""
    rng = np.random.RandomState(R % 1000 + (7 if beta == 0.125 else 0))
    b = f32(beta)
    regt = (rng.randint(-16, 17, size=(R, 4)) / 32.0).astype(f32)
    steps = np.asarray([b, np.nextafter(b, f32(0)), f32(0), -b, -np.nextafter(b, f32(0)), f32(0.03125), f32(-0.75), f32(2.0)], f32)
    e = steps[(np.arange(R)[:, None] * 3 + np.arange(4)[None, :]) % len(steps)]
    # the target is 0 where the difference must survive reg = regt + e and e = reg - regt unrounded (0.375 +- 0.125 does too)
    regt = np.where((np.abs(e) == b) | (np.abs(e) == np.nextafter(b, f32(0))), f32(0), regt).astype(f32)
    if beta == 0.125:
        regt = np.where(np.abs(e) == b, f32(0.375), regt).astype(f32)
    reg = (regt + e).astype(f32)
    assert ((reg - regt) == e).all()
    obj = np.asarray([100.0, -100.0, 0.0, 1.5, -2.25, 30.0, -17.0], f32)[np.arange(R) % 7]
    u = (np.arange(R) * 7) % 10
    pos, neg = u < 3, (u >= 3) & (u < 7)
    if kind == "none":
        pos, neg = np.zeros(R, bool), np.zeros(R, bool)
    elif kind == "pos":
        neg = np.zeros(R, bool)
    elif kind == "neg":
        pos = np.zeros(R, bool)
    labels = np.where(pos, 1.0, np.where(neg, 0.0, -1.0)).astype(f32)
    return ro(obj), ro(reg), ro(labels), ro(regt), ro(pos), ro(neg)


def box_loss64(logits, breg, labels, regt, n_rows=None):
    """-> (classification loss, box loss), d / d logits, d / d breg in float64; rows labelled -1 are padding; the means run over
    n_rows (clamped to 1) when given, over R otherwise"""
    l, br = np.asarray(logits, np.float64), np.asarray(breg, np.float64)
    lab, rt = np.asarray(labels, np.int64), np.asarray(regt, np.float64)
    R, NC = l.shape
    inv = 1.0 / (max(float(n_rows), 1.0) if n_rows is not None else float(R))
    dl, db = np.zeros_like(l), np.zeros_like(br)
    ce = box = 0.0
    for i in range(R):
        if lab[i] < 0:
            continue
        mx = l[i].max()
        lse = mx + math.log(np.exp(l[i] - mx).sum())
        ce += lse - l[i, lab[i]]
        dl[i] = np.exp(l[i] - lse) * inv
        dl[i, lab[i]] -= inv
        if lab[i] > 0:
            for j in range(4):
                e = br[i, 4 * lab[i] + j] - rt[i, j]
                d = abs(e)
                box += 0.5 * d * d if d < 1.0 else d - 0.5
                db[i, 4 * lab[i] + j] = (e if d < 1.0 else math.copysign(1.0, e)) * inv
    return (ce * inv, box * inv), dl, db


def box_loss_inputs(R, NC, kind="mixed"):
    """logits [R, NC] (every other row alternates +-80), breg [R, 4 NC], labels [R], regt [R, 4].  kind: mixed (classes,
    background and -1 padding rows) / moderate (the same rows over logits of +-8) / background / padding.  The differences on the labelled class walk through exactly 1,
    exactly 0, -1 and plain values on both sides."""
    rng = np.random.RandomState(R + NC)
    if kind == "moderate":     # logits over -8 .. 14 and no +-80 rows: softmax - 1 cancels (box_loss_grad_bound)
        logits = (rng.randint(-64, 65, size=(R, NC)) / 8.0).astype(f32)
        odd = np.arange(1, R, 2)
        logits[odd, (3 * odd) % NC] += f32(6)          # every other row is confident about one class
    else:
        logits = (rng.randint(-8, 9, size=(R, NC)) / 8.0).astype(f32)     # (+-1: softmax - 1 stays well away from cancelling)
        alt = np.where(np.arange(NC) % 2 == 0, f32(80), f32(-80))
        logits[::2] = alt[None, :] * np.where(np.arange(len(logits[::2])) % 2 == 0, 1, -1)[:, None].astype(f32)
    labels = ((np.arange(R) * 5 + 1) % NC).astype(np.int64)
    labels[np.arange(R) % 3 == 1] = 0
    if kind in ("mixed", "moderate"):
        labels[np.arange(R) % 5 == 4] = -1
    elif kind == "background":
        labels[:] = 0
    else:
        labels[:] = -1
    regt = (rng.randint(-16, 17, size=(R, 4)) / 16.0).astype(f32)
    breg = (rng.randint(-40, 41, size=(R, 4 * NC)) / 16.0).astype(f32)
    steps = np.asarray([1.0, 0.0, -1.0, 0.25, -3.0, 1.5], f32)
    for i in range(R):
        if labels[i] > 0:
            breg[i, 4 * labels[i]:4 * labels[i] + 4] = regt[i] + steps[(i + np.arange(4)) % len(steps)]
    return ro(logits), ro(breg), ro(labels), ro(regt)


def box_loss_grad_bound(logits, labels, n_rows):
    """the absolute error fp32 may leave in d / d logits = (softmax - onehot) / n where softmax - 1 cancels: p = expf(l - lse)
    with lse = mx + logf(sum expf(l - mx)).  The sum of NC terms carries (NC - 1) u relative, i.e. that much absolute in its
    logarithm; logf (1 ulp = 2 u) and the addition of mx leave 3 u |lse|; l - lse rounds with u |l - lse|; expf (1 ulp) and the
    final subtraction and scaling add 4 u relative to p.  Together  p u (4 |lse| + |l - lse| + NC + 4) / n  per element."""
    l = np.asarray(logits, np.float64)
    mx = l.max(1, keepdims=True)
    lse = mx + np.log(np.exp(l - mx).sum(1, keepdims=True))
    p = np.exp(l - lse)
    b = p * U * (4.0 * np.abs(lse) + np.abs(l - lse) + l.shape[1] + 4.0) / max(float(n_rows), 1.0)
    return np.where(np.asarray(labels)[:, None] >= 0, b, 0.0)
