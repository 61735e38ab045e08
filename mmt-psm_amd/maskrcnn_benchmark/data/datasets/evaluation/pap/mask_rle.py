"""Run-length masks for the PAP evaluator: the five calls the reference makes into its vendored pycocotools
(`/root/reference/pycoco/_mask.pyx`: encode :144, decode :160, merge :177, area :190, iouIntUni :293-380; C side
`maskApi.c`: rleEncode :21-34, rleToString / rleFrString :204-236, rleIouInterUnion :239-260) restated on numpy, and the polygon rasteriser behind a sixth, `frPyObjects` (`maskApi.c`:
rleFrPoly :166-206), as `frPolygons`.

An RLE is COCO's: {"size": [h, w], "counts": ...} over the mask flattened COLUMN-major, runs alternating 0 / 1 starting with
zeros; `counts` is the compressed ASCII string (bytes or str) or a plain list of run lengths (COCO's "uncompressed" form).
Host code: evaluation runs once per checkpoint on a few hundred windows ("irrelevant to the throughput
metric").

Opt-in device path (`encode_device`, `iouIntUni(..., on_device=True)`): the dense mask work -- finding the runs of a pasted
mask, decoding every string for every (window, category), the pair intersections -- runs in the HIP kernels of
csrc/maskeval.hip (include/mmtpsm.h: mmt_mask_*); the host keeps the strings.  Same strings byte for byte, same integers.
It has no fallback: without a GPU or the library it raises."""
import numpy as np


def _runs(flat):
    """flat uint8 {0,1} -> run lengths, first run = zeros (possibly of length 0)"""
    n = flat.shape[0]
    if n == 0:
        return [0]
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    edges = np.concatenate(([0], change, [n]))
    runs = np.diff(edges).tolist()
    if flat[0]:
        runs = [0] + runs
    return runs


def _to_string(cnts):
    """maskApi.c:204-217: LEB128-like, 5 data bits + continuation bit per char (ASCII 48..111); from the third run on the
    difference to the run two places back is stored"""
    out = []
    for i, c in enumerate(cnts):
        x = int(c)
        if i > 2:
            x -= int(cnts[i - 2])
        more = True
        while more:
            ch = x & 0x1f
            x >>= 5
            more = (x != -1) if (ch & 0x10) else (x != 0)
            if more:
                ch |= 0x20
            out.append(chr(ch + 48))
    return "".join(out)


def _from_string(s):
    """maskApi.c:219-236"""
    if isinstance(s, bytes):
        s = s.decode("ascii")
    cnts, p, n = [], 0, len(s)
    while p < n:
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return cnts


def counts_of(rle):
    c = rle["counts"]
    return [int(v) for v in c] if isinstance(c, (list, tuple, np.ndarray)) else _from_string(c)


def encode(mask):
    """(h, w) -> RLE; (h, w, n) -> list of RLEs (`_mask.pyx:144`); counts as bytes like pycocotools"""
    m = np.asarray(mask)
    if m.ndim == 3:
        return [encode(m[:, :, i]) for i in range(m.shape[2])]
    h, w = m.shape
    runs = _runs((m != 0).astype(np.uint8).flatten(order="F"))
    return {"size": [int(h), int(w)], "counts": _to_string(runs).encode("ascii")}


def decode(rle):
    """RLE -> (h, w) uint8 in Fortran order; list of RLEs -> (h, w, n)"""
    if isinstance(rle, (list, tuple)):
        return np.stack([decode(r) for r in rle], axis=2) if len(rle) else np.zeros((0, 0, 0), np.uint8)
    h, w = rle["size"]
    cnts = counts_of(rle)
    vals = np.zeros(len(cnts), dtype=np.uint8)
    vals[1::2] = 1
    flat = np.repeat(vals, cnts)
    if flat.shape[0] != h * w:
        raise ValueError("RLE does not cover its %d x %d mask" % (h, w))
    return flat.reshape((h, w), order="F")


def area(rle):
    if isinstance(rle, (list, tuple)):
        return np.array([area(r) for r in rle], dtype=np.uint32)
    return np.uint32(sum(counts_of(rle)[1::2]))


def merge(rles, intersect=False):
    """union (or intersection) of several masks as one RLE (`_mask.pyx:177`)"""
    if not len(rles):
        raise ValueError("merge of an empty list")
    acc = decode(rles[0]).astype(bool)
    for r in rles[1:]:
        acc = (acc & decode(r).astype(bool)) if intersect else (acc | decode(r).astype(bool))
    return encode(acc.astype(np.uint8))


def _bbox(m):
    """rleToBbox (maskApi.c:135-151): [x, y, w, h] of the mask's extent; an empty mask is [0, 0, 0, 0].  The C code works on
    the runs: a run of ones that continues from the bottom of one column into the top of the next makes the box full height."""
    ys, xs = np.nonzero(m)
    if ys.size == 0:
        return 0.0, 0.0, 0.0, 0.0
    y0, y1 = int(ys.min()), int(ys.max())
    if m.shape[1] > 1 and bool(np.any(m[-1, :-1] & m[0, 1:])):
        y0, y1 = 0, m.shape[0] - 1
    return float(xs.min()), float(y0), float(xs.max() - xs.min() + 1), float(y1 - y0 + 1)


def _backend():
    """the HIP binding, or RuntimeError: the device path has no host fallback"""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("on_device=True: the mask kernels (csrc/maskeval.hip) need the MI355X; no GPU visible")
    from maskrcnn_benchmark import _hip
    _hip.lib()
    return _hip


def _runs_of_positions(pos, n):
    """ascending positions k in [0, n) where bit(k) != bit(k - 1), bit(-1) = 0 -> run lengths as `_runs` gives them: a leading
    position 0 is the zero-length first run of a mask that starts with a set pixel, no position at all is [n]"""
    if n == 0:
        return [0]
    pos = np.asarray(pos, dtype=np.int64)
    return np.diff(np.concatenate(([0], pos, [n]))).tolist()


def encode_device(masks):
    """uint8 GPU tensor (n, H, W) or (n, 1, H, W), non-zero = set -> [encode(m) for m in masks.cpu().numpy()] with the runs
    found on the device (mmt_mask_pack + mmt_mask_transition_*): only the transition counts and positions cross to the host"""
    H = _backend()
    if masks.dim() == 4 and masks.shape[1] == 1:
        masks = masks[:, 0]
    if masks.dim() != 3:
        raise RuntimeError("encode_device: (n, H, W) or (n, 1, H, W) masks")
    n, h, w = (int(v) for v in masks.shape)
    if n == 0:
        return []
    if h * w == 0:
        return [{"size": [h, w], "counts": _to_string([0]).encode("ascii")} for _ in range(n)]
    words, _ = H.mask_pack(masks)
    return _strings_of_words(H, words, h, w)


def _strings_of_words(H, words, h, w):
    """mask words on the device -> the list of RLE dicts; only the transition counts and positions cross to the host"""
    counts, pos = H.mask_transitions(words, h, w)
    pos, out, at = pos.numpy(), [], 0
    for c in counts.tolist():
        out.append({"size": [h, w], "counts": _to_string(_runs_of_positions(pos[at:at + c], h * w)).encode("ascii")})
        at += c
    return out


def encode_pasted_device(prob, boxes, h, w, thresh=0.5):
    """M x M probabilities (D, 1, M, M) or (D, M, M) and their boxes (D, 4) in an h x w image -> what
    encode_device(paste_mask_stack(prob, boxes, h, w, thresh)) returns, byte for byte, with the paste written straight into
    the codec's words (mmt_paste_mask_words): the (D, h, w) byte stack is never made"""
    H = _backend()
    h, w = int(h), int(w)
    if int(prob.shape[0]) == 0:
        return []
    words, _ = H.paste_mask_words(prob, boxes, h, w, thresh)
    return _strings_of_words(H, words, h, w)


def _poly_crossings(xy, h, w):
    """one polygon, float64 (k, 2) -> the column crossings a = x * h + y of rleFrPoly (maskApi.c:166-206), unsorted: the x5
    boundary walk edge by edge (every step is closed-form in t, and a crossing at step d needs steps d and d - 1 only; the walk
    never changes column between the last point of an edge and the first of the next, which are the same point)"""
    k = xy.shape[0]
    if k == 0:
        return np.zeros(0, np.int64)
    X = np.trunc(5.0 * xy[:, 0] + .5).astype(np.int64)
    Y = np.trunc(5.0 * xy[:, 1] + .5).astype(np.int64)
    found = [np.zeros(0, np.int64)]
    for j in range(k):
        xs, ys, xe, ye = int(X[j]), int(Y[j]), int(X[(j + 1) % k]), int(Y[(j + 1) % k])
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
            u, v = t + xs, np.trunc(ys + (float(ye - ys) / dx) * t + .5)
        else:
            u, v = np.trunc(xs + (float(xe - xs) / dy) * t + .5), t + ys
        ch = u[1:] != u[:-1]
        xd = np.where(u[1:] < u[:-1], u[1:], u[1:] - 1)[ch]
        xd = (xd + .5) / 5.0 - .5
        ok = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
        yd = np.ceil(np.clip((np.minimum(v[1:], v[:-1])[ch][ok] + .5) / 5.0 - .5, 0, h))
        found.append((xd[ok] * h + yd).astype(np.int64))
    return np.concatenate(found)


def _poly_fill(xy, h, w):
    """one polygon -> bool (h * w,) over the column-major flattening: rleFrPoly's sorted run lengths say that pixel q is the
    parity of the crossings at or below q; a crossing at h * w lies behind the last pixel"""
    a = _poly_crossings(xy, h, w)
    return (np.cumsum(np.bincount(a, minlength=h * w + 1)[:h * w]) & 1).astype(bool)


def _instances_of(segm):
    """a SegmentationMask, or a list of instances, each a Polygons or a list of flat [x0, y0, x1, y1, ...] polygons
    -> [[float64 (k, 2), ...], ...]"""
    out = []
    for inst in (segm.polygons if hasattr(segm, "polygons") else segm):
        polys = inst.polygons if hasattr(inst, "polygons") else inst
        out.append([np.asarray(p.detach().cpu().numpy() if hasattr(p, "detach") else p, dtype=np.float64).reshape(-1, 2) for p in polys])
    return out


def frPolygons(segm, h, w, on_device=False):
    """polygon ground truth -> one RLE per instance: `encode(decode(merge(frPyObjects(polys, h, w))))` of the reference's
    pycocotools (`_mask.pyx` frPyObjects -> maskApi.c:166-206 rleFrPoly; merge = union of the instance's polygons).  `segm`: a
    SegmentationMask or a list of instances, each a list of flat polygons.  Host: the boundary walk restated on numpy.
    on_device=True: `mmt_polygon_mask_words` (csrc/polyfill.hip, vertices in float32 as SegmentationMask keeps them), then the
    run boundaries as for every other device string; RuntimeError without a GPU or the library"""
    h, w = int(h), int(w)
    inst = _instances_of(segm)
    if on_device:
        H = _backend()
        import torch
        if not inst:
            return []
        if h * w == 0:
            return [{"size": [h, w], "counts": _to_string([0]).encode("ascii")} for _ in inst]
        device = torch.device("cuda", torch.cuda.current_device())
        polys = [p for i in inst for p in i]
        off = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int32)
        ends = np.cumsum([len(i) for i in inst])
        rng = np.stack([ends - [len(i) for i in inst], ends], 1).astype(np.int32)
        xy = np.concatenate(polys + [np.zeros((0, 2))], 0).astype(np.float32)
        words, _ = H.polygon_mask_words(torch.from_numpy(xy).to(device), torch.from_numpy(off).to(device),
                                        torch.from_numpy(rng).to(device), h, w)
        return _strings_of_words(H, words, h, w)
    out = []
    for polys in inst:
        acc = np.zeros(h * w, bool)
        for p in polys:
            acc |= _poly_fill(p, h, w)
        out.append({"size": [h, w], "counts": _to_string(_runs(acc.astype(np.uint8))).encode("ascii")})
    return out


def _expand_device(H, rles, device):
    """RLEs of ONE size -> (words, records on the host) (mmt_mask_expand): the host parses the strings and hands over the prefix
    sums of the runs"""
    import torch
    h, w = (int(v) for v in rles[0]["size"])
    ends, off = [], [0]
    for r in rles:
        e = np.cumsum(np.asarray(counts_of(r), dtype=np.int64))
        if e.shape[0] == 0 or e[-1] != h * w or (np.diff(e) < 0).any() or e[0] < 0:
            raise ValueError("RLE does not cover its %d x %d mask" % (h, w))
        ends.append(e.astype(np.int32))
        off.append(off[-1] + e.shape[0])
    ends = torch.from_numpy(np.concatenate(ends)).to(device)
    off = torch.tensor(off, dtype=torch.int64).to(device)
    words, rec = H.mask_expand(ends, off, h, w)
    return words, rec.cpu().numpy().astype(np.int64)


def _box_of_record(r, h):
    """`_bbox` from a device record (area, xmin, xmax, ymin, ymax, wrap)"""
    if r[0] == 0:
        return 0, 0, 0, 0
    return (r[1], 0, r[2] - r[1] + 1, h) if r[5] else (r[1], r[3], r[2] - r[1] + 1, r[4] - r[3] + 1)


def _iouIntUni_device(dt, gt, iscrowd):
    import torch
    H = _backend()
    m, n = len(dt), len(gt)
    device = torch.device("cuda", torch.cuda.current_device())
    groups = {}   # size -> ([detection indices], [ground-truth indices])
    for side, lst in enumerate((dt, gt)):
        for i, r in enumerate(lst):
            groups.setdefault(tuple(int(v) for v in r["size"]), ([], []))[side].append(i)
    if any(h * w == 0 for h, w in groups):
        raise RuntimeError("on_device=True: masks without pixels")
    inter = np.full((m, n), -1, dtype=np.int64)          # -1: boxes disjoint
    other = np.zeros((m, n), dtype=bool)                 # sizes differ
    area_d, box_d, box_g = np.zeros(m, np.int64), [None] * m, [None] * n
    area_g = np.zeros(n, np.int64)
    for (h, w), (di, gi) in groups.items():
        dw = gw = None
        if di:
            dw, drec = _expand_device(H, [dt[i] for i in di], device)
            area_d[di] = drec[:, 0]
            for i, r in zip(di, drec):
                box_d[i] = _box_of_record(r, h)
        if gi:
            gw, grec = _expand_device(H, [gt[i] for i in gi], device)
            area_g[gi] = grec[:, 0]
            for i, r in zip(gi, grec):
                box_g[i] = _box_of_record(r, h)
        if di and gi:
            dr = torch.from_numpy(drec.astype(np.int32)).to(device)
            gr = torch.from_numpy(grec.astype(np.int32)).to(device)
            inter[np.ix_(di, gi)] = H.mask_pair_intersections(dw, dr, gw, gr, h, w).cpu().numpy()
    if len(groups) > 1:   # pairs of unequal sizes: -1 where the boxes overlap, settled here before (and without) any launch for them
        for d in range(m):
            for g in range(n):
                if tuple(dt[d]["size"]) != tuple(gt[g]["size"]):
                    bd, bg = box_d[d], box_g[g]
                    ow = min(bd[0] + bd[2], bg[0] + bg[2]) - max(bd[0], bg[0])
                    oh = min(bd[1] + bd[3], bg[1] + bg[3]) - max(bd[1], bg[1])
                    other[d, g] = ow > 0 and oh > 0
    hit = (inter >= 0) & ~other
    i = np.where(hit, inter, 0)
    u = area_d[:, None] + area_g[None, :] - i
    if iscrowd is not None:
        crowd = np.array([bool(c) for c in iscrowd], dtype=bool)
        u = np.where(crowd[None, :], area_d[:, None], u)
    u = np.where(i == 0, 1, u)
    iou = np.where(hit, i / u, 0.0)
    iou[other] = -1
    return iou, np.where(hit, i, 0).astype(np.float64), np.where(hit, u, 0).astype(np.float64)


def iouIntUni(dt, gt, iscrowd, on_device=False):
    """(iou, intersection, union), each (len(dt), len(gt)) float64 -- the fork's addition to pycocotools (`_mask.pyx:293-380`,
    `maskApi.c:239-260`): pairs whose bounding boxes overlap get i = |d & g| and u = |d | g| (crowd gt: u = |d|) with the C
    code's `i == 0 -> u = 1`; a pair of different mask sizes gets iou -1.  Pairs whose boxes do not overlap have iou 0 and
    -- where the C code leaves its malloc'ed intersection / union cells unwritten -- intersection 0, union 0 here.
    [] when either list is empty.  on_device=True: the same three matrices from the expand and pair kernels of csrc/maskeval.hip
    (RuntimeError without a GPU or the library)."""
    m, n = len(dt), len(gt)
    if on_device:
        _backend()
    if m == 0 or n == 0:
        return []
    if on_device:
        return _iouIntUni_device(dt, gt, iscrowd)
    D = [decode(r).astype(bool) for r in dt]
    G = [decode(r).astype(bool) for r in gt]
    bd, bg = [_bbox(x) for x in D], [_bbox(x) for x in G]
    iou, inter, uni = np.zeros((m, n)), np.zeros((m, n)), np.zeros((m, n))
    for g in range(n):
        for d in range(m):
            w = min(bd[d][0] + bd[d][2], bg[g][0] + bg[g][2]) - max(bd[d][0], bg[g][0])
            h = min(bd[d][1] + bd[d][3], bg[g][1] + bg[g][3]) - max(bd[d][1], bg[g][1])
            if w <= 0 or h <= 0:
                continue
            if D[d].shape != G[g].shape:
                iou[d, g] = -1
                continue
            i = int(np.count_nonzero(D[d] & G[g]))
            u = int(np.count_nonzero(D[d] | G[g]))
            if i == 0:
                u = 1
            elif iscrowd is not None and iscrowd[g]:
                u = int(np.count_nonzero(D[d]))
            iou[d, g], inter[d, g], uni[d, g] = i / u, float(i), float(u)
    return iou, inter, uni
