"""Seeded inputs for the image-size polygon rasteriser (csrc/polyfill.hip: `mmt_polygon_mask_words`, `mmt_mask_words_integral`)
and what is built on it, shared by tests/test_polygon_image_inputs.py (the inputs against the oracle alone),
tests/test_polygon_words_host.py (the codec's host `frPolygons`) and tests/test_polygon_words_gpu.py (the kernels).  Plain numpy on
the CPU.

Sizes (H, W): the smallest mask; H * W off the word grid with H < 64 (a word spans several columns); a word per column; H above
64 and off the word grid, both ways round; very wide, very tall; and the workload's own 1000 x 1000 once, with 24 instances.

Classes, PER_CLASS instances each at every small size:
  i     ordinary blobs inside the image
  ii    polygons wholly outside the image, beyond each border in turn (empty masks)
  iii   polygons that cross every image edge
  iv    vertices on multiples of 0.5 and 0.1 (the `+ .5` rounding ties of the x5 walk)
  v     every vertex repeated, collinear runs, polygons of one and of two vertices
  vi    more than 64 and more than 256 edges; one edge longer than the image
  vii   instances of 2-3 overlapping polygons (their union is not their XOR)
  viii  instances with an empty polygon range
  ix    polygons whose boundary passes below the bottom row of the last column (the crossing at H * W, which is dropped)"""
import functools

import numpy as np

from mask_geometry_inputs import _blob

SIZES = [(1, 1), (37, 53), (64, 64), (150, 128), (128, 150), (5, 200), (130, 3)]
BIG = (1000, 1000)
BIG_INSTANCES = 24
CLASSES = ("i", "ii", "iii", "iv", "v", "vi", "vii", "viii", "ix")
PER_CLASS = 4


def _inside(rng, H, W, nv=None, rough=0.4):
    return _blob(rng, W * rng.uniform(0.3, 0.7), H * rng.uniform(0.3, 0.7), max(W * rng.uniform(0.12, 0.3), 0.4),
                 max(H * rng.uniform(0.12, 0.3), 0.4), nv or int(rng.randint(3, 25)), rough)


def _class_i(rng, H, W, i):
    return [_inside(rng, H, W)]


def _class_ii(rng, H, W, i):
    rx, ry = max(0.3 * W, 2.0), max(0.3 * H, 2.0)
    cx, cy = [(-rx - 2.0, 0.5 * H), (W + rx + 2.0, 0.5 * H), (0.5 * W, -ry - 2.0), (0.5 * W, H + ry + 2.0)][i % 4]
    return [_blob(rng, cx, cy, rx, ry, int(rng.randint(3, 25)))]


def _class_iii(rng, H, W, i):
    # a star around the centre with radii between 0.375 and 0.75 of the sides, one vertex at full radius towards each edge: the
    # boundary weaves in and out of the image through all four edges
    nv = int(rng.randint(12, 36))
    th = np.concatenate([rng.uniform(0, 2 * np.pi, nv), np.arange(4) * np.pi / 2])
    r = np.concatenate([1.0 - 0.5 * rng.uniform(0, 1, nv), np.ones(4)])
    o = np.argsort(th)
    th, r = th[o], r[o]
    cx, cy = 0.5 * W + rng.uniform(-0.05, 0.05) * W, 0.5 * H + rng.uniform(-0.05, 0.05) * H
    return [np.stack([cx + (0.75 * W + 1) * r * np.cos(th), cy + (0.75 * H + 1) * r * np.sin(th)], 1)]


def _class_iv(rng, H, W, i):
    step = 0.5 if i % 2 == 0 else 0.1
    return [np.round(_inside(rng, H, W) / step) * step]


def _class_v(rng, H, W, i):
    p = _inside(rng, H, W, nv=int(rng.randint(4, 12)))
    kind = i % 4
    if kind == 0:      # every vertex twice: zero-length edges
        return [np.repeat(p, 2, 0)]
    if kind == 1:      # an axis-aligned rectangle with several vertices along every side, every vertex twice
        lo, hi = p.min(0), p.max(0)
        t = np.linspace(0, 1, 5)[:-1, None]
        c = [np.array(lo), np.array([hi[0], lo[1]]), np.array(hi), np.array([lo[0], hi[1]])]
        return [np.repeat(np.concatenate([c[s] + t * (c[(s + 1) % 4] - c[s]) for s in range(4)], 0), 2, 0)]
    if kind == 2:      # one vertex, beside an ordinary polygon
        return [p[:1], _inside(rng, H, W)]
    return [p[:2], _inside(rng, H, W)]   # two vertices: an edge walked there and back


def _class_vi(rng, H, W, i):
    kind = i % 4
    if kind == 0:
        return [_inside(rng, H, W, nv=100, rough=0.6)]
    if kind == 1:
        return [_inside(rng, H, W, nv=300, rough=0.6)]
    if kind == 2:      # the first edge runs from left of the image to right of it
        return [np.array([[-0.5 * W - 1, 0.3 * H], [1.5 * W + 1, 0.45 * H], [0.5 * W, 2.0 * H + 1]])]
    return [_inside(rng, H, W, nv=70, rough=0.6), _inside(rng, H, W, nv=260, rough=0.3)]


def _class_vii(rng, H, W, i):
    cx, cy = W * rng.uniform(0.4, 0.6), H * rng.uniform(0.4, 0.6)
    return [_blob(rng, cx + rng.uniform(-0.1, 0.1) * W, cy + rng.uniform(-0.1, 0.1) * H, max(0.3 * W, 0.6), max(0.3 * H, 0.6),
                  int(rng.randint(5, 25)), rough=0.3) for _ in range(2 + i % 2)]


def _class_ix(rng, H, W, i):
    x0, y0 = W * rng.uniform(0.15, 0.4), H * rng.uniform(0.15, 0.4)
    x1, y1 = W + rng.uniform(1, 4), H + rng.uniform(1, 5)
    p = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])
    return [p if i % 2 == 0 else p[::-1].copy()]


_MAKERS = {"i": _class_i, "ii": _class_ii, "iii": _class_iii, "iv": _class_iv, "v": _class_v, "vi": _class_vi,
           "vii": _class_vii, "ix": _class_ix}


def _pack(instances, cls, rng):
    """instances: list of lists of (k, 2) arrays, None = an empty range somewhere -> the dict; instance order shuffled, the
    polygons stay where they were laid down (so the ranges are not sorted)"""
    polys, ranges = [], []
    for inst in instances:
        if inst is None:
            s = int(rng.randint(0, len(polys) + 1))
            ranges.append((s, s))
        else:
            ranges.append((len(polys), len(polys) + len(inst)))
            polys.extend(inst)
    order = rng.permutation(len(ranges))
    xy = np.concatenate(polys, 0).astype(np.float32) if polys else np.zeros((0, 2), np.float32)
    return {"poly_xy": xy, "poly_off": np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int32),
            "inst_poly": np.asarray(ranges, np.int32).reshape(-1, 2)[order], "cls": np.asarray(cls)[order]}


@functools.lru_cache(maxsize=None)
def cases(size, seed=0):
    """-> dict: poly_xy float32 (V, 2), poly_off int32 (NP + 1,), inst_poly int32 (G, 2), cls (G,) class names.  Treat as
    read-only: the dict is shared between tests"""
    H, W = size
    rng = np.random.RandomState(seed + 7919 * H + W)
    inst, cls = [], []
    if size == BIG:
        kinds = ["i", "iii", "vii", "ix", "vi", "iv"]
        for i in range(BIG_INSTANCES):
            c = kinds[i % len(kinds)]
            inst.append(_MAKERS[c](rng, H, W, i // len(kinds)))
            cls.append(c)
    else:
        for c in CLASSES:
            for i in range(PER_CLASS):
                inst.append(None if c == "viii" else _MAKERS[c](rng, H, W, i))
                cls.append(c)
    return _pack(inst, cls, rng)


def polygons_of(c, g):
    """the float32 (k, 2) polygons of instance g"""
    off = c["poly_off"]
    return [c["poly_xy"][off[p]:off[p + 1]] for p in range(*c["inst_poly"][g])]


def segm_of(c):
    """the cases as frPolygons takes them: a list of instances, each a list of flat float32 polygons"""
    return [[p.reshape(-1) for p in polygons_of(c, g)] for g in range(len(c["inst_poly"]))]


@functools.lru_cache(maxsize=None)
def oracle_masks(size, seed=0):
    """oracle.native.poly_mask of every instance -> uint8 (G, H, W); an empty range (which the oracle, like pycocotools' merge,
    is never asked for) is all zero.  Computed once per size; read-only"""
    from oracle import native
    H, W = size
    c = cases(size, seed)
    out = np.zeros((len(c["inst_poly"]), H, W), np.uint8)
    for g in range(len(out)):
        polys = polygons_of(c, g)
        if polys:
            out[g] = native.poly_mask([p.reshape(-1) for p in polys], H, W)
    out.setflags(write=False)
    return out
