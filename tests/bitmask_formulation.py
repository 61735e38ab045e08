"""Bitmap ground truth, restated on the host from the definitions alone ("Bitmap ground truth"): the window of
a box, the integer bilinear resampling of a window, the flips, and a column-major packer to words and records.  int64 torch, no
floats anywhere but the box coordinates.  A helper, not a test."""
import math

import torch

REC = 8   # area, xmin, xmax, ymin, ymax, wrap, 0, 0


def window(box, W, H):
    """(x1, y1, x2, y2) float32 -> (x0, y0, w, h), or None when a coordinate is not finite"""
    b = [float(v) for v in torch.as_tensor(box, dtype=torch.float32).reshape(4)]
    if not all(math.isfinite(v) for v in b):
        return None
    xa, ya, xb, yb = (int(min(max(round(v), -2 ** 30), 2 ** 30)) for v in b)   # round(): half to even
    x0, y0 = min(max(xa, 0), W - 1), min(max(ya, 0), H - 1)
    xe, ye = max(min(max(xb, 0), W), x0 + 1), max(min(max(yb, 0), H), y0 + 1)
    return x0, y0, xe - x0, ye - y0


def taps(n, out):
    """-> ia, ib, r, d for the `out` output indices over `n` source ones"""
    i = torch.arange(out, dtype=torch.int64)
    num = ((2 * i + 1) * n - out).clamp(min=0)
    d = 2 * out
    ia = torch.div(num, d, rounding_mode="floor")
    return ia, (ia + 1).clamp(max=n - 1), num - ia * d, d


def weighted_sum(src, OH, OW):
    """src (..., h, w) of {0, 1} -> (S int64 (..., OH, OW), dx * dy): S / (dx dy) is the bilinear value"""
    p = torch.as_tensor(src).to(torch.int64)
    h, w = p.shape[-2:]
    ia, ib, ry, dy = taps(h, OH)
    ja, jb, rx, dx = taps(w, OW)
    ra, rb = p.index_select(-2, ia), p.index_select(-2, ib)
    top = (dx - rx) * ra.index_select(-1, ja) + rx * ra.index_select(-1, jb)
    bot = (dx - rx) * rb.index_select(-1, ja) + rx * rb.index_select(-1, jb)
    return (dy - ry)[:, None] * top + ry[:, None] * bot, dx * dy


def resample(masks, win, OH, OW, flip=0):
    """masks (..., H, W) -> uint8 (..., OH, OW): the window resampled, ties set; flip bit 0 left-right, bit 1 top-bottom"""
    m = torch.as_tensor(masks)
    if win is None:
        return torch.zeros(tuple(m.shape[:-2]) + (OH, OW), dtype=torch.uint8)
    x0, y0, w, h = win
    S, dd = weighted_sum(m[..., y0:y0 + h, x0:x0 + w] != 0, OH, OW)
    out = (2 * S >= dd).to(torch.uint8)
    if flip & 1:
        out = out.flip(-1)
    if flip & 2:
        out = out.flip(-2)
    return out


def targets(masks, roi_inst, boxes, M):
    """masks (G, H, W), roi_inst (P,), boxes (P, 4) -> float32 (P, M, M)"""
    G, H, W = masks.shape
    out = torch.zeros((len(roi_inst), M, M), dtype=torch.float32)
    for p, (g, b) in enumerate(zip([int(v) for v in roi_inst], boxes)):
        if 0 <= g < G:
            out[p] = resample(masks[g], window(b, W, H), M, M).float()
    return out


def pack(masks):
    """uint8 (G, H, W) -> (words int64 (G, ceil(H W / 64)), records int32 (G, 8)): bit k of a mask is pixel (k % H, k / H)"""
    m = (torch.as_tensor(masks) != 0)
    G, H, W = m.shape
    nw = (H * W + 63) // 64
    flat = torch.zeros((G, nw * 64), dtype=torch.int64)
    flat[:, :H * W] = m.transpose(1, 2).reshape(G, H * W)
    words = (flat.reshape(G, nw, 64) << torch.arange(64, dtype=torch.int64)).sum(-1)   # (bit 63 wraps into the sign)
    rec = torch.zeros((G, REC), dtype=torch.int32)
    for g in range(G):
        ys, xs = m[g].nonzero(as_tuple=True)
        if ys.numel():
            wrap = int(W > 1 and bool((m[g, -1, :-1] & m[g, 0, 1:]).any()))
            rec[g, :6] = torch.tensor([ys.numel(), int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max()), wrap], dtype=torch.int32)
    return words, rec
