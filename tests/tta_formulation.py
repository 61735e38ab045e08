"""The two merges of test-time augmentation (GeneralizedRCNN.forward_tta; csrc/tta.hip) stated in plain fp64 torch: the checker of
the kernels (tests/test_tta_kernels_gpu.py) and of the model's taps (tests/test_tta_model_gpu.py).  `flips[v]`: view v was
computed on the mirror image."""
import torch


def merge_box(logits, reg, flips):
    """logits (V, R, C), reg (V, R, 4C) -> prob (R, C) = (sum_v softmax(logits_v)) / V, reg (R, 4C) = (sum_v s_v * reg_v) / V with
    s_v = -1 on the dx component of every class for a mirrored view; sums in ascending v"""
    V, R, C = logits.shape
    assert tuple(reg.shape) == (V, R, 4 * C) and len(flips) == V
    logits, reg = logits.to(torch.float64), reg.to(torch.float64)
    prob = torch.zeros((R, C), dtype=torch.float64)
    out = torch.zeros((R, 4 * C), dtype=torch.float64)
    for v in range(V):
        prob = prob + torch.softmax(logits[v], dim=1)
        s = torch.ones((4 * C,), dtype=torch.float64)
        if flips[v]:
            s[0::4] = -1.0
        out = out + s * reg[v]
    return prob / V, out / V


def merge_mask(logits, labels, flips):
    """logits (V, D, C, M, M), labels (D,) -> (D, M, M): p[d, y, x] = (sum_v sigmoid(logits[v, d, labels[d], y, x_v])) / V with
    x_v = M - 1 - x for a mirrored view; a label outside [0, C) gives a block of NaN"""
    V, D, C, M, _ = logits.shape
    assert len(flips) == V
    logits = logits.to(torch.float64)
    ok = (labels >= 0) & (labels < C)
    lab = torch.where(ok, labels, torch.zeros_like(labels))
    out = torch.zeros((D, M, M), dtype=torch.float64)
    for v in range(V):
        p = torch.sigmoid(logits[v][torch.arange(D), lab])
        out = out + (torch.flip(p, (2,)) if flips[v] else p)
    out = out / V
    out[~ok] = float("nan")
    return out
