"""Edge-case masks for the device mask codec (tests/test_mask_eval_gpu.py, tests/test_mask_eval_host.py): the smallest sizes
that reach every edge of the kernels of csrc/maskeval.hip -- H * W no multiple of 64, a single row, a single column, H = 64
(every column exactly one word, each column boundary on the carry) -- and, beyond the issue's list, one size above the strip
kernel's LDS limit (H > 4096: the word-per-thread pack kernel)."""
import numpy as np

SIZES = [(1, 1), (1, 70), (70, 1), (5, 6), (37, 53), (64, 3), (64, 64), (96, 96), (130, 67)]
TALL = (4100, 3)


def masks_of(h, w, seed=0):
    """-> [(name, uint8 (h, w))]: empty, full, one pixel at each end, a checkerboard over the column-major flattening (every
    position is a transition), Bernoulli(0.5), and for w > 1 the two pixels {(h-1, 0), (0, 1)} that make `wrap`"""
    out = [("empty", np.zeros((h, w), np.uint8)), ("full", np.ones((h, w), np.uint8))]
    m = np.zeros((h, w), np.uint8); m[0, 0] = 1
    out.append(("first", m))
    m = np.zeros((h, w), np.uint8); m[h - 1, w - 1] = 1
    out.append(("last", m))
    out.append(("checker", (np.arange(h * w) % 2 == 0).astype(np.uint8).reshape((h, w), order="F")))
    rng = np.random.RandomState(1000 * h + w + seed)
    out.append(("bernoulli", (rng.rand(h, w) < 0.5).astype(np.uint8)))
    if w > 1:
        m = np.zeros((h, w), np.uint8); m[h - 1, 0] = 1; m[0, 1] = 1
        out.append(("wrap", m))
    return out


def all_cases():
    return [(h, w, name, m) for h, w in SIZES for name, m in masks_of(h, w)]


def positions(mask):
    """where bit(k) != bit(k - 1) over the column-major flattening, bit(-1) = 0 (numpy)"""
    flat = (np.asarray(mask) != 0).astype(np.uint8).flatten(order="F")
    return np.flatnonzero(flat != np.concatenate(([0], flat[:-1])))
