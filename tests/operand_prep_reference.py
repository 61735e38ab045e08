"""Plain torch / numpy statements of what the operand-preparation kernels promise (include/mmtpsm.h: mmt_split_planes, mmt_split_planes_f16
/ _rb, mmt_pack_weight* and their batched forms, mmt_amax / mmt_amax_stats / mmt_sum_stats / _rb, mmt_stats_combine, mmt_rb_scales_update),
written from the header's words, and the seeded input builders the CPU and the GPU tests share.  Nothing here imports the library.

Conventions: planes are returned as torch.int16 (the bit patterns of bf16 / fp16 values), scales and maxima compare as their int32 bits.
`torch.Tensor.bfloat16()` and `.half()` round to nearest even and keep subnormals; fp32 arithmetic on the CPU keeps subnormals too."""
import math

import numpy as np
import torch

F16_MAX = 65504.0


def bits16(t):
    return t.contiguous().view(torch.int16)


def bits32(t):
    return torch.as_tensor(t, dtype=torch.float32).contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------ the two splits
def split_bf16x3(x):
    """x fp32 -> (3, n) bf16: p0 = rne(x), p1 = rne(x - p0), p2 = rne(x - p0 - p1); the residuals are exact in fp32"""
    x = x.reshape(-1).float()
    p0 = x.bfloat16()
    r1 = x - p0.float()
    p1 = r1.bfloat16()
    r2 = r1 - p1.float()
    p2 = r2.bfloat16()
    return torch.stack([p0, p1, p2])


def f16_scale_of(amax):
    """the power of two that puts amax into [2^13, 2^14]: 1 unless amax > 0, else 2^clamp(14 - frexp(amax).e, -100, 100)"""
    amax = float(np.float32(amax))
    if not amax > 0.0:
        return 1.0
    e = math.frexp(amax)[1]
    return math.ldexp(1.0, max(-100, min(100, 14 - e)))


def split_f16x2(x, s):
    """x fp32, s a power of two -> (2, n) fp16: r = clamp(fp32(x s), +-65504), h = rne(r), l = rne(r - h) (the residual is exact in fp32)"""
    r = (x.reshape(-1).float() * torch.tensor(s, dtype=torch.float32)).clamp(-F16_MAX, F16_MAX)
    h = r.half()
    l = (r - h.float()).half()
    return torch.stack([h, l])


# ------------------------------------------------------------------------------------------ layouts
def packed_elems(Cout, K):
    return (K // 16) * ((Cout + 31) // 32) * 512


def pack_layout(Cout, K):
    """position inside a packed plane of element (row n, column k) of a [32 ceil(Cout / 32)][K] matrix (rows >= Cout are the padding):
    the tiling [K / 16][ceil(Cout / 32)][32 rows][2 halves][8], the two 8-element halves of a 16-k step swapped in rows 8-15 and 24-31
    of every 32-row block -> int64 array [rows padded][K]"""
    assert K % 16 == 0 and Cout > 0
    nb32 = (Cout + 31) // 32
    n = np.arange(nb32 * 32, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    step, blk, r = k // 16, n // 32, n % 32
    half = ((k % 16) // 8) ^ ((r >> 3) & 1)
    return ((step * nb32 + blk) * 32 + r) * 16 + half * 8 + k % 8


def pack(mat_planes, Cout, K):
    """(q, Cout, K) int16 planes of a matrix -> (q, packed_elems) in the packed order, rows >= Cout zero"""
    pos = torch.from_numpy(pack_layout(Cout, K)[:Cout].reshape(-1))
    out = torch.zeros(mat_planes.shape[0], packed_elems(Cout, K), dtype=torch.int16)
    out[:, pos] = mat_planes.reshape(mat_planes.shape[0], -1)
    return out


def flipped_matrix(w, scale):
    """w [Cout][KH][KW][Cin] fp32, scale [Cout] or None -> the data-gradient matrix [Cin][(KH-1-kh, KW-1-kw, co)] = w * scale[co], the
    product rounded once to fp32"""
    v = w.float() if scale is None else w.float() * scale.float().view(-1, 1, 1, 1)
    return v.flip(1, 2).permute(3, 1, 2, 0).contiguous()     # [Cin][KH][KW][Cout]


def row_blocked(planes, rows, W, C):
    """(q, rows * W * C) planes indexed like the NHWC tensor -> the same values in the order [rows][C / 16][W][16]"""
    q = planes.shape[0]
    return planes.reshape(q, rows, W, C // 16, 16).permute(0, 1, 3, 2, 4).reshape(q, -1).contiguous()


# ------------------------------------------------------------------------------------------ statistics
class Slot(object):
    """one 33-float statistics slot as the header words it: amax = max |x| (fp32, exact); sums[k] / counts[k], k < 16: the fp64 sum of
    |x| and the element count over the SAMPLE that goes into partial k; terms = the most values one thread adds, nblocks[k] = blocks
    that add into partial k (both only size the rounding bound of a test)"""

    def __init__(self):
        self.amax, self.sums, self.counts, self.terms, self.nblocks = 0.0, np.zeros(16), np.zeros(16), 0, np.zeros(16, dtype=np.int64)


def stats_blocks(n):
    return min((n // 4 + 255) // 256, 2048)


def stats_slot(x, blocks=None):
    """mmt_amax_stats / mmt_sum_stats over n = x.numel() values (n % 4 == 0): `blocks` = min(ceil(n / 4 / 256), 2048) blocks of 256
    threads; thread t of block b owns the float4 indices b 256 + t + j blocks 256; the sample is every block with b % 16 == 0, block b
    adding into partial (b >> 4) & 15"""
    a = x.reshape(-1).double().abs().numpy()
    n4 = a.size // 4
    blocks = stats_blocks(a.size) if blocks is None else blocks
    s = Slot()
    s.amax = float(a.max()) if a.size else 0.0
    per4 = a.reshape(n4, 4).sum(1)
    i = np.arange(n4, dtype=np.int64)
    b = (i // 256) % blocks
    s.terms = 4 * int(-(-n4 // (blocks * 256)))
    for blk in range(0, blocks, 16):
        sel = b == blk
        k = (blk >> 4) & 15
        s.sums[k] += per4[sel].sum()
        s.counts[k] += 4 * int(sel.sum())
        s.nblocks[k] += 1
    return s


def stats_slot_rb(y, rows, W, C):
    """mmt_sum_stats_rb: one block per (32 pixels of an image row, up to 256 channels); the grid is (rows * ceil(W / 32), ceil(C / 256));
    the sample is every block whose linear index lin = blockIdx.y * gridDim.x + blockIdx.x has lin % 16 == 0, into partial (lin >> 4) & 15"""
    a = y.reshape(rows, W, C).double().abs().numpy()
    segs, gx = (W + 31) // 32, rows * ((W + 31) // 32)
    s = Slot()
    s.amax = float(a.max()) if a.size else 0.0
    s.terms = 32
    for by in range((C + 255) // 256):
        for bx in range(gx):
            lin = by * gx + bx
            if lin % 16:
                continue
            row, w0, c0 = bx // segs, (bx % segs) * 32, by * 256
            part = a[row, w0:w0 + 32, c0:c0 + 256]
            k = (lin >> 4) & 15
            s.sums[k] += part.sum()
            s.counts[k] += part.size
            s.nblocks[k] += 1
    return s


def stats_combine(slots):
    """slots: list of n <= 8 float32 tensors of 33 -> out[0] = the largest maximum, out[i] = the sources' [i] added in order, from 0, in
    fp32.  A NaN maximum in any source gives a NaN maximum."""
    out = torch.zeros(33, dtype=torch.float32)
    for s in slots:
        s = s.float().cpu()
        out[1:] = out[1:] + s[1:]
        out[0] = s[0] if (torch.isnan(s[0]) or (not torch.isnan(out[0]) and s[0] > out[0])) else out[0]
    return out


def rb_scales_update(state):
    """state [n][2] fp32 = (scale, pending maximum) -> the same after the step's update: 0 < pending < 3e38 gives scale = the power of two
    that puts 2 x pending into [2^13, 2^14), anything else (0, inf, NaN, >= 3e38) keeps the scale; every pending word is cleared"""
    out = state.clone().float().cpu().reshape(-1, 2)
    for i in range(out.shape[0]):
        p = float(out[i, 1])
        if 0.0 < p < 3.0e38:
            out[i, 0] = f16_scale_of(p) * 0.5
        out[i, 1] = 0.0
    return out


# ------------------------------------------------------------------------------------------ seeded inputs
BF16_MAX = float.fromhex("0x1.fep127")


def wide_normals(n, seed):
    """random normals times 2^U[-40, 40]: normal fp32 numbers over 80 binades"""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(-40, 41, (n,), generator=g).float()
    return torch.randn(n, generator=g) * torch.exp2(e)


def edge_values():
    """exact bf16 and fp16 rounding ties (both parities of the kept mantissa), +-0, powers of two, the largest finite bf16, values one
    ulp either side of a tie -- all normal fp32 or zero"""
    v = []
    for k in (8, 9, 16, 17, 11, 12, 22, 23):                       # 1 + 2^-k and 1 + 3 2^-k: ties at the bf16 (k = 8), second term (16) ...
        for m in (1.0, 3.0):
            t = 1.0 + m * 2.0 ** -k
            v += [t, -t, float(np.nextafter(np.float32(t), np.float32(2))), float(np.nextafter(np.float32(t), np.float32(0)))]
    v += [2049.0, -2049.0, 2051.0, 4098.0, 4102.0, 2049.0 + 2.0 ** -11]   # fp16 ties: 11 significant bits, quantum 2 at 2048
    v += [0.0, -0.0, 1.0, -1.0, 2.0 ** -100, 2.0 ** 100, -2.0 ** 63, 2.0 ** -126, BF16_MAX, -BF16_MAX, 65504.0, 65519.0, 65520.0]
    out = torch.tensor(v, dtype=torch.float32)
    pad = (-out.numel()) % 8
    return torch.cat([out, torch.zeros(pad)])


def f16_tail_values(seed, amax=37.5):
    """one tensor with its maximum `amax` and values at 2^-15 ... 2^-30 of it (random mantissas, both signs): where the low fp16 term and
    then the high one turn subnormal under the tensor's own scale"""
    g = torch.Generator().manual_seed(seed)
    ks = torch.arange(15, 31).repeat_interleave(16).float()
    m = (1.0 + torch.rand(ks.numel(), generator=g)) * (torch.randint(0, 2, (ks.numel(),), generator=g) * 2 - 1).float()
    out = torch.cat([torch.tensor([amax, -amax * 0.75]), amax * m * torch.exp2(-ks - 1)])
    pad = (-out.numel()) % 8
    return torch.cat([out, torch.zeros(pad)])


def fp32_subnormals(n, seed):
    """fp32 subnormals (and a few normal neighbours): only |reconstruction - x| <= 2^-126 is asked of these"""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(1, 1 << 23, (n,), generator=g, dtype=torch.int32)
    bits[::7] += 1 << 23                                           # smallest normal binade
    sign = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32) * (-(1 << 31))
    return (bits | sign).view(torch.float32)


def mixed_values(n, seed):
    """n values (n % 8 == 0): the edge values, a tail tensor's values and wide normals, shuffled"""
    fixed = torch.cat([edge_values(), f16_tail_values(seed)])
    if n <= 8:
        g = torch.Generator().manual_seed(seed)
        return fixed[torch.randperm(fixed.numel(), generator=g)[:n]].contiguous()
    reps = torch.cat([fixed, wide_normals(max(n - fixed.numel(), 0), seed + 1)])[:n]
    g = torch.Generator().manual_seed(seed + 2)
    return reps[torch.randperm(n, generator=g)].contiguous()
