"""The references of tests/operand_prep_reference.py hold the properties include/mmtpsm.h promises of the operand-preparation kernels
(CPU only; tests/test_operand_prep_gpu.py compares the kernels with these references bit for bit)."""
import math

import numpy as np
import pytest
import torch

import operand_prep_reference as R

N = 1 << 20


def test_bf16x3_is_exact_where_the_third_term_is_representable():
    """fp32 carries 24 significant bits.  p0 = rne(x) keeps 8 of them, so x - p0 is a multiple of ulp32(x) no larger than 2^15 of them
    in magnitude (half a bf16 ulp): at most 16 significant bits, exact in fp32.  p1 keeps 8 of those, the rest is a multiple of ulp32(x)
    no larger than 2^7 of them: 8 bits, which p2 holds exactly -- as long as ulp32(x) >= 2^-133, the bf16 subnormal quantum, that is
    |x| >= 2^-110.  (The header promises <= 2^-27 |x|.)"""
    x = torch.cat([R.wide_normals(N, 1), R.edge_values(), R.f16_tail_values(3)])
    x = x[(x.abs() >= 2.0 ** -110) | (x == 0)]
    p = R.split_bf16x3(x).double()
    assert torch.equal(p.sum(0), x.double())
    # each term is the rounding of what is left: |x - p0| <= 2^-8 |x|, |x - p0 - p1| <= 2^-16 |x| (half an ulp of an 8-bit significand is at
    # most 2^-8 of the value)
    assert ((x.double() - p[0]).abs() <= 2.0 ** -8 * x.double().abs()).all()
    assert ((x.double() - p[0] - p[1]).abs() <= 2.0 ** -16 * x.double().abs()).all()
    # ties go to the even neighbour: 1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6
    t = R.split_bf16x3(torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8)])).double()
    assert t[0].tolist() == [1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6)]
    assert t[1].tolist() == [2.0 ** -8, -2.0 ** -8, -2.0 ** -8, 2.0 ** -8]


@pytest.mark.parametrize("amax", [1.0, 37.5, 2.0 ** 13, float(np.nextafter(np.float32(2.0 ** 13), np.float32(0))), 4.9, 1e-3, 2.0 ** -80, 2.0 ** 80])
def test_f16_scale_puts_the_maximum_into_the_top_binade(amax):
    """frexp gives amax = m 2^e with m in [0.5, 1): amax 2^(14 - e) = m 2^14 lies in [2^13, 2^14)"""
    s = R.f16_scale_of(amax)
    assert math.frexp(s)[0] == 0.5
    assert 2.0 ** 13 <= float(np.float32(amax)) * s <= 2.0 ** 14


def test_f16_scale_of_at_its_edges():
    assert R.f16_scale_of(0.0) == 1.0 and R.f16_scale_of(-3.0) == 1.0 and R.f16_scale_of(float("nan")) == 1.0
    assert R.f16_scale_of(2.0 ** -120) == 2.0 ** 100      # 14 + 119 clamps to 100
    assert R.f16_scale_of(3e38) == 2.0 ** -100            # 14 - 128 clamps to -100
    assert R.f16_scale_of(2.0 ** 13) == 1.0 and R.f16_scale_of(float(np.nextafter(np.float32(2.0 ** 13), np.float32(0)))) == 2.0


def test_f16x2_error_bound():
    """h = rne(r) leaves |r - h| <= 2^-11 |r| (11 significant bits).  While l = rne(r - h) is a normal fp16 number it leaves 2^-11 of
    that: |r - h - l| <= 2^-22 |r|.  Where |r - h| < 2^-14, l is subnormal, a multiple of the quantum 2^-24, and leaves at most half of
    it: 2^-25.  Hence |r - h - l| <= max(2^-22 |r|, 2^-25) for every |r| <= 65504."""
    x = torch.cat([torch.randn(N, generator=torch.Generator().manual_seed(5)), R.f16_tail_values(6, amax=4.0)])
    s = R.f16_scale_of(float(x.abs().max()))
    hl = R.split_f16x2(x, s).double()
    r = x.double() * s
    err = (r - hl[0] - hl[1]).abs()
    bound = torch.maximum(2.0 ** -22 * r.abs(), torch.tensor(2.0 ** -25, dtype=torch.float64))
    print("largest |r - h - l| / bound: %.3f" % float((err / bound).max()))
    assert (err <= bound).all()
    l = hl[1][:N]
    sub = ((l != 0) & (l.abs() < 2.0 ** -14)) | ((l == 0) & ((r[:N] - hl[0][:N]) != 0))
    frac = float(sub.double().mean())
    print("share of N(0,1) values whose low term is subnormal or lost: %.4f" % frac)
    assert frac > 1e-4       # the subnormal case is present in ordinary data
    # the tail values: h normal down to 2^-28 of the maximum, then subnormal; the bound holds throughout (asserted above), and the
    # values are not simply flushed: every tail value above 2^-38 of the maximum keeps a non-zero h
    tail = hl[0][N + 2:N + 2 + 256]
    assert (tail != 0).all()


def test_f16x2_saturates_and_never_overflows():
    x = torch.tensor([1e6, -1e6, 65519.0, 65520.0, 65504.0, 3e38, -3e38, float("inf"), -float("inf")])
    hl = R.split_f16x2(x, 16.0).float()
    assert torch.isfinite(hl).all()
    assert hl[0].abs().eq(65504.0).all() and hl[1].eq(0).all()


@pytest.mark.parametrize("Cout,K", [(33, 16), (64, 32), (80, 576), (15, 16)])
def test_pack_layout_is_a_bijection(Cout, K):
    pos = R.pack_layout(Cout, K)
    units = (K // 16) * ((Cout + 31) // 32)
    assert pos.shape == (32 * ((Cout + 31) // 32), K)
    assert np.array_equal(np.sort(pos.reshape(-1)), np.arange(units * 512))
    assert R.packed_elems(Cout, K) == units * 512
    # one lane's 8 elements are consecutive in k, a row's 16-k step is one 32-byte run with its halves swapped in rows 8-15 and 24-31
    assert np.array_equal(pos[0, :16], np.arange(16))
    assert np.array_equal(pos[8, :16], 8 * 16 + np.r_[np.arange(8, 16), np.arange(0, 8)])
    assert np.array_equal(pos[16, :16], 16 * 16 + np.arange(16))
    assert np.array_equal(pos[24, :16], 24 * 16 + np.r_[np.arange(8, 16), np.arange(0, 8)])
    # padding rows are zero in a packed plane
    m = torch.arange(1, Cout * K + 1, dtype=torch.int16).reshape(1, Cout, K)
    p = R.pack(m, Cout, K)
    assert int((p != 0).sum()) == Cout * K and torch.equal(p[0, torch.from_numpy(pos[:Cout].reshape(-1))], m.reshape(-1))


def test_flipped_matrix_and_row_blocked_orders():
    g = torch.Generator().manual_seed(9)
    w, sc = torch.randn(16, 3, 2, 5, generator=g), torch.randn(16, generator=g)
    f = R.flipped_matrix(w, sc)
    assert f.shape == (5, 3, 2, 16)
    assert f[4, 0, 1, 7] == w[7, 2, 0, 4] * sc[7]
    x = torch.arange(2 * 3 * 32, dtype=torch.int16).reshape(1, -1)          # rows 2, W 3, C 32
    rb = R.row_blocked(x, 2, 3, 32).reshape(2, 2, 3, 16)
    assert rb[1, 1, 2, 5] == (1 * 3 + 2) * 32 + 16 + 5


def test_stats_slot_samples_every_sixteenth_block():
    n = 4 * 256 * 257
    x = torch.arange(1, n + 1, dtype=torch.float32)
    s = R.stats_slot(x)
    assert R.stats_blocks(n) == 257 and s.amax == n
    # blocks 0 and 256 -> partial 0, block 16 -> partial 1, ... 240 -> 15; one trip each: 1024 values per block
    assert s.counts.tolist() == [2048.0] + [1024.0] * 15 and s.nblocks.tolist() == [2] + [1] * 15 and s.terms == 4
    blk = lambda b: float(torch.arange(b * 1024 + 1, b * 1024 + 1025, dtype=torch.float64).sum())
    assert s.sums[0] == blk(0) + blk(256) and s.sums[1] == blk(16)
    s = R.stats_slot(torch.ones(4 * 256 * 2048 + 4))    # above the cap: thread 0 of block 0 takes a second trip
    assert s.counts[0] == 8 * 1024 + 4 and s.counts[1] == 8 * 1024 and s.terms == 8
    s = R.stats_slot_rb(torch.ones(2 * 40 * 272), 2, 40, 272)   # grid (4, 2): lin 0 samples 32 x 256, nothing else
    assert s.counts.tolist() == [32.0 * 256] + [0.0] * 15


def test_stats_combine_and_scales_update():
    a, b = torch.zeros(33), torch.zeros(33)
    a[0], b[0], a[1], b[1], a[17], b[17] = 3.0, 5.0, 0.1, 0.2, 4.0, 8.0
    out = R.stats_combine([a, b])
    assert out[0] == 5.0 and out[1] == torch.tensor(0.1) + torch.tensor(0.2) and out[17] == 12.0
    b[0] = float("nan")
    assert torch.isnan(R.stats_combine([a, b])[0]) and torch.isnan(R.stats_combine([b, a])[0])
    st = torch.tensor([[7.0, 0.0], [7.0, 1.0], [7.0, 2.0 ** -120], [7.0, 3.1e38], [7.0, float("inf")], [7.0, float("nan")]])
    out = R.rb_scales_update(st)
    assert out[:, 1].eq(0).all()
    assert out[:, 0].tolist() == [7.0, 2.0 ** 12, 2.0 ** 99, 7.0, 7.0, 7.0]   # 2 x 1.0 -> [2^13, 2^14): 2^12


def test_builders_are_seeded_and_normal():
    for f in (lambda: R.mixed_values(4096, 3), lambda: R.wide_normals(64, 1), lambda: R.f16_tail_values(2), lambda: R.fp32_subnormals(64, 4)):
        assert torch.equal(R.bits32(f()), R.bits32(f()))
    for v in (R.mixed_values(8 * 256 + 8, 3), R.edge_values(), R.f16_tail_values(2)):
        assert v.numel() % 8 == 0 and ((v == 0) | (v.abs() >= 2.0 ** -126)).all() and torch.isfinite(v).all()
    sub = R.fp32_subnormals(64, 4)
    assert (sub.abs() < 2.0 ** -125).all() and (sub != 0).all() and (sub.abs() < 2.0 ** -126).any()
