"""The operand-preparation kernels (csrc/conv_prep.hip, the passes of csrc/conv_pgemm.hip) against tests/operand_prep_reference.py, BIT FOR
BIT: planes compare as int16, scales and maxima as int32.  Inputs of the bit-exact comparisons are normal fp32 numbers and zeros; of
fp32 subnormals only |reconstruction - x| <= 2^-126 is asked of the bf16 split (TINY, as in tests/test_loss_optim_edges_gpu.py), and
2^-25 of the scaled value of the fp16 split, whose scale stops at 2^100.

Sizes: one thread (n = 8), a second block holding one item, and the smallest size above each entry point's grid cap, where the
grid-stride loop takes a second trip.  The only derived tolerance is the one on the sampled sums of the statistics slots (see
_check_slot): every other assertion is an equality."""
import ctypes

import numpy as np
import pytest
import torch

import operand_prep_reference as R

pytestmark = pytest.mark.gpu

EINVAL = -22
U = 2.0 ** -24
TINY = 2.0 ** -126
FILL = 0x5a5a          # what a plane buffer holds before a call: a gap must still hold it afterwards
WORST = {}             # largest measured error / bound per check, printed by the tests


@pytest.fixture(scope="module")
def hip():
    from maskrcnn_benchmark import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return _hip


def call(H, name, *args):
    rc = getattr(H.lib(), name)(*args, H._stream())
    torch.cuda.synchronize()
    return rc


def word(v):
    """a device float holding v"""
    return torch.tensor([v], dtype=torch.float32).cuda()


def planes_buf(q, stride):
    return torch.full((q, stride), FILL, dtype=torch.int16, device="cuda")


def same_bits16(got, want):
    got, want = got.cpu(), want.cpu()
    bad = (got != want).nonzero()
    assert bad.numel() == 0, "%d of %d words differ, first at %s: got %s want %s" % (
        bad.shape[0], want.numel(), bad[0].tolist(), hex(int(got[tuple(bad[0])]) & 0xffff), hex(int(want[tuple(bad[0])]) & 0xffff))


def same_bits32(got, want):
    got, want = R.bits32(torch.as_tensor(got).cpu()), R.bits32(torch.as_tensor(want))
    assert torch.equal(got.reshape(-1), want.reshape(-1)), (got.reshape(-1)[:8].tolist(), want.reshape(-1)[:8].tolist())


def values(n, seed):
    return R.mixed_values(n, seed) if n <= (1 << 16) else R.wide_normals(n, seed)


def stat_values(n, seed):
    """normals times 2^U[-8, 8]: sums and maxima that mean something"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * torch.exp2(torch.randint(-8, 9, (n,), generator=g).float())


def weights(n, seed):
    """mixed values whose product with a scale in [0.5, 2) stays a normal fp32 number: magnitudes folded into [2^-60, 2^60]"""
    v = R.mixed_values(n, seed)
    v = torch.where(v.abs() > 2.0 ** 60, torch.sign(v) * 1.5, v)
    return torch.where((v != 0) & (v.abs() < 2.0 ** -60), torch.sign(v) * 1.25 * 2.0 ** -60, v)


def row_scale(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.5 + 1.5 * torch.rand(n, generator=g)) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()


# ------------------------------------------------------------------------------------------ split passes
@pytest.mark.parametrize("n,gap", [(8, 0), (8, 8), (8 * 256 + 8, 24), (8 * 256 * 8192 + 8, 0)])
def test_split_planes_bf16(hip, n, gap):
    x = values(n, 11)
    pl = planes_buf(3, n + gap)
    assert call(hip, "mmt_split_planes", x.cuda().data_ptr(), pl.data_ptr(), n + gap, n) == 0
    same_bits16(pl[:, :n], R.bits16(R.split_bf16x3(x)))
    assert (pl[:, n:] == FILL).all()


@pytest.mark.parametrize("n,gap", [(8, 0), (8 * 256 + 8, 24), (8 * 256 * 2048 + 8, 0)])
@pytest.mark.parametrize("over", [1.0, 16.0])
def test_split_planes_f16_host_scale(hip, n, gap, over):
    """over = 16: a scale 16 x too large (a stale one) saturates to +-65504 with a zero low term, never inf"""
    x = values(n, 12)
    if n > (1 << 16):
        x = x * 2.0 ** -30     # (wide normals reach 2^42: keep x s finite in fp32 so that the comparison is about the split)
    s = R.f16_scale_of(float(x.abs().max())) * over
    pl = planes_buf(2, n + gap)
    assert call(hip, "mmt_split_planes_f16", x.cuda().data_ptr(), pl.data_ptr(), n + gap, n, s, None, None, None, None) == 0
    want = R.split_f16x2(x, s)
    same_bits16(pl[:, :n], R.bits16(want))
    assert (pl[:, n:] == FILL).all()
    got = pl[:, :n].cpu().view(torch.float16).float()
    assert torch.isfinite(got).all()
    sat = (x.double() * s).abs() >= 65504.0
    assert (got[0][sat].abs() == 65504.0).all() and (got[1][sat] == 0).all()
    if over > 1 and n > 8:
        assert sat.any()


AMAX_WORDS = [0.0, 2.0 ** 13, float(np.nextafter(np.float32(2.0 ** 13), np.float32(0))), 1.0, 37.5, 2.0 ** -120, 2.0 ** -140, 3e38]


@pytest.mark.parametrize("amax", AMAX_WORDS)
def test_split_planes_f16_device_amax(hip, amax):
    """the scale derived on the device from *amax (any word, not necessarily this tensor's maximum), and the delayed-scaling triple:
    amax_next receives this tensor's maximum, zero_slot is zeroed"""
    n = 8 * 256 + 8
    x = values(n, 13)
    pl = planes_buf(2, n)
    st = torch.tensor([-1.0, 0.0, 5.0], dtype=torch.float32).cuda()      # scale_out, amax_next, zero_slot
    am = word(amax)
    assert call(hip, "mmt_split_planes_f16", x.cuda().data_ptr(), pl.data_ptr(), n, n, 1.0, am.data_ptr(), st.data_ptr(),
                st.data_ptr() + 4, st.data_ptr() + 8) == 0
    s = R.f16_scale_of(amax)
    same_bits32(st, [s, float(x.abs().max()), 0.0])
    same_bits16(pl, R.bits16(R.split_f16x2(x, s)))
    assert torch.isfinite(pl.cpu().view(torch.float16).float()).all()


def test_split_planes_f16_stale_device_amax_saturates(hip):
    """the maximum a scale is derived from may be an older tensor's: one 16 x too small gives a scale 16 x too large, and what leaves the
    fp16 range saturates to +-65504 with a zero low term -- never inf"""
    n = 8 * 256 + 8
    x = stat_values(n, 16)
    amax = float(x.abs().max()) / 16.0
    pl, st = planes_buf(2, n), word(-1.0)
    assert call(hip, "mmt_split_planes_f16", x.cuda().data_ptr(), pl.data_ptr(), n, n, 1.0, word(amax).data_ptr(), st.data_ptr(), None, None) == 0
    s = R.f16_scale_of(amax)
    assert s == 16.0 * R.f16_scale_of(float(x.abs().max()))
    same_bits32(st, [s])
    same_bits16(pl, R.bits16(R.split_f16x2(x, s)))
    got = pl.cpu().view(torch.float16).float()
    sat = (x.double() * s).abs() >= 65504.0
    assert sat.any() and torch.isfinite(got).all()
    assert (got[0][sat].abs() == 65504.0).all() and (got[1][sat] == 0).all()


@pytest.mark.parametrize("rows,W,C", [(3, 5, 16), (2, 33, 272), (386, 40, 272)])
def test_split_planes_f16_rb(hip, rows, W, C):
    """both kernels: the one-trip form and, above 2^22 elements, the LDS form (W not a multiple of 32, a second channel block of 16);
    the planes start as NaN patterns: every element is written"""
    n = rows * W * C
    assert (n > (1 << 22)) == (rows == 386)
    x = values(n, 14) if n <= (1 << 16) else R.wide_normals(n, 14) * 2.0 ** -30
    gap = 8 if n <= (1 << 16) else 0
    pl = torch.full((2, n + gap), 0x7fff, dtype=torch.int16, device="cuda")
    amax = float(x.abs().max())
    st = word(-1.0)
    assert call(hip, "mmt_split_planes_f16_rb", x.cuda().data_ptr(), pl.data_ptr(), n + gap, rows, W, C, word(amax).data_ptr(),
                st.data_ptr()) == 0
    s = R.f16_scale_of(amax)
    same_bits32(st, [s])
    same_bits16(pl[:, :n], R.row_blocked(R.bits16(R.split_f16x2(x, s)), rows, W, C))
    assert (pl[:, n:] == 0x7fff).all()


def test_bf16_split_of_fp32_subnormals_loses_at_most_the_smallest_normal(hip):
    n = 16 * 64
    x = R.fp32_subnormals(n, 15)
    pl = planes_buf(3, n)
    assert call(hip, "mmt_split_planes", x.cuda().data_ptr(), pl.data_ptr(), n, n) == 0
    rec = pl.cpu().view(torch.bfloat16).double().sum(0)
    assert ((rec - x.double()).abs() <= TINY).all()


@pytest.mark.parametrize("kind", ["f16", "f16_rb"])
def test_f16_split_of_fp32_subnormals(hip, kind):
    """The fp16 forms cannot promise 2^-126 for such a tensor: the scale's exponent is clamped to 2^100, so a tensor whose maximum is
    below 2^-100 2^13 is not lifted into the top binade, and values below 2^-125 land under half the fp16 subnormal quantum.  What the
    split promises in scaled units, |r - h - l| <= 2^-25, is 2^-25 / s here; the planes still equal the reference bit for bit."""
    n = 16 * 64
    x = R.fp32_subnormals(n, 15)
    amax = float(x.abs().max())
    s = R.f16_scale_of(amax)
    assert s == 2.0 ** 100
    pl, st = planes_buf(2, n), word(-1.0)
    if kind == "f16":
        assert call(hip, "mmt_split_planes_f16", x.cuda().data_ptr(), pl.data_ptr(), n, n, 1.0, word(amax).data_ptr(), st.data_ptr(), None, None) == 0
        want = R.bits16(R.split_f16x2(x, s))
    else:
        assert call(hip, "mmt_split_planes_f16_rb", x.cuda().data_ptr(), pl.data_ptr(), n, 1, 64, 16, word(amax).data_ptr(), st.data_ptr()) == 0
        want = R.row_blocked(R.bits16(R.split_f16x2(x, s)), 1, 64, 16)
    same_bits32(st, [s])
    same_bits16(pl, want)
    rec = pl.cpu().view(torch.float16).double().sum(0) / s
    if kind == "f16_rb":
        rec = rec.reshape(1, 1, 64, 16).permute(0, 2, 1, 3).reshape(-1)
    assert ((rec - x.double()).abs() <= max(TINY, 2.0 ** -25 / s)).all()


# ------------------------------------------------------------------------------------------ packed weight planes
FWD = [(33, 16), (64, 32), (80, 576), (15, 16)]
FLIP = [(16, 1, 1, 33), (48, 3, 3, 40), (64, 7, 7, 16)]


def _packed_ref(mat, f16_scale=None):
    """mat [rows][K] fp32 -> the packed planes the kernels must write"""
    rows, K = mat.shape
    pl = R.split_bf16x3(mat) if f16_scale is None else R.split_f16x2(mat, f16_scale)
    return R.pack(R.bits16(pl).reshape(-1, rows, K), rows, K)


@pytest.mark.parametrize("Cout,K", FWD)
def test_pack_weight_forward(hip, Cout, K):
    w = weights(Cout * K, 20 + Cout).reshape(Cout, K)
    n = R.packed_elems(Cout, K)
    assert hip.lib().mmt_packed_weight_elems(Cout, K) == n
    wd = w.cuda()
    pl = planes_buf(3, n + 8)
    assert call(hip, "mmt_pack_weight", wd.data_ptr(), pl.data_ptr(), n + 8, Cout, K) == 0
    same_bits16(pl[:, :n], _packed_ref(w))
    assert (pl[:, n:] == FILL).all()
    amax = float(w.abs().max())
    for host in (True, False):      # the scale from the host, or derived from a device maximum and written to scale_out
        pl, st = planes_buf(2, n + 8), word(-1.0)
        s = R.f16_scale_of(amax)
        assert call(hip, "mmt_pack_weight_f16", wd.data_ptr(), pl.data_ptr(), n + 8, Cout, K, s if host else 1.0,
                    None if host else word(amax).data_ptr(), st.data_ptr()) == 0
        same_bits32(st, [s])
        same_bits16(pl[:, :n], _packed_ref(w, s))
        assert (pl[:, n:] == FILL).all()


@pytest.mark.parametrize("Cout,KH,KW,Cin", FLIP)
@pytest.mark.parametrize("scaled", [False, True])
def test_pack_weight_flipped(hip, Cout, KH, KW, Cin, scaled):
    w = weights(Cout * KH * KW * Cin, 30 + Cin).reshape(Cout, KH, KW, Cin)
    sc = row_scale(Cout, 31) if scaled else None
    assert sc is None or (sc < 0).any()
    mat = R.flipped_matrix(w, sc).reshape(Cin, KH * KW * Cout)
    n = R.packed_elems(Cin, KH * KW * Cout)
    wd, sd = w.cuda(), None if sc is None else sc.cuda()
    pl = planes_buf(3, n + 8)
    assert call(hip, "mmt_pack_weight_flipped", wd.data_ptr(), hip._p(sd), pl.data_ptr(), n + 8, Cout, KH, KW, Cin) == 0
    same_bits16(pl[:, :n], _packed_ref(mat))
    assert (pl[:, n:] == FILL).all()
    amax = float(mat.abs().max())
    pl, st = planes_buf(2, n + 8), word(-1.0)
    assert call(hip, "mmt_pack_weight_flipped_f16", wd.data_ptr(), hip._p(sd), pl.data_ptr(), n + 8, Cout, KH, KW, Cin,
                word(amax).data_ptr(), st.data_ptr()) == 0
    s = R.f16_scale_of(amax)
    same_bits32(st, [s])
    same_bits16(pl[:, :n], _packed_ref(mat, s))
    assert (pl[:, n:] == FILL).all()


def _dev_bytes(a):
    return torch.from_numpy(np.frombuffer(a.tobytes(), dtype=np.uint8).copy()).cuda()


def test_pack_weights_batched_forward(hip):
    """one table of four matrices (one with Cout % 32 != 0 first, so that the first wave's run of 32 units crosses three matrices;
    one maximum in the last element in memory): planes equal the single-matrix entry points bit for bit, stat = (max, its scale)"""
    dims = [(33, 16), (64, 32), (80, 576), (15, 16)]
    mats = [weights(c * k, 40 + i).reshape(c, k) * 10.0 ** (i - 2) for i, (c, k) in enumerate(dims)]
    mats[2][-1, -1] = 3.0 * float(mats[2].abs().max())
    base = torch.cat([m.reshape(-1) for m in mats]).cuda()
    desc = np.zeros(4, dtype=np.dtype([("src", "<i8"), ("dst", "<i8"), ("Cout", "<i4"), ("K", "<i4"), ("unit0", "<i4"), ("pad", "<i4")]))
    assert desc.dtype.itemsize == 32
    src = dst = unit = 0
    unit_desc = []
    for i, (c, k) in enumerate(dims):
        desc[i] = (src, dst, c, k, unit, 0)
        src, dst = src + c * k, dst + R.packed_elems(c, k)
        unit_desc += [i] * (R.packed_elems(c, k) // 512)
        unit += R.packed_elems(c, k) // 512
    assert unit > 32 and len(set(unit_desc[:32])) == 3
    dd, ud = _dev_bytes(desc), torch.tensor(unit_desc, dtype=torch.int32).cuda()
    stride = dst + 8
    pl = planes_buf(3, stride)
    assert call(hip, "mmt_pack_weights", base.data_ptr(), pl.data_ptr(), stride, dd.data_ptr(), ud.data_ptr(), unit) == 0
    pf, stat = planes_buf(2, stride), torch.full((4, 2), -1.0, device="cuda")
    assert call(hip, "mmt_pack_weights_f16", base.data_ptr(), pf.data_ptr(), stride, dd.data_ptr(), ud.data_ptr(), unit, 4, stat.data_ptr()) == 0
    assert (pl[:, dst:] == FILL).all() and (pf[:, dst:] == FILL).all()
    for i, (c, k) in enumerate(dims):
        n, off = R.packed_elems(c, k), int(desc[i]["dst"])
        amax = float(mats[i].abs().max())
        same_bits32(stat[i], [amax, R.f16_scale_of(amax)])
        one, onef = planes_buf(3, n), planes_buf(2, n)
        wd = mats[i].cuda()
        assert call(hip, "mmt_pack_weight", wd.data_ptr(), one.data_ptr(), n, c, k) == 0
        assert call(hip, "mmt_pack_weight_f16", wd.data_ptr(), onef.data_ptr(), n, c, k, 1.0, word(amax).data_ptr(), None) == 0
        same_bits16(pl[:, off:off + n], one)
        same_bits16(pf[:, off:off + n], onef)
        same_bits16(one, _packed_ref(mats[i]))
        same_bits16(onef, _packed_ref(mats[i], R.f16_scale_of(amax)))


def test_pack_weights_batched_flipped(hip):
    """the data-gradient table: a matrix whose row length is no multiple of 8 (the scalar branch of the maximum), scales with negative
    entries and none, a maximum in the last element in memory, a wave's run of 32 units across three matrices"""
    dims = [(16, 3, 3, 3), (16, 1, 1, 33), (48, 3, 3, 40), (64, 7, 7, 16)]
    ws = [weights(int(np.prod(d)), 50 + i).reshape(d) * 10.0 ** (i - 2) for i, d in enumerate(dims)]
    ws[0][-1, -1, -1, -1] = 3.0 * float(ws[0].abs().max())
    scs = [row_scale(16, 51), None, row_scale(48, 52), None]
    wd = [w.cuda() for w in ws]
    sd = [None if s is None else s.cuda() for s in scs]
    desc = np.zeros(4, dtype=np.dtype([("w", "<u8"), ("scale", "<u8"), ("dst", "<u8"), ("stride", "<i8"), ("Cout", "<i4"), ("KH", "<i4"),
                                       ("KW", "<i4"), ("Cin", "<i4"), ("unit0", "<i4"), ("pad", "<i4")]))
    assert desc.dtype.itemsize == 56
    unit, unit_desc, bufs = 0, [], []
    for f16 in (False, True):
        unit, unit_desc, bufs = 0, [], []
        for i, (co, kh, kw, ci) in enumerate(dims):
            n = R.packed_elems(ci, kh * kw * co)
            bufs.append(planes_buf(2 if f16 else 3, n + 8))
            desc[i] = (wd[i].data_ptr(), 0 if sd[i] is None else sd[i].data_ptr(), bufs[i].data_ptr(), n + 8, co, kh, kw, ci, unit, 0)
            unit_desc += [i] * (n // 512)
            unit += n // 512
        assert len(set(unit_desc[:32])) == 3
        dd, ud = _dev_bytes(desc), torch.tensor(unit_desc, dtype=torch.int32).cuda()
        stat = torch.full((4, 2), -1.0, device="cuda")
        if f16:
            assert call(hip, "mmt_pack_weights_flipped_f16", dd.data_ptr(), ud.data_ptr(), unit, 4, stat.data_ptr()) == 0
        else:
            assert call(hip, "mmt_pack_weights_flipped", dd.data_ptr(), ud.data_ptr(), unit) == 0
        for i, (co, kh, kw, ci) in enumerate(dims):
            n = R.packed_elems(ci, kh * kw * co)
            mat = R.flipped_matrix(ws[i], scs[i]).reshape(ci, kh * kw * co)
            amax = float(mat.abs().max())
            one = planes_buf(2 if f16 else 3, n)
            if f16:
                same_bits32(stat[i], [amax, R.f16_scale_of(amax)])
                assert call(hip, "mmt_pack_weight_flipped_f16", wd[i].data_ptr(), hip._p(sd[i]), one.data_ptr(), n, co, kh, kw, ci,
                            word(amax).data_ptr(), None) == 0
            else:
                assert call(hip, "mmt_pack_weight_flipped", wd[i].data_ptr(), hip._p(sd[i]), one.data_ptr(), n, co, kh, kw, ci) == 0
            same_bits16(bufs[i][:, :n], one)
            assert (bufs[i][:, n:] == FILL).all()
            same_bits16(one, _packed_ref(mat, R.f16_scale_of(amax) if f16 else None))


@pytest.mark.parametrize("Cout,KH,KW,Cin", [(15, 1, 1, 33), (40, 3, 3, 12)])
@pytest.mark.parametrize("scaled", [False, True])
def test_weight_flip_transpose(hip, Cout, KH, KW, Cin, scaled):
    w = weights(Cout * KH * KW * Cin, 60).reshape(Cout, KH, KW, Cin)
    sc = row_scale(Cout, 61) if scaled else None
    out = torch.full((Cin, KH, KW, Cout), 7.0, device="cuda")
    assert call(hip, "mmt_weight_flip_transpose", w.cuda().data_ptr(), None if sc is None else sc.cuda().data_ptr(), out.data_ptr(),
                Cout, KH, KW, Cin) == 0
    same_bits32(out, R.flipped_matrix(w, sc))


# ------------------------------------------------------------------------------------------ maxima and statistics slots
@pytest.mark.parametrize("n", [4, 4 * 256 + 4, 4 * 256 * 2048 + 4])
def test_amax_is_exact_and_accumulates(hip, n):
    x = stat_values(n, 70)
    xd = x.cuda()
    want = float(x.abs().max())
    for start in (0.0, want * 0.5, want * 2.0):      # it accumulates onto the word, keeping the larger value
        am = word(start)
        assert call(hip, "mmt_amax", xd.data_ptr(), n, None, 0, 0, am.data_ptr()) == 0
        same_bits32(am, [max(start, want)])


@pytest.mark.parametrize("inner", [4, 36])
@pytest.mark.parametrize("rows", [1, 3])
def test_amax_with_rowscale(hip, inner, rows):
    """max |x[i] rowscale[(i / inner) % rows]|: the product is rounded to fp32, the sign of the scale does not matter"""
    n = inner * rows * 59
    x, rs = stat_values(n, 71), row_scale(rows, 72) * torch.tensor([1.0, 100.0, 0.01])[:rows]
    rs[0] = -rs[0].abs()
    want = (x.reshape(-1, rows, inner) * rs.view(1, rows, 1)).abs().max()
    am = word(0.0)
    assert call(hip, "mmt_amax", x.cuda().data_ptr(), n, rs.cuda().data_ptr(), inner, rows, am.data_ptr()) == 0
    same_bits32(am, [float(want)])


def _check_slot(name, slot, want):
    """slot: 33 floats from the device; want: R.Slot.  Maximum and counts exact.  A sampled sum adds non-negative numbers, so its
    relative error is at most the number of roundings on the longest path from a term to the result times 2^-24: the T terms a thread
    adds, the 6 shuffle stages of a wave, the B blocks that add into the partial: (T + 6 + B) 2^-24.
    Largest error / bound measured on an MI355X over the cases of this file: mmt_amax_stats 0.167, mmt_sum_stats 0.173,
    mmt_sum_stats_rb 0.043."""
    slot = slot.cpu()
    same_bits32(slot[0], [want.amax])
    assert slot[17:33].double().tolist() == want.counts.tolist(), (slot[17:33].tolist(), want.counts.tolist())
    for k in range(16):
        if want.counts[k] == 0:
            assert slot[1 + k] == 0
            continue
        bound = (want.terms + 6 + int(want.nblocks[k])) * U * want.sums[k]
        err = abs(float(slot[1 + k].double()) - want.sums[k])
        WORST[name] = max(WORST.get(name, 0.0), err / bound if bound > 0 else 0.0)
        assert err <= bound, (k, float(slot[1 + k]), want.sums[k], err / bound)
    print("%s: largest error of a sampled sum / bound so far %.3f" % (name, WORST.get(name, 0.0)))


# n = 4: one float4; 17 blocks: block 16 samples one float4 into partial 1; 257 blocks: partial 0 gets blocks 0 and 256; above the cap
STAT_SIZES = [4, 4 * (16 * 256 + 1), 4 * (256 * 256 + 1), 4 * 256 * 2048 + 4]


@pytest.mark.parametrize("n", STAT_SIZES)
def test_amax_stats(hip, n):
    x = stat_values(n, 73)
    slot = torch.zeros(33, device="cuda")
    assert call(hip, "mmt_amax_stats", x.cuda().data_ptr(), n, slot.data_ptr()) == 0
    _check_slot("amax_stats", slot, R.stats_slot(x))


@pytest.mark.parametrize("n", STAT_SIZES)
@pytest.mark.parametrize("terms", [2, 3, 4, "alias"])
def test_sum_stats(hip, n, terms):
    ts = [stat_values(n, 74 + i) for i in range(2 if terms == "alias" else terms)]
    y = (ts[0] + ts[1])
    for t in ts[2:]:
        y = y + t
    td = [t.cuda() for t in ts]
    out = td[0] if terms == "alias" else torch.full((n,), 9.0, device="cuda")
    ptrs = [t.data_ptr() for t in td] + [None] * (4 - len(td))
    slot = torch.zeros(33, device="cuda")
    assert call(hip, "mmt_sum_stats", ptrs[0], ptrs[1], ptrs[2], ptrs[3], out.data_ptr(), n, slot.data_ptr()) == 0
    same_bits32(out, y)
    _check_slot("sum_stats", slot, R.stats_slot(y))


@pytest.mark.parametrize("rows,W,C", [(3, 5, 16), (2, 33, 272), (130, 40, 272)])
@pytest.mark.parametrize("terms", [2, 4])
@pytest.mark.parametrize("planes", [True, False])
def test_sum_stats_rb(hip, rows, W, C, terms, planes):
    """(130, 40, 272): a grid of (260, 2) blocks -- the sample is every 16th LINEAR block index, blocks 0 and 256 meet in partial 0, the
    second grid row holds the 16-channel blocks"""
    n = rows * W * C
    ts = [stat_values(n, 80 + i) for i in range(terms)]
    y = ts[0] + ts[1]
    for t in ts[2:]:
        y = y + t
    td = [t.cuda() for t in ts]
    ptrs = [t.data_ptr() for t in td] + [None] * (4 - len(td))
    out, slot, nxt = torch.full((n,), 9.0, device="cuda"), torch.zeros(33, device="cuda"), word(0.0)
    s = R.f16_scale_of(float(y.abs().max())) * 0.5       # a producing site's scale: one binade of head-room
    pl = torch.full((2, n + 8), 0x7fff, dtype=torch.int16, device="cuda")
    assert call(hip, "mmt_sum_stats_rb", ptrs[0], ptrs[1], ptrs[2], ptrs[3], out.data_ptr(), rows, W, C, slot.data_ptr(),
                pl.data_ptr() if planes else None, n + 8 if planes else 0, word(s).data_ptr(), nxt.data_ptr()) == 0
    same_bits32(out, y)
    _check_slot("sum_stats_rb", slot, R.stats_slot_rb(y, rows, W, C))
    same_bits32(nxt, slot[:1].cpu())
    if planes:
        same_bits16(pl[:, :n], R.row_blocked(R.bits16(R.split_f16x2(y, s)), rows, W, C))
        assert (pl[:, n:] == 0x7fff).all()
    else:
        assert (pl == 0x7fff).all()


@pytest.mark.parametrize("n", [1, 3, 8])
def test_stats_combine(hip, n):
    g = torch.Generator().manual_seed(90 + n)
    slots = [torch.cat([torch.rand(17, generator=g) * 10.0 ** i, torch.randint(1, 5000, (16,), generator=g).float()]) for i in range(n)]
    dev = [s.cuda() for s in slots]
    arr = (ctypes.c_void_p * n)(*[d.data_ptr() for d in dev])
    out = torch.full((33,), -1.0, device="cuda")
    assert call(hip, "mmt_stats_combine", arr, n, out.data_ptr()) == 0
    same_bits32(out, R.stats_combine(slots))


def test_stats_combine_refuses_no_slot_and_more_than_eight(hip):
    dev = [torch.zeros(33, device="cuda") for _ in range(9)]
    arr = (ctypes.c_void_p * 9)(*[d.data_ptr() for d in dev])
    out = torch.full((33,), -1.0, device="cuda")
    assert call(hip, "mmt_stats_combine", arr, 0, out.data_ptr()) == EINVAL
    assert call(hip, "mmt_stats_combine", arr, 9, out.data_ptr()) == EINVAL
    assert (out == -1.0).all()


def test_stats_combine_keeps_a_nan_maximum(hip):
    """a NaN maximum in any source gives a NaN maximum (the consumer's range guard then takes the exact path), wherever it stands"""
    for where in (0, 1, 2):
        slots = [torch.ones(33) * (i + 1) for i in range(3)]
        slots[where][0] = float("nan")
        dev = [s.cuda() for s in slots]
        arr = (ctypes.c_void_p * 3)(*[d.data_ptr() for d in dev])
        out = torch.full((33,), -1.0, device="cuda")
        assert call(hip, "mmt_stats_combine", arr, 3, out.data_ptr()) == 0
        assert torch.isnan(out[0]).item(), where
        same_bits32(out[1:], R.stats_combine(slots)[1:])


@pytest.mark.parametrize("n", [1, 257])
def test_rb_scales_update(hip, n):
    """pending 0 keeps its scale; 1.0 and 2^-120 (exponent clamp) give new ones; 3.1e38, inf and NaN keep the old scale; every pending
    word is cleared"""
    pend = [0.0, 1.0, 2.0 ** -120, 3.1e38, float("inf"), float("nan"), 37.5, 2.0 ** 13]
    st = torch.tensor([[7.0 + i, pend[(i + (n == 1)) % len(pend)]] for i in range(n)], dtype=torch.float32)
    dev = torch.cat([st.reshape(-1), torch.tensor([-3.0, -3.0])]).cuda()
    assert call(hip, "mmt_rb_scales_update", dev.data_ptr(), n) == 0
    same_bits32(dev[:2 * n], R.rb_scales_update(st))
    assert (dev[2 * n:] == -3.0).all()
    if n > 1:
        for p in pend:
            one = torch.tensor([5.0, p]).cuda()
            assert call(hip, "mmt_rb_scales_update", one.data_ptr(), 1) == 0
            same_bits32(one, R.rb_scales_update(torch.tensor([[5.0, p]])))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_maxima_and_split_passes_keep_a_nonfinite_value(hip, bad):
    """one NaN or inf in a tensor: every recorded maximum is that value's magnitude (NaN orders above inf), and the fp16 split passes
    leave the value as it is -- the clamp is for finite values under a stale scale -- with every other element as the reference has it"""
    n = 4 * 256 * 3
    x = stat_values(n, 97)
    x[n - 3] = bad
    xd = x.cuda()
    want_nan, am, slot, slot2 = bad != bad, word(0.0), torch.zeros(33, device="cuda"), torch.zeros(33, device="cuda")
    assert call(hip, "mmt_amax", xd.data_ptr(), n, None, 0, 0, am.data_ptr()) == 0
    assert call(hip, "mmt_amax_stats", xd.data_ptr(), n, slot.data_ptr()) == 0
    y = torch.empty(n, device="cuda")
    assert call(hip, "mmt_sum_stats", xd.data_ptr(), torch.zeros(n, device="cuda").data_ptr(), None, None, y.data_ptr(), n, slot2.data_ptr()) == 0
    for m in (am[0], slot[0], slot2[0]):
        assert bool(torch.isnan(m)) if want_nan else float(m) == float("inf")
    rows, W, C = 3, 16, 64
    for kind in ("f16", "rb"):
        pl, st = planes_buf(2, n), word(-1.0)
        if kind == "f16":
            assert call(hip, "mmt_split_planes_f16", xd.data_ptr(), pl.data_ptr(), n, n, 1.0, word(4.0).data_ptr(), st.data_ptr(), None, None) == 0
        else:
            assert call(hip, "mmt_split_planes_f16_rb", xd.data_ptr(), pl.data_ptr(), n, rows, W, C, word(4.0).data_ptr(), st.data_ptr()) == 0
        s = R.f16_scale_of(4.0)
        got = pl.cpu()
        if kind == "rb":
            got = got.reshape(2, rows, C // 16, W, 16).permute(0, 1, 3, 2, 4).reshape(2, n)
        want = R.bits16(R.split_f16x2(torch.where(torch.isfinite(x), x, torch.zeros(())), s))
        keep = torch.ones(n, dtype=torch.bool)
        keep[n - 3] = False
        same_bits16(got[:, keep], want[:, keep])
        h = got[0].view(torch.float16).float()[n - 3]
        assert (bool(torch.isnan(h)) if want_nan else float(h) == bad), (kind, float(h))
        assert not bool(torch.isfinite(got[1].view(torch.float16).float()[n - 3]))


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(hip):
    x = torch.ones(64, device="cuda")
    pl = planes_buf(3, 64)
    X, P = x.data_ptr(), pl.data_ptr()
    slot = torch.zeros(33, device="cuda")
    S = slot.data_ptr()
    am = word(1.0).data_ptr()
    bad = [
        ("mmt_split_planes", (X, P, 64, 12)),                  # n % 8 != 0
        ("mmt_split_planes", (X + 4, P, 64, 8)),               # x off the 16-byte grid
        ("mmt_split_planes", (X, P + 4, 64, 8)),               # planes off the 16-byte grid
        ("mmt_split_planes", (X, P, 8, 16)),                   # plane_stride < n
        ("mmt_split_planes", (X, P, 20, 16)),                  # plane_stride % 8 != 0
        ("mmt_split_planes_f16", (X, P, 64, 12, 1.0, None, None, None, None)),
        ("mmt_split_planes_f16", (X + 4, P, 64, 8, 1.0, None, None, None, None)),
        ("mmt_split_planes_f16", (X, P, 8, 16, 1.0, None, None, None, None)),
        ("mmt_split_planes_f16", (X, P, 20, 16, 1.0, None, None, None, None)),
        ("mmt_split_planes_f16_rb", (X, P, 64, 1, 2, 24, am, None)),        # C % 16 != 0
        ("mmt_split_planes_f16_rb", (X, P, 16, 1, 2, 16, am, None)),        # plane_stride < n
        ("mmt_pack_weight", (X, P, 64, 2, 24)),                # K % 16 != 0
        ("mmt_pack_weight", (X, P, 64, 2, 16)),                # plane_stride < 512
        ("mmt_pack_weight_f16", (X, P, 64, 2, 24, 1.0, None, None)),
        ("mmt_pack_weight_flipped", (X, None, P, 1024, 8, 1, 1, 2)),        # flipped: Cout % 16 != 0
        ("mmt_pack_weight_flipped_f16", (X, None, P, 1024, 8, 1, 1, 2, am, None)),
        ("mmt_amax", (X, 6, None, 0, 0, am)),                  # n % 4 != 0
        ("mmt_amax", (X + 4, 8, None, 0, 0, am)),
        ("mmt_amax_stats", (X + 4, 8, S)),
        ("mmt_sum_stats", (X, X, None, X, X, 8, S)),           # d without c
        ("mmt_sum_stats", (X, X + 4, None, None, X, 8, S)),
        ("mmt_sum_stats_rb", (X, X, None, None, X, 1, 2, 24, S, None, 0, am, None)),      # C % 16 != 0
        ("mmt_sum_stats_rb", (X, X, None, X, X, 1, 2, 16, S, None, 0, am, None)),         # d without c
    ]
    assert hip.lib().mmt_packed_weight_elems(2, 24) == -1
    for name, args in bad:
        assert call(hip, name, *args) == EINVAL, (name, args)
    # n == 0: accepted, nothing written
    assert call(hip, "mmt_split_planes", X, P, 64, 0) == 0
    assert call(hip, "mmt_split_planes_f16", X, P, 64, 0, 1.0, None, None, None, None) == 0
    assert call(hip, "mmt_split_planes_f16_rb", X, P, 64, 0, 2, 16, am, None) == 0
    assert call(hip, "mmt_amax", X, 0, None, 0, 0, S) == 0
    assert call(hip, "mmt_amax_stats", X, 0, S) == 0
    assert call(hip, "mmt_sum_stats", X, X, None, None, X, 0, S) == 0
    assert call(hip, "mmt_rb_scales_update", S, 0) == 0
    assert (pl == FILL).all() and (slot == 0).all() and (x == 1).all()


# ------------------------------------------------------------------------------------------ the consumers honour subnormal terms
def test_conv_keeps_a_value_whose_fp16_terms_are_subnormal(hip):
    """1x1 convolution on the tiled fp16-split route, w = a selection of one input channel: x has its maximum 1.0 in one pixel and 2^-30
    in another (same channel), under x's own scale 2^13 that value is 2^-17: h = 2^-17 is an fp16 SUBNORMAL (8 quanta of 2^-24), l = 0,
    and the product with w's term is exact.  csrc/conv_shared.h documents |error| <= 2^-25 in scaled units here, 2^-38 of the maximum:
    the output must be 2^-30 to that bound.  A matrix unit that flushed subnormal fp16 inputs would give 0."""
    H = hip
    prev = H.get_conv_precision()
    H.set_conv_precision(3)
    H.set_f16x2(True)
    try:
        ci0 = 5
        g = torch.Generator().manual_seed(95)
        x = (torch.randn(2, 64, 16, 16, generator=g) * 2.0 ** -8)
        x[:, ci0] = x[:, ci0].abs() * 2.0 ** -4
        x[0, ci0, 3, 4] = 1.0
        x[1, ci0, 7, 9] = 2.0 ** -30
        w = torch.zeros(64, 64, 1, 1)
        w[:, ci0] = 1.0
        xd = x.cuda().contiguous(memory_format=torch.channels_last)
        wd = w.cuda().contiguous(memory_format=torch.channels_last)
        crest = float(x.abs().max() / x.abs().mean())
        assert crest < 2.0 ** 17
        a = H.ConvArgs()
        a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW = 2, 16, 16, 64, 64, 1, 1
        a.stride, a.pad, a.Ho, a.Wo, a.out_stride = 1, 0, 16, 16, 1
        assert H.conv_route(a, H.ENTRY_F16, H.ASSUME_X | H.ASSUME_W | H.ASSUME_W_PLANES | H.ASSUME_F16_SCALARS).family == 3   # MMT_ROUTE_DMA: the tiled kernel
        s0 = dict(H.F16_STATS)
        y = H.conv_forward(xd, wd, None, None, 1, 0)
        torch.cuda.synchronize()
        assert H.F16_STATS.get("tiled", 0) - s0.get("tiled", 0) == 1 and H.F16_STATS.get("fallback", 0) == s0.get("fallback", 0)
        got = y[1, :, 7, 9].double().cpu()
        print("outputs at the 2^-30 pixel: min %.6g max %.6g (2^-30 = %.6g)" % (float(got.min()), float(got.max()), 2.0 ** -30))
        assert ((got - 2.0 ** -30).abs() <= 2.0 ** -38).all()
        assert (y[0, :, 3, 4] == 1.0).all()
    finally:
        H.set_f16x2(None)
        H.set_conv_precision(prev)
