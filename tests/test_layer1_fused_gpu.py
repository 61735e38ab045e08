"""A frozen layer1 bottleneck's conv2 (3x3, 64 -> 64) and conv3 (1x1, 64 -> 256 + residual + ReLU) as ONE launch (include/mmtpsm.h:
mmt_c64_conv3_fused; csrc/conv_stem.hip: conv3x3_c64_kernel<1>; _hip.c64_conv3_fused; layers/fused.py::bottleneck_forward).  o2, the
3x3's output, never reaches memory: it is split inside the launch with the producing site's LAGGED scale and every tile tests its own
values against it.  Checked here, on maps of one tile (8 x 16), ragged in both directions (9 x 17, 20 x 36) and 32 x 32, N = 1 and 2:
  * handed the scale the un-fused chain derives (o2's own maximum), `out` is BIT-IDENTICAL to conv3x3_c64 -> conv1x1_rows: same
    products in the same order -- with the identity residual and with block 0's downsample output;
  * with the lagged scale -- made for a tensor half as large, and a site's first call -- conv3 stays within 3e-6 of sum |a||b| of an
    fp64 reference (the bound of tests/test_rb_epilogue_gpu.py; the reference takes the un-fused launch's o2, which the first case
    shows to be the fused launch's);
  * a tile with one element 10^4 x the scale's range takes the exact path: the same bound;
  * the recorded maxima are torch.amax of the tensors (out; o2's pending maximum at its site);
  * a three-block layer1 chain agrees with the un-fused chain, and a block that gradients flow through keeps the old launches;
  * the NEXT block's conv1 behind conv3 in the same launch (conv3x3_c64_kernel<2>): o1_next and out bit-identical to the three
    launches at their scales, a last block without one, the lagged scale of `out` and a scale of zero against fp64, a wave of `out`
    beyond the scale's range, o1_next's recorded maximum, and the chain with o1_next handed from block to block."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, ROOT)

SHAPES = [(1, 8, 16), (2, 9, 17), (1, 20, 36), (2, 32, 32)]


@pytest.fixture()
def hip():
    from maskrcnn_benchmark import _hip as H
    H.lib()
    prev = H.get_conv_precision()
    H.set_conv_precision(3)
    H.set_f16x2(True)      # (also forgets every producing site)
    yield H
    H.C64_FUSE = True
    H.set_f16x2(None)
    H.set_conv_precision(prev)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _block(g, cin, down=False):
    """weights and folded FrozenBN of one bottleneck with 64 bottleneck and 256 output channels"""
    def w(co, ci, k):
        return _cl((torch.randn(co, ci, k, k, generator=g) * (2.0 / (k * k * ci)) ** 0.5).cuda())

    def bn(c):
        return (torch.rand(c, generator=g) + 0.5).cuda(), (torch.randn(c, generator=g) * 0.1).cuda()
    s1, b1 = bn(64)
    s2, b2 = bn(64)
    s3, b3 = bn(256)
    sd, bd = bn(256) if down else (None, None)
    return dict(w1=w(64, cin, 1), w2=w(64, 64, 3), w3=w(256, 64, 1), wd=w(256, cin, 1) if down else None,
                bn=(s1, b1, s2, b2, s3, b3, sd, bd))


def _inputs(H, shape, seed, down=False):
    """x, the block, o1 = conv1(x) with its statistics recorded, the residual operand"""
    N, Hh, W = shape
    g = torch.Generator().manual_seed(seed + 7 * N + Hh + W)
    cin = 64 if down else 256
    x = _cl(torch.randn(N, cin, Hh, W, generator=g).relu().cuda())
    blk = _block(g, cin, down)
    s1, b1, s2, b2, s3, b3, sd, bd = blk["bn"]
    o1 = H.conv_forward(x, blk["w1"], s1, b1, relu=True)
    r = H.conv_forward(x, blk["wd"], sd, bd) if down else x
    return x, blk, o1, r


def _unfused(H, blk, o1, r, site=None, affine3=True):
    s1, b1, s2, b2, s3, b3, sd, bd = blk["bn"]
    o2 = H.conv_forward(o1, blk["w2"], s2, b2, 1, 1, relu=True, rb_site=site)
    out = H.conv_forward(o2, blk["w3"], s3 if affine3 else None, b3 if affine3 else None, 1, 0, relu=True, res=r, res_mode=1)
    return o2, out


def _slot_max(t):
    slot = t._mmt_amax[0]
    return float(slot.pool.dev[slot.idx][0])


@pytest.mark.parametrize("down", [False, True], ids=["identity-residual", "block0-downsample"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_same_scale_is_bit_identical(hip, shape, down):
    H = hip
    x, blk, o1, r = _inputs(H, shape, 1, down)
    s1, b1, s2, b2, s3, b3, sd, bd = blk["bn"]
    o2, want = _unfused(H, blk, o1, r)
    n0 = H.F16_STATS.get("c64_fused", 0)
    out = H.c64_conv3_fused(o1, blk["w2"], s2, b2, blk["w3"], s3, b3, r, o2_amax=o2._mmt_amax[0])
    assert out is not None and H.F16_STATS.get("c64_fused", 0) == n0 + 1
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert _slot_max(out) == float(out.abs().max())          # the maximum the consumers of `out` derive their scale from


def _conv3_error(o2, w3, out):
    """largest |out - fp64| / sum |a||b| of conv3 alone (no affine, zero residual: out = relu(conv1x1(o2)), and
    |relu(a) - relu(b)| <= |a - b|)"""
    ref = F.conv2d(o2.double().cpu(), w3.double().cpu()).relu()
    bound = F.conv2d(o2.abs().double().cpu(), w3.abs().double().cpu())
    return ((out.double().cpu() - ref).abs() / bound.clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_lagged_scale_against_fp64(hip, shape):
    """step 1: the site has no scale -- not a call for the fused launch (the binding gives a site's first call to the two old
    launches, so this half exercises the old kernels and the hand-over of o2's maximum to the site, not the new kernel); step 2: the
    fused launch on a tensor twice what the scale was made for (the head-room is 2 x: the largest term lands in [2^13, 2^14))"""
    H = hip
    x, blk, o1, r = _inputs(H, shape, 2)
    s1, b1, s2, b2, s3, b3, sd, bd = blk["bn"]
    zero = torch.zeros_like(r)
    site = H.o2_site(blk["w3"])
    assert H.c64_conv3_fused(o1, blk["w2"], s2, b2, blk["w3"], None, None, zero) is None     # first call
    o2, out1 = _unfused(H, blk, o1, zero, site, affine3=False)
    torch.cuda.synchronize()
    assert _conv3_error(o2, blk["w3"], out1) <= 3e-6
    row = H._rb_site(site, o1.device).state
    assert float(row[1]) == float(o2.abs().max())                                            # the pending maximum
    H.rb_scales_update()
    s = float(row[0])
    assert 2.0 ** 12 <= float(o2.abs().max()) * s < 2.0 ** 13
    # step 2: o2 doubles (conv2 without shift is linear in o1 up to the ReLU; with it, nearly) -- the fused launch, lagged scale
    o1b = H.conv_forward(x * 2.0, blk["w1"], s1, b1 * 2.0, relu=True)
    o2b, _ = _unfused(H, blk, o1b, zero, None, affine3=False)
    out2 = H.c64_conv3_fused(o1b, blk["w2"], s2, b2, blk["w3"], None, None, zero)
    assert out2 is not None
    torch.cuda.synchronize()
    assert float(o2b.abs().max()) * s >= 2.0 ** 12.9                                         # (really beyond the scale's own tensor)
    assert _conv3_error(o2b, blk["w3"], out2) <= 3e-6
    assert float(row[1]) == float(o2b.abs().max())
    assert _slot_max(out2) == float(out2.abs().max())


def test_a_tile_beyond_the_scales_range_takes_the_exact_path(hip):
    """a 3 x 3 block of pixels of o1 at 4e4 against a unit-variance rest, and one output channel of conv2 that sums its whole window:
    that channel of o2 is 10^4 x beyond the fp16 range at the site's scale in ONE tile (saturated planes would be off by orders of
    magnitude), while o1's own crest factor, <= 5e4, stays below its guard's 2^17 -- that tile computes conv3 with fp32 FMAs, the
    others stay on the matrix pipe"""
    H = hip
    N, Hh, W = 2, 20, 36
    g = torch.Generator().manual_seed(5)
    blk = _block(g, 256)
    blk["w2"][0] = 1.0
    s1, b1, s2, b2, s3, b3, sd, bd = blk["bn"]
    o1 = _cl(torch.randn(N, 64, Hh, W, generator=g).cuda())
    zero = _cl(torch.zeros(N, 256, Hh, W, device="cuda"))
    site = H.o2_site(blk["w3"])
    _unfused(H, blk, o1, zero, site, affine3=False)
    H.rb_scales_update()
    o1b = o1.clone()
    o1b[1, :, 10:13, 18:21] = 4.0e4                                                          # inside the tile rows 8-15, columns 16-31
    o2b, _ = _unfused(H, blk, o1b, zero, None, affine3=False)
    fb0 = H.F16_STATS.get("fallback", 0)
    out = H.c64_conv3_fused(o1b, blk["w2"], s2, b2, blk["w3"], None, None, zero)
    assert out is not None and H.F16_STATS.get("fallback", 0) == fb0                          # no site left the fp16 split on the host
    torch.cuda.synchronize()
    row = H._rb_site(site, o1.device).state
    s = float(row[0])
    assert float(o2b.abs().max()) * s >= 1.0e4 * 65504.0                                     # one element 10^4 x the scale's range
    assert _conv3_error(o2b, blk["w3"], out) <= 3e-6
    # WHICH tiles left the matrix path: the same launch told to derive the same scale from a maximum (2^13 / s maps to s) makes no tile
    # test and keeps every tile on the matrix pipe.  Outside the spike's tile the two agree bit for bit -- those tiles were on the
    # matrix pipe in the guarded launch too (neither o1's grid-wide guard nor another arithmetic took them) --, inside it the
    # unguarded launch saturates and is off by orders of magnitude
    same_scale = torch.tensor([2.0 ** 13 / s], device="cuda")
    forced = H.c64_conv3_fused(o1b, blk["w2"], s2, b2, blk["w3"], None, None, zero, o2_amax=same_scale)
    torch.cuda.synchronize()
    tile = torch.zeros(N, 1, Hh, W, dtype=torch.bool, device="cuda")
    tile[1, :, 8:16, 16:32] = True
    away = (~tile).expand_as(out)
    assert torch.equal(out[away], forced[away])
    inside = tile.expand_as(out)
    assert not torch.equal(out[inside], forced[inside])
    ref = F.conv2d(o2b.double().cpu(), blk["w3"].double().cpu()).relu()
    ins = inside.cpu()
    assert float((forced.double().cpu() - ref)[ins].abs().max()) > 1.0e3 * float((out.double().cpu() - ref)[ins].abs().max())
    assert _slot_max(out) == float(out.abs().max())


def _chain(H, blocks, x):
    from maskrcnn_benchmark.layers import fused
    for blk in blocks:
        x = fused.bottleneck_forward(x, blk["w1"], blk["w2"], blk["w3"], blk["wd"], blk["bn"], 1, frozen=True)[2]
    return x


def test_three_block_chain_against_the_unfused_chain(hip):
    """layer1 as the backbone runs it when frozen: block 0 with its downsample, two more.  Step 1 takes the old launches (no site has a
    scale), step 2 the fused one in all three blocks.  Both chains keep every convolution within 3e-6 of its sum |a||b|; they differ
    in the three conv3 alone, by at most twice that, and what block 0 and 1 differ by passes through the (He-scaled, gain ~ 1)
    convolutions behind them: 3 x 2 x 3e-6 of the largest output, doubled for the gains' spread"""
    H = hip
    g = torch.Generator().manual_seed(11)
    blocks = [_block(g, 64, True), _block(g, 256), _block(g, 256)]
    x = _cl(torch.randn(2, 64, 20, 36, generator=g).relu().cuda())
    y1 = _chain(H, blocks, x)
    H.rb_scales_update()
    n0 = H.F16_STATS.get("c64_fused", 0)
    y2 = _chain(H, blocks, x)
    assert H.F16_STATS.get("c64_fused", 0) == n0 + 3
    H.C64_FUSE = False
    y3 = _chain(H, blocks, x)
    assert H.F16_STATS.get("c64_fused", 0) == n0 + 3
    torch.cuda.synchronize()
    assert torch.equal(y1, y3)
    assert (y2 - y3).abs().max().item() <= 3.6e-5 * float(y3.abs().max())
    assert _slot_max(y2) == float(y2.abs().max())


def test_a_block_with_gradients_keeps_the_old_launches(hip):
    """FREEZE_CONV_BODY_AT = 1: layer1 trains -- its node saves o1 and o2 for the backward pass, so the three launches stay"""
    H = hip
    from maskrcnn_benchmark.layers import fused
    g = torch.Generator().manual_seed(13)
    blk = _block(g, 256)
    x = _cl(torch.randn(1, 256, 9, 17, generator=g).relu().cuda())
    H._amax_of(x)
    with torch.no_grad():                                     # frozen: step 1 makes the site ready, step 2 is fused
        fused.BottleneckFn.apply(x, blk["w1"], blk["w2"], blk["w3"], None, blk["bn"], 1)
        H.rb_scales_update()
        n0 = H.F16_STATS.get("c64_fused", 0)
        y_frozen = fused.BottleneckFn.apply(x, blk["w1"], blk["w2"], blk["w3"], None, blk["bn"], 1)
        assert H.F16_STATS.get("c64_fused", 0) == n0 + 1
    ws = [blk[k].clone().requires_grad_(True) for k in ("w1", "w2", "w3")]
    xg = x.clone().requires_grad_(True)
    H._amax_of(xg)
    y = fused.BottleneckFn.apply(xg, ws[0], ws[1], ws[2], None, blk["bn"], 1)
    assert H.F16_STATS.get("c64_fused", 0) == n0 + 1          # not fused
    (y * (y > 0)).sum().backward()
    torch.cuda.synchronize()
    assert all(w.grad is not None and torch.isfinite(w.grad).all() for w in ws) and torch.isfinite(xg.grad).all()
    assert (y.detach() - y_frozen).abs().max().item() <= 1.2e-5 * float(y_frozen.abs().max())   # (one conv3 apart: 2 x 3e-6, gains as above)


# ---- the NEXT block's conv1 (1x1, 256 -> 64) behind conv3 in the same launch: o1_next

def _next(g):
    """conv1 and bn1 of the block behind: (w1, scale1, shift1)"""
    w1 = _cl((torch.randn(64, 256, 1, 1, generator=g) * (2.0 / 256) ** 0.5).cuda())
    return w1, (torch.rand(64, generator=g) + 0.5).cuda(), (torch.randn(64, generator=g) * 0.1).cuda()


@pytest.mark.parametrize("down", [False, True], ids=["identity-residual", "block0-downsample"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_o1_next_same_scales_is_bit_identical(hip, shape, down):
    """handed the scales the un-fused chain derives (the maxima of o2 and of out), `out` AND `o1_next` are bit-identical to
    conv3x3_c64 -> conv3 -> conv1 of the next block; the recorded maximum of o1_next is torch.amax of it; and a LAST block -- the same
    call without a next conv1 -- stores the same `out`"""
    H = hip
    x, blk, o1, r = _inputs(H, shape, 3, down)
    s1, b1, s2, b2, s3, b3, sd, bd = blk["bn"]
    w1n, s1n, b1n = _next(torch.Generator().manual_seed(17))
    o2, want = _unfused(H, blk, o1, r)
    want_n = H.conv_forward(want, w1n, s1n, b1n, relu=True)
    n0 = H.F16_STATS.get("c64_fused_next", 0)
    got = H.c64_conv3_fused(o1, blk["w2"], s2, b2, blk["w3"], s3, b3, r, o2_amax=o2._mmt_amax[0], nxt=(w1n, s1n, b1n),
                            out_amax=want._mmt_amax[0])
    assert got is not None and got[1] is not None and H.F16_STATS.get("c64_fused_next", 0) == n0 + 1
    out, o1n = got
    last = H.c64_conv3_fused(o1, blk["w2"], s2, b2, blk["w3"], s3, b3, r, o2_amax=o2._mmt_amax[0])     # the last block: no next conv1
    assert H.F16_STATS.get("c64_fused_next", 0) == n0 + 1
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(last, want)
    assert tuple(o1n.shape) == tuple(want_n.shape) and torch.equal(o1n, want_n)
    assert _slot_max(o1n) == float(o1n.abs().max()) and _slot_max(out) == float(out.abs().max())


def _conv1_error(out, w1n, o1n):
    ref = F.conv2d(out.double().cpu(), w1n.double().cpu()).relu()
    bound = F.conv2d(out.abs().double().cpu(), w1n.abs().double().cpu())
    return ((o1n.double().cpu() - ref).abs() / bound.clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], ids=["2x9x17", "1x20x36"])
def test_o1_next_lagged_scales_and_no_scale_against_fp64(hip, shape):
    """step 1: no site has a scale -- the old launches record the maxima of o2 and of out; step 2: tensors twice what the scales were
    made for, conv3 and the next conv1 fused; step 3: both sites' scales zeroed (what a caller must not do, and the launch's answer to
    it: every tile exact).  o1_next against fp64 of the `out` the launch stored, <= 3e-6 of sum |a||b|"""
    H = hip
    x, blk, o1, r = _inputs(H, shape, 4)
    s1, b1, s2, b2, s3, b3, sd, bd = blk["bn"]
    w1n, _, _ = _next(torch.Generator().manual_seed(19))
    zero = torch.zeros_like(r)
    assert H.c64_conv3_fused(o1, blk["w2"], s2, b2, blk["w3"], None, None, zero, nxt=(w1n, None, None)) is None
    o2 = H.conv_forward(o1, blk["w2"], s2, b2, 1, 1, relu=True, rb_site=H.o2_site(blk["w3"]))
    out1 = H.conv_forward(o2, blk["w3"], None, None, 1, 0, relu=True, res=zero, res_mode=1, rb_site=H.out_site(w1n))
    torch.cuda.synchronize()
    row = H._rb_site(H.out_site(w1n), o1.device).state
    assert float(row[1]) == float(out1.abs().max())
    H.rb_scales_update()
    o1b = H.conv_forward(x * 2.0, blk["w1"], s1, b1 * 2.0, relu=True)
    o2b = H.conv_forward(o1b, blk["w2"], s2, b2, 1, 1, relu=True)
    out, o1n = H.c64_conv3_fused(o1b, blk["w2"], s2, b2, blk["w3"], None, None, zero, nxt=(w1n, None, None))
    assert o1n is not None
    torch.cuda.synchronize()
    assert float(out.abs().max()) * float(row[0]) >= 2.0 ** 12.9
    assert _conv3_error(o2b, blk["w3"], out) <= 3e-6 and _conv1_error(out, w1n, o1n) <= 3e-6
    assert float(row[1]) == float(out.abs().max()) and _slot_max(o1n) == float(o1n.abs().max())
    row2 = H._rb_site(H.o2_site(blk["w3"]), o1.device).state
    row[0] = 0.0
    row2[0] = 0.0
    out0, o1n0 = H.c64_conv3_fused(o1b, blk["w2"], s2, b2, blk["w3"], None, None, zero, nxt=(w1n, None, None))
    torch.cuda.synchronize()
    assert _conv3_error(o2b, blk["w3"], out0) <= 3e-6 and _conv1_error(out0, w1n, o1n0) <= 3e-6
    assert _slot_max(o1n0) == float(o1n0.abs().max()) and _slot_max(out0) == float(out0.abs().max())


def test_a_wave_beyond_the_out_scales_range_computes_o1_next_exactly(hip):
    """the residual carries one pixel 10^7 x the rest: `out` there leaves the fp16 range at its site's scale, the wave that owns the
    pixel computes its 32 pixels of o1_next with fp32 FMAs (a saturated operand would be off by orders of magnitude)"""
    H = hip
    x, blk, o1, r = _inputs(H, (2, 20, 36), 6)
    s1, b1, s2, b2, s3, b3, sd, bd = blk["bn"]
    w1n, _, _ = _next(torch.Generator().manual_seed(23))
    o2 = H.conv_forward(o1, blk["w2"], s2, b2, 1, 1, relu=True, rb_site=H.o2_site(blk["w3"]))
    H.conv_forward(o2, blk["w3"], s3, b3, 1, 0, relu=True, res=r, res_mode=1, rb_site=H.out_site(w1n))
    H.rb_scales_update()
    rb = r.clone()
    rb[1, :, 11, 19] = 1.0e7
    out, o1n = H.c64_conv3_fused(o1, blk["w2"], s2, b2, blk["w3"], s3, b3, rb, nxt=(w1n, None, None))
    torch.cuda.synchronize()
    row = H._rb_site(H.out_site(w1n), o1.device).state
    assert float(out.abs().max()) * float(row[0]) >= 1.0e4 * 65504.0
    assert _conv1_error(out, w1n, o1n) <= 3e-6


def test_layer1_chain_hands_o1_next_from_block_to_block(hip):
    """the frozen layer1 as the backbone runs it (layers/fused.py::frozen_stage): step 1 the old launches (no site has a scale), step 2
    three fused launches, the first two of which also run the next block's conv1 and hand its result over -- no separate conv1 launch
    for blocks 1 and 2.  Against the un-fused chain: every convolution of either chain is within 3e-6 of its sum |a||b|; they differ in
    the three conv3 and the two handed-over conv1, each by at most twice that, passed on through (He-scaled, gain ~ 1) convolutions:
    5 x 2 x 3e-6 of the largest output, doubled for the gains' spread"""
    H = hip
    from maskrcnn_benchmark.layers import fused
    g = torch.Generator().manual_seed(29)
    blocks = [_block(g, 64, True), _block(g, 256), _block(g, 256)]
    args = [(b["w1"], b["w2"], b["w3"], b["wd"], b["bn"], 1, False) for b in blocks]
    x = _cl(torch.randn(2, 64, 20, 36, generator=g).relu().cuda())
    y1 = fused.frozen_stage(x, args)
    H.rb_scales_update()
    n0, m0, c0 = H.F16_STATS.get("c64_fused", 0), H.F16_STATS.get("c64_fused_next", 0), H.F16_STATS.get("tiled", 0)
    y2 = fused.frozen_stage(x, args)
    assert H.F16_STATS.get("c64_fused", 0) == n0 + 3 and H.F16_STATS.get("c64_fused_next", 0) == m0 + 2
    assert H.F16_STATS.get("tiled", 0) == c0 + 2              # block 0's conv1 and its downsample: nothing else left the fused launch
    H.C64_FUSE = False
    y3 = fused.frozen_stage(x, args)
    torch.cuda.synchronize()
    assert torch.equal(y1, y3)
    assert (y2 - y3).abs().max().item() <= 6.0e-5 * float(y3.abs().max())
    assert _slot_max(y2) == float(y2.abs().max())
