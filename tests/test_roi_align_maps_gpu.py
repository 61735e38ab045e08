"""`mmt_roi_align_maps_forward` / `_backward` (csrc/roi_align.hip): every ROI pooled from several maps of their own widths into one
channel-concatenated tensor in one launch -- the ROIAlign of the CSPN mask head.  A map's slice must be bit-identical to the
single-level `roi_align_forward` on that map and to the oracle's restatement of the reference's CPU ROIAlign; channels no map owns
stay untouched; the backward (fp32 atomics) against the oracle with the tolerance tests/test_hip_kernels.py carries for the
atomics form.
Deliberate: at K = 300 with 25 x 25 bins the oracle (seconds per map on the CPU) is asked for every sixth ROI only -- forward on those
ROIs, backward with a gradient that is zero on the others --, while ALL ROIs are compared with the single-level kernel, bit for bit
forward and within the atomics' tolerance backward; that kernel is itself pinned to the oracle on all of its ROIs by
tests/test_hip_kernels.py.  At 7 x 7 bins, and for K = 1, the oracle sees every ROI.  Runs on the MI355X box only (-m gpu)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 2
SIZES = [(64, 80), (32, 40), (16, 20), (8, 10)]
SCALES = [1.0, 0.5, 0.25, 0.125]
CHANNELS = {"partial": (4, 8, 36, 260),     # a partial wave, a partial second pass, more than one 256-channel pass
            "cspn": (32, 64, 128, 256)}
PAD = 4                                       # channels of the output that no map owns


@pytest.fixture(scope="module")
def hip():
    from maskrcnn_benchmark import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return _hip


def cl(x):  # NCHW cpu tensor -> NHWC-dense cuda tensor
    return x.cuda().contiguous(memory_format=torch.channels_last)


def make_rois(K, seed):
    """ROIs in image coordinates (map 0 is 64 x 80 at scale 1): over every border, sub-pixel, larger than the map, images mixed"""
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(K, 2, generator=g) * torch.tensor([80 + 30., 64 + 30.]) - 20
    wh = torch.rand(K, 2, generator=g) * 60 + 1
    wh[::7] = torch.rand(wh[::7].shape, generator=g) * 0.9      # sub-pixel on every map
    wh[3::11] = 120.                                            # larger than the map
    if K > 4:
        xy[1], wh[1] = torch.tensor([-15., -12.]), torch.tensor([30., 25.])      # over the top-left corner
        xy[2], wh[2] = torch.tensor([70., 55.]), torch.tensor([40., 30.])        # over the bottom-right corner
        xy[4], wh[4] = torch.tensor([-200., -200.]), torch.tensor([50., 50.])    # wholly outside: every sample is empty
    img = torch.randint(0, N, (K,), generator=g).float()
    return torch.cat([img[:, None], xy, xy + wh], 1)


_INPUTS = {}


def inputs(name):
    if name not in _INPUTS:
        g = torch.Generator().manual_seed(len(name))
        _INPUTS[name] = [torch.randn(N, c, h, w, generator=g) for c, (h, w) in zip(CHANNELS[name], SIZES)]
    return _INPUTS[name]


def offsets(chs):
    """the maps side by side behind PAD channels that no map owns -> (c_off, out_C)"""
    off = [PAD + sum(chs[:i]) for i in range(len(chs))]
    return off, PAD + sum(chs)


@pytest.mark.parametrize("name", sorted(CHANNELS))
@pytest.mark.parametrize("res,sr", [(25, 2), (7, 2), (25, 0), (7, 0)])
@pytest.mark.parametrize("K", [0, 1, 300])
def test_forward_and_backward(hip, name, res, sr, K):
    from oracle import native
    feats, chs = inputs(name), CHANNELS[name]
    rois = make_rois(K, 17 + K + res)
    off, out_C = offsets(chs)
    dfeats, drois = [cl(f) for f in feats], rois.cuda()
    out = torch.full((K, res, res, out_C), float("nan"), device="cuda").permute(0, 3, 1, 2)
    y = hip.roi_align_maps_forward(dfeats, SCALES, drois, res, res, sr, c_off=off, out=out)
    assert y is out
    assert torch.isnan(y[:, :PAD]).all()
    # the oracle on every ROI, or -- 25 x 25 bins of 300 ROIs on the CPU take seconds -- on every sixth
    sub = torch.arange(0, K, 6) if (K > 100 and res > 7) else torch.arange(K)
    lv = torch.zeros((K,), dtype=torch.int32, device="cuda")
    for m, f in enumerate(feats):
        mine = y[:, off[m]:off[m] + chs[m]]
        single = hip.roi_align_forward([dfeats[m]], [SCALES[m]], drois, lv, res, res, sr)
        assert torch.equal(mine, single), (name, m)
        ref = native.roi_align_forward(f, rois[sub], SCALES[m], res, res, sr)
        assert torch.equal(mine[sub.cuda()].cpu(), ref), (name, m)
    # one map alone (written at offset 0 of a tensor of its own) equals its slice of the four-map call
    alone = hip.roi_align_maps_forward([dfeats[2]], [SCALES[2]], drois, res, res, sr)
    assert tuple(alone.shape) == (K, chs[2], res, res)
    assert torch.equal(alone, y[:, off[2]:off[2] + chs[2]])

    # backward.  Against the single-level kernel with a dense gradient (all ROIs), and against the oracle with a gradient that is
    # zero off `sub` (rows of zeros add nothing: the oracle then needs those ROIs only)
    g = torch.Generator().manual_seed(K + res)
    go = torch.randn(K, out_C, res, res, generator=g)
    shapes = [tuple(f.shape) for f in feats]
    grads = hip.roi_align_maps_backward(cl(go), shapes, SCALES, drois, res, res, sr, c_off=off)
    gs = torch.zeros_like(go)
    gs[sub] = go[sub]
    grads_sub = grads if len(sub) == K else hip.roi_align_maps_backward(cl(gs), shapes, SCALES, drois, res, res, sr, c_off=off)
    for m, f in enumerate(feats):
        assert tuple(grads[m].shape) == shapes[m]
        sl = slice(off[m], off[m] + chs[m])
        single = hip.roi_align_backward(cl(go[:, sl]), [shapes[m]], [SCALES[m]], drois, lv, res, res, sr)[0]
        gr = native.roi_align_backward(go[sub][:, sl], rois[sub], SCALES[m], res, res, *shapes[m], sr)
        # fp32 atomics: the tolerance of tests/test_hip_kernels.py::test_roi_align_fpn_fused_and_backward
        atol = 5e-6 * max(1.0, float(gr.abs().max()))
        torch.testing.assert_close(grads_sub[m].cpu(), gr, rtol=1e-4, atol=atol)
        atol = 5e-6 * max(1.0, float(single.abs().max()))
        torch.testing.assert_close(grads[m], single, rtol=1e-4, atol=2 * atol)   # (both sides carry the atomics' error)
    if K == 0:
        assert all(not t.any() for t in grads)


def test_refused_arguments(hip):
    feats = [cl(torch.randn(N, c, h, w)) for c, (h, w) in zip((8, 6, 12), SIZES)]
    rois = make_rois(5, 1).cuda()
    out = torch.zeros((5, 7, 7, 28), device="cuda").permute(0, 3, 1, 2)
    with pytest.raises(RuntimeError, match="mmt_roi_align_maps_forward failed with code -22"):   # C % 4 != 0
        hip.roi_align_maps_forward(feats, SCALES[:3], rois, 7, 7, 2, c_off=(0, 8, 16), out=out)
    ok = [feats[0], feats[2]]
    with pytest.raises(RuntimeError, match="code -22"):                                           # an offset off a multiple of 4
        hip.roi_align_maps_forward(ok, SCALES[:2], rois, 7, 7, 2, c_off=(0, 10), out=out)
    with pytest.raises(RuntimeError, match="code -22"):                                           # slices that overlap
        hip.roi_align_maps_forward(ok, SCALES[:2], rois, 7, 7, 2, c_off=(0, 4), out=out)
    with pytest.raises(RuntimeError, match="code -22"):                                           # a slice past out_C
        hip.roi_align_maps_forward(ok, SCALES[:2], rois, 7, 7, 2, c_off=(0, 20), out=out)
    with pytest.raises(RuntimeError, match="code -22"):                                           # a negative sampling ratio
        hip.roi_align_maps_forward(ok, SCALES[:2], rois, 7, 7, -1)
    assert not out.any()                                                                          # nothing was launched
    with pytest.raises(RuntimeError, match="1..4 maps"):
        hip.roi_align_maps_forward([], [], rois, 7, 7, 2)
    with pytest.raises(RuntimeError, match="1..4 maps"):
        hip.roi_align_maps_forward([feats[0]] * 5, [1.0] * 5, rois, 7, 7, 2)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        hip.roi_align_maps_forward([f.cpu() for f in ok], SCALES[:2], rois, 7, 7, 2)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        hip.roi_align_maps_forward(ok, SCALES[:2], rois.cpu(), 7, 7, 2)
    go = torch.zeros((5, 7, 7, 20), device="cuda").permute(0, 3, 1, 2)
    shapes = [tuple(f.shape) for f in ok]
    with pytest.raises(RuntimeError, match="GPU tensor"):
        hip.roi_align_maps_backward(go.cpu(), shapes, SCALES[:2], rois, 7, 7, 2)
    with pytest.raises(RuntimeError, match="mmt_roi_align_maps_backward failed with code -22"):
        hip.roi_align_maps_backward(go, shapes, SCALES[:2], rois, 7, 7, 2, c_off=(0, 10))
    with pytest.raises(RuntimeError, match="1..4 maps"):
        hip.roi_align_maps_backward(go, shapes * 3, SCALES[:2] * 3, rois, 7, 7, 2)


def test_an_image_index_outside_the_batch_reads_nothing(hip):
    """a ROI whose image index is not 0 .. N-1 gets zeros forward and adds no gradient (the single-level kernel would read past the map)"""
    feats = [cl(f) for f in inputs("cspn")]
    rois = make_rois(6, 3)
    rois[1, 0], rois[4, 0] = float(N), -1.0
    y = hip.roi_align_maps_forward(feats, SCALES, rois.cuda(), 7, 7, 2)
    good = torch.tensor([0, 2, 3, 5])
    ref = hip.roi_align_maps_forward(feats, SCALES, rois[good].cuda(), 7, 7, 2)
    assert torch.equal(y[good.cuda()], ref) and not y[1].any() and not y[4].any()
    go = torch.randn(6, 480, 7, 7)
    a = hip.roi_align_maps_backward(cl(go), [tuple(f.shape) for f in feats], SCALES, rois.cuda(), 7, 7, 2)
    b = hip.roi_align_maps_backward(cl(go[good]), [tuple(f.shape) for f in feats], SCALES, rois[good].cuda(), 7, 7, 2)
    for s, t in zip(a, b):
        torch.testing.assert_close(s, t, rtol=1e-4, atol=5e-6 * max(1.0, float(t.abs().max())))
