"""Geometry on mask words on the MI355X (csrc/bitmasks.hip: `mmt_mask_words_resample`, `mmt_mask_words_targets`) and the
BinaryMaskList built on it, against the host restatement of the rules (tests/bitmask_formulation.py).  Source masks: the polygon
cases of tests/polygon_image_inputs.py rasterised by the existing `polygon_mask_words`, random masks at densities 0.1, 0.5 and 0.9,
an empty and a full mask.  Everything is in integers: words, records, targets and strings are compared with equality."""
import numpy as np
import pytest
import torch

import bitmask_formulation as bf
import polygon_image_inputs as pi

pytestmark = pytest.mark.gpu

EINVAL = -22
SIZES = [(1, 1), (37, 53), (128, 150), (5, 200), (300, 257), (16384, 2)]
ids = lambda s: "%dx%d" % tuple(s)   # noqa: E731


@pytest.fixture(scope="module")
def hip():
    from maskrcnn_benchmark import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return _hip


_SRC = {}


def source(hip, size):
    """-> (bytes uint8 (G, H, W) on the host, words, records on the device), made once per size; read-only"""
    if size not in _SRC:
        H, W = size
        c = pi.cases(size)
        xy, off, rng = (torch.from_numpy(c[k].copy()).cuda() for k in ("poly_xy", "poly_off", "inst_poly"))
        pw, _ = hip.polygon_mask_words(xy, off, rng, H, W)
        poly = hip.mask_words_integral(pw, list(range(pw.shape[0] + 1)), H, W).to(torch.uint8).cpu()
        gen = torch.Generator().manual_seed(H * 100003 + W)
        rand = [(torch.rand((H, W), generator=gen) < d).to(torch.uint8) for d in (0.1, 0.5, 0.9)]
        m = torch.cat([poly, torch.stack(rand + [torch.zeros((H, W), dtype=torch.uint8), torch.ones((H, W), dtype=torch.uint8)])])
        words, rec = hip.mask_pack(m.cuda())
        hw, hr = bf.pack(m)
        assert torch.equal(words.cpu(), hw) and torch.equal(rec.cpu(), hr)     # the helper's packer is the library's
        _SRC[size] = (m, words, rec)
    return _SRC[size]


def resample_abi(hip, words, size, win, flip, out_size, fill=0xFF, out=None):
    """mmt_mask_words_resample into outputs whose every byte is `fill` beforehand -> (code, words, records)"""
    H, W = size
    OH, OW = out_size
    G = words.shape[0]
    if out is None:
        out = torch.empty((G, (OH * OW + 63) // 64), dtype=torch.int64, device="cuda")
        out.view(torch.uint8).fill_(fill)
    rec = torch.empty((G, 8), dtype=torch.int32, device="cuda")
    rec.view(torch.uint8).fill_(fill)
    torch.cuda.synchronize()
    code = hip._lib_raw().mmt_mask_words_resample(words.data_ptr(), G, H, W, win[0], win[1], win[2], win[3], flip, OH, OW,
                                                  out.data_ptr(), rec.data_ptr(), None)
    torch.cuda.synchronize()
    return code, out, rec


def check_resample(hip, size, win, flip, out_size):
    m, words, rec = source(hip, size)
    want = bf.resample(m, win, out_size[0], out_size[1], flip)
    ww, wr = bf.pack(want)
    pw, pr = hip.mask_pack(want.cuda())
    code, gw, gr = resample_abi(hip, words, size, win, flip, out_size)
    assert code == 0
    bad = (gw.cpu() != ww).any(1).nonzero().reshape(-1).tolist()
    print("%s window %s flip %d -> %s: %d masks, %d bits set, masks that differ: %s" % (size, win, flip, out_size, len(m),
                                                                                      int(want.sum()), bad))
    assert torch.equal(gw.cpu(), ww) and torch.equal(gw, pw)          # every word, tail bits zero
    assert torch.equal(gr, pr) and torch.equal(gr.cpu(), wr)          # every record, as mmt_mask_pack gives it
    return want, gw, gr


# ------------------------------------------------------------------------------------------ 1. resample
@pytest.mark.parametrize("size", SIZES, ids=ids)
def test_identity_window_copies_words_and_records(hip, size):
    from maskrcnn_benchmark.structures.segmentation_mask import BinaryMaskList
    H, W = size
    m, words, rec = source(hip, size)
    code, gw, gr = resample_abi(hip, words, size, (0, 0, W, H), 0, size)
    assert code == 0 and torch.equal(gw, words) and torch.equal(gr, rec)
    w2, r2 = BinaryMaskList(m, (W, H)).resize((W, H)).mask_words()
    assert torch.equal(w2, words) and torch.equal(r2, rec)


@pytest.mark.parametrize("size", SIZES, ids=ids)
def test_flips(hip, size):
    from maskrcnn_benchmark.structures.segmentation_mask import BinaryMaskList, FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM
    H, W = size
    m, words, rec = source(hip, size)
    full = (0, 0, W, H)
    for flip in range(4):
        want = m.flip(2) if flip & 1 else m
        want = want.flip(1) if flip & 2 else want
        pw, pr = hip.mask_pack(want.contiguous().cuda())
        code, gw, gr = resample_abi(hip, words, size, full, flip, size)
        assert code == 0 and torch.equal(gw, pw) and torch.equal(gr, pr), flip
        code, back, brec = resample_abi(hip, gw, size, full, flip, size)
        assert code == 0 and torch.equal(back, words) and torch.equal(brec, rec), flip
    b = BinaryMaskList(m, (W, H))
    for method, dim in ((FLIP_LEFT_RIGHT, 2), (FLIP_TOP_BOTTOM, 1)):
        f = b.transpose(method)
        assert torch.equal(f.mask_words()[0], hip.mask_pack(m.flip(dim).contiguous().cuda())[0])
        assert torch.equal(f.transpose(method).mask_words()[0], words) and torch.equal(f.transpose(method).mask_words()[1], rec)


def _scaled(size, num, den):
    return tuple(max((s * num + den // 2) // den, 1) for s in size)


SCALES = ([(s, _scaled(s, *f)) for s in [(1, 1), (37, 53), (128, 150), (5, 200)] for f in ((2, 1), (5, 4), (1, 2), (4, 5))]
          + [((300, 257), (600, 514)), ((300, 257), (150, 128)), ((300, 257), (240, 206)),
             ((16384, 2), (16383, 3)), ((16384, 2), (8192, 1)), ((16384, 2), (16384, 4)), ((37, 53), (30, 41))])


@pytest.mark.parametrize("size,out", SCALES, ids=["%dx%d-%dx%d" % (s + o) for s, o in SCALES])
def test_scales(hip, size, out):
    from maskrcnn_benchmark.structures.segmentation_mask import BinaryMaskList
    H, W = size
    want, gw, gr = check_resample(hip, size, (0, 0, W, H), 0, out)
    w2, r2 = BinaryMaskList(source(hip, size)[0], (W, H)).resize((out[1], out[0])).mask_words()
    assert torch.equal(w2, gw) and torch.equal(r2, gr)


def _windows(H, W):
    """interior, touching each border, 1 x 1 (a corner and the middle), full"""
    w2, h2 = max(W // 2, 1), max(H // 2, 1)
    wins = {(W // 4, H // 4, w2, h2), (0, H // 4, w2, h2), (W - w2, H // 4, w2, h2), (W // 4, 0, w2, h2), (W // 4, H - h2, w2, h2),
            (0, 0, 1, 1), (W - 1, H - 1, 1, 1), (W // 2, H // 2, 1, 1), (0, 0, W, H)}
    return sorted(wins)


@pytest.mark.parametrize("size", SIZES, ids=ids)
def test_crop_windows(hip, size):
    from maskrcnn_benchmark.structures.segmentation_mask import BinaryMaskList
    H, W = size
    m = source(hip, size)[0]
    b = BinaryMaskList(m, (W, H))
    for win in _windows(H, W):
        x0, y0, w, h = win
        want, gw, gr = check_resample(hip, size, win, 0, (h, w))              # the crop itself: a copy of the window
        assert torch.equal(want, m[:, y0:y0 + h, x0:x0 + w])
        check_resample(hip, size, win, 1, (min(2 * h + 1, 16384), max(w // 2, 1)))   # crop, scale and flip at once
        c = b.crop([x0, y0, x0 + w, y0 + h])
        assert tuple(c.size) == (w, h) and torch.equal(c.mask_words()[0], gw) and torch.equal(c.mask_words()[1], gr)


@pytest.mark.parametrize("size,out", [((37, 53), (30, 41)), ((128, 150), (64, 75)), ((16384, 2), (16383, 3))])
def test_every_word_tail_bit_and_record_is_written(hip, size, out):
    H, W = size
    words = source(hip, size)[1]
    runs = [resample_abi(hip, words, size, (0, 0, W, H), 0, out, fill=f) for f in (0xFF, 0x00, 0x5A)]
    assert all(r[0] == 0 for r in runs)
    assert all(torch.equal(r[1], runs[0][1]) and torch.equal(r[2], runs[0][2]) for r in runs[1:])
    tail = (out[0] * out[1]) & 63
    if tail:
        assert int((runs[0][1][:, -1] >> tail).abs().sum()) == 0
    assert int(runs[0][2][:, 6:].abs().sum()) == 0


def test_two_runs_give_equal_bits(hip):
    size, out = (300, 257), (240, 206)
    m, words, rec = source(hip, size)
    roi, boxes = (t.cuda() for t in _rois(size, len(m), 28))

    def run():
        return (hip.mask_words_resample(words, 300, 257, (0, 0, 257, 300), 1, *out),
                hip.mask_words_targets(words, roi, boxes, 300, 257, 28))

    first = run()
    hip.set_deterministic(True)      # no float atomics: deterministic mode has nothing to refuse
    try:
        second = run()
    finally:
        hip.set_deterministic(False)
    third = run()
    for other in (second, third):
        assert torch.equal(first[0][0], other[0][0]) and torch.equal(first[0][1], other[0][1]) and torch.equal(first[1], other[1])


# ------------------------------------------------------------------------------------------ 2. targets
def _rois(size, G, M, seed=0):
    """about 40 ROIs: (roi_inst int32 (P,), boxes float32 (P, 4))"""
    H, W = size
    rng = np.random.RandomState(seed + 31 * H + W + M)
    b = []
    for _ in range(10):                                   # inside, any size
        x1, y1 = rng.uniform(0, W - 2), rng.uniform(0, H - 2)
        b.append([x1, y1, rng.uniform(x1 + 1, W), rng.uniform(y1 + 1, H)])
    for _ in range(4):                                    # larger than M where the mask allows, and smaller than M
        x1, y1 = rng.uniform(0, 0.1 * W), rng.uniform(0, 0.1 * H)
        b.append([x1, y1, x1 + 0.85 * W, y1 + 0.85 * H])
        x1, y1 = rng.uniform(0, W - 8), rng.uniform(0, H - 8)
        b.append([x1, y1, x1 + rng.randint(2, 7), y1 + rng.randint(2, 7)])
    for _ in range(6):                                    # half-integer corners: the rounding ties
        x1, y1 = rng.randint(0, W // 2) + 0.5, rng.randint(0, H // 2) + 0.5
        b.append([x1, y1, x1 + rng.randint(1, W // 2), y1 + rng.randint(1, H // 2) + (0.0 if rng.rand() < 0.5 else 1.0)])
    b += [[-0.3 * W, -0.2 * H, 0.5 * W, 0.6 * H], [0.5 * W, 0.4 * H, 1.4 * W, 1.2 * H], [-5.0, 3.0, W + 9.0, H - 2.0],      # partly outside
          [-40.0, 2.0, -3.0, 20.0], [W + 3.0, 2.0, W + 30.0, 20.0], [4.0, -30.0, 20.0, -2.0], [4.0, H + 1.0, 20.0, H + 25.0],  # wholly outside
          [-3e9, -3e9, 3e9, 3e9], [0.0, 0.0, float(W), float(H)], [0.0, 0.0, W - 1.0, H - 1.0],
          [0.7 * W, 0.7 * H, 0.2 * W, 0.3 * H], [20.0, 10.0, 20.0, 30.0],                                                  # inverted, empty
          [12.0, 9.0, 13.0, 10.0], [W - 1.0, H - 1.0, float(W), float(H)], [0.2, 0.2, 0.4, 0.4]]                              # one pixel
    nan, inf = float("nan"), float("inf")
    b += [[nan, 2.0, 20.0, 20.0], [2.0, 2.0, 20.0, nan], [2.0, 2.0, inf, 20.0], [-inf, 2.0, 20.0, 20.0], [inf, inf, inf, inf]]
    boxes = torch.tensor(b, dtype=torch.float32)
    roi = torch.from_numpy(rng.randint(0, G, len(b)).astype(np.int32))
    roi[3], roi[11], roi[19] = -1, G, 2 ** 30
    roi[0] = G - 1                                        # the full mask under an inside box: all ones
    roi[-1] = G - 2                                       # (the random masks at the end of the set meet the odd boxes too)
    roi[24:27] = torch.tensor([G - 3, G - 4, G - 5], dtype=torch.int32)
    return roi, boxes


def targets_abi(hip, words, size, roi, boxes, M, G=None):
    H, W = size
    P = boxes.shape[0]
    out = torch.full((P, max(M, 1), max(M, 1)), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    code = hip._lib_raw().mmt_mask_words_targets(words.data_ptr(), words.shape[0] if G is None else G, H, W, roi.data_ptr(),
                                                 boxes.data_ptr(), P, M, out.data_ptr(), None)
    torch.cuda.synchronize()
    return code, out


@pytest.mark.parametrize("size", [(37, 53), (128, 150), (300, 257)], ids=ids)
@pytest.mark.parametrize("M", [1, 25, 28, 32])
def test_targets(hip, size, M):
    H, W = size
    m, words, rec = source(hip, size)
    G = len(m)
    roi, boxes = _rois(size, G, M)
    assert 35 <= len(roi) <= 50
    want = bf.targets(m, roi, boxes, M)
    none = torch.tensor([not (0 <= int(g) < G) or bf.window(b, W, H) is None for g, b in zip(roi, boxes)])
    assert int(none.sum()) == 8 and int(want[none].abs().sum()) == 0
    code, got = targets_abi(hip, words, size, roi.cuda(), boxes.cuda(), M)
    assert code == 0
    bad = (got.cpu() != want).flatten(1).any(1).nonzero().reshape(-1).tolist()
    print("%s M %d: %d ROIs, %d bits set, ROIs that differ: %s" % (size, M, len(roi), int(want.sum()), bad))
    assert torch.equal(got.cpu(), want)                   # every element written (none is NaN any more), zeros where no window
    assert 0 < int(want.sum()) < want.numel()
    assert torch.equal(hip.mask_words_targets(words, roi.cuda(), boxes.cuda(), H, W, M), got)


def test_targets_of_no_rois_or_no_masks_are_no_ops(hip):
    size = (37, 53)
    m, words, rec = source(hip, size)
    roi, boxes = _rois(size, len(m), 28)
    roi, boxes = roi.cuda(), boxes.cuda()
    code, out = targets_abi(hip, words, size, roi[:0], boxes[:0], 28)
    assert code == 0 and out.shape[0] == 0
    code, out = targets_abi(hip, words, size, roi, boxes, 28, G=0)
    assert code == 0 and bool(torch.isnan(out).all())
    assert hip._lib_raw().mmt_mask_words_targets(None, 0, 37, 53, None, None, 0, 28, None, None) == 0
    assert hip._lib_raw().mmt_mask_words_resample(None, 0, 37, 53, 0, 0, 53, 37, 0, 37, 53, None, None, None) == 0
    # the binding: zeros for ROIs that have no masks to take from, an empty stack for no ROIs
    assert int(hip.mask_words_targets(words[:0], roi, boxes, 37, 53, 28).abs().sum()) == 0
    assert hip.mask_words_targets(words, roi[:0], boxes[:0], 37, 53, 28).shape == (0, 28, 28)
    w0, r0 = hip.mask_words_resample(words[:0], 37, 53, (0, 0, 53, 37), 0, 20, 20)
    assert w0.shape == (0, 7) and r0.shape == (0, 8)


# ------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_write_nothing(hip):
    size = (37, 53)
    m, words, rec = source(hip, size)
    G = len(m)
    raw = hip._lib_raw()
    roi, boxes = _rois(size, G, 28)
    roi, boxes = roi.cuda(), boxes.cuda()
    for M in (0, 33, -1):
        code, out = targets_abi(hip, words, size, roi, boxes, M)
        assert code == EINVAL and bool(torch.isnan(out).all()), M
    for bad_size in ((16385, 1), (1, 16385), (16384, 4097), (8193, 8192), (0, 5), (5, -1)):
        code, out = targets_abi(hip, words, bad_size, roi, boxes, 28)
        assert code == EINVAL and bool(torch.isnan(out).all()), bad_size
    code, out = targets_abi(hip, words, size, roi, boxes, 28, G=65536)
    assert code == EINVAL and bool(torch.isnan(out).all())
    code, out = targets_abi(hip, words, size, roi, boxes, 28, G=-1)
    assert code == EINVAL and bool(torch.isnan(out).all())
    out = torch.full((len(roi), 28, 28), float("nan"), device="cuda")
    for args in ((None, roi, boxes, out), (words, None, boxes, out), (words, roi, None, out), (words, roi, boxes, None)):
        ptr = [None if a is None else a.data_ptr() for a in args]
        assert raw.mmt_mask_words_targets(ptr[0], G, 37, 53, ptr[1], ptr[2], len(roi), 28, ptr[3], None) == EINVAL
        assert raw.mmt_mask_words_targets(ptr[0], G, 37, 53, ptr[1], ptr[2], -1, 28, ptr[3], None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())

    def refused(size=size, win=(0, 0, 53, 37), flip=0, out_size=(30, 41), words=words):
        small = torch.empty((G, 64), dtype=torch.int64, device="cuda")   # (never written: sized for no particular output)
        small.view(torch.uint8).fill_(0xFF)
        code, o, r = resample_abi(hip, words, size, win, flip, out_size, out=small)
        return code == EINVAL and bool((o.view(torch.uint8) == 0xFF).all()) and bool((r.view(torch.uint8) == 0xFF).all())

    assert refused(size=(16385, 1), win=(0, 0, 1, 1)) and refused(size=(16384, 4097), win=(0, 0, 1, 1))
    assert refused(out_size=(16385, 1)) and refused(out_size=(1, 16385)) and refused(out_size=(8193, 8192)) and refused(out_size=(0, 4))
    for win in ((0, 0, 54, 37), (0, 0, 53, 38), (1, 0, 53, 37), (0, 1, 53, 37), (-1, 0, 5, 5), (0, -1, 5, 5), (3, 3, 0, 5), (3, 3, 5, 0),
                (53, 0, 1, 1), (0, 37, 1, 1), (2 ** 31 - 1, 0, 2, 2), (0, 0, 2 ** 31 - 1, 1)):
        assert refused(win=win), win
    assert refused(flip=4) and refused(flip=-1)
    # aliasing: the output on the input, or anywhere overlapping it
    keep = words.clone()
    nw = words.shape[1]
    rec2 = torch.full((G, 8), -1, dtype=torch.int32, device="cuda")
    for at in (0, 8 * (nw // 2), 8 * (G * nw - 1)):
        code = raw.mmt_mask_words_resample(keep.data_ptr(), G, 37, 53, 0, 0, 53, 37, 1, 37, 53, keep.data_ptr() + at, rec2.data_ptr(), None)
        assert code == EINVAL, at
    code = raw.mmt_mask_words_resample(keep.data_ptr() + 8 * nw, G - 1, 37, 53, 0, 0, 53, 37, 1, 37, 53, keep.data_ptr(), rec2.data_ptr(), None)
    assert code == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(keep, words) and bool((rec2 == -1).all())
    o, r = hip._mask_buffers(G, 30, 41, "cuda")
    for args in ((None, o, r), (words, None, r), (words, o, None)):
        ptr = [None if a is None else a.data_ptr() for a in args]
        assert raw.mmt_mask_words_resample(ptr[0], G, 37, 53, 0, 0, 53, 37, 0, 30, 41, ptr[1], ptr[2], None) == EINVAL
    assert raw.mmt_mask_words_resample(words.data_ptr(), 65536, 37, 53, 0, 0, 53, 37, 0, 30, 41, o.data_ptr(), r.data_ptr(), None) == EINVAL
    assert raw.mmt_mask_words_resample(words.data_ptr(), -1, 37, 53, 0, 0, 53, 37, 0, 30, 41, o.data_ptr(), r.data_ptr(), None) == EINVAL


def test_the_binding_refuses_host_tensors_and_passes_refusals_on(hip):
    m, words, rec = source(hip, (37, 53))
    roi, boxes = _rois((37, 53), len(m), 28)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        hip.mask_words_resample(words.cpu(), 37, 53, (0, 0, 53, 37), 0, 30, 41)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        hip.mask_words_targets(words.cpu(), roi.cuda(), boxes.cuda(), 37, 53, 28)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        hip.mask_words_targets(words, roi, boxes.cuda(), 37, 53, 28)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        hip.mask_words_targets(words, roi.cuda(), boxes, 37, 53, 28)
    with pytest.raises(RuntimeError):
        hip.mask_words_targets(words, roi.cuda(), boxes.cuda(), 37, 53, 33)
    with pytest.raises(RuntimeError):
        hip.mask_words_resample(words, 37, 53, (0, 0, 54, 37), 0, 30, 41)
    with pytest.raises(RuntimeError):
        hip.mask_words_resample(words, 37, 53, (0, 0, 53, 37), 0, 16385, 1)
    with pytest.raises(RuntimeError):
        hip.mask_words_resample(words[:, :-1], 37, 53, (0, 0, 53, 37), 0, 30, 41)


# ------------------------------------------------------------------------------------------ 4. the class
def test_class_round_trips(hip):
    from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle
    from maskrcnn_benchmark.structures.segmentation_mask import BinaryMaskList
    size = (37, 53)
    H, W = size
    m, words, rec = source(hip, size)
    G = len(m)
    for src in (m, m.cuda(), m.bool(), m.numpy()):
        b = BinaryMaskList(src, (W, H))
        got = b.get_mask_tensor()
        assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), m)
    assert torch.equal(b.mask_words()[0], words) and torch.equal(b.mask_words()[1], rec)
    assert torch.equal(b.decode(H, W).cpu(), m.to(torch.int32).sum(0).to(torch.int32))
    with pytest.raises(ValueError):
        b.decode(W, H)
    rles = mask_rle.encode(np.asfortranarray(m.numpy().transpose(1, 2, 0)))
    r = BinaryMaskList(rles, (W, H))
    assert r.rles() == rles and torch.equal(r.mask_words()[0], words) and torch.equal(r.mask_words()[1], rec)
    assert b.rles() == rles
    text = BinaryMaskList([dict(x, counts=x["counts"].decode("ascii")) for x in rles], (W, H))
    assert text.rles() == rles
    with pytest.raises(ValueError):
        BinaryMaskList([{"size": [H, W], "counts": [5, 7, H * W - 13]}], (W, H)).mask_words()   # runs that do not cover the mask
    # selection
    at = [3, 0, G - 1, 3]
    keep = torch.zeros(G, dtype=torch.bool)
    keep[::3] = True
    for item, rows in ((2, [2]), (-1, [G - 1]), (slice(1, 9, 2), list(range(1, 9, 2))), (at, at), (torch.tensor(at), at),
                       (torch.tensor(at).cuda(), at), (keep, keep.nonzero().reshape(-1).tolist()),
                       (keep.cuda(), keep.nonzero().reshape(-1).tolist())):
        s = b[item]
        assert len(s) == len(rows) and tuple(s.size) == (W, H)
        assert torch.equal(s.mask_words()[0], words[rows]) and torch.equal(s.mask_words()[1], rec[rows])
    assert [len(x) for x in b] == [1] * G and torch.equal(list(b)[5].mask_words()[0], words[5:6])
    # an empty list works everywhere
    for e in (BinaryMaskList([], (W, H)), b[[]], b[torch.zeros(G, dtype=torch.bool).cuda()]):
        assert len(e) == 0 and e.mask_words()[0].shape == (0, (H * W + 63) // 64) and e.rles() == []
        assert int(e.decode(H, W).abs().sum()) == 0 and e.get_mask_tensor().shape == (0, H, W)
        z = e.resize((20, 10)).transpose(0).crop([1, 1, 9, 9])
        assert len(z) == 0 and tuple(z.size) == (8, 8) and z.mask_words()[0].shape == (0, 1) and z.rles() == []
    # a resized list's strings
    big = b.resize((80, 56))
    want = bf.resample(m, (0, 0, W, H), 56, 80)
    assert big.rles() == mask_rle.encode(np.asfortranarray(want.numpy().transpose(1, 2, 0)))
    assert torch.equal(big.get_mask_tensor().cpu(), want)


@pytest.mark.parametrize("size", [(37, 53), (128, 150)], ids=ids)
def test_from_polygons_decodes_like_the_polygons(hip, size):
    from maskrcnn_benchmark.structures.segmentation_mask import BinaryMaskList, SegmentationMask
    H, W = size
    c = pi.cases(size)
    sm = SegmentationMask([[torch.from_numpy(p.reshape(-1).copy()) for p in inst] for inst in
                           ([pi.polygons_of(c, g) for g in range(len(c["inst_poly"]))])], (W, H), mode="poly")
    b = BinaryMaskList.from_polygons(sm)
    assert len(b) == len(sm) and tuple(b.size) == (W, H)
    assert torch.equal(b.decode(H, W), sm.decode(H, W))
    assert torch.equal(b.mask_words()[0], sm.mask_words()[0]) and torch.equal(b.mask_words()[1], sm.mask_words()[1])
    n = len(sm)
    assert torch.equal(b.mask_words()[0], source(hip, size)[1][:n])
