"""The image-size polygon rasteriser on the MI355X (csrc/polyfill.hip: `mmt_polygon_mask_words`, `mmt_mask_words_integral`) and
what is built on it, against the oracle's rleFrPoly restatement (oracle.native.poly_mask) on the inputs of
tests/polygon_image_inputs.py -- which tests/test_polygon_image_inputs.py holds against the oracle alone.  Nothing here has a
tolerance: words, records, integral maps and strings are compared with equality."""
import ctypes

import numpy as np
import pytest
import torch

import polygon_image_inputs as pi

pytestmark = pytest.mark.gpu

EINVAL = -22
ALL_SIZES = pi.SIZES + [pi.BIG]
ids = lambda s: "%dx%d" % s   # noqa: E731


@pytest.fixture(scope="module")
def hip():
    from maskrcnn_benchmark import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return _hip


_DEV, _WANT = {}, {}


def dev_cases(size):
    """(xy, poly_off, inst_poly) of the size's cases on the device, made once"""
    if size not in _DEV:
        c = pi.cases(size)
        _DEV[size] = tuple(torch.from_numpy(c[k].copy()).cuda() for k in ("poly_xy", "poly_off", "inst_poly"))
    return _DEV[size]


def want(hip, size):
    """mmt_mask_pack of the oracle's masks: (words, records), made once per size"""
    if size not in _WANT:
        _WANT[size] = hip.mask_pack(torch.from_numpy(pi.oracle_masks(size).copy()).cuda())
    return _WANT[size]


def words_through_the_abi(hip, size, fill=0xFF, ws_words=None, inst=None):
    """mmt_polygon_mask_words into outputs and a workspace whose every byte is `fill` beforehand -> (code, words, rec)"""
    H, W = size
    xy, off, rng = dev_cases(size)
    rng = rng if inst is None else inst
    NP = off.numel() - 1
    need = hip.polygon_workspace_words(NP, H, W)
    ws = torch.empty((max(need, 1),), dtype=torch.int64, device="cuda")
    words, rec = hip._mask_buffers(rng.shape[0], H, W, xy.device)
    for t in (ws, words, rec):
        t.view(torch.uint8).fill_(fill)
    torch.cuda.synchronize()
    code = hip._lib_raw().mmt_polygon_mask_words(xy.data_ptr(), off.data_ptr(), NP, rng.data_ptr(), rng.shape[0], H, W, ws.data_ptr(),
                                                 need if ws_words is None else ws_words, words.data_ptr(), rec.data_ptr(), None)
    torch.cuda.synchronize()
    return code, words, rec


# ------------------------------------------------------------------------------------------ 1. words and records
@pytest.mark.parametrize("size", ALL_SIZES, ids=ids)
def test_words_and_records_equal_the_packed_oracle_masks(hip, size):
    H, W = size
    want_w, want_r = want(hip, size)
    code, got_w, got_r = words_through_the_abi(hip, size)
    assert code == 0
    assert got_w.shape == want_w.shape == (len(pi.cases(size)["inst_poly"]), (H * W + 63) // 64)
    bad = (got_w != want_w).any(1).nonzero().reshape(-1).tolist()
    print("%dx%d: %d instances, %d pixels set, instances that differ: %s" % (H, W, len(want_w), int(want_r[:, 0].sum()),
                                                                            [(g, pi.cases(size)["cls"][g]) for g in bad]))
    assert torch.equal(got_w, want_w)
    assert torch.equal(got_r, want_r)
    # the binding
    w2, r2 = hip.polygon_mask_words(*dev_cases(size), H, W)
    assert torch.equal(w2, want_w) and torch.equal(r2, want_r)


@pytest.mark.parametrize("size", [(37, 53), (150, 128), pi.BIG], ids=ids)
def test_everything_is_written_and_the_workspace_is_cleared_by_the_library(hip, size):
    a = words_through_the_abi(hip, size, fill=0xFF)
    b = words_through_the_abi(hip, size, fill=0x00)
    c = words_through_the_abi(hip, size, fill=0x5A)
    assert a[0] == b[0] == c[0] == 0
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[1], c[1]) and torch.equal(a[2], c[2])
    assert torch.equal(a[1], want(hip, size)[0])


def test_two_runs_give_equal_bits(hip):
    for size in ((128, 150), pi.BIG):
        runs = [hip.polygon_mask_words(*dev_cases(size), *size) for _ in range(2)]
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    hip.set_deterministic(True)      # integer atomics: deterministic mode has nothing to refuse
    try:
        w, r = hip.polygon_mask_words(*dev_cases((128, 150)), 128, 150)
    finally:
        hip.set_deterministic(False)
    assert torch.equal(w, want(hip, (128, 150))[0]) and torch.equal(r, want(hip, (128, 150))[1])


# ------------------------------------------------------------------------------------------ 2. workspace and chunks
@pytest.mark.parametrize("size", [(37, 53), (150, 128)], ids=ids)
def test_small_workspace_is_refused_and_the_wrapper_splits_the_call(hip, size, monkeypatch):
    H, W = size
    xy, off, rng = dev_cases(size)
    NP = off.numel() - 1
    need = hip.polygon_workspace_words(NP, H, W)
    assert need >= NP * ((H * W + 63) // 64)
    code, words, rec = words_through_the_abi(hip, size, ws_words=need - 1)
    assert code == EINVAL
    assert bool((words.view(torch.uint8) == 0xFF).all()) and bool((rec.view(torch.uint8) == 0xFF).all())
    # room for about five polygons per call; a single instance of more polygons still gets what it needs
    monkeypatch.setattr(hip, "POLYGON_WS_WORDS", hip.polygon_workspace_words(5, H, W))
    calls = hip.C_CALLS[0]
    w2, r2 = hip.polygon_mask_words(xy, off, rng, H, W)
    assert hip.C_CALLS[0] - calls > 3
    assert torch.equal(w2, want(hip, size)[0]) and torch.equal(r2, want(hip, size)[1])
    monkeypatch.setattr(hip, "POLYGON_WS_WORDS", 1)           # one instance per call
    w3, r3 = hip.polygon_mask_words(xy, off, rng, H, W)
    assert torch.equal(w3, want(hip, size)[0]) and torch.equal(r3, want(hip, size)[1])


def test_no_instances(hip):
    H, W = 37, 53
    xy, off, rng = dev_cases((H, W))
    code, words, rec = words_through_the_abi(hip, (H, W), inst=rng[:0].contiguous())
    assert code == 0 and words.shape[0] == 0
    L = hip._lib_raw()
    guard = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    assert L.mmt_polygon_mask_words(None, None, 0, None, 0, H, W, None, 0, guard.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert bool((guard == -1).all())
    w, r = hip.polygon_mask_words(xy, off, rng[:0], H, W)
    assert tuple(w.shape) == (0, (H * W + 63) // 64) and tuple(r.shape) == (0, 8)
    seg = hip.mask_words_integral(w, [0, 0, 0], H, W)
    assert tuple(seg.shape) == (2, H, W) and seg.dtype == torch.int32 and int(seg.abs().sum()) == 0
    # no polygons at all, but instances (empty ranges): empty masks
    z = torch.zeros((3, 2), dtype=torch.int32, device="cuda")
    w, r = hip.polygon_mask_words(torch.zeros(0, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), z, H, W)
    assert int(w.abs().sum()) == 0 and int(r.abs().sum()) == 0 and w.shape[0] == 3


# ------------------------------------------------------------------------------------------ 3. integral map
def integral_through_the_abi(hip, words, off, H, W):
    seg = torch.empty((len(off) - 1, H, W), dtype=torch.int32, device="cuda")
    seg.view(torch.uint8).fill_(0xFF)
    torch.cuda.synchronize()
    arr = (ctypes.c_int32 * len(off))(*off)
    code = hip._lib_raw().mmt_mask_words_integral(words.data_ptr(), ctypes.cast(arr, ctypes.c_void_p), len(off) - 1, H, W,
                                                  seg.data_ptr(), None)
    torch.cuda.synchronize()
    return code, seg


@pytest.mark.parametrize("size", ALL_SIZES, ids=ids)
def test_integral_equals_the_sum_of_the_oracle_masks(hip, size):
    H, W = size
    m = pi.oracle_masks(size).astype(np.int32)
    G = len(m)
    words = want(hip, size)[0]
    code, seg = integral_through_the_abi(hip, words, [0, G], H, W)
    assert code == 0 and np.array_equal(seg.cpu().numpy()[0], m.sum(0))
    assert m.sum(0).max() > 1 or H * W == 1                      # instances overlap: the map is not a mask
    # three images, the middle one without instances, the third not starting at a multiple of anything
    a = G // 3 + 1
    off = [0, a, a, G]
    code, seg = integral_through_the_abi(hip, words, off, H, W)
    assert code == 0
    got = seg.cpu().numpy()
    assert np.array_equal(got[0], m[:a].sum(0)) and int(np.abs(got[1]).sum()) == 0 and np.array_equal(got[2], m[a:].sum(0))
    assert torch.equal(hip.mask_words_integral(words, torch.tensor(off), H, W), seg)
    # a first image that does not start at mask 0
    code, seg = integral_through_the_abi(hip, words, [2, G - 1], H, W)
    assert code == 0 and np.array_equal(seg.cpu().numpy()[0], m[2:G - 1].sum(0))


# ------------------------------------------------------------------------------------------ 4. structures and codec
def _segmentation_mask(size):
    from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask
    c = pi.cases(size)
    keep = [g for g in range(len(c["inst_poly"])) if c["inst_poly"][g, 1] > c["inst_poly"][g, 0]]
    polys = [[torch.from_numpy(p.reshape(-1).copy()) for p in pi.polygons_of(c, g)] for g in keep]
    return SegmentationMask(polys, (size[1], size[0]), mode="poly"), keep


@pytest.mark.parametrize("size", [(37, 53), (128, 150), pi.BIG], ids=ids)
def test_decode_and_convert(hip, size):
    H, W = size
    sm, keep = _segmentation_mask(size)
    m = pi.oracle_masks(size)[keep]
    got = sm.decode(H, W)
    assert got.dtype == torch.int32 and tuple(got.shape) == (H, W) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), m.astype(np.int32).sum(0))
    words, rec = sm.mask_words()
    assert sm.mask_words()[0] is words and sm.mask_words("cuda")[0] is words     # cached beside the packed vertices
    assert torch.equal(words, want(hip, size)[0][keep]) and torch.equal(rec, want(hip, size)[1][keep])
    for g in (0, len(keep) // 2, len(keep) - 1):
        one = sm.polygons[g].convert("mask")
        assert one.dtype == torch.uint8 and tuple(one.shape) == (H, W) and one.is_cuda
        assert np.array_equal(one.cpu().numpy(), m[g])
    with pytest.raises(ValueError):
        sm.decode(H + 1, W)


def test_decode_of_an_empty_list(hip):
    from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask
    z = SegmentationMask([], (53, 37), mode="poly").decode(37, 53)
    assert z.dtype == torch.int32 and tuple(z.shape) == (37, 53) and z.is_cuda and int(z.abs().sum()) == 0


@pytest.mark.parametrize("size", [(1, 1), (37, 53), (150, 128), (5, 200), pi.BIG], ids=ids)
def test_device_strings_equal_the_host_strings(hip, size):
    from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle
    H, W = size
    segm = pi.segm_of(pi.cases(size))
    got = mask_rle.frPolygons(segm, H, W, on_device=True)
    host = mask_rle.frPolygons(segm, H, W)
    assert got == host and len(got) == len(segm)
    assert got == [mask_rle.encode(m) for m in pi.oracle_masks(size)]
    assert mask_rle.frPolygons([], H, W, on_device=True) == []


# ------------------------------------------------------------------------------------------ 5. refused arguments
def test_entry_points_refuse_bad_arguments_and_write_nothing(hip):
    L = hip._lib_raw()
    H, W = 37, 53
    xy, off, rng = dev_cases((H, W))
    NP, G = off.numel() - 1, rng.shape[0]
    need = hip.polygon_workspace_words(NP, H, W)
    ws = torch.empty((need,), dtype=torch.int64, device="cuda")
    words, rec = hip._mask_buffers(G, H, W, xy.device)
    for t in (ws, words, rec):
        t.view(torch.uint8).fill_(0xFF)
    torch.cuda.synchronize()
    outside = [torch.tensor(v, dtype=torch.int32, device="cuda") for v in ([[0, NP + 1]], [[-1, 1]], [[NP + 1, NP + 1]], [[0, 1], [2, -3]])]

    def call(xy=xy.data_ptr(), off=off.data_ptr(), NP=NP, rng=rng.data_ptr(), G=G, H=H, W=W, ws=ws.data_ptr(), ws_words=need,
             words=words.data_ptr(), rec=rec.data_ptr()):
        return L.mmt_polygon_mask_words(xy, off, NP, rng, G, H, W, ws, ws_words, words, rec, None)

    refused = {
        "null xy": dict(xy=None), "null poly_off": dict(off=None), "null inst_poly": dict(rng=None), "null ws": dict(ws=None),
        "null words": dict(words=None), "null rec": dict(rec=None),
        "H == 0": dict(H=0), "H < 0": dict(H=-37), "W == 0": dict(W=0), "W < 0": dict(W=-53),
        "H * W == 2^31": dict(H=65536, W=32768), "H * W >= 2^31": dict(H=46341, W=46341),
        "G < 0": dict(G=-1), "G > 65535": dict(G=65536), "NP < 0": dict(NP=-1),
        "workspace one word short": dict(ws_words=need - 1), "no workspace": dict(ws_words=0),
    }
    for i, t in enumerate(outside):
        refused["inst_poly outside [0, NP] (%d)" % i] = dict(rng=t.data_ptr(), G=t.shape[0])
    for name, kw in refused.items():
        assert call(**kw) == EINVAL, name
    torch.cuda.synchronize()
    for t in (words, rec):
        assert bool((t.view(torch.uint8) == 0xFF).all())
    n = ctypes.c_int64(-1)
    for kw in (dict(NP=-1), dict(H=0), dict(W=-1), dict(H=65536, W=32768)):
        a = dict(NP=NP, H=H, W=W)
        a.update(kw)
        assert L.mmt_polygon_mask_words_workspace(a["NP"], a["H"], a["W"], ctypes.byref(n)) == EINVAL
    assert L.mmt_polygon_mask_words_workspace(NP, H, W, None) == EINVAL
    assert L.mmt_polygon_mask_words_workspace(0, H, W, ctypes.byref(n)) == 0 and n.value == 0
    # and the arguments as they are do run
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(words, want(hip, (H, W))[0]) and torch.equal(rec, want(hip, (H, W))[1])

    seg = torch.empty((1, H, W), dtype=torch.int32, device="cuda")
    seg.view(torch.uint8).fill_(0xFF)
    torch.cuda.synchronize()

    def integral(words=words.data_ptr(), off=(0, G), N=1, H=H, W=W, seg=seg.data_ptr()):
        arr = None if off is None else ctypes.cast((ctypes.c_int32 * len(off))(*off), ctypes.c_void_p)
        return L.mmt_mask_words_integral(words, arr, N, H, W, seg, None)

    refused = {
        "null words": dict(words=None), "null img_off": dict(off=None), "null seg": dict(seg=None),
        "N < 0": dict(N=-1), "H == 0": dict(H=0), "W < 0": dict(W=-53), "H * W == 2^31": dict(H=65536, W=32768),
        "negative start": dict(off=(-1, G)), "falling offsets": dict(off=(3, 2)), "more than 65535 instances": dict(off=(0, 65536)),
    }
    for name, kw in refused.items():
        assert integral(**kw) == EINVAL, name
    torch.cuda.synchronize()
    assert bool((seg.view(torch.uint8) == 0xFF).all())
    assert integral(N=0, off=None, seg=None, words=None) == 0
    assert integral(words=None, off=(0, 0)) == 0                  # an image without instances needs no words
    torch.cuda.synchronize()
    assert int(seg.abs().sum()) == 0
