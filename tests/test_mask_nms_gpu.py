"""mmt_mask_nms (csrc/masknms.hip) through `_hip.mask_nms` and through the C ABI, against the plain formulation of
tests/mask_nms_formulation.py.  Everything is integer, so every comparison is equality: keep flags and count."""
import ctypes

import numpy as np
import pytest
import torch

import mask_nms_formulation as F

pytestmark = pytest.mark.gpu

EINVAL = -22


@pytest.fixture(scope="module")
def H():
    from maskrcnn_benchmark import _hip
    _hip.lib()
    return _hip


def _pack(H, masks):
    return H.mask_pack(torch.from_numpy(np.ascontiguousarray(masks).astype(np.uint8)).cuda())


def _run(H, masks, scores, labels, thresh, measure="iou", class_agnostic=False):
    words, rec = _pack(H, masks)
    keep, count = H.mask_nms(words, rec, torch.from_numpy(np.asarray(scores)).cuda(), torch.from_numpy(np.asarray(labels)).cuda(),
                             masks.shape[1], masks.shape[2], thresh, measure, class_agnostic)
    assert keep.dtype == torch.uint8 and tuple(keep.shape) == (masks.shape[0],) and keep.is_cuda
    assert count.dtype == torch.int32 and tuple(count.shape) == (1,) and count.is_cuda
    return keep.cpu().numpy(), int(count.item())


def _same(H, masks, scores, labels, thresh, measure="iou", class_agnostic=False, what=""):
    want = F.reference(masks, scores, labels, thresh, measure, class_agnostic)
    got, n = _run(H, masks, scores, labels, thresh, measure, class_agnostic)
    assert got.tolist() == want.tolist(), (what, got.tolist(), want.tolist())
    assert n == int(want.sum()), (what, n)
    return want


@pytest.mark.parametrize("size", F.SIZES, ids=["%dx%d" % s for s in F.SIZES])
def test_named_cases(H, size):
    for name, c in F.named_cases(*size).items():
        want = _same(H, c["masks"], c["scores"], c["labels"], c["thresh"], c["measure"], c["class_agnostic"], name)
        assert want.tolist() == c["expect"].tolist(), name


@pytest.fixture(scope="module")
def blobs():
    return F.random_blobs(200, 100, 120, seed=5)


@pytest.mark.parametrize("class_agnostic", [False, True], ids=["per-class", "agnostic"])
@pytest.mark.parametrize("measure", ["iou", "iomin"])
def test_200_random_blobs(H, blobs, measure, class_agnostic):
    want = _same(H, *blobs, 0.5, measure, class_agnostic)
    assert 0 < int(want.sum()) < 200
    # another threshold on the same masks: 0.3 acts as 314573 / 2^20
    _same(H, *blobs, 0.3, measure, class_agnostic)


def test_8_masks_at_1000x1000(H):
    masks, scores, labels = F.random_blobs(8, 1000, 1000, seed=2, n_labels=1)
    masks[5] = masks[1]          # a certain duplicate
    scores = np.asarray([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2], dtype=np.float32)
    want = _same(H, masks, scores, labels, 0.5)
    assert want[5] == 0 and (masks.shape[1] * masks.shape[2] + 63) // 64 == 15625


def test_one_detection_and_1024_detections(H):
    masks, scores, labels = F.random_blobs(1, 37, 53, seed=1)
    assert _same(H, masks, scores, labels, 0.5).tolist() == [1]
    assert _same(H, np.zeros((1, 37, 53), dtype=bool), scores, labels, 0.5).tolist() == [1]     # an empty mask stays
    masks, scores, labels = F.random_blobs(1024, 16, 16, seed=3)
    want = _same(H, masks, scores, labels, 0.5)
    assert 64 < int(want.sum()) < 1024       # more kept rows than one 64-position chunk of the sweep holds
    _same(H, masks, scores, labels, 0.25, "iomin", True)


def _raw(H, words, rec, order, labels, D, Hh, W, tq, measure, agnostic, ws, ws_bytes, keep, count):
    p = lambda t: None if t is None else t.data_ptr()
    return H.lib().mmt_mask_nms(p(words), p(rec), p(order), p(labels), D, Hh, W, tq, measure, agnostic, p(ws), ws_bytes, p(keep),
                                p(count), H._stream())


def _raw_inputs(H, D=6, size=(37, 53), seed=4):
    masks, _, labels = F.random_blobs(D, size[0], size[1], seed=seed, n_labels=1)
    masks[D - 1] = masks[0]                                         # the last row, with the lowest score, is a certain duplicate
    scores = np.linspace(0.9, 0.4, D).astype(np.float32)
    words, rec = _pack(H, masks)
    order = torch.sort(torch.from_numpy(scores).cuda(), descending=True, stable=True)[1].to(torch.int32)
    lab = torch.from_numpy(labels).cuda().to(torch.int32)
    need = ctypes.c_int64(0)
    assert H.lib().mmt_mask_nms_workspace(D, ctypes.byref(need)) == 0 and need.value >= D * D
    ws = torch.empty((need.value,), dtype=torch.uint8, device="cuda")
    return masks, scores, labels, words, rec, order, lab, ws, int(need.value)


def test_every_output_is_written(H):
    masks, scores, labels, words, rec, order, lab, ws, need = _raw_inputs(H)
    D = masks.shape[0]
    ws.fill_(0xFF)
    keep = torch.full((D + 8,), 0xFF, dtype=torch.uint8, device="cuda")     # eight guard bytes behind the flags
    count = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    assert _raw(H, words, rec, order, lab, D, 37, 53, F.quantise(0.5), 0, 0, ws, need, keep, count) == 0
    want = F.reference(masks, scores, labels, 0.5)
    k = keep.cpu().numpy()
    assert set(k[:D].tolist()) <= {0, 1} and k[:D].tolist() == want.tolist() and want[D - 1] == 0
    assert (k[D:] == 0xFF).all()
    assert count.cpu().tolist() == [int(want.sum()), -1]


def test_deterministic_mode_same_bytes(H):
    masks, scores, labels = F.random_blobs(200, 100, 120, seed=9)
    was = H.get_deterministic()
    got = []
    try:
        for mode in (True, True, False, False):
            H.set_deterministic(mode)
            got.append(_run(H, masks, scores, labels, 0.5))
    finally:
        H.set_deterministic(was)
    for k, n in got[1:]:
        assert k.tobytes() == got[0][0].tobytes() and n == got[0][1]
    assert got[0][0].tolist() == F.reference(masks, scores, labels, 0.5).tolist()


def test_refusals_through_the_c_abi(H):
    masks, scores, labels, words, rec, order, lab, ws, need = _raw_inputs(H)
    D, tq = masks.shape[0], F.quantise(0.5)
    keep = torch.full((D,), 0xFF, dtype=torch.uint8, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    args = dict(words=words, rec=rec, order=order, labels=lab, D=D, Hh=37, W=53, tq=tq, measure=0, agnostic=0, ws=ws, ws_bytes=need,
                keep=keep, count=count)
    for change in (dict(D=1025), dict(tq=0), dict(tq=(1 << 20) + 1), dict(measure=2), dict(ws_bytes=need - 1), dict(keep=None),
                   dict(D=-1), dict(measure=-1), dict(Hh=0), dict(W=-3), dict(Hh=1 << 16, W=1 << 15), dict(ws=None), dict(count=None),
                   dict(words=None), dict(order=None)):
        assert _raw(H, **dict(args, **change)) == EINVAL, change
    torch.cuda.synchronize()
    assert (keep.cpu().numpy() == 0xFF).all() and count.cpu().tolist() == [-1]      # nothing was launched: nothing was written
    assert _raw(H, **args) == 0 and int(count.item()) == int(F.reference(masks, scores, labels, 0.5).sum())
    # the wrapper refuses the same before any launch
    s, lb = torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda()
    for bad in (dict(thresh=0.0), dict(thresh=1.5), dict(measure="dice")):
        kw = dict(dict(thresh=0.5, measure="iou"), **bad)
        with pytest.raises(RuntimeError):
            H.mask_nms(words, rec, s, lb, 37, 53, kw["thresh"], kw["measure"])
    with pytest.raises(RuntimeError):
        H.mask_nms(words, rec, s, lb, 37, 60, 0.5)                                   # the words of a 37 x 53 image
    big = torch.zeros((1025, 1), dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="1024"):
        H.mask_nms(big, torch.zeros((1025, 8), dtype=torch.int32, device="cuda"), torch.zeros(1025, device="cuda"),
                   torch.zeros(1025, dtype=torch.int64, device="cuda"), 8, 8, 0.5)


def test_no_detections_write_a_zero_count(H):
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    assert _raw(H, None, None, None, None, 0, 37, 53, F.quantise(0.5), 0, 0, None, 0, None, count) == 0
    assert count.cpu().tolist() == [0]
    words, rec = H.mask_pack(torch.zeros((0, 37, 53), dtype=torch.uint8, device="cuda"))
    keep, n = H.mask_nms(words, rec, torch.zeros(0, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"), 37, 53, 0.5)
    assert tuple(keep.shape) == (0,) and n.cpu().tolist() == [0]
