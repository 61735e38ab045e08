"""mmt_soft_nms_batched and mmt_det_postprocess_soft (csrc/softnms.hip, csrc/select.hip) through `_hip` and through the C ABI,
against the plain formulation of tests/soft_nms_formulation.py.  The linear method is compared by equality with the float32
restatement; the gaussian method by pick order with the float64 oracle and by a tolerance computed here."""
import ctypes

import numpy as np
import pytest
import torch

import soft_nms_formulation as F

pytestmark = pytest.mark.gpu

EINVAL = -22
# the sizes of the issue, and those where a thread takes its second, third and fourth candidate (512 threads per segment)
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024, 1025, 1537, 2048)
LIN = dict(nms_thresh=0.5, sigma=0.5, min_score=0.001)


@pytest.fixture(scope="module")
def H():
    from maskrcnn_benchmark import _hip
    _hip.lib()
    return _hip


def _cat(segs):
    """[(boxes, scores)] with an empty segment in front of, between and behind them -> boxes, scores, seg_off, bounds"""
    offs, bounds = [0], []
    for b, s in segs:
        offs.append(offs[-1])                       # an empty one
        bounds.append((offs[-1], offs[-1] + len(s)))
        offs.append(offs[-1] + len(s))
    offs.append(offs[-1])
    boxes = np.concatenate([b for b, _ in segs]).astype(np.float32).reshape(-1, 4)
    scores = np.concatenate([s for _, s in segs]).astype(np.float32)
    return boxes, scores, np.asarray(offs, np.int32), bounds


def _expected(segs, method, max_n, dtype=np.float32, thr=0.5, sigma=0.5, min_score=0.001):
    """the formulation per segment -> picked (B, max_n) with -1 where nothing is written, counts, scores"""
    B = 2 * len(segs) + 1
    picked = np.full((B, max_n), -1, np.int32)
    cnt = np.zeros(B, np.int32)
    out = []
    for i, (b, s) in enumerate(segs):
        p, sc = F.soft_nms(b, s, method, thr, sigma, min_score, dtype)
        picked[2 * i + 1, :len(p)] = p
        cnt[2 * i + 1] = len(p)
        out.append(sc)
    return picked, cnt, np.concatenate(out)


def _raw(H, boxes, scores, seg_off, B, max_n, method, thr, sigma, min_score, picked, cnt, out):
    p = lambda t: None if t is None else t.data_ptr()
    return H.lib().mmt_soft_nms_batched(p(boxes), p(scores), p(seg_off), B, max_n, method, thr, sigma, min_score, p(picked), p(cnt),
                                        p(out), H._stream())


def _run_raw(H, segs, method, max_n, **kw):
    """through the C ABI with 0xFF-filled outputs: what is not written stays -1"""
    boxes, scores, offs, bounds = _cat(segs)
    B = len(offs) - 1
    t = lambda a: torch.from_numpy(a).cuda()
    picked = torch.full((B, max_n), -1, dtype=torch.int32, device="cuda")
    cnt = torch.full((B + 1,), -1, dtype=torch.int32, device="cuda")
    out = torch.full((len(scores) + 1,), float("nan"), dtype=torch.float32, device="cuda")
    k = dict(LIN, **kw)
    assert _raw(H, t(boxes), t(scores), t(offs), B, max_n, method, k["nms_thresh"], k["sigma"], k["min_score"], picked, cnt, out) == 0
    torch.cuda.synchronize()
    cnt, out = cnt.cpu().numpy(), out.cpu().numpy()
    assert cnt[B] == -1 and np.isnan(out[-1])                  # the guards behind the arrays
    return picked.cpu().numpy(), cnt[:B], out[:-1]


@pytest.mark.parametrize("kind", sorted(F.KINDS))
def test_linear_is_the_float32_formulation_bit_for_bit(H, kind):
    segs = [F.KINDS[kind](n) for n in SIZES]
    want_p, want_c, want_s = _expected(segs, "linear", 2048)
    got_p, got_c, got_s = _run_raw(H, segs, 0, 2048)
    print("%s: picks per segment %s" % (kind, want_c[1::2].tolist()))
    assert got_c.tolist() == want_c.tolist()
    assert np.array_equal(got_p, want_p)                       # (and -1 behind every count: nothing else is written)
    assert got_s.tobytes() == want_s.tobytes()
    # what the kinds are there for
    n = np.asarray(SIZES)
    if kind == "all-equal":
        assert want_c[1::2].tolist() == (n > 0).astype(int).tolist()
    if kind in ("disjoint", "chain"):
        assert want_c[1::2].tolist() == n.tolist()
    if kind == "disjoint":
        assert np.array_equal(want_p[-2], np.arange(2048))
    if kind == "chain":
        assert not np.array_equal(want_p[-2], np.arange(2048))  # decayed boxes are overtaken
    if kind in ("clustered", "equal-scores"):
        assert 1024 < want_c[-2] < 2048                        # some fall below MIN_SCORE, most are picked


def test_wrapper_and_a_smaller_bound(H):
    """`_hip.soft_nms_batched` on the same data with max_n = the longest segment, torch tensors in and out"""
    segs = [F.KINDS["clustered"](n) for n in (65, 0, 257)]
    boxes, scores, offs, _ = _cat(segs)
    want_p, want_c, want_s = _expected(segs, "linear", 257)
    picked, cnt, out = H.soft_nms_batched(torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(offs).cuda(),
                                          257, "linear", 0.5, 0.5, 0.001)
    assert picked.dtype == torch.int32 and tuple(picked.shape) == (7, 257) and cnt.dtype == torch.int32 and out.dtype == torch.float32
    assert torch.equal(cnt.cpu(), torch.from_numpy(want_c))
    for b in range(7):
        assert torch.equal(picked[b, :want_c[b]].cpu(), torch.from_numpy(want_p[b, :want_c[b]]))
    assert torch.equal(out.cpu(), torch.from_numpy(want_s))
    assert H.soft_nms_batched(torch.zeros((4096, 4)).cuda(), torch.zeros(4096).cuda(), torch.tensor([0, 4096], dtype=torch.int32).cuda(),
                              4096) is None
    # in place: out_scores may be the scores array
    t = lambda a: torch.from_numpy(a).cuda()
    sc = t(scores)
    pk = torch.empty((7, 257), dtype=torch.int32, device="cuda")
    ct = torch.empty((7,), dtype=torch.int32, device="cuda")
    assert _raw(H, t(boxes), sc, t(offs), 7, 257, 0, 0.5, 0.5, 0.001, pk, ct, sc) == 0
    assert torch.equal(sc.cpu(), torch.from_numpy(want_s)) and torch.equal(ct.cpu(), torch.from_numpy(want_c))


def test_gaussian_pick_order_and_scores(H):
    tol = F.gaussian_tolerance()
    segs = [F.clustered(n, seed) for n, seed in F.GAUSS_INPUTS]
    g = F.GAUSS
    want_p, want_c, want_s = _expected(segs, "gaussian", 64, np.float64, g["thr"], g["sigma"], g["min_score"])
    got_p, got_c, got_s = _run_raw(H, segs, 1, 64, nms_thresh=g["thr"], sigma=g["sigma"], min_score=g["min_score"])
    dev = F.rel_dev(got_s, want_s)
    print("gaussian: tolerance %.3e (4 x the float32 restatement's deviation from float64), the kernel deviates by %.3e" % (tol, dev))
    assert got_c.tolist() == want_c.tolist()
    assert np.array_equal(got_p, want_p)
    assert dev <= tol
    # the threshold plays no part in the gaussian method, sigma does
    again = _run_raw(H, segs, 1, 64, nms_thresh=0.9, sigma=g["sigma"], min_score=g["min_score"])
    assert np.array_equal(again[0], got_p) and again[2].tobytes() == got_s.tobytes()
    wide = _run_raw(H, segs, 1, 64, nms_thresh=g["thr"], sigma=2.0, min_score=g["min_score"])
    assert wide[2].tobytes() != got_s.tobytes()


# ------------------------------------------------------------------------------------------------------ det_postprocess_soft
def _det_inputs(n, nc, seed):
    """two images of n and n // 2 + 1 rows: clustered boxes per class; probabilities in steps of 1 / 64, so that equal scores
    meet in the sort and at the cut, a fifth of them below the score threshold"""
    rng = np.random.RandomState(seed)
    per = [n, n // 2 + 1]
    R = sum(per)
    prob = (rng.randint(4, 64, size=(R, nc)) / 64.0).astype(np.float32)
    prob[rng.uniform(size=(R, nc)) < 0.2] = 1.0 / 64.0          # below SCORE_THRESH
    dec = np.zeros((R, nc * 4), np.float32)
    for j in range(nc):
        b, _ = F.clustered(R, seed * 64 + j)
        dec[:, 4 * j:4 * j + 4] = b[rng.permutation(R)]
    return prob, dec, per


def _raw_det(H, prob, dec, per, nc, thr, nms, D, method, sigma, min_score, soft=True):
    """through the C ABI with 0xFF-filled outputs -> boxes, scores, labels, counts (numpy, whole arrays), return code"""
    N = len(per)
    offs = np.concatenate([[0], np.cumsum(per)]).astype(np.int32)
    host = (ctypes.c_int32 * (N + 1))(*offs.tolist())
    fn = H.lib().mmt_det_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_long, [ctypes.c_int] * 3
    ws = torch.empty((fn(int(offs[-1]), N, nc) // 16 + 1, 4), dtype=torch.float32, device="cuda")
    cap = max(max(per) * (nc - 1), 1)
    ob = torch.full((N, cap, 4), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    os_ = torch.full((N, cap), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    ol = torch.full((N, cap), -1, dtype=torch.int64, device="cuda")
    oc = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    p, d, ro = torch.from_numpy(prob).cuda(), torch.from_numpy(dec).cuda(), torch.from_numpy(offs).cuda()
    if soft:
        rc = H.lib().mmt_det_postprocess_soft(p.data_ptr(), d.data_ptr(), ro.data_ptr(), ctypes.cast(host, ctypes.c_void_p), N, nc, thr,
                                              nms, D, method, sigma, min_score, ws.data_ptr(), ob.data_ptr(), os_.data_ptr(),
                                              ol.data_ptr(), oc.data_ptr(), H._stream())
    else:
        rc = H.lib().mmt_det_postprocess(p.data_ptr(), d.data_ptr(), ro.data_ptr(), ctypes.cast(host, ctypes.c_void_p), N, nc, thr, nms,
                                         D, ws.data_ptr(), ob.data_ptr(), os_.data_ptr(), ol.data_ptr(), oc.data_ptr(), H._stream())
    torch.cuda.synchronize()
    return ob.view(torch.int32).cpu().numpy(), os_.view(torch.int32).cpu().numpy(), ol.cpu().numpy(), oc.cpu().numpy(), rc


def _check_det(got, want):
    ob, os_, ol, oc, rc = got
    assert rc == 0
    assert oc.tolist() == [len(w[1]) for w in want]
    for i, (bb, sc, lb) in enumerate(want):
        n = len(sc)
        assert ob[i, :n].tobytes() == bb.astype(np.float32).tobytes()
        assert os_[i, :n].tobytes() == sc.astype(np.float32).tobytes()
        assert ol[i, :n].tolist() == lb.tolist()
        assert (ob[i, n:] == -1).all() and (os_[i, n:] == -1).all() and (ol[i, n:] == -1).all()      # the tails are not written


@pytest.mark.parametrize("nc", [3, 4], ids=["two-classes", "three-classes"])
@pytest.mark.parametrize("n", [65, 257, 2048])
def test_det_postprocess_soft_is_filter_results_soft(H, n, nc):
    prob, dec, per = _det_inputs(n, nc, seed=n + nc)
    full = F.filter_results_soft(prob, dec, per, 0.05, 0.5, 0, "linear", 0.5, 0.001)       # once; the cuts are taken from it
    small, large = len(full[1][1]), len(full[0][1])
    assert 8 < small < large
    for bb, sc, lb in full:
        assert len(np.unique(sc)) < len(sc) and set(lb.tolist()) == set(range(1, nc))
    # DETECTIONS_PER_IMG: none, below, at and above the smaller image's survivor count (the larger image is cut by all three)
    cuts = [0, small // 2, small, small + 1]
    # and one that falls on a tie: the cut keeps more than D
    tie = next(D for D in range(2, small) if len(F.cut_detections(full, D)[1][1]) > D)
    for D in cuts + [tie]:
        want = F.cut_detections(full, D)
        _check_det(_raw_det(H, prob, dec, per, nc, 0.05, 0.5, D, 0, 0.5, 0.001), want)
    print("n = %d, nc = %d: %d and %d survivors, cuts %s, D = %d keeps %d" % (n, nc, large, small, cuts, tie,
                                                                             len(F.cut_detections(full, tie)[1][1])))


def test_without_overlaps_linear_is_the_existing_path(H):
    """no two candidates of a class reach IoU >= thr: nothing decays, every candidate is picked, and mmt_det_postprocess_soft
    returns what mmt_det_postprocess returns, bit for bit"""
    rng = np.random.RandomState(11)
    nc, per = 3, [300, 257]
    R = sum(per)
    prob = rng.uniform(0.0, 1.0, size=(R, nc)).astype(np.float32)
    prob[::7] = 0.01
    dec = np.zeros((R, nc * 4), np.float32)
    for j in range(nc):
        b, _ = F.disjoint(R)
        jit = rng.uniform(0.0, 2.0, size=(R, 1)).astype(np.float32)        # boxes of 9 px, 15 px apart: still disjoint
        dec[:, 4 * j:4 * j + 4] = (b + jit)[rng.permutation(R)]
    for D in (0, 100, 200):
        hard = _raw_det(H, prob, dec, per, nc, 0.05, 0.5, D, 0, 0.5, 0.001, soft=False)
        soft = _raw_det(H, prob, dec, per, nc, 0.05, 0.5, D, 0, 0.5, 0.001)
        assert hard[4] == 0 and soft[4] == 0 and hard[3].min() > 0
        for a, b in zip(hard[:4], soft[:4]):
            assert a.tobytes() == b.tobytes()
    # and the wrapper pair
    p, d = torch.from_numpy(prob).cuda(), torch.from_numpy(dec).cuda()
    a = H.det_postprocess(p, d, per, 0.05, 0.5, 100, zero_tails=True)
    b = H.det_postprocess_soft(p, d, per, 0.05, 0.5, 100, zero_tails=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_every_refusal_returns_einval_and_writes_nothing(H):
    b, s = F.clustered(65, 1)
    t = lambda a: torch.from_numpy(a).cuda()
    picked = torch.full((1, 65), -1, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    out = torch.full((65,), -1.0, dtype=torch.float32, device="cuda")
    args = dict(boxes=t(b), scores=t(s), seg_off=t(np.asarray([0, 65], np.int32)), B=1, max_n=65, method=0, thr=0.5, sigma=0.5,
                min_score=0.001, picked=picked, cnt=cnt, out=out)
    inf, nan = float("inf"), float("nan")
    for change in (dict(max_n=2049), dict(method=2), dict(method=-1), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=inf),
                   dict(sigma=nan), dict(min_score=0.0), dict(min_score=1.5), dict(min_score=nan), dict(min_score=-0.1),
                   dict(thr=0.0), dict(thr=1.5), dict(thr=nan), dict(B=-1), dict(max_n=-1), dict(boxes=None), dict(scores=None),
                   dict(seg_off=None), dict(picked=None), dict(cnt=None), dict(out=None)):
        assert _raw(H, **dict(args, **change)) == EINVAL, change
    torch.cuda.synchronize()
    assert (picked.cpu().numpy() == -1).all() and cnt.cpu().tolist() == [-1] and (out.cpu().numpy() == -1.0).all()
    # B == 0 is a no-op; an empty segment writes its count; min_score and nms_thresh of exactly 1 are inside
    assert _raw(H, **dict(args, B=0)) == 0 and cnt.cpu().tolist() == [-1]
    assert _raw(H, **dict(args, seg_off=t(np.asarray([0, 0], np.int32)))) == 0 and cnt.cpu().tolist() == [0]
    cnt.fill_(-1)
    assert _raw(H, **dict(args, max_n=0, boxes=None, scores=None, picked=None, out=None)) == 0 and cnt.cpu().tolist() == [0]
    cnt.fill_(-1)
    assert _raw(H, **dict(args, min_score=1.0, thr=1.0)) == 0 and cnt.cpu().tolist() == [0]       # (every score is below 1)
    assert _raw(H, **args) == 0 and int(cnt.item()) == len(F.soft_nms(b, s, "linear", 0.5, 0.5, 0.001)[0])
    # mmt_det_postprocess_soft: the same refusals before its first launch, and those of mmt_det_postprocess
    prob, dec, per = _det_inputs(65, 3, seed=5)
    for method, sigma, min_score, nms in ((2, 0.5, 0.001, 0.5), (0, 0.0, 0.001, 0.5), (0, inf, 0.001, 0.5), (0, 0.5, 0.0, 0.5),
                                          (0, 0.5, 1.5, 0.5), (1, 0.5, 0.001, 0.0), (1, 0.5, 0.001, 1.5)):
        ob, os_, ol, oc, rc = _raw_det(H, prob, dec, per, 3, 0.05, nms, 100, method, sigma, min_score)
        assert rc == EINVAL, (method, sigma, min_score, nms)
        assert (ob == -1).all() and (os_ == -1).all() and (ol == -1).all() and (oc == -1).all()
    big = np.zeros((2049, 3), np.float32)
    assert _raw_det(H, big, np.zeros((2049, 12), np.float32), [2049], 3, 0.05, 0.5, 100, 0, 0.5, 0.001)[4] == EINVAL
    # the wrappers raise before any launch, and keep det_postprocess's None for what is out of range
    p, d = torch.from_numpy(prob).cuda(), torch.from_numpy(dec).cuda()
    for bad in (dict(method="quadratic"), dict(sigma=0.0), dict(sigma=inf), dict(min_score=0.0), dict(min_score=2.0)):
        with pytest.raises(ValueError):
            H.det_postprocess_soft(p, d, per, 0.05, 0.5, 100, **bad)
        with pytest.raises(ValueError):
            H.soft_nms_batched(t(b), t(s), args["seg_off"], 65, **dict(dict(method="linear"), **bad))
    with pytest.raises(ValueError):
        H.det_postprocess_soft(p, d, per, 0.05, 0.0, 100)
    assert H.det_postprocess_soft(torch.from_numpy(big).cuda(), torch.zeros((2049, 12)).cuda(), [2049], 0.05, 0.5, 100) is None


def test_deterministic_mode_same_bytes(H):
    segs = [F.clustered(n, n) for n in (257, 513)]
    was = H.get_deterministic()
    got = []
    try:
        for mode in (True, True, False, False):
            H.set_deterministic(mode)
            got.append(_run_raw(H, segs, 1, 513))
    finally:
        H.set_deterministic(was)
    for g in got[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g, got[0]))
