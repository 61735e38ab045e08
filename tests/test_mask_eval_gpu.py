"""The PAP evaluator's mask work on the device (csrc/maskeval.hip behind data/datasets/evaluation/pap/mask_rle.py: pack, expand
from runs, transitions, pair intersections) against the host codec it replaces: the same run-length strings byte for byte,
the same integer areas / intersections / unions, hence statistics equal with `==`; and against the reference's own outputs
in tests/golden/pap_eval.json.  The shapes are the smallest that reach each edge of the kernels (tests/mask_cases.py)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLD
import mask_cases
import pap_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mu():
    from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle
    return mask_rle


@pytest.fixture(scope="module")
def H():
    from maskrcnn_benchmark import _hip
    _hip.lib()
    return _hip


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(os.path.join(GOLD, "pap_eval.json")))


@pytest.fixture(scope="module")
def data(mu):
    """the windows of pap_inputs.make(7), encoded by the HOST codec"""
    gts, dts = pap_inputs.make(7)
    for lst in (gts, dts):
        for x in lst:
            r = mu.encode(x["mask"])
            x["segmentation"] = {"size": r["size"], "counts": r["counts"].decode("ascii")}
    return gts, dts


def _key(x):
    return x["image_id"]["file_name"] + "_%d_%d" % tuple(x["image_id"]["location"])


def _strip(lst):
    return [{k: v for k, v in x.items() if k != "mask"} for x in lst]


def _sizes():
    return mask_cases.SIZES + [mask_cases.TALL]


def _same(a, b):
    """== through dicts, lists and arrays (NaN equal to NaN: 0 / 0 statistics of a window without detections)"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and not isinstance(b, np.ndarray):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, (np.ndarray, float, np.floating)) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f" and b.dtype.kind == "f")
    return a == b


# ---------------------------------------------------------------------------------------------------------------- 1. codec
@pytest.mark.parametrize("h,w", _sizes())
def test_encode_device_equals_encode(mu, h, w):
    cases = mask_cases.masks_of(h, w)
    stack = torch.from_numpy(np.stack([m for _, m in cases])).cuda()
    own = mu.encode_device(stack)
    assert len(own) == len(cases)
    for (name, m), r in zip(cases, own):
        ref = mu.encode(m)
        assert r["size"] == ref["size"] and r["counts"] == ref["counts"], (h, w, name)
    # the (n, 1, H, W) form of the pasted stack, and values other than 1 count as set
    again = mu.encode_device((stack * 7)[:, None])
    assert [r["counts"] for r in again] == [r["counts"] for r in own]
    assert mu.encode_device(stack[:0]) == []


def test_encode_device_on_the_fixture_windows(mu, H, fixture):
    gts, dts = pap_inputs.make(7)
    allm = gts + dts
    assert len(allm) == 165
    stack = torch.from_numpy(np.stack([x["mask"] for x in allm])).cuda()
    assert [r["counts"].decode("ascii") for r in mu.encode_device(stack)] == fixture["rle_counts"]
    _, rec = H.mask_pack(stack)
    assert rec[:, 0].cpu().tolist() == fixture["areas"]


# ---------------------------------------------------------------------------------------------------------------- 2. expand
def _record_of(mu, m):
    x, y, bw, bh = mu._bbox(m)
    return int(mu.area(mu.encode(m))), (x, y, bw, bh)


@pytest.mark.parametrize("h,w", _sizes())
def test_expand_then_transitions_is_the_identity(mu, H, h, w):
    cases = mask_cases.masks_of(h, w)
    rles = [mu.encode(m) for _, m in cases]
    dev = torch.device("cuda", torch.cuda.current_device())
    words, rec = mu._expand_device(H, rles, dev)
    counts, pos = H.mask_transitions(words, h, w)
    pos, at = pos.numpy(), 0
    for (name, m), r, c, rc in zip(cases, rles, counts.tolist(), rec):
        assert mu._runs_of_positions(pos[at:at + c], h * w) == mu.counts_of(r), (h, w, name)
        at += c
        area, box = _record_of(mu, m)
        assert int(rc[0]) == area and tuple(float(v) for v in mu._box_of_record(rc, h)) == box, (h, w, name)
        assert list(rc[6:]) == [0, 0]
    # pack gives the same words and the same records
    pw, prec = H.mask_pack(torch.from_numpy(np.stack([m for _, m in cases])).cuda())
    assert torch.equal(pw, words) and np.array_equal(prec.cpu().numpy(), rec)


def test_expand_takes_the_uncompressed_list_form(mu, H):
    rl = {"size": [4, 3], "counts": [2, 3, 7]}
    words, rec = mu._expand_device(H, [rl], torch.device("cuda", torch.cuda.current_device()))
    counts, pos = H.mask_transitions(words, 4, 3)
    assert mu._runs_of_positions(pos.numpy(), 12) == [2, 3, 7]
    m = mu.decode(rl)
    assert int(rec[0][0]) == 3 and tuple(float(v) for v in mu._box_of_record(rec[0], 4)) == mu._bbox(m)
    with pytest.raises(ValueError):
        mu._expand_device(H, [{"size": [4, 3], "counts": [2, 3, 6]}], torch.device("cuda", torch.cuda.current_device()))


# ---------------------------------------------------------------------------------------------------------------- 3. pairs
def _both(mu, d, g, crowd):
    host = mu.iouIntUni(d, g, crowd)
    dev = mu.iouIntUni(d, g, crowd, on_device=True)
    for a, b in zip(host, dev):
        assert b.dtype == np.float64 and np.array_equal(a, b)
    return dev


def test_pairs_on_the_disjoint_box_masks_twice(mu):
    a = np.zeros((40, 40), np.uint8); a[2:8, 3:9] = 1
    b = np.zeros((40, 40), np.uint8); b[20:30, 22:31] = 1
    c = np.zeros((40, 40), np.uint8); c[33:39, 1:5] = 1
    o = np.zeros((40, 40), np.uint8); o[5:25, 5:25] = 1
    e = np.zeros((40, 40), np.uint8)
    R = [mu.encode(np.asfortranarray(m)) for m in (a, b, c, o, e)]
    for _ in range(2):
        iou, inter, uni = _both(mu, R, R[:4], [0, 0, 0, 0])
        disjoint = np.array([[0, 1, 1, 0], [1, 0, 1, 0], [1, 1, 0, 1], [0, 0, 1, 0], [1, 1, 1, 1]], bool)
        assert (iou[disjoint] == 0).all() and (inter[disjoint] == 0).all() and (uni[disjoint] == 0).all()
        assert inter[3, 0] == 12 and uni[3, 0] == 36 + 400 - 12 and inter[1, 3] == 15


def test_pairs_edge_cases(mu):
    a = np.zeros((40, 40), np.uint8); a[4:10, 3:9] = 1           # columns 3..8
    t = np.zeros((40, 40), np.uint8); t[4:10, 9:15] = 1          # columns 9..14: the boxes touch, w == 0
    o = np.zeros((40, 40), np.uint8); o[5:25, 5:25] = 1
    e = np.zeros((40, 40), np.uint8)
    z = np.zeros((40, 40), np.uint8); z[0:3, 0:3] = 1; z[30:33, 30:33] = 1   # boxes overlap o's, no common pixel with a: i == 0 -> u = 1
    A, T, O, E, Z = (mu.encode(m) for m in (a, t, o, e, z))
    iou, inter, uni = _both(mu, [A], [T], [0])
    assert iou[0, 0] == 0 and inter[0, 0] == 0 and uni[0, 0] == 0
    _both(mu, [E, A], [A, E], [0, 0])                             # an empty mask on either side
    iou, inter, uni = _both(mu, [Z], [A, O], [0, 0])
    assert inter[0, 0] == 0 and uni[0, 0] == 1
    iou, inter, uni = _both(mu, [A, O, Z], [O, A], [1, 0])        # a crowd ground truth: u = |d|
    assert uni[0, 0] == 36 and uni[0, 1] == 36 and uni[1, 1] == 36 + 400 - 20
    _both(mu, [A, O], [O, A], None)
    # unequal sizes: -1 where the boxes overlap
    s = np.zeros((30, 50), np.uint8); s[5:25, 5:25] = 1
    S = mu.encode(s)
    iou, inter, uni = _both(mu, [A, S, E], [O, S, T], [0, 0, 0])
    assert iou[1, 0] == -1 and iou[0, 1] == -1 and iou[1, 1] == 1.0 and inter[1, 0] == 0 and uni[1, 0] == 0
    # the wrap masks (full-height box by the run-based rule) and a word-aligned height
    for h, w in ((64, 3), (37, 53), (130, 67)):
        R = [mu.encode(m) for _, m in mask_cases.masks_of(h, w)]
        _both(mu, R, R, [0] * len(R))
    assert mu.iouIntUni([], [A], [], on_device=True) == [] and mu.iouIntUni([A], [], [], on_device=True) == []


def test_pairs_on_every_fixture_window(mu, fixture, data):
    gts, dts = data
    for k in sorted({_key(x) for x in gts + dts}):
        for cat in (1, 2):
            g = [x["segmentation"] for x in gts if _key(x) == k and x["category_id"] == cat]
            d = [x["segmentation"] for x in dts if _key(x) == k and x["category_id"] == cat]
            if g and d:
                _both(mu, d, g, [0] * len(g))
    img, cat = fixture["window"]["key"]
    g = [x for x in gts if _key(x) == img and x["category_id"] == cat]
    d = sorted([x for x in dts if _key(x) == img and x["category_id"] == cat], key=lambda q: -q["score"])
    iou, inter, uni = mu.iouIntUni([x["segmentation"] for x in d], [x["segmentation"] for x in g], [0] * len(g), on_device=True)
    np.testing.assert_allclose(iou, np.array(fixture["window"]["iou"]), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(np.where(iou > 0, inter, 0), np.array(fixture["window"]["inter"]))
    np.testing.assert_array_equal(np.where(iou > 0, uni, 0), np.array(fixture["window"]["union"]))


# ---------------------------------------------------------------------------------------------------------------- 4. evaluator
def test_evaluator_on_device_equals_host_and_reference(fixture, data):
    from maskrcnn_benchmark.data.datasets.evaluation.pap.pap_eval import evaluate_predictions_on_pap
    gts, dts = data
    host = evaluate_predictions_on_pap(_strip(gts), _strip(dts), None, "segm")
    ev = evaluate_predictions_on_pap(_strip(gts), _strip(dts), None, "segm", on_device=True)
    assert ev.on_device and not host.on_device
    assert _same(ev.evalImgs, host.evalImgs)
    assert _same(ev.stats, host.stats)
    assert _same(ev.eval["precision"], host.eval["precision"]) and _same(ev.eval["recall"], host.eval["recall"])
    # and the reference's own evaluator, at the tolerances of tests/test_pap_eval.py
    assert len(ev.evalImgs) == len(fixture["per_window"])
    for own, ref in zip(ev.evalImgs, fixture["per_window"]):
        assert (own is None) == (ref is None)
        if ref is None:
            continue
        assert own["image_id"] == ref["image_id"] and own["category_id"] == ref["category_id"]
        assert float(own["AJI"][0, 0]) == pytest.approx(ref["AJI"], rel=1e-12, abs=1e-15)
        assert float(own["F1"]) == pytest.approx(ref["F1"], rel=1e-12)
        assert float(own["FNRo"]) == ref["FNRo"] and float(own["FDR"]) == ref["FDR"]
        np.testing.assert_allclose(np.asarray(own["DSC"], float), np.asarray(ref["DSC"], float), rtol=1e-12, atol=0)
        np.testing.assert_allclose(np.asarray(own["TPRp"], float), np.asarray(ref["TPRp"], float), rtol=1e-12, atol=0)
    assert float(ev.eval["precision"].sum()) == pytest.approx(fixture["precision_sum"], rel=1e-12)
    np.testing.assert_allclose(ev.eval["recall"], np.array(fixture["recall"]), rtol=1e-12)
    for m, per in fixture["stats"].items():
        for k, v in per.items():
            own = float(np.asarray(ev.stats[m][k if k == "all" else int(k)]).reshape(-1)[0])
            assert own == pytest.approx(v, rel=1e-12, abs=1e-15), (m, k, own, v)


# ---------------------------------------------------------------------------------------------------------------- 5. plumbing
def _dataset_and_predictions(data, masks_of):
    """the dataset stub of tests/test_pap_eval.py::test_dataset_to_evaluator_plumbing; masks_of(detections, BoxList) fills the
    `mask` field (and may set the boxes)"""
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    gts, dts = data
    ids = {}
    for x in gts + dts:
        ids.setdefault(_key(x), x["image_id"])
    order = sorted(ids)

    class DS(object):
        maxWS = pap_inputs.SIZE
        id_to_img_map = {i: ids[k] for i, k in enumerate(order)}
        contiguous_category_id_to_json_id = {1: 1, 2: 2}

        def get_ground_truth(self, original_id):
            g = [x for x in gts if x["image_id"] is original_id or x["image_id"] == original_id]
            b = BoxList(torch.zeros((len(g), 4)), (self.maxWS, self.maxWS), "xyxy")
            b.add_field("labels", torch.tensor([x["category_id"] for x in g], dtype=torch.int64))
            b.add_field("masks", [x["segmentation"] for x in g])
            return b

    preds = {}
    for i, k in enumerate(order):
        d = [x for x in dts if _key(x) == k]
        b = masks_of(d)
        b.add_field("scores", torch.tensor([x["score"] for x in d], dtype=torch.float64))
        b.add_field("labels", torch.tensor([x["category_id"] for x in d], dtype=torch.int64))
        preds[i] = b
    return DS(), preds


def _evaluate_both_ways(ds, preds):
    from maskrcnn_benchmark.data.datasets.evaluation import evaluate
    res_h, pap_h = evaluate(ds, preds, None, iou_types=("segm",), box_only=False)
    res_d, pap_d = evaluate(ds, preds, None, iou_types=("segm",), box_only=False, on_device=True)
    assert len(pap_d) == len(pap_h) > 0
    for a, b in zip(pap_d, pap_h):
        assert isinstance(a["segmentation"]["counts"], str) and a == b
    assert _same(dict(res_d.results["segm"]), dict(res_h.results["segm"]))
    return pap_d


def test_plumbing_with_window_sized_masks_on_the_gpu(data):
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    S = pap_inputs.SIZE

    def masks_of(d):
        b = BoxList(torch.zeros((len(d), 4)), (S, S), "xyxy")
        b.add_field("mask", torch.from_numpy(np.stack([x["mask"] for x in d])[:, None]).cuda() if d
                    else torch.zeros((0, 1, S, S), dtype=torch.uint8).cuda())
        return b

    ds, preds = _dataset_and_predictions(data, masks_of)
    pap = _evaluate_both_ways(ds, preds)
    assert sorted(p["segmentation"]["counts"] for p in pap) == sorted(x["segmentation"]["counts"] for x in data[1])


def test_plumbing_with_probabilities_that_need_pasting(data):
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    S = pap_inputs.SIZE
    rng = np.random.RandomState(5)

    def masks_of(d):
        boxes = []
        for x in d:
            ys, xs = np.nonzero(x["mask"])
            boxes.append([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1] if ys.size else [0, 0, 4, 4])
        b = BoxList(torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4), (S, S), "xyxy")
        b.add_field("mask", torch.from_numpy(rng.rand(len(d), 1, 28, 28).astype(np.float32)))
        return b

    ds, preds = _dataset_and_predictions(data, masks_of)
    _evaluate_both_ways(ds, preds)


# ---------------------------------------------------------------------------------------------------------------- 6. error codes
def test_entry_points_refuse_bad_arguments(H):
    """argument checks of the library: nothing is launched, the pointers are never followed"""
    L = H._lib_raw()
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.addressof(buf)
    EINVAL = -22
    big = (65536, 32768)                                          # H * W == 2^31
    calls = {
        "mmt_mask_pack": lambda n, h, w, a=p: L.mmt_mask_pack(a, n, h, w, a, a, None),
        "mmt_mask_expand": lambda n, h, w, a=p: L.mmt_mask_expand(a, a, n, h, w, a, a, None),
        "mmt_mask_transition_counts": lambda n, h, w, a=p: L.mmt_mask_transition_counts(a, n, h, w, a, None),
        "mmt_mask_transition_positions": lambda n, h, w, a=p: L.mmt_mask_transition_positions(a, n, h, w, a, a, None),
        "mmt_mask_pair_intersections": lambda n, h, w, a=p: L.mmt_mask_pair_intersections(a, a, n, a, a, n, h, w, a, None),
    }
    for name, f in calls.items():
        assert f(1, *big) == EINVAL, name
        assert f(1, 46341, 46341) == EINVAL, name                 # the first square at or above 2^31
        assert f(-1, 8, 8) == EINVAL, name
        assert f(1, 0, 8) == EINVAL and f(1, 8, -1) == EINVAL, name
        assert f(1, 8, 8, None) == EINVAL, name                   # null pointers where arrays are needed
        assert f(0, 8, 8, None) == 0, name                        # a count of zero is a no-op
    assert L.mmt_mask_pair_intersections(p, p, 0, p, p, 3, 8, 8, p, None) == 0
    assert L.mmt_mask_pair_intersections(p, p, 3, p, p, -1, 8, 8, p, None) == EINVAL
