"""Paste straight into mask words (csrc/masks.hip: paste_words_kernel, `mmt_paste_mask_words`) and what is built on it, bit for
bit against the route it replaces -- `mmt_paste_mask_stack` into a zeroed byte stack, then `mmt_mask_pack` -- which
tests/test_mask_geometry_gpu.py holds against the oracle and tests/test_mask_eval_gpu.py against pycocotools strings.  Nothing
here has a tolerance: words, records, strings and stacks are compared with equality."""
import numpy as np
import pytest
import torch

import mask_geometry_inputs as mg
import pap_inputs

pytestmark = pytest.mark.gpu

EINVAL = -22
# (IH, IW): H a multiple of 64; words that straddle two columns (twice); H < 64, a word spans many columns (twice); above the
# height (4096) at which mmt_mask_pack changes kernel.  The boxes were drawn for the first: on the others many fall partly or
# wholly outside.
CANVASES = [mg.CANVAS, (127, 150), (65, 33), (30, 200), (1, 1), (4100, 5)]


@pytest.fixture(scope="module")
def hip():
    from maskrcnn_benchmark import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return _hip


@pytest.fixture(scope="module")
def inputs():
    """{M: (prob (D, M, M), boxes (D, 4), rows drawn to reach the first canvas)} on the device: the paste cases, then full
    probabilities in boxes that lie wholly outside it"""
    out = {}
    for M, (prob, boxes) in mg.paste_cases().items():
        ob = mg.outside_boxes()
        p = np.concatenate([prob, np.ones((len(ob), M, M), np.float32)])
        out[M] = (torch.from_numpy(p).cuda(), torch.from_numpy(np.concatenate([boxes, ob]).astype(np.float32)).cuda(), len(boxes))
    return out


def words_through_the_abi(hip, prob, boxes, ih, iw, thresh):
    """mmt_paste_mask_words into buffers whose every byte is 0xFF beforehand"""
    D, M = prob.shape[0], prob.shape[-1]
    words, rec = hip._mask_buffers(D, ih, iw, prob.device)
    words.view(torch.uint8).fill_(0xFF)
    rec.view(torch.uint8).fill_(0xFF)
    torch.cuda.synchronize()
    code = hip._lib_raw().mmt_paste_mask_words(prob.data_ptr(), boxes.data_ptr(), D, M, ih, iw, thresh, words.data_ptr(),
                                               rec.data_ptr(), None)
    torch.cuda.synchronize()
    assert code == 0
    return words, rec


# ------------------------------------------------------------------------------------------ 1. the two-launch route
@pytest.mark.parametrize("canvas", CANVASES, ids=lambda c: "%dx%d" % c)
@pytest.mark.parametrize("M", mg.PASTE_M)
def test_words_and_records_equal_stack_then_pack(hip, inputs, M, canvas):
    ih, iw = canvas
    prob, boxes, drawn = inputs[M]
    stack = hip.paste_mask_stack(prob, boxes, ih, iw, mg.PASTE_THRESH)
    want_w, want_r = hip.mask_pack(stack[:, 0])
    filled = (stack.reshape(len(stack), -1).sum(1) > 0).float()
    print("M=%d %dx%d: %d of %d masks non-empty, %d pixels set" % (M, ih, iw, int(filled.sum()), len(filled), int(stack.sum())))
    if canvas == mg.CANVAS:   # not empty against empty (tests/test_paste_words_host.py: the oracle says the same of these inputs)
        assert filled[:drawn].mean().item() > 0.8 and int(filled[drawn:].sum()) == 0
    got_w, got_r = words_through_the_abi(hip, prob, boxes, ih, iw, mg.PASTE_THRESH)
    assert got_w.shape == want_w.shape == (len(boxes), (ih * iw + 63) // 64)
    assert torch.equal(got_w, want_w)
    assert torch.equal(got_r, want_r)
    # the binding, which takes (D, 1, M, M) as well
    w2, r2 = hip.paste_mask_words(prob[:, None], boxes, ih, iw, mg.PASTE_THRESH)
    assert torch.equal(w2, want_w) and torch.equal(r2, want_r)


def test_binding_refuses_host_tensors(hip):
    with pytest.raises(RuntimeError):
        hip.paste_mask_words(torch.ones(1, 7, 7), torch.zeros(1, 4).cuda(), 8, 8, 0.5)
    with pytest.raises(RuntimeError):
        hip.paste_mask_words(torch.ones(1, 7, 7).cuda(), torch.zeros(1, 4), 8, 8, 0.5)


# ------------------------------------------------------------------------------------------ 2. strings
def test_strings_equal_encode_device_of_the_stack(hip, inputs):
    from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle
    ih, iw = 127, 150
    for M in mg.PASTE_M:
        prob, boxes, _ = inputs[M]
        want = mask_rle.encode_device(hip.paste_mask_stack(prob, boxes, ih, iw, mg.PASTE_THRESH))
        got = mask_rle.encode_pasted_device(prob, boxes, ih, iw, mg.PASTE_THRESH)
        assert len(want) == len(boxes) and got == want
        assert len({r["counts"] for r in got}) > len(got) // 2          # (not one string many times)
        assert mask_rle.encode_pasted_device(prob[:, None], boxes, ih, iw) == want   # the threshold's default is the cases' 0.5
    assert mask_rle.encode_pasted_device(torch.zeros((0, 1, 28, 28)).cuda(), torch.zeros((0, 4)).cuda(), ih, iw) == []


def test_masker_rle_single_image(hip, inputs):
    from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.mask_head import Masker
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    prob, boxes, _ = inputs[28]
    m = Masker(threshold=0.5, padding=1)
    bl = BoxList(boxes, (150, 127), "xyxy")
    assert m.rle_single_image(prob[:, None], bl) == mask_rle.encode_device(m.forward_single_image(prob[:, None], bl))
    assert m.rle_single_image(prob[:0, None], BoxList(boxes[:0], (150, 127), "xyxy")) == []


# ------------------------------------------------------------------------------------------ 3. refused arguments
def test_entry_point_refuses_bad_arguments_and_writes_nothing(hip):
    L = hip._lib_raw()
    M = 7
    prob, boxes = torch.ones(2, M, M).cuda(), torch.tensor([[1.0, 1.0, 6.0, 6.0]] * 2).cuda()
    words, rec = hip._mask_buffers(2, 8, 8, prob.device)
    words.view(torch.uint8).fill_(0xFF)
    rec.view(torch.uint8).fill_(0xFF)
    torch.cuda.synchronize()
    p, b, w, r = prob.data_ptr(), boxes.data_ptr(), words.data_ptr(), rec.data_ptr()

    def call(prob=p, boxes=b, D=2, M=M, IH=8, IW=8, words=w, rec=r):
        return L.mmt_paste_mask_words(prob, boxes, D, M, IH, IW, 0.5, words, rec, None)

    refused = {
        "null prob": dict(prob=None), "null boxes": dict(boxes=None), "null words": dict(words=None), "null rec": dict(rec=None),
        "M == 0": dict(M=0), "M < 0": dict(M=-3),
        "(M+2)^2 * 4 > 64 KiB": dict(M=127),                       # 129^2 * 4 = 66564
        "IH == 0": dict(IH=0), "IH < 0": dict(IH=-8), "IW == 0": dict(IW=0), "IW < 0": dict(IW=-8),
        "IH * IW == 2^31": dict(IH=65536, IW=32768), "IH * IW >= 2^31": dict(IH=46341, IW=46341),
        "D < 0": dict(D=-1), "D > 65535": dict(D=65536),
    }
    for name, kw in refused.items():
        assert call(**kw) == EINVAL, name
    assert call(D=0) == 0
    assert call(D=0, prob=None, boxes=None, words=None, rec=None) == 0
    torch.cuda.synchronize()
    assert bool((words.view(torch.uint8) == 0xFF).all()) and bool((rec.view(torch.uint8) == 0xFF).all())
    # and the largest M it takes does run: (126 + 2)^2 * 4 = 64 KiB exactly
    M = 126
    big = torch.ones(2, M, M).cuda()
    assert call(prob=big.data_ptr(), M=M) == 0
    torch.cuda.synchronize()
    want_w, want_r = hip.mask_pack(hip.paste_mask_stack(big, boxes, 8, 8, 0.5)[:, 0])
    assert torch.equal(words, want_w) and torch.equal(rec, want_r) and int(rec[0, 0]) > 0


# ------------------------------------------------------------------------------------------ 4. POSTPROCESS_MASKS
def test_postprocess_masks_returns_the_pasted_stack(hip, synth, weights):
    from maskrcnn_benchmark.config import make_default_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    from maskrcnn_benchmark.structures.image_list import to_image_list
    SIZE = 160
    imgs, _ = synth.make_labeled(2, SIZE, 4, seed=1234)
    unl = synth.make_unlabeled(2, SIZE, 3, seed=4321)
    outs, teach = [], []
    for flag in (False, True):
        cfg = make_default_cfg()
        cfg.MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS = flag
        torch.manual_seed(0)
        model = build_detection_model(cfg, is_teacher=True).cuda()
        model.load_state_dict(weights, strict=False)
        model.eval()
        with torch.no_grad():
            outs.append(model(to_image_list(list(imgs.cuda()), 32)))
            g = torch.Generator(device="cuda")
            g.manual_seed(5)
            model.set_rng(g)
            teach.append(model.forward_teacher([to_image_list(list(u.cuda()), 32) for u in unl[:2]]))
        thr = cfg.MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS_THRESHOLD
    plain, pasted = outs
    assert len(plain) == len(pasted) == 2
    n_set = 0
    for a, b in zip(plain, pasted):
        assert len(a) == len(b) > 0 and b.size == (SIZE, SIZE)
        assert torch.equal(a.bbox, b.bbox)
        assert torch.equal(a.get_field("scores"), b.get_field("scores")) and torch.equal(a.get_field("labels"), b.get_field("labels"))
        m, prob = b.get_field("mask"), a.get_field("mask")
        assert tuple(prob.shape) == (len(a), 1, 28, 28) and prob.dtype == torch.float32      # the default is untouched
        assert m.dtype == torch.uint8 and tuple(m.shape) == (len(b), 1, SIZE, SIZE)
        assert torch.equal(m, hip.paste_mask_stack(prob, a.bbox, SIZE, SIZE, thr))
        n_set += int(m.sum())
    assert n_set > 0
    # the teacher's pseudo-mask is the mask generator's and stays integral
    ta, tb = teach
    assert len(ta["seg_mask"]) == len(tb["seg_mask"]) == 2
    for x, y in zip(ta["seg_mask"], tb["seg_mask"]):
        assert y.dtype == torch.int32 and tuple(y.shape) == (SIZE, SIZE) and torch.equal(x, y)
    assert sum(int(y.sum()) for y in tb["seg_mask"]) > 0


# ------------------------------------------------------------------------------------------ 5. evaluator
def test_evaluator_on_device_strings_equal_the_stack_route(hip):
    """28 x 28 probabilities cut out of the dense detections of tests/pap_inputs.py (their boxes: the masks' extents), through
    prepare_for_pap_segmentation(on_device=True), against the route it took before: paste into bytes, then encode_device"""
    from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle
    from maskrcnn_benchmark.data.datasets.evaluation.pap.pap_eval import prepare_for_pap_segmentation
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.mask_head import Masker
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    S = pap_inputs.SIZE
    gts, dts = pap_inputs.make()
    ids = {}
    for x in gts + dts:
        ids.setdefault(x["image_id"]["id"], x["image_id"])
    order = sorted(ids)

    class DS(object):
        maxWS = S
        id_to_img_map = {i: ids[k] for i, k in enumerate(order)}
        contiguous_category_id_to_json_id = {1: 1, 2: 2}

        def get_ground_truth(self, original_id):
            g = [x for x in gts if x["image_id"] == original_id]
            b = BoxList(torch.zeros((len(g), 4)), (S, S), "xyxy")
            b.add_field("labels", torch.tensor([x["category_id"] for x in g], dtype=torch.int64))
            rles = [mask_rle.encode(np.asfortranarray(x["mask"])) for x in g]
            for r in rles:
                r["counts"] = r["counts"].decode("utf-8")
            b.add_field("masks", rles)
            return b

    preds = {}
    for i, k in enumerate(order):
        d = [x for x in dts if x["image_id"]["id"] == k]
        boxes, probs = [], []
        for x in d:
            ys, xs = np.nonzero(x["mask"])
            x0, y0, x1, y1 = int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1
            crop = torch.from_numpy(x["mask"][y0:y1, x0:x1].astype(np.float32))[None, None]
            probs.append(torch.nn.functional.interpolate(crop, size=(28, 28), mode="bilinear", align_corners=False)[0])
            boxes.append([x0, y0, x1, y1])
        b = BoxList(torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4), (S, S), "xyxy")
        b.add_field("mask", torch.stack(probs) if probs else torch.zeros((0, 1, 28, 28)))
        b.add_field("scores", torch.tensor([x["score"] for x in d], dtype=torch.float64))
        b.add_field("labels", torch.tensor([x["category_id"] for x in d], dtype=torch.int64))
        preds[i] = b
    _, got = prepare_for_pap_segmentation(preds, DS(), on_device=True)
    masker = Masker(threshold=0.5, padding=1)
    want = []
    for i in sorted(preds):
        if len(preds[i]):
            p = preds[i].resize((S, S))
            want += mask_rle.encode_device(masker.forward_single_image(p.get_field("mask").cuda(), p.to(torch.device("cuda"))))
    assert len(got) == len(want) == len(dts) > 40
    for a, b in zip(got, want):
        assert isinstance(a["segmentation"]["counts"], str)
        assert a["segmentation"]["counts"] == b["counts"].decode("utf-8") and list(a["segmentation"]["size"]) == [S, S]
    assert len({a["segmentation"]["counts"] for a in got}) > len(got) // 2
    areas = [mask_rle.area(dict(a["segmentation"], counts=a["segmentation"]["counts"].encode("ascii"))) for a in got]
    assert sum(a > 0 for a in areas) > 0.8 * len(areas)            # the pasted detections have pixels
