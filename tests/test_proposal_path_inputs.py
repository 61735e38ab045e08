"""tests/proposal_path_inputs.py on the CPU: every builder reaches the edge it names (asserted on the constructed inputs, so a
later edit cannot turn an edge case into an ordinary one), and the plain references agree with what the project already
trusts -- the CPU oracle's ROIAlign within the derived rounding bounds, the fp32 tensor modules (Matcher, BoxCoder,
box_iou_tensor, LevelMapper) with equal integers, torch's float64 autograd for the two losses."""
import math

import numpy as np
import pytest
import torch

import proposal_path_inputs as pp

f32 = np.float32


# ================================================================================================================ ROIAlign
def _named(PH, PW, sr):
    names, rois, levels = pp.roi_list(PH, PW, sr)
    out = {}
    for n, r, l in zip(names, rois, levels):
        H, W, s = pp.ROI_LEVELS[l]
        out[n] = (r, int(l), pp.roi_samples(r, s, PH, PW, sr, H, W))
    return names, rois, levels, out


@pytest.mark.parametrize("sr", pp.ROI_SRS)
@pytest.mark.parametrize("PH,PW", pp.ROI_POOLS)
def test_roi_list_reaches_its_edges(PH, PW, sr):
    names, rois, levels, d = _named(PH, PW, sr)
    assert 28 <= len(names) <= 48 and len(set(names)) == len(names)
    bases = sorted({n.split("/")[0] for n in names if not n.startswith("inside_again")})
    for b in bases:   # every named ROI on image 0 and on image 1, and the levels mixed
        imgs = sorted(int(d[n][0][0]) for n in names if n.split("/")[0] == b)
        assert imgs == [0, 1], b
    assert set(levels.tolist()) == {0, 1}
    assert (levels[rois[:, 0] == 0] == 1).any() and (levels[rois[:, 0] == 1] == 0).any()
    for n, (r, l, (ys, ye, xs, xe)) in d.items():
        H, W, s = pp.ROI_LEVELS[l]
        rsw, rsh, rw, rh = pp.roi_extent(r, s)
        base = n.split("/")[0]
        if base == "inside":
            assert not ye.any() and not xe.any() and ys.min() > 0 and ys.max() < H - 1 and xs.min() > 0 and xs.max() < W - 1
        elif base == "zero_size":
            assert r[3] == r[1] and r[4] == r[2] and rw == 1 and rh == 1
        elif base == "inverted":
            assert r[3] < r[1] and rw == 1
        elif base == "sub_pixel":
            assert 0 < (r[3] - r[1]) * s < 1 and 0 < (r[4] - r[2]) * s < 1
        elif base == "left_of_map":
            assert xe.all() and not ye.any()
        elif base == "above_map":
            assert ye.all() and not xe.any()
        elif base == "beyond_far_corner":
            assert ye.all() and xe.all() and ys.min() > H and xs.min() > W
        elif base == "straddles_top_left":
            assert rsh < -1 and rsh + rh > 1 and rsw < -1 and rsw + rw > 1      # from the empty zone over the clamped one into the map
        elif base == "last_row_and_column":
            assert not ye.any() and not xe.any() and ys.min() > H - 1 and xs.min() > W - 1
        elif base == "tile_seam" and l == 0:
            assert math.floor(rsh) == 7 and math.floor(rsw) == 7     # the last row / column of tile 0; the map goes on to 8 / 10
        elif base == "ends_before_seam" and l == 0:
            assert math.floor(rsh + rh) == 7 and math.floor(rsw + rw) == 7
        elif base == "wide_400":
            assert r[3] - r[1] == 400 and rsw < 0 and rsw + rw > W and rsh < 0 and rsh + rh > H
        elif base == "y_at_minus_1":
            assert ys[0] == f32(-1.0) and not ye[0]
        elif base == "x_at_minus_1":
            assert xs[0] == f32(-1.0) and not xe[0]
        elif base == "y_at_H":
            assert ys[-1] == f32(H) and not ye[-1]
        elif base == "x_at_W":
            assert xs[-1] == f32(W) and not xe[-1]
        elif base.endswith("_beyond"):
            on = d[n.replace("_beyond", "")]
            j = 2 if base[0] == "y" else 1
            assert (np.delete(on[0], j) == np.delete(r, j)).all() and on[0][j] != r[j]     # one coordinate moved
            c, e = (ys, ye) if base[0] == "y" else (xs, xe)
            if "minus_1" in base:
                assert e[0] and c[0] < f32(-1.0) and c[0] >= np.nextafter(f32(-1.0), f32(-np.inf)) - f32(2e-7)
            else:
                L = H if base[0] == "y" else W
                assert e[-1] and c[-1] > f32(L) and c[-1] <= f32(L) + f32(4e-6)
    same = [n for n in names if n.startswith("inside_again")]
    assert len(same) == 3 and all((d[n][0] == rois[0]).all() and d[n][1] == levels[0] for n in same)


def test_roi_many_takes_a_second_list_pass():
    rois, levels = pp.roi_many()
    assert len(rois) == 300 > 256 and (levels == 0).all() and (rois[:, 0] == 1).all()
    assert (rois[::3] == rois[0]).all() and len(np.unique(rois, axis=0)) > 100


def _oracle_forward_check(C, PH, PW, sr):
    from oracle import native
    feats, rois, levels, names, per = pp.roi_forward_case(C, PH, PW, sr)
    for l, (H, W, s) in enumerate(pp.ROI_LEVELS):
        idx, ref, sabs, grid = per[l]
        got = native.roi_align_forward(torch.from_numpy(feats[l].copy()), torch.from_numpy(rois[idx].copy()), s, PH, PW, sr).numpy()
        bound = pp.roi_forward_bound(sabs, grid)
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= bound).all(), (l, float((err - bound).max()))
        assert (got[sabs == 0] == 0).all() and (ref[sabs == 0] == 0).all()
        for i, k in enumerate(idx):
            if names[k].split("/")[0] in ("left_of_map", "above_map", "beyond_far_corner"):
                assert (sabs[i] == 0).all(), names[k]
        if sr == 0:
            assert grid.max() > 3      # the adaptive grid really grows


@pytest.mark.parametrize("sr", pp.ROI_SRS)
@pytest.mark.parametrize("PH,PW", pp.ROI_POOLS)
def test_roi_reference_forward_vs_oracle(PH, PW, sr):
    _oracle_forward_check(6, PH, PW, sr)


def test_roi_reference_forward_vs_oracle_second_channel_pass():
    _oracle_forward_check(260, 2, 3, 2)


@pytest.mark.parametrize("sr", pp.ROI_SRS)
@pytest.mark.parametrize("PH,PW", [(2, 3), (7, 7)])
def test_roi_reference_backward_vs_oracle(PH, PW, sr):
    from oracle import native
    C = 6
    gout, rois, levels, per = pp.roi_backward_case(C, PH, PW, sr)
    for l, (H, W, s) in enumerate(pp.ROI_LEVELS):
        ref, sabs, T = per[l]
        idx = np.nonzero(levels == l)[0]
        got = native.roi_align_backward(torch.from_numpy(gout[idx].copy()), torch.from_numpy(rois[idx].copy()), s, PH, PW,
                                        pp.ROI_N, C, H, W, sr).numpy()
        bound = pp.roi_backward_bound(sabs, T)
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= bound).all(), (l, float((err - bound).max()))
        assert (got[sabs == 0] == 0).all()
        assert T.max() > 8       # texels where many contributions meet


def test_bf16_round_is_torch_s():
    a = np.random.RandomState(0).standard_normal(4096).astype(f32)
    a[:4] = (1.00390625, 1.01171875, -1.00390625, 0.0)     # ties: to even
    assert np.array_equal(pp.bf16_round(a), torch.from_numpy(a).to(torch.bfloat16).float().numpy())


# ================================================================================================================= matcher
def _area(b):
    return (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)


def test_match_inputs_hold_their_cases():
    cands, gts, labels = pp.match_inputs()
    coff = pp.offsets([len(c) for c in cands])
    assert coff.tolist() == [0, 3, 3, 303, 308]
    # block 0 (candidates 0 .. 255) touches images 0, 1 (empty) and 2; block 1 (256 .. 307) images 2 and 3
    assert coff[1] <= 255 and coff[2] == coff[1] and coff[2] <= 255 < coff[3] and coff[3] < 308 <= 512
    q0, q2 = pp.iou64(gts[0], cands[0]), pp.iou64(gts[2], cands[2])
    assert q0[0, 0] == 0.5 and q0[1, 1] == 0.3 and q0[0, 2] == 0.7 and q0[1].max() == 0.3     # 0.3 is box 1's best: restored
    assert (gts[2][0] == gts[2][1]).all() and (q2[0] == q2[1]).all()
    assert q2[0, pp.C_HALF] == 0.5 and q2[0, pp.C_07] == 0.7 and q2[0, pp.C_03] == 0.3 and q2[2, pp.C_EQUAL] == 1.0
    c = cands[2]
    assert c[pp.C_AREA0, 2] == c[pp.C_AREA0, 0] - 1 and _area(c)[pp.C_AREA0] == 0 and (q2[:, pp.C_AREA0] == 0).all()
    assert (c[pp.C_TWIN] == c[pp.C_07]).all()
    assert (q2[3] == 0).all()                     # the box nothing overlaps
    assert (q2[:3].max(0) > 0).sum() > 20 and (q2[:3].max(0) == 0).sum() > 20
    # the same values in fp32, against the fp32 thresholds
    from maskrcnn_benchmark.structures.boxlist_ops import box_iou_tensor
    g, cc = torch.from_numpy(gts[2].copy()), torch.from_numpy(c.copy())
    q32 = box_iou_tensor(g, _area(g), cc, _area(cc)).numpy()
    assert q32[0, pp.C_HALF] == f32(0.5) and q32[0, pp.C_07] == f32(0.7) and q32[0, pp.C_03] == f32(0.3)
    assert len(gts[1]) == 1 and len(cands[1]) == 0 and len(gts[3]) == 0 and len(cands[3]) == 5


@pytest.mark.parametrize("lowq", [False, True])
@pytest.mark.parametrize("high,low", pp.MATCH_THRESHOLDS)
def test_matcher_formulation_vs_tensor_modules(high, low, lowq):
    from maskrcnn_benchmark.modeling.matcher import Matcher
    from maskrcnn_benchmark.structures.boxlist_ops import box_iou_tensor
    cands, gts, labels = pp.match_inputs()
    exp = pp.match_expected(cands, gts, labels, high, low, lowq, pp.MATCH_WEIGHTS)
    matcher = Matcher(high, low, allow_low_quality_matches=lowq)
    for i in (0, 2):
        g, c = torch.from_numpy(gts[i].copy()), torch.from_numpy(cands[i].copy())
        ref = matcher(box_iou_tensor(g, _area(g), c, _area(c))).numpy()
        assert np.array_equal(exp[i][0], ref), i
        rl = labels[i][np.maximum(ref, 0)].copy()
        rl[ref == -1], rl[ref == -2] = 0, -1
        assert np.array_equal(exp[i][2], rl)
    m2 = exp[2][0]
    assert m2[pp.C_HALF] == (0 if (lowq or high == 0.5) else -2)           # first of the two identical boxes
    assert m2[pp.C_07] == 0 and m2[pp.C_TWIN] == 0 and m2[pp.C_EQUAL] == 2
    assert m2[pp.C_03] == (0 if lowq else (-1 if low == 0.5 else -2))
    if lowq:
        assert (m2 >= 0).all()      # every candidate has IoU 0 == top with the uncovered box: all keep their arg-max
        assert exp[0][0].tolist() == [0 if high == 0.5 else -2, 1, 0]
    else:
        assert (m2 == -1).any() and (m2 >= 0).any()
    assert (exp[3][0] == -1).all() and (exp[3][2] == 0).all() and (exp[3][3] == 0).all() and (exp[3][1] == 0).all()
    assert exp[1][0].shape == (0,)


def _encode_margin():
    from maskrcnn_benchmark.modeling.box_coder import BoxCoder
    cands, gts, labels = pp.match_inputs()
    worst = 0.0
    for weights in ((1.0, 1.0, 1.0, 1.0), pp.MATCH_WEIGHTS):
        for i in (0, 2):
            for gi in range(len(gts[i])):
                g = np.repeat(gts[i][gi:gi + 1], len(cands[i]), 0)
                keep = _area(cands[i]) > 0
                got = BoxCoder(weights).encode(torch.from_numpy(g[keep].copy()), torch.from_numpy(cands[i][keep].copy())).numpy()
                worst = max(worst, pp.rel_err(got, pp.encode64(g[keep], cands[i][keep], weights)))
    return worst


def test_encode_fp32_margin():
    """measured: the fp32 tensor formulation of BoxCoder.encode on the CPU lies within ENCODE_REL (relative) of encode64 on
    every (ground truth, candidate) pair of the matcher inputs -- the division's rounding in front of the logarithm, amplified
    where the ratio is near 1, is most of it; zero targets are exactly zero in both.  The kernel gets twice the figure."""
    worst = _encode_margin()
    print("encode fp32 vs float64, largest relative error: %.3e" % worst)
    assert worst <= pp.ENCODE_REL and worst >= 0.5 * pp.ENCODE_REL, worst


# ============================================================================================================ level mapper
def test_level_boxes_hold_their_cases():
    from maskrcnn_benchmark.modeling.poolers import LevelMapper
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    names, boxes = pp.level_boxes()
    l64, l32 = pp.level_ref(boxes, np.float64), pp.level_ref(boxes, np.float32)
    assert np.array_equal(l64, l32)                      # a condition on the inputs: no box sits where the precision decides
    d = dict(zip(names, l64.tolist()))
    area = _area(boxes.astype(np.float64))
    for s, lv, below in ((56, 0, 0), (112, 1, 0), (224, 2, 1), (448, 3, 2), (896, 3, 3)):     # 56 and 896 sit behind the clamps
        i = names.index("sqrt_area_%d" % s)
        assert math.sqrt(area[i]) == s and np.sqrt(_area(boxes)[i]) == f32(s) and math.log2(s / 224.0) == round(math.log2(s / 224.0))
        assert area[i + 1] == s * (s - 1) and names[i + 1] == "below_%d" % s
        assert d["sqrt_area_%d" % s] == lv and d["below_%d" % s] == below
    no_eps = pp.level_ref(boxes, np.float32, eps=0.0)
    for s in (112, 224):                                   # eps decides: without it the level is one lower
        i = names.index("eps_decides_%d" % s)
        assert math.sqrt(area[i]) < s and l32[i] == d["sqrt_area_%d" % s] and no_eps[i] == l32[i] - 1
    assert np.array_equal(np.delete(no_eps, [names.index("eps_decides_%d" % s) for s in (112, 224)]),
                          np.delete(l32, [names.index("eps_decides_%d" % s) for s in (112, 224)]))
    b = boxes[names.index("one_pixel")]
    assert b[2] == b[0] and b[3] == b[1] and d["one_pixel"] == 0
    b = boxes[names.index("area_0")]
    assert b[2] == b[0] - 1 and area[names.index("area_0")] == 0 and d["area_0"] == 0
    assert d["clamp_4000"] == 3 and math.floor(4 + math.log2(4000 / 224.0)) > 5
    mapper = LevelMapper(pp.LEVEL_KMIN, pp.LEVEL_KMAX, pp.LEVEL_S0, pp.LEVEL_LVL0, pp.LEVEL_EPS)
    got = mapper([BoxList(torch.from_numpy(boxes.copy()), (4000, 4000), "xyxy")]).numpy()
    assert np.array_equal(got, l64)


# ============================================================================================================== box decode
@pytest.mark.parametrize("R", [1, 257])
@pytest.mark.parametrize("ncls", [1, 3])
@pytest.mark.parametrize("weights", pp.DECODE_WEIGHTS, ids=["w1", "w10"])
def test_decode_inputs_and_formulation(weights, ncls, R):
    from maskrcnn_benchmark.modeling.box_coder import BoxCoder
    codes, boxes, row_off, lim = pp.decode_inputs(R, ncls, weights)
    clip = f32(pp.DECODE_CLIP)
    above = np.nextafter(clip, f32(np.inf))
    qs = np.concatenate([codes[:, 2::4] / f32(weights[2]), codes[:, 3::4] / f32(weights[3])], 1)
    assert qs.dtype == f32
    if R > 3:
        qs = np.delete(qs, (2, 3), 0)
    want = (clip, -40.0) if R == 1 and ncls == 1 else (clip, above, -40.0, 0.0)
    for v in want:
        assert (qs == f32(v)).any(), v
    assert row_off[0] == row_off[1] == 0 and row_off[-1] == row_off[-2] == R
    coder = BoxCoder(weights)
    ref = pp.decode64(codes, boxes, weights, float(clip))
    t32 = coder.decode(torch.from_numpy(codes.copy()), torch.from_numpy(boxes.copy())).numpy()
    scale = np.maximum(np.abs(ref).max(1), 1.0)[:, None]
    assert (np.abs(t32 - ref) <= 1e-6 * scale + 1e-4).all()
    # -40: the width collapses, x2 == x1 - 1 to fp32
    k = np.argwhere(codes[:, 2::4] / f32(weights[2]) == f32(-40.0))
    if len(k):
        r, c = k[0]
        assert abs((ref[r, 4 * c + 2] - ref[r, 4 * c]) + 1.0) < 1e-12
    if R > 3:
        cl = pp.decode64(codes, boxes, weights, float(clip), row_off, lim)
        img = 1     # rows 2 and 3 belong to image 1 (the first one is empty)
        assert row_off[img] <= 2 and 3 < row_off[img + 1]
        assert (cl[2].reshape(-1, 4) == np.asarray([lim[img][0], lim[img][1]] * 2)).all() and (ref[2].reshape(-1, 4)[:, :2] > lim[img]).all()
        assert (cl[3] == 0).all() and (ref[3] < 0).all()


# ================================================================================================================== losses
@pytest.mark.parametrize("kind", ["mixed", "none", "pos", "neg"])
@pytest.mark.parametrize("R", [1, 257])
@pytest.mark.parametrize("beta", pp.RPN_BETAS, ids=["ninth", "eighth"])
def test_rpn_loss_formulation_vs_autograd(beta, R, kind):
    obj, reg, labels, regt, pos, neg = pp.rpn_loss_inputs(R, beta, kind)
    b = f32(beta)
    d = np.abs(reg - regt)
    assert (labels[~(pos | neg)] == -1).all() and (labels[pos] == 1).all() and (labels[neg] == 0).all()
    if kind in ("mixed", "pos"):
        assert (d[pos] == b).any() and (d[pos] == np.nextafter(b, f32(0))).any() and (d[pos] == 0).any()
    if R > 1 and kind != "none":
        s = pos | neg
        assert (obj[s] == 100).any() and (obj[s] == -100).any()
    (lo, lb), dobj, dreg = pp.rpn_loss64(obj, reg, labels, regt, pos, neg, float(b))
    if kind == "none":
        assert lo == 0 and lb == 0 and not dobj.any() and not dreg.any()
    if kind == "neg":
        assert lb == 0 and not dreg.any()
    assert (dreg[(reg - regt) == 0] == 0).all()
    o, r = torch.tensor(obj, dtype=torch.float64, requires_grad=True), torch.tensor(reg, dtype=torch.float64, requires_grad=True)
    s = torch.tensor(pos | neg)
    n = max(int(s.sum()), 1)
    dd = torch.abs(r - torch.tensor(regt, dtype=torch.float64))
    sl1 = torch.where(dd < float(b), 0.5 * dd * dd / float(b), dd - 0.5 * float(b))
    wb = (sl1 * torch.tensor(pos, dtype=torch.float64)[:, None]).sum() / n
    wo = (torch.nn.functional.binary_cross_entropy_with_logits(o, torch.tensor(labels, dtype=torch.float64).clamp(min=0), reduction="none")
          * s.double()).sum() / n
    wo.backward()
    wb.backward()
    assert lo == pytest.approx(wo.item(), rel=1e-12, abs=1e-300) and lb == pytest.approx(wb.item(), rel=1e-12, abs=1e-300)
    assert np.allclose(dobj, o.grad.numpy(), rtol=1e-12, atol=1e-300) and np.allclose(dreg, r.grad.numpy(), rtol=1e-12, atol=0)


def test_rpn_loss_long_input_runs_past_the_block_cap():
    R = 256 * 1024 + 257          # MMT_RPN_LOSS_MAX_BLOCKS blocks of 256, then a ragged second trip of the grid-stride loop
    obj, reg, labels, regt, pos, neg = pp.rpn_loss_inputs(R, 0.125)
    assert len(obj) == R and R > 256 * 1024 and (R - 256 * 1024) % 256 != 0 and pos[-257:].any() and neg[-257:].any()


@pytest.mark.parametrize("kind", ["mixed", "moderate", "background", "padding"])
@pytest.mark.parametrize("R", [1, 257])
@pytest.mark.parametrize("NC", [2, 81])
def test_box_loss_formulation_vs_autograd(NC, R, kind):
    logits, breg, labels, regt = pp.box_loss_inputs(R, NC, kind)
    n_rows = int((labels >= 0).sum())
    (lc, lb), dl, db = pp.box_loss64(logits, breg, labels, regt, n_rows)
    if kind == "padding":
        assert n_rows == 0 and lc == 0 and lb == 0 and not dl.any() and not db.any()
        return
    if kind == "background":
        assert lb == 0 and not db.any()
    if kind == "moderate":
        e = np.exp(logits.astype(np.float64) - logits.max(1, keepdims=True))
        assert 5 < np.abs(logits).max() <= 14 and (R == 1 or (1 - (e / e.sum(1, keepdims=True)).max(1)).min() < 2e-2)     # NC 2: 4e-6, NC 81: 1e-2
    else:
        assert (np.abs(logits) == 80).all(1).any()
    if kind in ("mixed", "moderate"):
        fg = np.nonzero(labels > 0)[0]
        e = np.stack([breg[i, 4 * labels[i]:4 * labels[i] + 4] - regt[i] for i in fg])
        assert (np.abs(e) == 1).any() and (R == 1 or (e == 0).any())
        assert R == 1 or ((labels == -1).any() and (labels == 0).any())
    keep = labels >= 0
    l2 = torch.tensor(logits[keep], dtype=torch.float64, requires_grad=True)
    b2 = torch.tensor(breg[keep], dtype=torch.float64, requires_grad=True)
    lab = torch.tensor(labels[keep])
    wc = torch.nn.functional.cross_entropy(l2, lab)
    idx = (4 * lab)[:, None] + torch.arange(4)[None, :]
    d = torch.abs(torch.gather(b2, 1, idx) - torch.tensor(regt[keep], dtype=torch.float64))
    wb = (torch.where(d < 1.0, 0.5 * d * d, d - 0.5) * (lab > 0).double()[:, None]).sum() / n_rows
    wc.backward()
    wb.backward()
    assert lc == pytest.approx(wc.item(), rel=1e-12) and lb == pytest.approx(wb.item(), rel=1e-12, abs=1e-300)
    assert np.allclose(dl[keep], l2.grad.numpy(), rtol=1e-10, atol=1e-15)      # (softmax - 1 cancels in float64 too: 1e-16 of 1) and np.allclose(db[keep], b2.grad.numpy(), rtol=1e-12, atol=0)
    assert not dl[~keep].any() and not db[~keep].any()
