"""The kernels between the RPN and the heads at their edges: ROIAlign (csrc/roi_align.hip), the target matcher, box decode and
the level mapper (csrc/targets.hip) and the two detection losses (csrc/losses.hip) on the constructed inputs of
tests/proposal_path_inputs.py, against its plain references (tests/test_proposal_path_inputs.py checks both on the CPU).

Tolerances.  ROIAlign forward: (8 gh gw + 2) 2^-24 S_abs / count per element -- one rounding per product and per add of the
kernel's chain plus the division, S_abs the sum of the magnitudes the reference added; backward: (T + 3) 2^-24 S_abs per texel,
T the number of contributions (the order of the atomics is free, so the bound is on the sum of magnitudes); where S_abs is 0 the
result is exactly 0.  Matches, labels, levels, clamped corners and the "exactly 0" cases: equality.  Regression targets: twice
the relative error of the fp32 tensor formulation on the CPU against float64 on the same inputs (measured 2.28e-6, recorded as
proposal_path_inputs.ENCODE_REL; logf of another library).  Decoded corners: 1e-6 * scale + 1e-4 as in
test_hip_kernels.py::test_box_decode_kernel.  Loss sums: rel 1e-5 against float64; gradients rtol 1e-5, atol 1e-9 as in the two
loss tests there (the plain logits stay within +-1 so that softmax - 1 does not cancel below what fp32 can hold to 1e-5)."""
import ctypes

import numpy as np
import pytest
import torch

import proposal_path_inputs as pp

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def hip():
    from maskrcnn_benchmark import _hip
    _hip.lib()
    return _hip


@pytest.fixture(autouse=True)
def _scatter_by_default(monkeypatch):
    monkeypatch.delenv("MMT_ROI_BWD_DENSE", raising=False)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()      # (a copy: the inputs are read-only)


def cl(a, dtype=None):
    """[N, C, H, W] array -> NHWC-dense cuda tensor"""
    t = torch.from_numpy(np.array(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous(memory_format=torch.channels_last)


def host(t):
    return t.detach().cpu().numpy()


def stream():
    return torch.cuda.current_stream().cuda_stream


# ================================================================================================================ ROIAlign
def _check_forward(got, per, names=None):
    """got [K, C, PH, PW] against the per-level references: the bound, exact zeros where nothing was added, NaN / Inf in place"""
    worst = 0.0
    for idx, ref, sabs, grid in per:
        if not len(idx):
            continue
        g = got[idx].astype(np.float64)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(g), np.isnan(ref))
        assert np.array_equal(g[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
        bound = pp.roi_forward_bound(np.where(fin, sabs, 0.0), grid)
        err = np.where(fin, np.abs(g - np.where(fin, ref, 0.0)), 0.0)
        assert (err <= bound).all(), float((err - bound).max())
        assert (g[fin & (sabs == 0)] == 0).all()
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


@pytest.mark.parametrize("sr", pp.ROI_SRS)
@pytest.mark.parametrize("PH,PW", pp.ROI_POOLS)
@pytest.mark.parametrize("C", pp.ROI_CS)
def test_roi_forward(hip, C, PH, PW, sr):
    """C = 4 / 64: one pass of the float4 channel loop (with idle lanes at 4); 260: a second, ragged pass; 6: the VEC == 1
    kernel.  sr = 0: the adaptive grid.  ROIs: proposal_path_inputs.roi_list"""
    feats, rois, levels, names, per = pp.roi_forward_case(C, PH, PW, sr)
    y = hip.roi_align_forward([cl(f) for f in feats], pp.ROI_SCALES, dev(rois), dev(levels), PH, PW, sr)
    assert tuple(y.shape) == (len(rois), C, PH, PW)
    got = host(y)
    _check_forward(got, per)
    for k, n in enumerate(names):
        if n.split("/")[0] in ("left_of_map", "above_map", "beyond_far_corner") or n.endswith("_beyond") and (PH, PW, sr) == (1, 1, 1):
            assert (got[k] == 0).all(), n      # every sample empty: exactly 0


@pytest.mark.parametrize("PH,PW,sr", [(2, 3, 2), (7, 7, 0), (1, 1, 3)])
@pytest.mark.parametrize("C", [4, 64, 260])
def test_roi_forward_bf16(hip, C, PH, PW, sr):
    """the bf16-storage forward (taps widened exactly, fp32 arithmetic) against the reference fed the bf16-rounded map -- with
    ROIs that leave the map"""
    feats, rois, levels, names, per = pp.roi_forward_case(C, PH, PW, sr, bf16=True)
    y = hip.roi_align_forward([cl(f, torch.bfloat16) for f in feats], pp.ROI_SCALES, dev(rois), dev(levels), PH, PW, sr)
    assert y.dtype == torch.float32
    got = host(y)
    _check_forward(got, per)
    for k, n in enumerate(names):
        if n.split("/")[0] in ("left_of_map", "above_map", "beyond_far_corner"):
            assert (got[k] == 0).all(), n


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("C", [4, 6])
def test_roi_forward_empty_samples_read_nothing(hip, C, bad):
    """texel (0, 0) of every image is NaN (+Inf) on otherwise finite maps.  An empty sample has weight 0 and indices 0: adding
    0 * texel (0, 0) for it -- as the forward did before it skipped empty samples -- leaks NaN into ROIs that never touch the
    texel.  An ROI whose samples are all empty pools exactly 0; one that taps the texel with a non-zero weight pools NaN (Inf)."""
    PH, PW, sr = 2, 3, 2
    clean, rois, levels, names, _ = pp.roi_forward_case(C, PH, PW, sr)
    feats = [f.copy() for f in clean]
    for f in feats:
        f[:, :, 0, 0] = bad
    per = []
    with np.errstate(invalid="ignore"):
        for l, (H, W, s) in enumerate(pp.ROI_LEVELS):
            idx = np.nonzero(levels == l)[0]
            per.append((idx,) + pp.roi_align_reference(feats[l], rois[idx], s, PH, PW, sr))
    got = host(hip.roi_align_forward([cl(f) for f in feats], pp.ROI_SCALES, dev(rois), dev(levels), PH, PW, sr))
    for k, n in enumerate(names):
        base = n.split("/")[0]
        if base in ("left_of_map", "above_map", "beyond_far_corner"):
            assert (got[k] == 0).all(), n
        if base in ("inside", "last_row_and_column", "y_at_H_beyond"):
            assert np.isfinite(got[k]).all(), n
    tapped = sum(int((~np.isfinite(ref)).sum()) for _, ref, _, _ in per)
    assert tapped > 0 and not np.isfinite(got[[k for k, n in enumerate(names) if n.startswith("straddles_top_left")]]).all()
    with np.errstate(invalid="ignore"):
        _check_forward(got, per)


def test_roi_forward_no_roi_and_one_bin(hip):
    """K = 0; and K = 1 at 1 x 1: one bin, three of the block's four waves have nothing to do"""
    C = 64
    feats = pp.roi_features(C)
    y = hip.roi_align_forward([cl(f) for f in feats], pp.ROI_SCALES, torch.zeros(0, 5).cuda(), torch.zeros(0).int().cuda(), 7, 7, 2)
    assert tuple(y.shape) == (0, C, 7, 7)
    roi = np.asarray([[1.0, 3.0, 2.0, 15.0, 13.0]], f32)
    y = hip.roi_align_forward([cl(f) for f in feats], pp.ROI_SCALES, dev(roi), torch.zeros(1).int().cuda(), 1, 1, 2)
    ref, sabs, grid = pp.roi_align_reference(feats[0], roi, 0.5, 1, 1, 2)
    _check_forward(host(y), [(np.arange(1), ref, sabs, grid)])
    g = hip.roi_align_backward(cl(np.ones((1, C, 1, 1), f32)), pp.roi_shapes(C), pp.ROI_SCALES, dev(roi), torch.zeros(1).int().cuda(), 1, 1, 2)
    gr, gs, T = pp.roi_align_backward_reference(np.ones((1, C, 1, 1)), roi, 0.5, 1, 1, 2, pp.roi_shapes(C)[0])
    assert (np.abs(host(g[0]) - gr) <= pp.roi_backward_bound(gs, T)).all() and not host(g[1]).any()


def test_roi_forward_many_copies(hip):
    feats, rois, levels, names, per = pp.roi_forward_case(64, 2, 3, 2, many=True)
    y = hip.roi_align_forward([cl(f) for f in feats], pp.ROI_SCALES, dev(rois), dev(levels), 2, 3, 2)
    _check_forward(host(y), per)


def _check_backward(grads, per, prefill=None):
    for l, (ref, sabs, T) in enumerate(per):
        g = host(grads[l]).astype(np.float64)
        if prefill is not None and prefill[l] is not None:
            # the pre-fill is one more term of every texel's sum: T + 1 terms of magnitudes S_abs + |pre-fill|
            p = prefill[l].astype(np.float64)
            bound = (T[:, None] + 4.0) * pp.U * (sabs + np.abs(p))
            assert (np.abs(g - (p + ref)) <= bound).all(), l
            assert np.array_equal(g[sabs == 0], p[sabs == 0])
        else:
            bound = pp.roi_backward_bound(sabs, T)
            err = np.abs(g - ref)
            assert (err <= bound).all(), (l, float((err - bound).max()))
            assert (g[sabs == 0] == 0).all()


@pytest.mark.parametrize("PH,PW", [(2, 3), (7, 7)])
@pytest.mark.parametrize("sr", pp.ROI_SRS)
@pytest.mark.parametrize("C", pp.ROI_CS)
def test_roi_backward_scatter(hip, C, sr, PH, PW):
    """sr = 2: the folded 2 x 2 path (C = 4 and 260: its `c < C` tails; C = 6 goes there too); every other sr: the generic
    per-sample path, VEC == 4 and VEC == 1.  Then `into=`: a pre-filled level keeps its content plus the reference."""
    gout, rois, levels, per = pp.roi_backward_case(C, PH, PW, sr)
    shapes = pp.roi_shapes(C)
    args = (cl(gout), shapes, pp.ROI_SCALES, dev(rois), dev(levels), PH, PW, sr)
    grads = hip.roi_align_backward(*args)
    _check_backward(grads, per)
    rng = np.random.RandomState(C + sr)
    pre = [rng.standard_normal(shapes[0]).astype(f32), None]
    into = [cl(pre[0]), None]
    out = hip.roi_align_backward(*args, into=into)
    assert out[0].data_ptr() == into[0].data_ptr()
    _check_backward(out, per, prefill=pre)


def test_roi_backward_all_empty_adds_nothing(hip):
    C, PH, PW, sr = 64, 7, 7, 2
    names, rois, levels = pp.roi_list(PH, PW, sr)
    pick = [k for k, n in enumerate(names) if n.split("/")[0] in ("left_of_map", "above_map", "beyond_far_corner")]
    assert len(pick) == 6
    for s in (2, 3):     # the folded and the generic path
        gout = pp.roi_gout(len(pick), C, PH, PW)
        grads = hip.roi_align_backward(cl(gout), pp.roi_shapes(C), pp.ROI_SCALES, dev(rois[pick]), dev(levels[pick]), PH, PW, s)
        assert all(not host(g).any() for g in grads)


def _tile_call(hip, entry, gout_d, rois_d, levels_d, K, PH, PW, sr, bufs, *mask):
    p = hip._pyramid([b.permute(0, 3, 1, 2) for b in bufs], pp.ROI_SCALES, bufs)
    rc = getattr(hip.lib(), entry)(ctypes.byref(p), rois_d.data_ptr(), levels_d.data_ptr(), K, PH, PW, sr, gout_d.data_ptr(), *mask,
                                   stream())
    torch.cuda.synchronize()
    return rc


def _nan_bufs(C):
    return [torch.full((pp.ROI_N, H, W, C), float("nan"), device="cuda") for H, W, _ in pp.ROI_LEVELS]


@pytest.mark.parametrize("PH,PW,many", [(7, 7, False), (2, 3, False), (2, 3, True)], ids=["7x7", "2x3", "300-copies"])
def test_roi_backward_tiles(hip, PH, PW, many, monkeypatch):
    """the tile-gather form at C = 64, sr = 2 on maps that are no multiple of the tile: every element written over NaN, equal to
    the reference, bit-equal from call to call and to the wrapper's opt-in path; with accumulate_mask 0b01 level 0 is pre-fill +
    sum and level 1 the sum alone.  (test_deterministic_kernels_gpu.py::test_roi_align_backward_ordered asserts the accumulate
    rule against the kernel's own plain result on random ROIs; here it is tied to the reference, on the edge ROIs.)"""
    C, sr = 64, 2
    gout, rois, levels, per = pp.roi_backward_case(C, PH, PW, sr, many=many)
    K = len(rois)
    g_d, r_d, l_d = cl(gout), dev(rois), dev(levels)
    runs = []
    for _ in range(2):
        bufs = _nan_bufs(C)
        assert _tile_call(hip, "mmt_roi_align_backward_ordered", g_d, r_d, l_d, K, PH, PW, sr, bufs, 0) == 0
        runs.append([b.permute(0, 3, 1, 2) for b in bufs])
    for a, b in zip(*runs):
        assert not torch.isnan(a).any().item() and torch.equal(a, b)
    _check_backward(runs[0], per)
    monkeypatch.setenv("MMT_ROI_BWD_DENSE", "1")
    dense = hip.roi_align_backward(g_d, pp.roi_shapes(C), pp.ROI_SCALES, r_d, l_d, PH, PW, sr)
    monkeypatch.delenv("MMT_ROI_BWD_DENSE")
    assert all(torch.equal(a, b) for a, b in zip(dense, runs[0]))
    scatter = hip.roi_align_backward(g_d, pp.roi_shapes(C), pp.ROI_SCALES, r_d, l_d, PH, PW, sr)
    _check_backward(scatter, per)
    # accumulate_mask 0b01
    H0, W0, _ = pp.ROI_LEVELS[0]
    pre = torch.from_numpy(np.random.RandomState(5).standard_normal((pp.ROI_N, H0, W0, C)).astype(f32)).cuda()
    bufs = _nan_bufs(C)
    bufs[0] = pre.clone()
    assert _tile_call(hip, "mmt_roi_align_backward_ordered", g_d, r_d, l_d, K, PH, PW, sr, bufs, 0b01) == 0
    assert torch.equal(bufs[0].permute(0, 3, 1, 2), pre.permute(0, 3, 1, 2) + runs[0][0])
    assert torch.equal(bufs[1].permute(0, 3, 1, 2), runs[0][1])


@pytest.mark.parametrize("C,sr", [(260, 2), (64, 3), (64, 0), (6, 2)])
def test_roi_backward_tiles_not_taken(hip, C, sr, monkeypatch):
    """what the tile kernel does not take (C no multiple of 64 or above 256, sr != 2): the entry point answers 1 and touches
    nothing; the wrapper's opt-in path still returns the reference-equal gradient (by the scatter kernel)"""
    PH, PW = 2, 3
    gout, rois, levels, per = pp.roi_backward_case(C, PH, PW, sr)
    g_d, r_d, l_d = cl(gout), dev(rois), dev(levels)
    monkeypatch.setenv("MMT_ROI_BWD_DENSE", "1")
    bufs = _nan_bufs(C)
    assert _tile_call(hip, "mmt_roi_align_backward_dense", g_d, r_d, l_d, len(rois), PH, PW, sr, bufs) == 1
    assert all(torch.isnan(b).all().item() for b in bufs)
    bufs = _nan_bufs(C)
    assert _tile_call(hip, "mmt_roi_align_backward_ordered", g_d, r_d, l_d, len(rois), PH, PW, sr, bufs, 0) == 1
    assert all(torch.isnan(b).all().item() for b in bufs)
    grads = hip.roi_align_backward(g_d, pp.roi_shapes(C), pp.ROI_SCALES, r_d, l_d, PH, PW, sr)
    _check_backward(grads, per)


# ================================================================================================================= matcher
def _check_targets(got, ref, tol):
    """regression targets: non-finite entries (the area-0 candidate divides by 0) in place, the others within tol (relative),
    zeros exact"""
    got, ref = got.astype(np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
    worst = pp.rel_err(got[fin], ref[fin])
    assert worst <= tol, worst
    return worst


@pytest.mark.parametrize("lowq", [False, True], ids=["plain", "lowq"])
@pytest.mark.parametrize("high,low", pp.MATCH_THRESHOLDS)
def test_match_targets_per_image(hip, high, low, lowq):
    """four images with [3, 0, 300, 5] candidates and [2, 1, 4, 0] ground-truth boxes: block 0 touches images 0, 1 (no
    candidate) and 2, block 1 images 2 and 3; IoUs exactly on the thresholds; identical boxes and candidates; an uncovered box
    under allow_low_quality; image 3 has no ground truth -- all background by the contract of include/mmtpsm.h"""
    cands, gts, labels = pp.match_inputs()
    with np.errstate(divide="ignore", invalid="ignore"):
        exp = pp.match_expected(cands, gts, labels, high, low, lowq, pp.MATCH_WEIGHTS)
    coff, goff = pp.offsets([len(c) for c in cands]), pp.offsets([len(g) for g in gts])
    m, li, reg = hip.match_targets(dev(np.concatenate(cands)), dev(coff), dev(np.concatenate(gts)), dev(goff), 4, high, low, lowq,
                                   gt_labels=dev(np.concatenate(labels)), box_labels=True, weights=pp.MATCH_WEIGHTS)
    m, li, reg = host(m), host(li), host(reg)
    for i in range(4):
        a, e = coff[i], coff[i + 1]
        assert np.array_equal(m[a:e], exp[i][0]), i
        assert np.array_equal(li[a:e], exp[i][2]), i
        _check_targets(reg[a:e], exp[i][3], 2 * pp.ENCODE_REL)
    assert (m[coff[3]:] == -1).all() and (li[coff[3]:] == 0).all() and (reg[coff[3]:] == 0).all()


@pytest.mark.parametrize("lowq", [False, True], ids=["plain", "lowq"])
@pytest.mark.parametrize("high,low", pp.MATCH_THRESHOLDS)
def test_match_targets_shared_grid(hip, high, low, lowq):
    """the RPN form: one grid of 300 candidates for all four images, with visibility; RPN labels and unit-weight targets"""
    cands, gts, labels = pp.match_inputs()
    grid = cands[2]
    vis = (np.arange(len(grid)) % 7) != 3
    w1 = (1.0, 1.0, 1.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        exp = pp.match_expected([grid] * 4, gts, labels, high, low, lowq, w1, visible=vis)
    A = len(grid)
    coff, goff = pp.offsets([A] * 4), pp.offsets([len(g) for g in gts])
    m, lf, reg = hip.match_targets(dev(grid), dev(coff), dev(np.concatenate(gts)), dev(goff), 4, high, low, lowq, visible=dev(vis),
                                   shared_cand=True, rpn_labels=True, weights=w1)
    m, lf, reg = host(m), host(lf), host(reg)
    for i in range(4):
        assert np.array_equal(m[i * A:(i + 1) * A], exp[i][0]), i
        assert np.array_equal(lf[i * A:(i + 1) * A], exp[i][1]), i
        _check_targets(reg[i * A:(i + 1) * A], exp[i][3], 2 * pp.ENCODE_REL)
    last = slice(3 * A, 4 * A)
    assert (m[last] == -1).all() and (reg[last] == 0).all() and np.array_equal(lf[last], np.where(vis, 0.0, -1.0))


def test_match_targets_return_code_and_top(hip):
    """through the C ABI: the batch with an image without ground truth is accepted (0); the per-box maxima of the low-quality
    pass -- the box of the image without candidates and the uncovered box stay 0, the box equal to a candidate reaches 1; a
    batch without any ground truth takes null gt / gt_labels and is all background"""
    cands, gts, labels = pp.match_inputs()
    coff, goff = pp.offsets([len(c) for c in cands]), pp.offsets([len(g) for g in gts])
    c_d, co_d, g_d, go_d, gl_d = dev(np.concatenate(cands)), dev(coff), dev(np.concatenate(gts)), dev(goff), dev(np.concatenate(labels))
    A, G = int(coff[-1]), int(goff[-1])
    top = torch.full((G,), -1, dtype=torch.int32, device="cuda")
    m = torch.full((A,), 77, dtype=torch.int32, device="cuda")
    li = torch.full((A,), 77, dtype=torch.int64, device="cuda")
    reg = torch.full((A, 4), 77.0, device="cuda")
    rc = hip.lib().mmt_match_targets(c_d.data_ptr(), co_d.data_ptr(), g_d.data_ptr(), go_d.data_ptr(), gl_d.data_ptr(), None, 4, A, G, 0,
                                     0.7, 0.3, 1, 10.0, 10.0, 5.0, 5.0, top.data_ptr(), m.data_ptr(), None, li.data_ptr(),
                                     reg.data_ptr(), stream())
    assert rc == 0
    torch.cuda.synchronize()
    t = host(top).view(f32)
    assert t.tolist() == [f32(0.7), f32(0.3), 0.0, t[3], t[3], 1.0, 0.0] and t[3] >= f32(0.7)
    assert not (host(m) == 77).any() and not (host(li) == 77).any() and not (host(reg) == 77.0).any()
    # no ground truth at all
    zero = dev(np.zeros(5, np.int32))
    m.fill_(77), li.fill_(77), reg.fill_(77.0)
    rc = hip.lib().mmt_match_targets(c_d.data_ptr(), co_d.data_ptr(), None, zero.data_ptr(), None, None, 4, A, 0, 0,
                                     0.7, 0.3, 1, 10.0, 10.0, 5.0, 5.0, top.data_ptr(), m.data_ptr(), None, li.data_ptr(),
                                     reg.data_ptr(), stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert (host(m) == -1).all() and (host(li) == 0).all() and (host(reg) == 0).all()


# ============================================================================================================ level mapper
def _level_args():
    return dict(s0=pp.LEVEL_S0, lvl0=pp.LEVEL_LVL0, eps=pp.LEVEL_EPS, k_min=pp.LEVEL_KMIN, k_max=pp.LEVEL_KMAX)


def test_level_mapper(hip):
    """sqrt(area) / s0 on powers of two, just below them (the next integer area; a few fp32 steps, where eps decides), area 1,
    area 0 and the k_max clamp; three images with [0, n, 1] boxes; levels omitted; an unaligned box tensor (the clone path)"""
    names, boxes = pp.level_boxes()
    want = pp.level_ref(boxes)
    n = len(boxes) - 1
    imgs = [torch.zeros(0, 4).cuda(), dev(boxes[:n]), dev(boxes[n:])]
    rois, levels = hip.roi_format_levels(imgs, **_level_args())
    exp_rois = np.concatenate([np.asarray([1.0] * n + [2.0], f32)[:, None], boxes], 1)
    assert np.array_equal(host(rois), exp_rois)
    bad = [(nm, int(a), int(b)) for nm, a, b in zip(names, host(levels), want) if a != b]
    assert not bad, bad
    assert levels.dtype == torch.int32
    rois2, none = hip.roi_format_levels(imgs)
    assert none is None and np.array_equal(host(rois2), exp_rois)
    flat = torch.zeros(4 * len(boxes) + 1, device="cuda")
    flat[1:] = dev(boxes).reshape(-1)
    odd = flat[1:].view(-1, 4)
    assert odd.data_ptr() & 15
    rois3, levels3 = hip.roi_format_levels([odd], **_level_args())
    assert np.array_equal(host(rois3)[:, 1:], boxes) and (host(rois3)[:, 0] == 0).all() and np.array_equal(host(levels3), want)
    one, lv1 = hip.roi_format_levels([dev(boxes[:1])], **_level_args())
    assert np.array_equal(host(one)[0, 1:], boxes[0]) and host(lv1).tolist() == [int(want[0])]


# ============================================================================================================== box decode
@pytest.mark.parametrize("R", [1, 257])
@pytest.mark.parametrize("ncls", [1, 3])
@pytest.mark.parametrize("weights", pp.DECODE_WEIGHTS, ids=["w1", "w10"])
def test_box_decode(hip, weights, ncls, R):
    """size codes with code / w exactly the clip, one step above it, -40 and 0; one row and two blocks; per-image limits with an
    empty first and an empty last image; boxes wholly outside clamp with all four corners"""
    codes, boxes, row_off, lim = pp.decode_inputs(R, ncls, weights)
    clip = float(f32(pp.DECODE_CLIP))
    ref = pp.decode64(codes, boxes, weights, clip)
    own = host(hip.box_decode(dev(codes), dev(boxes), weights, pp.DECODE_CLIP))
    scale = np.maximum(np.abs(ref).max(1), 1.0)[:, None]
    err = np.abs(own - ref)
    assert (err <= 1e-6 * scale + 1e-4).all(), float((err / scale).max())
    clipped = host(hip.box_decode(dev(codes), dev(boxes), weights, pp.DECODE_CLIP, dev(row_off), dev(lim)))
    img = np.searchsorted(row_off[1:], np.arange(R), side="right")
    l4 = np.tile(np.stack([lim[img, 0], lim[img, 1]] * 2, 1), (1, ncls))
    assert np.array_equal(clipped, np.minimum(np.maximum(own, 0), l4))          # the clamp itself is exact
    assert set(img.tolist()) <= {1, 2}
    if R > 3:
        assert (clipped[2] == l4[2]).all() and (own[2].reshape(-1, 4) > l4[2].reshape(-1, 4)).all()
        assert (clipped[3] == 0).all() and (own[3] < 0).all()


# ================================================================================================================== losses
RPN_LONG = 256 * 1024 + 257      # MMT_RPN_LOSS_MAX_BLOCKS full blocks and a ragged second trip of the grid-stride loop


@pytest.mark.parametrize("R,kind", [(1, "mixed"), (257, "mixed"), (257, "none"), (257, "pos"), (257, "neg"), (1, "none"), (RPN_LONG, "mixed")])
@pytest.mark.parametrize("beta", pp.RPN_BETAS, ids=["ninth", "eighth"])
def test_rpn_loss(hip, beta, R, kind):
    """|reg - regt| exactly beta, one step below and exactly 0; logits +-100; labels -1 on unsampled anchors; no anchor sampled:
    everything exactly 0.  (At |d| == beta the two branches of smooth-L1 agree in value and in gradient -- e / beta is exactly
    +-1 --, so `d < beta` cannot be told from `d <= beta` by any input; what the case pins is that neither branch is off there.)"""
    assert hip.RPN_LOSS_MAX_BLOCKS == 1024
    obj, reg, labels, regt, pos, neg = pp.rpn_loss_inputs(R, beta, kind)
    out, dobj, dreg = hip.rpn_loss(dev(obj), dev(reg), dev(labels), dev(regt), dev(pos), dev(neg), beta)
    out, dobj, dreg = host(out), host(dobj), host(dreg)
    with np.errstate(over="ignore"):
        (lo, lb), go, gr = pp.rpn_loss64(obj, reg, labels, regt, pos, neg, float(f32(beta)))
    print("rpn loss", R, kind, out.tolist(), (lo, lb))
    if kind == "none":
        assert not out.any() and not dobj.any() and not dreg.any()
    if kind == "neg":
        assert out[1] == 0 and not dreg.any()
    assert out[0] == pytest.approx(lo, rel=1e-5, abs=1e-9) and out[1] == pytest.approx(lb, rel=1e-5, abs=1e-9)
    assert np.allclose(dobj, go, rtol=1e-5, atol=1e-9) and np.allclose(dreg, gr, rtol=1e-5, atol=1e-9)
    assert (dreg[(reg - regt) == 0] == 0).all() and (dobj[~(pos | neg)] == 0).all() and (dreg[~pos] == 0).all()


@pytest.mark.parametrize("kind", ["mixed", "background", "padding"])
@pytest.mark.parametrize("R", [1, 257])
@pytest.mark.parametrize("NC", [2, 81])
def test_box_loss(hip, NC, R, kind):
    """NC = 2 (the smallest) and 81; |e| exactly 1 and 0; rows of logits alternating +-80; all background: the box loss is
    exactly 0; all rows padding with n_rows = 0: everything exactly 0; and mmt_box_loss_rows against mmt_box_loss on the kept
    rows, as test_hip_kernels.py::test_box_loss_on_a_fixed_capacity_batch does"""
    logits, breg, labels, regt = pp.box_loss_inputs(R, NC, kind)
    n_rows = int((labels >= 0).sum())
    l_d, b_d, lab_d, t_d = dev(logits), dev(breg), dev(labels), dev(regt)
    out, dl, db = hip.box_loss(l_d, b_d, lab_d, t_d, n_rows=(lab_d >= 0).sum())
    (lc, lb), gl, gb = pp.box_loss64(logits, breg, labels, regt, n_rows)
    o = host(out)
    print("box loss", NC, R, kind, o.tolist(), (lc, lb))
    if kind == "padding":
        assert n_rows == 0 and not o.any() and not host(dl).any() and not host(db).any()
        return
    if kind == "background":
        assert o[1] == 0 and not host(db).any()
    assert o[0] == pytest.approx(lc, rel=1e-5) and o[1] == pytest.approx(lb, rel=1e-5, abs=1e-9)
    assert np.allclose(host(dl), gl, rtol=1e-5, atol=1e-9) and np.allclose(host(db), gb, rtol=1e-5, atol=1e-9)
    keep = lab_d >= 0
    out0, dl0, db0 = hip.box_loss(l_d[keep], b_d[keep], lab_d[keep], t_d[keep])
    assert torch.allclose(out, out0, rtol=1e-6, atol=1e-7)
    assert torch.equal(dl[keep], dl0) and torch.equal(db[keep], db0)
    assert not dl[~keep].any().item() and not db[~keep].any().item()


@pytest.mark.parametrize("NC", [2, 81])
def test_box_loss_moderate_logits(hip, NC):
    """logits over -8 .. 14: a confident row has softmax within 1e-3 of 1 and softmax - 1 cancels, which rtol 1e-5 of the small
    result cannot hold in fp32; the gradient gets the absolute bound derived in proposal_path_inputs.box_loss_grad_bound on top.
    The loss values and the box gradient keep the tolerances of test_box_loss."""
    R = 257
    logits, breg, labels, regt = pp.box_loss_inputs(R, NC, "moderate")
    n_rows = int((labels >= 0).sum())
    lab_d = dev(labels)
    out, dl, db = hip.box_loss(dev(logits), dev(breg), lab_d, dev(regt), n_rows=(lab_d >= 0).sum())
    (lc, lb), gl, gb = pp.box_loss64(logits, breg, labels, regt, n_rows)
    o = host(out)
    err = np.abs(host(dl) - gl)
    bound = 1e-5 * np.abs(gl) + 1e-9 + pp.box_loss_grad_bound(logits, labels, n_rows)
    print("box loss moderate", NC, o.tolist(), (lc, lb), "largest gradient error / bound: %.3f" % float((err / bound).max()))
    assert o[0] == pytest.approx(lc, rel=1e-5) and o[1] == pytest.approx(lb, rel=1e-5, abs=1e-9)
    assert (err <= bound).all()
    assert np.allclose(host(db), gb, rtol=1e-5, atol=1e-9)
