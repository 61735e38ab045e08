"""The selection family (csrc/nms.hip, csrc/select.hip, the matcher of csrc/targets.hip) at its limits, ties and chains:
constructed inputs and plain numpy references from tests/selection_edge_inputs.py (tests/test_selection_edge_inputs.py
checks on the CPU that the inputs reach the paths they name).  Outputs are indices, masks, counts and copies of input
floats: everything is compared exactly.  The one place where indices are not compared is the top-k segment that holds
both +0.0 and -0.0 (the kernel orders +0 first, the reference leaves the order between equal values open): values there.
Not covered on purpose: NaN logits, and NMS segments of more than 4096 boxes (refused, see test_nms_limit)."""
import ctypes

import numpy as np
import pytest
import torch

import selection_edge_inputs as se

pytestmark = pytest.mark.gpu

EINVAL = "code -22"


@pytest.fixture(scope="module")
def hip():
    from maskrcnn_benchmark import _hip
    _hip.lib()
    return _hip


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


# ==================================================================================================================== NMS
def _segments(segs):
    off = np.concatenate([[0], np.cumsum([len(b) for b in segs])]).astype(np.int32)
    return np.concatenate([b.reshape(-1, 4) for b in segs]).astype(np.float32), off


@pytest.fixture(scope="module")
def nms_groups():
    return se.nms_groups()


@pytest.mark.parametrize("group", ["chains", "grid", "special", "pair_above", "random"])
def test_nms_group(hip, nms_groups, group):
    """one batched call per group: a chain that fills a chunk needs 63 rounds of the sweep's fixpoint iteration where random
    boxes need a handful (position i is final after i rounds; the 64th only confirms the fixpoint) -- 64, 65 and 200 boxes:
    a full chunk, one box into the next, three chunks and a part; the grid carries a suppression from chunk 0 to the last
    bit of word 63 at max_n = 4096 (64 KB of LDS), the specials are identical / all-zero / exact-threshold / zero-area
    boxes, the random segments sit on every chunk boundary"""
    max_n, thr, segs = nms_groups[group]
    boxes, off = _segments(segs)
    keep, cnt = hip.nms_batched(dev(boxes), dev(off), max_n, thr)
    keep, cnt = host(keep), host(cnt)
    for s, b in enumerate(segs):
        ref = se.nms_ref(b, thr)
        assert cnt[s] == len(ref), (group, s, cnt[s], len(ref))
        assert np.array_equal(keep[s, :cnt[s]], ref), (group, s)
    if group == "pair_above":
        assert cnt.tolist() == [2]
    if group == "chains":
        assert cnt.tolist() == [32, 33, 100]


def test_nms_workspace_and_tails(hip, nms_groups):
    """through the C ABI: whatever the mask workspace held before (0xFF bytes, zeros), the kept lists and counts are the
    same ("lower words are never read" holds), and `keep` stays untouched behind the count"""
    max_n, thr, segs = nms_groups["random"]
    boxes, off = _segments(segs)
    B, words = len(segs), (max_n + 63) // 64
    b_d, o_d = dev(boxes), dev(off)
    res = []
    for fill in (-1, 0):
        ws = torch.full((B * max_n * words,), fill, dtype=torch.int64, device="cuda")
        keep = torch.full((B, max_n), -1, dtype=torch.int32, device="cuda")
        cnt = torch.zeros((B,), dtype=torch.int32, device="cuda")
        rc = hip.lib().mmt_nms_batched(b_d.data_ptr(), o_d.data_ptr(), B, max_n, thr, ws.data_ptr(), keep.data_ptr(),
                                       cnt.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        res.append((host(keep), host(cnt)))
    (k1, c1), (k0, c0) = res
    assert np.array_equal(c1, c0) and np.array_equal(k1, k0)
    for s, b in enumerate(segs):
        ref = se.nms_ref(b, thr)
        assert c1[s] == len(ref) and np.array_equal(k1[s, :c1[s]], ref)
        assert (k1[s, c1[s]:] == -1).all()


def test_nms_limit(hip):
    """more than 64 mask words are refused before any launch; `_C.nms` raises instead of returning a truncated list"""
    from maskrcnn_benchmark import _C
    b = dev(se.random_boxes(4097, 1))
    off = dev(np.asarray([0, 4097], np.int32))
    with pytest.raises(RuntimeError, match=EINVAL):
        hip.nms_batched(b, off, 4097, 0.5)
    with pytest.raises(RuntimeError, match=EINVAL):
        _C.nms(b, torch.arange(4097, 0, -1, device="cuda").float(), 0.5)


# ================================================================================================================== top-k
def _head(lg, H, W, A):
    """[N, H*W*A] logits -> fused head output (N, 5A, H, W) with NHWC memory, as tests/test_select_gpu.py::_heads"""
    N = lg.shape[0]
    t = torch.from_numpy(np.ascontiguousarray(lg)).view(N, H, W, A)
    return torch.cat([t, torch.zeros(N, H, W, 4 * A)], 3).permute(0, 3, 1, 2).cuda()


def _check_topk(got, lg, k):
    got = host(got)
    assert got.shape == (lg.shape[0], k)
    for n in range(lg.shape[0]):
        assert np.array_equal(got[n], se.topk_ref(lg[n], k)), n


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("A", [1, 3])
def test_topk_small_levels(hip, A, N):
    """levels smaller than k (1 and 2 keys), exactly one 8192-key chunk, one key more than a chunk; L = 8 and L = 1;
    k = 1, 7, 2000 and the largest accepted 2048; logits on a grid of 1/8, so the cut falls among equal values"""
    sizes = se.TOPK_LEVELS[A]
    lgs = [se.topk_logits(N, h * w * A, 10 * l + A) for l, (h, w) in enumerate(sizes * 2)]
    heads = [_head(lg, h, w, A) for lg, (h, w) in zip(lgs, sizes * 2)]
    for k in se.TOPK_KS:
        ks = [min(k, lg.shape[1]) for lg in lgs]
        got = hip.rpn_topk(heads, ks, A)
        assert len(got) == 8
        for g, lg, kk in zip(got, lgs, ks):
            _check_topk(g, lg, kk)
        for l in range(4):
            _check_topk(hip.rpn_topk([heads[l]], [ks[l]], A)[0], lgs[l], ks[l])
    with pytest.raises(RuntimeError, match=EINVAL):
        hip.rpn_topk([heads[3]], [2049], A)


def test_topk_at_the_candidate_cap(hip):
    """4096 candidates (the sort path, full) and 4097 (the exact 64-bit path) on the 40 x 40 x 3 level, k = 2000"""
    lg = np.stack([se.topk_tie_case(4096), se.topk_tie_case(4097)])
    _check_topk(hip.rpn_topk([_head(lg, 40, 40, 3)], [2000], 3)[0], lg, 2000)


def test_topk_special_values(hip):
    lg = se.topk_special_segments()
    got = host(hip.rpn_topk([_head(lg, 40, 40, 3)], [2000], 3)[0])
    for n in (0, 1):
        assert np.array_equal(got[n], se.topk_ref(lg[n], 2000)), n
    assert np.array_equal(got[1], np.arange(2000))            # all -inf: the first k indices
    # both zeros: equal values, the order between them is open -- values, distinct indices, in range
    assert got[2].min() >= 0 and got[2].max() < 4800 and len(np.unique(got[2])) == 2000
    assert np.array_equal(lg[2][got[2]], lg[2][se.topk_ref(lg[2], 2000)])


# ================================================================================================================ sampler
@pytest.fixture(params=[True, False], ids=["wide", "one-block"])
def sampler_form(request, hip):
    old = (hip.SAMPLE_WIDE, hip.SAMPLE_WIDE_MIN)
    hip.SAMPLE_WIDE, hip.SAMPLE_WIDE_MIN = request.param, 1
    yield request.param
    hip.SAMPLE_WIDE, hip.SAMPLE_WIDE_MIN = old


def _check_sampler(hip, imgs, batch, max_pos):
    labels = np.concatenate([l for l, _ in imgs])
    keys = np.concatenate([k for _, k in imgs]).astype(np.float32)
    off = np.concatenate([[0], np.cumsum([len(l) for l, _ in imgs])]).astype(np.int32)
    pm, nm, cnt = hip.sample_fg_bg(dev(labels), dev(keys), dev(off), batch, max_pos)
    pm, nm, cnt = host(pm), host(nm), host(cnt)
    for i, (l, k) in enumerate(imgs):
        rp, rn, rc = se.sample_ref(l, k, batch, max_pos)
        assert cnt[i].tolist() == list(rc), (i, cnt[i], rc)
        assert np.array_equal(pm[off[i]:off[i + 1]], rp), i
        assert np.array_equal(nm[off[i]:off[i + 1]], rn), i


@pytest.mark.parametrize("member_is_pos", [True, False], ids=["pos", "neg"])
@pytest.mark.parametrize("kind", se.SAMPLER_TAU_KINDS)
def test_sampler_threshold_paths(hip, sampler_form, kind, member_is_pos):
    """members below tau: exactly num (the atomicMin path), num - 1 and 4097 (the select over the whole vector), 4096 (the
    list, full), and a key equal to tau (not below it); keys on a grid of 1/16, a crowd of them at tau"""
    labels, keys, batch, max_pos, _ = se.sampler_tau_case(kind, member_is_pos)
    _check_sampler(hip, [(labels, keys)], batch, max_pos)
    _check_sampler(hip, [(labels[:40], keys[:40]), (labels, keys), (labels[:0], keys[:0]), (labels, keys)], batch, max_pos)


@pytest.mark.parametrize("float_labels", [False, True], ids=["int64", "float"])
def test_sampler_ragged_images_and_quotas(hip, sampler_form, float_labels):
    """images of length 0, 1 and 2, an empty one between two others, one all ignored, one wide-form chunk and one label
    more; max_pos = 0, batch < max_pos, more positives than max_pos with fewer negatives than the rest of the batch; float
    labels 2.0, 0.5 (ignored) and -0.0 (negative); equal keys everywhere"""
    imgs = se.sampler_images(float_labels)
    for batch, max_pos in se.SAMPLER_QUOTAS:
        _check_sampler(hip, imgs, batch, max_pos)


def _many_images(n):
    r = np.random.RandomState(n)
    return [(r.choice([-1, 0, 0, 1], 10 + i).astype(np.int64), (r.randint(0, 16, 10 + i) / 16.0).astype(np.float32)) for i in range(n)]


def test_sampler_64_images(hip, sampler_form):
    _check_sampler(hip, _many_images(64), 8, 3)


def test_sampler_65_images(hip):
    """the wide entry point refuses 65 images before any launch; the binding takes the one-block form"""
    imgs = _many_images(65)
    labels = dev(np.concatenate([l for l, _ in imgs]))
    keys = dev(np.concatenate([k for _, k in imgs]))
    off = dev(np.concatenate([[0], np.cumsum([len(l) for l, _ in imgs])]).astype(np.int32))
    pm = torch.zeros(labels.shape, dtype=torch.uint8, device="cuda")
    nm = torch.zeros(labels.shape, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros((65, 2), dtype=torch.int32, device="cuda")
    ws = torch.zeros((hip._sample_ws_bytes(65) // 8,), dtype=torch.int64, device="cuda")
    rc = hip.lib().mmt_sample_fg_bg_wide(labels.data_ptr(), 0, keys.data_ptr(), off.data_ptr(), 65, labels.numel(), 8, 3,
                                         pm.data_ptr(), nm.data_ptr(), cnt.data_ptr(), ws.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
    assert rc == -22
    old = (hip.SAMPLE_WIDE, hip.SAMPLE_WIDE_MIN)
    hip.SAMPLE_WIDE, hip.SAMPLE_WIDE_MIN = True, 1
    try:
        _check_sampler(hip, imgs, 8, 3)
    finally:
        hip.SAMPLE_WIDE, hip.SAMPLE_WIDE_MIN = old


# ============================================================================================================ post-select
def _post(hip, c, post_n, fpn, training, cap, gt=None, gt_off=None, msf=False, zero_tails=False):
    out = hip.rpn_post_select(dev(c["boxes"]), dev(c["scores"]), dev(c["idx"]), dev(c["reg"]), dev(c["keep"]),
                              dev(c["keep_cnt"]), c["level_off"], c["own_pre"], post_n, fpn, training, cap,
                              None if gt is None else dev(gt), None if gt_off is None else dev(gt_off),
                              min_size_filter=msf, zero_tails=zero_tails)
    return [host(o) for o in out]


def _check_post(hip, c, post_n, fpn, training, gt=None, gt_off=None, msf=False, zero_tails=False, cap=None):
    kmax = c["kmax"]
    post = post_n if 0 < post_n < kmax else kmax
    ng = [0] * c["N"] if gt is None else np.diff(gt_off).tolist()
    if cap is None:
        cap = min(fpn, c["L"] * post) + max(ng)
    ob, osc, oi, orr, ol, oc = _post(hip, c, post_n, fpn, training, cap, gt, gt_off, msf, zero_tails)
    ref = se.post_select_ref(c["scores"], c["keep"], c["keep_cnt"], c["level_off"], c["own_pre"], post_n, fpn, training, msf)
    for n in range(c["N"]):
        pos = np.asarray([p for p, _ in ref[n]], np.int64)
        k = len(pos)
        assert oc[n] == k + ng[n], (n, oc[n], k, ng[n])
        assert np.array_equal(ob[n, :k], c["boxes"][n][pos]) and np.array_equal(osc[n, :k], c["scores"][n][pos]), n
        assert np.array_equal(oi[n, :k], c["idx"][n][pos]) and np.array_equal(orr[n, :k], c["reg"][n][pos]), n
        assert np.array_equal(ol[n, :k], np.asarray([l for _, l in ref[n]], np.int32)), n
        if ng[n]:
            g = slice(k, k + ng[n])
            assert np.array_equal(ob[n, g], gt[gt_off[n]:gt_off[n + 1]]) and (osc[n, g] == 1).all()
            assert (oi[n, g] == -1).all() and (orr[n, g] == 0).all() and (ol[n, g] == -1).all()
        if zero_tails:
            assert not ob[n, oc[n]:].any() and not osc[n, oc[n]:].any()
    return ref, oc


@pytest.fixture(scope="module")
def post_big():
    """N = 8, L = 8 (all 64 entries of bad_rank): segments with nothing kept, image 3 with nothing kept at all, own_pre
    below some kept positions"""
    sizes = [20, 16, 12, 8, 30, 5, 3, 1]
    r = np.random.RandomState(77)
    cnt = r.randint(0, 17, 64)
    cnt[::7] = 0
    cnt[24:32] = 0
    c = se.post_case(8, 8, 16, sizes, 70, cnt=cnt.tolist())
    c["own_pre"] = [20, 8, 12, 4, 15, 5, 1, 1]
    return c


@pytest.mark.parametrize("post_n,fpn", [(0, 10000), (5, 40), (16, 1), (40, 25), (5, 10000)])
def test_post_select_training(hip, post_big, post_n, fpn):
    """post_n = 0 and post_n >= kmax (no per-level cut), fpn_post_n = 1, cuts inside equal scores; ground truth appended,
    image 1 without any; rows behind the counts zero with zero_tails"""
    c = post_big
    beyond = sum(int((c["keep"][s, :c["keep_cnt"][s]] >= c["own_pre"][s % 8]).sum()) for s in range(64))
    assert beyond > 20                                          # kept positions outside this selector's own prefix
    gt, gt_off = se.post_gt(8)
    assert gt_off[1] == gt_off[2]
    ref, oc = _check_post(hip, c, post_n, fpn, True, gt, gt_off, zero_tails=True)
    assert oc[3] == gt_off[4] - gt_off[3] and len(ref[3]) == 0
    assert sum(len(x) for x in ref) == min(fpn, sum(len(x) for x in ref))
    _check_post(hip, c, post_n, fpn, True)                      # and without ground truth


def test_post_select_inference_small(hip, post_big):
    for post_n, fpn in ((0, 2048), (5, 7), (16, 1)):
        _check_post(hip, post_big, post_n, fpn, False)


def test_post_select_segment_limit(hip):
    """training ranks the batch in one block with 64 per-segment slots: 65 segments are refused before the launch"""
    c = se.post_case(13, 5, 4, [4] * 5, 3)
    with pytest.raises(RuntimeError, match=EINVAL):
        _post(hip, c, 0, 100, True, 100)
    _check_post(hip, c, 0, 100, False)                          # inference: 5 segments per block


def test_post_select_tie_across_images(hip):
    c = se.post_cross_image_tie()
    ref, oc = _check_post(hip, c, c["post_n"], c["fpn_post_n"], True)
    assert oc.tolist() == [3, 2]


def test_post_select_capacity(hip):
    """cap exactly what an image can receive runs and fills every row; one less is refused before the launch"""
    c = se.post_case(2, 2, 12, [40, 30], 9)
    ref, oc = _check_post(hip, c, 8, 1000, True, cap=16)
    assert oc.tolist() == [16, 16]
    with pytest.raises(RuntimeError, match=EINVAL):
        _post(hip, c, 8, 1000, True, 15)


def test_post_select_inference_full_list(hip):
    """the inference list of 2048 with more valid entries than that in every image; 2049 is refused"""
    c = se.post_case(2, 2, 1100, [1200, 1150], 13)
    assert (c["keep_cnt"] == 1100).all()
    ref, oc = _check_post(hip, c, 0, 2048, False)
    assert oc.tolist() == [2048, 2048]
    with pytest.raises(RuntimeError, match=EINVAL):
        _post(hip, c, 0, 2049, False, 2200)


@pytest.mark.parametrize("training", [True, False], ids=["training", "inference"])
@pytest.mark.parametrize("where", [0, 4, 8, None])
def test_post_select_min_size_filter(hip, where, training):
    """the box the min-size filter removed (score -1) holds no slot: the ranks behind it move up, rank `post` comes in"""
    c = se.post_min_size_case(where)
    ref, oc = _check_post(hip, c, c["post_n"], c["fpn_post_n"], training, msf=True)
    assert oc.tolist() == [16, 16]
    assert all(c["scores"][n][p] >= 0 for n in range(2) for p, _ in ref[n])


# ============================================================================================================= detections
@pytest.fixture(scope="module")
def det_cases():
    return se.det_cases()


@pytest.mark.parametrize("name", ["2048-rows-2-classes", "64-classes", "D-1", "D-above-n", "D-tie", "chain", "nothing-above",
                                  "at-threshold", "one-row"])
def test_det_postprocess_edges(hip, det_cases, name):
    c = det_cases[name]
    out = hip.det_postprocess(dev(c["prob"]), dev(c["dec"]), c["per"], c["thresh"], c["nms"], c["D"])
    assert out is not None
    ob, osc, ol, oc = [host(o) for o in out]
    ref = se.det_ref(c["prob"], c["dec"], c["per"], c["thresh"], c["nms"], c["D"])
    for n, (bb, ss, ll) in enumerate(ref):
        k = len(ss)
        assert oc[n] == k, (name, n, oc[n], k)
        assert np.array_equal(ob[n, :k], bb) and np.array_equal(osc[n, :k], ss) and np.array_equal(ol[n, :k], ll), (name, n)
    if name == "nothing-above":
        assert not oc.any()
    if name == "D-tie":
        assert oc.tolist() == [13]                              # ties at the D-th score stay
    if name == "D-1":
        assert (oc >= 1).all()


def test_det_postprocess_row_limit(hip):
    assert hip.det_postprocess(torch.zeros(2049, 2, device="cuda"), torch.zeros(2049, 8, device="cuda"), [2049], 0.05, 0.5,
                               100) is None


# ================================================================================================================ matcher
@pytest.mark.parametrize("allow_low_quality", [True, False], ids=["low-quality", "plain"])
@pytest.mark.parametrize("shared", [False, True], ids=["per-image", "shared"])
def test_match_targets_edges(hip, shared, allow_low_quality):
    """1, 255, 256, 257 and 3 candidates per image (a block spans one, two and three images) / one shared list for three
    images; a ground-truth box that meets no candidate (with low-quality matches it restores every candidate with IoU 0
    against it, as the reference does); candidate lists that end in all-zero boxes"""
    cand, cand_off, gt, gt_off, N, cands, gts = se.match_case(shared)
    for high, low in ((0.7, 0.3), (0.5, 0.5)):
        m, _, _ = hip.match_targets(dev(cands[0] if shared else cand), dev(cand_off), dev(gt), dev(gt_off), N, high, low,
                                    allow_low_quality=allow_low_quality, shared_cand=shared)
        m = host(m)
        for i in range(N):
            ref = se.match_ref(cands[0 if shared else i], gts[i], high, low, allow_low_quality)
            assert np.array_equal(m[cand_off[i]:cand_off[i + 1]], ref), (i, high)
