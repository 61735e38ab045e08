"""The inputs of tests/test_selection_edges_gpu.py against the plain references alone (no GPU): a chain that did not
chain, a tie case whose cut fell beside the tie or a sampler case on the wrong side of a threshold path would compare
equal whatever the kernel did in the path it was built for."""
import numpy as np
import pytest
import torch

import selection_edge_inputs as se

f32 = np.float32


@pytest.fixture(scope="module")
def nms_groups():
    return se.nms_groups()


def test_chain_suppresses_only_its_successor():
    b = se.chain(200)
    assert se.iou_f32(b[0], b[1]) == f32(2) / f32(3) and se.iou_f32(b[7], b[9]) == f32(3) / f32(7)
    for n in (64, 65, 200):
        assert se.nms_ref(se.chain(n), 0.5).tolist() == list(range(0, n, 2))
    assert len(se.nms_ref(b, 0.5)) == 100


def test_iou_special_values():
    assert se.iou_f32(se.EXACT_PAIR[0], se.EXACT_PAIR[1]) == f32(0.5)
    assert np.isnan(se.iou_f32([5, 5, 4, 4], [5, 5, 4, 4]))
    assert se.iou_f32([0, 0, 0, 0], [0, 0, 0, 0]) == f32(1)
    assert se.nms_ref(se.EXACT_PAIR, 0.5).tolist() == [0] and se.nms_ref(se.EXACT_PAIR, se.THR_UP).tolist() == [0, 1]
    assert f32(se.THR_UP) > f32(0.5) and f32(se.THR_UP) == se.THR_UP


def test_nms_ref_is_the_oracles_nms(nms_groups):
    from oracle import native
    for name, (max_n, thr, segs) in nms_groups.items():
        for b in segs:
            assert len(b) <= max_n
            scores = torch.arange(len(b), 0, -1).float()
            got = native.nms(torch.from_numpy(b), scores, thr).numpy()
            assert np.array_equal(got, se.nms_ref(b, thr)), (name, len(b))


def test_nms_cases_keep_what_they_claim(nms_groups):
    assert len(se.nms_ref(nms_groups["grid"][2][0], 0.5)) == 4095
    ident, zeros, pair, deg = nms_groups["special"][2]
    assert len(ident) == 4096 and len(se.nms_ref(ident, 0.5)) == 1
    assert len(zeros) == 100 and len(se.nms_ref(zeros, 0.5)) == 1
    assert len(se.nms_ref(pair, 0.5)) == 1
    flat = deg[:, 2] == deg[:, 0] - 1
    kept = se.nms_ref(deg, 0.5)
    assert flat.sum() >= 20 and flat[kept].sum() == flat.sum() and 0 < (~flat)[kept].sum() < (~flat).sum()
    assert [len(b) for b in nms_groups["random"][2]] == list(se.RANDOM_NS)
    for b in nms_groups["random"][2]:
        if len(b) >= 64:
            share = len(se.nms_ref(b, 0.5)) / len(b)
            print("n=%d kept share %.3f" % (len(b), share))
            assert 0.2 < share < 0.8, (len(b), share)


@pytest.mark.parametrize("candidates", [4096, 4097])
def test_topk_tie_cases_sit_on_the_switch(candidates):
    x = se.topk_tie_case(candidates)
    assert x.shape == (4800,)
    kth = x[se.topk_ref(x, 2000)[-1]]
    assert (x >= kth).sum() == candidates


def test_topk_special_segments():
    a, b, c = se.topk_special_segments()
    assert np.isposinf(a).sum() == 6 and np.isneginf(a).sum() == 6 and not np.isnan(a).any()
    tiny = np.finfo(f32).tiny
    assert ((a != 0) & (np.abs(a) < tiny)).sum() == 36 and (np.abs(a) == f32(3e38)).sum() == 12
    assert not np.signbit(a[a == 0]).any()                       # index-exact comparison: no -0.0 in there
    assert np.isneginf(b).all()
    z = c == 0
    assert np.signbit(c[z]).sum() > 100 and (~np.signbit(c[z])).sum() > 100
    assert (c > 0).sum() < 2000 < (c >= 0).sum()                 # the cut of k = 2000 falls among the zeros
    for N in (1, 3):
        x = se.topk_logits(N, 8193, 1)
        assert not np.signbit(x[x == 0]).any() and len(np.unique(x)) < 400


@pytest.mark.parametrize("member_is_pos", [True, False])
@pytest.mark.parametrize("kind", se.SAMPLER_TAU_KINDS)
def test_sampler_cases_sit_on_their_threshold_path(kind, member_is_pos):
    labels, keys, batch, max_pos, (members, num, below) = se.sampler_tau_case(kind, member_is_pos)
    member = labels >= 1 if member_is_pos else labels == 0
    pm, nm, (num_pos, num_neg) = se.sample_ref(labels, keys, batch, max_pos)
    assert member.sum() == members and (num_pos if member_is_pos else num_neg) == num
    tau = se.sampler_tau(num, members)
    assert tau == f32(0.5)
    want = {"num": num, "num-1": num - 1, "4096": 4096, "4097": 4097, "at-tau": num}[kind]
    assert (keys[member] < tau).sum() == want == below
    assert ((keys[member] == tau).sum() == 1) if kind == "at-tau" else ((keys[member] == tau).sum() > 10)
    assert (keys[~member] < tau).sum() > 500                     # non-members below tau must not count
    assert (pm if member_is_pos else nm).sum() == num
    if kind == "at-tau":
        assert not (pm | nm)[member & (keys == tau)].any()


def test_sampler_images_cover_the_lengths():
    for fl in (False, True):
        imgs = se.sampler_images(fl)
        lens = [len(l) for l, _ in imgs]
        assert lens[:6] == [5, 0, 7, 1, 2, 0] and 16384 in lens and 16385 in lens
        assert (imgs[6][0] < 0).all() if not fl else ((imgs[6][0] < 1) & (imgs[6][0] != 0)).all()
        lab = imgs[9][0]
        assert (lab >= 1).sum() == 280 and (lab == 0).sum() == 10
        if fl:
            allv = np.concatenate([l for l, _ in imgs])
            assert (allv == f32(0.5)).any() and (allv == 2).any() and np.signbit(allv[allv == 0]).any()
        keys = np.concatenate([k for _, k in imgs])
        assert np.array_equal(keys * 16, np.round(keys * 16)) and len(np.unique(keys)) == 16


def _cut_scores(c, training=True, msf=False):
    ent = se.post_entries(c["scores"], c["keep"], c["keep_cnt"], c["level_off"], c["own_pre"], c["post_n"], msf)
    order = np.argsort(-np.asarray([e[4] for e in ent], f32), kind="stable")
    return ent, order


def test_post_select_tie_spans_two_images():
    c = se.post_cross_image_tie()
    ent, order = _cut_scores(c)
    fpn = c["fpn_post_n"]
    last_in, first_out = ent[order[fpn - 1]], ent[order[fpn]]
    assert last_in[4] == first_out[4]
    group = [e for e in ent if e[4] == last_in[4]]
    assert {e[0] for e in group} == {0, 1}
    sel = se.post_select_ref(c["scores"], c["keep"], c["keep_cnt"], c["level_off"], c["own_pre"], c["post_n"], fpn, True)
    assert [p for p, _ in sel[0]] == [0, 1, 3] and [p for p, _ in sel[1]] == [0, 1]


@pytest.mark.parametrize("where", [0, 4, 8, None])
def test_post_select_min_size_cases(where):
    c = se.post_min_size_case(where)
    post = c["post_n"]
    assert 0 < post < c["kmax"] and (c["keep_cnt"] > post).all()
    neg = [(n, int(np.searchsorted(c["level_off"], p, "right")) - 1) for n, p in zip(*np.nonzero(c["scores"] < 0))]
    assert neg == ([] if where is None else [(0, 1)])
    ent = se.post_entries(c["scores"], c["keep"], c["keep_cnt"], c["level_off"], c["own_pre"], post, True)
    ranks = [e[2] for e in ent if e[0] == 0 and e[1] == 1]
    want = {None: list(range(8)), 0: list(range(1, 9)), 4: [0, 1, 2, 3, 5, 6, 7, 8], 8: list(range(8))}[where]
    assert ranks == want


def test_detection_cases_bind_where_they_should():
    cases = se.det_cases()
    for name, c in cases.items():
        sv = se.det_survivors(c["prob"], c["dec"], c["per"], c["thresh"], c["nms"])
        n = [len(s[1]) for s in sv]
        print(name, n)
        if c["binds"]:
            assert n[0] > c["D"] > 0, (name, n)
    c = cases["2048-rows-2-classes"]
    assert (c["prob"][:2048, 1] > c["thresh"]).all() and c["prob"].shape == (2049, 2)
    c = cases["D-tie"]
    ss = np.sort(se.det_survivors(c["prob"], c["dec"], c["per"], c["thresh"], c["nms"])[0][1])[::-1]
    assert ss[c["D"] - 1] == ss[c["D"]] == ss[c["D"] - 2]
    assert len(se.det_ref(c["prob"], c["dec"], c["per"], c["thresh"], c["nms"], c["D"])[0][1]) == 13
    c = cases["chain"]
    assert se.det_ref(c["prob"], c["dec"], c["per"], c["thresh"], c["nms"], c["D"])[0][1].shape == (35,)
    c = cases["nothing-above"]
    assert all(len(s[1]) == 0 for s in se.det_ref(c["prob"], c["dec"], c["per"], c["thresh"], c["nms"], c["D"]))
    c = cases["at-threshold"]
    assert (c["prob"][:, 1:] == f32(c["thresh"])).sum() > 5
    assert cases["64-classes"]["prob"].shape == (5, 64) and cases["one-row"]["prob"].shape[0] == 1


@pytest.mark.parametrize("shared", [False, True])
def test_matcher_cases(shared):
    cand, cand_off, gt, gt_off, N, cands, gts = se.match_case(shared)
    assert np.diff(cand_off).tolist() == ([300] * 3 if shared else list(se.MATCH_COUNTS))
    restored = 0
    for i in range(N):
        c = cands[0 if shared else i]
        mq = se.iou_matrix(gts[i], c)
        assert (mq.max(1) == 0).sum() >= 1                       # a ground-truth box that meets nothing
        if len(c) >= 3:
            assert not c[-1].any()
        on = se.match_ref(c, gts[i], 0.7, 0.3, True)
        off = se.match_ref(c, gts[i], 0.7, 0.3, False)
        restored += ((on >= 0) & (off < 0) & (mq.max(0) == 0)).sum()
        assert set(np.unique(off)) <= {-2, -1} | set(range(len(gts[i])))
        if len(c) >= 3:                                          # two equal maxima above `high`: the first is the match
            twice = ((mq == mq.max(0)) & (mq >= f32(0.7))).sum(0) > 1
            assert twice.any() and (off[twice] == mq.argmax(0)[twice]).all() and (off[twice] < len(gts[i]) - 1).all()
    assert restored > 10                                         # the IoU-0 quirk is really exercised
