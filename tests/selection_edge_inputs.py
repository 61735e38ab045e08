"""Constructed inputs and plain references for the selection family (csrc/nms.hip, csrc/select.hip, the matcher of
csrc/targets.hip): numpy on the CPU, loops and stable sorts, nothing from the product.  Whatever decides an outcome (IoU,
tau of the sampler, score comparisons) is computed in fp32 in the reference's operation order.

tests/test_selection_edge_inputs.py checks, with these references alone, that every builder reaches the code path it
names; tests/test_selection_edges_gpu.py runs the kernels on the same inputs and compares exactly."""
import numpy as np

f32 = np.float32
ONE, ZERO = f32(1), f32(0)


# =========================================================================================================== references
def iou_f32(a, b):
    """cpu/nms_cpu.cpp:22,45-57: "+1" areas, fp32, inter / (area_a + area_b - inter).  a (4,), b (4,) or (n, 4)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    aa = (a[2] - a[0] + ONE) * (a[3] - a[1] + ONE)
    ab = (b[..., 2] - b[..., 0] + ONE) * (b[..., 3] - b[..., 1] + ONE)
    xx1, yy1 = np.maximum(a[0], b[..., 0]), np.maximum(a[1], b[..., 1])
    xx2, yy2 = np.minimum(a[2], b[..., 2]), np.minimum(a[3], b[..., 3])
    w, h = np.maximum(ZERO, xx2 - xx1 + ONE), np.maximum(ZERO, yy2 - yy1 + ONE)
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (aa + ab - inter)


def nms_ref(boxes, thr):
    """greedy NMS over score-sorted boxes: box i, unless suppressed, suppresses every later j with IoU >= thr
    -> kept indices, ascending"""
    boxes = np.asarray(boxes, f32).reshape(-1, 4)
    n, thr = len(boxes), f32(thr)
    dead = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        if i + 1 < n:
            dead[i + 1:] |= iou_f32(boxes[i], boxes[i + 1:]) >= thr   # NaN >= thr is False
    return np.asarray(keep, np.int64)


def topk_ref(x, k):
    """value descending, index ascending"""
    return np.argsort(-np.asarray(x, f32), kind="stable")[:k]


def sample_ref(labels, keys, batch, max_pos):
    """one image -> pos mask, neg mask, (num_pos, num_neg): per class (labels >= 1 / labels == 0) the `num` members with
    the smallest keys, equal keys lower index first.  A quota that comes out negative (batch < num_pos) is nothing."""
    labels, keys = np.asarray(labels), np.asarray(keys, f32)
    out = []
    pos, neg = np.nonzero(labels >= 1)[0], np.nonzero(labels == 0)[0]
    num_pos = min(len(pos), max_pos)
    num_neg = max(0, min(len(neg), batch - num_pos))
    for members, num in ((pos, num_pos), (neg, num_neg)):
        m = np.zeros(len(labels), bool)
        m[members[np.argsort(keys[members], kind="stable")][:num]] = True
        out.append(m)
    return out[0], out[1], (num_pos, num_neg)


def sampler_tau(num, members):
    """the pre-filter of sample_kernel: fminf(1, 8.0f * (float)num / (float)members)"""
    return min(ONE, f32(8) * f32(num) / f32(members))


def post_entries(scores, keep, keep_cnt, level_off, own_pre, post_n, min_size_filter):
    """valid entries of rpn_post_kernel in (image, level, rank) order -> list of (image, level, rank, pos, score).
    rank < keep count; the FIRST kept box of a segment with a negative score (removed by the min-size filter) holds no
    slot, so the ranks behind it move up by one; slot < post (the per-level cut); position inside own_pre[level]."""
    N, L, kmax = scores.shape[0], len(level_off) - 1, keep.shape[1]
    post = post_n if 0 < post_n < kmax else kmax
    out = []
    for n in range(N):
        for l in range(L):
            seg, slot, removed = n * L + l, 0, False
            for j in range(min(int(keep_cnt[seg]), kmax)):
                p = int(keep[seg, j])
                s = scores[n, level_off[l] + p]
                if min_size_filter and not removed and s < 0:
                    removed = True
                    continue
                if slot >= post:
                    break
                slot += 1
                if p < own_pre[l]:
                    out.append((n, l, j, level_off[l] + p, s))
    return out


def post_select_ref(scores, keep, keep_cnt, level_off, own_pre, post_n, fpn_post_n, training, min_size_filter=False):
    """-> per image: list of (pos, level) in output order.  The best fpn_post_n entries by (score descending, entry
    order ascending): over the whole batch and emitted in entry order (training), or per image and emitted in that
    descending order (inference).  Ground truth is appended by the caller."""
    N = scores.shape[0]
    ent = post_entries(scores, keep, keep_cnt, level_off, own_pre, post_n, min_size_filter)
    sc = np.asarray([e[4] for e in ent], f32)
    img = np.asarray([e[0] for e in ent], np.int64)
    out = []
    if training:
        sel = np.zeros(len(ent), bool)
        sel[np.argsort(-sc, kind="stable")[:fpn_post_n]] = True
        for n in range(N):
            out.append([(ent[i][3], ent[i][1]) for i in np.nonzero(sel & (img == n))[0]])
    else:
        for n in range(N):
            mine = np.nonzero(img == n)[0]
            order = mine[np.argsort(-sc[mine], kind="stable")[:fpn_post_n]]
            out.append([(ent[i][3], ent[i][1]) for i in order])
    return out


def det_survivors(prob, dec, per, thresh, nms_thr):
    """filter_results before the DETECTIONS_PER_IMG cut -> per image (boxes, scores, labels): per foreground class the
    rows with prob > thresh in stable descending score order through nms_ref, survivors in ascending row order"""
    prob, dec = np.asarray(prob, f32), np.asarray(dec, f32)
    nc, out, r0 = prob.shape[1], [], 0
    for R in per:
        bb, ss, ll = [np.zeros((0, 4), f32)], [np.zeros(0, f32)], [np.zeros(0, np.int64)]
        for j in range(1, nc):
            sc = prob[r0:r0 + R, j]
            rows = np.nonzero(sc > f32(thresh))[0]
            rows = rows[np.argsort(-sc[rows], kind="stable")]
            bx = dec[r0 + rows, 4 * j:4 * j + 4]
            kept = np.sort(rows[nms_ref(bx, nms_thr)])
            bb.append(dec[r0 + kept, 4 * j:4 * j + 4])
            ss.append(sc[kept])
            ll.append(np.full(len(kept), j, np.int64))
        out.append((np.concatenate(bb), np.concatenate(ss), np.concatenate(ll)))
        r0 += R
    return out


def det_ref(prob, dec, per, thresh, nms_thr, D):
    """filter_results: det_survivors, then with more than D > 0 of them every one whose score >= the D-th largest"""
    out = []
    for bb, ss, ll in det_survivors(prob, dec, per, thresh, nms_thr):
        if len(ss) > D > 0:
            k = ss >= np.sort(ss)[len(ss) - D]
            bb, ss, ll = bb[k], ss[k], ll[k]
        out.append((bb, ss, ll))
    return out


def iou_matrix(gt, cand):
    """boxlist_iou in fp32: [G, A], inter / (area_gt + area_cand - inter) with "+1" sides"""
    gt, cand = np.asarray(gt, f32).reshape(-1, 4), np.asarray(cand, f32).reshape(-1, 4)
    ga = (gt[:, 2] - gt[:, 0] + ONE) * (gt[:, 3] - gt[:, 1] + ONE)
    ca = (cand[:, 2] - cand[:, 0] + ONE) * (cand[:, 3] - cand[:, 1] + ONE)
    lt = np.maximum(gt[:, None, :2], cand[None, :, :2])
    rb = np.minimum(gt[:, None, 2:], cand[None, :, 2:])
    wh = np.maximum(rb - lt + ONE, ZERO)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (ga[:, None] + ca[None, :] - inter)


def match_ref(cand, gt, high, low, allow_low_quality):
    """Matcher of one image: first arg-max over the ground truth, -1 below `low`, -2 between, and with
    allow_low_quality every candidate that attains some ground-truth box's best IoU gets its arg-max back -- also where
    that best IoU is 0 (a ground-truth box that overlaps nothing restores every candidate with IoU 0 against it)"""
    mq = iou_matrix(gt, cand)
    vals, arg = mq.max(0), mq.argmax(0)
    m = arg.astype(np.int32).copy()
    m[vals < f32(low)] = -1
    m[(vals >= f32(low)) & (vals < f32(high))] = -2
    if allow_low_quality:
        upd = (mq == mq.max(1)[:, None]).any(0)
        m[upd] = arg[upd]
    return m


# ============================================================================================================ NMS inputs
def chain(n):
    """box i suppresses only box i + 1 at thr 0.5: IoU(i, i+1) = 2/3, IoU(i, i+2) = 3/7"""
    i = np.arange(n, dtype=f32)
    return np.stack([2 * i, 0 * i, 2 * i + 9, 0 * i + 9], 1).astype(f32)


def random_boxes(n, seed):
    """boxes of 16..48 px thrown onto a field that grows with n, so that the kept share stays away from 0 and 1"""
    r = np.random.RandomState(seed)
    side = max(1.0, np.sqrt(n) * 7.0)
    xy = np.floor(r.rand(n, 2) * side)
    wh = np.floor(r.rand(n, 2) * 32 + 16)
    return np.concatenate([xy, xy + wh], 1).astype(f32)


def grid_4096():
    """64 x 64 disjoint 10 x 10 boxes; the last is a copy of the first: chunk 0 sets the last bit of word 63"""
    i = np.arange(4096)
    x, y = (i % 64) * 20.0, (i // 64) * 20.0
    b = np.stack([x, y, x + 9, y + 9], 1).astype(f32)
    b[4095] = b[0]
    return b


def degenerate_mix():
    """x2 = x1 - 1 boxes (area 0, IoU NaN against themselves) between normal ones, some of them repeated"""
    r = np.random.RandomState(7)
    b = random_boxes(150, 8)
    for i in range(3, 150, 5):
        x, y = np.floor(r.rand(2) * 100)
        b[i] = (x, y, x - 1, y - 1)
    b[40:50] = b[30:40]
    b[23] = b[18] = b[13]
    return b


RANDOM_NS = (0, 1, 63, 64, 65, 127, 128, 129, 4095, 4096)
THR_UP = float(np.nextafter(f32(0.5), f32(1)))
EXACT_PAIR = np.asarray([[0, 0, 9, 9], [0, 0, 9, 4]], f32)    # IoU exactly 0.5


def nms_groups():
    """name -> (max_n, thr, [boxes per segment]); one batched call each"""
    return {
        "chains": (256, 0.5, [chain(64), chain(65), chain(200)]),
        "grid": (4096, 0.5, [grid_4096()]),
        "special": (4096, 0.5, [np.tile(np.asarray([[3, 4, 40, 50]], f32), (4096, 1)), np.zeros((100, 4), f32), EXACT_PAIR,
                                degenerate_mix()]),
        "pair_above": (64, THR_UP, [EXACT_PAIR]),
        "random": (4096, 0.5, [random_boxes(n, 100 + n) for n in RANDOM_NS]),
    }


# ========================================================================================================== top-k inputs
TOPK_LEVELS = {1: [(1, 1), (1, 2), (64, 128), (3, 2731)], 3: [(1, 1), (3, 5), (16, 16), (40, 40)]}
TOPK_KS = (1, 7, 2000, 2048)


def topk_logits(N, n, seed):
    """[N, n] logits on a grid of 1/8: every value many times once n is large"""
    r = np.random.RandomState(seed)
    return (np.round(r.randn(N, n) * 3.0 * 8) / 8).astype(f32) + ZERO   # (+ 0: the rounding leaves no -0.0 behind)


def topk_tie_case(candidates, seed=5):
    """4800 logits (the 40 x 40 x 3 level), k = 2000: 100 distinct values above one value held `candidates - 100` times,
    distinct values below -> exactly `candidates` keys are >= the k-th largest"""
    n, r = 4800, np.random.RandomState(seed)
    v = np.concatenate([2.0 + np.arange(100) / 128.0, np.full(candidates - 100, 0.75),
                        -1.0 - np.arange(n - candidates) / 128.0]).astype(f32)
    return v[r.permutation(n)]


def topk_special_segments():
    """[3, 4800]: infinities, denormals and +-3e38 among ordinary values; all -inf; both zeros (the last one is compared
    by value, see the GPU test)"""
    n, r = 4800, np.random.RandomState(9)
    a = (np.round(r.randn(n) * 64) / 16).astype(f32) + ZERO
    a[r.permutation(n)[:60]] = np.tile(np.asarray([np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -1e-39, 3e38, -3e38, 1.1754942e-38,
                                                   -1.1754942e-38], f32), 6)
    b = np.full(n, -np.inf, f32)
    c = (np.round(r.randn(n) * 2) / 2).astype(f32) + ZERO     # ~ 950 zeros, all +0.0 ...
    c[(c == 0) & (np.arange(n) % 2 == 1)] = f32(-0.0)         # ... and every other one of them -0.0
    return np.stack([a, b, c])


# ========================================================================================================= sampler inputs
def _quantised_keys(r, n, lo, hi):
    """multiples of 1/16 in [lo, hi)"""
    return (r.randint(int(lo * 16), int(hi * 16), n) / 16.0).astype(f32)


def sampler_tau_case(kind, member_is_pos, seed=0):
    """one image whose sampled class has `members` members and a quota `num` with tau = 8 num / members = 0.5 exactly, and
    exactly `below` members under tau.  kind: "num", "num-1", "4096", "4097", "at-tau" (below = num and one key == tau).
    The other labels are ignored ones and a few of the other class, with small keys that must not count.
    -> labels int64, keys, batch, max_pos, (members, num, below)"""
    r = np.random.RandomState(seed + len(kind))
    num, members = (256, 4096) if kind in ("num", "num-1", "at-tau") else (1024, 16384)
    below = {"num": num, "num-1": num - 1, "4096": 4096, "4097": 4097, "at-tau": num}[kind]
    n = members + 1000
    is_member = np.zeros(n, bool)
    is_member[r.permutation(n)[:members]] = True
    keys = _quantised_keys(r, n, 0.0, 0.5)                       # non-members: all below tau
    mk = _quantised_keys(r, members, 0.5625, 1.0)                # members: above tau ...
    mk[r.permutation(members)[:below]] = _quantised_keys(r, below, 0.0, 0.5)   # ... but `below` of them
    if kind == "at-tau":
        mk[np.nonzero(mk > 0.5)[0][:1]] = 0.5
    else:
        hi = np.nonzero(mk > 0.5)[0]
        mk[hi[:len(hi) // 8]] = 0.5                              # and in the other cases a crowd AT tau
    keys[is_member] = mk
    other = np.where(np.arange(n) % 3 == 0, -1, 0 if member_is_pos else 1)
    labels = np.where(is_member, 2 if member_is_pos else 0, other).astype(np.int64)
    if member_is_pos:
        batch, max_pos = num, num                                # no negatives are drawn
    else:
        n_other = int((labels >= 1).sum())
        batch, max_pos = num + n_other, n_other                  # every positive, then `num` negatives
    return labels, keys, batch, max_pos, (members, num, below)


SAMPLER_TAU_KINDS = ("num", "num-1", "4096", "4097", "at-tau")


def sampler_images(float_labels, seed=3):
    """ragged images with keys on a grid of 1/16 -> list of (labels, keys): lengths 0, 1 and 2, an empty image between
    two others, an all-ignored image, one wide-form chunk exactly and one element more, many positives with few negatives"""
    r = np.random.RandomState(seed)
    out = []
    for n in (5, 0, 7, 1, 2, 0, 50, 16384, 16385, 300, 1, 40):
        lab = r.choice([-1, 0, 0, 0, 1, 2], n).astype(np.int64)
        out.append([lab, _quantised_keys(r, n, 0.0, 1.0)])
    out[6][0][:] = -1                                            # all ignored
    out[9][0][:] = np.where(np.arange(300) < 280, 1, np.where(np.arange(300) < 290, 0, -1))   # 280 positives, 10 negatives
    out[10][0][:] = 1
    if float_labels:
        for o in out:
            lab = o[0].astype(f32)
            lab[o[0] == -1] = np.where(np.arange((o[0] == -1).sum()) % 2 == 0, 0.5, -1.0)     # 0.5 is ignored too
            lab[o[0] == 0] = np.where(np.arange((o[0] == 0).sum()) % 2 == 0, -0.0, 0.0)       # -0.0 is a negative
            o[0] = lab
    return [tuple(o) for o in out]


SAMPLER_QUOTAS = ((256, 128), (64, 0), (4, 16), (300, 128), (1, 1))   # (batch, max_pos): usual, no positives wanted, batch < max_pos


# ===================================================================================================== post-select inputs
def post_case(N, L, kmax, sizes, seed, cnt=None, tie_free=False):
    """synthetic NMS output: per segment an ascending list of kept positions inside its level (as the sweep emits them),
    scores on a grid of 1/64 in (0, 1) (ties) -> dict"""
    r = np.random.RandomState(seed)
    level_off = [0]
    for s in sizes:
        level_off.append(level_off[-1] + s)
    sumk = level_off[-1]
    if tie_free:
        scores = np.stack([(r.permutation(sumk) + 1.0) / (sumk + 1.0) for _ in range(N)]).astype(f32)
    else:
        scores = (r.randint(1, 64, (N, sumk)) / 64.0).astype(f32)
    keep = np.full((N * L, kmax), -1, np.int32)
    keep_cnt = np.zeros(N * L, np.int32)
    for seg in range(N * L):
        s = sizes[seg % L]
        c = min(kmax, s) if cnt is None else min(cnt[seg], kmax, s)
        keep_cnt[seg] = c
        keep[seg, :c] = np.sort(r.permutation(s)[:c])
    boxes = (np.arange(N * sumk * 4).reshape(N, sumk, 4) % 977).astype(f32)
    idx = (np.arange(N * sumk).reshape(N, sumk) * 7 + 1).astype(np.int64)
    reg = (np.arange(N * sumk * 4).reshape(N, sumk, 4) % 31).astype(f32) / 8 - 2
    return dict(N=N, L=L, kmax=kmax, level_off=level_off, scores=scores, keep=keep, keep_cnt=keep_cnt, boxes=boxes, idx=idx,
                reg=reg, own_pre=list(sizes))


def post_cross_image_tie():
    """two images, one level, fpn_post_n = 5: 0.9 and 0.8 first, then five entries of 0.5 -- two in image 0, three in
    image 1 -- of which the cut takes three: both of image 0, the first of image 1"""
    c = post_case(2, 1, 6, [6], 1)
    c["scores"] = np.asarray([[0.9, 0.5, 0.25, 0.5, 0.125, 0.0625], [0.5, 0.8, 0.5, 0.125, 0.5, 0.0625]], f32)
    c["keep"] = np.tile(np.arange(6, dtype=np.int32), (2, 1))
    c["keep_cnt"] = np.asarray([6, 6], np.int32)
    c["post_n"], c["fpn_post_n"] = 0, 5
    return c


def post_min_size_case(where):
    """N = 2, L = 2, kmax = 12, post_n = 8: in segment (image 0, level 1) the box at rank `where` was removed by the
    min-size filter (score -1).  where: 0, 4 (middle), 8 (= post, the look-ahead rank) or None"""
    c = post_case(2, 2, 12, [40, 30], 21, tie_free=True)
    c["post_n"], c["fpn_post_n"], c["removed_rank"] = 8, 1000, where
    if where is not None:
        c["scores"][0, c["level_off"][1] + c["keep"][1, where]] = -1.0
    return c


def post_gt(N, seed=2, empty=1):
    """ground truth of N images, image `empty` has none -> gt [G, 4], gt_off [N + 1]"""
    r = np.random.RandomState(seed)
    cnt = [0 if n == empty else 1 + (n * 5) % 4 for n in range(N)]
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    gt = np.floor(r.rand(off[-1], 4) * 300).astype(f32)
    gt[:, 2:] += gt[:, :2]
    return gt, off


# ======================================================================================================= detection inputs
def _det_boxes(r, R, nc, spread):
    xy = np.floor(r.rand(R, nc, 2) * spread)
    wh = np.floor(r.rand(R, nc, 2) * 40 + 10)
    return np.concatenate([xy, xy + wh], 2).reshape(R, nc * 4).astype(f32)


def det_cases():
    """name -> dict(prob [R, nc], dec [R, nc * 4], per, thresh, nms, D, binds: the cut is meant to bind)"""
    r = np.random.RandomState(31)
    out = {}

    def add(name, per, nc, D, thresh=0.05, spread=400.0, binds=False, prob=None, dec=None):
        R = sum(per)
        p = (r.randint(0, 257, (R, nc)) / 256.0).astype(f32) if prob is None else prob    # a grid of 1/256: ties
        out[name] = dict(prob=p, dec=_det_boxes(r, R, nc, spread) if dec is None else dec, per=per, thresh=thresh, nms=0.5,
                         D=D, binds=binds)

    add("2048-rows-2-classes", [2048, 1], 2, 100, spread=1500.0, binds=True,
        prob=((r.permutation(2049 * 2) + 1000.0) / 8192.0).reshape(2049, 2).astype(f32))
    add("64-classes", [5], 64, 100)
    add("D-1", [30, 20], 3, 1, binds=True)
    add("D-above-n", [30, 20], 3, 1000)
    # 80 disjoint candidates: 8 distinct scores on top, then five of 0.75 around the D = 10-th place, the rest below
    pt = np.zeros((40, 3), f32)
    v = np.concatenate([0.8 + np.arange(8) / 64.0, np.full(5, 0.75), 0.25 + np.arange(67) / 256.0]).astype(f32)
    pt[:, 1:] = v[r.permutation(80)].reshape(40, 2)
    i = np.arange(40 * 3, dtype=f32) * 60
    dt = np.stack([i, 0 * i, i + 20, 0 * i + 20], 1).reshape(40, 12).astype(f32)
    add("D-tie", [40], 3, 10, binds=True, prob=pt, dec=dt)
    ch = np.zeros((70, 8), f32)
    ch[:, 4:] = chain(70)
    pc = np.zeros((70, 2), f32)
    pc[:, 1] = 0.9 - np.arange(70) / 128.0
    add("chain", [70], 2, 100, prob=pc, dec=ch)
    add("nothing-above", [20, 10, 3], 4, 10, thresh=1.0)
    pe = (r.randint(0, 8, (60, 3)) / 8.0).astype(f32)
    add("at-threshold", [60], 3, 100, thresh=0.5, prob=pe)
    add("one-row", [1], 3, 100)
    return out


# ========================================================================================================= matcher inputs
MATCH_COUNTS = (1, 255, 256, 257, 3)        # candidates per image: one 256-thread block spans one, two and three images


def match_case(shared, seed=41):
    """-> cand, cand_off, gt, gt_off, n_images, per-image candidate lists, per-image ground truth.  Every image has one
    ground-truth box far from every candidate and one that is there twice (the first of two equal maxima is the match), met
    exactly by one candidate; every candidate list ends in all-zero boxes (fixed-capacity tails); shared: one list of 300
    for three images"""
    r = np.random.RandomState(seed)
    counts = (300,) * 3 if shared else MATCH_COUNTS

    def boxes(n, lo, span):
        xy = np.floor(r.rand(n, 2) * span) + lo
        wh = np.floor(r.rand(n, 2) * 60 + 8)
        return np.concatenate([xy, xy + wh], 1).astype(f32)

    cands = []
    for n in (counts[:1] if shared else counts):
        c = boxes(n, 20, 200)
        if n >= 3:
            c[-max(1, n // 8):] = 0
        cands.append(c)
    gts = []
    for i in range(len(counts)):
        g = boxes(2 + i % 3, 20, 200)
        g[(i + 1) % 2] = (5000, 5000, 5050, 5040)               # overlaps nothing
        if len(g) > 2:
            g[2] = cands[0 if shared else i][0]                  # and one that some candidate meets exactly
        g = np.concatenate([g, g[i % 2][None]])                  # the other random one a second time, at the end
        c = cands[0 if shared else i]
        if len(c) >= 3:
            c[1 + i if shared else 1] = g[i % 2]
        gts.append(g)
    cand_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    gt_off = np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int32)
    return np.concatenate(cands), cand_off, np.concatenate(gts), gt_off, len(counts), cands, gts
