"""The two merge kernels of test-time augmentation (csrc/tta.hip: mmt_tta_merge_box, mmt_tta_merge_mask) against their fp64
formulation (tests/tta_formulation.py).

The bounds, u = 2^-24 (the unit roundoff of fp32), E = 1 the documented maximum ulp error of the device `expf` (HIP math API: expf,
1 ulp; one ulp is at most 2u relative), every output in [0, 1]:

  box probabilities.  One view: the argument x - max is rounded once (relative u, which moves exp(x - max) by |x - max| u relative,
  i.e. the PROBABILITY by at most t e^-t u <= 0.37 u absolute, the row sum being >= 1); the numerator carries expf's 2E u, the row
  sum 2E u + 0.37 u + (C - 1) u for its C - 1 additions in any order, the division u: (4E + C + 0.74) u on a value <= 1.  The
  merge adds V such values (V - 1 additions, each u relative on partial sums whose quotient by V stays <= 1) and divides once:
        |prob - formulation| <= (4E + C + V + 1) u        = 77 u = 4.6e-6 at C = 64, V = 8  (the issue's ceiling is 1e-5)
  mask probabilities.  The stable sigmoid is one expf (2E u), one addition (u), one division (u) whichever the sign; then the V - 1
  additions and the division by V:
        |prob - formulation| <= (2E + 2 + V) u             = 12 u = 7.2e-7 at V = 8
  regression.  V - 1 additions and one division of exactly represented inputs (the sign flip is exact), as the issue sets it:
        |reg - formulation| <= (V + 1) u max|reg|

Largest errors measured on the MI355X over the cases below: see MEASURED (asserted nowhere: the bounds above are the bar).

Mutants these tests catch (each is built into the formulation by `_mutant` and must be FARTHER from the kernel's output than the
bound, on inputs of the cases below -- a kernel with that mistake would therefore fail the comparison):
  no_dx_negation       a mirrored view's dx enters the mean with its sign
  negate_dw            dw is negated instead of dx
  no_mask_mirror       a mirrored view's mask logits are read left to right
  wrong_class_channel  the plane of class (label + 1) % C
  divide_by_k          the sums are divided by the number of un-mirrored views instead of V"""
import pytest
import torch

import tta_formulation as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EXPF_ULP = 1
# largest |kernel - formulation| measured on the MI355X over this file's cases (box probabilities, mask probabilities, and the
# regression error as a multiple of u max|reg|)
MEASURED = {"box_prob": 1.27e-7, "mask_prob": 1.39e-7, "reg_over_u_maxreg": 0.74}


def box_bound(V, C):
    return (4 * EXPF_ULP + C + V + 1) * U


def mask_bound(V):
    return (2 * EXPF_ULP + 2 + V) * U


def reg_bound(V, reg):
    return (V + 1) * U * float(reg.abs().max())


def _alt(V):
    return [v % 2 == 1 for v in range(V)]


def _box_inputs(V, R, C, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((V, R, C), generator=g) * 4.0
    reg = torch.randn((V, R, 4 * C), generator=g) * 2.0
    return logits, reg


def _mask_inputs(V, D, C, M, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((V, D, C, M, M), generator=g) * 4.0
    labels = torch.randint(0, C, (D,), generator=g, dtype=torch.int64)
    return logits, labels


def _mutant(kind, logits, second, flips):
    """the formulation with one named mistake -> the tensor that mistake changes (reg for the dx / dw ones, prob otherwise)"""
    V = len(flips)
    if kind == "no_dx_negation":
        return F.merge_box(logits, second, [False] * V)[1]
    if kind == "negate_dw":
        r = second.clone().to(torch.float64)
        for v in range(V):
            if flips[v]:
                r[v][:, 2::4] *= -1
        return F.merge_box(logits, r, [False] * V)[1]
    if kind == "no_mask_mirror":
        return F.merge_mask(logits, second, [False] * V)
    if kind == "wrong_class_channel":
        return F.merge_mask(logits, (second + 1) % logits.shape[2], flips)
    if kind == "divide_by_k_box":
        return F.merge_box(logits, second, flips)[0] * V / max(1, V - sum(flips))
    if kind == "divide_by_k_mask":
        return F.merge_mask(logits, second, flips) * V / max(1, V - sum(flips))
    raise KeyError(kind)


BOX_CASES = [(1, 1, 2), (2, 3, 3), (3, 257, 64), (8, 4099, 3), (2, 4099, 64), (8, 257, 2), (1, 257, 3), (8, 3, 64)]


@pytest.mark.parametrize("V,R,C", BOX_CASES)
def test_merge_box_against_the_formulation(V, R, C):
    from maskrcnn_benchmark import _hip as H
    logits, reg = _box_inputs(V, R, C, 100 + V + R + C)
    flips = _alt(V)
    prob, out = H.tta_merge_box(logits.cuda(), reg.cuda(), flips)
    rp, rr = F.merge_box(logits, reg, flips)
    ep = float((prob.cpu().double() - rp).abs().max())
    er = float((out.cpu().double() - rr).abs().max())
    print("merge_box V=%d R=%d C=%d: prob err %.3g (bound %.3g), reg err %.3g = %.2f u max|reg|"
          % (V, R, C, ep, box_bound(V, C), er, er / (U * float(reg.abs().max()))))
    assert prob.shape == (R, C) and out.shape == (R, 4 * C)
    assert ep <= box_bound(V, C) <= 1e-5
    assert er <= reg_bound(V, reg)
    assert float(prob.min()) >= 0.0 and float(prob.max()) <= 1.0
    # the same bits on a second call
    prob2, out2 = H.tta_merge_box(logits.cuda(), reg.cuda(), flips)
    assert torch.equal(prob, prob2) and torch.equal(out, out2)
    if V > 1:   # (with mirrored views present the named mistakes are visible)
        for kind in ("no_dx_negation", "negate_dw"):
            assert float((out.cpu().double() - _mutant(kind, logits, reg, flips)).abs().max()) > 100 * reg_bound(V, reg), kind
        assert float((prob.cpu().double() - _mutant("divide_by_k_box", logits, reg, flips)).abs().max()) > 100 * box_bound(V, C)


@pytest.mark.parametrize("mask", range(8))
def test_merge_box_every_flip_mask_of_three_views(mask):
    from maskrcnn_benchmark import _hip as H
    V, R, C = 3, 257, 3
    logits, reg = _box_inputs(V, R, C, 7)
    flips = [bool((mask >> v) & 1) for v in range(V)]
    prob, out = H.tta_merge_box(logits.cuda(), reg.cuda(), flips)
    rp, rr = F.merge_box(logits, reg, flips)
    assert float((prob.cpu().double() - rp).abs().max()) <= box_bound(V, C)
    assert float((out.cpu().double() - rr).abs().max()) <= reg_bound(V, reg)
    # dy, dw, dh never change sign; dx of exactly the mirrored views does: the other seven masks are farther than the bound
    for other in range(8):
        if other != mask:
            wrong = F.merge_box(logits, reg, [bool((other >> v) & 1) for v in range(V)])[1]
            assert float((out.cpu().double() - wrong).abs().max()) > 100 * reg_bound(V, reg)


def test_merge_box_one_view_and_equal_views_are_the_view():
    """V = 1 and two identical un-mirrored views return the view's regression to the bit and its softmax within one view's bound;
    the two results are the same bits ((a + a) / 2 == a)"""
    from maskrcnn_benchmark import _hip as H
    logits, reg = _box_inputs(1, 257, 3, 11)
    p1, r1 = H.tta_merge_box(logits.cuda(), reg.cuda(), [False])
    p2, r2 = H.tta_merge_box(logits.repeat(2, 1, 1).cuda(), reg.repeat(2, 1, 1).cuda(), [False, False])
    assert torch.equal(r1.cpu(), reg[0]) and torch.equal(r2, r1) and torch.equal(p2, p1)
    assert float((p1.cpu().double() - torch.softmax(logits[0].double(), 1)).abs().max()) <= box_bound(1, 3)


def test_merge_box_extreme_logits_and_a_nan_row():
    from maskrcnn_benchmark import _hip as H
    V, R, C = 3, 9, 3
    logits, reg = _box_inputs(V, R, C, 5)
    logits[:, 0] = torch.tensor([100.0, -100.0, 0.0])
    logits[:, 1] = torch.tensor([-100.0, -100.0, -100.0])
    logits[0, 2] = torch.tensor([100.0, 100.0, -100.0])
    logits[1, 4, 1] = float("nan")              # one view's row -> that row of the output, no other
    flips = [False, True, False]
    prob, out = H.tta_merge_box(logits.cuda(), reg.cuda(), flips)
    rp, rr = F.merge_box(logits, reg, flips)
    prob, out = prob.cpu().double(), out.cpu().double()
    assert torch.isnan(prob[4]).all() and torch.isnan(rp[4]).all()
    keep = [r for r in range(R) if r != 4]
    assert not torch.isnan(prob[keep]).any()
    assert float((prob[keep] - rp[keep]).abs().max()) <= box_bound(V, C)
    assert float((out - rr).abs().max()) <= reg_bound(V, reg)          # the regression of the NaN row is untouched by it
    assert float(prob[0, 0]) == 1.0 and abs(float(prob[1].sum()) - 1.0) < 1e-6


MASK_CASES = [(1, 1, 2, 1), (2, 3, 3, 7), (3, 257, 3, 28), (8, 4099, 2, 7), (2, 4099, 3, 28), (8, 3, 64, 28), (3, 257, 64, 1),
              (1, 257, 3, 7)]


@pytest.mark.parametrize("V,D,C,M", MASK_CASES)
def test_merge_mask_against_the_formulation(V, D, C, M):
    from maskrcnn_benchmark import _hip as H
    logits, labels = _mask_inputs(V, D, C, M, 200 + V + D + C + M)
    flips = _alt(V)
    prob = H.tta_merge_mask(logits.cuda(), labels.cuda(), flips)
    ref = F.merge_mask(logits, labels, flips)
    assert prob.shape == (D, 1, M, M)
    e = float((prob[:, 0].cpu().double() - ref).abs().max())
    print("merge_mask V=%d D=%d C=%d M=%d: err %.3g (bound %.3g)" % (V, D, C, M, e, mask_bound(V)))
    assert e <= mask_bound(V) <= 1e-5
    assert torch.equal(prob, H.tta_merge_mask(logits.cuda(), labels.cuda(), flips))      # the same bits on a second call
    got = prob[:, 0].cpu().double()
    assert float((got - _mutant("wrong_class_channel", logits, labels, flips)).abs().max()) > 100 * mask_bound(V)
    if V > 1:
        assert float((got - _mutant("divide_by_k_mask", logits, labels, flips)).abs().max()) > 100 * mask_bound(V)
        if M > 1:   # (M = 1: the mirror image of a 1 x 1 plane is itself)
            assert float((got - _mutant("no_mask_mirror", logits, labels, flips)).abs().max()) > 100 * mask_bound(V)


@pytest.mark.parametrize("mask", range(8))
def test_merge_mask_every_flip_mask_of_three_views(mask):
    from maskrcnn_benchmark import _hip as H
    V, D, C, M = 3, 5, 3, 7
    logits, labels = _mask_inputs(V, D, C, M, 9)
    flips = [bool((mask >> v) & 1) for v in range(V)]
    got = H.tta_merge_mask(logits.cuda(), labels.cuda(), flips)[:, 0].cpu().double()
    assert float((got - F.merge_mask(logits, labels, flips)).abs().max()) <= mask_bound(V)
    for other in range(8):
        if other != mask:
            wrong = F.merge_mask(logits, labels, [bool((other >> v) & 1) for v in range(V)])
            assert float((got - wrong).abs().max()) > 100 * mask_bound(V)


def test_merge_mask_extremes_bad_labels_and_identities():
    from maskrcnn_benchmark import _hip as H
    V, D, C, M = 2, 6, 3, 7
    logits, labels = _mask_inputs(V, D, C, M, 13)
    logits[:, 0] = 100.0
    logits[:, 1] = -100.0
    logits[1, 2, :, 3, 1] = float("nan")
    labels[3], labels[4] = -1, C                # no such plane: NaN for that detection's block, nothing else
    flips = [False, True]
    got = H.tta_merge_mask(logits.cuda(), labels.cuda(), flips)[:, 0].cpu().double()
    ref = F.merge_mask(logits, labels, flips)
    assert torch.isnan(got[3]).all() and torch.isnan(got[4]).all()
    assert bool((got[0] == 1.0).all()) and bool((got[1] >= 0).all()) and float(got[1].max()) < 1e-40
    assert torch.equal(torch.isnan(got), torch.isnan(ref))              # (the NaN logit: its mirrored pixel only)
    assert int(torch.isnan(got[2]).sum()) == 1 and bool(torch.isnan(got[2, 3, M - 1 - 1]))
    ok = ~torch.isnan(ref)
    assert float((got[ok] - ref[ok]).abs().max()) <= mask_bound(V)
    # one view / two equal un-mirrored views: the same bits, the view's own sigmoid
    l1, lab = _mask_inputs(1, 257, 3, 7, 17)
    a = H.tta_merge_mask(l1.cuda(), lab.cuda(), [False])
    b = H.tta_merge_mask(l1.repeat(2, 1, 1, 1, 1).cuda(), lab.cuda(), [False, False])
    assert torch.equal(a, b)
    assert float((a[:, 0].cpu().double() - torch.sigmoid(l1[0].double())[torch.arange(257), lab]).abs().max()) <= mask_bound(1)


def test_empty_inputs_launch_nothing():
    from maskrcnn_benchmark import _hip as H
    prob, out = H.tta_merge_box(torch.zeros((2, 0, 3), device="cuda"), torch.zeros((2, 0, 12), device="cuda"), [False, True])
    assert prob.shape == (0, 3) and out.shape == (0, 12)
    m = H.tta_merge_mask(torch.zeros((2, 0, 3, 7, 7), device="cuda"), torch.zeros((0,), dtype=torch.int64, device="cuda"), [False, True])
    assert m.shape == (0, 1, 7, 7)
    L = H._lib_raw()
    # R = 0 / D = 0 return 0 whatever the pointers are: nothing is launched, nothing is read
    assert L.mmt_tta_merge_box(None, None, 2, 0, 3, 2, None, None, None) == 0
    assert L.mmt_tta_merge_mask(None, None, 2, 0, 3, 7, 2, None, None) == 0
    torch.cuda.synchronize()


def test_refused_arguments():
    """every malformed argument returns MMT_EINVAL before any launch: the outputs keep their sentinel"""
    from maskrcnn_benchmark import _hip as H
    L = H._lib_raw()
    EINVAL = -22
    V, R, C, M = 2, 5, 3, 7
    lg = torch.zeros((V, R, C), device="cuda")
    rg = torch.zeros((V, R, 4 * C), device="cuda")
    prob = torch.full((R, C), 7.0, device="cuda")
    out = torch.full((R, 4 * C), 7.0, device="cuda")
    p = lambda t: t.data_ptr()
    s = H._stream()
    good = [p(lg), p(rg), V, R, C, 1, p(prob), p(out), s]
    bad = {"V=0": (2, 0), "V=9": (2, 9), "R<0": (3, -1), "C=0": (4, 0), "C=65": (4, 65), "flip_mask<0": (5, -1),
           "flip_mask=2^V": (5, 1 << V), "logits NULL": (0, None), "reg NULL": (1, None), "prob NULL": (6, None),
           "reg_out NULL": (7, None)}
    for name, (i, v) in bad.items():
        a = list(good)
        a[i] = v
        assert L.mmt_tta_merge_box(*a) == EINVAL, name
    torch.cuda.synchronize()
    assert bool((prob == 7.0).all()) and bool((out == 7.0).all())
    assert L.mmt_tta_merge_box(*good) == 0

    ml = torch.zeros((V, R, C, M, M), device="cuda")
    lab = torch.zeros((R,), dtype=torch.int64, device="cuda")
    mp = torch.full((R, M, M), 7.0, device="cuda")
    good = [p(ml), p(lab), V, R, C, M, 1, p(mp), s]
    bad = {"V=0": (2, 0), "V=9": (2, 9), "D<0": (3, -1), "C=0": (4, 0), "C=65": (4, 65), "M=0": (5, 0), "M=1025": (5, 1025),
           "flip_mask<0": (6, -1), "flip_mask=2^V": (6, 1 << V), "logits NULL": (0, None), "labels NULL": (1, None),
           "prob NULL": (7, None)}
    for name, (i, v) in bad.items():
        a = list(good)
        a[i] = v
        assert L.mmt_tta_merge_mask(*a) == EINVAL, name
    torch.cuda.synchronize()
    assert bool((mp == 7.0).all())
    assert L.mmt_tta_merge_mask(*good) == 0
    torch.cuda.synchronize()

    # the Python binding refuses what does not describe such a call, before it reaches the library
    with pytest.raises(ValueError):
        H.tta_merge_box(lg, rg[:, :, :8], [False, True])
    with pytest.raises(ValueError):
        H.tta_merge_box(lg, rg, [False])
    with pytest.raises(ValueError):
        H.tta_merge_box(lg.double(), rg, [False, True])
    with pytest.raises(ValueError):
        H.tta_merge_mask(ml, lab.to(torch.int32), [False, True])
    with pytest.raises(ValueError):
        H.tta_merge_mask(ml[:, :, :, :, :5], lab, [False, True])
    with pytest.raises(ValueError):
        H.tta_merge_mask(torch.zeros((9, 1, 2, 3, 3), device="cuda"), lab[:1], [False] * 9)
    with pytest.raises(RuntimeError):      # C > 64: the library's refusal surfaces as an error, nothing falls back
        H.tta_merge_box(torch.zeros((1, 2, 65), device="cuda"), torch.zeros((1, 2, 260), device="cuda"), [False])
