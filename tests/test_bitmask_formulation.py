"""The host restatement of the bitmap-ground-truth rules (tests/bitmask_formulation.py) against fp64
F.interpolate(mode="bilinear", align_corners=False): the integer weights give the same values to 1e-12, and away from exact ties at
1/2 the threshold agrees everywhere -- ties are frequent on binary inputs, which is why the rule is in integers.  Then the window
rule on the inputs where rounding and clamping decide.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import bitmask_formulation as bf

SHAPES = [((7, 5), (28, 28)), ((100, 63), (28, 28)), ((1, 1), (28, 28)), ((3, 200), (28, 28)), ((64, 64), (32, 32)),
          ((50, 50), (25, 25)), ((37, 53), (30, 41)), ((1000, 999), (28, 28))]
DENSITIES = (0.1, 0.5, 0.9)


def _mask(shape, density, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) < density).to(torch.uint8)


def _case(k, src, dst, density):
    m = _mask(src, density, 1000 * k + int(density * 10))
    S, dd = bf.weighted_sum(m, *dst)
    ref = F.interpolate(m[None, None].double(), size=dst, mode="bilinear", align_corners=False)[0, 0]
    return m, S, dd, ref


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_integer_weights_are_bilinear(k):
    src, dst = SHAPES[k]
    for density in DENSITIES:
        m, S, dd, ref = _case(k, src, dst, density)
        assert S.shape == ref.shape and int(S.min()) >= 0 and int(S.max()) <= dd
        assert (S.double() / dd - ref).abs().max().item() <= 1e-12
        away = 2 * S != dd
        assert torch.equal((ref >= 0.5)[away], (2 * S >= dd)[away])
        out = bf.resample(m, (0, 0, src[1], src[0]), *dst)
        assert torch.equal(out, (2 * S >= dd).to(torch.uint8))
        assert bool(out[2 * S == dd].all())            # ties count as set


def test_ties_do_occur():
    ties = total = 0
    for k, (src, dst) in enumerate(SHAPES):
        for density in DENSITIES:
            _, S, dd, _ = _case(k, src, dst, density)
            ties += int((2 * S == dd).sum())
            total += S.numel()
    assert ties > 0 and ties < total, (ties, total)


def test_same_size_is_a_copy_and_a_line_survives_a_halving():
    m = _mask((37, 53), 0.5, 3)
    assert torch.equal(bf.resample(m, (0, 0, 53, 37), 37, 53), m)
    assert torch.equal(bf.resample(m, (5, 7, 20, 11), 11, 20), m[7:18, 5:25])
    line = torch.zeros((40, 40), dtype=torch.uint8)
    line[:, 17] = 1
    half = bf.resample(line, (0, 0, 40, 40), 20, 20)
    assert bool(half[:, 8].all()) and int(half.sum()) == 20


def test_flips_act_on_the_destination():
    m = _mask((9, 14), 0.5, 4)
    full = (0, 0, 14, 9)
    assert torch.equal(bf.resample(m, full, 9, 14, flip=1), m.flip(1))
    assert torch.equal(bf.resample(m, full, 9, 14, flip=2), m.flip(0))
    assert torch.equal(bf.resample(m, full, 9, 14, flip=3), m.flip(0).flip(1))
    assert torch.equal(bf.resample(m, full, 18, 7, flip=1), bf.resample(m, full, 18, 7).flip(1))


@pytest.mark.parametrize("box,want", [
    ((2.5, 3.5, 10.5, 11.5), (2, 4, 8, 8)),              # half to even: 2.5 -> 2, 3.5 -> 4, 10.5 -> 10, 11.5 -> 12
    ((0.5, 1.5, 4.49, 4.51), (0, 2, 4, 3)),
    ((-7.0, -3.0, 6.0, 5.0), (0, 0, 6, 5)),              # negative start
    ((10.0, 20.0, 500.0, 400.0), (10, 20, 90, 40)),      # beyond the image: clipped at W, H (the end is exclusive)
    ((-50.0, -60.0, -10.0, -20.0), (0, 0, 1, 1)),        # wholly outside, above left: one pixel on the border
    ((300.0, 200.0, 400.0, 260.0), (99, 59, 1, 1)),      # wholly outside, below right
    ((30.0, 40.0, 10.0, 20.0), (30, 40, 1, 1)),          # inverted
    ((30.0, 40.0, 30.0, 40.0), (30, 40, 1, 1)),          # empty
    ((0.0, 0.0, 100.0, 60.0), (0, 0, 100, 60)),          # full
    ((-3e9, -3e9, 3e9, 3e9), (0, 0, 100, 60)),           # beyond int32: clamped in float first
    ((3e38, 0.0, 3.3e38, 5.0), (99, 0, 1, 5)),
])
def test_window_rule(box, want):
    assert bf.window(box, 100, 60) == want


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_window_of_a_non_finite_box_is_none(bad):
    for at in range(4):
        b = [1.0, 2.0, 30.0, 40.0]
        b[at] = bad
        assert bf.window(b, 100, 60) is None
    m = _mask((60, 100), 0.9, 5)
    assert int(bf.resample(m, None, 28, 28).sum()) == 0


def test_packer_layout():
    m = torch.zeros((2, 37, 53), dtype=torch.uint8)
    m[0, 5, 0] = m[0, 36, 1] = m[0, 0, 2] = 1            # positions 5, 37 + 36 = 73, 74: bottom of a column, top of the next
    words, rec = bf.pack(m)
    assert words.shape == (2, (37 * 53 + 63) // 64) and rec.shape == (2, 8)
    assert int(words[0, 0]) == 1 << 5 and int(words[0, 1]) == (1 << 9) | (1 << 10) and int(words[0, 2:].abs().sum()) == 0
    assert rec[0].tolist() == [3, 0, 2, 0, 36, 1, 0, 0] and rec[1].tolist() == [0] * 8
    full = torch.ones((1, 8, 8), dtype=torch.uint8)
    words, rec = bf.pack(full)
    assert int(words[0, 0]) == -1 and rec[0].tolist() == [64, 0, 7, 0, 7, 1, 0, 0]
