"""The weight gradient's launches are what they were before its routing had one owner (csrc/conv_route.hip: wgrad_route): one case
per kernel family, each the smallest shape that reaches the family with more than one pixel range where it has ranges (workspace and
reduce launch included); dw, accumulated into a non-zero start with a row scale, is compared BIT FOR BIT with the digests that
tests/golden/gen_golden_wgrad_bits.py recorded on the MI355X at the commit before (tests/golden/wgrad_bits.json: SHA-256 of dw's
bytes in memory order; every case ran twice there and gave one digest).  dbias is held to the bound the other weight-gradient
tests use, 3e-6 of the largest column's sum |dy| (of dy as stored): its sums use float atomics across blocks once M > 1024.
The register-splitting kernel (conv_wgrad_split_kernel) is reached only by operands past 2^31 bytes: the host test pins its route."""
import hashlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_bits.json")

PL = (1, 128, 16, 32, 128)      # the plane-fed kernel's smallest layer with two pixel ranges (T = 16 super-steps)
# name: (precision, f16x2, (N, Cin, H, W, Cout), k, x bf16, dy bf16, planes, counter that moves)
CASES = {
    "planes_three_tap": (3, True, PL, 3, 0, 0, True, "wgrad_pl"),
    "planes_one_tap": (3, True, PL, 1, 0, 0, True, "wgrad_pl"),
    "f16_decode2": (3, True, (1, 64, 32, 32, 64), 1, 0, 0, False, "wgrad"),      # M = 1024: two ranges
    "f16_decode1": (3, True, (4, 64, 26, 10, 64), 1, 0, 0, False, "wgrad"),      # Wo = 10, M = 1040
    "f16_decode0": (3, True, (64, 64, 4, 4, 64), 1, 0, 0, False, "wgrad"),       # 4 x 4 maps
    "bf16x3": (3, False, (1, 64, 32, 32, 64), 1, 0, 0, False, None),
    "cout6": (3, True, (1, 64, 32, 32, 6), 1, 0, 0, False, None),                # Cout % 4 != 0: no 4-channel loads, no fp16 split
    "bf16_x": (1, True, (1, 64, 32, 32, 64), 1, 1, 0, False, None),
    "bf16_dy": (1, True, (1, 64, 32, 32, 64), 1, 0, 1, False, None),
    "bf16_x_dy": (1, True, (1, 64, 32, 32, 64), 3, 1, 1, False, None),
    "fp32_fast": (0, True, (1, 64, 32, 32, 64), 3, 0, 0, False, None),
    "fp32_slow": (0, True, (64, 64, 4, 4, 64), 1, 0, 0, False, None),
}
GROUP = ("planes_three_tap", "planes_one_tap")   # the same two as a batch of two (a quarter of their own ranges each)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _operands(name):
    prec, f16, (N, Cin, Hh, W, Cout), k, xb, db, planes, _ = CASES[name]
    g = torch.Generator().manual_seed(sum(ord(c) for c in name))
    x = _cl(torch.randn((N, Cin, Hh, W), generator=g).relu().cuda())
    dy = _cl((torch.randn((N, Cout, Hh, W), generator=g) * 1e-3).cuda())
    rs = (torch.rand(Cout, generator=g) + 0.5).cuda()
    dw = _cl((torch.randn((Cout, Cin, k, k), generator=g) * 1e-5).cuda())
    if xb:
        x = x.bfloat16()
    if db:
        dy = dy.bfloat16()
    bias = torch.zeros((Cout,), device="cuda")
    return x, dy, rs, dw, bias


def _attach(H, name, x, dy):
    """what the producers of the operands leave behind: recorded maxima, and for the plane-fed cases the row-blocked planes"""
    if CASES[name][0] != 3 or x.dtype != torch.float32:
        return
    for t in (x, dy):
        t._mmt_amax = H._amax_of(t)
        if CASES[name][6]:
            H.f16_split_pg(t)


def digest(dw):
    return hashlib.sha256(dw.permute(0, 2, 3, 1).contiguous().cpu().numpy().tobytes()).hexdigest()


def _check_bias(bias, dy):
    if bias is not None:
        ref = dy.double().sum((0, 2, 3))
        assert (bias.double() - ref).abs().max().item() <= 3e-6 * dy.double().abs().sum((0, 2, 3)).max().item()


def run_case(H, name):
    """-> digest of dw after one launch of the case (mode and switches set and restored here)"""
    prec, f16, shape, k, _, _, _, counter = CASES[name]
    prev = H.get_conv_precision()
    H.set_conv_precision(prec)
    H.set_f16x2(f16)
    try:
        x, dy, rs, dw, bias = _operands(name)
        _attach(H, name, x, dy)
        n0 = {c: H.F16_STATS.get(c, 0) for c in ("wgrad", "wgrad_pl", "wgrad_grouped")}
        H.conv_wgrad(x, dy, tuple(dw.shape), 1, k // 2, dw, rs, bias)
        torch.cuda.synchronize()
        moved = {c for c in n0 if H.F16_STATS.get(c, 0) != n0[c]}
        assert moved == ({counter} if counter else set()), moved   # the family the case is named after ran, nothing else
        _check_bias(bias, dy)
        return digest(dw)
    finally:
        H.set_f16x2(None)
        H.set_conv_precision(prev)


def run_group(H):
    prev = H.get_conv_precision()
    H.set_conv_precision(3)
    H.set_f16x2(True)
    try:
        jobs = []
        for name in GROUP:
            x, dy, rs, dw, bias = _operands(name)
            _attach(H, name, x, dy)
            jobs.append((x, dy, tuple(dw.shape), 1, CASES[name][3] // 2, dw, rs, bias))
        n0 = H.F16_STATS.get("wgrad_grouped", 0)
        H.conv_wgrad_group(jobs)
        torch.cuda.synchronize()
        assert H.F16_STATS.get("wgrad_grouped", 0) == n0 + len(GROUP)
        for j in jobs:
            _check_bias(j[7], j[1])
        return hashlib.sha256("".join(digest(j[5]) for j in jobs).encode()).hexdigest()
    finally:
        H.set_f16x2(None)
        H.set_conv_precision(prev)


@pytest.fixture(scope="module")
def hip():
    from maskrcnn_benchmark import _hip as H
    H.lib()
    return H


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_dw_bit_identical(hip, golden, name):
    assert run_case(hip, name) == golden[name]


def test_group_of_two_bit_identical(hip, golden):
    assert run_group(hip) == golden["group_of_two"]
