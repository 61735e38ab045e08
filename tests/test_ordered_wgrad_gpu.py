"""The ordered form of the stem weight gradient (include/mmtpsm.h: mmt_stem_wgrad_ordered; csrc/stem_bwd.hip, csrc/ordered.h;
bound as _hip.stem_wgrad_ordered), which layers/fused.py::StemFn takes in deterministic mode.

Per case of tests/test_stem_backward_gpu.py::WGRAD_CASES ((1, 8, 8) is one tile, (4, 160, 160) is 800 tiles over 512 blocks), with
the mode on: the result into zeros against the fp64 formulation within the bar of the unordered kernel's own test (imported, not a
new number), with and without rowscale; into a non-zero dw the result is BITWISE base + (the result into zeros); five calls give five
bit-equal results; a NaN-filled workspace changes nothing (every partial that is read was written); a null or one-float-short
workspace is refused with -22 and a NaN-filled dw stays NaN; the library's workspace query is what the binding allocates.  Whether
five runs of the unordered kernel differed is printed, not asserted."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import stem_formulations as sf  # noqa: E402
import test_stem_backward_gpu as ts  # noqa: E402

SHAPE = (64, 3, 7, 7)


@pytest.fixture()
def hip():
    from maskrcnn_benchmark import _hip as H
    H.lib()
    H.set_deterministic(True)
    yield H
    H.set_deterministic(False)


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _rel(got, ref):
    return ((got.detach().double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()   # (the measure of ts._report)


class _Capture(object):
    """hands the binding's torch.empty workspaces out to the test: the size the binding allocated, and a way to poison the memory
    before the launch reads or writes it"""

    def __init__(self, H, fill=None):
        self.H, self.fill, self.sizes = H, fill, []

    def __enter__(self):
        self.orig = self.H._wgrad_ordered_ws

        def ws(floats, device, what):
            t = self.orig(floats, device, what)
            self.sizes.append(t.numel())
            if self.fill is not None:
                t.fill_(self.fill)
            return t
        self.H._wgrad_ordered_ws = ws
        return self

    def __exit__(self, *exc):
        self.H._wgrad_ordered_ws = self.orig


@pytest.mark.parametrize("case", ts.WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_stem_weight_gradient_ordered(hip, case):
    H = hip
    N, Hh, Ww = case
    x, dy, scale = ts._wgrad_inputs(case)
    xd, dyd, sd = x.cuda(), ts._dev(dy), scale.cuda()
    ref = sf.stem_wgrad_reference(x, dy)
    ref_scaled = ref * scale.double().view(-1, 1, 1, 1)   # (what stem_wgrad_reference does with a rowscale: one fp64 convolution)

    def run(dw, with_scale=True):
        return H.stem_wgrad_ordered(xd, dyd, dw, sd if with_scale else None)

    def zeros():
        return _cl(torch.zeros(SHAPE))

    first = run(zeros())
    dev = _rel(first, ref_scaled)
    print("stem %-16s ordered into zeros         worst |got - fp64| / max |fp64| = %.3e" % (case, dev))
    assert dev <= ts.BAR, (case, dev)
    dev = _rel(run(zeros(), False), ref)
    print("stem %-16s ordered without rowscale   worst |got - fp64| / max |fp64| = %.3e" % (case, dev))
    assert dev <= ts.BAR, (case, dev)
    for _ in range(4):   # five calls, bit-equal
        assert torch.equal(run(zeros()), first), (case, "two ordered calls differ")
    # accumulate: one rounding per element, base + sum
    g = torch.Generator().manual_seed(5)
    base = _cl(torch.randn(SHAPE, generator=g) * ref.abs().max().float())
    assert torch.equal(run(base.clone()), base + first), (case, "dw += is not bitwise base + (the result into zeros)")
    # a poisoned workspace: everything the finish reads was written by stage one
    with _Capture(H, float("nan")):
        assert torch.equal(run(zeros()), first), (case, "a partial was read that stage one had not written")
    # the unordered kernel, for the record
    H.set_deterministic(False)
    try:
        outs = [H.stem_wgrad(xd, dyd, zeros(), sd) for _ in range(5)]
        torch.cuda.synchronize()
    finally:
        H.set_deterministic(True)
    print("stem %-16s five unordered runs %s" % (case, "DIFFERED" if any(not torch.equal(o, outs[0]) for o in outs[1:]) else "were bit-equal"))

    # the C ABI: the query is what the binding allocated; a null or short workspace is refused and writes nothing
    L = H.lib()
    need = L.mmt_stem_wgrad_ws_floats(N, Hh, Ww)
    with _Capture(H) as cap:
        run(zeros())
    assert cap.sizes == [need] and need > 0
    nan = _cl(torch.full(SHAPE, float("nan")))
    ws = torch.empty((need,), device="cuda")
    args = (xd.data_ptr(), dyd.data_ptr(), sd.data_ptr(), nan.data_ptr(), N, Hh, Ww)
    assert L.mmt_stem_wgrad_ordered(*args, None, need, H._stream()) == -22
    assert L.mmt_stem_wgrad_ordered(*args, ws.data_ptr(), need - 1, H._stream()) == -22
    torch.cuda.synchronize()
    assert torch.isnan(nan).all().item()


def test_refused_shapes_are_refused_by_the_ordered_entry_point_too(hip):
    """the shape checks of mmt_stem_wgrad: an empty image, a null gradient"""
    H = hip
    L = H.lib()
    assert L.mmt_stem_wgrad_ws_floats(1, 0, 8) == -22
    ws = torch.empty((1 << 16,), device="cuda")
    img = torch.zeros((1, 3, 8, 8), device="cuda")
    dws = _cl(torch.full(SHAPE, float("nan")))
    assert L.mmt_stem_wgrad_ordered(img.data_ptr(), None, None, dws.data_ptr(), 1, 8, 8, ws.data_ptr(), ws.numel(), H._stream()) == -22
    assert L.mmt_stem_wgrad_ordered(img.data_ptr(), img.data_ptr(), None, dws.data_ptr(), 1, 0, 8, ws.data_ptr(), ws.numel(),
                                    H._stream()) == -22
    torch.cuda.synchronize()
    assert torch.isnan(dws).all().item()
