"""The mask geometry kernels of csrc/masks.hip at their edges, exactly against the oracle: the polygon rasteriser on the eight
classes of tests/mask_geometry_inputs.py and on a comb with more crossings than the capped list once held, the evaluator's
paste on boxes from zero area to beyond the canvas, and the teacher's integral paste with rows that cast no vote.
(tests/test_mask_geometry_inputs.py checks, without a GPU, that these inputs are worth comparing on.)"""
import numpy as np
import pytest
import torch

import mask_geometry_inputs as mg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from maskrcnn_benchmark import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return _hip


@pytest.fixture(scope="module")
def cases():
    return mg.raster_cases()


def cl(x):  # NCHW cpu tensor -> NHWC-dense cuda tensor
    return x.cuda().contiguous(memory_format=torch.channels_last)


def rasterise(hip, c, M):
    out, ovf = hip.polygon_targets(torch.from_numpy(c["poly_xy"]).cuda(), torch.from_numpy(c["poly_off"]).cuda(),
                                   torch.from_numpy(c["roi_poly"]).cuda(), torch.from_numpy(c["boxes"]).cuda(), M)
    return out.cpu().numpy(), int(ovf)


# ------------------------------------------------------------------------------------------ rasteriser
@pytest.mark.parametrize("M", mg.RASTER_M)
def test_polygon_targets_equal_the_oracle_on_every_class(hip, cases, M):
    got, ovf = rasterise(hip, cases, M)                      # one launch for all ROIs
    want = mg.oracle_targets(cases, M)
    for c in mg.CLASSES:                                     # (class by class, so that a failure names its class)
        sel = cases["cls"] == c
        np.testing.assert_array_equal(got[sel], want[sel], err_msg="class " + c)
    assert ovf == 0


def test_polygon_targets_empty_range_is_all_zero(hip, cases):
    empty = cases["roi_poly"][:, 1] == cases["roi_poly"][:, 0]
    assert empty.sum() >= 5
    got, _ = rasterise(hip, cases, 28)
    assert (got[empty] == 0).all()
    # and a launch of nothing but empty ranges, at both ends of the polygon list
    c = dict(cases, roi_poly=np.asarray([[0, 0], [3, 3], [len(cases["poly_off"]) - 1] * 2], np.int32), boxes=cases["boxes"][:3])
    got, ovf = rasterise(hip, c, 28)
    assert (got == 0).all() and ovf == 0


@pytest.mark.parametrize("M", [33, 64])
def test_polygon_targets_refuses_sizes_beyond_its_pixel_registers(hip, cases, M):
    with pytest.raises(RuntimeError):
        rasterise(hip, cases, M)
    torch.cuda.synchronize()


@pytest.mark.parametrize("edges", [60, 130])
@pytest.mark.parametrize("M", mg.RASTER_M)
def test_polygon_targets_comb_beyond_the_old_crossing_cap(hip, M, edges):
    """60 (and, beyond one pass of 64 edges, 130) full-width edges: 1680 (3640) crossings at M = 28, where the list kept 1536 and
    the target came out wrong with nothing but a flag nobody read.  Edges are walked in passes of 64 now; no list can fill."""
    c = mg.comb(edges)
    got, ovf = rasterise(hip, c, M)
    np.testing.assert_array_equal(got, mg.oracle_targets(c, M))
    assert ovf == 0


# ------------------------------------------------------------------------------------------ paste
@pytest.mark.parametrize("M", mg.PASTE_M)
def test_paste_mask_stack_equals_the_oracle(hip, M):
    from oracle import model as om
    ih, iw = mg.CANVAS
    prob, boxes = mg.paste_cases()[M]
    got = hip.paste_mask_stack(torch.from_numpy(prob).cuda(), torch.from_numpy(boxes).cuda(), ih, iw, mg.PASTE_THRESH).cpu().numpy()
    want = np.stack([om.paste_mask(torch.from_numpy(p), torch.from_numpy(b), ih, iw, mg.PASTE_THRESH).numpy()
                     for p, b in zip(prob, boxes)])
    assert want.sum() > 10000 and (want.reshape(len(want), -1).sum(1) > 0).mean() > 0.8   # the pastes are not empty canvases
    np.testing.assert_array_equal(got[:, 0], want)


@pytest.mark.parametrize("M", mg.PASTE_M)
def test_paste_leaves_the_canvas_zero_for_boxes_outside_it(hip, M):
    ih, iw = mg.CANVAS
    boxes = torch.from_numpy(mg.outside_boxes()).cuda()
    D = len(boxes)
    got = hip.paste_mask_stack(torch.ones(D, M, M).cuda(), boxes, ih, iw, mg.PASTE_THRESH)
    assert got.shape == (D, 1, ih, iw) and int(got.sum()) == 0
    seg = hip.paste_masks(cl(torch.full((D, 3, M, M), 20.0)), torch.ones(D).int().cuda(), boxes, torch.zeros(D).int().cuda(), 1, ih, iw,
                          mg.PASTE_THRESH)
    assert int(seg.abs().sum()) == 0


@pytest.mark.parametrize("M", [14, 28])
def test_paste_masks_integral_map_with_rows_that_cast_no_vote(hip, M):
    """NC = 3, labels in {1, 2}, two images, every fifth row img = -1.  The device sigmoid differs from the host's by a few 1e-7, so
    a pixel is left out where some detection's fp64 bilinear value lies within 2e-6 of the threshold -- at most 1 in 10 000 of
    the pixels the expanded boxes cover; every other pixel of both maps is equal."""
    ih, iw = mg.CANVAS
    logits, labels, boxes, img = mg.integral_case(M)
    want, left, n_left, n_cov = mg.integral_reference(logits, labels, boxes, img)
    assert n_left <= mg.LEFT_OUT_CAP * n_cov, (n_left, n_cov)
    seg = hip.paste_masks(cl(torch.from_numpy(logits)), torch.from_numpy(labels).cuda(), torch.from_numpy(boxes).cuda(),
                          torch.from_numpy(img).cuda(), 2, ih, iw, mg.PASTE_THRESH).cpu().numpy()
    print("M=%d: %d pixels left out of %d covered; %d differ before leaving out" % (M, n_left, n_cov, (seg != want).sum()))
    np.testing.assert_array_equal(np.where(left, 0, seg), np.where(left, 0, want))
    # the rows behind the counts cast no vote: with them dropped from the list the maps are the same, bit for bit
    keep = torch.from_numpy(img >= 0)
    seg2 = hip.paste_masks(cl(torch.from_numpy(logits)[keep]), torch.from_numpy(labels)[keep].cuda(), torch.from_numpy(boxes)[keep].cuda(),
                           torch.from_numpy(img)[keep].cuda(), 2, ih, iw, mg.PASTE_THRESH).cpu().numpy()
    np.testing.assert_array_equal(seg, seg2)
