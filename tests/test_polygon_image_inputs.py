"""The inputs of tests/polygon_image_inputs.py against the oracle alone (no GPU): every class does what its name says, so that
the kernel tests that use them are not comparing empty masks with empty masks."""
import numpy as np
import pytest

import polygon_image_inputs as pi
from oracle import native

ALL_SIZES = pi.SIZES + [pi.BIG]


def _of(c, name):
    return [g for g in range(len(c["cls"])) if c["cls"][g] == name]


@pytest.mark.parametrize("size", pi.SIZES, ids=lambda s: "%dx%d" % s)
def test_every_class_is_present_and_ranges_are_valid(size):
    c = pi.cases(size)
    NP = len(c["poly_off"]) - 1
    assert c["poly_xy"].dtype == np.float32 and c["poly_off"].dtype == np.int32 and c["inst_poly"].dtype == np.int32
    assert (c["inst_poly"] >= 0).all() and (c["inst_poly"] <= NP).all()
    for name in pi.CLASSES:
        assert len(_of(c, name)) == pi.PER_CLASS
    assert pi.cases(size) is c                                   # one generation per size
    assert not (np.diff(c["inst_poly"][:, 0]) >= 0).all()         # the ranges are not in polygon order


def test_big_case():
    c = pi.cases(pi.BIG)
    assert len(c["inst_poly"]) == pi.BIG_INSTANCES
    m = pi.oracle_masks(pi.BIG)
    assert m.shape == (pi.BIG_INSTANCES, 1000, 1000)
    assert (m.reshape(len(m), -1).sum(1) > 1000).all()


@pytest.mark.parametrize("size", ALL_SIZES, ids=lambda s: "%dx%d" % s)
def test_masks_are_not_trivial(size):
    m = pi.oracle_masks(size)
    c = pi.cases(size)
    filled = m.reshape(len(m), -1).sum(1)
    for name in ("i", "iii", "vii", "ix"):
        g = _of(c, name)
        if min(size) >= 37:
            assert (filled[g] > 0).all(), name
        else:   # a blob a fraction of a pixel wide may miss every pixel centre
            assert (filled[g] > 0).sum() * 2 >= len(g), name
    if size[0] * size[1] > 1:
        assert len({m[g].tobytes() for g in range(len(m))}) > len(m) // 2


@pytest.mark.parametrize("size", pi.SIZES, ids=lambda s: "%dx%d" % s)
def test_class_ii_is_empty_and_class_viii_has_no_polygons(size):
    c, m = pi.cases(size), pi.oracle_masks(size)
    for g in _of(c, "ii"):
        assert len(pi.polygons_of(c, g)) == 1 and int(m[g].sum()) == 0
    for g in _of(c, "viii"):
        assert pi.polygons_of(c, g) == [] and int(m[g].sum()) == 0


def test_class_iii_reaches_every_image_edge():
    for size in pi.SIZES[1:]:
        c, m = pi.cases(size), pi.oracle_masks(size)
        u = np.zeros(size, bool)
        for g in _of(c, "iii"):
            xy = pi.polygons_of(c, g)[0]
            assert xy[:, 0].min() < 0 and xy[:, 0].max() > size[1] and xy[:, 1].min() < 0 and xy[:, 1].max() > size[0]
            u |= m[g].astype(bool)
        assert u[0].any() and u[-1].any() and u[:, 0].any() and u[:, -1].any()


def test_class_vii_union_differs_from_xor():
    n = 0
    for size in pi.SIZES[1:] + [pi.BIG]:
        c, m = pi.cases(size), pi.oracle_masks(size)
        for g in _of(c, "vii"):
            polys = pi.polygons_of(c, g)
            assert 2 <= len(polys) <= 3
            single = [native.poly_mask([p.reshape(-1)], *size).astype(bool) for p in polys]
            x = np.zeros(size, bool)
            for s in single:
                x ^= s
            assert np.array_equal(np.logical_or.reduce(single), m[g].astype(bool))
            n += int((x != m[g].astype(bool)).sum())
            if min(size) >= 37:
                assert (x != m[g].astype(bool)).any(), (size, g)
    assert n > 0


@pytest.mark.parametrize("size", ALL_SIZES, ids=lambda s: "%dx%d" % s)
def test_class_ix_has_a_crossing_at_the_end_of_the_mask(size):
    from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle
    H, W = size
    c = pi.cases(size)
    for g in _of(c, "ix"):
        a = np.concatenate([mask_rle._poly_crossings(p.astype(np.float64), H, W) for p in pi.polygons_of(c, g)])
        assert a.max() == H * W and a.min() >= 0, (size, g)


def test_class_vi_edge_counts():
    for size in pi.SIZES:
        c = pi.cases(size)
        n = sorted(len(p) for g in _of(c, "vi") for p in pi.polygons_of(c, g))
        assert sum(v > 64 for v in n) >= 3 and sum(v > 256 for v in n) >= 2
        H, W = size
        longest = max(np.abs(np.diff(np.concatenate([p, p[:1]]), axis=0)).max() for g in _of(c, "vi") for p in pi.polygons_of(c, g))
        assert longest > max(H, W)


def test_class_iv_vertices_are_on_the_grid():
    c = pi.cases((150, 128))
    for k, g in enumerate(_of(c, "iv")):
        xy = pi.polygons_of(c, g)[0].astype(np.float64)
        assert np.abs(xy * 10 - np.round(xy * 10)).max() < 1e-3
