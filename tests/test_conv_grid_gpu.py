"""Every cell of the convolution grid (tests/conv_grid_cases.py) on the device, element by element: each (cell, form) case runs through
the binding (conv_forward; layers.fused._dgrad for the data-gradient forms; conv_wgrad and conv_wgrad_group with one and with two
jobs), the path it took is read from the binding's own evidence (the F16_STATS delta, the PROFILE record's tag and K split under
PROFILE_ALL, as tests/test_conv_paths_gpu.py reads them), and the result is held to |y - ref| <= bound * max(B, 2^-126) for EVERY
element, ref and B from the fp64 reference of conv_grid_cases and bound = twice the coefficient the host test derives for the case's
arithmetic and K (bf16-stored y: plus 2^-8 |ref|, the unit roundoff of its 8 significant bits).  A failure names the worst element as (image, row, column, channel) and
its place inside the cell's tile.  Where the launch records statistics of y the slot must hold max |y|.

Writes outside the output: every route that accepts a destination gets it INSIDE a larger buffer, 4 KiB of a NaN-free bit pattern on
both sides, the destination itself pre-filled with NaN (the strided scatter: NaN at the pixels it owns, zeros between them, as the
binding's own zero-filled allocation has them); afterwards both bands are bit-identical and no NaN is left.
  band-checked:      every "lib" cell (mmt_conv_forward through conv_forward(y_out=...): fp32, split, tiled DMA-fed incl. split-K and
                     bf16-stored x, row-resident, tap-strip on bf16 planes and on bf16 x, the strided scatter), and dw of every
                     weight-gradient route.
  NOT band-checked:  the fp16-split kinds ("f16" cells: tiled, row-resident, patch, tap-strip and plane-fed launches of
                     mmt_conv_forward_f16x2 / mmt_conv3x3_strip_f16x2 / mmt_conv_forward_pg) and the data-gradient forms: the
                     binding allocates their output itself.
The weight gradient runs once into zeros and once into a non-zero dw; dbias, an fp32 sum of the M = N Ho Wo values of a column of dy
in some order, is held to sqrt(M) 2^-24 of the column's sum |dy|: each of the M additions rounds by at most 2^-24 of a partial sum
that sum |dy| bounds, and the roundings, of either sign, add in quadrature (6e-7 at M = 105, 2e-6 at M = 1150).

What the device run confirms of the path, and what it cannot: the binding exposes the kind the dispatcher chose (F16_STATS: tiled /
tap-strip / plane-fed on the fp16 split, nothing for the library's dispatch) and, under PROFILE_ALL, the route's tag and the tiled
kernels' K ranges.  The tag of the row-resident and patch kernels is the tile variant, as of a tiled kernel; the record's K split is
1 for the tap-strip and plane-fed kinds whatever their ranges; for the weight gradient the record carries the pixel ranges, and
F16_STATS tells plane-fed, fp16 split and grouped apart.  Family, tile, strip width, plane-fed tile height, K ranges of the strip and
plane-fed kernels, pixel decode and storage bits rest on the host test, which asks the route with the block this file's calls fill.

The cell "split_*" (operands split in registers: no packed weight planes) cannot be reached through conv_forward, which always
packs the planes; it is launched through the library's C entry point with the block conv_forward would fill, minus the planes.

The large references (3x3 over 32768 and more pixels) run as fp64 unfold + matmul on the device (conv_grid_cases.products_unfold; the
host test checks that form against the CPU convolution)."""
import ctypes
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import conv_grid_cases as G  # noqa: E402

BAND = 4096            # bytes on either side of a destination
PATTERN = 0x5A5A       # 16-bit pattern of the bands: 0x5A5A5A5A is a finite fp32, 0x5A5A a finite bf16
REPORT = {"worst": {}, "times": []}


@pytest.fixture(scope="module")
def hip():
    from maskrcnn_benchmark import _hip as H
    H.lib()
    prev = H.get_conv_precision()
    yield H
    H.PROFILE, H.PROFILE_ALL = None, False
    H.set_f16x2(None)
    H.set_conv_precision(prev)
    _PROD.clear()


def cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def banded(shape, dtype, fill):
    """an NCHW-shaped, NHWC-dense destination inside a larger buffer -> (buffer viewed as int16, view, elements of a band)"""
    N, C, Hh, W = shape
    n, esz = N * C * Hh * W, torch.empty((), dtype=dtype).element_size()
    pad = BAND // esz
    buf = torch.empty(n + 2 * pad, dtype=dtype, device="cuda")
    buf.view(torch.int16).fill_(PATTERN)
    mid = buf[pad:pad + n]
    mid.copy_(fill.permute(0, 2, 3, 1).reshape(-1)) if isinstance(fill, torch.Tensor) else mid.fill_(fill)
    return buf, mid.view(N, Hh, W, C).permute(0, 3, 1, 2), pad


def bands_intact(buf, pad):
    b = buf.view(torch.int16)
    k = pad * (buf.element_size() // 2)
    return bool((b[:k] == PATTERN).all().item() and (b[-k:] == PATTERN).all().item())


_PROD = {}   # (shape, x stored as bf16, which weight) -> (sum x w, sum |x||w|) on the device: the last few, shared by a cell's forms


def products_for(key, x, w, s, p):
    if key not in _PROD:
        while len(_PROD) >= 3:
            _PROD.pop(next(iter(_PROD)))
        N, Cin, Hh, W = x.shape
        Cout, k = w.shape[0], w.shape[2]
        Ho, Wo = G.out_hw((N, Cin, Hh, W, Cout, k, s, p))
        if 2.0 * N * Ho * Wo * Cout * Cin * k * k > 2e9:
            _PROD[key] = G.products_unfold(x.cuda(), w.cuda(), s, p)
        else:
            _PROD[key] = tuple(t.cuda() for t in G.products(x, w, s, p))
    return _PROD[key]


def worst_element(y, ref, B, bound, shape, route, out_stride=1, y_ulp=0.0):
    """-> (worst ratio of |y - ref| to its limit, text naming the element)"""
    lim = bound * B.clamp_min(G.TINY) + y_ulp * ref.abs()
    ratio = (y.double() - ref).abs() / lim
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    worst, at = ratio.reshape(-1).max(0)
    n, c, h, q = (int(v) for v in torch.unravel_index(at, ratio.shape))
    Ho, Wo = G.out_hw(shape)
    m = (n * Ho + h // out_stride) * Wo + q // out_stride
    bm, bn = max(route["bm"], 1), max(route["bn"], 1)
    text = "ratio %.3g at (image %d, row %d, column %d, channel %d), tile row %d of %d, tile column %d of %d: y %.9g ref %.9g B %.3g" % (
        worst.item(), n, h, q, c, m % bm, bm, c % bn, bn, y[n, c, h, q].item(), ref[n, c, h, q].item(), B[n, c, h, q].item())
    return worst.item(), text


def launch_split(H, a_fill, x, w, y, o):
    """mmt_conv_forward with the block conv_forward fills, without packed weight planes"""
    N, Cin, Hh, W = x.shape
    Cout, k = w.shape[0], w.shape[2]
    s, p = a_fill
    Ho, Wo = G.out_hw((N, Cin, Hh, W, Cout, k, s, p))
    a = H._conv_shape(H.ConvArgs(), N, Hh, W, Cin, Cout, k, k, s, p, Ho, Wo)
    a.x, a.w, a.y = x.data_ptr(), w.data_ptr(), y.data_ptr()
    a.scale, a.shift, a.relu = H._p(o["scale"]), H._p(o["shift"]), 1 if o["relu"] else 0
    if o["res"] is not None:
        a.res, a.res_mode = o["res"].data_ptr(), o["res_mode"]
    if o["mask"] is not None:
        a.mask, a.mask_scale = o["mask"].data_ptr(), o["mask_scale"]
    if o["mul"] is not None:
        a.mul = o["mul"].data_ptr()
    if o["out_stride"] > 1:
        a.out_stride, (a.out_H, a.out_W) = o["out_stride"], o["out_hw"]
    r = H.conv_route(a, H.ENTRY_LIB)
    H._check(H.lib().mmt_conv_forward(ctypes.byref(a), H._stream()), "mmt_conv_forward")
    return r


def run_forward(H, cell, form):
    from maskrcnn_benchmark.layers import fused
    c = G.CELLS[cell]
    N, Cin, Hh, W, Cout, k, s, p = c["shape"]
    Ho, Wo = G.out_hw(c["shape"])
    o = G.operands(cell, form)
    f16 = c["entry"] == "f16"
    H.set_conv_precision(c["mode"])
    H.set_f16x2(f16)
    dgrad = form in G.DGRAD
    prod = products_for((c["shape"], c["x_bf16"], cell + "/dgrad" if dgrad else "fwd"), o["x"], o["w"], s, p)
    dev = {k_: (cl(v) if isinstance(v, torch.Tensor) and v.dim() == 4 else v.cuda() if isinstance(v, torch.Tensor) else v) for k_, v in o.items()}
    ref, B = G.conv_ref(None, None, dev, s, p, prod)
    x = dev["x"]
    band = None
    kw = dict(relu=o["relu"], res=dev["res"], res_mode=o["res_mode"], mask=dev["mask"], mask_scale=o["mask_scale"])
    dest = (N, Cout) + (o["out_hw"] or (Ho, Wo))
    if not f16 and not dgrad:
        fill = float("nan")
        if form == "scatter":   # NaN where the scatter writes, zeros between (the binding's own allocation is zero-filled)
            fill = torch.zeros(dest, device="cuda")
            fill[:, :, ::2, ::2] = float("nan")
        band = banded(dest, o["y_dtype"], fill)
        kw["y_out"] = band[1]
    if form == "scatter":
        kw.update(out_stride=2, out_hw=o["out_hw"])
    s0 = dict(H.F16_STATS)
    H.PROFILE, H.PROFILE_ALL = [], True
    t0 = time.time()
    try:
        if c["no_planes"]:
            route = launch_split(H, (s, p), x, dev["w"], band[1], dev)
            assert route.family == G.SPLIT and route.tag == c["route"]["tag"]
            y = band[1]
        elif dgrad:
            y = fused._dgrad(x, dev["w_fwd"], (N, Cout, Hh, W), 1, k - 1 - p, dev["rowscale"], mask=dev["mask"], mask_scale=o["mask_scale"],
                             res=dev["res"], res_mode=o["res_mode"])
        else:
            y = H.conv_forward(x, dev["w"], dev["scale"], dev["shift"], s, p, mul=dev["mul"], **kw)
        torch.cuda.synchronize()
        rec = H.PROFILE
    finally:
        H.PROFILE, H.PROFILE_ALL = None, False
    took = time.time() - t0
    # ---- the path, from the binding's evidence
    delta = {k_: H.F16_STATS.get(k_, 0) - s0.get(k_, 0) for k_ in ("tiled", "conv", "pg", "fallback")}
    fam, r = c["route"]["family"], c["route"]
    kind = {G.STRIP: "conv", G.PG: "pg"}.get(fam, "tiled")
    assert delta == dict({"tiled": 0, "conv": 0, "pg": 0, "fallback": 0}, **({kind: 1} if f16 else {})), (cell, form, delta)
    if not c["no_planes"]:
        assert len(rec) == 1 and len(rec[0]) == 7, (cell, form, len(rec))
        ks = 1 if fam in (G.STRIP, G.PG) else r["ksplit"]    # (the record carries the tiled kernels' K ranges)
        assert (rec[0][3][0], rec[0][4]) == ("fwd%d" % r["tag"], ks), (cell, form, rec[0][3], rec[0][4])
        assert rec[0][3][1:] == (N, Hh, W, Cin, Cout, k, s, 2 if form == "scatter" else 1)
    # ---- every element
    assert y.shape == ref.shape and y.dtype == o["y_dtype"]
    arith = G.arithmetic(cell)
    bound = G.bound_of(arith, k * k * Cin)
    worst, text = worst_element(y, ref, B, bound, c["shape"], r, 2 if form == "scatter" else 1, 2.0 ** -8 if o["y_dtype"] == torch.bfloat16 else 0.0)
    print("%s/%s [%s K=%d bound %.3g]: %s; %.0f ms" % (cell, form, arith, k * k * Cin, bound, text, took * 1e3))
    REPORT["worst"][arith] = max(REPORT["worst"].get(arith, (0.0, "")), (worst * bound, "%s/%s" % (cell, form)))
    assert not torch.isnan(y).any().item(), (cell, form, "NaN left in y")
    assert worst <= 1.0, (cell, form, text)
    if band is not None:
        assert bands_intact(band[0], band[2]), (cell, form, "a byte outside the destination was written")
    # ---- the statistics slot
    am = getattr(y, "_mmt_amax", None)
    if f16 and form != "scatter":
        assert am is not None, (cell, form)
    if am is not None:
        assert am[1] == y._version and am[0].pool.dev[am[0].idx][0].item() == y.abs().max().item(), (cell, form)


@pytest.mark.parametrize("cell,form", G.cases(), ids=["%s-%s" % cf for cf in G.cases()])
def test_forward_case(hip, cell, form):
    t0 = time.time()
    run_forward(hip, cell, form)
    torch.cuda.synchronize()
    REPORT["times"].append((time.time() - t0, "%s-%s" % (cell, form)))


# ------------------------------------------------------------------------------------------ the weight gradient
def run_wgrad(H, cell, how):
    c = G.WCELLS[cell]
    N, Cin, Hh, W, Cout, k, s, p = c["shape"]
    o = G.wgrad_operands(cell)
    H.set_conv_precision(c["mode"])
    H.set_f16x2(bool(c["have"]))
    dw_ref, B, db_ref, db_B = (t.cuda() for t in G.wgrad_ref(o["x"], o["dy"], o["rowscale"], c["shape"]))
    arith, M = G.warithmetic(cell), G.edges_w(cell)["M"]
    bound = G.wbound_of(arith, M)
    njobs = 2 if how == "group2" else 1
    for start in ("zeros", "nonzero"):
        x, dy = cl(o["x"]), cl(o["dy"])
        if c["have"]:   # what the producers of the operands leave behind: recorded maxima, row-blocked planes
            for t in (x, dy):
                t._mmt_amax = H._amax_of(t)
                if c["have"] == "planes":
                    H.f16_split_pg(t)
        dw0 = torch.zeros(Cout, Cin, k, k) if start == "zeros" else o["dw0"]
        jobs, bands = [], []
        for j in range(njobs):
            band = banded((Cout, Cin, k, k), torch.float32, dw0.cuda())
            bias = torch.zeros(Cout, device="cuda")
            bands.append((band, bias))
            jobs.append((x, dy, (Cout, Cin, k, k), s, p, band[1], o["rowscale"].cuda(), bias))
        s0 = dict(H.F16_STATS)
        if how == "single":
            H.PROFILE, H.PROFILE_ALL = [], True
            try:
                H.conv_wgrad(*jobs[0])
                torch.cuda.synchronize()
                rec = H.PROFILE
            finally:
                H.PROFILE, H.PROFILE_ALL = None, False
        else:
            H.conv_wgrad_group(jobs)
            torch.cuda.synchronize()
        delta = {k_: H.F16_STATS.get(k_, 0) - s0.get(k_, 0) for k_ in ("wgrad", "wgrad_pl", "wgrad_grouped")}
        delta = {k_: v for k_, v in delta.items() if v}
        if how != "single":
            assert delta == ({"wgrad_grouped": njobs} if c["have"] else {}), (cell, how, delta)
        elif c["have"] == "planes":
            assert delta == {"wgrad_pl": 1}, (cell, delta)
        else:
            assert delta == ({"wgrad": 1} if c["have"] else {}), (cell, delta)
            assert len(rec) == 1 and rec[0][3][0] == "wgrad" and rec[0][4] == c["route"]["splits"], (cell, rec[0][3], rec[0][4])
        want, lim = dw_ref + dw0.double().cuda(), B + dw0.double().abs().cuda()
        for (band, bias) in bands:
            dw = band[1]
            ratio = (dw.double() - want).abs() / (bound * lim.clamp_min(G.TINY))
            ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
            worst, at = ratio.reshape(-1).max(0)
            co, ci, kh, kw_ = (int(v) for v in torch.unravel_index(at, ratio.shape))
            text = "ratio %.3g at (cout %d, cin %d, kh %d, kw %d): dw %.9g ref %.9g B %.3g" % (
                worst.item(), co, ci, kh, kw_, dw[co, ci, kh, kw_].item(), want[co, ci, kh, kw_].item(), lim[co, ci, kh, kw_].item())
            print("wgrad %s/%s/%s [%s M=%d bound %.3g]: %s" % (cell, how, start, arith, M, bound, text))
            key = "wgrad " + arith
            REPORT["worst"][key] = max(REPORT["worst"].get(key, (0.0, "")), (worst.item() * bound, "%s/%s/%s" % (cell, how, start)))
            assert worst.item() <= 1.0, (cell, how, start, text)
            assert bands_intact(band[0], band[2]), (cell, how, start, "a byte outside dw was written")
            berr = ((bias.double() - db_ref).abs() / (M ** 0.5 * 2.0 ** -24 * db_B.clamp_min(G.TINY))).max().item()
            assert berr <= 1.0, (cell, how, start, "dbias", berr)


WRUNS = [(cell, how) for cell, c in G.WCELLS.items() if cell not in G.WNOT_RUN
         for how in (("single", "group1", "group2") if c["have"] else ("single",))]


@pytest.mark.parametrize("cell,how", WRUNS, ids=["%s-%s" % ch for ch in WRUNS])
def test_wgrad_case(hip, cell, how):
    t0 = time.time()
    run_wgrad(hip, cell, how)
    torch.cuda.synchronize()
    REPORT["times"].append((time.time() - t0, "wgrad-%s-%s" % (cell, how)))


def test_report():
    """the worst error per arithmetic as a multiple of B, the slowest case and the total (printed: -s)"""
    for arith, (v, where) in sorted(REPORT["worst"].items()):
        print("worst |y - ref| / B, %s: %.3g (%s)" % (arith, v, where))
    if REPORT["times"]:
        print("cases: %d, total %.1f s, slowest %.2f s (%s)" % ((len(REPORT["times"]), sum(t for t, _ in REPORT["times"])) + max(REPORT["times"])))
        assert max(REPORT["times"])[0] < 10.0
