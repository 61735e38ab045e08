"""The convolution grid (tests/conv_grid_cases.py) against the library's route, on the host: every case reaches the cell it names, the
cells one step under a threshold land on the neighbour the table names, the (cell, form) pairs reached are the hand-written list, the
edges a cell claims hold on its inputs, and the error coefficients the GPU test holds the kernels to (COEFF) are what an emulation of
each arithmetic measures on the grid's own inputs.  The bare library as in tests/test_conv_route.py: no device, no launch."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conv_grid_cases as G  # noqa: E402
import conv_route_cases as C  # noqa: E402
import operand_prep_reference as R  # noqa: E402

SWITCHES = C.SWITCHES + ("MMT_WGRAD_PLANES", "MMT_WGRAD_GROUP")


@pytest.fixture()
def hip():
    from maskrcnn_benchmark import _hip as H
    L = ctypes.CDLL(H.LIB_PATH)   # (the bare library: no device, no launch)
    L.mmt_conv_route.argtypes = [ctypes.POINTER(H.ConvArgs), ctypes.c_int, ctypes.c_int, ctypes.POINTER(H.ConvRoute)]
    L.mmt_conv_wgrad_route.argtypes = [ctypes.POINTER(H.ConvArgs), ctypes.c_int, ctypes.POINTER(H.WgradRoute)]
    prev = L.mmt_get_conv_precision()
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    yield H, L
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    L.mmt_set_conv_precision(prev)


def block(H, cell, form, shape=None):
    """the argument block of a case as the binding fills it before it asks the route (maskrcnn_benchmark/_hip.py: conv_forward): x, y,
    the weight or only its planes (a dgrad form), the packed planes where the binding packs them (a split mode, Cin % 16 == 0,
    Cout > 32), the epilogue's operands and the storage bits"""
    c = G.CELLS[cell]
    N, Cin, Hh, W, Cout, k, s, p = shape or c["shape"]
    dgrad = form in G.DGRAD
    a = C.fill(H.ConvArgs, (N, Cin, Hh, W, Cout, k, s, p, 2 if form == "scatter" else 1, int(dgrad), 0), int(c["x_bf16"]), "kind", False)
    if form == "scatter":
        a.out_H, a.out_W = 2 * a.Ho - 1, 2 * a.Wo - 1
    if c["no_planes"] or c["mode"] == 0 or Cin % 16 or Cout <= 32:
        a.w_planes, a.w_plane_stride = None, 0
    if form == "affine_relu":
        a.scale, a.shift, a.relu = 0x5000, 0x6000, 1
    if form in ("res1", "dgrad_res", "bf16_io"):
        a.res, a.res_mode = 0xb000, 1
    if form in ("res2", "res3"):
        a.res, a.res_mode = 0xb000, int(form[3])
    if form in ("mask", "dgrad_mask", "bf16_io", "scatter"):
        a.mask, a.mask_scale = 0xc000, 1.5
    if form == "mul":
        a.mul, a.relu = 0xd000, 1
    if form == "bf16_io":
        a.io_bf16 = H.IO_X | H.IO_Y | H.IO_RES | H.IO_MASK
    return a


def ask(H, L, cell, form, shape=None):
    """the route of the launch the binding issues for the case (_hip._conv_kind): the fp16 split asks with the planes of x and the
    scalars promised; the library's dispatch in mode 3 is given planes of x when it would run the tap-strip kernel on them"""
    c = G.CELLS[cell]
    assert L.mmt_set_conv_precision(c["mode"]) == 0
    a, r = block(H, cell, form, shape), H.ConvRoute()
    if c["entry"] == "f16":
        assert L.mmt_conv_route(ctypes.byref(a), H.ENTRY_F16, H.ASSUME_X_PLANES | H.ASSUME_F16_SCALARS, ctypes.byref(r)) == 0
        return r
    if c["mode"] == 3 and not c["x_bf16"]:
        assert L.mmt_conv_route(ctypes.byref(a), H.ENTRY_LIB, H.ASSUME_X_PLANES, ctypes.byref(r)) == 0
        if r.family == H.ROUTE_STRIP:
            return r
    assert L.mmt_conv_route(ctypes.byref(a), H.ENTRY_LIB, 0, ctypes.byref(r)) == 0
    return r


def fields(r):
    """the fields a launch switches on.  pg_rows: of the plane-fed launch only -- elsewhere the route fills it with the plan the
    plane-fed kernel WOULD run (zero or not with the epilogue form), which no launch reads"""
    d = {f: getattr(r, f) for f in G.ROUTE_FIELDS}
    if r.family != G.PG:
        d["pg_rows"] = 0
    return d


def test_every_case_reaches_its_cell(hip):
    H, L = hip
    bad = []
    for cell, form in G.cases():
        r = ask(H, L, cell, form)
        c = G.CELLS[cell]
        if fields(r) != c["route"] or (c["panels"] is not None and r.panels != c["panels"]):
            bad.append((cell, form, fields(r), r.panels))
    assert not bad, "cases that no longer run on the cell they name (cell, form, the route's answer, panels): %r" % bad[:6]


def test_one_step_below_the_threshold_is_the_neighbour(hip):
    H, L = hip
    n = 0
    for cell, c in G.CELLS.items():
        if c["below"] is None:
            continue
        shape, other = c["below"]
        r = ask(H, L, cell, "plain", shape)
        assert fields(r) != c["route"], cell
        assert G.CELLS[other]["entry"] == c["entry"]
        want = dict(G.CELLS[other]["route"])
        got = fields(r)
        for f in ("family", "tag", "bm", "bn", "ksplit", "kgroups", "strip_tw", "x_form"):
            assert got[f] == want[f], (cell, "one step below lands on", got, "not on", other)
        n += 1
    assert n >= 10


# what the issue's list asks for, by (entry, family, bm, bn, split over K, strip width, K groups / all panels in a block): every one
# must be the launch class of a cell of the table (test_the_grid_covers_the_issues_list)
REQUIRED = {
    "FP32, Cin % 16 != 0": ("lib", G.FP32, 64, 64, False, 0, 1), "FP32 variant 0": ("lib", G.FP32, 128, 32, False, 0, 1),
    "SPLIT without planes": ("lib", G.SPLIT, 64, 64, False, 0, 1),
    "DMA variant 1": ("lib", G.DMA, 128, 128, False, 0, 1), "DMA variant 2": ("lib", G.DMA, 64, 64, False, 0, 1),
    "DMA variant 3": ("lib", G.DMA, 128, 64, False, 0, 1), "DMA split over K": ("lib", G.DMA, 128, 128, True, 0, 1),
    "DMA_BF16X": ("lib", G.DMA_BF16X, 64, 64, False, 0, 1), "ROWS": ("lib", G.ROWS, 128, 32, False, 0, 1), "C64": ("f16", G.C64, 0, 0, False, 0, 1),
    "STRIP 128": ("f16", G.STRIP, 256, 128, False, 128, 1), "STRIP 64": ("f16", G.STRIP, 256, 128, False, 64, 1),
    "STRIP 128, K ranges": ("lib", G.STRIP, 256, 128, True, 128, 1), "STRIP 64, K ranges": ("lib", G.STRIP, 256, 128, True, 64, 1),
    "PG 64": ("f16", G.PG, 64, 128, False, 0, 4), "PG 128": ("f16", G.PG, 128, 128, False, 0, 2), "PG 256": ("f16", G.PG, 256, 128, False, 0, 1),
    "PG 64, K ranges": ("f16", G.PG, 64, 128, True, 0, 4),
}


def launch_class(entry, r):
    return (entry, r["family"], r["bm"], r["bn"], r["ksplit"] > 1, r["strip_tw"] if r["family"] == G.STRIP else 0, r["kgroups"])


def feasible(cell, form):
    """can the binding issue the form on the cell's shape at all?  (Not a question to the route: it is about the operands.)  bf16
    storage is mode 1 with x stored as bf16; a planes-only weight needs packed planes (a split mode, Cin % 16 == 0, Cout > 32); res2
    needs a parent pixel for every pixel"""
    c = G.CELLS[cell]
    N, Cin, Hh, W, Cout, k, s, p = c["shape"]
    Ho, Wo = G.out_hw(c["shape"])
    if form == "bf16_io":
        return c["x_bf16"]
    if form in G.DGRAD:
        return not (c["no_planes"] or c["mode"] == 0 or Cin % 16 or Cout <= 32)
    return form != "res2" or (Ho % 2 == 0 and Wo % 2 == 0)


def test_admitted_forms_are_what_the_route_admits(hip):
    """per cell, the forms of FORMS for which the route still answers the cell (asked form by form with the block the binding fills)
    == the hand-written admitted(cell); a form the predicate gained or lost fails here with the cell's name.  And every admitted pair
    is a case of the grid"""
    H, L = hip
    wrong = {}
    for cell, c in G.CELLS.items():
        got = set()
        for form in G.FORMS:
            if not feasible(cell, form):
                continue
            r = ask(H, L, cell, form)
            if fields(r) == c["route"] and (c["panels"] is None or r.panels == c["panels"]):
                got.add(form)
        if got != set(G.admitted(cell)):
            wrong[cell] = (sorted(got - set(G.admitted(cell))), sorted(set(G.admitted(cell)) - got))
    assert not wrong, "cell: (forms the route admits that the table lacks, forms listed that the route sends elsewhere): %r" % wrong
    assert set(G.cases()) == {(cell, f) for cell in G.CELLS for f in G.admitted(cell)}
    assert {f for _, f in G.cases()} == set(G.FORMS)


def test_the_grid_covers_the_issues_list():
    have = {launch_class(c["entry"], c["route"]) for c in G.CELLS.values()}
    missing = [name for name, k in REQUIRED.items() if k not in have]
    assert not missing, missing
    assert {c["panels"] == -(-c["shape"][4] // 32) for c in G.CELLS.values() if c["route"]["family"] == G.ROWS} == {True, False}
    assert any(c["x_bf16"] and c["route"]["family"] == G.STRIP and c["route"]["ksplit"] == 1 for c in G.CELLS.values())
    assert {G.arithmetic(c) for c in G.CELLS} == {"fp32", "bf16", "bf16x2", "bf16x3", "f16x2"}


def test_the_production_grid_lands_on_listed_cells(hip):
    """every launch class (entry, family, tile, split over K or not, strip width, K groups) the route answers over the shapes of the
    detectors (tests/conv_route_cases.py) is the class of a cell of the table: a new kernel or tile with no numeric case fails here"""
    H, L = hip

    cls = launch_class
    have = {cls(c["entry"], c["route"]) for c in G.CELLS.values()}
    missing = {}
    r = H.ConvRoute()
    for mode in (0, 1, 2, 3):
        assert L.mmt_set_conv_precision(mode) == 0
        for case in C.cases():
            a = C.fill(H.ConvArgs, case, 0, "launch", False)
            if mode == 0 or case[1] % 16 or case[4] <= 32:
                a.w_planes = None
            a.x_planes = None
            if mode == 3:
                assert L.mmt_conv_route(ctypes.byref(a), H.ENTRY_F16, H.ASSUME_X_PLANES, ctypes.byref(r)) == 0
                if r.family != H.ROUTE_NONE:
                    k = cls("f16", fields(r))
                    if k not in have:
                        missing.setdefault(k, case)
            assert L.mmt_conv_route(ctypes.byref(a), H.ENTRY_LIB, 0, ctypes.byref(r)) == 0
            k = cls("lib", fields(r))
            if k not in have:
                missing.setdefault(k, case)
    assert not missing, "launch classes without a cell (class: first shape): %r" % missing


def test_edges_hold_on_the_inputs():
    seen = {"single_k_step": 0, "map_1x1": 0, "fc": 0}
    for cell, c in G.CELLS.items():
        e = G.edges(cell)
        N, Cin, Hh, W, Cout, k, s, p = c["shape"]
        fam = c["route"]["family"]
        if fam == G.STRIP:      # the predicate demands whole tiles of pixels; the channels hang over where K is not split
            assert e["m_overhang"] == 0 and (e["n_overhang"] != 0) == (c["route"]["ksplit"] == 1), cell
        elif fam != G.C64 and cell not in ("dma_1x1map",):
            assert e["n_overhang"] != 0, cell
            assert e["m_overhang"] != 0 or fam == G.ROWS and cell == "f16_rows_groups", cell
        if k == 3:
            assert N >= 2, cell
            if fam not in (G.STRIP, G.C64) and not e["map_1x1"]:
                assert e["tile_crosses_image"] and e["last_tile_spans_rows"], (cell, e)
        for key in ("single_k_step", "map_1x1"):
            seen[key] += bool(e[key])
        seen["fc"] += e["K"] == 12544
        for form in G.admitted(cell):
            o = G.operands(cell, form) if e["M"] * Cin < (1 << 20) else None
            if o is None:
                continue
            x, w = o["x"].float(), o["w"].float()
            if N >= 2:      # the scaled-down regions are there: last image, first channel slab, last block of output channels
                assert x[-1].abs().max() <= 0.05 * x[0].abs().max() + 1e-30, (cell, form)
            if Cin > 16:
                assert x[0, :16].abs().max() <= 0.05 * x[0, 16:].abs().max(), (cell, form)
            nb = ((Cout - 1) % 32) + 1
            if Cout > nb:
                assert w[-nb:].abs().max() <= 0.05 * w[:-nb].abs().max(), (cell, form)
            if form not in G.DGRAD:
                assert (x >= 0).all()
    assert all(v >= 1 for v in seen.values()), seen
    for cell, c in G.WCELLS.items():
        if cell in G.WNOT_RUN:
            continue
        o = G.wgrad_operands(cell)
        if c["shape"][0] >= 2:
            assert o["x"][-1].float().abs().max() <= 0.05 * o["x"][0].float().abs().max(), cell
    assert any(c["have"] == "planes" and c["shape"][0] >= 2 for c in G.WCELLS.values())


def test_weight_gradient_cases_reach_their_cells(hip):
    H, L = hip
    r = H.WgradRoute()
    have = {"": 0, "maxima": H.WG_HAVE_MAXIMA, "planes": H.WG_HAVE_MAXIMA | H.WG_HAVE_PLANES}
    fams, splits = set(), set()
    for cell, c in G.WCELLS.items():
        assert L.mmt_set_conv_precision(c["mode"]) == 0
        N, Cin, Hh, W, Cout, k, s, p = c["shape"]
        a = C.fill(H.ConvArgs, (N, Cin, Hh, W, Cout, k, s, p, 1, 0, 0), 0, "shape", False)
        a.io_bf16 = (H.IO_X if c["x_bf16"] else 0) | (H.IO_DY if c["dy_bf16"] else 0)
        assert L.mmt_conv_wgrad_route(ctypes.byref(a), have[c["have"]], ctypes.byref(r)) == 0
        got = {f: getattr(r, f) for f in G.WROUTE_FIELDS}
        assert got == c["route"], (cell, got)
        fams.add((r.family, r.terms, r.decode if r.family == G.WG_PIPE_F16 else -1))
        splits.add(r.splits > 1)
        if cell in G.WNOT_RUN:
            continue
        assert N * Cin * Hh * W < (1 << 22), cell   # (below WGRAD_F16_MIN_ELEMS: the binding takes no reduction pass of its own)
    want = {(G.WG_PLANES_1, 2, -1), (G.WG_PLANES_3, 2, -1), (G.WG_PIPE_F16, 2, 0), (G.WG_PIPE_F16, 2, 1), (G.WG_PIPE_F16, 2, 2),
            (G.WG_PIPE, 1, -1), (G.WG_PIPE, 2, -1), (G.WG_PIPE, 3, -1), (G.WG_SPLIT, 2, -1), (G.WG_FP32_FAST, 0, -1), (G.WG_FP32_SLOW, 0, -1)}
    assert fams == want and splits == {True, False}
    assert {c["route"]["bf"] for c in G.WCELLS.values()} == {0, 1, 2, 3} and {c["route"]["vec4"] for c in G.WCELLS.values()} == {0, 1}


# ------------------------------------------------------------------------------------------ the coefficients
def split_terms(a, arith, amax=None):
    """the operand as the terms the kernels multiply, fp32 tensors whose sum is (nearly) a: tests/operand_prep_reference.py's splits"""
    shape = a.shape
    if arith == "fp32":
        return [a.float()], 1.0
    if arith == "bf16":
        return [a.float().bfloat16().float()], 1.0
    if arith in ("bf16x2", "bf16x3"):
        p = R.split_bf16x3(a.float())
        return [p[i].float().reshape(shape) for i in range(2 if arith == "bf16x2" else 3)], 1.0
    s = R.f16_scale_of(a.float().abs().max().item() if amax is None else amax)
    p = R.split_f16x2(a.float(), s)
    return [p[0].float().reshape(shape), p[1].float().reshape(shape)], s


def kept(arith):
    """(i, j) of the products x_i w_j a kernel adds up: all with i + j < the number of terms"""
    n = {"fp32": 1, "bf16": 1, "bf16x2": 2, "bf16x3": 3, "f16x2": 2}[arith]
    return [(i, j) for i in range(n) for j in range(n) if i + j < n]


STEP = {"fp32": 2, "bf16": 16, "bf16x2": 16, "bf16x3": 16, "f16x2": 16}   # reduction elements one MFMA adds to the accumulator


def emulate(a, b, arith):
    """a (rows, R), b (cols, R) fp32 -> the (rows, cols) sums over R as a kernel forms them: both operands split into their terms, ONE
    fp32 accumulator per output element, into which every kept product of every STEP reduction elements is added in turn (the sum
    inside a step exact, as an MFMA forms it; torch's fp64 matmul of <= 16 products of 24-bit numbers is), divided by the scales"""
    at, sa = split_terms(a, arith)
    bt, sb = split_terms(b, arith)
    at, bt = [t.double() for t in at], [t.double().t().contiguous() for t in bt]
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    step = STEP[arith]
    for r0 in range(0, a.shape[1], step):
        for i, j in kept(arith):
            acc = acc + (at[i][:, r0:r0 + step] @ bt[j][r0:r0 + step]).float()
    return acc.double() / (sa * sb)


def crop(x, k, rows=2048):
    """at most `rows` output pixels per image of x (the top rows of every image: the inputs are independent draws), the last image kept"""
    N, Cin, Hh, W = x.shape
    if Hh * W <= rows:
        return x
    return x[:, :, :max(rows // W, k), :]


def measure_forward(cell):
    c = G.CELLS[cell]
    N, Cin, Hh, W, Cout, k, s, p = c["shape"]
    o = G.operands(cell, "plain")
    x, w = crop(o["x"].float(), k), o["w"].float()
    Ho, Wo = G.out_hw(c["shape"])
    want = 2048 if k * k * Cin <= 2304 else 512       # output pixels a coefficient is measured on, whatever the cell's own size:
    if N * Ho * Wo < want and not c["x_bf16"]:        # the worst of few elements says little, so a small case gets more images drawn the same way
        more = torch.randn(-(-(want - N * Ho * Wo) // (Ho * Wo)), Cin, Hh, W, generator=G._gen("emulation/" + cell)).relu()
        more[:, :16] *= G.DOWN
        x = torch.cat([x, more])
    acc, mag = (t.permute(0, 2, 3, 1).reshape(-1, Cout) for t in G.products(x, w, s, p))
    cols = F.unfold(x, (k, k), padding=p, stride=s).permute(0, 2, 1).reshape(-1, Cin * k * k)
    emu = emulate(cols, w.reshape(Cout, -1), G.arithmetic(cell))
    return ((emu - acc).abs() / mag.clamp_min(G.TINY)).max().item()


def measure_wgrad(cell):
    c = G.WCELLS[cell]
    N, Cin, Hh, W, Cout, k, s, p = c["shape"]
    o = G.wgrad_operands(cell)
    x, dy = o["x"].float(), o["dy"].float()
    dw, B, _, _ = G.wgrad_ref(x, dy, torch.ones(Cout), c["shape"])
    cols = F.unfold(x, (k, k), padding=p, stride=s).permute(1, 0, 2).reshape(Cin * k * k, -1)     # (K, pixels)
    emu = emulate(dy.permute(1, 0, 2, 3).reshape(Cout, -1), cols, G.warithmetic(cell)).reshape(Cout, Cin, k, k)
    return ((emu - dw).abs() / B.clamp_min(G.TINY)).max().item()


def measured_table():
    out = {}
    for cell, c in G.CELLS.items():
        N, Cin, Hh, W, Cout, k, s, p = c["shape"]
        key = (G.arithmetic(cell), k * k * Cin)
        out[key] = max(out.get(key, 0.0), measure_forward(cell))
    wout = {}
    for cell, c in G.WCELLS.items():
        if cell in G.WNOT_RUN:
            continue
        key = (G.warithmetic(cell), G.edges_w(cell)["M"])
        wout[key] = max(wout.get(key, 0.0), measure_wgrad(cell))
    return out, wout


def test_coefficients_are_what_the_emulation_measures():
    fwd, wg = measured_table()
    print("forward:", {k: "%.3g" % v for k, v in sorted(fwd.items())})
    print("wgrad:", {k: "%.3g" % v for k, v in sorted(wg.items())})
    assert set(fwd) == set(G.COEFF) and set(wg) == set(G.WCOEFF), (sorted(set(fwd) ^ set(G.COEFF)), sorted(set(wg) ^ set(G.WCOEFF)))
    for table, got in ((G.COEFF, fwd), (G.WCOEFF, wg)):
        for key, c in table.items():
            assert 0.5 * c <= got[key] <= 1.25 * c, (key, "table", c, "measured", got[key])
    # which cases need more than the project's 3e-6, and that no other does
    for (arith, K), c in list(G.COEFF.items()) + list(G.WCOEFF.items()):
        if arith != "bf16x2":   # (the two-term bf16 split sits AT 3e-6: 1.9e-6 ... 3.1e-6, from the dropped x1 w1 product)
            assert (c > G.PROJECT_BOUND) == (arith == "bf16"), (arith, K, c)


def test_unfold_products_are_the_convolution():
    """the fp64 unfold + matmul form of the products (the GPU test runs it on the device for the large cases) against F.conv2d"""
    o = G.operands("dma_v2_m3", "plain")
    a = G.products(o["x"], o["w"], 1, 1)
    b = G.products_unfold(o["x"], o["w"], 1, 1)
    for u, v in zip(a, b):
        assert (u - v).abs().max().item() <= 1e-13 * a[1].max().item()
    x = torch.randn(2, 16, 9, 11, generator=torch.Generator().manual_seed(3))
    w = torch.randn(8, 16, 3, 3, generator=torch.Generator().manual_seed(4))
    a, b = G.products(x, w, 2, 1), G.products_unfold(x, w, 2, 1)
    assert (a[0] - b[0]).abs().max().item() <= 1e-13 * a[1].max().item()


def test_reference_epilogue_on_a_hand_example():
    """conv_ref's epilogue against the library's scalar statement of it (csrc/conv_shared.h: conv_epilogue_finish), spelled out per
    element on a 1x1 case small enough to loop over"""
    g = torch.Generator().manual_seed(11)
    x, w = torch.randn(1, 4, 4, 6, generator=g), torch.randn(3, 4, 1, 1, generator=g)
    top, fine = torch.randn(1, 3, 2, 3, generator=g), torch.randn(1, 3, 8, 12, generator=g)
    msk = torch.randn(1, 3, 7, 11, generator=g)
    base = dict(scale=torch.rand(3, generator=g) + 0.5, shift=torch.randn(3, generator=g), relu=True, res=top, res_mode=2, mask=None,
                mask_scale=1.0, mul=None, out_stride=1, out_hw=None)
    v, B = G.conv_ref(x, w, base, 1, 0)
    raw = torch.einsum("nchw,oc->nohw", x.double(), w[:, :, 0, 0].double())
    for h in range(4):
        for q in range(6):
            for co in range(3):
                e = raw[0, co, h, q] * base["scale"][co].double() + base["shift"][co].double() + top[0, co, h >> 1, q >> 1].double()
                assert abs(v[0, co, h, q] - max(e, 0)) <= 1e-14 and B[0, co, h, q] >= abs(e) - 1e-14
    o3 = dict(base, scale=None, shift=None, relu=False, res=fine, res_mode=3)
    v, _ = G.conv_ref(x, w, o3, 1, 0)
    assert abs(v[0, 1, 2, 3] - (raw[0, 1, 2, 3] + fine[0, 1, 4:6, 6:8].double().sum())) <= 1e-14
    sc = dict(base, scale=None, shift=None, relu=False, res=None, res_mode=0, mask=msk, mask_scale=1.5, out_stride=2, out_hw=(7, 11))
    v, B = G.conv_ref(x, w, sc, 1, 0)
    assert v.shape == (1, 3, 7, 11) and (v[:, :, 1::2] == 0).all() and (v[:, :, :, 1::2] == 0).all()
    assert abs(v[0, 2, 4, 6] - (raw[0, 2, 2, 3] * 1.5 if msk[0, 2, 4, 6] > 0 else 0.0)) <= 1e-14
    assert ((B == 0) == (v == 0)).all()
