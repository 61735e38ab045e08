"""Who owns the derived forms of a weight (packed bf16 / fp16 planes, the flipped fp32 tensor): a flattened model's FlatParams for
its parameters (engine/flat.py: `form`), `_hip.LOOSE` for everything else.  Neither may serve what belonged to a dead owner, nor
what a raw-pointer update (the library's SGD / EMA kernels: no version counter moves) made stale."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu


def cl(x):
    return x.cuda().contiguous(memory_format=torch.channels_last)


def dead_owners(H):
    """registry entries, of either kind, whose owner is gone: there must be none"""
    return [k for k, e in H.LOOSE.entries.items() if e.ref() is None] + ["FLATS"] * (len(H.FLATS) - len(list(H.FLATS.items())))


@pytest.fixture
def H():
    from maskrcnn_benchmark import _hip
    _hip.lib()
    mode = _hip.get_conv_precision()
    _hip.set_conv_precision(3)
    yield _hip
    _hip.set_f16x2(None)
    _hip.set_conv_precision(mode)


@pytest.mark.parametrize("f16x2", [False, True])
def test_rebuilt_model_never_sees_its_predecessors_forms(H, f16x2):
    """build -> steps -> free -> build -> steps in one process, without emptying the allocator's cache: buffers (and Python ids) come
    back, every round ends at the same plane generation, and every round's forward and data gradients must be its OWN weights'.
    (With the caches this replaced the data gradient was off by the factors below in EVERY round: the first layer's flipped fp32 weights,
    kept by tensor version alone, did not follow `flat.data.mul_` + `refresh_planes`; no address or id repeated in that run.)"""
    from maskrcnn_benchmark.layers import Conv2d
    from maskrcnn_benchmark.engine.flat import flatten_model
    H.set_f16x2(f16x2)
    ptrs, ids, repeated = set(), set(), {"address": False, "id": False}

    def run(m, x):
        xx = x.clone().requires_grad_(True)
        y = m[1](m[0](xx, relu=True), input_relu=True)
        y.sum().backward()
        return y.detach(), xx.grad

    def ref(m, x):
        xx = x.double().clone().requires_grad_(True)
        y = F.conv2d(F.relu(F.conv2d(xx, m[0].weight.double(), m[0].bias.double(), 1, 1)), m[1].weight.double(), m[1].bias.double())
        y.sum().backward()
        return y.detach(), xx.grad

    for rnd in range(3):
        torch.manual_seed(40 + rnd)
        m = nn.Sequential(Conv2d(32, 64, 3, 1, 1), Conv2d(64, 48, 1, 1, 0)).cuda()
        flat = flatten_model(m)
        x = cl(torch.randn(2, 32, 20, 20))
        run(m, x)   # registers the data-gradient forms
        for f in (1.5 + rnd, 0.5):
            flat.data.mul_(f)
            flat.refresh_planes()
        assert flat.plane_gen == 3
        repeated["address"] |= flat.data.data_ptr() in ptrs
        repeated["id"] |= id(flat) in ids
        ptrs.add(flat.data.data_ptr())
        ids.add(id(flat))
        (y, gx), (yr, gr) = run(m, x), ref(m, x)
        assert (y.double() - yr).abs().max().item() < 1e-5 * yr.abs().max().item(), rnd
        assert (gx.double() - gr).abs().max().item() < 1e-5 * gr.abs().max().item(), rnd
        mine = list(flat.records)
        assert mine and all(H.FLATS.get(q) is flat for q in mine)
        del m, flat, x, y, gx, yr, gr
        assert dead_owners(H) == [] and not any(q in H.FLATS for q in mine), rnd   # the owner took its registry entries with it
    print("repeated across rounds:", repeated)


FORMS = {
    "f16": lambda H, w: H.f16_weight_planes(w),
    "f16_dgrad": lambda H, w: H.f16_weight_planes(w, flipped=True),
    "f32_dgrad": lambda H, w: (H.weight_flip_transpose(w.detach(), owner=w),),
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_loose_weight_follows_a_raw_pointer_update(H, form):
    """a Parameter outside every flat buffer: each form is packed once, and packed again after the library's SGD kernel rewrote the
    weight through raw pointers; a loose tensor outside the written range keeps its planes where they are.  (With the per-form caches
    this replaced, "f16" and "f16_dgrad" came back bit-equal to the planes packed BEFORE the update; only the fp32 form followed it.)"""
    H.set_f16x2(True)
    get = FORMS[form]
    g = torch.Generator().manual_seed(7)
    w = nn.Parameter(cl(torch.randn(64, 64, 3, 3, generator=g)))
    stem = cl(torch.randn(64, 16, 4, 4, generator=g))   # (shaped like the frozen stem's space-to-depth filter)
    k0 = H.F16_STATS["weight_pack"]
    a = get(H, w)
    c0 = H.C_CALLS[0]
    b = get(H, w)
    assert H.C_CALLS[0] == c0 and all(p is q or p.data_ptr() == q.data_ptr() for p, q in zip(a, b))   # one pack for two calls
    assert H.F16_STATS["weight_pack"] - k0 == (0 if form == "f32_dgrad" else 1)
    sp, ss = H.f16_weight_planes(stem)
    v0, c0 = w._version, H.C_CALLS[0]
    H.sgd_momentum(w.detach(), torch.ones_like(w), torch.zeros_like(w), 0.5, 0.0, 0.9, True)
    assert w._version == v0
    sp2, ss2 = H.f16_weight_planes(stem)
    assert H.C_CALLS[0] - c0 == 1 and sp2.data_ptr() == sp.data_ptr() and ss2.data_ptr() == ss.data_ptr()   # nobody wrote `stem`
    c = get(H, w)
    fresh = get(H, nn.Parameter(w.detach().clone()))
    assert len(c) == len(fresh)
    for i, (p, q) in enumerate(zip(c, fresh)):
        assert torch.equal(p, q), "%s: stale tensor %d served after a raw-pointer update" % (form, i)
    del w, a, b, c, fresh, stem, sp, ss, sp2, ss2
    assert dead_owners(H) == []


def test_loose_flip_of_a_flat_weight_without_planes_follows_the_buffer(H):
    """a flat model's parameter the buffer packs no planes for (the RPN predictors: Cout 15) is in no registry of packed matrices;
    its flipped fp32 weights are a loose form, kept between two updates and stale after `flat.data` moved under a refresh"""
    from maskrcnn_benchmark.layers import Conv2d
    from maskrcnn_benchmark.engine.flat import flatten_model
    torch.manual_seed(9)
    m = nn.Sequential(Conv2d(256, 64, 1, 1, 0), Conv2d(256, 15, 1, 1, 0)).cuda()   # (one matrix with planes, one without)
    flat = flatten_model(m)
    w = m[1].weight
    assert m[0].weight.data_ptr() in H.FLATS
    assert w.data_ptr() not in H.FLATS and H.pack_weight_flipped(w) is None
    a = H.weight_flip_transpose(w.detach(), owner=w)
    c0 = H.C_CALLS[0]
    assert H.weight_flip_transpose(w.detach(), owner=w) is a and H.C_CALLS[0] == c0
    v0 = w._version
    flat.data.mul_(1.5)
    flat.refresh_planes()
    assert w._version == v0
    b = H.weight_flip_transpose(w.detach(), owner=w)
    assert torch.equal(b, w.detach().flip(2, 3).transpose(0, 1)) and not torch.equal(b, a)


def test_fresh_view_of_a_flat_weight_is_served_from_the_bulk_planes(H):
    """a Linear layer hands its weight over as a new 4-D view on every call: both calls are served from the buffer's planes"""
    from maskrcnn_benchmark.engine.flat import flatten_model
    H.set_f16x2(True)
    torch.manual_seed(3)
    lin = nn.Linear(64, 48).cuda()
    flat = flatten_model(lin)
    lo = flat.planes16.data_ptr()
    hi = lo + flat.planes16.numel() * 2
    c0, k0 = H.C_CALLS[0], H.F16_STATS["weight_pack"]
    p1, s1 = H.f16_weight_planes(lin.weight.view(48, 64, 1, 1))
    p2, s2 = H.f16_weight_planes(lin.weight.view(48, 64, 1, 1))
    b1, b2 = flat.form(lin.weight.view(48, 64, 1, 1), "bf16"), flat.form(lin.weight.view(48, 64, 1, 1), "bf16")
    assert H.C_CALLS[0] == c0 and H.F16_STATS["weight_pack"] == k0
    assert lo <= p1.data_ptr() < hi and p2.data_ptr() == p1.data_ptr() and s2.data_ptr() == s1.data_ptr()
    assert b1 is not None and b2.data_ptr() == b1.data_ptr() and b1.untyped_storage().data_ptr() == flat.planes.untyped_storage().data_ptr()
    # ... and they are the weight's planes: the same bits as a per-call pack of a copy
    q1, t1 = H.f16_weight_planes(cl(lin.weight.detach().view(48, 64, 1, 1).clone()))
    assert torch.equal(p1, q1) and torch.equal(s1, t1)
