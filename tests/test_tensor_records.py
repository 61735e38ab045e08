"""What producers leave on tensor objects (`_mmt_amax`, `_mmt_rb`, `_mmt_planes`) and the site table of the row-blocked plane scales,
host side (no GPU): who voids the records, what `carry` takes along, what a launch is handed for a record, which slots the lagged site
test queues, and a site's life cycle against a library stub."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mmt-psm_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

CPU = torch.device("cpu")


class _Lib(object):
    """stands for the loaded library: notes every call and answers 0; a route query says that the kernel writes row-blocked planes"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            if name == "mmt_conv_route":
                args[3]._obj.writes_rb = 1
            return 0
        return f

    def named(self, name):
        return [a for n, a in self.calls if n == name]


@pytest.fixture()
def hip(monkeypatch):
    from maskrcnn_benchmark import _hip as H
    stub = _Lib()
    monkeypatch.setattr(H, "lib", lambda: stub)
    monkeypatch.setattr(H, "_stream", lambda: 0)
    monkeypatch.setattr(H, "_DET", False)
    monkeypatch.setattr(H, "RB_EPI", True)
    H.rb_reset()
    yield H, stub
    H.rb_reset()


def _full(H, x):
    """x with all three records, as producers leave them -> (slot, bf16 planes, row-blocked planes, scale)"""
    slot = torch.zeros(1)
    x._mmt_amax = (slot, x._version)
    bf = torch.arange(3 * x.numel(), dtype=torch.float32).reshape(3, x.numel()).to(torch.bfloat16)
    x._mmt_planes = (bf, x._version)
    rb = torch.arange(2 * x.numel(), dtype=torch.float32).reshape(2, x.numel()).to(torch.float16)
    sc = torch.ones(1)
    H._rb_attach(x, rb, sc, "epi")
    return slot, bf, rb, sc


def _none(H, x):
    return H._recorded(x) is None and H._rb_of(x) is None and H.planes_of(x) is None


def test_a_modified_or_dropped_tensor_carries_nothing(hip):
    H, _ = hip
    x = torch.zeros(4, 2, 3, 3)
    slot, bf, rb, sc = _full(H, x)
    assert H._recorded(x)[0] is slot and H.planes_of(x) is bf
    r = H._rb_of(x)
    assert len(r) == 5 and r[0] is rb and r[1] is sc and r[2] == x._version and r[3] == "epi" and r[4] is None
    x.add_(1.0)
    assert _none(H, x)
    _full(H, x)
    assert not _none(H, x)
    H.drop(x)
    assert _none(H, x)
    assert x._mmt_amax is None and x._mmt_rb is None and x._mmt_planes is None


def test_carry_takes_batch_slices_by_whole_images(hip):
    H, _ = hip
    x = torch.zeros(4, 2, 3, 3)
    per = 18
    slot, bf, rb, sc = _full(H, x)
    d = x[1:3]
    H.carry(x, d, images=(1, 3))
    assert H._recorded(d)[0] is slot
    assert torch.equal(H.planes_of(d), bf[:, per:3 * per])
    r = H._rb_of(d)
    assert torch.equal(r[0], rb[:, per:3 * per]) and r[0].data_ptr() == rb[:, per:].data_ptr()
    assert r[1] is sc and r[2] == d._version and r[3] == "epi" and r[4] is None
    # a view of the whole tensor: everything as it is
    v = x.view(4, 2, 9, 1)
    H.carry(x, v)
    assert H._recorded(v)[0] is slot and H.planes_of(v) is bf and H._rb_of(v)[0] is rb and H._rb_of(v)[3:] == ("epi", None)


def test_carry_inside_planes_of_the_leading_images(hip):
    H, _ = hip
    x = torch.zeros(4, 2, 3, 3)
    per = 18
    slot, bf, rb, sc = _full(H, x)
    H._rb_attach(x, rb[:, :3 * per], sc, "epi", 3)
    d = x[1:3]
    H.carry(x, d, images=(1, 3))
    r = H._rb_of(d)
    assert torch.equal(r[0], rb[:, per:3 * per]) and r[3] == "epi" and r[4] is None     # the slice is covered as a whole
    e = x[2:4]
    H.carry(x, e, images=(2, 4))
    assert H._rb_of(e) is None                                                           # image 3 has no planes
    assert H._recorded(e)[0] is slot and torch.equal(H.planes_of(e), bf[:, 2 * per:])    # (the other two records do not depend on it)
    v = x.view(4, 2, 9, 1)
    H.carry(x, v)
    assert H._rb_of(v)[3:] == ("epi", 3)                                                 # an alias keeps what is covered


def test_carry_switches_and_carry_stats(hip):
    H, _ = hip
    x = torch.zeros(4, 2, 3, 3)
    slot, bf, rb, sc = _full(H, x)
    a, b, c = x.view(4, 18), x.view(4, 18), x.view(4, 18)
    H.carry(x, a, rb=False)
    assert H._recorded(a)[0] is slot and H.planes_of(a) is bf and H._rb_of(a) is None
    H.carry(x, b, planes=False)
    assert H._recorded(b)[0] is slot and H.planes_of(b) is None and H._rb_of(b)[0] is rb
    H.carry_stats(x, c)
    assert H._recorded(c)[0] is slot and H.planes_of(c) is None and H._rb_of(c) is None
    x.add_(1.0)                                   # stale: nothing goes along
    d = torch.zeros(4, 18)
    H.carry_stats(x, d)
    H.carry(x, d)
    assert _none(H, d) and getattr(d, "_mmt_amax", None) is None


def _plan_slot(H, idx=3):
    plan = object.__new__(H.LaunchPlan)          # (no device: the fields a slot looks at)
    plan.base, plan.gen, plan.pool = 4096, 0, None
    return H._Slot(plan, idx)


def _pool_slot(H, idx=3):
    pool = object.__new__(H._StatPool)
    pool.base, pool.gen, pool.host_gen, pool.event = 8192, 0, -1, None
    return H._Slot(pool, idx)


def test_what_a_launch_is_handed_for_a_record(hip, monkeypatch):
    """the weight gradient's job: the address of the maximum always, the full slot as the guard only where there is one"""
    H, _ = hip
    monkeypatch.setattr(H, "F16X2", True)
    monkeypatch.setattr(H, "_PREC", 3)
    x, dy, dw = torch.zeros(2, 4, 3, 3), torch.zeros(2, 8, 3, 3), torch.zeros(8, 4, 1, 1)
    one = torch.zeros(1)
    slot = _pool_slot(H)
    assert slot.data_ptr() == slot.ptr == 8192 + 3 * 4 * H.STAT_W
    x._mmt_amax = (one, x._version)
    dy._mmt_amax = (slot, dy._version)
    try:
        j, r, f16, alive = H._wgrad_job(x, dy, (8, 4, 1, 1), 1, 0, dw, None, None, 0)
        assert f16 and alive == ()
        assert j.a.f16_x_amax == one.data_ptr() and j.a.f16_guard_x is None
        assert j.a.f16_dy_amax == slot.ptr and j.a.f16_guard_dy == slot.ptr
        dy.add_(1.0)                               # a stale record is no record
        j, r, f16, alive = H._wgrad_job(x, dy, (8, 4, 1, 1), 1, 0, dw, None, None, 0)
        assert not f16 and j.a.f16_x_amax is None and j.a.f16_guard_dy is None
    finally:
        H._SITES.pop(("wgx", dw.data_ptr()), None)
        H._SITES.pop(("wgd", dw.data_ptr()), None)
        H._WPLAN.clear()


def test_site_test_queues_slots_that_travel_only(hip):
    H, _ = hip
    x = torch.zeros(4)
    cases = ((_plan_slot(H), False), (_pool_slot(H), True), (torch.zeros(1), False))
    for n, (slot, queued) in enumerate(cases):
        site = ("test-records", n)
        x._mmt_amax = (slot, x._version)
        try:
            assert H._site_ok(site, x, count=False) is True
            assert (H._SITES[site][1] is slot) if queued else (H._SITES[site][1] is None)
        finally:
            H._SITES.pop(site, None)


def _produce(H, key, y):
    a = H.ConvArgs()
    return a, H._rb_produce(a, y, key)


def test_site_life_cycle(hip):
    H, lib = hip
    y = torch.zeros(2, 16, 3, 3)
    a, got = _produce(H, ("site", 1), y)
    state = H._RB[CPU.index].state
    assert got is None and a.y_amax_next and not a.y_rb and not lib.calls       # a new site: the pending maximum alone
    b, got = _produce(H, ("site", 2), y)
    assert got is None and b.y_amax_next not in (None, a.y_amax_next)
    epoch = H._RB_EPOCH[0]
    H.rb_scales_update()
    assert lib.named("mmt_rb_scales_update") == [(state.data_ptr(), 2, 0)]      # the table's base, its two sites
    assert H._RB_EPOCH[0] == epoch + 1
    H.rb_scales_update()                                                        # nothing produced since
    assert len(lib.named("mmt_rb_scales_update")) == 1 and H._RB_EPOCH[0] == epoch + 1
    a2, got = _produce(H, ("site", 1), y)                                       # ready: the route is asked, the planes are made
    assert len(lib.named("mmt_conv_route")) == 1
    pl, view, images = got
    assert images is None and tuple(pl.shape) == (2, y.numel()) and pl.dtype == torch.float16
    assert a2.y_rb == pl.data_ptr() and a2.y_rb_stride == y.numel() and a2.y_rb_rows == 0
    assert a2.y_amax_next == a.y_amax_next and a2.y_rb_scale == view.data_ptr() and a2.y_amax_next == a2.y_rb_scale + 4
    _, got = _produce(H, ("site", 1), y)
    assert got[1] is view and len(lib.named("mmt_conv_route")) == 1             # (both answers are kept)
    # planes for the leading image only
    a3, got = _produce(H, ("site", 1, H.RbLead(1)), y)
    assert got[2] == 1 and tuple(got[0].shape) == (2, y.numel() // 2) and a3.y_rb_rows == 9 and a3.y_rb_scale == a2.y_rb_scale
    H.rb_scales_update()                                                        # produced again, nobody new: no new epoch
    assert len(lib.named("mmt_rb_scales_update")) == 2 and H._RB_EPOCH[0] == epoch + 1
    # a third site after the update is not ready until the next one
    c, got = _produce(H, ("site", 3), y)
    assert got is None and len(lib.named("mmt_conv_route")) == 1
    H.rb_scales_update()
    assert lib.named("mmt_rb_scales_update")[-1] == (state.data_ptr(), 3, 0) and H._RB_EPOCH[0] == epoch + 2
    H.rb_reset()
    assert H._RB == {} and H._RB_EPOCH[0] == epoch + 3


def test_site_layout_through_the_device_view(hip):
    H, lib = hip
    y = torch.zeros(1, 16, 2, 2)
    for k in range(3):
        _produce(H, ("site", k), y)
    H.rb_scales_update()
    state = H._RB[CPU.index].state
    assert tuple(state.shape) == (H._RB_MAX, 2) and state.dtype == torch.float32
    assert bool((state[:, 0] == 1.0).all()) and bool((state[:, 1] == 0.0).all())
    a, (pl, view, images) = _produce(H, ("site", 1), y)
    view[0] = 0.25
    want = torch.zeros_like(state)
    want[:, 0] = 1.0
    want[1, 0] = 0.25
    assert torch.equal(state, want)
    assert a.y_rb_scale == state[1].data_ptr() and a.y_amax_next == state[1, 1:].data_ptr()
    # the site's handle: one object per key, its addresses and both views name that row
    s = H._rb_site(("site", 1), CPU)
    assert s is H._rb_site(("site", 1), CPU) and s.index == 1 and s.ready and s.scale_view is view
    assert s.scale == state.data_ptr() + 8 * s.index == a.y_rb_scale and s.pending == s.scale + 4 == a.y_amax_next
    assert s.state.data_ptr() == s.scale and tuple(s.state.shape) == (2,)
    s.state[1] = 7.0
    want[1, 1] = 7.0
    assert torch.equal(state, want)
    assert s.produced                                                           # (by the launch above)
    H.rb_scales_update()
    assert not s.produced and s.produce() == s.pending and s.produced
    fresh = H._rb_site(("site", 9), CPU)
    assert fresh.index == 3 and not fresh.ready and not fresh.produced


def test_a_full_table_refuses_new_sites(hip, monkeypatch):
    H, lib = hip
    monkeypatch.setattr(H, "_RB_MAX", 2)
    y = torch.zeros(1, 16, 2, 2)
    a, _ = _produce(H, ("site", 1), y)
    b, _ = _produce(H, ("site", 2), y)
    c, got = _produce(H, ("site", 3), y)
    assert a.y_amax_next and b.y_amax_next and got is None and not c.y_amax_next     # full: not even a pending maximum
    a2, _ = _produce(H, ("site", 1), y)
    assert a2.y_amax_next == a.y_amax_next                                           # (known sites go on)
    H.rb_scales_update()
    assert lib.named("mmt_rb_scales_update") == [(H._RB[CPU.index].state.data_ptr(), 2, 0)]
    assert ctypes.sizeof(ctypes.c_float) * 2 == b.y_amax_next - a.y_amax_next        # one (scale, pending) pair per site
