"""Flat parameter storage: all parameters of a model live in ONE fp32 device buffer
[trainable weights | trainable biases | frozen], each nn.Parameter being a view (conv weights keep their
channels_last strides).  Gradients and SGD momentum mirror the layout.  This is what turns the reference's
132-tensor EMA loop (engine/MTtrainer.py:277-281), its 121-group SGD (solver/build.py:18) and the (new) data
parallel gradient all-reduce into single launches / single collectives over contiguous memory."""
import collections
import struct
import weakref

import torch

from .. import _hip as H


class WeightRecord(object):
    """one packed weight matrix of a flat buffer: where it lies, and the views of the bulk planes that serve its forward forms"""
    __slots__ = ("source", "offset", "cout", "k", "desc", "version", "bf16", "f16", "dgrad")

    def __init__(self, source, offset, cout, k, desc, bf16):
        self.source, self.offset, self.cout, self.k, self.desc, self.bf16 = source, offset, cout, k, desc, bf16
        # version: of the parameter at the last refresh; f16: (planes, scale word), views of planes16 / stat16[desc], made when those are
        # allocated; dgrad: data-gradient form -> DgradForm
        self.version, self.f16, self.dgrad = source._version, None, {}


class DgradForm(object):
    """one data-gradient form of a weight matrix: planes of its own, re-packed in place by the bulk launch of its kind"""
    __slots__ = ("w", "scale", "scale_version", "dims", "planes", "stat", "gen", "served")

    def __init__(self, w, scale, planes, stat, gen):
        # gen: the plane generation the planes were last packed (or stamped) for; stat (fp16): (max |w scale|, scale word) on the
        # device, the bulk table's row once it has one
        self.w, self.scale, self.planes, self.stat, self.gen = w, scale, planes, stat, gen
        self.scale_version = None if scale is None else scale._version
        self.dims = (w.shape[0], w.shape[2], w.shape[3], w.shape[1])   # Cout, KH, KW, Cin
        self.served = planes if stat is None else (planes, stat[1:2])


Table = collections.namedtuple("Table", "descs units n_units n_descs entries stat")


def _table(rows, dev, entries=(), with_stat=False):
    """device descriptor table of a bulk packing launch; rows: (struct format, leading fields, 512-element units) per matrix, every
    descriptor ending in (its first unit, 0).  with_stat: a (max, scale word) row per entry, which the entries then serve"""
    descs, unit_desc, unit0 = [], [], 0
    for fmt, fields, units in rows:
        unit_desc += [len(descs)] * units
        descs.append(struct.pack(fmt, *(tuple(fields) + (unit0, 0))))
        unit0 += units
    stat = torch.zeros((len(descs), 2), dtype=torch.float32, device=dev) if with_stat else None
    for i, e in enumerate(entries if with_stat else ()):
        e.stat, e.served = stat[i], (e.planes, stat[i, 1:2])
    return Table(torch.frombuffer(bytearray(b"".join(descs)), dtype=torch.uint8).to(dev),
                 torch.tensor(unit_desc, dtype=torch.int32, device=dev), unit0, len(descs), list(entries), stat)


def _is_bias(name):
    return "bias" in name  # solver/build.py:14


class FlatParams(object):
    def __init__(self, model):
        named = list(model.named_parameters())
        tw = [(n, p) for n, p in named if p.requires_grad and not _is_bias(n)]
        tb = [(n, p) for n, p in named if p.requires_grad and _is_bias(n)]
        fz = [(n, p) for n, p in named if not p.requires_grad]
        dev = named[0][1].device

        def pad4(n):
            return (n + 7) // 8 * 8  # 32-byte aligned views: float4 kernels, and 16-byte aligned bf16 plane slices

        self.index = {}
        off = 0
        for group in (tw, tb, fz):
            for n, p in group:
                self.index[n] = (off, p.numel())
                off += pad4(p.numel())  # 16-byte aligned views for the float4 kernels
            off = pad4(off)
            if group is tw:
                self.n_weights = off
            elif group is tb:
                self.n_biases = off - self.n_weights
        self.n_trainable = self.n_weights + self.n_biases
        self.total = off
        self.data = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(self.n_trainable, dtype=torch.float32, device=dev)
        self.momentum = torch.zeros(self.n_trainable, dtype=torch.float32, device=dev)
        # names of the parameters that received a gradient since the last zero_grad: fused backward nodes report their direct
        # writes (layers/fused.py::_touch, looked up by slot address), autograd deliveries are seen by a hook.  FlatSGD
        # updates only these, which is torch.optim.SGD's `if p.grad is None: continue` (solver/build.py)
        self.touched = set()
        me = weakref.ref(self)
        for n, p in named:
            o, k = self.index[n]
            view = self._view_like(self.data[o:o + k], p)
            view.copy_(p.data)
            p.data = view
            p._flat_ref = me   # (what is derived from a parameter outside the bulk packs asks for the buffer's plane generation)
            if p.requires_grad:
                p.grad = self._view_like(self.grad[o:o + k], p)
                # fused backward nodes accumulate weight gradients straight into this slot (layers/fused.py)
                p._flat_grad = p.grad
                H.GRAD_SLOTS[p.grad.data_ptr()] = (me, n)
                p.register_post_accumulate_grad_hook(lambda q, n=n, me=me: me() is not None and me().touched.add(n))
        self.planes = None                   # bf16 planes of all packed matrices, [3, total]
        self.planes16 = self.stat16 = None   # fp16 two-term planes of the same matrices + (max, scale) per matrix
        self.records = {}                    # weight address -> WeightRecord (filled when the planes are allocated)
        self.plane_gen = 0                   # bumped by every refresh: the parameters changed under raw pointers
        self._bulk = {"bf16": -1, "f16": -1}  # generation the bulk launch of a forward form last ran for
        self._epoch = -1                     # _hip.PLANES_EPOCH (the arithmetic mode's counter) at the last refresh
        self._lazy_bf16 = False
        self._fwd = None                     # descriptor table of the forward forms
        self._dgrad_tables = {"f16_dgrad": None, "bf16_dgrad": None}
        self._named = named
        self.refresh_planes()

    # ---- derived forms of the weight matrices.  THE owner: what a convolution reads instead of a weight of this buffer is kept
    # here, and `form` alone decides whether it is current.  Invariants:
    #  * address stability: the FORWARD forms once served -- planes and scale word -- keep their device addresses for the life of
    #    this object (recorded launch plans hold them), and so do the planes of a registered data-gradient form; the bulk re-pack
    #    writes in place.  _hip.LAYOUT_EPOCH is bumped exactly where the plane buffers are allocated below, nowhere else.  NOT stable:
    #    the scale word of an fp16 data-gradient form -- the per-call pack's own until the first refresh, then a row of its table's
    #    `stat`, and every `register` rebuilds that table with new rows for all entries -- and the planes of a form registered again
    #    (another scale vector, a stale scale).  No recorded plan contains a data-gradient launch.
    #  * one validity rule, decided in `form` and nowhere else.  A form is served only when (a) the weight was not written through
    #    torch since the last refresh (its version counter), (b) the form was packed for the current plane generation -- "bf16" also
    #    while its bulk launch is deferred: the launch that reads it calls `ensure_bf16` first --, (c) under the arithmetic mode that
    #    is still the current one (_hip.PLANES_EPOCH), (d) data-gradient forms: with the same scale vector at the same version, and
    #    (e) for a matrix of these dimensions.  The weight is found by ADDRESS: a Linear layer hands its weight over as a fresh 4-D
    #    view every call and a backward pass sees new objects; inside this buffer the address names the matrix.
    #  * nothing is built, launched or allocated on a hit: two dict lookups, a handful of comparisons, a cached view.
    #  * the packing arithmetic is the library's (include/mmtpsm.h: mmt_pack_weights*), the same launches as a per-call pack.
    def refresh_planes(self):
        """split-bf16 conv modes (mmt_set_conv_precision != 0): re-pack every weight matrix of the parameter buffer into
        its three bf16 planes (include/mmtpsm.h: mmt_pack_weights) -- ONE launch over a device descriptor table; called
        after everything that rewrites parameters through raw pointers (SGD, EMA, teacher initialisation).
        Convolutions find this object by their weight's address (_hip.FLATS) and ask `form`."""
        self.plane_gen += 1  # the parameters changed: every form packed for an earlier generation is stale
        if not self.data.is_cuda or H.get_conv_precision() == 0:
            return
        dev = self.data.device
        if self.planes is None:
            rows, off = [], 0
            for n, p in self._named:
                if p.dim() < 2 or p.shape[0] <= 32 or (p.numel() // p.shape[0]) % 16:
                    continue  # such layers always run on the fp32 kernel
                if getattr(p, "_mmt_grouped", False):
                    continue  # conv2 of a grouped bottleneck: csrc/conv_group.hip reads the fp32 weight, nobody reads dense planes
                cout, k = p.shape[0], p.numel() // p.shape[0]
                rows.append(("qqiiii", (self.index[n][0], off, cout, k), H.packed_elems(cout, k) // 512, p))
                off += H.packed_elems(cout, k)
            self.planes = torch.empty((3, max(off, 8)), dtype=torch.bfloat16, device=dev)
            H.LAYOUT_EPOCH[0] += 1   # (recorded launch plans hold plane addresses)
            for d, (_, (o, off, cout, k), units, p) in enumerate(rows):
                self.records[p.data_ptr()] = WeightRecord(p, o, cout, k, d, self.planes[:, off:off + units * 512])
            self._fwd = _table([r[:3] for r in rows], dev)
            H.FLATS.update((q, self) for q in self.records)
        t = self._fwd
        # on the fp16 split (the default) next to nothing reads the bf16 planes -- only a site that fell back, or a shape the
        # fp16 kernels do not take: they are packed on first use of a generation (`ensure_bf16`) instead of after every step
        f16 = self._lazy_bf16 = bool(H.F16X2 and H.get_conv_precision() == 3 and t.n_descs)
        if f16:
            # the default arithmetic's form of the same matrices: two fp16 planes of w * s, s per matrix from its maximum
            # (reduction launch + packing launch over the same tables); stat16[d] = (max |w_d|, s_d)
            if self.planes16 is None:
                H.LAYOUT_EPOCH[0] += 1
                self.planes16 = torch.empty((2, self.planes.shape[1]), dtype=torch.float16, device=dev)
                self.stat16 = torch.zeros((t.n_descs, 2), dtype=torch.float32, device=dev)
                for r in self.records.values():
                    off = r.bf16.storage_offset()
                    r.f16 = (self.planes16[:, off:off + r.bf16.shape[1]], self.stat16[r.desc, 1:2])
            H._check(H.lib().mmt_pack_weights_f16(self.data.data_ptr(), self.planes16.data_ptr(), self.planes16.stride(0),
                                                  t.descs.data_ptr(), t.units.data_ptr(), t.n_units, t.n_descs,
                                                  self.stat16.data_ptr(), H._stream()), "mmt_pack_weights_f16")
            self._bulk["f16"] = self.plane_gen
        for r in self.records.values():
            r.version = r.source._version
        self._epoch = H.PLANES_EPOCH
        # the registered data-gradient forms follow, one launch per kind, and are stamped for this generation (the bf16 kind's
        # launch comes with the forward planes': `ensure_bf16`, below or deferred)
        for form in ("f16_dgrad", "bf16_dgrad") if f16 else ("bf16_dgrad",):
            for e in self._pack_dgrad(form, launch=form == "f16_dgrad"):
                e.gen, e.scale_version = self.plane_gen, None if e.scale is None else e.scale._version
        if not f16:
            self.ensure_bf16()   # (not deferred: the forward planes, then the data-gradient ones, now)

    def source(self, w):
        """the record of `w` when it IS one of this buffer's packed matrices as last refreshed -- (a), (c), (e) above -- else None"""
        r = self.records.get(w.data_ptr())
        if (r is None or r.version != w._version or self._epoch != H.PLANES_EPOCH
                or r.cout != w.shape[0] or r.cout * r.k != w.numel()):
            return None
        return r

    def form(self, w, form, scale=None):
        """what a launch reads for the weight `w` -- "bf16" / "bf16_dgrad": packed planes, "f16" / "f16_dgrad": (packed planes, one-
        element view of the scale word) -- or None when this buffer holds no current one: THE validity rule, (a) - (e) above"""
        r = self.source(w)
        if r is None:
            return None
        if form == "bf16":
            return r.bf16 if self._bulk[form] == self.plane_gen or self._lazy_bf16 else None
        if form == "f16":
            return r.f16 if self._bulk[form] == self.plane_gen else None
        e = r.dgrad.get(form)
        if (e is None or e.gen != self.plane_gen or e.scale is not scale or (scale is not None and e.scale_version != scale._version)
                or e.dims != (w.shape[0], w.shape[2], w.shape[3], w.shape[1])):
            return None
        return e.served

    def register(self, form, w, scale, planes, stat=None):
        """a data-gradient form of `w` (rows x `scale`) the caller just packed into `planes` (fp16: `stat` = its (max, scale word) pair):
        served from now on, from the next refresh on re-packed in place by the bulk launch.  -> False: not a `source`, nothing taken"""
        r = self.source(w)
        if r is not None:
            r.dgrad[form] = DgradForm(w, scale, planes, stat, self.plane_gen)
            self._dgrad_tables[form] = None
        return r is not None

    def dgrad_forms(self, form):
        """the registered data-gradient forms of one kind"""
        return [r.dgrad[form] for r in self.records.values() if form in r.dgrad]

    def _pack_dgrad(self, form, launch=True):
        """the bulk launch over the registered data-gradient forms of one kind (table rebuilt when one was registered since) -> them"""
        t = self._dgrad_tables[form]
        if t is None:
            ents = self.dgrad_forms(form)
            if not ents:
                return ents
            rows = [("qqqqiiiiii", (e.w.data_ptr(), H._p(e.scale) or 0, e.planes.data_ptr(), e.planes.stride(0)) + e.dims,
                     e.planes.shape[1] // 512) for e in ents]
            t = self._dgrad_tables[form] = _table(rows, self.data.device, ents, form == "f16_dgrad")
        if launch and t.stat is not None:
            H._check(H.lib().mmt_pack_weights_flipped_f16(t.descs.data_ptr(), t.units.data_ptr(), t.n_units, t.n_descs,
                                                          t.stat.data_ptr(), H._stream()), "mmt_pack_weights_flipped_f16")
        elif launch:
            H._check(H.lib().mmt_pack_weights_flipped(t.descs.data_ptr(), t.units.data_ptr(), t.n_units, H._stream()),
                     "mmt_pack_weights_flipped")
        return t.entries

    def ensure_bf16(self):
        """the bf16 planes of this parameter generation, packed now if they were deferred (called right before a launch that
        reads them, on that launch's stream: all consumers of a model's planes sit on one stream)"""
        if self._bulk["bf16"] == self.plane_gen or self.planes is None:
            return
        H.pack_weights(self.data, self.planes, self._fwd.descs, self._fwd.units, self._fwd.n_units)
        # a weight registered since the last bulk pack (`register` drops the table) must not leave the OTHER entries un-packed:
        # the refresh already stamped them for this generation
        self._pack_dgrad("bf16_dgrad")
        self._bulk["bf16"] = self.plane_gen

    def active_ranges(self, names, lo, hi):
        """merged [a, b) element ranges inside [lo, hi) of the flat buffer covered by the parameters in `names`
        (padding between neighbours included, so adjacent parameters merge into one range)"""
        spans = sorted(self.index[n] for n in names if lo <= self.index[n][0] < hi)
        order = sorted(o for o, _ in self.index.values() if lo <= o < hi) + [hi]
        nxt = {o: order[i + 1] for i, o in enumerate(order[:-1])}
        out = []
        for o, _ in spans:
            b = nxt[o]
            if out and out[-1][1] == o:
                out[-1][1] = b
            else:
                out.append([o, b])
        return [(a, b) for a, b in out]

    @staticmethod
    def _view_like(flat, p):
        if p.dim() == 4:  # memory is [O][H][W][I] (channels_last) for every 4-D weight on the path
            o, i, h, w = p.shape
            return flat.view(o, h, w, i).permute(0, 3, 1, 2)
        return flat.view(p.shape)


def flatten_model(model):
    if getattr(model, "_flat", None) is None:
        model._flat = FlatParams(model)
    return model._flat
