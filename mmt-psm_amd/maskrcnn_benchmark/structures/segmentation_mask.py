"""Polygon instance masks (reference: structures/segmentation_mask.py:53-247).

The reference keeps polygons as Python lists of small CPU tensors and rasterises them one ROI at a time
through pycocotools (mask_head/loss.py:37-75).  Here a SegmentationMask also owns a packed device copy
(vertex array + offsets) so that crop / resize / rasterise of all positive ROIs is ONE kernel launch
(`_hip.polygon_targets`); the list-of-tensors view is kept for API parity (indexing, iteration, flips).
"""
import torch

FLIP_LEFT_RIGHT = 0
FLIP_TOP_BOTTOM = 1


class Polygons(object):
    def __init__(self, polygons, size, mode=None):
        if isinstance(polygons, Polygons):
            polygons = polygons.polygons
        self.polygons = [torch.as_tensor(p, dtype=torch.float32).reshape(-1) for p in polygons]
        self.size = size
        self.mode = mode

    def transpose(self, method):
        if method not in (FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM):
            raise NotImplementedError("Only FLIP_LEFT_RIGHT and FLIP_TOP_BOTTOM implemented")
        w, h = self.size
        dim, idx = (w, 0) if method == FLIP_LEFT_RIGHT else (h, 1)
        out = []
        for p in self.polygons:
            q = p.clone()
            q[idx::2] = dim - p[idx::2] - 1
            out.append(q)
        return Polygons(out, self.size, self.mode)

    def crop(self, box):
        w, h = max(box[2] - box[0], 1), max(box[3] - box[1], 1)
        out = []
        for p in self.polygons:
            q = p.clone()
            q[0::2] = q[0::2] - box[0]
            q[1::2] = q[1::2] - box[1]
            out.append(q)
        return Polygons(out, (w, h), self.mode)

    def resize(self, size, *a, **kw):
        rw, rh = (float(s) / float(o) for s, o in zip(size, self.size))
        out = []
        for p in self.polygons:
            q = p.clone()
            q[0::2] *= rw
            q[1::2] *= rh
            out.append(q)
        return Polygons(out, size, self.mode)

    def convert(self, mode, device=None):
        """convert("mask") -> uint8 [h, w] on the device: the union of this instance's polygons as pycocotools rasterises them
        (reference structures/segmentation_mask.py:127-137, frPyObjects + merge + decode), through the image-size rasteriser
        `_hip.polygon_mask_words`.  The reference returns the same values as a CPU tensor; for any other mode it falls through
        and returns None, here that raises"""
        if mode != "mask":
            raise NotImplementedError("Polygons.convert(%r): only 'mask' is built" % (mode,))
        w, h = int(self.size[0]), int(self.size[1])
        return SegmentationMask([self], self.size, self.mode).decode(h, w, device).to(torch.uint8)

    def __repr__(self):
        return "Polygons(num_polygons={}, image_width={}, image_height={}, mode={})".format(
            len(self.polygons), self.size[0], self.size[1], self.mode)


class SegmentationMask(object):
    def __init__(self, polygons, size, mode=None):
        assert isinstance(polygons, list)
        self.polygons = [p if isinstance(p, Polygons) else Polygons(p, size, mode) for p in polygons]
        self.size = size
        self.mode = mode
        self._packed = None
        self._words = None

    def packed(self, device):
        """-> (xy float32 [V,2] flattened, poly_off int32 [NP+1], inst_range int32 [G,2]) on `device`"""
        if self._packed is None or self._packed[0].device != torch.device(device):
            xy, off, rng = [], [0], []
            for inst in self.polygons:
                b = len(off) - 1
                for p in inst.polygons:
                    xy.append(p)
                    off.append(off[-1] + p.numel() // 2)
                rng.append([b, len(off) - 1])
            xy = torch.cat(xy) if xy else torch.zeros(0)
            self._packed = (xy.to(device), torch.tensor(off, dtype=torch.int32, device=device),
                            torch.tensor(rng, dtype=torch.int32, device=device).reshape(-1, 2))
        return self._packed

    @staticmethod
    def _device(device):
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("polygon masks are rasterised on the GPU (csrc/polyfill.hip); no MI355X visible")
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:   # "cuda": the index a tensor there reports, so that the cache is found again
            device = torch.device("cuda", torch.cuda.current_device())
        return device

    def mask_words(self, device=None):
        """-> (words int64 [G, ceil(h * w / 64)], records int32 [G, 8]) on the device: every instance rasterised at the mask's own
        size into the run-length codec's words (`_hip.polygon_mask_words`; layout: include/mmtpsm.h, mmt_mask_pack).  Cached
        beside the packed vertices"""
        device = self._device(device)
        if self._words is None or self._words[0].device != device:
            from maskrcnn_benchmark import _hip
            xy, off, rng = self.packed(device)
            self._words = _hip.polygon_mask_words(xy, off, rng, int(self.size[1]), int(self.size[0]))
        return self._words

    def decode(self, h, w, device=None):
        """-> int32 [h, w] on the device: the number of instances that cover each pixel (reference
        structures/segmentation_mask.py:174-181, which returns the same values as a float64 numpy array).  (h, w) must be the
        mask's own (size[1], size[0]) -- in the reference any other size breaks the addition --; an empty list gives zeros"""
        if (int(h), int(w)) != (int(self.size[1]), int(self.size[0])):
            raise ValueError("decode(%d, %d) of a %d x %d mask" % (h, w, self.size[1], self.size[0]))
        device = self._device(device)
        if len(self.polygons) == 0:
            return torch.zeros((int(h), int(w)), dtype=torch.int32, device=device)
        from maskrcnn_benchmark import _hip
        words, _ = self.mask_words(device)
        return _hip.mask_words_integral(words, [0, len(self.polygons)], int(h), int(w))[0]

    def transpose(self, method):
        return SegmentationMask([p.transpose(method) for p in self.polygons], self.size, self.mode)

    def crop(self, box):
        w, h = box[2] - box[0], box[3] - box[1]
        return SegmentationMask([p.crop(box) for p in self.polygons], (w, h), self.mode)

    def resize(self, size, *a, **kw):
        return SegmentationMask([p.resize(size, *a, **kw) for p in self.polygons], size, self.mode)

    def to(self, *a, **kw):
        return self

    def __getitem__(self, item):
        if isinstance(item, (int, slice)):
            sel = self.polygons[item]
            sel = sel if isinstance(sel, list) else [sel]
        else:
            if isinstance(item, torch.Tensor) and item.dtype in (torch.uint8, torch.bool):
                item = item.nonzero().reshape(-1)
            sel = [self.polygons[int(i)] for i in (item.tolist() if isinstance(item, torch.Tensor) else item)]
        return SegmentationMask(sel, self.size, self.mode)

    def __iter__(self):
        return iter(self.polygons)

    def __len__(self):
        return len(self.polygons)

    def __repr__(self):
        return "SegmentationMask(num_instances={}, image_width={}, image_height={})".format(
            len(self.polygons), self.size[0], self.size[1])


def mask_window(box, W, H):
    """the window (x0, y0, w, h) of a box (x1, y1, x2, y2) in a W x H mask, or None when a coordinate is not finite
    (include/mmtpsm.h, mmt_mask_words_targets: the same rule on the host): the coordinates rounded half to even in float32 and
    clamped to +-2^30, the start clamped into the mask, the end exclusive and at least one pixel behind the start"""
    import numpy as np
    b = np.asarray([float(v) for v in box], dtype=np.float32)
    if b.shape != (4,):
        raise ValueError("a box is (x1, y1, x2, y2)")
    if not np.isfinite(b).all():
        return None
    xa, ya, xb, yb = (int(v) for v in np.clip(np.rint(b), np.float32(-2.0 ** 30), np.float32(2.0 ** 30)))
    x0, y0 = min(max(xa, 0), W - 1), min(max(ya, 0), H - 1)
    xe, ye = max(min(max(xb, 0), W), x0 + 1), max(min(max(yb, 0), H), y0 + 1)
    return x0, y0, xe - x0, ye - y0


class BinaryMaskList(object):
    """Bitmap instance masks: ground truth that does not come as polygons -- one binary image per cell, COCO run-length strings,
    label images.  The masks live on the device as the run-length codec's 64-bit words with one record each (include/mmtpsm.h,
    mmt_mask_pack) and never as byte planes: crop, resize and flip are `mmt_mask_words_resample`, the M x M targets of the mask head
    `mmt_mask_words_targets` (csrc/bitmasks.hip).  Same surface as SegmentationMask; construction, `len`, `size` and the geometry
    calls work on the host (they are recorded), the words are made on first use and cached, and use without a GPU raises.

    masks: a uint8 / bool tensor or numpy array (G, h, w) or (h, w), on the host or the device; a list of RLE dicts
    {"size": [h, w], "counts": str | bytes | list}; or another BinaryMaskList.  size = (w, h)."""

    def __init__(self, masks, size):
        w, h = int(size[0]), int(size[1])
        self.size = (w, h)
        self._words = None
        self._rles = None
        if isinstance(masks, BinaryMaskList):
            if tuple(int(v) for v in masks.size) != (w, h):
                raise ValueError("a %d x %d BinaryMaskList given as one of %d x %d" % (masks.size[0], masks.size[1], w, h))
            self._n, self._make, self._rles = len(masks), masks.mask_words, masks._rles
        elif isinstance(masks, (list, tuple)):
            for r in masks:
                if not isinstance(r, dict) or "size" not in r or "counts" not in r:
                    raise ValueError("a list of masks holds RLE dicts {'size': [h, w], 'counts': ...}")
                if [int(v) for v in r["size"]] != [h, w]:
                    raise ValueError("an RLE of %s in a %d x %d (h x w) BinaryMaskList" % (list(r["size"]), h, w))
            self._rles = list(masks)
            self._n, self._make = len(masks), self._words_of_rles
        else:
            import numpy as np
            if isinstance(masks, np.ndarray):
                masks = torch.from_numpy(np.ascontiguousarray(masks))
            if not isinstance(masks, torch.Tensor):
                raise ValueError("BinaryMaskList takes an array (G, h, w), a list of RLE dicts or a BinaryMaskList, not %s"
                                 % type(masks).__name__)
            if masks.dtype not in (torch.uint8, torch.bool):
                raise ValueError("mask arrays are uint8 or bool, not %s" % masks.dtype)
            if masks.dim() == 2:
                masks = masks[None]
            if masks.dim() != 3 or tuple(masks.shape[1:]) != (h, w):
                raise ValueError("masks of shape %s in a %d x %d (h x w) BinaryMaskList" % (tuple(masks.shape), h, w))
            self._bytes = masks
            self._n, self._make = int(masks.shape[0]), self._words_of_bytes

    @classmethod
    def from_polygons(cls, segmentation_mask):
        """the instances of a SegmentationMask, rasterised at its size (its `mask_words`, adopted)"""
        return cls._derived(len(segmentation_mask), segmentation_mask.size, segmentation_mask.mask_words)

    @classmethod
    def _derived(cls, n, size, make):
        out = cls.__new__(cls)
        out.size = (int(size[0]), int(size[1]))
        out._n, out._make, out._words, out._rles = int(n), make, None, None
        return out

    # ---- producers (each -> (words, records) on `device`)
    def _words_of_bytes(self, device):
        from maskrcnn_benchmark import _hip
        return _hip.mask_pack(self._bytes.to(device).to(torch.uint8))

    def _words_of_rles(self, device):
        import numpy as np
        from maskrcnn_benchmark import _hip
        from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle
        w, h = self.size
        if not self._rles:
            return _hip._mask_buffers(0, h, w, device)
        ends, off = [], [0]
        for r in self._rles:
            e = np.cumsum(np.asarray(mask_rle.counts_of(r), dtype=np.int64))
            if e.shape[0] == 0 or e[-1] != h * w or (np.diff(e) < 0).any() or e[0] < 0:
                raise ValueError("RLE does not cover its %d x %d mask" % (h, w))
            ends.append(e.astype(np.int32))
            off.append(off[-1] + e.shape[0])
        return _hip.mask_expand(torch.from_numpy(np.concatenate(ends)).to(device), torch.tensor(off, dtype=torch.int64).to(device), h, w)

    def mask_words(self, device=None):
        """-> (words int64 [G, ceil(h * w / 64)], records int32 [G, 8]) on the device (layout: include/mmtpsm.h, mmt_mask_pack);
        made on first use, then cached"""
        device = SegmentationMask._device(device)
        if self._words is None or self._words[0].device != device:
            self._words = self._make(device)
        return self._words

    def source_rles(self):
        """the RLE dicts this list was built from, untouched, or None for any other source (or after any geometry)"""
        return self._rles

    # ---- consumers
    def decode(self, h, w, device=None):
        """-> int32 [h, w] on the device: the number of instances that cover each pixel, as SegmentationMask.decode"""
        if (int(h), int(w)) != (self.size[1], self.size[0]):
            raise ValueError("decode(%d, %d) of a %d x %d mask" % (h, w, self.size[1], self.size[0]))
        device = SegmentationMask._device(device)
        if self._n == 0:
            return torch.zeros((int(h), int(w)), dtype=torch.int32, device=device)
        from maskrcnn_benchmark import _hip
        words, _ = self.mask_words(device)
        return _hip.mask_words_integral(words, [0, self._n], int(h), int(w))[0]

    def get_mask_tensor(self, device=None):
        """-> uint8 [G, h, w] on the device (for inspection: nothing on the training path wants the bytes)"""
        device = SegmentationMask._device(device)
        w, h = self.size
        if self._n == 0:
            return torch.zeros((0, h, w), dtype=torch.uint8, device=device)
        from maskrcnn_benchmark import _hip
        words, _ = self.mask_words(device)
        return _hip.mask_words_integral(words, list(range(self._n + 1)), h, w).to(torch.uint8)

    def rles(self, device=None):
        """-> the codec's dicts {"size": [h, w], "counts": bytes}, one per instance; only the run boundaries cross to the host"""
        device = SegmentationMask._device(device)
        if self._n == 0:
            return []
        from maskrcnn_benchmark import _hip
        from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle
        words, _ = self.mask_words(device)
        return mask_rle._strings_of_words(_hip, words, self.size[1], self.size[0])

    # ---- geometry (recorded here, run with the words)
    def _resampled(self, window, flip, size):
        w, h = self.size
        ow, oh = int(size[0]), int(size[1])
        if ow < 1 or oh < 1:
            raise ValueError("masks resampled to %d x %d" % (ow, oh))
        parent = self

        def make(device):
            from maskrcnn_benchmark import _hip
            words, _ = parent.mask_words(device)
            return _hip.mask_words_resample(words, h, w, window, flip, oh, ow)
        return BinaryMaskList._derived(self._n, (ow, oh), make)

    def transpose(self, method):
        if method not in (FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM):
            raise NotImplementedError("Only FLIP_LEFT_RIGHT and FLIP_TOP_BOTTOM implemented")
        w, h = self.size
        return self._resampled((0, 0, w, h), 1 if method == FLIP_LEFT_RIGHT else 2, self.size)

    def resize(self, size, *a, **kw):
        w, h = self.size
        return self._resampled((0, 0, w, h), 0, size)

    def crop(self, box):
        w, h = self.size
        win = mask_window(box, w, h)
        if win is None:
            raise ValueError("crop to a box with a non-finite coordinate")
        return self._resampled(win, 0, (win[2], win[3]))

    def to(self, *a, **kw):
        return self

    # ---- selection
    def __getitem__(self, item):
        n = self._n
        if isinstance(item, torch.Tensor) and item.is_cuda:
            # rows of the words are selected on the device; the index is not read back
            if item.dtype not in (torch.int64, torch.bool, torch.uint8):
                raise IndexError("a device index is an int64 or bool tensor")
            words, rec = self.mask_words(item.device)
            item = item.reshape(-1)
            if item.dtype != torch.int64:
                item = item.to(torch.bool)
            sel = (words[item].contiguous(), rec[item].contiguous())
            out = BinaryMaskList._derived(sel[0].shape[0], self.size, lambda device: (sel[0].to(device), sel[1].to(device)))
            out._words = sel
            return out
        if isinstance(item, int):
            idx = [range(n)[item]]
        elif isinstance(item, slice):
            idx = list(range(n))[item]
        else:
            t = torch.as_tensor(item)
            if t.dtype in (torch.uint8, torch.bool):
                if t.numel() != n:
                    raise IndexError("a mask of %d entries for %d instances" % (t.numel(), n))
                t = t.reshape(-1).nonzero().reshape(-1)
            idx = [range(n)[int(i)] for i in t.reshape(-1).tolist()]
        parent = self

        def make(device):
            words, rec = parent.mask_words(device)
            at = torch.tensor(idx, dtype=torch.int64, device=device)
            return words.index_select(0, at), rec.index_select(0, at)
        return BinaryMaskList._derived(len(idx), self.size, make)

    def __iter__(self):
        return (self[i] for i in range(self._n))

    def __len__(self):
        return self._n

    def __repr__(self):
        return "BinaryMaskList(num_instances={}, image_width={}, image_height={})".format(self._n, self.size[0], self.size[1])
