"""What `mmt_paste_mask_words` and its callers promise without a GPU: the header and the binding agree, the POSTPROCESS_MASKS flag
selects the per-detection masker (and only in the post-processor), the device route has no host fallback, the inputs that
tests/test_paste_words_gpu.py compares on are not empty canvases, and the kernel needs no scratch memory."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import mask_geometry_inputs as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd", "tools"))


def test_header_declares_the_entry_point_and_the_binding_matches():
    from maskrcnn_benchmark import _hip
    text = open(os.path.join(ROOT, "include", "mmtpsm.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+mmt_paste_mask_words\s*\(([^)]*)\)\s*;", text)
    assert m, "include/mmtpsm.h does not declare mmt_paste_mask_words"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["prob", "boxes", "D", "M", "IH", "IW", "thresh", "words", "rec", "stream"]
    sig = _hip._SIGS["mmt_paste_mask_words"]
    assert len(sig) == len(params)
    for p, c in zip(params, sig):
        want = _hip.c_void_p if "*" in p else {"int": _hip.c_int, "float": _hip.c_float}[p.split()[0]]
        assert c is want, (p, c)
    assert "mmt_paste_mask_words" in _hip.exported_symbols()


def test_flag_selects_the_per_detection_masker_in_the_post_processor_only():
    from maskrcnn_benchmark.config import make_default_cfg
    from maskrcnn_benchmark.modeling.roi_heads.mask_head import mask_head as mh
    cfg = make_default_cfg()
    assert cfg.MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS is False
    assert mh.make_roi_mask_post_processor(cfg).masker is None
    cfg.MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS = True
    cfg.MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS_THRESHOLD = 0.4
    pp, gen = mh.make_roi_mask_post_processor(cfg), mh.make_roi_mask_generator(cfg)
    assert type(pp.masker) is mh.DetectionMasker and pp.masker.threshold == 0.4 and pp.masker.padding == 1
    assert type(gen.masker) is mh.Masker and gen.masker.threshold == 0.4           # the teacher's integral pseudo-mask
    assert hasattr(mh.Masker, "rle_single_image")


def test_device_route_raises_without_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # (a machine with a GPU is told it has none)
    from maskrcnn_benchmark import _hip
    from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle
    with pytest.raises(RuntimeError):
        mask_rle.encode_pasted_device(torch.ones(1, 1, 28, 28), torch.tensor([[1.0, 1.0, 9.0, 9.0]]), 16, 16)
    with pytest.raises(RuntimeError):
        mask_rle.encode_pasted_device(torch.ones(0, 1, 28, 28), torch.zeros(0, 4), 16, 16)
    with pytest.raises(RuntimeError):
        _hip.paste_mask_words(torch.ones(1, 28, 28), torch.tensor([[1.0, 1.0, 9.0, 9.0]]), 16, 16, 0.5)


def test_reference_route_inputs_are_not_empty_on_the_oracle():
    """tests/test_paste_words_gpu.py compares two device routes with each other; on the canvas the boxes were drawn for, the
    oracle's paste (oracle/model.py::paste_mask) says that more than 80 % of them have pixels"""
    from oracle import model as om
    ih, iw = mg.CANVAS
    for M, (prob, boxes) in mg.paste_cases().items():
        filled = [bool(om.paste_mask(torch.from_numpy(p), torch.from_numpy(b), ih, iw, mg.PASTE_THRESH).any()) for p, b in zip(prob, boxes)]
        assert np.mean(filled) > 0.8, (M, np.mean(filled))


def test_words_kernel_uses_no_scratch_and_spills_nothing(tmp_path):
    import codeobj
    if not os.path.exists(codeobj.LIB) or not os.path.exists(os.path.join(codeobj.LLVM, "clang-offload-bundler")):
        pytest.skip("library or LLVM tools not present")
    t = codeobj.kernel_table(workdir=str(tmp_path))
    d = codeobj.demangle(sorted(t))
    mine = {d[n]: t[n] for n in t if "paste_words_kernel" in d[n]}
    assert len(mine) == 1, sorted(mine)
    for n, r in mine.items():
        print(n, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        assert r["vgpr"] <= 64, (n, r)      # eight waves per SIMD, the most a CU holds, fit up to 64 registers a lane
