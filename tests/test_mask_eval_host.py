"""The host half of the device mask codec (data/datasets/evaluation/pap/mask_rle.py: positions of the run boundaries -> run
lengths -> string) against `encode`, with the positions taken from numpy; and the rule that the device path has no fallback:
on a machine without a GPU `on_device=True` raises.  CPU tests."""
import numpy as np
import pytest
import torch

import mask_cases


def test_cases_are_the_61_of_the_issue():
    assert len(mask_cases.all_cases()) == 61


def test_positions_to_runs_to_string_reproduces_encode():
    from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle as mu
    cases = mask_cases.all_cases() + [mask_cases.TALL + c for c in mask_cases.masks_of(*mask_cases.TALL)]
    for h, w, name, m in cases:
        runs = mu._runs_of_positions(mask_cases.positions(m), h * w)
        assert runs == mu._runs((m != 0).astype(np.uint8).flatten(order="F")), (h, w, name)
        assert sum(runs) == h * w
        assert mu._to_string(runs).encode("ascii") == mu.encode(m)["counts"], (h, w, name)
    assert mu._runs_of_positions([], 12) == [12] and mu._runs_of_positions([0], 12) == [0, 12]
    assert mu._runs_of_positions([], 0) == [0]


def test_box_of_record_is_bbox():
    from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle as mu
    for h, w, name, m in mask_cases.all_cases():
        ys, xs = np.nonzero(m)
        if ys.size == 0:
            rec = [0] * 8
        else:
            wrap = int(w > 1 and bool(np.any(m[-1, :-1] & m[0, 1:])))
            rec = [int(m.sum()), int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max()), wrap, 0, 0]
        assert tuple(float(v) for v in mu._box_of_record(rec, h)) == mu._bbox(m), (h, w, name)


def test_on_device_raises_without_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # (a machine with a GPU is told it has none)
    from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle as mu
    from maskrcnn_benchmark.data.datasets.evaluation.pap.pap_eval import prepare_for_pap_segmentation, evaluate_predictions_on_pap
    r = mu.encode(np.ones((5, 6), np.uint8))
    assert mu.iouIntUni([r], [r], [0])[1][0, 0] == 30           # the default stays the host path
    with pytest.raises(RuntimeError):
        mu.iouIntUni([r], [r], [0], on_device=True)
    with pytest.raises(RuntimeError):
        mu.encode_device(torch.ones((1, 5, 6), dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        prepare_for_pap_segmentation({}, object(), on_device=True)
    g = {"image_id": {"file_name": "s", "location": (0, 0), "id": 1}, "category_id": 1, "segmentation": r}
    with pytest.raises(RuntimeError):
        evaluate_predictions_on_pap([g], [dict(g, score=0.5)], None, "segm", on_device=True)
