"""Timing of the CSPN mask head's ROIAlign (csrc/roi_align.hip: mmt_roi_align_maps_forward / _backward) and of one mean-teacher
step with CSPN.yaml's model keys.  A measurement script: nothing is gated on its numbers.

Kernel: K = 256 ROIs pooled at 25 x 25 from the four pair outputs of the head on the bench's 1024 x 1024 padded crops (N = 2;
32 / 64 / 128 / 256 channels at 1024 / 512 / 256 / 128 pixels) into the 480-channel tensor -- one launch, against the only other way
to the same values: four single-level `roi_align_forward` calls and a `torch.cat`; backward the same (four `roi_align_backward`
calls on channel slices of the gradient made dense first).  HIP events around REPS back-to-back launches, median of ROUNDS rounds
after a warm-up, one process (the warm-up of tools/bench_gconv.py).  The bound printed is the pooled tensor written (read, backward)
once at 6.3 TB/s.

Step: the bench's trainer (bench.py::build, untouched) with the CSPN keys against the default configuration, same process.

    python mmt-psm_amd/tools/bench_cspn.py [--no-step]
"""
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from bench_gconv import HBM, REPS, ROUNDS, WARM, timed  # noqa: E402

CSPN_KEYS = ["MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR", "PRCNNFeatureExtractor", "MODEL.ROI_MASK_HEAD.PREDICTOR", "PRCNNPredictor",
             "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", 25, "MODEL.ROI_MASK_HEAD.RESOLUTION", 25,
             "MODEL.RELATION_MASK.TYPE", "LIAM", "MODEL.RELATION_MASK.USE_RELATION", False]
K, RES, N, SIZE = 256, 25, 2, 1024
WIDTHS, SCALES = (32, 64, 128, 256), (1.0, 0.5, 0.25, 0.125)


def kernel():
    from maskrcnn_benchmark import _hip as H
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    feats = [torch.relu(torch.randn((N, SIZE >> m, SIZE >> m, c), generator=g, device=dev)).permute(0, 3, 1, 2)
             for m, c in enumerate(WIDTHS)]
    # boxes like the bench's instances (16-gons of radius 8 .. 80 pixels) anywhere in the crop
    ctr = torch.rand((K, 2), generator=g, device=dev) * 1000
    half = 8 + torch.rand((K, 2), generator=g, device=dev) * 72
    img = torch.randint(0, N, (K, 1), generator=g, device=dev).float()
    rois = torch.cat([img, ctr - half, ctr + half], 1).contiguous()
    lv = torch.zeros((K,), dtype=torch.int32, device=dev)
    shapes = [tuple(f.shape) for f in feats]
    go = torch.randn((K, RES, RES, sum(WIDTHS)), generator=g, device=dev).permute(0, 3, 1, 2)
    nbytes = 4.0 * K * RES * RES * sum(WIDTHS)
    print("ROIAlign over four maps, K %d, %d x %d bins, %d channels; %d launches per event pair, median of %d, %d warm-up; pooled "
          "tensor %.1f MB = %.1f us at 6.3 TB/s" % (K, RES, RES, sum(WIDTHS), REPS, ROUNDS, WARM, nbytes / 1e6, nbytes / HBM * 1e6))

    def four_fwd():
        return torch.cat([H.roi_align_forward([f], [s], rois, lv, RES, RES, 2) for f, s in zip(feats, SCALES)], 1)

    def four_bwd():
        out, o = [], 0
        for s, sc, c in zip(shapes, SCALES, WIDTHS):
            out.append(H.roi_align_backward(go[:, o:o + c].contiguous(memory_format=torch.channels_last), [s], [sc], rois, lv,
                                            RES, RES, 2)[0])
            o += c
        return out
    a, b = H.roi_align_maps_forward(feats, SCALES, rois, RES, RES, 2), four_fwd()
    assert torch.equal(a, b), "the one-launch form and four launches + cat disagree"
    t1 = timed(lambda: H.roi_align_maps_forward(feats, SCALES, rois, RES, RES, 2))
    t4 = timed(four_fwd)
    print("  forward   one launch %8.1f us (%.1f %% of the bound)   four launches + cat %8.1f us   ratio %.3f"
          % (t1 * 1e6, 100 * nbytes / HBM / t1, t4 * 1e6, t1 / t4))
    t1 = timed(lambda: H.roi_align_maps_backward(go, shapes, SCALES, rois, RES, RES, 2))
    t4 = timed(four_bwd)
    print("  backward  one launch %8.1f us (clears of the four gradient maps included on both sides)   four launches on dense "
          "slices %8.1f us   ratio %.3f" % (t1 * 1e6, t4 * 1e6, t1 / t4))


def step(keys, tag):
    import bench
    import maskrcnn_benchmark.config as config
    base = config.make_default_cfg

    def cfg_with_keys():
        cfg = base()
        cfg.merge_from_list(list(keys))
        return cfg
    config.make_default_cfg = cfg_with_keys
    try:
        cfg, trainer, batch = bench.build(torch.device("cuda", 0), 0)
    finally:
        config.make_default_cfg = base
    it = cfg.MT.START_MT + 400
    ms = []
    for i in range(10):
        data = batch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        losses = trainer.train_step(it + i, *data)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    finite = all(torch.isfinite(v).item() for v in losses.values())
    print("mean-teacher step, %s, 2 + 2 crops of 1000 x 1000: steps 4-10 median %.1f ms (all: %s), losses finite after 10 steps: %s "
          "-- a single observation" % (tag, statistics.median(ms[3:]), " ".join("%.1f" % m for m in ms), finite))
    del trainer, batch
    torch.cuda.empty_cache()


def main():
    from maskrcnn_benchmark import _hip as H
    H.lib()
    assert torch.cuda.is_available(), "needs the MI355X"
    kernel()
    if "--no-step" not in sys.argv:
        step([], "default configuration")
        step(CSPN_KEYS, "CSPN keys (PRCNNFeatureExtractor / PRCNNPredictor, 25 x 25)")


if __name__ == "__main__":
    main()
