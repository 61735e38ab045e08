"""Timing of the grouped 3x3 convolution kernels (csrc/conv_group.hip) on the ResNeXt-32x8d stage shapes at the bench's size
(N = 4, maps 256 / 128 / 64 / 32 of a 1024-padded crop) and on the stride-2 shapes of the stages' first blocks.

Per shape and direction (forward, data gradient, weight gradient): time (HIP events around REPS back-to-back launches, median of
ROUNDS rounds after a warm-up, one process), achieved TFLOP/s on the algorithmic 2 * 9 * C * Cg FLOP per output pixel, and the
fraction of the compulsory-traffic time (each operand tensor read once, the result written once, at 6.3 TB/s -- the achievable HBM
rate of the MI355X).  For the stride-1 forward also the only way to compute the same values without these kernels: the dense
`_hip.conv_forward` on the block-diagonal expansion of the same weight (G times the FLOP), or why it refuses the shape.

    python mmt-psm_amd/tools/bench_gconv.py [--step]      # --step: also one ResNeXt mean-teacher configuration at 1000 x 1000
"""
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

HBM = 6.3e12
REPS, ROUNDS, WARM = 10, 20, 3
#         N  C     Cg  H    W    stride
SHAPES = [(4, 256, 8, 256, 256, 1), (4, 512, 16, 128, 128, 1), (4, 1024, 32, 64, 64, 1), (4, 2048, 64, 32, 32, 1),
          (4, 512, 16, 256, 256, 2), (4, 1024, 32, 128, 128, 2), (4, 2048, 64, 64, 64, 2)]


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / REPS)
    return statistics.median(ms) * 1e-3


def line(tag, t, flop, nbytes):
    return "  %-14s %9.1f us  %7.2f TFLOP/s  %5.1f %% of the compulsory-traffic time (%.1f us)" % (
        tag, t * 1e6, flop / t / 1e12, 100.0 * (nbytes / HBM) / t, nbytes / HBM * 1e6)


def main():
    from maskrcnn_benchmark import _hip as H
    H.lib()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    print("grouped 3x3 convolution, fp32-input MFMA; %d launches per event pair, median of %d, %d warm-up" % (REPS, ROUNDS, WARM))
    for N, C, Cg, Hh, Ww, s in SHAPES:
        Ho, Wo = (Hh - 1) // s + 1, (Ww - 1) // s + 1
        x = torch.relu(torch.randn((N, Hh, Ww, C), generator=g, device=dev)).permute(0, 3, 1, 2)
        w = (torch.randn((C, 3, 3, Cg), generator=g, device=dev) * (2.0 / (9 * Cg)) ** 0.5).permute(0, 3, 1, 2)
        dy = torch.randn((N, Ho, Wo, C), generator=g, device=dev).permute(0, 3, 1, 2)
        sc = 0.5 + torch.rand((C,), generator=g, device=dev)
        sh = torch.randn((C,), generator=g, device=dev) * 0.1
        dw = torch.zeros_like(w)
        dx = torch.empty_like(x)
        flop = 2.0 * 9 * C * Cg * N * Ho * Wo
        io = 4.0 * C * N * (Hh * Ww + Ho * Wo)
        print("N %d  C %d  Cg %d (G %d)  %d x %d  stride %d   %.2f GFLOP" % (N, C, Cg, C // Cg, Hh, Ww, s, flop / 1e9))
        t = timed(lambda: H.gconv3x3_forward(x, w, sc, sh, s, relu=True))
        print(line("forward", t, flop, io))
        print(line("data gradient", timed(lambda: H.gconv3x3_dgrad(dy, w, (Hh, Ww), s, scale=sc, mask=x, out=dx)), flop, io))
        print(line("weight gradient", timed(lambda: H.gconv3x3_wgrad(x, dy, (C, Cg, 3, 3), s, dw, sc)), flop, io))
        if s == 1:
            try:
                wd = torch.zeros((C, 3, 3, C), device=dev)
                wg = w.permute(0, 2, 3, 1)   # [C][3][3][Cg]
                for gi in range(C // Cg):
                    wd[gi * Cg:(gi + 1) * Cg, :, :, gi * Cg:(gi + 1) * Cg] = wg[gi * Cg:(gi + 1) * Cg]
                wd = wd.permute(0, 3, 1, 2)
                y = H.gconv3x3_forward(x, w, sc, sh, 1, relu=True)
                yd = H.conv_forward(x, wd, sc, sh, 1, 1, relu=True)
                err = ((y - yd).abs().max() / y.abs().max()).item()
                td = timed(lambda: H.conv_forward(x, wd, sc, sh, 1, 1, relu=True))
                print("  %-14s %9.1f us  (dense conv_forward on the block-diagonal weight, %d x the FLOP; max |difference| / max |y| = %.1e)"
                      "  grouped / dense = %.3f" % ("dense forward", td * 1e6, C // Cg, err, t / td))
                del wd, yd, y
            except Exception as e:   # (recorded, not hidden: the dense path refusing a shape is a result)
                print("  dense forward  refused: %s: %s" % (type(e).__name__, e))
        del x, w, dy, dw, dx
        torch.cuda.empty_cache()
    if "--step" in sys.argv:
        step()


def step():
    """one observation: the bench's trainer (bench.py::build, untouched) on the ResNeXt-50 32x8d configuration at 1000 x 1000"""
    import bench
    import maskrcnn_benchmark.config as config
    base = config.make_default_cfg

    def resnext_cfg():
        cfg = base()
        cfg.merge_from_list(["MODEL.RESNETS.NUM_GROUPS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 8, "MODEL.RESNETS.STRIDE_IN_1X1", False])
        return cfg
    config.make_default_cfg = resnext_cfg
    try:
        cfg, trainer, batch = bench.build(torch.device("cuda", 0), 0)
    finally:
        config.make_default_cfg = base
    it = cfg.MT.START_MT + 400
    ms = []
    for i in range(8):
        data = batch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        losses = trainer.train_step(it + i, *data)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    assert all(torch.isfinite(v).item() for v in losses.values())
    print("mean-teacher step, R-50-FPN 32x8d (STRIDE_IN_1X1 False), 2 + 2 crops of 1000 x 1000: steps 4-8 median %.1f ms "
          "(all: %s) -- a single observation" % (statistics.median(ms[3:]), " ".join("%.1f" % m for m in ms)))


if __name__ == "__main__":
    main()
