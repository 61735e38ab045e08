"""The two kernels of the stem's backward (csrc/stem_bwd.hip) at the student's full-size batch, N = 4 x 1024^2: time per launch,
bytes/s against the compulsory traffic and, for the weight gradient, FLOP/s against the fp32-input MFMA peak.
  python bench_stem_bwd.py [N] [size]
10 launches per event pair, median of 20 pairs after 3 warm-up pairs.  Compulsory traffic: max-pool backward reads y and g once and
writes dy once; the weight gradient reads the image and dy once (dw is 37 KB).  FLOP: 2 x 64 x 147 per output pixel."""
import os
import statistics
import sys

import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
from maskrcnn_benchmark import _hip as H

PEAK_F32_MFMA = 157.3e12   # FLOP/s, MI355X data sheet: fp32 matrix
PEAK_HBM = 8.0e12          # B/s

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4
S = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
H.lib()
g = torch.Generator().manual_seed(0)
x = (torch.randn((N, 3, S, S), generator=g) * 60.0).cuda()
Ho = (S - 1) // 2 + 1
Hp = (Ho - 1) // 2 + 1
y = torch.relu(torch.randn((N, 64, Ho, Ho), generator=g)).cuda().contiguous(memory_format=torch.channels_last)
gp = torch.randn((N, 64, Hp, Hp), generator=g).cuda().contiguous(memory_format=torch.channels_last)
dy = torch.empty_like(y)
dw = torch.zeros((64, 7, 7, 3), device="cuda").permute(0, 3, 1, 2)
scale = (torch.rand(64, generator=g) + 0.5).cuda()


def timed(fn, per=10, pairs=20, warm=3):
    out = []
    for i in range(warm + pairs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        b.synchronize()
        if i >= warm:
            out.append(a.elapsed_time(b) * 1e3 / per)   # us per launch
    return statistics.median(out), min(out), max(out)


print("stem backward kernels at N = %d, %d x %d (y %d x %d, pooled %d x %d); median [min .. max] of 20 x 10 launches" % (N, S, S, Ho, Ho, Hp, Hp))
med, lo, hi = timed(lambda: H.maxpool3x3s2_backward(y, gp, out=dy))
bytes_ = 4.0 * (2 * y.numel() + gp.numel())
print("mmt_maxpool3x3s2_backward  %8.1f us [%.1f .. %.1f]   %.2f TB/s of compulsory traffic (%.0f MB) = %.0f %% of %.1f TB/s"
      % (med, lo, hi, bytes_ / med / 1e6, bytes_ / 1e6, 100 * bytes_ / (med * 1e-6) / PEAK_HBM, PEAK_HBM / 1e12))
med, lo, hi = timed(lambda: H.stem_wgrad(x, y, dw, scale))
bytes_ = 4.0 * (x.numel() + y.numel())
flop = 2.0 * 64 * 147 * N * Ho * Ho
print("mmt_stem_wgrad             %8.1f us [%.1f .. %.1f]   %.2f TB/s of compulsory traffic (%.0f MB) = %.0f %% of %.1f TB/s;  "
      "%.1f TFLOP/s (%.1f GFLOP) = %.0f %% of the %.0f TFLOP/s fp32-MFMA peak"
      % (med, lo, hi, bytes_ / med / 1e6, bytes_ / 1e6, 100 * bytes_ / (med * 1e-6) / PEAK_HBM, PEAK_HBM / 1e12,
         flop / med / 1e6, flop / 1e9, 100 * flop / (med * 1e-6) / PEAK_F32_MFMA, PEAK_F32_MFMA / 1e12))
