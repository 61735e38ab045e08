"""The plane-fed weight gradient (csrc/conv_wgpl.hip) alone, on the step's plane-fed shapes: ms per call as tools/bench_wgrad.py
times them (events around 20 calls, planes attached beforehand), three repeats per shape.  `MMT_LIB=path` points the binding at
another build of libmmtpsm.so (A/B of two builds on one box: run the two alternately); prints one JSON line."""
import json, os, sys, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from maskrcnn_benchmark import _hip as hip
if os.environ.get("MMT_LIB"):
    hip.LIB_PATH = os.path.abspath(os.environ["MMT_LIB"])
hip.lib()
hip.set_conv_precision(3)
hip.set_f16x2(True)
def cl(x): return x.contiguous(memory_format=torch.channels_last)
SHAPES = [(2, 256, 256, 256, 256, 3), (2, 256, 128, 128, 256, 3), (2, 256, 64, 64, 256, 3), (2, 128, 128, 128, 128, 3),
          (2, 512, 32, 32, 512, 3), (4, 256, 64, 64, 256, 3)]
out = {}
for N, Cin, H, W, Cout, k in SHAPES:
    g = torch.Generator().manual_seed(N + Cin + H)
    x = cl(torch.randn(N, Cin, H, W, generator=g).relu().cuda())
    dy = cl((torch.randn(N, Cout, H, W, generator=g) * 1e-3).cuda())
    for t in (x, dy):
        t._mmt_amax = hip._amax_of(t)
        hip.f16_split_pg(t)
    dw = cl(torch.zeros(Cout, Cin, k, k, device='cuda'))
    n0 = hip.F16_STATS.get("wgrad_pl", 0)
    for _ in range(3): hip.conv_wgrad(x, dy, (Cout, Cin, k, k), 1, k // 2, dw)
    assert hip.F16_STATS.get("wgrad_pl", 0) == n0 + 3
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        it = 20; e0.record()
        for _ in range(it): hip.conv_wgrad(x, dy, (Cout, Cin, k, k), 1, k // 2, dw)
        e1.record(); torch.cuda.synchronize()
        ms.append(round(e0.elapsed_time(e1) / it * 1e3, 1))
    out["%d,%d,%d,%d,%d,%d" % (N, Cin, H, W, Cout, k)] = ms
print(json.dumps({"lib": hip.LIB_PATH, "us_per_call": out}))
