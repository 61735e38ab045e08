"""The bare backbone at FREEZE_CONV_BODY_AT 2, 1 and 0 on the student's full-size pair (2 + 2 images of 1024 x 1024): the stem alone
(one-launch and un-fused), forward_pair, and forward_pair + backward of both halves, device time between events, median of 8 after
3 warm-ups; at 0 also the two kernels of the stem's backward at N = 2.  What the key costs inside the student's backbone pass, to
set against the whole step of tools/freeze_steps.py.
  python freeze_backbone.py"""
import os
import statistics
import sys

import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
from maskrcnn_benchmark import _hip as H
from maskrcnn_benchmark.config import make_default_cfg
from maskrcnn_benchmark.modeling.backbone.backbone import build_backbone, forward_pair
from maskrcnn_benchmark.layers import fused
H.lib()


def timed(fn, n=8, warm=3):
    out = []
    for i in range(warm + n):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warm:
            out.append(a.elapsed_time(b))
    return statistics.median(out)


g = torch.Generator().manual_seed(0)
xa = (torch.randn((2, 3, 1024, 1024), generator=g) * 60).cuda()
xb = (torch.randn((2, 3, 1024, 1024), generator=g) * 60).cuda()
for fa in (2, 1, 0):
    cfg = make_default_cfg()
    cfg.merge_from_list(["MODEL.BACKBONE.FREEZE_CONV_BODY_AT", fa])
    bb = build_backbone(cfg).cuda().train()
    st = bb.body.stem
    xc = torch.cat([xa, xb], 0)
    with torch.no_grad():
        print("freeze_at %d: stem(x) no-grad N=4 %.3f ms; forward_raw N=4 %.3f ms" % (fa, timed(lambda: st(xc)), timed(lambda: st.forward_raw(xc))))
    def fwd():
        return forward_pair(bb, xa, xb)
    def fb():
        pa, pb = forward_pair(bb, xa, xb)
        (sum(p.sum() for p in pa) + sum(p.sum() for p in pb)).backward()
        fused.join_wgrads()
    print("freeze_at %d: forward_pair %.3f ms; forward_pair + backward %.3f ms (device time between events)" % (fa, timed(fwd), timed(fb)))
    if fa == 0:
        with torch.no_grad():
            y, p = st.forward_raw(xa)
        gp = torch.randn_like(p)
        dw = torch.zeros((64, 7, 7, 3), device="cuda").permute(0, 3, 1, 2)
        print("  N=2: maxpool_bwd %.3f ms, stem_wgrad %.3f ms" % (timed(lambda: H.maxpool3x3s2_backward(y, gp)), timed(lambda: H.stem_wgrad(xa, y, dw))))
    del bb
