"""The ordered form of the stem weight gradient (deterministic mode; csrc/stem_bwd.hip, csrc/ordered.h) beside the atomic form,
through the C ABI on inputs already on the device.

Shape: the stem at N = --batch images of --side x --side.  Arms: `atomic` = mmt_stem_wgrad (this build's kernel with a null
workspace: the kernel as it was plus one wave-uniform branch in the epilogue), `ordered` = mmt_stem_wgrad_ordered (stage one + the
finish launch) on a workspace allocated once.
After warm-up, --reps repetitions in which the arms take turns (the order rotates); an arm's sample is --inner back-to-back calls
between two device events, divided by --inner.  Medians, with the range, the workspace bytes, and what the workspace traffic alone
(written once, read once) costs at the measured HBM copy rate (--hbm-tbs).

    python mmt-psm_amd/tools/bench_ordered_wgrad.py > profiles/ordered_wgrad.txt"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
from maskrcnn_benchmark import _hip


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--side", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--hbm-tbs", type=float, default=6.29)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ordered_wgrad.py measures on the MI355X; no GPU visible")
    L, dev, st = _hip.lib(), torch.device("cuda", 0), _hip._stream
    cases = []
    N, S = a.batch, a.side
    x, dy = torch.randn((N, 3, S, S), device=dev), cl(torch.randn((N, 64, S // 2, S // 2), device=dev))
    dw = torch.zeros((64 * 147,), device=dev)
    need = L.mmt_stem_wgrad_ws_floats(N, S, S)
    ws = torch.empty((need,), device=dev)
    shape = (x.data_ptr(), dy.data_ptr(), None, dw.data_ptr(), N, S, S)
    cases.append(("stem %d^2 N %d" % (S, N), need, (x, dy, dw, ws), lambda shape=shape: L.mmt_stem_wgrad(*shape, st()),
                  lambda shape=shape, ws=ws, need=need: L.mmt_stem_wgrad_ordered(*shape, ws.data_ptr(), need, st())))

    p = torch.cuda.get_device_properties(0)
    print("box: %s (%s), %d compute units, torch %s, HIP %s" % (p.name, getattr(p, "gcnArchName", "?"), p.multi_processor_count,
                                                                 torch.__version__, torch.version.hip))
    print("us per call by device events over %d back-to-back calls, %d repetitions, arms in turn: median (min .. max)" % (a.inner, a.reps))
    for name, need, _keep, atomic, ordered in cases:
        arms = [("atomic", atomic), ("ordered", ordered)]
        for _, f in arms:
            for _ in range(3):
                assert f() == 0
        torch.cuda.synchronize()
        times = {n: [] for n, _ in arms}
        for r in range(a.reps):
            for k in range(2):
                n, f = arms[(k + r) % 2]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.inner):
                    f()
                e1.record()
                torch.cuda.synchronize()
                times[n].append(e0.elapsed_time(e1) * 1e3 / a.inner)
        ta, to = times["atomic"], times["ordered"]
        print("  %-30s atomic %8.1f (%.1f .. %.1f)   ordered %8.1f (%.1f .. %.1f)   x %.2f   workspace %7.2f MB: %.1f us written + read at %.2f TB/s"
              % (name, float(np.median(ta)), min(ta), max(ta), float(np.median(to)), min(to), max(to), float(np.median(to)) / float(np.median(ta)),
                 4 * need / 1e6, 2 * 4 * need / (a.hbm_tbs * 1e12) * 1e6, a.hbm_tbs))


if __name__ == "__main__":
    main()
