"""tests/det_worker.py with configuration keys: ONE fresh process that merges `--set KEY VALUE` pairs into the default configuration,
builds the bench's trainer from seed 0 on it, switches deterministic mode on (unless --off), takes a few mean-teacher steps and
prints det_worker's SHA-256 lines after every step -- two runs of it are compared line by line
(tests/test_deterministic_backbones_gpu.py).

Usage: python tests/det_cfg_worker.py [--set MODEL.BACKBONE.FREEZE_CONV_BODY_AT 0]... [--crop 160] [--n-inst 4] [--steps 3] [--off]"""
import argparse
import contextlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from det_worker import state_digests  # noqa: E402


@contextlib.contextmanager
def default_cfg_with(keys):
    """while it is open, make_default_cfg() returns the defaults with `keys` (a flat KEY, VALUE, ... list) merged in -- how
    tests/test_freeze_at_gpu.py::_trainer hands a key to bench.build"""
    import maskrcnn_benchmark.config as C
    keep = C.make_default_cfg

    def with_keys():
        cfg = keep()
        cfg.merge_from_list(list(keys))
        return cfg
    C.make_default_cfg = with_keys
    try:
        yield
    finally:
        C.make_default_cfg = keep


def build(keys, crop=160, n_inst=4, base_lr=0.005):
    """bench.build's (cfg, trainer, batch) from seed 0 on the defaults with `keys` merged in"""
    import bench
    torch.manual_seed(0)
    with default_cfg_with(keys):
        cfg, trainer, batch = bench.build(torch.device("cuda", 0), 0, crop=crop, n_inst=n_inst, base_lr=base_lr)
    trainer.seed_rng(0)
    return cfg, trainer, batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", nargs=2, action="append", default=[], metavar=("KEY", "VALUE"))
    ap.add_argument("--crop", type=int, default=160)
    ap.add_argument("--n-inst", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--off", action="store_true", help="the default mode (for comparison)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    from maskrcnn_benchmark import _hip as H
    H.set_deterministic(not a.off)
    cfg, trainer, batch = build([s for kv in a.set for s in kv], a.crop if a.crop else None, a.n_inst if a.n_inst else None)
    for i in range(a.steps):
        il, tg, ul = batch()
        losses = trainer.train_step(cfg.MT.START_MT + 400 + i, il, tg, ul)
        torch.cuda.synchronize()
        for name, h in state_digests(trainer, losses) + [("loss-names", ",".join(sorted(losses)))]:
            print("DIGEST step %d %s %s" % (i, name, h), flush=True)


if __name__ == "__main__":
    main()
