"""Deterministic mode with a trainable stem, which it used to refuse: the stem weight gradient now runs on its ordered form
(include/mmtpsm.h: mmt_stem_wgrad_ordered).

Configurations, merged into the bench's trainer (bench.build at 160 x 160, four instances, BASE_LR 0.005) the way
tests/test_freeze_at_gpu.py::_trainer does, three steps from START_MT + 400:
  (b) FREEZE_CONV_BODY_AT 0        (d) FREEZE_CONV_BODY_AT 1 (never refused, never shown to repeat either)
Two trainers from seed 0 in one process end every step with bit-identical student, momentum and teacher buffers and losses
(tests/test_deterministic_step_gpu.py::_first_difference, imported); so do two fresh processes on (b).  Not vacuous: the
mean-teacher losses are there, student and teacher moved, the stem filter moved in (b) and stayed in (d), a layer1 weight moved in
both, and (b) went through the ordered entry point and never through the unordered one (the counter is the `_hip._check` hook of
tools/call_hist.py and tests/test_deterministic_kernels_gpu.py: it lives inside that test's body, so the same four lines stand here).
Parity is kept: the oracle's step at FREEZE_CONV_BODY_AT 0 through tests/test_freeze_at_gpu.py's own helpers and tolerances with the
mode on.  With the mode off the step calls what it called before."""
import collections
import contextlib
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import det_cfg_worker as W  # noqa: E402
from test_deterministic_step_gpu import STEPS, _first_difference  # noqa: E402

CONFIGS = {
    "b-trainable-stem": ["MODEL.BACKBONE.FREEZE_CONV_BODY_AT", 0],
    "d-freeze-at-1": ["MODEL.BACKBONE.FREEZE_CONV_BODY_AT", 1],
}
STEM = "backbone.body.stem.conv1.weight"
LAYER1 = "backbone.body.layer1.0.conv2.weight"
WGRADS = ("mmt_stem_wgrad", "mmt_stem_wgrad_ordered")


@pytest.fixture()
def hip():
    from maskrcnn_benchmark import _hip as H
    H.lib()
    yield H
    H.set_deterministic(False)


@contextlib.contextmanager
def _counting(H):
    """the C-ABI call histogram: every direct library call passes through _hip._check with its symbol"""
    hist = collections.Counter()
    orig = H._check

    def counting(code, what):
        hist[what] += 1
        return orig(code, what)
    H._check = counting
    try:
        yield hist
    finally:
        H._check = orig


def _run(keys, steps=STEPS):
    """-> per step (student, momentum, teacher, losses), the slices of the student's flat buffer that hold STEM and LAYER1, cfg"""
    cfg, trainer, batch = W.build(keys)
    out = []
    for i in range(steps):
        il, tg, ul = batch()
        losses = trainer.train_step(cfg.MT.START_MT + 400 + i, il, tg, ul)
        torch.cuda.synchronize()
        assert "mt_fg_loss" in losses and "mt_classifier" in losses, sorted(losses)   # the mean-teacher branch is active
        out.append((trainer.flat_s.data.clone(), trainer.flat_s.momentum.clone(), trainer.flat_t.data.clone(),
                    {k: v.detach().clone() for k, v in losses.items()}))
    return out, {n: trainer.flat_s.index[n] for n in (STEM, LAYER1)}, cfg


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_two_trainers_in_one_process_stay_bit_identical(hip, name):
    H = hip
    keys = CONFIGS[name]
    stem = name.startswith("b")
    H.set_deterministic(True)
    with _counting(H) as hist:
        a, where, cfg = _run(keys)
        b, _, _ = _run(keys)
    H.set_deterministic(False)
    assert cfg.MODEL.BACKBONE.FREEZE_CONV_BODY_AT == keys[-1]
    diff = _first_difference(a, b)
    assert diff is None, diff
    first, last = a[0], a[STEPS - 1]
    assert not torch.equal(first[0], last[0]) and not torch.equal(first[2], last[2])   # SGD and the EMA moved
    for n, moves in ((STEM, stem), (LAYER1, True)):
        o, k = where[n]
        assert (not torch.equal(first[0][o:o + k], last[0][o:o + k])) == moves, (n, moves)
    counts = {k: hist[k] for k in WGRADS}
    print("deterministic %-18s stem weight-gradient calls %s" % (name, counts))
    assert counts["mmt_stem_wgrad"] == 0 and (counts["mmt_stem_wgrad_ordered"] > 0) == stem, counts


def _child(keys, env):
    cmd = [sys.executable, os.path.join(ROOT, "tests", "det_cfg_worker.py")]
    for k, v in zip(keys[0::2], keys[1::2]):
        cmd += ["--set", k, str(v)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    return out.returncode, [l for l in out.stdout.splitlines() if l.startswith("DIGEST ")], out.stderr[-2000:]


def test_two_fresh_processes_stay_bit_identical():
    env = dict(os.environ)
    env.pop("MMT_DETERMINISTIC", None)
    keys = CONFIGS["b-trainable-stem"]
    rc, first, err = _child(keys, env)
    assert rc == 0, err                       # (anything else: the second child is not started)
    assert len(first) == 5 * STEPS and all("mt_fg_loss" in l for l in first if " loss-names " in l), first
    rc, second, err = _child(keys, env)
    assert rc == 0, err
    assert first == second, [(a, b) for a, b in zip(first, second) if a != b][:1]


def test_a_deterministic_step_at_freeze_0_is_the_oracles_step(hip, synth, state_shapes, weights):
    """tests/test_freeze_at_gpu.py::test_full_step_matches_oracle at FREEZE_CONV_BODY_AT 0 (mean-teacher step) with the mode on: its
    helpers and the tolerances of tests/test_train_step_gpu.py::_check_step, called, not copied"""
    import test_freeze_at_gpu as tf
    H = hip
    H.set_deterministic(True)
    with _counting(H) as hist:
        tf.test_full_step_matches_oracle(synth, state_shapes, weights, 0, 1400)
    assert hist["mmt_stem_wgrad_ordered"] > 0 and hist["mmt_stem_wgrad"] == 0, {k: hist[k] for k in WGRADS}


def test_mode_off_calls_the_unordered_entry_point(hip):
    H = hip
    H.set_deterministic(False)
    with _counting(H) as hist:
        _run(CONFIGS["b-trainable-stem"], steps=1)
    counts = {k: hist[k] for k in WGRADS}
    assert counts["mmt_stem_wgrad"] > 0 and counts["mmt_stem_wgrad_ordered"] == 0, counts
