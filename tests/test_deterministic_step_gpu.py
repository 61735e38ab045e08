"""Deterministic mode, the whole training step (`_hip.set_deterministic`): same seed, same build, same weights and batches -> after
every `train_step` the student's flat buffer, its momentum buffer, the teacher's flat buffer and every loss are bit-identical, in one
process and in two fresh ones, in the default schedule and with MMT_OVERLAP_TEACHER=0, in arithmetic modes 3 and 0, with IR-Net off
and on; and a deterministic step is still the oracle's step."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

STEPS = 3


@pytest.fixture()
def hip():
    from maskrcnn_benchmark import _hip as H
    H.lib()
    prev = H.get_conv_precision()
    yield H
    H.set_deterministic(False)
    if H.get_conv_precision() != prev:
        H.set_conv_precision(prev)


def _run(irnet):
    """a trainer built from seed 0 takes STEPS mean-teacher steps -> per step (student, momentum, teacher, losses)"""
    import bench
    torch.manual_seed(0)
    cfg, trainer, batch = bench.build(torch.device("cuda", 0), 0, irnet=irnet, crop=160, n_inst=4, base_lr=0.005)
    trainer.seed_rng(0)
    out = []
    for i in range(STEPS):
        il, tg, ul = batch()
        losses = trainer.train_step(cfg.MT.START_MT + 400 + i, il, tg, ul)
        torch.cuda.synchronize()
        assert "mt_fg_loss" in losses and "mt_classifier" in losses, sorted(losses)   # the mean-teacher branch is active
        out.append((trainer.flat_s.data.clone(), trainer.flat_s.momentum.clone(), trainer.flat_t.data.clone(),
                    {k: v.detach().clone() for k, v in losses.items()}))
    return out


def _first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        for name, u, v in zip(("student", "momentum", "teacher"), x[:3], y[:3]):
            if not torch.equal(u, v):
                return "step %d, %s: %d of %d elements differ" % (i, name, int((u != v).sum()), u.numel())
        assert set(x[3]) == set(y[3])
        for k in sorted(x[3]):
            if not torch.equal(x[3][k], y[3][k]):
                return "step %d, loss %s: %r vs %r" % (i, k, float(x[3][k]), float(y[3][k]))
    return None


@pytest.mark.parametrize("irnet", [False, True], ids=["plain", "irnet"])
@pytest.mark.parametrize("mode", [3, 0], ids=["default-f16x2-split", "fp32-mfma"])
@pytest.mark.parametrize("overlap", [True, False], ids=["teacher-on-side-stream", "serial"])
def test_two_trainers_in_one_process_stay_bit_identical(hip, monkeypatch, overlap, mode, irnet):
    H = hip
    monkeypatch.setenv("MMT_OVERLAP_TEACHER", "1" if overlap else "0")
    H.set_conv_precision(mode)
    H.set_deterministic(True)
    a = _run(irnet)
    b = _run(irnet)
    H.set_deterministic(False)
    diff = _first_difference(a, b)
    assert diff is None, diff
    assert not torch.equal(a[0][0], a[STEPS - 1][0]) and not torch.equal(a[0][2], a[STEPS - 1][2])   # SGD and the EMA moved


def test_default_mode_for_the_record(hip, capsys):
    """printed, not asserted: do two runs of the same three steps differ with the mode off?"""
    H = hip
    H.set_deterministic(False)
    diff = _first_difference(_run(False), _run(False))
    with capsys.disabled():
        print("\nmode off, two trainers from seed 0: %s" % (diff or "no difference in %d steps" % STEPS))


def _child(extra, env):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "det_worker.py")] + extra, env=env, capture_output=True, text=True,
                         timeout=240)
    return out.returncode, [l for l in out.stdout.splitlines() if l.startswith("DIGEST ")], out.stderr[-2000:]


@pytest.mark.parametrize("irnet", [False, True], ids=["plain", "irnet"])
def test_two_fresh_processes_stay_bit_identical(irnet):
    env = dict(os.environ)
    env.pop("MMT_DETERMINISTIC", None)
    extra = ["--irnet"] if irnet else []
    rc, first, err = _child(extra, env)
    assert rc == 0, err                       # (anything else: the second child is not started)
    assert len(first) == 5 * STEPS and all("mt_fg_loss" in l for l in first if " loss-names " in l), first
    rc, second, err = _child(extra, env)
    assert rc == 0, err
    assert first == second, [(a, b) for a, b in zip(first, second) if a != b][:1]


def test_a_deterministic_step_is_the_oracles_step(hip, synth, state_shapes, weights):
    """parity is not lost: tests/test_train_step_gpu.py::test_full_step_matches_oracle (mean-teacher step, first step) with the mode on,
    its tolerances (_check_step) imported, not copied"""
    import test_train_step_gpu as ts
    from maskrcnn_benchmark.utils.replay import Replay
    import bench
    H = hip
    H.set_deterministic(True)
    iteration = 1400
    cfg, trainer, batch = bench.build(torch.device("cuda", 0), 0, crop=160, n_inst=4)
    ts._load(trainer, weights)
    H.rb_reset()
    om, ot = ts._oracle_trainer(synth, state_shapes, weights)
    imgs, tgs = synth.make_labeled(2, 160, 4, seed=1234)
    unl = synth.make_unlabeled(2, 160, 3, seed=4321)
    ot.last_epoch = trainer.scheduler.last_epoch
    ref_losses, (ta, tb, tc) = ot.step(iteration, imgs, ts._oracle_targets(om, tgs), unl, seeds=(99, 100, 101))
    before_s = {n: ts._param(trainer.flat_s, trainer.student, n) for n in state_shapes["param_order"]}
    before_t = {n: ts._param(trainer.flat_t, trainer.teacher, n) for n in state_shapes["param_order"]}
    stu = {"rpn_sampler": ta["rpn_sampler"], "roi_sampler": ta["roi_sampler"], "rpn_proposals": ta["rpn_proposals"],
           "dropout": list(ta["dropout"]) + list(tc.get("dropout", []))}
    trainer.student.set_replay(Replay(stu))
    trainer.teacher.set_replay(Replay(tb))
    try:
        il, tg, ul = batch()
        losses = trainer.train_step(iteration, il, tg, ul)
        torch.cuda.synchronize()
    finally:
        trainer.student.set_replay(None)
        trainer.teacher.set_replay(None)
        H.set_deterministic(False)
    try:
        ts._check_step(cfg, trainer, ot, state_shapes, weights, losses, ref_losses, before_s, before_t, iteration)
    finally:
        H.rb_reset()
