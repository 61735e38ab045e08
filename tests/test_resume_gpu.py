"""Resuming a mean-teacher run from its checkpoint (engine/MTtrainer.py::save_model / resume): in deterministic mode a run that was
saved after step 2 and resumed -- in a trainer seeded differently, in the same process or a fresh one, step by step or through
`train()` -- ends in the same bits as the run that kept going; before the teacher moves the initial teacher comes back, not the
student; in the default mode the buffers come back exactly and training goes on.  The trainer is tests/test_deterministic_step_gpu.py's
(the bench's at 160 x 160, iterations from START_MT + 400: consistency branch and EMA active)."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)


@pytest.fixture()
def hip():
    from maskrcnn_benchmark import _hip as H
    H.lib()
    yield H
    H.set_deterministic(False)


def _build(save_dir, irnet=False):
    import bench
    from maskrcnn_benchmark.utils.checkpoint import Checkpointer
    cfg, trainer, batch = bench.build(torch.device("cuda", 0), 0, irnet=irnet, crop=160, n_inst=4, base_lr=0.005)
    trainer.ckpt_s = Checkpointer(trainer.student, trainer.optimizer, trainer.scheduler, save_dir=str(save_dir), save_to_disk=True)
    trainer.ckpt_t = Checkpointer(trainer.teacher, save_dir=str(save_dir), save_to_disk=True)
    return cfg, trainer, batch


def _buffers(trainer):
    torch.cuda.synchronize()
    return trainer.flat_s.data.clone(), trainer.flat_s.momentum.clone(), trainer.flat_t.data.clone()


def _step(cfg, trainer, batch, step):
    """step 1, 2, ... = iteration START_MT + 400, + 401, ... -> (student, momentum, teacher, losses)"""
    il, tg, ul = batch()
    losses = trainer.train_step(cfg.MT.START_MT + 399 + step, il, tg, ul)
    assert "mt_fg_loss" in losses and "mt_classifier" in losses, sorted(losses)   # the mean-teacher branch is active
    return _buffers(trainer) + ({k: v.detach().clone() for k, v in losses.items()},)


def _difference(x, y):
    for name, u, v in zip(("student", "momentum", "teacher"), x[:3], y[:3]):
        if not torch.equal(u, v):
            return "%s: %d of %d elements differ" % (name, int((u != v).sum()), u.numel())
    if set(x[3]) != set(y[3]):
        return "losses %s vs %s" % (sorted(x[3]), sorted(y[3]))
    for k in sorted(x[3]):
        if not torch.equal(x[3][k], y[3][k]):
            return "loss %s: %r vs %r" % (k, float(x[3][k]), float(y[3][k]))
    return None


def _scramble(trainer):
    """the random streams of a trainer that is about to resume: anything but the saved run's"""
    trainer.seed_rng(7)
    random.seed(99)
    np.random.seed(98)


@pytest.mark.parametrize("irnet", [False, True], ids=["plain", "irnet"])
def test_resumed_run_is_the_straight_run(hip, tmp_path, irnet):
    H = hip
    H.set_deterministic(True)
    torch.manual_seed(0)
    cfg, a, batch = _build(tmp_path, irnet)
    a.seed_rng(0)
    straight = {}
    for step in (1, 2, 3, 4):
        straight[step] = _step(cfg, a, batch, step)
        if step == 2:
            a.save_model(cfg.MT.START_MT + 401)
    del a
    torch.manual_seed(123)
    cfg, b, batch = _build(tmp_path, irnet)
    _scramble(b)
    at = b.resume()
    assert at == cfg.MT.START_MT + 401 and b.start_iter == at + 1
    for step in (3, 4):
        diff = _difference(straight[step], _step(cfg, b, batch, step))
        assert diff is None, "step %d, %s" % (step, diff)
    assert all(not torch.equal(u, v) for u, v in zip(straight[2][:3], straight[4][:3]))   # SGD, momentum and the EMA moved on


def _child(args, env):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "resume_worker.py")] + args, env=env, capture_output=True, text=True,
                         timeout=240)
    return out.returncode, [l for l in out.stdout.splitlines() if l.startswith("DIGEST ")], out.stderr[-2000:]


@pytest.mark.parametrize("irnet", [False, True], ids=["plain", "irnet"])
def test_resumed_in_a_fresh_process(tmp_path, irnet):
    env = dict(os.environ)
    env.pop("MMT_DETERMINISTIC", None)
    extra = ["--irnet"] if irnet else []
    rc, straight, err = _child([str(tmp_path), "straight"] + extra, env)
    assert rc == 0, err                       # (anything else: the second child is not started)
    assert len(straight) == 5 * 4 and all("mt_fg_loss" in l for l in straight if " loss-names " in l), straight
    rc, resumed, err = _child([str(tmp_path), "resume"] + extra, env)
    assert rc == 0, err
    tail = [l for l in straight if l.startswith(("DIGEST step 3 ", "DIGEST step 4 "))]
    assert len(resumed) == 5 * 2 and resumed == tail, [(x, y) for x, y in zip(tail, resumed) if x != y][:1]


def test_resume_before_the_teacher_moves(hip, tmp_path, synth):
    """below START_MT - 10 the EMA has not run: the teacher is the INITIAL copy, and that -- not the student -- is what comes back"""
    cfg, a, batch = _build(tmp_path)
    initial = a.flat_t.data.clone()
    for iteration in (1, 2):
        assert iteration < cfg.MT.START_MT - 10
        il, tg, _ = batch()
        a.train_step(iteration, il, tg, None)
    a.save_model(2)
    student, momentum, teacher = _buffers(a)
    rng = a.rng_state()
    assert torch.equal(teacher, initial) and not torch.equal(student, initial)
    assert not os.path.exists(os.path.join(str(tmp_path), "t_model_0000002.pth"))     # (the teacher's own file: past START_MT only)
    torch.manual_seed(123)
    cfg, b, batch = _build(tmp_path)
    other = synth.make_weights({k: tuple(v.shape) for k, v in b.student.state_dict().items()}, seed=1)
    b.student.load_state_dict(other, strict=False)
    b.teacher.load_state_dict(other, strict=False)
    _scramble(b)
    assert not torch.equal(b.flat_t.data, initial)
    assert b.resume() == 2 and b.start_iter == 3
    torch.cuda.synchronize()
    assert torch.equal(b.flat_t.data, initial) and torch.equal(b.flat_s.data, student) and torch.equal(b.flat_s.momentum, momentum)
    assert not torch.equal(b.flat_t.data, b.flat_s.data)
    assert b.optimizer.steps == a.optimizer.steps == 2 and b.scheduler.last_epoch == a.scheduler.last_epoch
    assert b.optimizer.lr_factor == a.optimizer.lr_factor
    assert b.optimizer.param_groups[0]["lr"] == a.optimizer.param_groups[0]["lr"] == a.optimizer.base_lr * a.optimizer.lr_factor
    got = b.rng_state()
    for k in ("gen_s", "gen_t", "torch_cpu", "torch_device"):
        assert torch.equal(got[k], rng[k]), k
    assert got["python"] == rng["python"]
    assert torch.equal(got["numpy"]["keys"], rng["numpy"]["keys"]) and got["numpy"]["pos"] == rng["numpy"]["pos"]


def test_default_mode(hip, tmp_path):
    H = hip
    assert not H.get_deterministic()
    torch.manual_seed(0)
    cfg, a, batch = _build(tmp_path)
    for step in (1, 2):
        _step(cfg, a, batch, step)
    at_save = _buffers(a)
    sites = len(H._RB[0].sites)
    a.save_model(cfg.MT.START_MT + 401)
    assert sites > 0 and len(H._RB[0].sites) == sites      # outside deterministic mode a save leaves the adaptive state alone
    assert os.path.exists(os.path.join(str(tmp_path), "t_model_%07d.pth" % (cfg.MT.START_MT + 401)))
    del a
    torch.manual_seed(123)
    cfg, b, batch = _build(tmp_path)
    _scramble(b)
    assert b.resume() == cfg.MT.START_MT + 401
    assert all(torch.equal(u, v) for u, v in zip(at_save, _buffers(b)))
    after = _step(cfg, b, batch, 3)
    assert all(bool(torch.isfinite(v)) for v in after[3].values()), after[3]
    assert not torch.equal(after[0], at_save[0])


def _loaders(batch, n=5):
    """n labeled and n unlabeled batches as list loaders; unlabeled batch j is scaled by (1 + j / 32): which one a step gets matters"""
    labeled, unlabeled = [], []
    for j in range(n):
        il, tg, ul = batch()
        for u in ul:
            u.tensors = u.tensors * (1.0 + j / 32.0)
        labeled.append((il, tg, j))
        unlabeled.append((ul, j))
    return labeled, unlabeled


def _record_unlabeled(trainer, unlabeled):
    """-> the list that fills with the marks of the unlabeled batches `train_step` receives"""
    marks, got, step = {id(ul): j for ul, j in unlabeled}, [], trainer.train_step

    def train_step(iteration, data_s, target_s, data_u=None):
        got.append(marks[id(data_u)])
        return step(iteration, data_s, target_s, data_u)
    trainer.train_step = train_step
    return got


def test_the_loop_resumes(hip, tmp_path):
    H = hip
    H.set_deterministic(True)
    torch.manual_seed(0)
    cfg, a, batch = _build(tmp_path)
    a.seed_rng(0)
    first = cfg.MT.START_MT + 400
    labeled, unlabeled = _loaders(batch)
    a.dataloader_s, a.dataloader_u, a.start_iter = labeled, unlabeled, first
    a.checkpoint_period = first + 1                        # one save, after the second batch
    got = _record_unlabeled(a, unlabeled)
    a.train()
    assert got == [0, 1, 2, 3, 4] and a.unlabeled_seen == 5
    saved = sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("model_"))
    assert saved == ["model_%07d.pth" % (first + 1)], saved
    straight = _buffers(a)
    del a
    torch.manual_seed(123)
    cfg, b, batch = _build(tmp_path)
    _scramble(b)
    labeled, unlabeled = _loaders(batch)
    b.dataloader_s, b.dataloader_u = labeled[2:], unlabeled     # the labeled loader is the caller's to position
    b.checkpoint_period = first + 1
    got = _record_unlabeled(b, unlabeled)
    assert b.resume() == first + 1 and b.unlabeled_seen == 2
    b.train()
    assert got == [2, 3, 4] and b.unlabeled_seen == 5 and b.last_iteration == first + 4
    resumed = _buffers(b)
    for name, u, v in zip(("student", "momentum", "teacher"), straight, resumed):
        assert torch.equal(u, v), "%s: %d of %d elements differ" % (name, int((u != v).sum()), u.numel())
