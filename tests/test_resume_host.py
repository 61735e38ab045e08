"""Resuming a mean-teacher run, the host side (engine/MTtrainer.py::state_dict / save_model / resume, utils/checkpoint.py::save): what
`resume` refuses, what it restores, how the unlabeled loader is fast-forwarded, and that a checkpoint file appears whole or not at all.
Tiny CPU models on flat storage stand in for the detectors -- no kernel is on this path; the steps themselves are in
tests/test_resume_gpu.py."""
import logging
import os
import random

import numpy as np
import pytest
import torch
from torch import nn

from conftest import GOLD


class _Tiny(nn.Module):
    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a = nn.Linear(4, 3)
        self.b = nn.Linear(3, 2)
        for p in self.parameters():
            p.data.copy_(torch.randn(p.shape, generator=g))

    def set_rng(self, generator):
        pass


def _trainer(save_dir, seed=0, unlabeled=None):
    from maskrcnn_benchmark.config import make_default_cfg
    from maskrcnn_benchmark.engine.MTtrainer import MTtrainer
    from maskrcnn_benchmark.engine.flat import flatten_model
    from maskrcnn_benchmark.solver.build import FlatSGD, WarmupMultiStepLR
    from maskrcnn_benchmark.utils.checkpoint import Checkpointer
    cfg = make_default_cfg()
    student, teacher = _Tiny(seed), _Tiny(seed + 100)
    opt = FlatSGD(flatten_model(student), 0.01, 0.9, 1e-4, 2.0, 0.0)
    sched = WarmupMultiStepLR(opt, (30, 40), warmup_iters=10)
    ckpt = Checkpointer(student, opt, sched, save_dir=str(save_dir), save_to_disk=True)
    return MTtrainer(student, teacher, {"source": [None] * 50, "no_label": unlabeled}, opt, sched, ckpt, None, 10 ** 9, cfg)


def _advance(t, seed):
    """some run state worth restoring: momentum, schedule, counters, random streams"""
    g = torch.Generator().manual_seed(seed)
    t.flat_s.momentum.copy_(torch.randn(t.flat_s.momentum.shape, generator=g))
    pad = torch.ones_like(t.flat_s.momentum, dtype=torch.bool)
    for n, (o, k) in t.flat_s.index.items():
        pad[o:o + k] = False
    t.flat_s.momentum[pad] = 0          # the padding between slots is never written by a step
    for _ in range(7 + seed):
        t.scheduler.step()
    t.optimizer.steps = 7 + seed
    t.unlabeled_seen, t.skipped_pairs, t.last_iteration = 13 + seed, 2 + seed, 6 + seed
    torch.manual_seed(500 + seed)
    random.seed(600 + seed)
    np.random.seed(700 + seed)


@pytest.fixture()
def saved(tmp_path):
    t = _trainer(tmp_path)
    _advance(t, 1)
    t.save_model(t.last_iteration)
    return t, os.path.join(str(tmp_path), "model_%07d.pth" % t.last_iteration)


def _rewrite(path, change):
    d = torch.load(path, map_location="cpu")
    change(d)
    torch.save(d, path)


def _same_rng(a, b):
    assert set(a) == set(b)
    for k in ("gen_s", "gen_t", "torch_cpu", "torch_device"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or torch.equal(a[k], b[k])), k
    assert a["python"] == b["python"]
    assert torch.equal(a["numpy"]["keys"], b["numpy"]["keys"]) and {k: v for k, v in a["numpy"].items() if k != "keys"} == \
        {k: v for k, v in b["numpy"].items() if k != "keys"}


def test_state_is_restored_into_another_trainer(saved, tmp_path):
    a, path = saved
    entry = torch.load(path, map_location="cpu")
    assert {"model", "optimizer", "scheduler", "iteration", "trainer"} == set(entry) and entry["iteration"] == 7
    tr = entry["trainer"]
    assert set(tr) == {"format", "iteration", "optimizer", "scheduler", "teacher", "rng", "unlabeled_seen", "skipped_pairs",
                       "world_size", "deterministic", "checksums"}
    assert tr["format"] == 1 and tr["world_size"] == 1 and len(tr["rng"]) == 1 and tr["deterministic"] is False
    assert all(type(v) is int for v in tr["checksums"].values()) and set(tr["checksums"]) == {"student", "momentum", "teacher"}
    rng_at_save = a.rng_state()
    b = _trainer(tmp_path, seed=5)
    _advance(b, 3)
    assert not torch.equal(a.flat_s.data, b.flat_s.data) and not torch.equal(a.flat_t.data, b.flat_t.data)
    assert b.resume() == 7 and b.start_iter == 8 and b.last_iteration == 7
    assert torch.equal(a.flat_s.data, b.flat_s.data) and torch.equal(a.flat_s.momentum, b.flat_s.momentum)
    assert torch.equal(a.flat_t.data, b.flat_t.data) and not torch.equal(b.flat_t.data, b.flat_s.data)
    assert b.optimizer.steps == a.optimizer.steps == 8 and b.scheduler.last_epoch == a.scheduler.last_epoch
    assert b.optimizer.lr_factor == a.optimizer.lr_factor
    assert b.optimizer.param_groups[0]["lr"] == a.optimizer.base_lr * a.optimizer.lr_factor
    assert (b.unlabeled_seen, b.skipped_pairs) == (14, 3)
    _same_rng(b.rng_state(), rng_at_save)
    assert torch.equal(torch.rand(3), torch.rand(3, generator=torch.Generator().set_state(rng_at_save["torch_cpu"])))
    assert b.resume(path) == 7                                     # by name


def test_missing_file(tmp_path):
    t = _trainer(tmp_path)
    with pytest.raises(FileNotFoundError):
        t.resume()                                                  # no last_checkpoint in the directory
    with pytest.raises(FileNotFoundError):
        t.resume(os.path.join(str(tmp_path), "model_0000001.pth"))
    t.ckpt_s.tag_last_checkpoint(os.path.join(str(tmp_path), "gone.pth"))
    with pytest.raises(FileNotFoundError):
        t.resume()                                                  # a tag that names a file that is not there


def test_file_without_trainer_entry(saved, tmp_path):
    a, path = saved
    before = a.flat_s.data.clone()
    _rewrite(path, lambda d: d.pop("trainer"))
    with pytest.raises(ValueError, match="Checkpointer.load"):
        a.resume(path)
    with pytest.raises(ValueError, match="no `trainer` entry"):
        a.resume(os.path.join(GOLD, "checkpoint_ref_tiny.pth"))     # a file the reference wrote
    assert torch.equal(a.flat_s.data, before) and a.start_iter == 0


def test_other_format(saved):
    a, path = saved
    _rewrite(path, lambda d: d["trainer"].__setitem__("format", 2))
    with pytest.raises(ValueError, match="format 2"):
        a.resume(path)


def test_other_world_size(saved):
    a, path = saved
    _rewrite(path, lambda d: d["trainer"].__setitem__("world_size", 2))
    with pytest.raises(RuntimeError, match="world size 2"):
        a.resume(path)


def test_momentum_of_another_shape_and_unknown_name_are_both_listed(saved):
    a, path = saved
    before = (a.flat_s.data.clone(), a.flat_s.momentum.clone(), a.flat_t.data.clone())

    def change(d):
        m = d["trainer"]["optimizer"]["momentum_buffers"]
        m["a.weight"] = torch.zeros(5, 4)
        m["c.weight"] = torch.zeros(2, 2)
        del m["b.bias"]
    _rewrite(path, change)
    with pytest.raises(ValueError) as e:
        a.resume(path)
    msg = str(e.value)
    assert "momentum a.weight" in msg and "[5, 4]" in msg and "momentum c.weight" in msg and "momentum b.bias" in msg
    assert all(torch.equal(x, y) for x, y in zip(before, (a.flat_s.data, a.flat_s.momentum, a.flat_t.data)))   # nothing was written


def test_parameter_names_and_shapes(saved):
    a, path = saved

    def change(d):
        d["model"]["a.weight"] = torch.zeros(3, 5)
        d["trainer"]["teacher"]["extra.bias"] = torch.zeros(1)
        del d["trainer"]["teacher"]["b.weight"]
    _rewrite(path, change)
    with pytest.raises(ValueError) as e:
        a.resume(path)
    msg = str(e.value)
    assert "student a.weight" in msg and "teacher extra.bias" in msg and "teacher b.weight" in msg


@pytest.mark.parametrize("which", ["student", "momentum", "teacher"])
def test_corrupted_checksum(saved, which):
    a, path = saved
    _rewrite(path, lambda d: d["trainer"]["checksums"].__setitem__(which, d["trainer"]["checksums"][which] + 1))
    with pytest.raises(RuntimeError, match="restored %s buffer" % which):
        a.resume(path)


def test_a_changed_weight_fails_its_checksum(saved):
    a, path = saved
    _rewrite(path, lambda d: d["model"]["b.weight"].mul_(1.5))
    with pytest.raises(RuntimeError, match="student"):
        a.resume(path)


def test_deterministic_mode_mismatch_only_warns(saved, caplog):
    a, path = saved
    _rewrite(path, lambda d: d["trainer"].__setitem__("deterministic", True))
    with caplog.at_level(logging.WARNING, logger="maskrcnn_benchmark.trainer"):
        assert a.resume(path) == 7
    assert any("bit-for-bit guarantee" in r.getMessage() for r in caplog.records)


def test_killed_save_leaves_the_previous_checkpoint(saved, tmp_path, monkeypatch):
    a, first = saved
    real = torch.save

    def dies_half_way(obj, f, *args, **kwargs):
        with open(f, "wb") as h:
            h.write(b"half a checkpoint")
        raise KeyboardInterrupt("killed")
    monkeypatch.setattr(torch, "save", dies_half_way)
    with pytest.raises(KeyboardInterrupt):
        a.save_model(20)
    monkeypatch.setattr(torch, "save", real)
    assert not os.path.exists(os.path.join(str(tmp_path), "model_0000020.pth"))
    assert a.ckpt_s.get_checkpoint_file() == first
    assert sorted(os.listdir(str(tmp_path))) == ["last_checkpoint", os.path.basename(first)]
    assert a.resume() == 7                                          # ... and it still loads


def test_the_file_is_still_a_reference_checkpoint(saved):
    from maskrcnn_benchmark.utils.checkpoint import Checkpointer
    a, path = saved
    m = _Tiny(9)
    extra = Checkpointer(m).load(path, test=True)
    assert {"optimizer", "scheduler", "iteration", "trainer"} == set(extra) and extra["iteration"] == 7
    assert all(torch.equal(v, a.student.state_dict()[k]) for k, v in m.state_dict().items())
    assert set(extra["optimizer"]) >= {"momentum_buffers", "steps", "lr_factor"} and "last_epoch" in extra["scheduler"]


class _Seeking(list):
    def fast_forward(self, n):
        self.skipped = n
        del self[:n]


def test_unlabeled_loader_is_fast_forwarded_once(tmp_path):
    loader = [("u%d" % i, None) for i in range(5)]
    a = _trainer(tmp_path, unlabeled=list(loader))
    assert [a._next_unlabeled() for _ in range(7)] == ["u0", "u1", "u2", "u3", "u4", "u0", "u1"] and a.unlabeled_seen == 7
    a.last_iteration = 3
    a.save_model(3)
    b = _trainer(tmp_path, seed=2, unlabeled=list(loader))
    b.resume()
    assert b.unlabeled_seen == 7
    assert [b._next_unlabeled() for _ in range(4)] == ["u2", "u3", "u4", "u0"] and b.unlabeled_seen == 11   # 7 % 5 passed over, once
    c = _trainer(tmp_path, seed=3, unlabeled=_Seeking(loader))
    c.resume()
    assert [c._next_unlabeled() for _ in range(2)] == ["u2", "u3"] and c.dataloader_u.skipped == 2


def test_teacher_file_tagged_last_in_a_shared_directory(saved, tmp_path):
    """past START_MT `save_model` writes t_<name>.pth second, so `last_checkpoint` names it: `resume()` takes the student's file"""
    from maskrcnn_benchmark.utils.checkpoint import Checkpointer
    a, path = saved
    a.ckpt_t = Checkpointer(a.teacher, save_dir=str(tmp_path), save_to_disk=True)
    a.last_iteration = a.start_mt + 5
    a.save_model(a.last_iteration)
    assert os.path.basename(a.ckpt_s.get_checkpoint_file()) == "t_model_%07d.pth" % (a.start_mt + 5)
    assert a.resume() == a.start_mt + 5
