"""MT.AUG_S > 1: mirrored student views in the mean-teacher step (reference generalized_rcnn.py:201-215, 243-282; box_head.py:80;
box_head/loss.py:185-237; engine/MTtrainer.py:255).

  * the MGD kernel over S student views (csrc/losses.hip: mmt_mgd_views_*) through fg_hint_loss against the oracle in fp64: value and
    every student's gradient;
  * one whole mean-teacher step with AUG_K = 2, AUG_S = 2 at 160 x 160 against an oracle step that feeds the last two views to its
    forward_student, only the random draws replayed;
  * AUG_S = 1 never reaches the new entry points;
  * HARD_NEG False: one random negative subset per student view;
  * the full 1000 x 1000 crops at the bench's batch with AUG_S = 2."""
import math
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

import test_train_step_gpu as tts   # noqa: E402  (the existing step's helpers and its bars: _load, _check_step, ...)

DEV = torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------ 1. MGD over views
LEVELS = [(9, 8), (5, 7), (3, 4), (2, 1), (1, 1)]   # even and odd widths, W = 1; the 1 x 1 level's pooled mask is empty


def _seg(n, ih, iw, g):
    """a rectangle of ones over ~1/3 of each image plus sparse noise: the coarse 1 x 1 level pools to an empty mask"""
    seg = (torch.rand((n, ih, iw), generator=g) < 0.1).to(torch.int32)
    seg[:, :ih // 2 + 2, :(iw * 3) // 5] = 1
    return seg


@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("nt", [2, 4])
@pytest.mark.parametrize("S", [2, 3])
def test_mgd_views_match_oracle(S, nt, C):
    from oracle import model as om
    from maskrcnn_benchmark.modeling.detector.generalized_rcnn import fg_hint_loss
    g = torch.Generator().manual_seed(100 * S + 10 * nt + C)
    N = 2
    teachers = [[torch.randn((N, C, h, w), generator=g) for (h, w) in LEVELS] for _ in range(nt)]
    students = [[torch.randn((N, C, h, w), generator=g) for (h, w) in LEVELS] for _ in range(S)]
    seg = _seg(N, 36, 32, g)
    masks = [seg[i] for i in range(N)]
    # the empty level is really empty, the others are not
    pooled = [torch.nn.functional.adaptive_avg_pool2d(seg[:, None].float(), hw) > 0.5 for hw in LEVELS]
    assert not bool(pooled[-1].any()) and all(bool(p.any()) for p in pooled[:-1])

    ts_d = [[t.double() for t in v] for v in teachers]
    ss_d = [[s.double().requires_grad_(True) for s in v] for v in students]
    ref = om.fg_hint_loss(ts_d, ss_d, masks)
    ref.backward()

    ts_g = [[t.to(DEV).contiguous(memory_format=torch.channels_last) for t in v] for v in teachers]
    ss_g = [[s.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True) for s in v] for v in students]
    out = fg_hint_loss(ts_g, ss_g, [m.to(DEV) for m in masks])
    out.backward()
    torch.cuda.synchronize()
    assert float(out.detach()) == pytest.approx(float(ref.detach()), rel=1e-5)
    for j in range(S):
        for l in range(len(LEVELS)):
            gr, gp = ss_d[j][l].grad, ss_g[j][l].grad.double().cpu()
            scale = gr.abs().max().item()
            if l == len(LEVELS) - 1:
                assert scale == 0.0 and gp.abs().max().item() == 0.0, (j, l)   # empty mask: no gradient
                continue
            assert (gp - gr).abs().max().item() <= 1e-5 * scale, (S, nt, C, j, l)


def test_mgd_views_beyond_the_register_budget_is_refused():
    from maskrcnn_benchmark import _hip as H
    from maskrcnn_benchmark.modeling.detector.generalized_rcnn import fg_hint_loss
    mk = lambda: torch.randn((1, 8, 2, 3), device=DEV).contiguous(memory_format=torch.channels_last)   # noqa: E731
    masks = [torch.ones((4, 4), dtype=torch.int32, device=DEV)]
    with pytest.raises(NotImplementedError, match="AUG_S = 5"):
        fg_hint_loss([[mk()] for _ in range(2)], [[mk()] for _ in range(5)], masks)
    with pytest.raises(NotImplementedError, match="AUG_S = 3 with 8 teacher views"):
        fg_hint_loss([[mk()] for _ in range(8)], [[mk()] for _ in range(3)], masks)
    m = torch.ones((1, 2, 3), device=DEV)
    with pytest.raises(RuntimeError, match="register budget"):
        H.mgd_views_forward([mk() for _ in range(3)], [False, True, False], [mk() for _ in range(8)], [False] * 8, m)


# ------------------------------------------------------------------------------------------------ 2. whole step, AUG_S = 2
@pytest.fixture(scope="module")
def small():
    return tts._bench().build(DEV, 0, crop=160, n_inst=4)


def _views(cfg, unl):
    from maskrcnn_benchmark.structures.image_list import to_image_list
    return [to_image_list(list(u.to(DEV)), cfg.DATALOADER.SIZE_DIVISIBILITY) for u in unl]


def _set_aug_s(cfg, trainer, s):
    cfg.MT.AUG_S = s
    trainer.student_bs = s


def _oracle_trainer_s(state_shapes, weights, aug_s):
    """oracle.model.Trainer.step with the last `aug_s` unlabeled views going to forward_student (the oracle itself is fixed to one)"""
    from oracle import model as om

    class TrainerS(om.Trainer):
        def step(self, iteration, images, targets, unlabeled=None, seeds=(None, None, None)):
            cfg = self.cfg
            taps_a, taps_b, taps_c = {}, {}, {}
            torch.manual_seed(seeds[0])
            loss = om.forward_supervised(self.s, cfg, images, targets, taps_a)
            assert iteration > cfg.mt_start and cfg.mt_lambda > 0
            torch.manual_seed(seeds[1])
            k = len(unlabeled) - aug_s
            tr = om.forward_teacher(self.t, cfg, unlabeled[:k], taps_b)
            torch.manual_seed(seeds[2])
            loss.update(om.forward_student(self.s, cfg, unlabeled[-aug_s:], tr, taps_c))
            self.last_epoch += 1
            f = om.lr_factor(self.last_epoch)
            for g in self.opt.param_groups:
                g["lr"] = g["initial_lr"] * f
            wl = om.weight_sum_losses(cfg, loss, iteration, self.max_iter)
            self.opt.zero_grad()
            sum(wl.values()).backward()
            self.opt.step()
            alpha = om.ema_alpha(cfg, iteration - (cfg.mt_start - 10))
            with torch.no_grad():
                om.ema_update([self.t[k_] for k_ in self.param_order], [self.s[k_].detach() for k_ in self.param_order], alpha)
            return {k_: v.detach() for k_, v in wl.items()}, (taps_a, taps_b, taps_c)

    return om, TrainerS(weights, om.default_cfg(), state_shapes["trainable"], state_shapes["param_order"])


def test_full_step_aug_s2_matches_oracle(small, synth, state_shapes, weights):
    from maskrcnn_benchmark.utils.replay import Replay
    from maskrcnn_benchmark import _hip as H
    cfg, trainer, batch = small
    iteration = 1400
    tts._load(trainer, weights)
    snap = tts._snapshot(trainer)
    H.rb_reset()
    om, ot = _oracle_trainer_s(state_shapes, weights, 2)
    imgs, tgs = synth.make_labeled(2, 160, 4, seed=1234)
    unl = synth.make_unlabeled(2, 160, 4, seed=4321)
    ot.last_epoch = trainer.scheduler.last_epoch
    ref_losses, (ta, tb, tc) = ot.step(iteration, imgs, tts._oracle_targets(om, tgs), unl, seeds=(99, 100, 101))
    assert len(tc["dropout"]) == 2   # one dropout draw per student view in the oracle
    before_s = {n: tts._param(trainer.flat_s, trainer.student, n) for n in state_shapes["param_order"]}
    before_t = {n: tts._param(trainer.flat_t, trainer.teacher, n) for n in state_shapes["param_order"]}
    stu = {"rpn_sampler": ta["rpn_sampler"], "roi_sampler": ta["roi_sampler"], "rpn_proposals": ta["rpn_proposals"],
           "dropout": list(ta["dropout"]) + list(tc["dropout"])}
    _set_aug_s(cfg, trainer, 2)
    trainer.student.set_replay(Replay(stu))
    trainer.teacher.set_replay(Replay(tb))
    trainer.student.taps, trainer.teacher.taps = {}, {}
    try:
        il, tg, _ = batch()
        losses = trainer.train_step(iteration, il, tg, _views(cfg, unl))
        torch.cuda.synchronize()
        left = trainer.student._replay.d.get("dropout")
    finally:
        _set_aug_s(cfg, trainer, 1)
        trainer.student.set_replay(None)
        trainer.teacher.set_replay(None)
        trainer.student.taps = trainer.teacher.taps = None
    assert not left   # every recorded dropout mask (supervised + both student views) was consumed
    try:
        dev = {k: abs(float(losses[k]) - float(ref_losses[k])) / abs(float(ref_losses[k])) for k in ("mt_fg_loss", "mt_classifier")}
        print("AUG_S=2 relative deviation from the oracle: mt_fg_loss %.3e  mt_classifier %.3e" % (dev["mt_fg_loss"],
                                                                                                  dev["mt_classifier"]))
        tts._check_step(cfg, trainer, ot, state_shapes, weights, losses, ref_losses, before_s, before_t, iteration)
        assert dev["mt_fg_loss"] < 1e-4 and dev["mt_classifier"] < 1e-4, dev
    finally:
        tts._restore(trainer, snap)
        H.rb_reset()


# ------------------------------------------------------------------------------------------------ 3. AUG_S = 1 is untouched
def test_aug_s1_never_calls_the_view_kernels(small, weights, monkeypatch):
    from maskrcnn_benchmark import _hip as H
    cfg, trainer, batch = small
    assert trainer.student_bs == 1 and cfg.MT.AUG_S == 1
    tts._load(trainer, weights)
    snap = tts._snapshot(trainer)
    calls = {"views": 0, "level": 0}

    def refuse(*a, **k):
        calls["views"] += 1
        raise AssertionError("AUG_S = 1 reached mmt_mgd_views_*")

    orig_level = H.mgd_level_forward

    def level(*a, **k):
        calls["level"] += 1
        return orig_level(*a, **k)

    monkeypatch.setattr(H, "mgd_views_forward", refuse)
    monkeypatch.setattr(H, "mgd_views_backward", refuse)
    monkeypatch.setattr(H, "mgd_level_forward", level)
    try:
        il, tg, ul = batch()
        assert len(ul) == 3
        losses = trainer.train_step(1400, il, tg, ul)
        torch.cuda.synchronize()
    finally:
        tts._restore(trainer, snap)
    assert calls["views"] == 0
    assert calls["level"] == 5   # today's per-level path, once per pyramid level
    assert "mt_fg_loss" in losses and "mt_classifier" in losses
    assert all(math.isfinite(float(v)) for v in losses.values())


# ------------------------------------------------------------------------------------------------ 4. HARD_NEG False, S = 2
def test_random_negatives_are_drawn_per_view(monkeypatch):
    from maskrcnn_benchmark.config import make_default_cfg
    from maskrcnn_benchmark.layers import fused
    from maskrcnn_benchmark.modeling.roi_heads.box_head.box_head import make_roi_box_loss_evaluator
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    cfg = make_default_cfg()
    cfg.merge_from_list(["MT.HARD_NEG", False])
    ev = make_roi_box_loss_evaluator(cfg)
    ev.fg_bg_sampler.generator = torch.Generator(device=DEV).manual_seed(7)
    g = torch.Generator().manual_seed(3)
    labels = torch.zeros(512, dtype=torch.int64)
    labels[torch.randperm(512, generator=g)[:60]] = torch.randint(1, 3, (60,), generator=g)
    labels[-12:] = -1                                     # padding rows of a fixed-capacity list: never kept
    labels = labels.to(DEV)
    props = []
    for half in labels.split(256):
        b = BoxList(torch.rand((256, 4), device=DEV) * 100, (160, 160), "xyxy")
        b.add_field("labels", half)
        props.append(b)
    nc = cfg.MODEL.ROI_BOX_HEAD.NUM_CLASSES
    teacher = [torch.randn((512, nc), device=DEV) for _ in range(4)]
    rows = []
    orig = fused.PSMLossFn.apply

    def spy(cl, t, roww, *a):
        rows.append(roww.clone())
        return orig(cl, t, roww, *a)

    monkeypatch.setattr(fused.PSMLossFn, "apply", spy)
    student = [torch.randn((512, nc), device=DEV) for _ in range(2)]
    loss = ev.evaluatePSM(student, teacher, props)
    torch.cuda.synchronize()
    assert math.isfinite(float(loss)) and len(rows) == 2
    pos, neg = labels > 0, labels == 0
    n_keep = min(int(neg.sum()), int(pos.sum()) // 2)
    kept = []
    for r in rows:
        assert torch.equal(r[pos], torch.ones_like(r[pos]))
        k = (r > 0) & ~pos
        assert int(k.sum()) == n_keep
        assert bool(neg[k].all())            # only negatives are kept
        kept.append(k)
    assert not torch.equal(kept[0], kept[1])  # two independent draws
    # S = 1 keeps its single draw
    rows.clear()
    ev.evaluatePSM(student[:1], teacher, props)
    assert len(rows) == 1 and rows[0].dim() == 1 and int(((rows[0] > 0) & ~pos).sum()) == n_keep


# ------------------------------------------------------------------------------------------------ 5. full size
def test_fullsize_aug_s2_steps(synth):
    bench = tts._bench()
    cfg, trainer, batch = bench.build(DEV, 0, base_lr=1e-4)   # (the bench's own LR is 0: nothing would move)
    _set_aug_s(cfg, trainer, 2)
    unl = synth.make_unlabeled(bench.N_UNLAB, bench.CROP, cfg.MT.AUG_K + 2, seed=4321)
    it0 = cfg.MT.START_MT + 400
    for i in range(3):
        before = trainer.flat_s.data.clone()
        il, tg, _ = batch()
        losses = trainer.train_step(it0 + i, il, tg, _views(cfg, unl))
        torch.cuda.synchronize()
        assert "mt_fg_loss" in losses and "mt_classifier" in losses
        assert all(math.isfinite(float(v)) for v in losses.values()), losses
        assert float(losses["mt_fg_loss"]) > 0 and float(losses["mt_classifier"]) > 0
        assert not torch.equal(before, trainer.flat_s.data)
    assert trainer.skipped_pairs == 0
