"""MODEL.BACKBONE.FREEZE_CONV_BODY_AT 0 and 1 on the GPU: the stem (layers/fused.py::StemFn on csrc/stem_bwd.hip) and layer1 train.

  * the backbone against the reference's own CPU backbone at FREEZE_CONV_BODY_AT 0, recorded by tests/golden/gen_golden_freeze.py:
    gradient samples of the stem, layer1 and layer2.0.conv1 within 1e-4 * max |reference tensor| (the model-tap bar of
    tests/test_resnext_model_gpu.py); at 1 the stem has no gradient and layer1's are the same; at 2 neither has one and the two new
    bindings are never called;
  * forward_pair at 0 against two separate passes;
  * one whole iteration against the oracle (oracle/model.py::Trainer with the extended trainable set) with the quantities and
    tolerances of tests/test_train_step_gpu.py::_check_step -- on the parent of this feature the stem's update is zero and the
    oracle's is not;
  * nothing derived from the stem filter goes stale under the raw-pointer updates of SGD and the EMA (space-to-depth filter, its
    packed planes, a recorded launch plan of the teacher's backbone);
  * bf16 activation storage refuses a trainable stem."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT, load_synth

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

BAR = 1e-4
STEM = "body.stem.conv1.weight"


def _cfg(freeze_at):
    from maskrcnn_benchmark.config import make_default_cfg
    cfg = make_default_cfg()
    cfg.merge_from_list(["MODEL.BACKBONE.FREEZE_CONV_BODY_AT", freeze_at])
    return cfg


def _backbone(weights, freeze_at):
    from maskrcnn_benchmark import _hip as H
    from maskrcnn_benchmark.modeling.backbone.backbone import build_backbone
    H.lib()
    bb = build_backbone(_cfg(freeze_at))
    missing, unexpected = bb.load_state_dict({k[len("backbone."):]: v for k, v in weights.items() if k.startswith("backbone.")},
                                             strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return bb.cuda().train()


def _images():
    from maskrcnn_benchmark.structures.image_list import to_image_list
    imgs, _ = load_synth().make_labeled(2, 160, 4, seed=1234)
    return to_image_list(list(imgs), 32).tensors.cuda()


def _nchw(t):
    return t.detach().float().cpu().contiguous().reshape(-1)


def _level_loss(pyr):
    import grouped_formulations as gf
    return sum((p * gf.level_weights(l, p.shape).to(p.device)).sum() for l, p in enumerate(pyr))


class _Counter(object):
    """counts the calls of the two new bindings (the nodes reach them through the module's attributes)"""

    def __init__(self, H):
        self.H, self.n = H, 0
        self.keep = (H.maxpool3x3s2_backward, H.stem_wgrad)

    def __enter__(self):
        def wrap(f):
            def w(*a, **k):
                self.n += 1
                return f(*a, **k)
            return w
        self.H.maxpool3x3s2_backward, self.H.stem_wgrad = wrap(self.keep[0]), wrap(self.keep[1])
        return self

    def __exit__(self, *a):
        self.H.maxpool3x3s2_backward, self.H.stem_wgrad = self.keep


@pytest.mark.parametrize("freeze_at", [0, 1, 2])
def test_backbone_gradients_match_the_reference_backbone(weights, freeze_at):
    from maskrcnn_benchmark import _hip as H
    from maskrcnn_benchmark.layers import fused
    fx = np.load(os.path.join(GOLD, "freeze0_160.npz"))
    names = sorted(k[2:-4] for k in fx.files if k.startswith("g:") and k.endswith(":val"))
    assert len(names) == 7 and STEM in names and sum(".layer1." in n for n in names) == 5
    bb = _backbone(weights, freeze_at)
    with _Counter(H) as calls:
        _level_loss(bb(_images())).backward()
        fused.join_wgrads()
    params = dict(bb.named_parameters())
    assert calls.n == (2 if freeze_at == 0 else 0)
    for n in names:
        g = params[n].grad
        if (n == STEM and freeze_at >= 1) or (".layer1." in n and freeze_at >= 2):
            assert g is None and not params[n].requires_grad, n
            continue
        assert g is not None and list(g.shape) == list(fx["g:%s:shape" % n]), n
        got, ref = _nchw(g)[torch.from_numpy(fx["g:%s:idx" % n])], torch.from_numpy(fx["g:%s:val" % n])
        dev = (got.double() - ref.double()).abs().max().item() / float(fx["g:%s:max" % n])
        print("freeze_at %d  d %-44s worst |got - ref| / max |ref| = %.3e" % (freeze_at, n, dev))
        assert dev <= BAR, (n, dev)
    for n, p in params.items():
        if (".stem." in n and freeze_at >= 1) or (".layer1." in n and freeze_at >= 2):
            assert p.grad is None, n


def test_forward_pair_at_0(weights):
    """one N = 4 forward, a StemFn node per half.  Both arms run with MMT_SPLITK=0 / MMT_STRIP=0, where every convolution is
    bit-identical whatever batch its image sits in (tests/test_train_step_gpu.py): the pyramids are then those of two separate
    passes bit for bit; the weight gradients differ by the order of the atomics."""
    from maskrcnn_benchmark.layers import fused
    from maskrcnn_benchmark.modeling.backbone.backbone import forward_pair
    bb = _backbone(weights, 0)
    g = torch.Generator().manual_seed(3)
    xa = (torch.randn((2, 3, 160, 160), generator=g) * 50.0).cuda()
    xb = (torch.randn((2, 3, 160, 160), generator=g) * 50.0).cuda()
    watch = {n: p for n, p in bb.named_parameters() if n in (STEM, "body.layer1.0.conv1.weight")}
    assert len(watch) == 2
    old = {k: os.environ.get(k) for k in ("MMT_SPLITK", "MMT_STRIP")}
    try:
        os.environ["MMT_SPLITK"] = "0"
        os.environ["MMT_STRIP"] = "0"
        pa, pb = forward_pair(bb, xa, xb)
        sa, sb = bb(xa), bb(xb)
        assert len(pa) == len(pb) == len(sa) == 5
        for a, b, c, d in zip(pa, pb, sa, sb):
            assert torch.equal(a.detach(), c.detach()) and torch.equal(b.detach(), d.detach())
        assert all(t.requires_grad for t in pa + pb)
        _level_loss(pa).backward()
        _level_loss(pb).backward()
        fused.join_wgrads()
        got = {n: p.grad.detach().clone() for n, p in watch.items()}
        for p in bb.parameters():
            p.grad = None
        _level_loss(sa).backward()
        _level_loss(sb).backward()
        fused.join_wgrads()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for n, p in watch.items():
        assert p.grad.abs().max().item() > 0
        dev = (got[n].double() - p.grad.double()).abs().max().item() / p.grad.abs().max().item()
        print("forward_pair at 0, both halves vs separate passes: d %-30s worst %.3e" % (n, dev))
        assert dev <= 1e-5, (n, dev)


_TRAINERS = {}


def _trainer(freeze_at):
    """bench.py::build's trainer at 160 x 160 with the key merged into its configuration (one per value and module run)"""
    if freeze_at not in _TRAINERS:
        import bench
        import maskrcnn_benchmark.config as C
        keep = C.make_default_cfg
        try:
            def with_key():
                cfg = keep()
                cfg.merge_from_list(["MODEL.BACKBONE.FREEZE_CONV_BODY_AT", freeze_at])
                return cfg
            C.make_default_cfg = with_key
            _TRAINERS[freeze_at] = bench.build(torch.device("cuda", 0), 0, crop=160, n_inst=4)
        finally:
            C.make_default_cfg = keep
        assert _TRAINERS[freeze_at][0].MODEL.BACKBONE.FREEZE_CONV_BODY_AT == freeze_at
    return _TRAINERS[freeze_at]


def _extended(state_shapes, model):
    """a copy of the fixture's lists with the names the key's requires_grad rule adds to `trainable`"""
    added = [n for n, p in model.named_parameters() if p.requires_grad and n not in state_shapes["trainable"]]
    out = dict(state_shapes)
    have = set(state_shapes["trainable"]) | set(added)
    out["trainable"] = [n for n in state_shapes["param_order"] if n in have]
    return out, added


@pytest.mark.parametrize("iteration", [1400, 5], ids=["mean-teacher-step", "before-START_MT"])
@pytest.mark.parametrize("freeze_at", [0, 1])
def test_full_step_matches_oracle(synth, state_shapes, weights, freeze_at, iteration):
    import test_train_step_gpu as ts
    from maskrcnn_benchmark.utils.replay import Replay
    from maskrcnn_benchmark import _hip as H
    cfg, trainer, batch = _trainer(freeze_at)
    shapes, added = _extended(state_shapes, trainer.student)
    assert len(added) == (11 if freeze_at == 0 else 10) and (("backbone." + STEM) in added) == (freeze_at == 0)
    ts._load(trainer, weights)
    snap = ts._snapshot(trainer)
    H.rb_reset()
    om, ot = ts._oracle_trainer(synth, shapes, weights)
    imgs, tgs = synth.make_labeled(2, 160, 4, seed=1234)
    unl = synth.make_unlabeled(2, 160, 3, seed=4321)
    ot.last_epoch = trainer.scheduler.last_epoch
    ref_losses, (ta, tb, tc) = ot.step(iteration, imgs, ts._oracle_targets(om, tgs), unl, seeds=(99, 100, 101))
    before_s = {n: ts._param(trainer.flat_s, trainer.student, n) for n in shapes["param_order"]}
    before_t = {n: ts._param(trainer.flat_t, trainer.teacher, n) for n in shapes["param_order"]}
    # random draws only; the proposal list rides along for Replay.align (order of near-tied scores), never as values
    stu = {"rpn_sampler": ta["rpn_sampler"], "roi_sampler": ta["roi_sampler"], "rpn_proposals": ta["rpn_proposals"],
           "dropout": list(ta["dropout"]) + list(tc.get("dropout", []))}
    trainer.student.set_replay(Replay(stu))
    trainer.teacher.set_replay(Replay(tb))
    trainer.student.taps, trainer.teacher.taps = {}, {}
    try:
        il, tg, ul = batch()
        losses = trainer.train_step(iteration, il, tg, ul)
        torch.cuda.synchronize()
    finally:
        trainer.student.set_replay(None)
        trainer.teacher.set_replay(None)
        trainer.student.taps = trainer.teacher.taps = None
    try:
        for n in added:   # the oracle moved what the key unfroze (so the comparison below is not one of zeros)
            assert (ot.s[n].detach() - weights[n]).abs().max().item() > 0, n
        ts._check_step(cfg, trainer, ot, shapes, weights, losses, ref_losses, before_s, before_t, iteration)
    finally:
        ts._restore(trainer, snap)
        H.rb_reset()


def _fresh_stem(cfg, model):
    from maskrcnn_benchmark.modeling.backbone.backbone import StemWithFixedBatchNorm
    m = StemWithFixedBatchNorm(cfg)
    m.load_state_dict({k: v.detach().clone() for k, v in model.backbone.body.stem.state_dict().items()})
    return m.cuda()


def test_no_stale_stem_after_a_step(weights):
    import test_train_step_gpu as ts
    from maskrcnn_benchmark import _hip as H
    cfg, trainer, batch = _trainer(0)
    ts._load(trainer, weights)
    snap = ts._snapshot(trainer)
    student, teacher = trainer.student, trainer.teacher
    g = torch.Generator().manual_seed(8)
    xs = [(torch.randn(s, generator=g) * 50.0).cuda() for s in ((2, 3, 160, 160), (1, 3, 150, 154))]
    xv = (torch.randn((8, 3, 160, 160), generator=g) * 50.0).cuda()
    keep = H.LAUNCH_PLANS
    try:
        # two un-compared steps first: the producing sites get their plane scales, which is part of a plan's key -- every step of a
        # run but its first two is in this state (weights, momentum and schedule restored afterwards)
        for it in (1400, 1401):
            il, tg, ul = batch()
            trainer.train_step(it, il, tg, ul)
        torch.cuda.synchronize()
        ts._restore(trainer, snap)
        with torch.no_grad():   # everything derived from the filters exists before the step: caches, and a recorded plan
            for x in xs:
                student.backbone.body.stem(x)
                teacher.backbone.body.stem(x)
            H.LAUNCH_PLANS = True
            old = [tuple(t.clone() for t in teacher.run_backbone(xv)) for _ in range(3)]   # run, record, replay
            for a, b in zip(old[0], old[2]):
                assert torch.equal(a, b)
        w_s = student.backbone.body.stem.conv1.weight.detach().clone()
        w_t = teacher.backbone.body.stem.conv1.weight.detach().clone()
        il, tg, ul = batch()
        trainer.train_step(1400, il, tg, ul)
        torch.cuda.synchronize()
        assert (student.backbone.body.stem.conv1.weight != w_s).any().item(), "SGD did not move the stem"
        assert (teacher.backbone.body.stem.conv1.weight != w_t).any().item(), "the EMA did not move the teacher's stem"
        for model in (student, teacher):
            fresh = _fresh_stem(cfg, model)
            for x in xs:
                with torch.no_grad():
                    want = fresh(x)
                    assert torch.equal(model.backbone.body.stem(x), want), tuple(x.shape)
        for x in xs:   # the student's recording pass (the un-fused launches of the StemFn node) reads the same filter
            out = student.backbone.body.stem(x)
            assert out.requires_grad
            with torch.no_grad():
                assert torch.equal(out.detach(), _fresh_stem(cfg, student)(x)), tuple(x.shape)
        with torch.no_grad():
            H.LAUNCH_PLANS = True
            planned = tuple(t.clone() for t in teacher.run_backbone(xv))     # the recorded plan, replayed on the new weights
            H.LAUNCH_PLANS = False
            plain = tuple(t.clone() for t in teacher.run_backbone(xv))
        assert any(p.seen >= 4 and not p.dead and p.calls for p in H._LAUNCH_PLANS.values())   # (it was a replay)
        for a, b in zip(planned, plain):
            assert torch.equal(a, b), (a - b).abs().max().item()
        assert any(not torch.equal(a, c) for a, c in zip(planned, old[0]))    # (the teacher did change)
    finally:
        H.LAUNCH_PLANS = keep
        ts._restore(trainer, snap)
        H.rb_reset()


def test_trainable_stem_not_offered_with_bf16_storage(weights):
    from maskrcnn_benchmark import _hip as H
    bb = _backbone(weights, 0)
    prev = H.get_conv_precision()
    H.set_conv_precision(1)
    H.set_bf16_storage(True)
    try:
        with pytest.raises(NotImplementedError, match="FREEZE_CONV_BODY_AT"):
            bb(_images())
    finally:
        H.set_bf16_storage(False)
        H.set_conv_precision(prev)
