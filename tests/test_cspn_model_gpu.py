"""The CSPN mask head on the MI355X (reference configs/pap/CSPN.yaml; modeling/roi_heads/mask_head/mask_head.py: PRCNNFeatureExtractor,
PRCNNPredictor): against the reference's own outputs (tests/golden/cspn160.npz), against the plain-torch restatement for the
gradients the reference cannot give (tests/cspn_formulation.py, itself pinned to the reference by tests/test_cspn_config.py), in
evaluation mode, and through one mean-teacher step.  160 x 160 crops, in the default arithmetic and on the fp32-input MFMA."""
import collections
import json
import os

import pytest
import torch

import cspn_formulation as cf
from conftest import GOLD, T, gold

pytestmark = pytest.mark.gpu

SIZE = 160
FE = "mask_heads.mask.feature_extractor."


@pytest.fixture(scope="module")
def cspn_weights(synth):
    with open(os.path.join(GOLD, "state_shapes_cspn.json")) as f:
        return synth.make_weights(json.load(f)["shapes"], seed=0)


@pytest.fixture(scope="module")
def data(synth):
    imgs, tgs = synth.make_labeled(2, SIZE, 4, seed=1234)
    boxes = cf.fixture_boxes(tgs, SIZE)
    return imgs, tgs, boxes, cf.matched_labels(boxes, tgs)


def _training_yardstick(cspn_weights, data, choices=None):
    """loss and gradients of the training path (positives only) by the restatement in double"""
    imgs, tgs, boxes, labels = data
    sd = {k: v.double().requires_grad_(True) for k, v in cspn_weights.items() if k.startswith(cf.PRE + "feature_extractor.")
          or k.startswith(cf.PRE + "predictor.")}
    pos = [b[l > 0] for b, l in zip(boxes, labels)]
    _, _, lp = cf.head(sd, imgs.double(), [b.double() for b in pos], choices=choices)
    loss = cf.mask_loss(lp, pos, tgs)
    loss.backward()
    return {"loss": loss.item(), "grads": {k: v.grad for k, v in sd.items()}}


@pytest.fixture(scope="module")
def yardstick(cspn_weights, data):
    """the restatement in double on the fixture's inputs, computed once: logits of all boxes, its own pool choices, and loss /
    gradients of the training path"""
    imgs, tgs, boxes, labels = data
    sd = {k: v.double() for k, v in cspn_weights.items() if k.startswith(cf.PRE)}
    with torch.no_grad():
        _, _, logits = cf.head(sd, imgs.double(), [b.double() for b in boxes])
        choices = cf.pool_choices(cf.maps(sd, imgs.double()))
    out = _training_yardstick(cspn_weights, data)
    out.update(logits=logits, choices=choices)
    return out


@pytest.fixture(scope="module", params=[3, 0], ids=["default-f16x2-split", "fp32-mfma"])
def setup(request, cspn_weights):
    from maskrcnn_benchmark import _hip
    from maskrcnn_benchmark.config import make_default_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    _hip.lib()
    prev = _hip.get_conv_precision()
    _hip.set_conv_precision(request.param)
    request.addfinalizer(lambda: _hip.set_conv_precision(prev))
    cfg = cf.apply_keys(make_default_cfg())
    model = build_detection_model(cfg, is_student=True).cuda()
    missing, unexpected = model.load_state_dict(cspn_weights, strict=False)
    assert all("cell_anchors" in k for k in missing) and not unexpected, (missing, unexpected)
    return cfg, model


def _targets(tgs):
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask
    out = []
    for t in tgs:
        b = BoxList(t["boxes"].cuda(), t["size"], "xyxy")
        b.add_field("labels", t["labels"].cuda())
        b.add_field("masks", SegmentationMask([[p for p in inst] for inst in t["polys"]], t["size"], mode="poly"))
        out.append(b)
    return out


def _proposals(boxes, labels, tgs):
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    out = []
    for b, l, t in zip(boxes, labels, tgs):
        p = BoxList(b.cuda(), t["size"], "xyxy")
        p.add_field("labels", l.cuda())
        out.append(p)
    return out


def _images(imgs):
    from maskrcnn_benchmark.structures.image_list import to_image_list
    return to_image_list(list(imgs.cuda()), 32)


def _rel(a, b, scale):
    return (a - b).abs().max().item() / scale


def test_head_on_the_fixture_inputs(setup, data):
    """pooled samples and logits within 1e-4 of the tensor's maximum, loss_seg within 1e-4 relative -- against the reference's own
    numbers"""
    _, model = setup
    imgs, tgs, boxes, labels = data
    g = gold("cspn160")
    head = model.mask_heads.mask
    fe = head.feature_extractor
    seen = {}
    hook = fe.posconv1.register_forward_pre_hook(lambda m, a: seen.update(pooled=a[0].detach()))
    model.train()
    with torch.no_grad():
        x, _ = fe(_images(imgs).tensors, _proposals(boxes, labels, tgs))
        logits = head.predictor(x)
    hook.remove()
    for name, t in (("pooled", seen["pooled"]), ("logits", logits)):
        assert list(t.shape) == g[name + "_shape"].tolist()
        got = t.contiguous().reshape(-1)[T(g[name + "_idx"]).cuda()].cpu().double()
        err = _rel(got, T(g[name + "_val"]), float(g[name + "_max"]))
        print(name, "error / max", err)
        assert err < 1e-4, (name, err)
    pos = torch.cat(labels) > 0
    assert torch.equal(torch.cat(labels), T(g["labels"]))
    props = [p[(l > 0).nonzero().squeeze(1).cuda()] for p, l in zip(_proposals(boxes, labels, tgs), labels)]
    loss = head.loss_evaluator(props, logits[pos.cuda()].contiguous(memory_format=torch.channels_last), _targets(tgs)).item()
    print("loss_seg", loss, float(g["loss_seg"]))
    assert loss == pytest.approx(float(g["loss_seg"]), rel=1e-4)


def test_gradients_against_the_formulation(setup, data, yardstick, cspn_weights):
    """the training path -- the head keeps the positives, pools them, loss at 25 x 25 --: loss within 1e-4, the gradient of every
    PRCNN parameter within 2e-3 of the tensor's maximum (the gradient bar of tests/test_model_gpu.py).
    The one discrete decision of the head is replayed, as tests/test_model_gpu.py replays such decisions: where a max-pool window
    holds two candidates that are neighbours in fp32, the yardstick takes the element the device took (cspn_formulation._pool
    refuses anything that is not such a tie).  On this data the fp32-input arithmetic meets one: channel 111 of conv6's output,
    149.843424 against 149.843438, 2e-8 of the map's maximum apart; un-replayed it moves conv6's weight gradient in that channel
    by 5e-4 of its maximum and conv1's by 3.4e-3."""
    _, model = setup
    imgs, tgs, boxes, labels = data
    head = model.mask_heads.mask
    fe = head.feature_extractor
    model.train()
    for p in model.parameters():
        p.grad = None
    pooled_from, hooks = {}, []
    for i, name in enumerate(("conv2", "conv4", "conv6")):
        hooks.append(getattr(fe, name).register_forward_hook(lambda m, a, out, i=i: pooled_from.__setitem__(i, out.detach())))
    _, _, losses = head(None, _proposals(boxes, labels, tgs), _targets(tgs), _images(imgs))
    for h in hooks:
        h.remove()
    choices = cf.pool_choices([pooled_from[i].cpu().double().contiguous() for i in range(3)])
    ties = sum(int((c != y).sum()) for c, y in zip(choices, yardstick["choices"]))
    print("pool windows decided the other way than in double:", ties)
    assert ties <= 4
    want = yardstick if ties == 0 else _training_yardstick(cspn_weights, data, choices)
    assert losses["loss_seg"].item() == pytest.approx(want["loss"], rel=1e-4)
    losses["loss_seg"].backward()
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    errs = {}
    for n in cf.PRCNN_NAMES:
        for leaf in ("weight", "bias"):
            k = cf.PRE + n + "." + leaf
            ref = want["grads"][k]
            errs[k] = _rel(named[k].grad.detach().cpu().double(), ref, ref.abs().max().item() + 1e-12)
            print(k, "gradient error / max", errs[k])
    assert len(errs) == 22
    assert all(e < 2e-3 for e in errs.values()), {k: e for k, e in errs.items() if not e < 2e-3}
    assert all(p.grad is None for n, p in model.named_parameters() if not n.startswith(cf.PRE))


def test_eval_mode_forward(setup, data, yardstick):
    """evaluation: 25 x 25 probabilities = the sigmoid of the training-mode logits of the same boxes, pasted into the image within
    the pseudo-mask bar of tests/test_model_gpu.py (< 1e-4 of the pixels differ from the oracle's paste of the yardstick's logits)"""
    from oracle import model as om
    _, model = setup
    imgs, tgs, boxes, labels = data
    head = model.mask_heads.mask
    cls = [l.clamp(min=1) for l in labels]         # a class for every box: the post-processor reads the predicted class's channel
    il = _images(imgs)
    model.train()
    with torch.no_grad():
        for _ in range(2):   # (the second pass: every fp16-split site has seen these tensors, as it has when the eval pass runs)
            x, _ = head.feature_extractor(il.tensors, _proposals(boxes, cls, tgs))
            logits = head.predictor(x)
    model.eval()
    try:
        with torch.no_grad():
            _, result, losses = head(None, _proposals(boxes, cls, tgs), None, il)
            assert losses == {}
            prob = torch.cat([r.get_field("mask") for r in result])
            assert tuple(prob.shape) == (48, 1, 25, 25)
            want = logits.sigmoid()[torch.arange(48, device="cuda"), torch.cat(cls).cuda()][:, None]
            # the same launches on the same inputs in both modes of the module: the same bits
            print("eval probabilities against sigmoid(training-mode logits): max difference", (prob - want).abs().max().item())
            assert torch.equal(prob, want)
            # the evaluator's per-detection paste and the teacher's integral pseudo-mask, against the oracle on the yardstick's logits
            masker = head.mask_generator.masker
            ref_prob = yardstick["logits"].float().sigmoid()[torch.arange(48), torch.cat(cls)]
            for i, r in enumerate(result):
                stack = masker.forward_single_image(r.get_field("mask"), r)
                ref = torch.stack([om.paste_mask(m, b, SIZE, SIZE) for m, b in zip(ref_prob[24 * i:24 * i + 24], boxes[i])])
                mism = (stack[:, 0].cpu() != ref).float().mean().item()
                print("paste mismatch", mism)
                assert mism < 1e-4, mism
            head.set_teacher_mode("test")
            _, result, _ = head(None, _proposals(boxes, cls, tgs), None, il)
            dets = [om.Boxes(b, t["size"], {"labels": c}) for b, c, t in zip(boxes, cls, tgs)]
            ref = om.mask_generate(om.default_cfg(), yardstick["logits"].float(), dets)
            for r, s in zip(result, ref):
                mism = (r.get_field("mask").sum(0)[0].cpu().long() != s).float().mean().item()
                assert mism < 1e-4, mism
    finally:
        head.set_teacher_mode(None)
        model.train()


def _cspn_trainer(monkeypatch, **kw):
    """bench.build's trainer with CSPN.yaml's model keys on top of its defaults"""
    import bench
    import maskrcnn_benchmark.config as config
    plain = config.make_default_cfg
    monkeypatch.setattr(config, "make_default_cfg", lambda: cf.apply_keys(plain()))
    try:
        return bench.build(torch.device("cuda", 0), 0, crop=SIZE, n_inst=4, **kw)
    finally:
        monkeypatch.setattr(config, "make_default_cfg", plain)


def test_one_train_step(setup, monkeypatch):
    """one mean-teacher step with the CSPN keys (the fixture sets the arithmetic): finite losses, every parameter of the extractor
    moves, the teacher moves by the EMA of the student"""
    from maskrcnn_benchmark import _hip as H
    cfg, trainer, batch = _cspn_trainer(monkeypatch)
    assert type(trainer.student.mask_heads.mask.feature_extractor).__name__ == "PRCNNFeatureExtractor"
    assert type(trainer.teacher.mask_heads.mask.predictor).__name__ == "PRCNNPredictor"
    it = cfg.MT.START_MT + 400
    names = [n for n, _ in trainer.student.named_parameters() if n.startswith(FE)]
    assert len(names) == 20
    before = {n: p.detach().clone() for n, p in trainer.student.named_parameters() if n in names}
    t0 = trainer.flat_t.data.clone()
    trainer.seed_rng(5)
    il, tg, ul = batch()
    c0 = H.C_CALLS[0]
    losses = trainer.train_step(it, il, tg, ul)
    trainer.sync_teacher()
    torch.cuda.synchronize()
    assert H.C_CALLS[0] > c0
    assert set(losses) == {"loss_classifier", "loss_box_reg", "loss_seg", "loss_objectness", "loss_rpn_box_reg", "mt_fg_loss",
                           "mt_classifier"}, sorted(losses)
    assert all(torch.isfinite(v).item() for v in losses.values()), losses
    after = dict(trainer.student.named_parameters())
    for n in names:
        assert torch.isfinite(after[n]).all() and not torch.equal(after[n].detach(), before[n]), n
    # mmt_ema_update's formula on the two flat buffers: t <- t * (float) alpha + s * (float) (1 - alpha)
    alpha = min(1 - 1 / (it + 1), cfg.MT.ALPHA)
    a32, b32 = torch.tensor(alpha).float().item(), torch.tensor(1 - alpha).float().item()
    want = t0 * a32 + trainer.flat_s.data * b32
    torch.testing.assert_close(trainer.flat_t.data, want, rtol=1e-6, atol=1e-9)   # (one rounding: the kernel may contract the two terms)
    assert not torch.equal(trainer.flat_t.data, t0)


def test_default_step_issues_the_launches_it_did_before(monkeypatch):
    """the C-ABI call histogram of a default-config 160 x 160 step (tests/test_deterministic_kernels_gpu.py's counter) is the same
    before and after a CSPN model has been built and stepped in the process, and holds none of the new entry points"""
    from maskrcnn_benchmark import _hip as H
    import bench
    cfg, trainer, batch = bench.build(torch.device("cuda", 0), 0, crop=SIZE, n_inst=4, base_lr=0.0)   # (learning rate 0: every step is the same step)
    it = cfg.MT.START_MT + 400

    def step(tr, bt, count):
        hist = collections.Counter()
        orig = H._check

        def counting(code, what):
            hist[what] += 1
            return orig(code, what)
        tr.seed_rng(5)
        il, tg, ul = bt()
        if count:
            H._check = counting
        try:
            c0 = H.C_CALLS[0]
            tr.train_step(it, il, tg, ul)
            torch.cuda.synchronize()
        finally:
            H._check = orig
        return hist, H.C_CALLS[0] - c0

    for _ in range(3):      # plain, recorded, replayed: the launch plans are warm
        step(trainer, batch, False)
    before = step(trainer, batch, True)
    _, ctrainer, cbatch = _cspn_trainer(monkeypatch, base_lr=0.0)
    cspn = step(ctrainer, cbatch, True)
    del ctrainer, cbatch
    after = step(trainer, batch, True)
    assert before == after, (before, after)
    assert not any("roi_align_maps" in k for k in before[0])
    assert cspn[0]["mmt_roi_align_maps_forward"] >= 2 and cspn[0]["mmt_roi_align_maps_backward"] == 1, cspn[0]


def test_refusals(setup, data):
    """deterministic mode refuses the backward kernel by name and says the CSPN head is not offered there; bf16 activation storage
    refuses the head at construction, naming the key"""
    from maskrcnn_benchmark import _hip as H
    from maskrcnn_benchmark.config import make_default_cfg
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.mask_head import build_roi_mask_head
    go = torch.zeros((1, 7, 7, 8), device="cuda").permute(0, 3, 1, 2)
    rois = torch.tensor([[0., 1., 1., 9., 9.]], device="cuda")
    H.set_deterministic(True)
    try:
        with pytest.raises(NotImplementedError, match="CSPN mask head.* is not offered in deterministic mode: roi_align_maps_kernel"):
            H.roi_align_maps_backward(go, [(1, 8, 16, 16)], [1.0], rois, 7, 7, 2)
    finally:
        H.set_deterministic(False)
    assert len(H.roi_align_maps_backward(go, [(1, 8, 16, 16)], [1.0], rois, 7, 7, 2)) == 1
    prev = H.get_conv_precision()
    H.set_conv_precision(1)          # bf16 storage is in effect on the bf16 arithmetic only
    H.set_bf16_storage(True)
    try:
        assert H.bf16_storage()
        with pytest.raises(NotImplementedError, match="FEATURE_EXTRACTOR"):
            build_roi_mask_head(cf.apply_keys(make_default_cfg()))
        build_roi_mask_head(make_default_cfg())      # the default head is offered there as before
    finally:
        H.set_bf16_storage(False)
        H.set_conv_precision(prev)
