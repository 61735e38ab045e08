"""The guarded optimiser step on the device (include/mmtpsm.h: mmt_grad_guard, mmt_sgd_momentum_guarded; solver/build.py:
FlatSGD.enable_guard): the fp64 gradient norm against torch's, a non-finite gradient leaves parameters and momentum alone, a guard
that only observes changes no bit, a clipped step is `sgd_momentum` on the scaled gradient, and the same four properties of the
whole mean-teacher step (the bench's trainer at 160 x 160, deterministic mode, iterations from START_MT + 400 as in
tests/test_resume_gpu.py).

Tolerance of the norm, relative 1e-7, derived: an fp64 sum of at most 2^26 non-negative terms errs by less than 2^26 * 2^-53 =
7.5e-9 of the total in any order (half of that after the square root), and the one rounding of the result to fp32 adds at most
2^-24 = 6e-8."""
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

GRID = 4096 * 256 * 4       # elements of one full pass of stage one's largest grid
# 1, 3: the tail does everything; 4, 5: one float4 (and a tail); 1023: one block; GRID + 1 / + 4: one element / one float4 past a full
# first pass; 2 GRID + 3: beyond the block limit, a tail of 3; 5 GRID + 7: long enough for the four-loads-in-flight loop AND its
# remainder loop
NORM_SIZES = [1, 3, 4, 5, 1023, GRID + 1, GRID + 4, 2 * GRID + 3, 5 * GRID + 7]
SGD_SIZES = [1, 2, 3, 4, 5, 7, 1023, 4194307]      # tests/test_loss_optim_edges_gpu.py::test_sgd_momentum_three_steps_every_tail's


@pytest.fixture()
def hip():
    from maskrcnn_benchmark import _hip as H
    H.lib()
    assert torch.cuda.is_available()
    yield H
    H.set_deterministic(False)


def _guard(H, g, max_norm=0.0, bufs=None):
    """one `grad_guard` call -> (state on the device, its words as a CPU float tensor, the same words as Python ints)"""
    state, ws = bufs if bufs is not None else H.grad_guard_buffers(g.device)
    H.grad_guard(g, state, ws, max_norm)
    words = state.cpu()
    return state, words, words.view(torch.int32).tolist()


# ------------------------------------------------------------------------------------------ the norm
@pytest.mark.parametrize("n", NORM_SIZES)
def test_norm_against_fp64(hip, n):
    H = hip
    g = torch.randn(n, generator=torch.Generator().manual_seed(n))
    want = float(g.double().pow(2).sum().sqrt())
    gd = g.cuda()
    bufs = H.grad_guard_buffers(gd.device)
    _, words, ints = _guard(H, gd, 0.0, bufs)
    got = float(words[H.GUARD_NORM])
    print("n %d: norm %.9g, fp64 %.17g, relative error %.3g" % (n, got, want, abs(got - want) / want))
    assert abs(got - want) <= 1e-7 * want
    assert float(words[H.GUARD_COEF]) == 1.0 and ints[H.GUARD_SKIP] == 0
    assert ints[H.GUARD_SEEN:H.GUARD_CONSECUTIVE + 1] == [1, 0, 0, 0]
    _, again, ints = _guard(H, gd, 0.0, bufs)                         # the same input, the same bits
    assert torch.equal(again[0:2].view(torch.int32), words[0:2].view(torch.int32)) and ints[H.GUARD_SEEN] == 2
    assert torch.equal(gd.cpu(), g)


def test_a_square_beyond_fp32_is_still_finite(hip):
    """3e38 squared overflows fp32, not fp64: the gradient is finite and so is the verdict"""
    H = hip
    g = torch.randn(1023, generator=torch.Generator().manual_seed(3))
    g[517] = 3e38
    want = float(g.double().pow(2).sum().sqrt())
    _, words, ints = _guard(H, g.cuda())
    got = float(words[H.GUARD_NORM])
    assert np.isfinite(got) and abs(got - want) <= 1e-7 * want
    assert ints[H.GUARD_SKIP] == 0 and ints[H.GUARD_SKIPPED] == 0 and float(words[H.GUARD_COEF]) == 1.0


# ------------------------------------------------------------------------------------------ non-finite gradients
N_BAD = 3 * 1024 + 3      # three blocks and a tail of 3


@pytest.mark.parametrize("where", [0, N_BAD // 2, N_BAD - 1], ids=["first", "middle", "last-in-tail"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_a_non_finite_gradient_skips_the_step(hip, bad, where):
    H = hip
    gen = torch.Generator().manual_seed(11)
    clean = torch.randn(N_BAD, generator=gen).cuda()
    g = clean.clone()
    g[where] = bad
    p, buf = torch.randn(N_BAD, generator=gen).cuda(), torch.randn(N_BAD, generator=gen).cuda()
    p0, buf0, g0 = p.clone(), buf.clone(), g.clone()
    for max_norm in (0.0, 1.0):                                         # with and without a clip: the skip comes first
        bufs = H.grad_guard_buffers(g.device)
        state, words, ints = _guard(H, g, max_norm, bufs)
        assert ints[H.GUARD_SKIP] == 1 and float(words[H.GUARD_COEF]) == 0.0 and not np.isfinite(float(words[H.GUARD_NORM]))
        for first in (False, True):
            H.sgd_momentum_guarded(p, g, buf, 0.01, 1e-4, 0.9, first, state)
        torch.cuda.synchronize()
        assert torch.equal(p, p0) and torch.equal(buf, buf0)
        assert torch.equal(g.view(torch.int32), g0.view(torch.int32))
        assert ints[H.GUARD_SEEN:H.GUARD_CONSECUTIVE + 1] == [1, 1, 0, 1]   # seen, skipped, clipped, consecutive
        _, words, ints = _guard(H, clean, max_norm, bufs)                # a clean step follows
        assert ints[H.GUARD_SKIP] == 0 and float(words[H.GUARD_COEF]) > 0.0
        assert ints[H.GUARD_SEEN:H.GUARD_CONSECUTIVE + 1] == [2, 1, 1 if max_norm else 0, 0]


# ------------------------------------------------------------------------------------------ a guard that lets the step through
@pytest.mark.parametrize("n", SGD_SIZES)
@pytest.mark.parametrize("first", [True, False])
def test_an_unclipped_step_is_sgd_momentum_bit_for_bit(hip, n, first):
    H = hip
    gen = torch.Generator().manual_seed(n + 1)
    a = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen).cuda() for _ in range(2)]
    for max_norm in (0.0, 1e30):                                        # no clipping / a limit far above the norm
        p, q = a.clone().cuda(), a.clone().cuda()
        bp = torch.full((n,), float("nan")).cuda() if first else torch.zeros(n).cuda()
        bq = bp.clone()
        bufs = H.grad_guard_buffers(p.device)
        for step, gr in enumerate(grads):
            H.sgd_momentum(p, gr, bp, 0.01, 1e-4, 0.9, first and step == 0)
            state, words, ints = _guard(H, gr, max_norm, bufs)
            assert float(words[H.GUARD_COEF]) == 1.0 and ints[H.GUARD_SKIP] == 0
            H.sgd_momentum_guarded(q, gr, bq, 0.01, 1e-4, 0.9, first and step == 0, state)
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)) and torch.equal(bp.view(torch.int32), bq.view(torch.int32))
        assert ints[H.GUARD_SEEN:H.GUARD_CONSECUTIVE + 1] == [2, 0, 0, 0]
        assert not torch.equal(p.cpu(), a)


# ------------------------------------------------------------------------------------------ a clipped step
@pytest.mark.parametrize("n", [5, 1023, 300003])
@pytest.mark.parametrize("first", [True, False])
def test_a_clipped_step(hip, n, first):
    H = hip
    gen = torch.Generator().manual_seed(n + 2)
    a, b0, gr = torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    norm = float(gr.double().pow(2).sum().sqrt())
    max_norm = 0.25 * norm
    g = gr.cuda()
    state, words, ints = _guard(H, g, max_norm)
    coef = float(words[H.GUARD_COEF])
    assert ints[H.GUARD_SKIP] == 0 and ints[H.GUARD_CLIPPED] == 1
    assert abs(coef - max_norm / (norm + 1e-6)) <= 3e-7 * coef and coef < 0.2500001   # fp32: the norm, the sum, the quotient
    p, buf = a.clone().cuda(), b0.clone().cuda()
    H.sgd_momentum_guarded(p, g, buf, 0.01, 1e-4, 0.9, first, state)
    q, bq = a.clone().cuda(), b0.clone().cuda()
    H.sgd_momentum(q, g * state[H.GUARD_COEF], bq, 0.01, 1e-4, 0.9, first)         # torch's fp32 multiply, then the plain kernel
    assert torch.equal(p.view(torch.int32), q.view(torch.int32)) and torch.equal(buf.view(torch.int32), bq.view(torch.int32))
    assert torch.equal(g.cpu(), gr)                                                  # the gradient itself is not scaled
    # torch in fp64: clip_grad_norm_, then SGD (whose first step ignores the buffer, as `first` does)
    w = torch.nn.Parameter(a.double())
    w.grad = gr.double()
    opt = torch.optim.SGD([w], lr=0.01, momentum=0.9, weight_decay=1e-4)
    if not first:
        opt.state[w]["momentum_buffer"] = b0.double().clone()
    torch.nn.utils.clip_grad_norm_([w], max_norm)
    opt.step()
    np.testing.assert_allclose(p.cpu().numpy(), w.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(buf.cpu().numpy(), opt.state[w]["momentum_buffer"].numpy(), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------ refused arguments
def test_refused_arguments(hip):
    H = hip
    dev = torch.device("cuda", 0)
    g, p, buf = (torch.randn(64, device=dev) for _ in range(3))
    p0, buf0 = p.clone(), buf.clone()
    state, ws = H.grad_guard_buffers(dev)
    longer = torch.zeros(H.GRAD_GUARD_STATE_WORDS + 5, device=dev)
    guard_calls = [
        (g[1:], state, ws),                                                          # off the 16-byte grid
        (g[::2], state, ws),                                                         # not dense
        (g.double(), state, ws), (g.half(), state, ws),                              # not fp32
        (g.cpu(), state, ws),                                                        # not on the device
        (g, state[:-1], ws), (g, longer, ws),                                        # state: the wrong size
        (g, longer[1:1 + H.GRAD_GUARD_STATE_WORDS], ws),                             # ... the right size, misaligned
        (g, state.view(torch.int32), ws), (g, state.double(), ws),                   # ... the wrong dtype
        (g, state, ws.float()), (g, state, ws[:-1]), (g, state, ws[1:]),             # workspace: dtype, size
    ]
    for args in guard_calls:
        with pytest.raises(RuntimeError):
            H.grad_guard(*args, 0.0)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            H.grad_guard(g, state, ws, bad)
    sgd_calls = [
        (p[1:], g[1:], buf[1:], state), (p[:-1], g[1:], buf[:-1], state), (p[:-1], g[:-1], buf[1:], state),
        (p, g[:-4], buf, state), (p.double(), g, buf, state), (p, g, buf, state[:-1]), (p, g, buf, state.view(torch.int32)),
        (p, g, buf, state.cpu()),
    ]
    for a, b, c, st in sgd_calls:
        with pytest.raises(RuntimeError):
            H.sgd_momentum_guarded(a, b, c, 0.01, 1e-4, 0.9, False, st)
    torch.cuda.synchronize()
    assert torch.equal(p, p0) and torch.equal(buf, buf0) and not state.any()      # nothing was launched


# ------------------------------------------------------------------------------------------ the training step
def _build(save_dir=None):
    import bench
    from maskrcnn_benchmark.utils.checkpoint import Checkpointer
    torch.manual_seed(0)
    cfg, trainer, batch = bench.build(torch.device("cuda", 0), 0, crop=160, n_inst=4, base_lr=0.005)
    trainer.seed_rng(0)
    if save_dir is not None:
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


def _poison(trainer, value=float("nan")):
    """every `optimizer.step` from now on finds one bad value in the flat gradient; -> the undo"""
    opt, step = trainer.optimizer, trainer.optimizer.step

    def poisoned():
        trainer.flat_s.grad[trainer.flat_s.n_weights // 2] = value
        step()
    opt.step = poisoned
    return lambda: setattr(opt, "step", step)


def test_a_guard_that_only_observes_changes_no_bit(hip):
    H = hip
    H.set_deterministic(True)
    runs = []
    for guarded in (False, True):
        cfg, trainer, batch = _build()
        if guarded:
            trainer.optimizer.enable_guard(max_norm=0.0)
        runs.append([_step(cfg, trainer, batch, s) for s in (1, 2)])
    for s, (x, y) in enumerate(zip(*runs), 1):
        for name, u, v in zip(("student", "momentum", "teacher"), x[:3], y[:3]):
            assert torch.equal(u, v), "step %d, %s: %d of %d elements differ" % (s, name, int((u != v).sum()), u.numel())
        assert sorted(x[3]) == sorted(y[3]) and all(torch.equal(x[3][k], y[3][k]) for k in x[3]), "step %d: losses" % s
    assert not torch.equal(runs[0][0][0], runs[0][1][0])                           # the steps did move the student
    st = trainer.optimizer.guard_stats()
    assert (st["seen"], st["skipped"], st["clipped"], st["consecutive"]) == (2, 0, 0, 0)
    want = float(trainer.flat_s.grad.double().pow(2).sum().sqrt())                # the last step's gradient is still there
    assert want > 0 and abs(st["norm"] - want) <= 1e-7 * want


def test_a_poisoned_step_is_skipped_and_the_counters_resume(hip, tmp_path):
    H = hip
    H.set_deterministic(True)
    cfg, a, batch = _build(tmp_path)
    a.optimizer.enable_guard(max_norm=0.0)
    one = _step(cfg, a, batch, 1)
    undo = _poison(a)
    two = _step(cfg, a, batch, 2)
    undo()
    assert torch.equal(two[0], one[0]) and torch.equal(two[1], one[1])             # student and momentum: untouched
    assert bool(torch.isfinite(two[2]).all()) and bool(torch.isfinite(two[0]).all())
    assert not torch.equal(two[2], one[2])                                         # the EMA still ran, on the unchanged student
    st = a.optimizer.guard_stats()
    assert (st["seen"], st["skipped"], st["consecutive"]) == (2, 1, 1) and not np.isfinite(st["norm"])
    assert a.optimizer.steps == 2 and a.last_iteration == cfg.MT.START_MT + 401    # schedule and iteration counter advance
    three = _step(cfg, a, batch, 3)
    assert not torch.equal(three[0], two[0]) and not torch.equal(three[1], two[1]) and bool(torch.isfinite(three[0]).all())
    st = a.optimizer.guard_stats()
    assert (st["seen"], st["skipped"], st["consecutive"]) == (3, 1, 0) and np.isfinite(st["norm"])
    # the counters are part of the checkpoint
    a.save_model(cfg.MT.START_MT + 402)
    del a
    cfg, b, batch = _build(tmp_path)
    b.optimizer.enable_guard(max_norm=0.0)
    assert b.optimizer.guard_stats()["seen"] == 0
    assert b.resume() == cfg.MT.START_MT + 402
    got = b.optimizer.guard_stats()
    assert {k: got[k] for k in ("seen", "skipped", "clipped", "consecutive")} == {k: st[k] for k in ("seen", "skipped", "clipped", "consecutive")}
    assert torch.equal(b.flat_s.data, three[0]) and torch.equal(b.flat_s.momentum, three[1])


def test_train_gives_up_at_the_skip_limit(hip):
    H = hip
    cfg, t, batch = _build()
    t.optimizer.enable_guard(max_norm=0.0, max_consecutive_skips=1)
    first = cfg.MT.START_MT + 400                                                  # a multiple of 20: the log line's iteration
    labeled, unlabeled = [], []
    for j in range(3):
        il, tg, ul = batch()
        labeled.append((il, tg, j))
        unlabeled.append((ul, j))
    t.dataloader_s, t.dataloader_u, t.start_iter = labeled, unlabeled, first
    before = _buffers(t)
    _poison(t, float("inf"))
    with pytest.raises(RuntimeError, match="MAX_CONSECUTIVE_SKIPS 1"):
        t.train()
    assert t.last_iteration == first                                               # at the first log line, not after the loader
    after = _buffers(t)
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
