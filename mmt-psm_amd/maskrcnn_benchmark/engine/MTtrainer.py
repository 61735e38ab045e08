"""Mean-teacher engine (reference: engine/MTtrainer.py:16-281): per-iteration
  [A] student(image, target)  [B] teacher.forward_teacher(K augs)  [C] student.forward_student(aug, teacher dict)
  [D] weighted loss sum -> backward -> SGD  [E] EMA teacher update.
Arithmetic of loss weighting (weight_sum_losses, including the reference's ramp-down-with-ramp-up-length quirk)
and of the EMA (alpha = min(1 - 1/(it+1), MT.ALPHA)) is reproduced; EMA and SGD are single launches over flat
storage; with WORLD_SIZE > 1 the student gradients are averaged by ONE RCCL all-reduce over the flat gradient
buffer (new functionality: the reference has no gradient synchronisation at all)."""
import logging
import os
import random
import time
from functools import partial

import numpy as np
import torch
import torch.distributed as dist

from maskrcnn_benchmark import _hip as H
from maskrcnn_benchmark.engine.flat import flatten_model
from maskrcnn_benchmark.layers import fused
from maskrcnn_benchmark.utils.miscellaneous import sigmoid_rampdown, sigmoid_rampup
from maskrcnn_benchmark.utils.model_serialization import load_state_dict, refresh_derived, strip_prefix_if_present


# priority -1: HIP maps streams of one priority onto a few hardware queues round-robin; once RCCL has created its own
# streams (torch.distributed initialised) a default-priority side stream lands on the SAME hardware queue as the
# main stream and the overlap silently disappears (measured: 63.7 vs 59.9 ms/step).  A different priority class
# has its own queues.
_TEACHER_PRIO = -1


def get_world_size():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def reduce_loss_dict(loss_dict):
    """MTtrainer.py:16-42: rank 0 gets the average (logging only)"""
    ws = get_world_size()
    if ws < 2:
        return dict(loss_dict)
    with torch.no_grad():
        names = sorted(loss_dict.keys())  # same order on every rank
        allv = torch.stack([loss_dict[k].reshape(()) for k in names], 0)
        dist.reduce(allv, dst=0)
        if dist.get_rank() == 0:
            allv /= ws
        return {k: v for k, v in zip(names, allv)}


def mt_weight(step, rampup_length, rampdown_length, total_length, l=1, start_mt=1000):
    if (step - start_mt) < rampup_length and (step - start_mt) > 0:
        return l * sigmoid_rampup(step - start_mt, rampup_length)
    if (total_length - step) < rampdown_length:
        return l * sigmoid_rampdown(total_length - step, rampup_length)  # sic: ramp-UP length (MTtrainer.py:92)
    return l


def weight_sum_losses(loss_dict, step, rampup_length, rampdown_length, total_length, l=1, balanced=None, start_mt=1000):
    """MTtrainer.py:67-109"""
    w = mt_weight(step, rampup_length, rampdown_length, total_length, l, start_mt)
    out = {}
    for k, v in loss_dict.items():
        v = w * v if "mt" in k else v
        if balanced is not None and k in balanced:
            v = v * balanced[k]
        out[k] = v
    return out


def init_teacher_weight(model_s, model_t):
    flatten_model(model_t).data.copy_(flatten_model(model_s).data)
    flatten_model(model_t).refresh_planes()


def allreduce_gradients(flat):
    """data-parallel exchange step: average the flat student gradient over ranks (RCCL over xGMI)"""
    ws = get_world_size()
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(flat.grad, op=dist.ReduceOp.SUM)
        if ws > 1:
            flat.grad.mul_(1.0 / ws)


_FLAG_SYNC = {}   # process-wide: the flag exchange's own communicator and stream (built once, collectively)


def sync_touched(flat):
    """Which parameters "have a gradient" this step must be the same on every rank: the all-reduce hands every rank the same
    averaged gradient, but `flat.touched` (what FlatSGD.step updates, torch SGD's `p.grad is None: continue`) is filled by
    THIS rank's backward nodes.  A rank whose teacher found no boxes skipped the consistency branch and never touched the
    hint adaptors while the others did -- and a supervised pass can take a degenerate route on one rank only (crops without
    ground truth: no mask-head positives) --; updating parameters on some ranks only would let the students, and with them the
    EMA teachers, drift apart for good.  The update set is therefore the UNION over ranks, EVERY step: one MAX
    all-reduce of a per-parameter flag vector (a few hundred bytes).
    Round 5: the flags are host data (filled while backward was ISSUED), so their exchange does not have to wait for the device:
    it runs on a communicator and a stream of its own -- behind nothing the step has queued -- and the read-back returns as soon
    as those few hundred bytes have crossed, with the backward pass still running (round 4 issued it on the gradient's
    communicator, behind every gradient piece, and read it back with a blocking `.tolist()`: a device drain in front of SGD)."""
    if get_world_size() < 2:
        return
    ent = flat.__dict__.get("_touch_sync")
    if ent is None:
        names = [n for n, (o, _) in sorted(flat.index.items(), key=lambda kv: kv[1][0]) if o < flat.n_trainable]
        host = torch.zeros((len(names),), dtype=torch.int32)
        back = torch.zeros((len(names),), dtype=torch.int32)
        if flat.grad.is_cuda:
            host, back = host.pin_memory(), back.pin_memory()
        ent = flat._touch_sync = (names, host, back)
    names, host, back = ent
    touched = flat.touched
    for i, n in enumerate(names):
        host[i] = 1 if n in touched else 0
    if "group" not in _FLAG_SYNC:   # (collective: every rank reaches its first step's exchange)
        _FLAG_SYNC["group"] = dist.new_group()
        _FLAG_SYNC["stream"] = torch.cuda.Stream(device=flat.grad.device) if flat.grad.is_cuda else None
    side = _FLAG_SYNC["stream"]
    if side is None:
        flags = host.clone()
        dist.all_reduce(flags, op=dist.ReduceOp.MAX, group=_FLAG_SYNC["group"])
        got = flags.tolist()
    else:
        with torch.cuda.stream(side):
            flags = host.to(flat.grad.device, non_blocking=True)
            dist.all_reduce(flags, op=dist.ReduceOp.MAX, group=_FLAG_SYNC["group"])
            back.copy_(flags, non_blocking=True)
            done = torch.cuda.Event()
            done.record(side)
        done.synchronize()        # the side stream's few operations only
        got = back.tolist()
    flat.touched.update(n for n, f in zip(names, got) if f)


class BucketedAllReduce(object):
    """The same exchange, started while the backward pass is still running.  The flat gradient is cut at the stage
    boundaries of the backbone ([layer2 | layer3 | layer4 | FPN + heads]: the weights region of engine/flat.py is in
    parameter order); backward runs through these pieces from the right, and a tensor hook on each stage output
    (modeling/backbone/backbone.py) says when the pieces to its right are final.  Each finished piece goes out as an
    asynchronous all-reduce that overlaps the backward of the earlier stages; whatever is left (layer2, the bias region)
    is reduced at the end.  One scaling pass by 1/world afterwards, as in `allreduce_gradients`.

    The sequence of collectives is the SAME on every rank whatever happened on it: always the stage pieces in the fixed
    order layer4, layer3, layer2, layer1 (each exactly one all-reduce over the same [lo, hi)), then the fixed remainder
    ranges in ascending order.  A piece whose hook did not fire often enough on this rank -- its teacher found no boxes
    and the consistency branch was skipped, so the second backbone pass was never back-propagated -- is sent from
    finish() as its own collective instead of being merged into a neighbour (ranks that did fire it sent exactly that)."""

    # a hook on the output of stage K fires when everything AFTER stage K is done; "heads" = hooks on the pyramid levels (round 5):
    # the RPN / box / mask heads, adaptors and relation modules -- half of the 82 MB that used to leave with the FPN -- go out when
    # the heads' backward ends, ~10 ms before the FPN's (profiles/r04_bench_rccl_world1.json: that piece was issued 3.5 ms before
    # the end of a 36 ms backward)
    AFTER = {"heads": None, "layer4": "backbone.fpn.", "layer3": "backbone.body.layer4.", "layer2": "backbone.body.layer3.",
             "layer1": "backbone.body.layer2."}
    ORDER = ("heads", "layer4", "layer3", "layer2", "layer1")  # firing order of the hooks in a backward pass

    def __init__(self, flat, body):
        self.flat, self.body = flat, body
        names = [n for n, _ in flat._named if n in flat.index and flat.index[n][0] < flat.n_weights]
        cuts = {}
        for stage, prefix in self.AFTER.items():
            if prefix is None:   # everything behind the backbone, in parameter order
                last_bb = max((i for i, n in enumerate(names) if n.startswith("backbone.")), default=-1)
                first = names[last_bb + 1] if 0 <= last_bb < len(names) - 1 else None
            else:
                first = next((n for n in names if n.startswith(prefix)), None)
            if first is not None:
                cuts[stage] = flat.index[first][0]
        # piece that becomes final when `stage` fires: [cut(stage), cut(previous firing stage) or n_weights)
        self.pieces, hi = {}, flat.n_weights
        for s_ in (s for s in self.ORDER if s in cuts):
            lo = cuts[s_]
            if lo < hi:
                self.pieces[s_] = (lo, hi)
            hi = min(hi, lo)
        # what no stage piece covers (the weights before the first cut, the bias region): fixed ranges, sent last
        self.rest, pos, n = [], 0, flat.grad.numel()
        for lo, hi in sorted(self.pieces.values()) + [(n, n)]:
            if pos < lo:
                self.rest.append((pos, lo))
            pos = max(pos, hi)
        self.reset()

    def reset(self):
        self.registered, self.fired, self.sent, self.works = {}, {}, set(), []
        self._marks = []

    def install(self):
        self.reset()
        self.body.grad_ready = self._event
        # MMT_DIST_TRACE=1: per-piece issue / completion times on the device clock (events on the step stream), so that the
        # first multi-GPU run shows at once whether the exchange hides behind the backward pass (`last_trace`)
        self.tracing = os.environ.get("MMT_DIST_TRACE") == "1" and self.flat.grad.is_cuda
        if self.tracing:
            self._t0 = torch.cuda.Event(enable_timing=True)
            self._t0.record()

    def _send(self, lo, hi):
        """one piece of the flat gradient goes out.  Its last contributions are weight gradients on the SIDE stream (layers/fused.py)
        and whatever the step stream has issued up to this hook.  Round 4: the collective is issued FROM the side stream, behind a
        side-waits-for-step-stream edge -- RCCL's stream then orders itself behind both, and the step stream is never made to wait
        (round 3 joined the side stream into the step stream here: four stalls of the data-gradient chain per backward pass, part of
        the +2.4 ms a process group cost at world size 1)."""
        g = self.flat.grad
        side = fused.side_stream_for_exchange(g.device) if g.is_cuda else None
        if getattr(self, "tracing", False):   # when backward reached this hook, on the STEP stream's clock (the mark used
            e = torch.cuda.Event(enable_timing=True)   # to be recorded inside the side-stream context and measured that queue)
            e.record()
            self._marks.append([lo, hi, e, None, time.perf_counter()])
        if side is None:
            fused.join_wgrads()   # no side stream in this configuration: the piece is final on the step stream
            self._issue(lo, hi)
            return
        with torch.cuda.stream(side):
            self._issue(lo, hi)

    def _issue(self, lo, hi):
        self.works.append(dist.all_reduce(self.flat.grad[lo:hi], op=dist.ReduceOp.SUM, async_op=True))

    def _event(self, stage, what):
        if what == "registered":
            self.registered[stage] = self.registered.get(stage, 0) + 1
            return
        self.fired[stage] = self.fired.get(stage, 0) + 1
        # several backbone passes in one step: the piece is final when the LAST registered pass has fired
        if stage in self.pieces and stage not in self.sent and self.fired[stage] == self.registered.get(stage, 0):
            # earlier pieces of the fixed order that this rank never completed go first, so the order stays the same
            for s_ in self.ORDER:
                if s_ == stage:
                    break
                if s_ in self.pieces and s_ not in self.sent:
                    self._send(*self.pieces[s_])
                    self.sent.add(s_)
            self._send(*self.pieces[stage])
            self.sent.add(stage)

    def finish(self):
        """after backward: reduce what no hook covered (fixed order), wait for everything, scale"""
        self.body.grad_ready = None
        for s_ in self.ORDER:
            if s_ in self.pieces and s_ not in self.sent:
                self._send(*self.pieces[s_])
                self.sent.add(s_)
        tracing = getattr(self, "tracing", False)
        if tracing:
            bw_end = torch.cuda.Event(enable_timing=True)
            bw_end.record()
            n_early = len(self._marks)
        for lo, hi in self.rest:
            self._send(lo, hi)
        for i, w in enumerate(self.works):
            if w is not None:
                w.wait()
            if tracing:
                e = torch.cuda.Event(enable_timing=True)
                e.record()       # the step stream gets here when piece i has arrived
                self._marks[i][3] = e
        ws = get_world_size()
        if ws > 1:
            self.flat.grad.mul_(1.0 / ws)
        if tracing:
            torch.cuda.synchronize()
            self.last_trace = {
                "backward_end_ms": round(self._t0.elapsed_time(bw_end), 3), "pieces_sent_before_backward_end": n_early,
                # what the exchange costs the step: from the end of backward to the arrival of the last piece (0 = fully hidden)
                "exposed_comm_ms": round(max([self._t0.elapsed_time(m[3]) for m in self._marks] + [0.0]) - self._t0.elapsed_time(bw_end), 3),
                "pieces": [{"range": [lo, hi], "mbytes": round((hi - lo) * 4 / 1e6, 2), "issued_ms": round(self._t0.elapsed_time(a), 3),
                            "arrived_ms": round(self._t0.elapsed_time(b), 3)} for lo, hi, a, b, _ in self._marks]}
            # (round 6) what the same issue schedule would cost at 8 GPUs under the xGMI model -- a prediction, never a measurement
            self.last_trace["predicted_8gpu"] = predict_exposed_comm(self.last_trace["pieces"], self.last_trace["backward_end_ms"], 8)
        self.reset()


XGMI_LINK_GBS = 153.0   # xGMI is a full mesh, 7 links x ~153 GB/s per GPU


def predict_exposed_comm(pieces, backward_end_ms, world=8, link_gbs=XGMI_LINK_GBS, latency_ms=0.05):
    """What the bucketed exchange would cost a step at `world` GPUs, from the issue times a (world-size-1) trace recorded and SURVEY
    section 5's xGMI model -- a number for the first real multi-GPU run to be wrong against (no 8-GPU node was
    ever available to the builder).  Two collective algorithms bracket what RCCL does on a full mesh:
      ring        2 (world - 1) hops of bytes / world over ONE link each:  t = 2 (world - 1) / world * bytes / link
      direct      reduce-scatter + all-gather over all world - 1 links at once:  t = 2 / world * bytes / link
    Pieces go out in issue order on one communicator: piece i starts at max(its issue time, the end of piece i - 1) and takes
    t(bytes) + a fixed launch / synchronisation latency.  exposed = end of the last piece - end of backward (>= 0).
    pieces: [{"mbytes", "issued_ms"}, ...] as in `dist_trace`."""
    out = {}
    for name, factor in (("ring", 2.0 * (world - 1) / world), ("direct", 2.0 / world)):
        t = 0.0
        for p in sorted(pieces, key=lambda q: q["issued_ms"]):
            t = max(t, p["issued_ms"]) + latency_ms + factor * p["mbytes"] * 1e6 / (link_gbs * 1e9) * 1e3
        out[name] = {"last_arrival_ms": round(t, 3), "exposed_comm_ms": round(max(0.0, t - backward_end_ms), 3)}
    out["model"] = ("SURVEY section 5: %d GPUs, full-mesh xGMI at %.0f GB/s per link, %.2f ms fixed cost per collective; ring = "
                    "2 (N - 1) / N x bytes over one link, direct = 2 / N x bytes over all links; issue times from this run's trace"
                    % (world, link_gbs, latency_ms))
    return out


def teacher_checksum(flat):
    """exact (integer) checksum of a flat parameter buffer: the sum of its words read as int32, in int64"""
    return flat.data.view(torch.int32).to(torch.int64).sum()


RESUME_FORMAT = 1   # of the `trainer` entry MTtrainer.save_model adds to the student's checkpoint file


def _word_sum(t):
    """`teacher_checksum` of any fp32 buffer, as a Python int"""
    return int(t.view(torch.int32).to(torch.int64).sum())


def _name_problems(what, saved, have):
    """-> one line per name of `saved` / `have` (name -> shape) that the other side lacks or holds in another shape"""
    out = ["%s %s: in this model, not in the file" % (what, n) for n in sorted(set(have) - set(saved))]
    out += ["%s %s: in the file, not in this model" % (what, n) for n in sorted(set(saved) - set(have))]
    out += ["%s %s: shape %s in the file, %s in this model" % (what, n, list(saved[n]), list(have[n]))
            for n in sorted(set(saved) & set(have)) if tuple(saved[n]) != tuple(have[n])]
    return out


def check_teacher_identity(flat_t):
    """the teachers are never exchanged -- they stay identical on all ranks because every rank applies the
    same EMA to the same (all-reduced) student from the same initial weights.  Asserted here with ONE small collective:
    max over ranks of (checksum, -checksum); equal teachers <=> max(c) == -max(-c)."""
    if get_world_size() < 2:
        return True
    c = teacher_checksum(flat_t)
    v = torch.stack([c, -c])
    dist.all_reduce(v, op=dist.ReduceOp.MAX)
    hi, neg_lo = v.tolist()
    if hi != -neg_lo:
        raise RuntimeError("teacher weights diverged between ranks (checksum max %d != min %d)" % (hi, -neg_lo))
    return True


class MTtrainer(object):
    def __init__(self, model_s, model_t, data_loader, optimizer, scheduler, ckpt_s, ckpt_t, checkpoint_period, cfg):
        self.cfg = cfg
        self.logger = logging.getLogger("maskrcnn_benchmark.trainer")
        self.scheduler, self.optimizer = scheduler, optimizer
        self.max_iter = len(data_loader["source"])
        self.start_iter = 0          # `resume` moves it behind the checkpoint's iteration
        self.last_iteration = -1     # the last completed iteration (what a checkpoint records)
        self.unlabeled_seen = 0      # batches drawn from the unlabeled loader so far
        self._unl_skip = 0           # batches the first use of the unlabeled loader after a `resume` passes over
        self.student, self.teacher = model_s, model_t
        self.student_bs, self.teacher_bs = cfg.MT.AUG_S, cfg.MT.AUG_K
        # (without a device: the host-side halves -- state_dict, resume and their refusals -- on CPU tensors; a step needs the device)
        self.device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.checkpoint_period, self.ckpt_s, self.ckpt_t = checkpoint_period, ckpt_s, ckpt_t
        self.lambda_value, self.alpha = cfg.MT.LAMBDA, cfg.MT.ALPHA
        self.start_mt = cfg.MT.START_MT
        self.balanced_weight = {"mt_classifier": cfg.MT.CLS_LOSS, "nms_loss": cfg.MODEL.RELATION_NMS.LOSS,
                                "mt_fg_loss": cfg.MT.FG_HINT}
        self.dataloader_s = data_loader["source"]
        self.dataloader_u = data_loader.get("no_label") if cfg.DATASETS.NO_LABEL else None
        self.n_step_unlabel = cfg.MT.N_STEP_UNLABEL
        self.weight_sum_loss = partial(weight_sum_losses, rampup_length=cfg.MT.RAMPUP_STEP,
                                       rampdown_length=cfg.MT.RAMPDOWN_STEP, total_length=self.max_iter,
                                       l=self.lambda_value, balanced=self.balanced_weight, start_mt=self.start_mt)
        self.flat_s = flatten_model(self.student)
        self.flat_t = flatten_model(self.teacher)
        self._unl_iter = None
        # The teacher's no-grad forward and the student's supervised forward are independent until the consistency
        # losses: run the teacher on its own HIP stream (issued from a helper thread -- both forwards contain host syncs),
        # so that its large convolutions fill the GPU while the other stream is in launch-latency-bound target / proposal
        # glue, and vice versa.  MMT_OVERLAP_TEACHER=0 restores the serial order.
        self.overlap_teacher = os.environ.get("MMT_OVERLAP_TEACHER", "1") != "0" and self.device.type == "cuda"
        self.early_sup_backward = True
        # "pair" (one N = 4 forward, two autograd graphs: the default) | "split" (two passes) | "batched" (one pass, one graph):
        # the alternatives are what tests/test_train_step_gpu.py compares the default schedule with
        self.student_passes = "pair"
        self.skipped_pairs = 0  # steps whose consistency branch was skipped (no pseudo box on some image)
        self.t_stream = torch.cuda.Stream(device=self.device, priority=_TEACHER_PRIO) if self.overlap_teacher else None
        self._bucketed = None  # BucketedAllReduce, built lazily when enabled (see _bucketed_allreduce)
        # One random stream per model: the teacher's forward runs in a helper thread beside the student's, and with the
        # global generator the interleaving of their draws (fg/bg sampler keys, dropout) would depend on thread timing.
        # With its own generator each model draws the same sequence in the overlapped and in the serial schedule.
        self.gen_s = self.gen_t = None
        if self.device.type == "cuda":
            self.gen_s = torch.Generator(device=self.device)
            self.gen_t = torch.Generator(device=self.device)
            self.seed_rng(torch.initial_seed())
            self.student.set_rng(self.gen_s)
            self.teacher.set_rng(self.gen_t)
        self.teacher_check_period = int(os.environ.get("MMT_TEACHER_CHECK_PERIOD", "100"))
        if H.get_deterministic():
            # a run is repeatable from ITS start: what an earlier trainer of this process taught the host side about tensor ranges
            # (producers' plane scales, delayed scales, site states) would make this trainer's first steps differ from a fresh process's
            H.reset_adaptive_state()

    def seed_rng(self, seed):
        """re-seed the student's and the teacher's random streams (samplers, dropout)"""
        if self.gen_s is not None:
            self.gen_s.manual_seed(int(seed) * 2 + 1)
            self.gen_t.manual_seed(int(seed) * 2 + 2)

    # ---- one iteration (the unit bench.py times)
    def train_step(self, iteration, data_s, target_s, data_u_list=None):
        use_mt = iteration > self.start_mt and self.lambda_value > 0 and data_u_list is not None
        bucketed = self._bucketed_allreduce()
        if bucketed is not None:
            bucketed.install()  # the stage hooks are registered by the forward passes below
        feats_s = feats_u = None
        early, cut = False, None
        job = None
        xu = None
        if use_mt:
            xs = data_s.tensors.to(self.device)
            # AUG_S > 1: the S views as one batch -- the same pass schedules as for the single view
            xu = data_u_list[-1].tensors.to(self.device) if self.student_bs == 1 else self._student_views(data_u_list)
        if xu is not None:
            if self.student_passes == "pair" and xs.shape == xu.shape:
                # one set of forward launches for both passes (N = 4), two autograd graphs (modeling/backbone/backbone.py:
                # forward_pair): the schedule below is that of "split"
                from maskrcnn_benchmark.modeling.backbone.backbone import forward_pair
                feats_s, fu = forward_pair(self.student.backbone, xs, xu)
                feats_u = [fu]
                early = True
            elif self.student_passes in ("split", "pair"):
                # Two student backbone passes, labeled crops and unlabeled view.  The supervised branch then runs its WHOLE
                # backward (heads, FPN, backbone) while this thread would otherwise only wait for the teacher -- the teacher is
                # the critical path of the forward and its launch-bound stretches leave the GPU room -- and only the
                # consistency branch is left for after the teacher.  (Batching the two passes makes larger GEMMs but keeps
                # the backbone backward behind the teacher: 50.0 vs 51.8 ms/step.)
                # Measured on the stationary bench (46.4 ms): starting the teacher BEFORE these passes 50.5, the unlabeled
                # view's pass issued after the supervised backward 46.5, batched 48.0, batched + teacher first 49.0 --
                # between 8 and 37 ms both streams hold convolution work and the step is the sum of the kernel times.
                feats_s = self.student.run_backbone(xs, 0)
                feats_u = [self.student.run_backbone(xu, 1)]
                early = True
            elif xs.shape[1:] == xu.shape[1:]:
                # one pass over [labeled crops ; unlabeled student view]; the two forwards consume their slice of the pyramid
                pyr = self.student.backbone(torch.cat([xs, xu], 0))
                n = xs.shape[0]
                parts = [fused.split_batch(l, n) for l in pyr]
                feats_s = tuple(p[0] for p in parts)
                feats_u = [tuple(p[1] for p in parts)]
                if self.early_sup_backward:
                    # graph cut at the pyramid: the heads run backward per branch (the supervised ones before the teacher
                    # is back), backbone + FPN once on the two slices' gradients together
                    roots = feats_s + feats_u[0]
                    feats_s = tuple(t.detach().requires_grad_(True) for t in feats_s)
                    feats_u = [tuple(t.detach().requires_grad_(True) for t in feats_u[0])]
                    cut = (roots, feats_s + feats_u[0])
                    early = True
        if use_mt and self.overlap_teacher and job is None:
            job = self._start_teacher(data_u_list)
        try:
            self.scheduler.step()
            if early:
                self.optimizer.zero_grad()
            loss_dict = self.forward_source(data_s, target_s, feats_s)
            if early:
                # the supervised pass's weight gradients are collected while its backward is issued and go to the side stream in
                # one batch behind it (layers/fused.py), beside the consistency branch
                defer = use_mt and job is not None
                if defer:
                    fused.defer_wgrads(True)
                try:
                    self._backward_roots(loss_dict, iteration)
                    losses_dict = self._weighted_detached(loss_dict, iteration)   # (for the log: behind the backward's launches)
                finally:
                    if defer:
                        fused.defer_wgrads(False)
                        fused.flush_deferred_wgrads()   # one batch, behind the supervised backward, beside the consistency branch
                unl = self.forward_unlabel(data_u_list, feats_u, job)
                job = None
                if unl:
                    self._backward_roots(unl, iteration)
                    unl = self._weighted_detached(unl, iteration)
                losses_dict.update(unl)
                self._pad_mt_keys(losses_dict)
                if cut is not None:
                    pairs = [(r, l.grad) for r, l in zip(*cut) if l.grad is not None]
                    torch.autograd.backward([r for r, _ in pairs], [g for _, g in pairs])
            else:
                if use_mt:
                    unl = self.forward_unlabel(data_u_list, feats_u, job)
                    job = None
                    loss_dict.update(unl)
                losses_dict = self.weight_sum_loss(loss_dict, iteration)
                self.optimizer.zero_grad()
                sum(v for v in losses_dict.values()).backward()
                if use_mt:
                    self._pad_mt_keys(losses_dict)
        finally:
            if job is not None:  # an exception before the join: never leave the helper thread running on t_stream
                job["thread"].join()
                torch.cuda.current_stream().wait_stream(self.t_stream)
            if bucketed is not None:
                bucketed.finish()
        fused.join_wgrads()   # the weight gradients of this step (side stream) before anything reads the flat gradient
        if bucketed is None:
            allreduce_gradients(self.flat_s)
        sync_touched(self.flat_s)   # every step: a degenerate route on one rank touches another set than its peers'
        # the previous step's EMA reads the student on the teacher's stream: SGD must not overwrite it first.  On a mean-teacher step
        # forward_unlabel's join has ordered the two already; before START_MT (and with no unlabeled batch) nothing else does
        self.sync_teacher()
        self.optimizer.step()
        # round 6: every launch of the step is ordered in front of this point (teacher joined, weight-gradient stream joined): the
        # producing sites' maxima of this step become their plane scales for the next one (_hip.rb_scales_update, one launch)
        H.rb_scales_update()
        if self.lambda_value > 0 and iteration > (self.start_mt - 10):
            self.update_teacher(iteration - (self.start_mt - 10))
            if self.teacher_check_period > 0 and iteration % self.teacher_check_period == 0:
                self.sync_teacher()
                check_teacher_identity(self.flat_t)
        self.last_iteration = iteration
        return losses_dict

    def _pad_mt_keys(self, losses):
        """A rank whose teacher found no boxes skips the consistency branch (reference: bare except, MTtrainer.py:258-265)
        and has no mt_* losses this step; the logging reduce (reduce_loss_dict) stacks the values of every key, so all
        ranks must carry the same keys: the skipped ones are reported as zeros (in place)."""
        for k, on in (("mt_fg_loss", self.cfg.MT.FG_HINT), ("mt_classifier", self.cfg.MT.CLS_LOSS)):
            if on and k not in losses:
                losses[k] = next(iter(losses.values())).detach().new_zeros(())
        return losses

    def _bucketed_allreduce(self):
        """the overlapped exchange, when there is somebody to exchange with"""
        # MMT_BUCKETED_ALLREDUCE=0 falls back to the single all-reduce after backward.  (With RCCL at world size 1 the two
        # cost the same, 59.6 vs 60.2 ms/step; what the overlap buys at 2..8 GPUs is the xGMI time of ~3/4 of the 176 MB.)
        if not (dist.is_available() and dist.is_initialized()) or os.environ.get("MMT_BUCKETED_ALLREDUCE", "1") == "0":
            return None
        if self._bucketed is None:
            self._bucketed = BucketedAllReduce(self.flat_s, self.student.backbone.body)
        return self._bucketed

    def train(self):
        self.student.train()
        self.teacher.eval()
        t0 = time.time()
        for iteration, (data_s, target_s, _) in enumerate(self.dataloader_s, self.start_iter):
            data_u = None
            if iteration > self.start_mt and self.lambda_value > 0 and self.dataloader_u is not None:
                data_u = self._next_unlabeled()
            losses_dict = self.train_step(iteration, data_s, target_s, data_u)
            if iteration % 20 == 0 or iteration == self.max_iter:
                red = reduce_loss_dict(losses_dict)
                guard = self._guard_report()   # (here, where the log line synchronises anyway: the guard's one read-back)
                self.logger.info("iter: %d  %s  lr: %.6f  max mem: %.0f%s", iteration,
                                 "  ".join("%s: %.4f" % (k, float(v)) for k, v in red.items()),
                                 self.optimizer.param_groups[0]["lr"], torch.cuda.max_memory_allocated() / 2 ** 20, guard)
            if self.ckpt_s is not None and iteration > 0 and iteration % self.checkpoint_period == 0:
                self.save_model(iteration)
        self.logger.info("Total training time: %.1f s", time.time() - t0)

    def _guard_report(self):
        """the guarded optimiser's part of the log line ("" with the guard off); raises once the run has skipped
        MAX_CONSECUTIVE_SKIPS steps in a row: every gradient since then was non-finite, and the weights have not moved.  The same
        on every rank: the verdicts come from the all-reduced gradient."""
        if getattr(self.optimizer, "guard", None) is None:
            return ""
        st = self.optimizer.guard_stats()
        limit = self.optimizer.guard["max_consecutive_skips"]
        if st["consecutive"] >= limit:
            raise RuntimeError("the last %d optimiser steps in a row were skipped for a non-finite gradient (SOLVER.GRAD_GUARD."
                               "MAX_CONSECUTIVE_SKIPS %d; %d of %d steps skipped in all): the run has diverged -- resume from a "
                               "checkpoint with a lower learning rate or a SOLVER.GRAD_GUARD.MAX_NORM"
                               % (st["consecutive"], limit, st["skipped"], st["seen"]))
        return "  grad_norm: %.4f  skipped: %d  clipped: %d" % (st["norm"], st["skipped"], st["clipped"])

    def _next_unlabeled(self):
        if self._unl_iter is None:
            skip, self._unl_skip = self._unl_skip, 0
            if skip and hasattr(self.dataloader_u, "fast_forward"):
                self.dataloader_u.fast_forward(skip)   # (a loader that can seek: told before it is iterated)
                skip = 0
            self._unl_iter = iter(self.dataloader_u)
            for _ in range(skip):                      # after a resume: where the interrupted run stood in the loader's current pass
                next(self._unl_iter)
        try:
            batch = next(self._unl_iter)[0]
        except StopIteration:
            self._unl_iter = iter(self.dataloader_u)
            batch = next(self._unl_iter)[0]
        self.unlabeled_seen += 1
        return batch

    def save_model(self, iteration=0, final=False):
        """the student's checkpoint (the reference's layout: model / optimizer / scheduler) with two extra entries, `iteration` and
        `trainer` (`state_dict`: everything `resume` needs); the teacher's own file as before.  Deterministic mode: the checkpoint is
        a restart point -- the adaptive arithmetic state is dropped once the file is written, so the step after it starts from what a
        resumed process starts from."""
        self.sync_teacher()
        name = "model_final" if final else "model_{:07d}".format(iteration)
        extra = {"iteration": iteration, "trainer": self.state_dict(iteration)}
        if getattr(self.ckpt_s, "optimizer", None) is self.optimizer:
            # the file's own `optimizer` / `scheduler` entries are the same objects: the momentum is stored once
            extra["optimizer"], extra["scheduler"] = extra["trainer"]["optimizer"], extra["trainer"]["scheduler"]
        self.ckpt_s.save(name, **extra)
        if iteration > self.start_mt and self.ckpt_t is not None:
            self.ckpt_t.save("t_" + name)
        if H.get_deterministic():
            H.reset_adaptive_state()
            self._forget_stem_forms()

    # ---- checkpoints as restart points
    def _forget_stem_forms(self):
        """the stems' cached space-to-depth filters and their planes are made again from the weights as they are NOW.  A frozen stem
        caches them by the parameter's version alone, and the EMA rewrites the teacher's whole flat buffer through raw pointers -- the
        frozen region too, where alpha t + (1 - alpha) s with t == s still rounds: the teacher's filter bytes drift by an ulp now and
        then while its cached form keeps the values of its first use.  A resumed process derives the form from the saved bytes, so a
        restart point makes the continuing run do the same."""
        for model in (self.student, self.teacher):
            stem = getattr(getattr(getattr(model, "backbone", None), "body", None), "stem", None)
            if stem is not None:
                stem._s2d_key = None
    def rng_state(self):
        """the six random streams a step can draw from, as CPU tensors and plain values: the student's and the teacher's device
        generators, torch's CPU generator, the current device's default generator, Python's `random`, `numpy.random`"""
        name, keys, pos, has_gauss, cached = np.random.get_state()
        version, words, gauss = random.getstate()
        on_device = self.device.type == "cuda"
        return {"gen_s": self.gen_s.get_state() if self.gen_s is not None else None,
                "gen_t": self.gen_t.get_state() if self.gen_t is not None else None,
                "torch_cpu": torch.get_rng_state(),
                "torch_device": torch.cuda.get_rng_state(self.device) if on_device else None,
                "python": [int(version), [int(w) for w in words], gauss],
                "numpy": {"name": str(name), "keys": torch.from_numpy(keys.astype(np.int64)), "pos": int(pos),
                          "has_gauss": int(has_gauss), "cached_gaussian": float(cached)}}

    def set_rng_state(self, state):
        """`rng_state` restored; a stream the saving process did not have (no device) is left alone"""
        if state.get("gen_s") is not None and self.gen_s is not None:
            self.gen_s.set_state(state["gen_s"])
            self.gen_t.set_state(state["gen_t"])
        torch.set_rng_state(state["torch_cpu"])
        if state.get("torch_device") is not None and self.device.type == "cuda":
            torch.cuda.set_rng_state(state["torch_device"], self.device)
        version, words, gauss = state["python"]
        random.setstate((version, tuple(words), gauss))
        n = state["numpy"]
        np.random.set_state((n["name"], n["keys"].numpy().astype(np.uint32), n["pos"], n["has_gauss"], n["cached_gaussian"]))

    def state_dict(self, iteration=None):
        """what `save_model` stores under `trainer` (plain values and CPU tensors): the whole run state that is not the student's
        `model` entry.  iteration: the last completed one (default: the last `train_step`'s).  Collective when torch.distributed is
        initialised: every rank's random streams are gathered, one entry per rank."""
        self.sync_teacher()
        rng = [self.rng_state()]
        if dist.is_available() and dist.is_initialized():
            rng = [None] * dist.get_world_size()
            dist.all_gather_object(rng, self.rng_state())
        teacher = self.teacher.state_dict()
        return {"format": RESUME_FORMAT,
                "iteration": int(self.last_iteration if iteration is None else iteration),
                "optimizer": self.optimizer.state_dict(),
                "scheduler": self.scheduler.state_dict(),
                "teacher": type(teacher)((k, v.detach().cpu()) for k, v in teacher.items()),
                "rng": rng,
                "unlabeled_seen": int(self.unlabeled_seen),
                "skipped_pairs": int(self.skipped_pairs),
                "world_size": get_world_size(),
                "deterministic": bool(H.get_deterministic()),
                "checksums": self.checksums()}

    def checksums(self):
        """`teacher_checksum` of the student's flat buffer, its momentum buffer and the teacher's flat buffer, as Python ints"""
        self.sync_teacher()
        return {"student": _word_sum(self.flat_s.data), "momentum": _word_sum(self.flat_s.momentum),
                "teacher": _word_sum(self.flat_t.data)}

    def resume(self, f=None):
        """continue the run a `save_model` file was written by: student, teacher, momentum, schedule, random streams and counters as
        they were after the saved iteration -> that iteration (`start_iter` is one more).  f: the file; default: the `last_checkpoint`
        of the student checkpointer's directory.  Refuses what it cannot restore exactly ("Resuming a run").  The
        labeled loader is the caller's to position at `start_iter`; the unlabeled one is fast-forwarded on first use."""
        if f is None:
            f = self.ckpt_s.get_checkpoint_file() if self.ckpt_s is not None and self.ckpt_s.has_checkpoint() else None
            if not f:
                raise FileNotFoundError("resume: no last_checkpoint in %r" % (getattr(self.ckpt_s, "save_dir", None),))
            # both checkpointers writing into one directory: past START_MT the tag names the teacher's t_<name> file, written second
            d, base = os.path.split(f)
            if base.startswith("t_") and os.path.isfile(os.path.join(d, base[2:])):
                f = os.path.join(d, base[2:])
        if not os.path.isfile(f):
            raise FileNotFoundError("resume: no checkpoint file %r" % (f,))
        ckpt = torch.load(f, map_location=torch.device("cpu"))
        tr = ckpt.get("trainer") if isinstance(ckpt, dict) else None
        if not isinstance(tr, dict) or "model" not in ckpt:
            raise ValueError("resume: %s has no `trainer` entry -- a checkpoint of the reference, or one written before runs could be "
                             "resumed, holds the weights only: load those with Checkpointer.load and start at iteration 0" % f)
        if tr.get("format") != RESUME_FORMAT:
            raise ValueError("resume: %s holds trainer format %r, this build reads format %d" % (f, tr.get("format"), RESUME_FORMAT))
        # names and shapes, every mismatch in one message, before anything is written
        model_sd = strip_prefix_if_present(ckpt["model"], prefix="module.")
        teacher_sd = strip_prefix_if_present(tr["teacher"], prefix="module.")
        named = dict(self.flat_s._named)
        shape = lambda d: {k: tuple(v.shape) for k, v in d.items()}
        bad = _name_problems("student", shape(model_sd), shape(strip_prefix_if_present(self.student.state_dict(), "module.")))
        bad += _name_problems("teacher", shape(teacher_sd), shape(strip_prefix_if_present(self.teacher.state_dict(), "module.")))
        bad += _name_problems("momentum", shape(tr["optimizer"].get("momentum_buffers", {})),
                              {n: tuple(named[n].shape) for n, (o, _) in self.flat_s.index.items() if o < self.flat_s.n_trainable})
        if bad:
            raise ValueError("resume: %s does not fit this trainer:\n  %s" % (f, "\n  ".join(bad)))
        if tr["world_size"] != get_world_size():
            raise RuntimeError("resume: %s was written at world size %d, this run has %d (the per-rank random streams and the data "
                               "split do not carry over)" % (f, tr["world_size"], get_world_size()))
        if bool(tr["deterministic"]) != bool(H.get_deterministic()):
            self.logger.warning("resume: %s was saved with deterministic mode %s and is resumed with it %s: the bit-for-bit guarantee "
                                "does not apply to this run", f, "on" if tr["deterministic"] else "off",
                                "on" if H.get_deterministic() else "off")
        self.sync_teacher()
        load_state_dict(self.student, model_sd)
        load_state_dict(self.teacher, teacher_sd)
        self.optimizer.load_state_dict(tr["optimizer"])
        self.scheduler.load_state_dict(tr["scheduler"])
        self.optimizer.lr_factor = float(tr["optimizer"]["lr_factor"])
        self.optimizer.param_groups[0]["lr"] = self.optimizer.base_lr * self.optimizer.lr_factor
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.set_rng_state(tr["rng"][rank])
        self.unlabeled_seen, self.skipped_pairs = int(tr["unlabeled_seen"]), int(tr["skipped_pairs"])
        self._unl_iter = None
        n_unl = len(self.dataloader_u) if hasattr(self.dataloader_u, "__len__") else 0   # (no unlabeled loader, or one without a length)
        self._unl_skip = self.unlabeled_seen % n_unl if n_unl else 0
        self.last_iteration = int(tr["iteration"])
        self.start_iter = self.last_iteration + 1
        # everything made from weights, again: packed planes of both buffers, what the models derive, the stem's cached filter forms
        for model, flat in ((self.student, self.flat_s), (self.teacher, self.flat_t)):
            flat.refresh_planes()
            refresh_derived(model)
        self._forget_stem_forms()
        # ... and nothing an earlier life of this process learnt about tensor ranges: a resumed run starts where a fresh process does
        H.reset_adaptive_state()
        got = self.checksums()
        for k in ("student", "momentum", "teacher"):
            if got[k] != int(tr["checksums"][k]):
                raise RuntimeError("resume: the restored %s buffer does not match %s (checksum %d, saved %d)"
                                   % (k, f, got[k], int(tr["checksums"][k])))
        self.logger.info("resumed from %s: iteration %d, %d unlabeled batches seen", f, self.last_iteration, self.unlabeled_seen)
        return self.last_iteration

    def forward_source(self, image, target, features=None):
        return self.student(image.to(self.device), [t.to(self.device) for t in target], features=features)

    def forward_only(self, data_s, target_s, data_u_list):
        """the three FORWARDS of one iteration and nothing else, without autograd, on the current stream: [A] supervised student
        forward with its losses, [B] the teacher's pseudo labels + K-aug x flip pyramids, [C] the student's consistency losses on
        the unlabeled view -- 2 + 8 + 2 = 12 image-forwards through the backbone at the bench's batch.  What BASELINE.json's
        north_star quotes its 0.5-of-roofline target on (bench.py: forward_leg); results are not used for training."""
        with torch.no_grad():
            out = dict(self.forward_source(data_s, target_s))
            out.update(self.forward_unlabel(data_u_list, None, None))
        return out

    def _loss_coeff(self, k, w):
        return (w if "mt" in k else 1.0) * (self.balanced_weight[k] if k in self.balanced_weight else 1.0)

    def _weighted_detached(self, loss_dict, iteration):
        """the weighted losses of `weight_sum_losses` as detached values (what a step returns for the log), in one multi-tensor launch"""
        w = mt_weight(iteration, self.cfg.MT.RAMPUP_STEP, self.cfg.MT.RAMPDOWN_STEP, self.max_iter, self.lambda_value, self.start_mt)
        keys = [k for k, v in loss_dict.items() if torch.is_tensor(v)]
        out = {k: v for k, v in loss_dict.items() if not torch.is_tensor(v)}
        if keys:
            vals = torch._foreach_mul([loss_dict[k].detach() for k in keys], [float(self._loss_coeff(k, w)) for k in keys])
            out.update(zip(keys, vals))
        return {k: out[k] for k in loss_dict}

    def _backward_roots(self, loss_dict, iteration):
        """backward of sum_k c_k loss_k (c_k = the weights of `weight_sum_losses`, MTtrainer.py:67-109) WITHOUT forming the sum: the
        losses are the roots, the weights their seed gradients.  `sum(weighted.values()).backward()` put ~20 scalar launches (the
        weighting multiplies, the chain of adds, their backward nodes) in front of the first kernel of each backward pass -- on the
        step's critical chain, at a point where the host is not ahead of the device."""
        w = mt_weight(iteration, self.cfg.MT.RAMPUP_STEP, self.cfg.MT.RAMPDOWN_STEP, self.max_iter, self.lambda_value, self.start_mt)
        roots, seeds = [], []
        cache = self.__dict__.setdefault("_seed_cache", {})
        for k, v in loss_dict.items():
            if not (torch.is_tensor(v) and v.requires_grad):
                continue
            c = self._loss_coeff(k, w)
            key = (float(c), v.dtype, v.device, tuple(v.shape))
            t = cache.get(key)
            if t is None:
                if len(cache) > 64:
                    cache.clear()
                t = cache[key] = torch.full(v.shape, float(c), dtype=v.dtype, device=v.device)
            roots.append(v)
            seeds.append(t)
        if roots:
            torch.autograd.backward(roots, seeds)

    def _start_teacher(self, data_u_list):
        """launch teacher.forward_teacher on the side stream from a helper thread; -> job dict (joined in forward_unlabel)"""
        import threading
        teacher_list = [f.to(self.device) for f in data_u_list[:self.teacher_bs]]
        # EMA / weight packing of the previous step, inputs.  (Round 4: letting the side stream start behind the step's FIRST launch
        # instead -- the teacher's N = 8 kernels then run beside the student's N = 4 forward -- was measured SLOWER, medians 38.1 /
        # 38.7 vs 37.6 / 36.1 ms on one box: the student's chain is the critical path and the high-priority side stream starves it.)
        self.t_stream.wait_stream(torch.cuda.current_stream())
        job = {}

        def run():
            try:
                torch.cuda.set_device(self.device)
                with torch.cuda.stream(self.t_stream), torch.no_grad():
                    job["result"] = self.teacher.forward_teacher(teacher_list)
            except BaseException as e:  # re-raised (or handled) by the step thread
                job["error"] = e

        job["thread"] = threading.Thread(target=run, name="mmt-teacher", daemon=True)
        job["thread"].start()
        return job

    def _student_views(self, data_u_list):
        """AUG_S > 1: the last AUG_S views of the unlabeled batch as one batch, odd views mirrored (generalized_rcnn.py:209-214) --
        the input of the step's student passes; None when the views' shapes differ (forward_student then runs them one by one)"""
        views = [u.tensors for u in data_u_list[-self.student_bs:]]
        if any(v.shape != views[0].shape for v in views):
            return None
        views = [v.to(self.device) for v in views]
        return torch.cat([torch.flip(v, (3,)) if j % 2 == 1 else v for j, v in enumerate(views)], 0)

    def forward_unlabel(self, data_u_list, features=None, job=None):
        """MTtrainer.py:247-275 (N_STEP_UNLABEL = 1)"""
        student = [s.to(self.device) for s in data_u_list[-self.student_bs:]]
        emb = None
        if features is not None and len(features) == 1 and len(student) > 1:
            # AUG_S > 1: features[0] is ONE pyramid over the S views (the step's student pass); forked as below when both consistency
            # losses consume it, the hint adaptor runs once over the batched levels, the box head too (forward_student)
            f_emb = f_box = features[0]
            if self.cfg.MT.FG_HINT and self.cfg.MT.CLS_LOSS and torch.is_grad_enabled():
                f_emb, f_box = fused.fork_levels(features[0], 2)
            n = f_box[0].shape[0] // len(student)
            if self.cfg.MT.FG_HINT:
                emb = self.student.get_emb_feature(self.student.view_slices(f_emb, n, len(student)))
            features = self.student.view_slices(f_box, n, len(student))
            f_emb = None
        elif features is not None and len(features) == 1 and self.cfg.MT.FG_HINT and self.cfg.MT.CLS_LOSS and torch.is_grad_enabled():
            # two consumers of every pyramid level (hint adaptor, box pooler): their gradients are summed in one launch
            f_emb, f_box = fused.fork_levels(features[0], 2)
            if job is None:
                emb = self.student.get_emb_feature([f_emb])
            features, f_emb = [f_box], [f_emb]
        else:
            f_emb = features
        if job is not None and features is not None and self.cfg.MT.FG_HINT and emb is None:
            emb = self.student.get_emb_feature(f_emb)  # independent of the teacher: queued before the wait
        try:
            if job is not None:
                job["thread"].join()
                # everything the teacher produced is read on this stream from here on.  (The side stream IS used again in this
                # step: update_teacher queues the EMA and the teacher's plane re-pack there -- behind the step stream -- and the
                # next step's SGD waits for them through sync_teacher.)  This join also covers an EMA still pending from the last step
                torch.cuda.current_stream().wait_stream(self.t_stream)
                self._teacher_pending = False
                if "error" in job:
                    raise job["error"]
                teacher_results = job["result"]
            else:
                self.sync_teacher()
                teacher_list = [f.to(self.device) for f in data_u_list[:self.teacher_bs]]
                with torch.no_grad():
                    teacher_results = self.teacher.forward_teacher(teacher_list)
        except ValueError as e:  # no pseudo boxes for an image: the reference skips the pair (bare except)
            self.logger.info("teacher produced no boxes (%s), skip this pair", e)
            self.skipped_pairs += 1
            return {}
        return self.student.forward_student(student, teacher_results, features=features, embeddings=emb)

    def update_teacher(self, it):
        """MTtrainer.py:277-281 as one launch over the flat parameter buffers.  With the teacher on its own stream the update and
        the re-packing of the teacher's weight planes run THERE (round 4): nothing on the step stream reads the teacher before the
        next `_start_teacher`, which orders the side stream behind the step stream anyway, so the next step's student forward no
        longer queues behind ~0.3 ms of full-chip HBM passes.  Whoever reads the teacher from outside a step (checkpoints, the
        identity check, tests) goes through `sync_teacher()` or a device-wide synchronize."""
        alpha = min(1 - 1 / (it + 1), self.alpha)
        if self.t_stream is not None and self.overlap_teacher:
            self.t_stream.wait_stream(torch.cuda.current_stream())     # the student's SGD step
            with torch.cuda.stream(self.t_stream):
                H.ema_update(self.flat_t.data, self.flat_s.data, alpha)
                self.flat_t.refresh_planes()
            self._teacher_pending = True
            return
        H.ema_update(self.flat_t.data, self.flat_s.data, alpha)
        self.flat_t.refresh_planes()

    def sync_teacher(self):
        """the step stream waits for a teacher update still queued on the teacher's stream"""
        if getattr(self, "_teacher_pending", False):
            torch.cuda.current_stream().wait_stream(self.t_stream)
            self._teacher_pending = False
