"""The guarded optimiser step without a device: the SOLVER.GRAD_GUARD keys, what `make_optimizer` does with them, and the host half
of the guard's state (`FlatSGD.state_dict` / `load_state_dict`, engine/MTtrainer.py's report and its give-up rule) on CPU tensors.
The kernels and the training step are tests/test_grad_guard_gpu.py's."""
import pytest
import torch


def _cfg(*pairs):
    from maskrcnn_benchmark.config import make_default_cfg
    cfg = make_default_cfg()
    if pairs:
        cfg.merge_from_list(list(pairs))
    return cfg


@pytest.fixture(scope="module")
def model():
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    return build_detection_model(_cfg(), is_student=True)


def test_the_three_keys_and_their_defaults():
    g = _cfg().SOLVER.GRAD_GUARD
    assert dict(g) == {"ENABLED": False, "MAX_NORM": 0.0, "MAX_CONSECUTIVE_SKIPS": 50}
    assert g.ENABLED is False and isinstance(g.MAX_NORM, float) and isinstance(g.MAX_CONSECUTIVE_SKIPS, int)


def test_merge_from_list_sets_them():
    g = _cfg("SOLVER.GRAD_GUARD.ENABLED", True, "SOLVER.GRAD_GUARD.MAX_NORM", 35.0, "SOLVER.GRAD_GUARD.MAX_CONSECUTIVE_SKIPS", 7).SOLVER.GRAD_GUARD
    assert dict(g) == {"ENABLED": True, "MAX_NORM": 35.0, "MAX_CONSECUTIVE_SKIPS": 7}
    # a command line hands strings over
    g = _cfg("SOLVER.GRAD_GUARD.ENABLED", "True", "SOLVER.GRAD_GUARD.MAX_NORM", "2.5", "SOLVER.GRAD_GUARD.MAX_CONSECUTIVE_SKIPS", "3").SOLVER.GRAD_GUARD
    assert g.ENABLED is True and g.MAX_NORM == 2.5 and g.MAX_CONSECUTIVE_SKIPS == 3 and isinstance(g.MAX_CONSECUTIVE_SKIPS, int)
    assert _cfg().SOLVER.GRAD_GUARD.ENABLED is False     # (the defaults are not shared between configurations)


def test_the_default_models_state_dict_is_unchanged(model, state_shapes):
    sd = model.state_dict()
    ref = state_shapes["shapes"]
    assert sorted(sd) == sorted(ref) and all(list(v.shape) == ref[k] for k, v in sd.items())
    assert [k for k, _ in model.named_parameters()] == state_shapes["param_order"]


def test_make_optimizer_follows_the_configuration(model):
    from maskrcnn_benchmark import _hip as H
    from maskrcnn_benchmark.solver import make_optimizer
    opt = make_optimizer(_cfg(), model)
    assert opt.guard is None and "guard" not in opt.state_dict()          # off: the checkpoint entry is what it always was
    with pytest.raises(RuntimeError):
        opt.guard_stats()
    opt = make_optimizer(_cfg("SOLVER.GRAD_GUARD.ENABLED", True, "SOLVER.GRAD_GUARD.MAX_NORM", 10.0), model)
    assert opt.guard["max_norm"] == 10.0 and opt.guard["max_consecutive_skips"] == 50
    state, ws = opt.guard["state"], opt.guard["ws"]
    assert state.dtype == torch.float32 and state.numel() == H.GRAD_GUARD_STATE_WORDS and not state.any()
    assert ws.dtype == torch.float64 and ws.numel() == H.GRAD_GUARD_WS
    assert opt.guard_stats() == {"norm": 0.0, "seen": 0, "skipped": 0, "clipped": 0, "consecutive": 0}
    opt.enable_guard(max_norm=0.0, max_consecutive_skips=2)                # again: new thresholds, the same buffers
    assert opt.guard["state"] is state and opt.guard["ws"] is ws and opt.guard["max_norm"] == 0.0
    for bad in (dict(max_norm=-1.0), dict(max_norm=float("nan")), dict(max_consecutive_skips=0)):
        with pytest.raises(ValueError):
            opt.enable_guard(**bad)


def test_the_counters_travel_through_the_state_dict(model):
    from maskrcnn_benchmark import _hip as H
    from maskrcnn_benchmark.solver import make_optimizer
    on = ("SOLVER.GRAD_GUARD.ENABLED", True)
    a = make_optimizer(_cfg(*on), model)
    ints = a.guard["state"].view(torch.int32)
    ints[H.GUARD_SEEN], ints[H.GUARD_SKIPPED], ints[H.GUARD_CLIPPED], ints[H.GUARD_CONSECUTIVE] = 120, 4, 17, 2
    a.guard["state"][H.GUARD_NORM] = 3.5
    sd = a.state_dict()
    assert sd["guard"] == {"norm": 3.5, "seen": 120, "skipped": 4, "clipped": 17, "consecutive": 2, "max_norm": 0.0,
                           "max_consecutive_skips": 50}
    b = make_optimizer(_cfg(*on, "SOLVER.GRAD_GUARD.MAX_NORM", 5.0), model)
    b.load_state_dict(sd)
    got = b.guard_stats()
    assert (got["seen"], got["skipped"], got["clipped"], got["consecutive"]) == (120, 4, 17, 2)
    assert b.guard["max_norm"] == 5.0                                      # the thresholds are this run's configuration
    without = {k: v for k, v in sd.items() if k != "guard"}
    b.load_state_dict(without)                                             # a file written with the guard off: counters stay
    assert b.guard_stats()["seen"] == 120
    off = make_optimizer(_cfg(), model)
    off.load_state_dict(sd)                                                # ... and a guarded file into an unguarded run
    assert off.guard is None and "guard" not in off.state_dict()


class _Opt(object):
    def __init__(self, guard, stats=None):
        self.guard, self._stats = guard, stats

    def guard_stats(self):
        return dict(self._stats)


def test_the_trainers_report_and_its_limit():
    from maskrcnn_benchmark.engine.MTtrainer import MTtrainer
    t = MTtrainer.__new__(MTtrainer)
    t.optimizer = _Opt(None)
    assert t._guard_report() == ""                                          # off: the log line is today's
    stats = {"norm": 12.25, "seen": 40, "skipped": 3, "clipped": 5, "consecutive": 1}
    t.optimizer = _Opt({"max_consecutive_skips": 2}, stats)
    assert t._guard_report() == "  grad_norm: 12.2500  skipped: 3  clipped: 5"
    t.optimizer = _Opt({"max_consecutive_skips": 2}, dict(stats, consecutive=2, norm=float("nan")))
    with pytest.raises(RuntimeError, match="MAX_CONSECUTIVE_SKIPS 2"):
        t._guard_report()
