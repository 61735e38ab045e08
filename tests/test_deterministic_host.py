"""Deterministic mode, host side (no GPU): the switch, the environment variable, torch's own flag, and the frozen site test."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mmt-psm_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)


@pytest.fixture()
def hip():
    from maskrcnn_benchmark import _hip as H
    yield H
    H.set_deterministic(False)


def _import_with(env_value):
    env = dict(os.environ)
    env.pop("MMT_DETERMINISTIC", None)
    if env_value is not None:
        env["MMT_DETERMINISTIC"] = env_value
    env["PYTHONPATH"] = os.pathsep.join([PKG, ROOT])
    code = ("import torch; from maskrcnn_benchmark import _hip as H; "
            "print(int(H.get_deterministic()), int(torch.are_deterministic_algorithms_enabled()), H.lib().mmt_get_deterministic())")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout.split()[-3:]


def test_environment_variable_is_honoured_at_import():
    assert _import_with("1") == ["1", "1", "1"]       # the binding, torch, and the library (set when it is loaded)
    assert _import_with("0") == ["0", "0", "0"]
    assert _import_with(None) == ["0", "0", "0"]


def test_switch_round_trips_and_restores_torchs_flag(hip):
    H = hip
    from torch.utils import deterministic as td
    assert not H.get_deterministic() and H.lib().mmt_get_deterministic() == 0
    fill0 = td.fill_uninitialized_memory
    for found in ((False, False), (True, True), (True, False)):
        torch.use_deterministic_algorithms(found[0], warn_only=found[1])
        try:
            calls = H.C_CALLS[0]
            H.set_deterministic(True)
            H.set_deterministic(True)                       # (twice: what it found is what the FIRST switch found)
            assert H.get_deterministic() and H.lib().mmt_get_deterministic() == 1
            assert torch.are_deterministic_algorithms_enabled() and not torch.is_deterministic_algorithms_warn_only_enabled()
            H.set_deterministic(False)
            assert not H.get_deterministic() and H.lib().mmt_get_deterministic() == 0
            assert (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()) == found
            assert td.fill_uninitialized_memory == fill0
            H.set_deterministic(False)                      # (off when off: nothing to restore)
            assert (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()) == found
            assert H.C_CALLS[0] == calls                    # a switch is not a launch: bench.py's calls per step do not count it
        finally:
            torch.use_deterministic_algorithms(False)


def test_bf16_storage_and_the_mode_exclude_each_other(hip):
    H = hip
    H.set_deterministic(True)
    with pytest.raises(NotImplementedError):
        H.set_bf16_storage(True)
    H.set_bf16_storage(False)
    H.set_deterministic(False)
    H.set_bf16_storage(True)
    try:
        with pytest.raises(NotImplementedError):
            H.set_deterministic(True)
        assert not H.get_deterministic() and not torch.are_deterministic_algorithms_enabled()
    finally:
        H.set_bf16_storage(False)


class _Event(object):
    def query(self):
        raise AssertionError("the lagged site test polled a statistics pool in deterministic mode")


class _Pool(object):
    """a statistics pool whose copy to the host is 'in flight': the default mode asks its event, the mode must not"""
    def __init__(self):
        self.gen = self.host_gen = 0
        self.event = _Event()


class _Pending(object):
    def __init__(self):
        self.pool, self.gen, self.idx = _Pool(), 0, 0


def test_site_test_is_frozen_in_the_mode(hip):
    H = hip
    x = torch.zeros(4)
    for state in (True, False):
        site = ("test-site", state)
        H._SITES[site] = [state, _Pending()]
        try:
            with pytest.raises(AssertionError):
                H._site_ok(site, x, count=False)            # the default mode polls
            H.set_deterministic(True)
            pend = H._SITES[site][1]
            assert H._site_ok(site, x, count=False) is state      # the site's current state, nothing polled ...
            assert H._SITES[site][1] is pend                      # ... nothing consumed or queued
            assert H._site_ok(("test-site", "new"), x, count=False) is True
            assert H._SITES[("test-site", "new")][1] is None
        finally:
            H.set_deterministic(False)
            H._SITES.pop(site, None)
            H._SITES.pop(("test-site", "new"), None)
