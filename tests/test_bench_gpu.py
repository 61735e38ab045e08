"""bench.py's plain run: the headline line with the number of timed steps asked for, none of the --full legs, and
--dump-outputs writing what the last timed step computed (float32 .npy files, bounded in size)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    d = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "imgs/sec" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 4 * 1e3 / out["ms_per_step"]) < 1e-2 * out["value"]   # 4 crops per step, one GPU
    assert not {"roofline", "forward_leg", "fp32_mfma_mode", "cpu_baseline"} & set(out), sorted(out)
    files = {f: np.load(str(d / f)) for f in os.listdir(str(d))}
    losses = out["config"]["losses"]
    assert set(files) == {k + ".npy" for k in losses} | {"student_grad.npy", "student_params.npy", "teacher_params.npy"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert sum(os.path.getsize(str(d / f)) for f in files) <= 64 << 20
    for k, v in losses.items():   # the dumped losses are the ones the line reports
        assert float(files[k + ".npy"]) == pytest.approx(v, abs=1e-5), k
    assert np.abs(files["student_grad.npy"]).max() > 0
