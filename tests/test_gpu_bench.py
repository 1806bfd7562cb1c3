"""bench.py on one GPU: a plain run times exactly --steps steps and carries none of --full's extras, and --dump-outputs writes
what the last timed step computed - the same arrays, bit for bit, whenever the arguments are the same (every kernel of the step
is deterministic, tests/test_gpu_trainer.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--height", "64", "--width", "96", "--batch_size", "2"]


def _bench(extra, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_lean_and_its_dump_repeats(tmp_path):
    a = _bench(["--dump-outputs", str(tmp_path / "a")])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in a, key
    assert a["steps"] == 3 and a["windows"]["n"] == 1 and a["ms_per_step"] > 0
    assert a["optimizer_steps_run"] == 6 + 1 + 3, a["optimizer_steps_run"]      # 6 settling steps, --warmup 1, --steps 3
    for key in ("roofline", "roofline_loss_path", "other_configs", "cpu_baseline", "cpu_baseline_1thread", "abs_rel_heldout_scene"):
        assert key not in a, key
    b = _bench(["--dump-outputs", str(tmp_path / "b")])
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    for want in ("loss.npy", "disp_0.npy", "disp_3.npy", "cam_T_cam_0_-1.npy", "cam_T_cam_0_1.npy", "params.npy"):
        assert want in names, (want, names)
    total = 0
    for n in names:
        x, y = np.load(str(tmp_path / "a" / n)), np.load(str(tmp_path / "b" / n))
        assert x.dtype == np.float32 and x.size > 0, n
        assert np.array_equal(x, y, equal_nan=True), "%s differs between two runs with the same arguments" % n
        total += x.nbytes
    assert total <= 64 << 20
    assert np.isfinite(np.load(str(tmp_path / "a" / "params.npy"))).all()
    assert float(np.load(str(tmp_path / "a" / "loss.npy"))) == a["final_loss"]
    assert a["param_checksum"] == b["param_checksum"]
