"""Graph-based depth correction without a GPU: the calibration reader, the no-CPU-fallback rule, the driver's command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_calibration_reads_cam_to_cam(tmp_path):
    from fusiondepth_amd.kitti_utils import Calibration
    P2 = [721.5377, 0.0, 609.5593, 44.85728, 0.0, 721.5377, 172.854, 0.2163791, 0.0, 0.0, 1.0, 0.002745884]
    P3 = [721.5377, 0.0, 609.5593, -339.5242, 0.0, 721.5377, 172.854, 2.199936, 0.0, 0.0, 1.0, 0.002729905]
    R0 = [0.9999239, 0.00983776, -0.007445048, -0.009869795, 0.9999421, -0.004278459, 0.007402527, 0.004351614, 0.9999631]
    text = "calib_time: 09-Jan-2012 13:57:47\ncorner_dist: 9.950000e-02\nR_rect_00: %s\nP_rect_02: %s\nP_rect_03: %s\n" % (
        " ".join(map(repr, R0)), " ".join(map(repr, P2)), " ".join(map(repr, P3)))
    path = tmp_path / "calib_cam_to_cam.txt"
    path.write_text(text)
    c = Calibration(str(path))
    assert (c.c_u, c.c_v, c.f_u, c.f_v) == (609.5593, 172.854, 721.5377, 721.5377)
    assert c.b_x == 44.85728 / -721.5377 and c.b_y == 0.2163791 / -721.5377
    assert c.baseline == -339.5242 / -721.5377 - 44.85728 / -721.5377
    assert abs(c.baseline - 0.5327) < 1e-3
    np.testing.assert_array_equal(c.P, np.array(P2).reshape(3, 4))
    np.testing.assert_array_equal(c.R0, np.array(R0).reshape(3, 3))


def test_gdc_refuses_cpu_tensors():
    from fusiondepth_amd.gdc import GDC
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cam = type("Cam", (), dict(c_u=609.5, c_v=172.8, f_u=721.5, f_v=721.5, b_x=-0.06, b_y=0.0))()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GDC(torch.ones(8, 8), -torch.ones(8, 8, dtype=torch.float64), cam, method="cg")


def test_inf_gdc_help_parses():
    r = subprocess.run([sys.executable, "-m", "fusiondepth_amd.inf_gdc", "--help"], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    for flag in ("--data_path", "--split_files", "--nbeams", "--random_sample"):
        assert flag in r.stdout
    from fusiondepth_amd import inf_gdc
    a = inf_gdc.parse_args([])
    assert a.split_files == list(inf_gdc.DEFAULT_SPLITS) and a.nbeams == 4 and a.random_sample == -1
