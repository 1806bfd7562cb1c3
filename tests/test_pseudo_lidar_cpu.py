"""The host side of the pseudo-LiDAR export: ``kitti_utils.rect_to_velo`` against the literal two-step chain of Pseudo-LiDAR's
``Calibration``, the point rule's restatement (tests/pseudo_lidar_ref.py) against the forward projection, its selection and order, the
path rule and the flags of ``export_detection``, and the boundary of the library (declared, exported, refused without a GPU)."""
import ctypes
import os

import numpy as np
import pytest

import kitti_tree
import pseudo_lidar_ref as PR

LIMIT = 1e-9                 # metres (and pixels): between float64 rounding noise (~1e-13 here) and float32 spacing at 80 m (7.6e-6)


def _fmt(a):
    return " ".join("%.17g" % v for v in np.asarray(a, dtype=np.float64).reshape(-1))


def _rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def _write_model_calib(d, im_h=375, im_w=1242):
    """A date folder that fulfils what the back-projection ASSUMES: rotations orthonormal to float64 rounding (the transpose stands for
    the inverse, kitti_util_from_pse.py's inverse_rigid_trans) and P_rect_02[2, 3] = 0 (``Calibration`` has no term for it).  KITTI's
    own files hold 7-digit values - orthonormal to 1e-7 only - and P[2, 3] = 0.0027; against those the round trip closes to the error
    of the model (1e-5 m, 1e-2 px), which says nothing about this code."""
    R = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]) @ _rot(2, 0.0075) @ _rot(1, 0.0148)
    R0 = _rot(0, 0.01) @ _rot(2, 0.005)
    P = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.0]])
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "calib_cam_to_cam.txt"), "w") as f:
        f.write("calib_time: 09-Jan-2012 13:57:47\nS_rect_02: %s\nR_rect_00: %s\nP_rect_02: %s\nP_rect_03: %s\n"
                % (_fmt([im_w, im_h]), _fmt(R0), _fmt(P), _fmt(P)))
    with open(os.path.join(d, "calib_velo_to_cam.txt"), "w") as f:
        f.write("R: %s\nT: %s\n" % (_fmt(R), _fmt([-4.069766e-03, -7.631618e-02, -2.717806e-01])))


def test_rect_to_velo_equals_the_two_step_chain(tmp_path):
    """project_rect_to_ref (inv(R0) @ p) then project_ref_to_velo ([p, 1] @ C2V.T, C2V = inverse_rigid_trans([R | T])), literally, on
    10 000 points up to 100 m.  Rounding noise is about 100 * 2^-52 * 10 = 2e-13 m."""
    from fusiondepth_amd import kitti_utils as KU
    d = str(tmp_path / "2011_09_26")
    kitti_tree.write_calib(d, 375, 1242)
    A, t = KU.rect_to_velo(d)
    assert A.shape == (3, 3) and t.shape == (3,) and A.dtype == t.dtype == np.float64
    intr, extr = KU.read_calib_file(os.path.join(d, "calib_cam_to_cam.txt")), KU.read_calib_file(os.path.join(d, "calib_velo_to_cam.txt"))
    R0, R, T = intr["R_rect_00"].reshape(3, 3), extr["R"].reshape(3, 3), extr["T"]
    C2V = np.zeros((3, 4))
    C2V[:, :3] = R.T
    C2V[:, 3] = np.dot(-R.T, T)
    rng = np.random.RandomState(1)
    p = rng.uniform(-100.0, 100.0, (10000, 3))
    ref = np.transpose(np.dot(np.linalg.inv(R0), np.transpose(p)))
    want = np.dot(np.hstack([ref, np.ones((len(ref), 1))]), np.transpose(C2V))
    got = p @ A.T + t
    err = np.abs(got - want).max()
    assert err < LIMIT, err
    assert np.abs(want).max() > 50.0


def test_restated_points_reproject_onto_their_pixels(tmp_path):
    """The geometry is right, not merely self-consistent: the unrounded points of the restatement, through ``velo_to_image``'s P
    (the FORWARD chain the rasteriser is tested with) and divided by depth, come back to (u, v, z)."""
    from fusiondepth_amd import kitti_utils as KU
    d = str(tmp_path / "model_date")
    _write_model_calib(d)
    calib = (KU.Calibration(os.path.join(d, "calib_cam_to_cam.txt")),) + KU.rect_to_velo(d)
    P, _ = KU.velo_to_image(d, 2)
    rng = np.random.RandomState(2)
    H, W = 6, 1242
    depth = rng.uniform(2.0, 80.0, (H, W)).astype(np.float32)
    X, Y, Z = PR.velo_coordinates(depth, calib)
    proj = np.stack([X, Y, Z, np.ones_like(X)], -1) @ P.T
    z = proj[..., 2]
    u, v = proj[..., 0] / z, proj[..., 1] / z
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    errs = [np.abs(u - uu).max(), np.abs(v - vv).max(), np.abs(z - depth.astype(np.float64)).max()]
    assert max(errs) < LIMIT, errs
    assert X.min() > 1.5 and np.abs(Y).max() > 20.0               # forward is +x of the Velodyne frame; the scene is wide


def test_selection_order_and_fourth_column():
    """A 2 x 3 map by hand: camera z -> Velodyne x, camera x -> -y, camera y -> -z; f = 1, c = (1, 0.5).  This pins the RESTATEMENT
    (it needs nothing of the package); tests/test_gpu_pseudo_lidar.py sends the same map through ``fd_points_export``."""
    depth, calib, by_hand = PR.hand_made_case()
    cloud, keep = PR.points(depth, calib)
    # (0,0): Z = 0.5 kept; (0,1): NaN; (0,2): Z = 1.0, not < 1; (1,0): X = -1 < 0; (1,1): Z = -1.5 kept; (1,2): X = 0 >= 0, Z = 0 kept
    assert keep.tolist() == [[True, False, False], [False, True, True]]
    assert cloud.dtype == np.float32 and cloud.shape == (3, 4)
    assert np.array_equal(cloud, by_hand)
    lower, _ = PR.points(depth, calib, max_high=0.5)              # Z < 0.5 drops the first point too
    assert np.array_equal(lower, cloud[1:])
    both, starts = PR.clouds([depth, np.full((1, 2), np.nan, np.float32), depth], [calib] * 3)
    assert starts.tolist() == [0, 3, 3, 6] and both[1].shape == (0, 4)


def test_path_rule():
    from fusiondepth_amd import export_detection as X
    assert X.bin_path("/data", "training 7 l", "pl") == os.path.join("/data", "training", "pl", "000007.bin")
    assert X.bin_path("root", "testing/a 123456 r", "clouds") == os.path.join("root", "testing/a", "clouds", "123456.bin")
    assert os.path.dirname(X.png_path("/data", "training 7 l", "pl")) == os.path.dirname(X.bin_path("/data", "training 7 l", "pl"))


def test_flags_are_taken_off_the_command_line(monkeypatch):
    """A command line without the new flags parses to the same call as before them: ``evaluate(opt, splits_dir)``, nothing else."""
    from fusiondepth_amd import export_detection as X
    from fusiondepth_amd.options import MonodepthOptions
    calls = []
    monkeypatch.setattr(X, "evaluate", lambda *a, **k: calls.append((a, k)))
    base = ["--eval_mono", "--det_name", "d", "--data_path", "kd"]
    X.main(["--splits_dir", "sp"] + base)
    X.main(base + ["--pl_name", "pl"])
    X.main(["--pl_max_high=0.25", "--splits_dir=s2"] + base + ["--pl_name=clouds"])
    want = vars(MonodepthOptions().parse(base))
    assert [len(a) for a, _ in calls] == [2, 2, 2] and all(vars(a[0]) == want for a, _ in calls)
    assert calls[0][0][1] == "sp" and calls[0][1] == {}
    assert calls[1][0][1] == "splits" and calls[1][1] == {"pl_name": "pl", "pl_max_high": 1.0}
    assert calls[2][0][1] == "s2" and calls[2][1] == {"pl_name": "clouds", "pl_max_high": 0.25}
    with pytest.raises(ValueError, match="pl_name"):
        X.main(base + ["--pl_name"])
    assert not hasattr(MonodepthOptions().parse(base), "pl_name")  # the options stay the reference's


@pytest.mark.parametrize("extra", [["--no_eval"], ["--eval_split", "benchmark"]])
def test_pl_name_is_refused_where_no_depth_is_scaled(monkeypatch, extra):
    import torch
    from fusiondepth_amd import export_detection as X
    from fusiondepth_amd.options import MonodepthOptions

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    monkeypatch.setattr(torch.Tensor, "cuda", no_gpu)
    opt = MonodepthOptions().parse(["--eval_mono", "--det_name", "d", "--load_weights_folder", "/nonexistent"] + extra)
    with pytest.raises(ValueError, match="--pl_name"):
        X.evaluate(opt, "splits", pl_name="pl")


def test_points_export_needs_the_gpu(monkeypatch):
    import torch
    from fusiondepth_amd import detection as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU"):
        D.points_export([torch.zeros(2, 3)], [None])
    with pytest.raises(RuntimeError, match="GPU"):
        D.points_export(None, [], packed=(torch.zeros(6), np.zeros(0, D.EXPORT_DESC)))


def test_library_declares_and_exports_the_call():
    import re
    from fusiondepth_amd import _lib, build
    lib = ctypes.CDLL(build.build(verbose=False))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "fdhip.h")).read(), flags=re.S)
    for name in ("fd_points_export", "fd_points_export_ws_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
    assert "#define FD_ABI_VERSION 8" in header and "} fd_points_calib;" in header
    assert _lib.SIGNATURES["fd_points_export"] == ("pppiliidpppp", "i")
    assert ctypes.sizeof(_lib.PointsCalib) == 144 and _lib.PointsCalib.A.offset == 48 and _lib.PointsCalib.t.offset == 120
    assert _lib.query("fd_points_export_ws_bytes", 16, 375) == 2 * 16 * 375 * 4      # a count and a first slot per row, separate arrays
    assert _lib.query("fd_points_export_ws_bytes", 1, 1) == 16
    assert _lib.query("fd_points_export_ws_bytes", 0, 5) == 0 and _lib.query("fd_points_export_ws_bytes", 65536, 5) == 0
