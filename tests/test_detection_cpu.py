"""The host side of the KITTI 3-D detection export (``fusiondepth_amd.detection``, ``fusiondepth_amd.export_detection``): the
calibration table, the object-layout path rules, the refusals - and the precondition of the exact-equality GPU tests
(tests/test_gpu_detection.py): on the fixture inputs the restatement's payload lies inside the uint16 range."""
import os
import types

import numpy as np
import pytest

import detection_ref as DR
import eigen_eval_ref as ER


def _opt(**over):
    o = types.SimpleNamespace(need_4beam=True, need_2_channel=True, need_full_res_4beam=False, need_inf_gdc=False, clone_gdc=False,
                              need_path=True, nbeams=4, random_sample=-1)
    for k, v in over.items():
        setattr(o, k, v)
    return o


def test_module_imports_without_a_gpu():
    import fusiondepth_amd.detection as D
    import fusiondepth_amd.export_detection as X
    assert callable(D.depth_export) and callable(D.KITTIDetecBatches) and callable(X.evaluate) and callable(X.main)
    assert D.EXPORT_DESC.itemsize == 24


def test_calibration_table_and_its_refusal():
    from fusiondepth_amd.detection import detec_calib_date
    table = {(375, 1242): "2011_09_26", (370, 1224): "2011_09_28", (374, 1238): "2011_09_29", (370, 1226): "2011_09_30",
             (376, 1241): "2011_10_03"}
    for (h, w), date in table.items():
        assert detec_calib_date(h, w) == date
    with pytest.raises(ValueError, match="300 x 1000"):
        detec_calib_date(300, 1000)
    with pytest.raises(ValueError):
        detec_calib_date(1242, 375)


def test_image_size_reads_the_header(tmp_path):
    from PIL import Image
    from fusiondepth_amd.detection import image_size
    path = str(tmp_path / "a.png")
    Image.fromarray(np.zeros((37, 53, 3), np.uint8)).save(path)
    assert image_size(path) == (37, 53)
    grey = str(tmp_path / "b.png")
    Image.fromarray(np.zeros((5, 9), np.uint16)).save(grey)
    assert image_size(grey) == (5, 9)


def test_paths_and_beam_folder_rules(tmp_path):
    from PIL import Image
    from fusiondepth_amd.detection import KITTIDetecBatches
    root = str(tmp_path)
    lines = ["training 7 l", "training 12 r"]
    b = KITTIDetecBatches(root, lines, 192, 640, [0], 4, is_train=False, img_ext=".png", opt=_opt())
    assert b.get_image_path("training", 7, "l") == os.path.join(root, "training", "image_02/data", "000007.png")
    assert b.get_image_path("training", 12, "r") == os.path.join(root, "training", "image_03/data", "000012.png")
    assert b.get_velo_path("training", 7) == os.path.join(root, "training", "velodyne_points/data/000007.bin")
    assert b.beam_folder() == "4beam" and b.get_beam_path("training", 7) == os.path.join(root, "training", "4beam/000007.bin")
    assert not b.load_depth                                    # no scan on disk
    # the reference's rule for this class: anything but -1 samples (the raw class tests > 0), and nbeams does not enter
    r = KITTIDetecBatches(root, lines, 192, 640, [0], 4, is_train=False, img_ext=".png", opt=_opt(random_sample=200, nbeams=2))
    assert r.beam_folder() == "random200" and r.get_beam_path("training", 12) == os.path.join(root, "training", "random200/000012.bin")
    assert KITTIDetecBatches(root, lines, 192, 640, [0], 4, opt=_opt(random_sample=0)).beam_folder() == "random0"
    assert KITTIDetecBatches(root, lines, 192, 640, [0], 4, opt=_opt(nbeams=2)).beam_folder() == "4beam"
    # the calibration date comes from the size of the line's image_02 frame, whatever the side, and becomes the item's date
    os.makedirs(os.path.join(root, "training", "image_02/data"))
    Image.fromarray(np.zeros((370, 1224, 3), np.uint8)).save(os.path.join(root, "training", "image_02/data/000012.png"))
    Image.fromarray(np.zeros((300, 1000, 3), np.uint8)).save(os.path.join(root, "training", "image_02/data/000007.png"))
    item = b.plan_batch(0, [1])[0]
    assert item["date"] == "2011_09_28" and b.calib_date("training", 12) == "2011_09_28"
    assert item["images"] == [os.path.join(root, "training", "image_03/data", "000012.png")]
    assert item["beams"] == [os.path.join(root, "training", "4beam/000012.bin")]
    with pytest.raises(ValueError, match="300 x 1000"):
        b.plan_batch(0, [0])


def test_raw_lidar_source_is_refused(tmp_path):
    from fusiondepth_amd.detection import KITTIDetecBatches
    with pytest.raises(NotImplementedError, match="raw"):
        KITTIDetecBatches(str(tmp_path), ["training 0 l"], 192, 640, [0], 4, opt=_opt(), lidar_source="raw")
    with pytest.raises(NotImplementedError, match="stereo"):    # the parent's refusals stay
        KITTIDetecBatches(str(tmp_path), ["training 0 l"], 192, 640, [0, "s"], 4, opt=_opt())


def test_output_names():
    from fusiondepth_amd.detection import detec_output_name, export_gt_depths_detec
    assert detec_output_name("detec") == "gt_depths.npz" and detec_output_name("detec4beam") == "4beam.npz"
    with pytest.raises(ValueError):
        detec_output_name("eigen")
    with pytest.raises(ValueError):
        export_gt_depths_detec("/nowhere", [], "eigen")


def test_det_name_is_required(tmp_path):
    from fusiondepth_amd import export_detection as X
    from fusiondepth_amd.options import MonodepthOptions
    with pytest.raises(ValueError, match="det_name"):
        X.evaluate(MonodepthOptions().parse(["--eval_mono", "--data_path", str(tmp_path)]), str(tmp_path))
    with pytest.raises(ValueError, match="eval_mono"):          # evaluate_depth's refusals come first
        X.evaluate(MonodepthOptions().parse(["--det_name", "pred"]), str(tmp_path))
    assert X.png_path("/data", "training 41 l", "pred") == os.path.join("/data", "training", "pred", "000041.png")


def test_quantiser_rule_of_the_restatement():
    q = np.array([0.0, 0.99, 1.0, 255.7, 65534.9, 65535.0, 7e4, np.inf, -0.5, -3.0, -np.inf, np.nan], np.float32)
    assert DR.quantize(q).tolist() == [0, 0, 1, 255, 65534, 65535, 65535, 65535, 0, 0, 0, 0]
    inside = np.array([1.0, 2.5, 660.0, 15605.9, 65534.5], np.float32)
    assert np.array_equal(DR.quantize(inside), inside.astype(np.uint16))


def test_fixture_payload_stays_inside_the_uint16_range():
    """The exact-equality tests compare ``astype(np.uint16)`` of the restatement with the kernel: that is only defined in range.  With
    the whole-map ratios and with the stereo factor 5.4, every product ``q`` of the fixture lies in [1, 65535) and none is NaN."""
    disps, gts = DR.fixture()
    ratios = ER.restate(list(disps), gts, "eigen_benchmark")["ratios"]
    # gt / pred lies in 1.3 * [0.9, 1.1] at every pixel, and so does the ratio of the medians
    assert ratios.shape == (len(DR.SIZES),) and np.isfinite(ratios).all() and 1.17 <= ratios.min() and ratios.max() <= 1.43, ratios
    lo, hi = np.inf, -np.inf
    for d, size, r in zip(disps, DR.SIZES, ratios):
        for scale, ratio in ((1.0, r), (5.4, None)):
            p, q, u = DR.restate(d, size, scale, ratio)
            assert p.shape == tuple(size) and not np.isnan(q).any() and q.min() >= 1 and q.max() < 65535, (size, scale, q.min(), q.max())
            assert np.array_equal(u, q.astype(np.uint16))
            lo, hi = min(lo, q.min()), max(hi, q.max())
    assert 600 < lo and hi < 65535
    # the Garg window of the 1x1 map is empty: no ratio there, which the quantiser rule turns into an all-zero export
    eigen = ER.restate(list(disps), gts, "eigen")
    assert eigen["counts"][0] == 0 and np.isnan(eigen["ratios"][0])
    assert (DR.restate(disps[0], DR.SIZES[0], 1.0, eigen["ratios"][0])[2] == 0).all()


def test_special_plane_of_the_restatement():
    d, where = DR.special_plane()
    _, _, u = DR.restate(d, DR.SRC)
    assert u[where["zero"]] == 65535 and u[where["nan"]] == 0 and u[where["negative"]] == 0 and u[where["far"]] == 65535
    plain = np.ones(DR.SRC, bool)
    for y, x in where.values():
        plain[max(y - 1, 0):y + 1, max(x - 1, 0):x + 1] = False  # a NaN reaches its upper and left neighbours through 0 * NaN
    assert ((u[plain] > 0) & (u[plain] < 65535)).all()
