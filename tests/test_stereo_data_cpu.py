"""``fusiondepth_amd.datasets.KITTIStereoBatches`` without a device: what a batch reads for the stereo partner "s"
(mono_dataset.py:156-163), ``stereo_T`` (mono_dataset.py:216-222), the per-image jitter draws, and that "s" arrives as a new class -
the four existing builders still refuse it."""
import types

import numpy as np
import pytest

FOLDER = "2011_09_26/2011_09_26_drive_0001_sync"


def _opt(**over):
    o = types.SimpleNamespace(need_4beam=True, need_2_channel=True, need_full_res_4beam=False, need_inf_gdc=False, clone_gdc=False,
                              need_path=False, nbeams=4, random_sample=-1)
    for k, v in over.items():
        setattr(o, k, v)
    return o


def _lines(n=6):
    return ["%s %d %s" % (FOLDER, i + 1, "lr"[i % 2]) for i in range(n)]


def _builder(frames, lines=None, **kw):
    from fusiondepth_amd.datasets import KITTIStereoBatches
    args = dict(is_train=True, img_ext=".png", opt=_opt(), batch_size=2, device="cpu")
    args.update(kw)
    return KITTIStereoBatches("/data/kitti", lines or _lines(), 192, 640, frames, 4, **args)


@pytest.mark.parametrize("frames", [[0, "s"], [0, -1, 1, "s"]])
@pytest.mark.parametrize("lidar_source", ["files", "raw"])
def test_plan_reads_the_other_camera_at_the_same_frame(frames, lidar_source):
    b = _builder(frames, lidar_source=lidar_source)
    temporal = [f for f in frames if f != "s"]
    for item, (index, side) in zip(b.plan_batch(0, [2, 3]), [(3, "l"), (4, "r")]):
        assert item["side"] == side and item["frame_index"] == index
        own, other = ("image_02", "image_03") if side == "l" else ("image_03", "image_02")
        want = ["/data/kitti/%s/%s/data/%010d.png" % (FOLDER, own, index + f) for f in temporal]
        want.append("/data/kitti/%s/%s/data/%010d.png" % (FOLDER, other, index))
        assert item["images"] == want
        # beams and scans for the integer frames only: "s" has no scan of its own
        if lidar_source == "files":
            assert item["beams"] == [b.get_beam_path(FOLDER, index + f) for f in temporal]
        else:
            assert item["frames"] == [index + f for f in temporal]
            assert item["beams"] == [b.get_velo_path(FOLDER, index + f) for f in temporal]
    only0 = _builder(frames, opt=_opt(need_2_channel=False), lidar_source=lidar_source).plan_batch(0, [2])[0]
    assert len(only0["beams"]) == 1 and only0["beams"][0].endswith("%010d.bin" % 3)
    assert b.lidar_frames() == temporal


def test_a_line_without_a_side_has_no_stereo_partner():
    lines = _lines(3) + [FOLDER]
    b = _builder([0, "s"], lines=lines)
    b.plan_batch(0, [0, 1])
    with pytest.raises(ValueError, match=FOLDER + r"'"):
        b.plan_batch(0, [2, 3])
    # without "s" the class is the plain loader and plans such a line as the parent does
    from fusiondepth_amd.datasets import KITTIStereoBatches
    with pytest.raises(KeyError):       # the parent's behaviour for a bare folder: no side, no image folder
        KITTIStereoBatches("/data/kitti", lines, 192, 640, [0], 4, opt=_opt(), device="cpu").plan_batch(0, [3])


def test_stereo_T_signs():
    from fusiondepth_amd.datasets import stereo_T
    for side, flip, want in (("l", False, -0.1), ("l", True, 0.1), ("r", False, 0.1), ("r", True, -0.1)):
        T = stereo_T(side, flip)
        assert T.dtype == np.float32 and T.shape == (4, 4)
        expect = np.eye(4, dtype=np.float32)
        expect[0, 3] = want
        assert np.array_equal(T, expect), (side, flip, T)


def test_per_image_jitter_draws_cover_the_stereo_slot():
    for frames in ([0, "s"], [0, -1, 1, "s"]):
        b = _builder(frames, jitter_per_image=True, seed=3)
        seen = 0
        for index in range(6):
            d = b.item_draws(0, index)
            if not d["do_color_aug"]:
                continue
            seen += 1
            assert len(d["jitter"]) == len(frames) and all(len(per_scale) == 4 for per_scale in d["jitter"])
            assert d["jitter"][-1][0] != d["jitter"][0][0]            # the slot of "s" has draws of its own
        assert seen
        assert not isinstance(_builder(frames, seed=3).item_draws(0, 0)["jitter"], list)


def test_frame_zero_is_still_required_and_the_other_refusals_stay():
    with pytest.raises(ValueError, match="contain 0"):
        _builder(["s"])
    with pytest.raises(NotImplementedError, match="need_full_res_4beam"):
        _builder([0, "s"], opt=_opt(need_full_res_4beam=True))
    with pytest.raises(NotImplementedError, match="need_inf_gdc"):
        _builder([0, "s"], opt=_opt(need_inf_gdc=True))
    with pytest.raises(NotImplementedError, match="clone_gdc"):
        _builder([0, "s"], opt=_opt(clone_gdc=True))


def test_the_four_existing_builders_still_refuse_the_stereo_frame(tmp_path):
    import completion_tree as CT
    from fusiondepth_amd.completion_data import KITTICompletionBatches
    from fusiondepth_amd.datasets import KITTIRAWBatches, KITTIRefinerBatches
    from fusiondepth_amd.detection import KITTIDetecBatches
    with pytest.raises(NotImplementedError, match="stereo"):
        KITTIRAWBatches("/d", _lines(), 192, 640, [0, "s"], 4, opt=_opt(), device="cpu")
    with pytest.raises(NotImplementedError, match="stereo"):
        KITTIRefinerBatches("/d", _lines(), 192, 640, [0, -1, 1, "s"], 4, opt=_opt(clone_gdc=True), device="cpu")
    with pytest.raises(NotImplementedError, match="stereo"):
        KITTIDetecBatches(str(tmp_path), ["training 0 l"], 192, 640, [0, "s"], 4, opt=_opt(), device="cpu")
    tree = CT.make_tree(str(tmp_path / "completion"))
    with pytest.raises(NotImplementedError, match="stereo"):
        KITTICompletionBatches(tree, 352, 1216, [0, "s"], 4, is_train=True, opt=CT.options(), device="cpu")
