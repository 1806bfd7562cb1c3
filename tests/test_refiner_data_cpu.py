"""Host side of the Refiner's data chain: the bilinear rule ``fd_resize_bilinear_batch`` implements, restated in numpy and pinned to
the installed torch's CPU ``F.interpolate`` bit for bit; ``KITTIRefinerBatches`` planning; ``drop_last``; the ``inf_depth_map``
command line."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------- the rule (include/fdhip.h)
def _fma(a, b, c):
    """float32 fused multiply-add: the float64 product of two float32 values is exact; the float64 sum is rounded once to 53 bits and
    then to 24 (double rounding could differ from a true fma only on an exact 53-bit tie pattern, which the comparison below would show)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _axis(n_in, n_out):
    scale = np.float32(n_in) / np.float32(n_out)
    d = np.arange(n_out, dtype=np.float32) + np.float32(0.5)
    src = _fma(np.full(n_out, scale, np.float32), d, np.full(n_out, -0.5, np.float32))
    src = np.maximum(src, np.float32(0))
    i0 = src.astype(np.int32)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(np.float32)
    l0 = np.float32(1.0) - l1
    return i0, i1, l0, l1


def resize_rule(x, size):
    x = np.asarray(x, dtype=np.float32)
    y0, y1, hy, ly = _axis(x.shape[0], size[0])
    x0, x1, hx, lx = _axis(x.shape[1], size[1])
    hx, lx, hy, ly = hx[None, :], lx[None, :], hy[:, None], ly[:, None]
    top = _fma(hx, x[y0][:, x0], lx * x[y0][:, x1])
    bot = _fma(hx, x[y1][:, x0], lx * x[y1][:, x1])
    return _fma(hy, top, ly * bot)


SHAPES = [((h, w), (48, 160)) for h, w in ((94, 311), (93, 307), (96, 312), (40, 100), (47, 161), (48, 160))] + \
         [((94, 311), s) for s in ((64, 96), (40, 160), (48, 128))] + \
         [((h, w), (192, 640)) for h, w in ((375, 1242), (370, 1226), (374, 1238), (376, 1241))]


@pytest.mark.parametrize("src,dst", SHAPES, ids=["%dx%d-%dx%d" % (s + d) for s, d in SHAPES])
def test_numpy_restatement_equals_torch_cpu_bitwise(src, dst):
    import kitti_tree
    x = kitti_tree.depth_like(np.random.default_rng(src[0] * 7 + dst[1]), *src)
    want = F.interpolate(torch.from_numpy(x)[None, None], list(dst), mode="bilinear", align_corners=False)[0, 0].numpy()
    got = resize_rule(x, dst)
    assert got.dtype == np.float32 and got.shape == dst
    assert np.array_equal(got, want), "%d of %d elements differ" % ((got != want).sum(), got.size)


# --------------------------------------------------------------------------------------------- planning
def _opt(**over):
    o = types.SimpleNamespace(need_4beam=True, need_2_channel=True, need_full_res_4beam=False, need_inf_gdc=False, clone_gdc=False,
                              need_path=False, nbeams=4, random_sample=-1)
    for k, v in over.items():
        setattr(o, k, v)
    return o


def _lines(n=7):
    return ["2011_09_26/2011_09_26_drive_0001_sync %d %s" % (i + 1, "lr"[i % 2]) for i in range(n)]


def _refiner_builder(**kw):
    from fusiondepth_amd.datasets import KITTIRefinerBatches
    args = dict(is_train=True, img_ext=".png", opt=_opt(clone_gdc=True), batch_size=2, device="cpu")
    args.update(kw)
    return KITTIRefinerBatches("/data/kitti", _lines(), 192, 640, [0, -1, 1], 4, **args)


def test_gdc_paths_and_when_the_key_is_planned():
    folder = "2011_09_26/2011_09_26_drive_0001_sync"
    b = _refiner_builder()
    assert b.need_gdc
    assert b.get_gdc_path(folder, 7, "l") == "/data/kitti/%s/inf_gdc_4beam/7_l.npy" % folder
    assert _refiner_builder(opt=_opt(clone_gdc=True, nbeams=2)).get_gdc_path(folder, 12, "r") == "/data/kitti/%s/inf_gdc_2beam/12_r.npy" % folder
    assert _refiner_builder(opt=_opt(clone_gdc=True, random_sample=200)).get_gdc_path(folder, 3, "l") == "/data/kitti/%s/inf_gdc_r200/3_l.npy" % folder
    plan = b.plan_batch(0, [2, 3])
    assert [p["gdc"] for p in plan] == [b.get_gdc_path(folder, 3, "l"), b.get_gdc_path(folder, 4, "r")]
    assert plan[0]["images"] == [b.get_image_path(folder, 3 + f, "l") for f in (0, -1, 1)]          # the parent's plan is untouched
    ev = _refiner_builder(is_train=False)                                      # clone_gdc alone, not training: no key
    assert not ev.need_gdc and "gdc" not in ev.plan_batch(0, [2])[0]
    for is_train in (False, True):
        nb = _refiner_builder(opt=_opt(need_inf_gdc=True), is_train=is_train)
        assert nb.need_gdc and nb.plan_batch(0, [2])[0]["gdc"] == b.get_gdc_path(folder, 3, "l")
    plain = _refiner_builder(opt=_opt())
    assert not plain.need_gdc and "gdc" not in plain.plan_batch(0, [2])[0]


def test_refiner_builder_still_refuses_stereo_and_full_res():
    from fusiondepth_amd.datasets import KITTIRefinerBatches
    with pytest.raises(NotImplementedError, match="stereo"):
        KITTIRefinerBatches("/d", _lines(), 192, 640, [0, "s"], 4, opt=_opt(clone_gdc=True))
    with pytest.raises(NotImplementedError, match="need_full_res_4beam"):
        _refiner_builder(opt=_opt(clone_gdc=True, need_full_res_4beam=True))


def test_gdc_staging_layout_is_planned_from_the_dates_image_size(tmp_path):
    import ctypes
    import kitti_tree
    from fusiondepth_amd import _lib
    from fusiondepth_amd.datasets import KITTIRefinerBatches
    kitti_tree.write_calib(str(tmp_path / "2011_09_26"), 375, 1242)
    kitti_tree.write_calib(str(tmp_path / "2011_09_30"), 370, 1226)
    lines = ["2011_09_26/a 1 l", "2011_09_30/b 2 l", "2011_09_26/a 3 l"]
    draws = lambda epoch, index: {"do_color_aug": False, "do_flip": index == 1, "jitter": None}
    b = KITTIRefinerBatches(str(tmp_path), lines, 192, 640, [0], 4, is_train=True, opt=_opt(clone_gdc=True), batch_size=3, device="cpu",
                            draws=draws)
    plan = b._plan_gdc(b.plan_batch(0, [0, 1, 2]))
    n0, n1 = 375 * 1242, 370 * 1226
    assert plan["descs"] == [(0, 375, 1242, False), (n0, 370, 1226, True), (n0 + n1, 375, 1242, False)]
    table = 3 * ctypes.sizeof(_lib.ResizeDesc)
    assert plan["table"] == (0, table) and plan["planes"][0] % 16 == 0 and plan["planes"][0] >= table
    assert plan["planes"][1] - plan["planes"][0] == 4 * (2 * n0 + n1) and plan["bytes"] == plan["planes"][1]
    assert ctypes.sizeof(_lib.ResizeDesc) == 24


# --------------------------------------------------------------------------------------------- drop_last
def test_drop_last_false_yields_the_trailing_partial_batch():
    from fusiondepth_amd.datasets import KITTIRAWBatches
    mk = lambda **kw: KITTIRAWBatches("/data/kitti", _lines(), 192, 640, [0], 4, is_train=False, opt=_opt(), device="cpu", **kw)
    for B in (1, 2, 3, 7, 8):
        assert len(mk(batch_size=B)) == 7 // B and len(mk(batch_size=B, drop_last=True)) == 7 // B
        assert len(mk(batch_size=B, drop_last=False)) == -(-7 // B)
    assert mk(batch_size=2).epoch_order(0) == [0, 1, 2, 3, 4, 5]
    assert mk(batch_size=2, drop_last=False).epoch_order(0) == [0, 1, 2, 3, 4, 5, 6]
    sh = mk(batch_size=3, drop_last=False, shuffle=True, seed=3)
    assert sorted(sh.epoch_order(0)) == list(range(7)) and sh.epoch_order(0)[:6] == mk(batch_size=3, shuffle=True, seed=3).epoch_order(0)
    assert len(_refiner_builder(drop_last=False)) == 4 and len(_refiner_builder()) == 3


# --------------------------------------------------------------------------------------------- inf_depth_map command line
def test_inf_depth_map_flags_and_output_paths():
    from fusiondepth_amd import inf_depth_map, inf_gdc
    a = inf_depth_map.parse_args(["--load_weights_folder", "w"])
    assert a.split_files == list(inf_gdc.DEFAULT_SPLITS) and a.nbeams == 4 and a.random_sample == -1 and a.batch_size == 1
    assert (a.num_layers, a.height, a.width, a.png, a.lidar_source, a.data_path) == (50, 192, 640, False, "files", "kitti_data/")
    a = inf_depth_map.parse_args(["--load_weights_folder", "w", "--data_path", "/k", "--split_files", "a.txt", "b.txt", "--nbeams", "2",
                                  "--png", "--num_layers", "18", "--height", "64", "--width", "96", "--batch_size", "3", "--workers", "2",
                                  "--lidar_source", "raw"])
    assert a.split_files == ["a.txt", "b.txt"] and (a.nbeams, a.png, a.num_layers, a.height, a.width) == (2, True, 18, 64, 96)
    assert (a.batch_size, a.workers, a.lidar_source) == (3, 2, "raw")
    with pytest.raises(SystemExit):
        inf_depth_map.parse_args([])                                          # the weights folder is required
    line = "2011_09_26/2011_09_26_drive_0001_sync 0000000007 l"
    assert inf_depth_map.out_path(a, line) == "/k/2011_09_26/2011_09_26_drive_0001_sync/inf_depth_2beam/7_l.npy"
    r = inf_depth_map.parse_args(["--load_weights_folder", "w", "--data_path", "/k", "--random_sample", "200"])
    assert inf_depth_map.out_path(r, line) == "/k/2011_09_26/2011_09_26_drive_0001_sync/inf_depth_r200/7_l.npy"
    # what the producer writes is what inf_gdc reads, for every naming
    for args in (a, r):
        g = inf_gdc.parse_args(["--data_path", "/k", "--nbeams", str(args.nbeams), "--random_sample", str(args.random_sample)])
        assert inf_gdc.frame_paths(g, line)["disp"] == inf_depth_map.out_path(args, line)
    o = inf_depth_map.loader_options(a)
    assert o.need_4beam and o.need_2_channel and o.need_path and o.nbeams == 2 and not o.clone_gdc
