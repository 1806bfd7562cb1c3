"""``fusiondepth_amd.datasets.KITTIRAWBatches`` end to end on a synthetic KITTI tree: every key of a batch against the same item
assembled from PIL + tests/augment_ref.py (colour) and the existing ``kitti_utils`` functions (LiDAR), bit for bit; batch order,
``drop_last``, the prefetching stream hand-over; and a Trainer epoch fed by the builder."""
import os
import types

import numpy as np
import pytest
import torch

import augment_ref as R
import inputs as gin

pytestmark = pytest.mark.gpu

FRAME_IDS = [0, -1, 1]


def _write_calib(d, im_h, im_w, sx=1.0, sy=1.0):
    """calib_cam_to_cam.txt / calib_velo_to_cam.txt of a date folder (formats of kitti_utils.py:14-30, 43-57); ``sx`` / ``sy`` scale
    the camera so that a smaller image sees the same scene."""
    gin.lidar_scan(1, n_points=1000, im_h=im_h, im_w=im_w)             # only its calibration is used
    cal = gin.lidar_scan.calib
    P = np.diag([sx, sy, 1.0]) @ cal["P_rect_02"]
    fmt = lambda a: " ".join("%.17g" % v for v in np.asarray(a, dtype=np.float64).reshape(-1))
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "calib_cam_to_cam.txt"), "w") as f:
        f.write("calib_time: 09-Jan-2012 13:57:47\nS_rect_02: %s\nR_rect_00: %s\nP_rect_02: %s\nP_rect_03: %s\n"
                % (fmt([im_w, im_h]), fmt(cal["R_rect_00"]), fmt(P), fmt(P)))
    with open(os.path.join(d, "calib_velo_to_cam.txt"), "w") as f:
        f.write("R: %s\nT: %s\n" % (fmt(cal["R"]), fmt(cal["T"])))


def _scan(rng, n):
    """float32 [n,4] Velodyne points; half of them 4 .. 7 m ahead (where an untrained network's depth lies, so the LiDAR loss of the
    trainer test has valid returns)."""
    fwd = np.where(rng.random(n) < 0.5, rng.uniform(4.0, 7.0, n), rng.uniform(2.0, 70.0, n))
    return np.stack([fwd, rng.uniform(-0.45, 0.45, n) * fwd, rng.uniform(-0.2, 0.12, n) * fwd, rng.random(n)], 1).astype(np.float32)


def make_tree(root, drives, frames=6, ext=".png", full_scans=True):
    """``drives``: [(date, drive, (im_h, im_w), camera scale)].  Writes images (PIL), calibration, ``4beam/`` scans for every frame
    and ``velodyne_points/data`` scans; returns the split lines of the frames that have both neighbours."""
    from PIL import Image
    rng = np.random.default_rng(77)
    lines = []
    for date, drive, (im_h, im_w), scale in drives:
        _write_calib(os.path.join(root, date), im_h, im_w, *scale)
        folder = "%s/%s" % (date, drive)
        for sub in ("image_02/data", "4beam", "velodyne_points/data"):
            os.makedirs(os.path.join(root, folder, sub), exist_ok=True)
        for i in range(frames):
            blocks = rng.integers(0, 256, (im_h // 16 + 1, im_w // 16 + 1, 3))
            img = np.repeat(np.repeat(blocks, 16, axis=0), 16, axis=1)[:im_h, :im_w] + rng.integers(-30, 31, (im_h, im_w, 3))
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(root, folder, "image_02/data/%010d%s" % (i, ext)))
            _scan(rng, 900).tofile(os.path.join(root, folder, "4beam/%010d.bin" % i))
            if full_scans:
                _scan(rng, 5000).tofile(os.path.join(root, folder, "velodyne_points/data/%010d.bin" % i))
        lines += ["%s %d l" % (folder, i) for i in range(1, frames - 1)]
    return lines


def _opt(**over):
    o = types.SimpleNamespace(need_4beam=True, need_2_channel=True, need_full_res_4beam=False, need_inf_gdc=False, clone_gdc=False,
                              need_path=True, nbeams=4, random_sample=-1)
    for k, v in over.items():
        setattr(o, k, v)
    return o


JITTERS = [((1.2, 0.8, 1.1, 0.1), [0, 1, 2, 3]), ((0.8, 1.2, 0.85, -0.1), [3, 2, 1, 0]), ((1.05, 0.95, 1.2, -0.04), [2, 0, 3, 1])]


def injected(epoch, index):
    """Flags and jitter parameters by item index: all four flag combinations occur."""
    aug, flip = bool(index % 2), bool((index // 2) % 2)
    return {"do_color_aug": aug, "do_flip": flip, "jitter": JITTERS[index % 3] if aug else None}


def expected_item(root, line, draws, height, width, num_scales):
    """One item the reference's way: PIL decode and flip, then the restatement for the pyramid / jitter / ToTensor, and the existing
    kitti_utils functions for the LiDAR keys."""
    from PIL import Image
    from fusiondepth_amd import functional as FD
    from fusiondepth_amd import kitti_utils
    folder, frame, side = line.split()
    frame = int(frame)
    calib = os.path.join(root, folder.split("/")[0])
    out = {}
    for f in FRAME_IDS:
        img = Image.open(os.path.join(root, folder, "image_02/data/%010d.png" % (frame + f))).convert("RGB")
        if draws["do_flip"]:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        pyr = R.pyramid(np.asarray(img), height, width, num_scales)
        for s in range(num_scales):
            out[("color", f, s)] = R.to_planes(pyr[s])
            aug = R.color_jitter(pyr[s], *draws["jitter"]) if draws["do_color_aug"] else pyr[s]
            out[("color_aug", f, s)] = R.to_planes(aug)
        beam = kitti_utils.get_4beam_device(calib, os.path.join(root, folder, "4beam/%010d.bin" % (frame + f)), 2, draws["do_flip"])
        two = FD.scatter_2channel(beam[None, None])[0]
        out[("2channel", f, 0)] = two.cpu().numpy()
        if f == 0:
            out["4beam"] = beam[None].cpu().numpy()
            out["2channel"] = two.cpu().numpy()
    gt = kitti_utils.generate_depth_map(calib, os.path.join(root, folder, "velodyne_points/data/%010d.bin" % frame), 2, shape=[375, 1242])
    if draws["do_flip"]:
        gt = np.fliplr(gt)
    out["depth_gt"] = gt[None].astype(np.float32)
    return out


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti"))
    lines = make_tree(root, [("2011_09_26", "2011_09_26_drive_0001_sync", (375, 1242), (1.0, 1.0)),
                             ("2011_09_30", "2011_09_30_drive_0016_sync", (370, 1226), (1.0, 1.0))])
    return root, lines


def _np(v):
    return v.cpu().numpy()


def test_every_key_of_every_batch(tree):
    from fusiondepth_amd import synthetic
    from fusiondepth_amd.datasets import KITTIRAWBatches
    root, lines = tree
    assert len(lines) == 8
    # batch 3 over 8 items: two batches, the last two items dropped; the second batch mixes the two drives' native sizes
    loader = KITTIRAWBatches(root, lines, 192, 640, FRAME_IDS, 4, is_train=True, img_ext=".png", opt=_opt(), batch_size=3, draws=injected)
    assert len(loader) == 2 and loader.load_depth
    batches = list(loader)
    torch.cuda.synchronize()
    assert len(batches) == 2
    K = synthetic.intrinsics(3, 192, 640, 4, "cuda")
    for bi, batch in enumerate(batches):
        idx = [3 * bi + k for k in range(3)]
        assert batch["date"] == [lines[i].split("/")[0] for i in idx] and batch["path"] == [lines[i] for i in idx]
        want = [expected_item(root, lines[i], injected(0, i), 192, 640, 4) for i in idx]
        keys = set(want[0])
        assert set(batch) == keys | set(K) | {"date", "path"}
        for key in sorted(keys, key=str):
            got = _np(batch[key])
            assert got.dtype == np.float32 and got.shape[0] == 3, key
            for k in range(3):
                assert got[k].shape == want[k][key].shape, (key, got[k].shape, want[k][key].shape)
                assert np.array_equal(got[k], want[k][key]), (bi, k, key, int((got[k] != want[k][key]).sum()))
        for key, v in K.items():
            assert np.array_equal(_np(batch[key]), _np(v)), key
        assert batch[("color", 0, 0)].shape == (3, 3, 192, 640) and batch["4beam"].shape == (3, 1, 192, 640)
        assert batch["2channel"].shape == (3, 2, 192, 640) and batch["depth_gt"].shape == (3, 1, 375, 1242)
    # an item without colour augmentation: color_aug equals color
    plain = KITTIRAWBatches(root, lines, 192, 640, FRAME_IDS, 4, is_train=False, img_ext=".png", opt=_opt(), batch_size=2)
    b0 = next(iter(plain))
    assert all(np.array_equal(_np(b0[("color_aug", f, s)]), _np(b0[("color", f, s)])) for f in FRAME_IDS for s in range(4))
    loader.close()
    plain.close()


def test_prefetched_batches_equal_unprefetched_ones_and_shuffle_order(tree):
    from fusiondepth_amd.datasets import KITTIRAWBatches
    root, lines = tree
    mk = lambda **kw: KITTIRAWBatches(root, lines, 192, 640, FRAME_IDS, 2, is_train=True, img_ext=".png", opt=_opt(), batch_size=2, shuffle=True,
                                      seed=4, **kw)
    a, b = mk(prefetch=True), mk(prefetch=False)
    for epoch in range(2):
        order = a.epoch_order(epoch)
        ba, bb = list(a), list(b)
        torch.cuda.synchronize()
        assert len(ba) == len(bb) == 4
        for i, (x, y) in enumerate(zip(ba, bb)):
            assert x["path"] == y["path"] == [lines[j] for j in order[2 * i:2 * i + 2]]
            assert set(x) == set(y)
            for k in x:
                if torch.is_tensor(x[k]):
                    assert np.array_equal(_np(x[k]), _np(y[k])), (epoch, i, k)
    assert a.epoch_order(0) != a.epoch_order(1)
    a.close()
    b.close()


def test_per_image_jitter_and_predecoded_frames(tree):
    """``jitter_per_image``: every (frame, scale) has its own draw; ``loader=``: frames handed over as arrays."""
    from PIL import Image
    from fusiondepth_amd.datasets import KITTIRAWBatches
    root, lines = tree
    per = [[((1.0 + 0.01 * (3 * fi + s), 0.9, 1.1, 0.02 * (s - 1)), [(fi + s + k) % 4 for k in range(4)]) for s in range(2)] for fi in range(3)]
    draws = lambda epoch, index: {"do_color_aug": True, "do_flip": False, "jitter": per}
    cache = {}

    def loader(path):
        if path not in cache:
            cache[path] = np.asarray(Image.open(path).convert("RGB"))
        return cache[path]

    b = KITTIRAWBatches(root, lines[:2], 96, 320, FRAME_IDS, 2, is_train=True, img_ext=".png", opt=_opt(need_4beam=False, need_2_channel=False),
                        batch_size=2, draws=draws, loader=loader, jitter_per_image=True)
    batch = next(iter(b))
    torch.cuda.synchronize()
    assert "4beam" not in batch and "2channel" not in batch and len(cache) == 4
    for k, line in enumerate(lines[:2]):
        folder, frame, _ = line.split()
        for fi, f in enumerate(FRAME_IDS):
            pyr = R.pyramid(cache[os.path.join(root, folder, "image_02/data/%010d.png" % (int(frame) + f))], 96, 320, 2)
            for s in range(2):
                want = R.to_planes(R.color_jitter(pyr[s], *per[fi][s]))
                assert np.array_equal(_np(batch[("color_aug", f, s)])[k], want), (k, f, s)
    b.close()


def test_trainer_epoch_fed_by_the_builder(tmp_path):
    """``Trainer(opts).train(KITTIRAWBatches(...))`` as is, at 64x96 and batch 2: the loss is finite, and the parameters after the epoch are
    bit-identical to a run fed the same batches from a pre-built list - the builder's stream hand-over is race-free."""
    from fusiondepth_amd.datasets import KITTIRAWBatches
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.trainer import Trainer
    root = str(tmp_path / "kitti")
    # native 128x192 frames; the camera is scaled with the image so that the scans still cover it
    lines = make_tree(root, [("2011_09_26", "2011_09_26_drive_0001_sync", (128, 192), (192 / 1242.0, 128 / 375.0)),
                             ("2011_09_28", "2011_09_28_drive_0002_sync", (128, 192), (192 / 1242.0, 128 / 375.0))], full_scans=False)

    def opts(name):
        return MonodepthOptions().parse(["--num_layers", "18", "--weights_init", "scratch", "--batch_size", "2", "--height", "64", "--width", "96",
                                         "--num_epochs", "1", "--png", "--data_path", root, "--log_dir", str(tmp_path / name),
                                         "--log_frequency", "1"])

    def builder(opt, **kw):
        return KITTIRAWBatches(opt.data_path, lines, opt.height, opt.width, opt.frame_ids, 4, is_train=True, img_ext=".png", opt=opt,
                               batch_size=opt.batch_size, shuffle=True, seed=1, **kw)

    def run(name, feed):
        opt = opts(name)
        torch.manual_seed(5)
        tr = Trainer(opt, verbose=False)
        tr.opt.num_epochs = 1                                      # the constructor derives the epoch count from the batch size
        torch.manual_seed(6)
        loader = feed(opt)
        tr.train(loader)
        torch.cuda.synchronize()
        return tr

    a = run("a", lambda opt: builder(opt))
    assert a.step == 4 and np.isfinite(a.last_log_time["loss"])

    def prebuilt(opt):
        b = builder(opt, prefetch=False)
        batches = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()} for batch in b]
        torch.cuda.synchronize()
        b.close()
        assert len(batches) == 4 and batches[0]["4beam"].shape == (2, 1, 64, 96) and batches[0][("color_aug", -1, 3)].shape == (2, 3, 8, 12)
        return batches

    b = run("b", prebuilt)
    assert b.step == 4
    pa, pb = a.flat.flat_param.cpu().numpy(), b.flat.flat_param.cpu().numpy()
    assert np.isfinite(pa).all() and np.array_equal(pa, pb), "%d parameters differ" % (pa != pb).sum()
    assert a.last_log_time["loss"] == b.last_log_time["loss"]
