"""A synthetic KITTI raw tree for the loader / producer tests (the helpers of tests/test_gpu_datasets.py, restated so that new test
files can share them), plus what the Refiner's data chain needs on top: ``inf_gdc`` maps and the CPU recipe they go through."""
import os

import numpy as np

import inputs as gin


def write_calib(d, im_h, im_w, sx=1.0, sy=1.0):
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


def scan(rng, n, down=0.2):
    """float32 [n,4] Velodyne points; half of them 4 .. 7 m ahead (where an untrained network's depth lies, so the LiDAR terms have
    valid returns).  ``down``: how far below the sensor's horizon they reach, as a slope; 0.2 ends at about 5/6 of a KITTI image's
    height, 0.35 covers it to the bottom row."""
    fwd = np.where(rng.random(n) < 0.5, rng.uniform(4.0, 7.0, n), rng.uniform(2.0, 70.0, n))
    return np.stack([fwd, rng.uniform(-0.45, 0.45, n) * fwd, rng.uniform(-down, 0.12, n) * fwd, rng.random(n)], 1).astype(np.float32)


def make_tree(root, drives, frames=6, ext=".png", full_scans=True, seed=77, down=0.2):
    """``drives``: [(date, drive, (im_h, im_w), camera scale)].  Writes images (PIL), calibration, ``4beam/`` scans for every frame
    and ``velodyne_points/data`` scans; returns the split lines of the frames that have both neighbours."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    lines = []
    for date, drive, (im_h, im_w), scale in drives:
        write_calib(os.path.join(root, date), im_h, im_w, *scale)
        folder = "%s/%s" % (date, drive)
        for sub in ("image_02/data", "4beam", "velodyne_points/data"):
            os.makedirs(os.path.join(root, folder, sub), exist_ok=True)
        for i in range(frames):
            blocks = rng.integers(0, 256, (im_h // 16 + 1, im_w // 16 + 1, 3))
            img = np.repeat(np.repeat(blocks, 16, axis=0), 16, axis=1)[:im_h, :im_w] + rng.integers(-30, 31, (im_h, im_w, 3))
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(root, folder, "image_02/data/%010d%s" % (i, ext)))
            scan(rng, 900, down).tofile(os.path.join(root, folder, "4beam/%010d.bin" % i))
            if full_scans:
                scan(rng, 5000, down).tofile(os.path.join(root, folder, "velodyne_points/data/%010d.bin" % i))
        lines += ["%s %d l" % (folder, i) for i in range(1, frames - 1)]
    return lines


def depth_like(rng, h, w):
    """A float32 [h,w] map with depth-like values in (0, 80) and some exact zeros."""
    m = rng.uniform(0.05, 80.0, (h, w)).astype(np.float32)
    m[rng.random((h, w)) < 0.03] = 0.0
    return m


def gdc_path(root, line, folder="inf_gdc_4beam"):
    drive, frame, side = line.split()
    return os.path.join(root, drive, folder, "%d_%s.npy" % (int(frame), side))


def write_gdc_maps(root, lines, sizes, seed=5, folder="inf_gdc_4beam"):
    """One ``inf_gdc`` map per split line, of its date's image size (``sizes``: date -> (h, w)) -> {line: map}."""
    rng = np.random.default_rng(seed)
    maps = {}
    for line in lines:
        h, w = sizes[line.split("/")[0]]
        maps[line] = depth_like(rng, h, w)
        path = gdc_path(root, line, folder)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, maps[line])
    return maps


def reference_gdc(path, do_flip, size):
    """kitti_dataset.py:166-173 on the CPU, at ``size`` instead of its hardcoded [192, 640]."""
    import torch
    import torch.nn.functional as F
    gdc = torch.from_numpy(np.load(path).astype(np.float32))
    gdc = F.interpolate(gdc.unsqueeze(0).unsqueeze(0), list(size), mode="bilinear", align_corners=False).squeeze()
    if do_flip:
        gdc = torch.fliplr(gdc)
    return gdc.numpy()
