"""numpy restatement of the reference's depth-completion data path and scorer, pinned bit for bit against what the reference
itself returns (tests/golden/completion_*.npz, tests/test_completion_cpu.py) and used by the GPU tests at shapes the golden does
not hold: ``get_paths_and_transform`` (completion_dataset.py:22-139), ``get_color`` / ``get_depth`` (kitti_completion.py:29-80), the
item schema (completion_dataset.py:272-369) and ``compute_errors`` (evaluate_completion.py:31-48).  Colour resampling and jitter go
through tests/augment_ref.py."""
import glob
import os

import numpy as np

import augment_ref as AR

CROP = (352, 1216)
PAD = (384, 1280)


def completion_paths(data_folder, split, val_split="select", verify=True):
    j = os.path.join
    get_rgb = glob_rgb = glob_gt = glob_d = None
    if split == "train":
        glob_d = j(data_folder, "data_depth_velodyne/train/*_sync/proj_depth/velodyne_raw/image_0[2,3]/*.png")
        glob_gt = j(data_folder, "data_depth_annotated/train/*_sync/proj_depth/groundtruth/image_0[2,3]/*.png")
        get_rgb = lambda p: "/".join([data_folder, "data_rgb"] + p.split("/")[-6:-4] + p.split("/")[-2:-1] + ["data"] + p.split("/")[-1:])
    elif split == "val" and val_split == "full":
        glob_d = j(data_folder, "data_depth_velodyne/val/*_sync/proj_depth/velodyne_raw/image_0[2,3]/*.png")
        glob_gt = j(data_folder, "data_depth_annotated/val/*_sync/proj_depth/groundtruth/image_0[2,3]/*.png")
        get_rgb = lambda p: "/".join(p.split("/")[:-7] + ["data_rgb"] + p.split("/")[-6:-4] + p.split("/")[-2:-1] + ["data"] + p.split("/")[-1:])
    elif split == "val" and val_split == "select":
        glob_d = j(data_folder, "depth_selection/val_selection_cropped/velodyne_raw/*.png")
        glob_gt = j(data_folder, "depth_selection/val_selection_cropped/groundtruth_depth/*.png")
        get_rgb = lambda p: p.replace("groundtruth_depth", "image")
    elif split == "test_completion":
        glob_d = j(data_folder, "depth_selection/test_depth_completion_anonymous/velodyne_raw/*.png")
        glob_rgb = j(data_folder, "depth_selection/test_depth_completion_anonymous/image/*.png")
    elif split == "test_prediction":
        glob_rgb = j(data_folder, "depth_selection/test_depth_prediction_anonymous/image/*.png")
    else:
        raise ValueError("Unrecognized split " + str(split))
    if glob_gt is not None:
        d, gt = sorted(glob.glob(glob_d)), sorted(glob.glob(glob_gt))
        rgb = [get_rgb(p) for p in gt]
    else:
        rgb = sorted(glob.glob(glob_rgb))
        gt = [None] * len(rgb)
        d = [None] * len(rgb) if split == "test_prediction" else sorted(glob.glob(glob_d))
    if verify and split == "train":
        def near(p, k):
            head, tail = os.path.split(p)
            return os.path.isfile(j(head, "%010d.png" % (int(tail[:tail.find(".")]) + k)))
        keep = [i for i in range(len(d)) if near(d[i], -1) and near(d[i], 1)]
        d, rgb, gt = [d[i] for i in keep], [rgb[i] for i in keep], [gt[i] for i in keep]
    if not d and not rgb and not gt:
        raise RuntimeError("Found 0 images under {}".format(glob_gt))
    if len(rgb) != len(d) or len(rgb) != len(gt):
        raise RuntimeError("Produced different sizes for datasets")
    return {"rgb": rgb, "d": d, "gt": gt}


def bottom_crop(a):
    h, w = a.shape[:2]
    i, j = h - CROP[0], int(round((w - CROP[1]) / 2.))
    return a[i:i + CROP[0], j:j + CROP[1]]


def pad(a):
    ypad, xpad = PAD[0] - a.shape[0], PAD[1] - a.shape[1]
    return np.pad(a, ((ypad, 0), (xpad // 2, xpad - xpad // 2)) + ((0, 0),) * (a.ndim - 2))


def load_png(path):
    from PIL import Image
    with Image.open(path) as img:
        return np.array(img if img.mode != "P" else img.convert("RGB"))


def get_color(rgb, do_flip, not_full_res):
    """kitti_completion.py:29-49 on a decoded [H,W,3] uint8 frame."""
    if do_flip:
        rgb = rgb[:, ::-1]
    if not_full_res:
        rgb = pad(rgb)
    else:
        rgb = bottom_crop(rgb)
    return np.ascontiguousarray(rgb)


def max_pool_ceil(a):
    """F.max_pool2d(a, 2, ceil_mode=True) of a 2-D map."""
    h, w = a.shape
    big = np.full(((h + 1) // 2 * 2, (w + 1) // 2 * 2), -np.inf, a.dtype)
    big[:h, :w] = a
    return big.reshape(big.shape[0] // 2, 2, big.shape[1] // 2, 2).max(axis=(1, 3))


def get_depth(png, do_flip, not_full_res, padding=True, pool=True):
    """kitti_completion.py:51-80 on the decoded integer map -> float32 [1,h,w]."""
    assert png.max() > 255
    depth = png.astype(np.float32) / 256.
    if do_flip:
        depth = np.fliplr(depth)
    if not not_full_res:
        depth = bottom_crop(depth).copy()
    if padding:
        depth = pad(depth)
    if pool:
        depth = max_pool_ceil(depth)
    return np.ascontiguousarray(depth)[None]


def colour_keys(frames, height, width, num_scales, jitter):
    """completion_dataset.py:248-267 for the cropped / padded frames {frame id: uint8 image}; ``jitter`` = (factors, order) or None."""
    out = {}
    for f, img in frames.items():
        for s, lvl in enumerate(AR.pyramid(img, height, width, num_scales)):
            out[("color", f, s)] = AR.to_planes(lvl)
            out[("color_aug", f, s)] = AR.to_planes(AR.color_jitter(lvl, *jitter)) if jitter is not None else out[("color", f, s)]
    return out


def depth_keys(paths, index, opt, is_train, frame_idxs, do_flip):
    """The depth keys of item ``index`` (completion_dataset.py:310-367) with ``completion_need2channel == "false"``."""
    nfr = opt.completion_not_full_res
    out = {}
    d = paths["d"][index]
    if is_train:
        head_d, tail = os.path.split(d)
        n = int(tail[:tail.find(".")])
        for f in frame_idxs:
            sparse = get_depth(load_png(os.path.join(head_d, "%010d.png" % (n + f))), do_flip, nfr, nfr, nfr) / np.float32(100.0)
            out[("2channel", f, 0)] = np.stack([sparse[0], sparse[0]])
    if not opt.completion_test:
        out["depth_gt"] = get_depth(load_png(paths["gt"][index]), do_flip, nfr, nfr, False)
    if opt.need_4beam:
        out["4beam"] = get_depth(load_png(d), do_flip, nfr, nfr, nfr) / np.float32(100.0)
        if opt.eval_gdc:
            out["full_res_4beam"] = get_depth(load_png(d), do_flip, nfr, True, False)
        out["2channel"] = np.stack([out["4beam"][0], out["4beam"][0]])
    return out


def item(paths, index, opt, is_train, frame_idxs, height, width, num_scales, do_flip=False, jitter=None):
    """One item of the reference's dataset as numpy arrays (K / inv_K left out: they are ``KITTIRAWBatches``')."""
    nfr = opt.completion_not_full_res
    rgb = paths["rgb"][index]
    frames = {}
    if is_train:
        head, tail = os.path.split(rgb)
        n = int(tail[:tail.find(".")])
        for f in frame_idxs:
            frames[f] = get_color(load_png(os.path.join(head, "%010d.png" % (n + f))), do_flip, nfr)
    else:
        frames[0] = get_color(load_png(rgb), do_flip, nfr)
    out = colour_keys(frames, height, width, num_scales, jitter)
    out.update(depth_keys(paths, index, opt, is_train, frame_idxs, do_flip))
    return out


def error_terms(gt, pred):
    """The two float32 difference maps the scorer averages: millimetres, and inverse kilometres."""
    gt, pred = gt.astype(np.float32), pred.astype(np.float32)
    d = gt * np.float32(1000.0) - pred * np.float32(1000.0)
    di = np.float32(1.0) / (gt * np.float32(0.001)) - np.float32(1.0) / (pred * np.float32(0.001))
    return d, di


def compute_errors(gt, pred):
    """(rmse, mae, irmse, imae) with numpy's own float32 means of the float32 terms; pinned to what the reference's
    compute_errors returned by tests/golden/completion_metrics.npz."""
    d, di = error_terms(gt, pred)
    return np.sqrt((d * d).mean()), np.abs(d).mean(), np.sqrt((di * di).mean()), float(np.abs(di).mean())


def compute_errors_f64_sums(gt, pred):
    """The same float32 terms, the four means taken in float64."""
    d, di = error_terms(gt, pred)
    m = lambda v: v.astype(np.float64).mean() if v.size else np.float64("nan")
    return np.sqrt(m(d * d)), m(np.abs(d)), np.sqrt(m(di * di)), m(np.abs(di))


def scored(pred, gt, scale=1.0, median_scaling=True):
    """The per-image recipe of evaluate_completion.py:297-355 (without GDC) -> (ratio or None, compute_errors' inputs (gt, pred))."""
    mask = gt > 0.1
    pred = pred * np.float32(scale)
    ratio = None
    if median_scaling:
        ratio = np.median(gt[mask]) / np.median(pred[mask])
        pred = pred * ratio
    p, g = pred[mask], gt[mask]
    p[p < 1e-3] = 1e-3
    p[p > 80] = 80
    return ratio, g, p
