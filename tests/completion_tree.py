"""A synthetic KITTI depth-completion tree for the loader / scorer tests, seeded like tests/kitti_tree.py: ``data_rgb``,
``data_depth_velodyne`` and ``data_depth_annotated`` for ``train`` and ``val``, ``depth_selection/val_selection_cropped`` and
``depth_selection/test_depth_completion_anonymous``.  Frames come in three of KITTI's sizes: 375x1242, 376x1241 (odd crop and pad
remainders; its crop column is the round-half-even case, 12) and 370x1226.  Depth PNGs are 16-bit (``Image.fromarray(uint16)`` is
mode ``I;16``), sparse maps about 3 % dense, ground truth about 10 %, with points within 2 pixels of the crop's edges and of the
2-channel scatter's window.  ``make_tree`` is deterministic: the golden generator and the tests build the same files."""
import os

import numpy as np

SIZES = {"2011_09_26_drive_0001_sync": (375, 1242), "2011_09_28_drive_0002_sync": (376, 1241), "2011_09_30_drive_0003_sync": (370, 1226)}
TRAIN_FRAMES = {"2011_09_26_drive_0001_sync": [5, 6, 7, 8, 9, 10],                   # 5 and 10 lack a sparse neighbour
                "2011_09_28_drive_0002_sync": [5, 6, 7, 9, 10, 11],                  # no frame 8: only 6 and 10 keep both neighbours
                "2011_09_30_drive_0003_sync": [5, 6, 7, 8]}
TRAIN_KEPT = {"2011_09_26_drive_0001_sync": [6, 7, 8, 9], "2011_09_28_drive_0002_sync": [6, 10], "2011_09_30_drive_0003_sync": [6, 7]}
VAL_DRIVE = "2011_10_03_drive_0004_sync"
VAL_FRAMES = [5, 6, 7]
VAL_SIZE = (370, 1224)
EIGHT_BIT_FRAME = 7                                          # the val sparse file whose maximum is <= 255
SELECT = [("2011_09_26_drive_0002_sync", 5, (352, 1216)), ("2011_09_26_drive_0005_sync", 13, (352, 1216)),
          ("2011_09_28_drive_0037_sync", 21, (376, 1241))]
TEST = [(0, (352, 1216)), (1, (375, 1242))]
CROP = (352, 1216)
ROI = (110, 350, 2, 1214)


def image(rng, h, w):
    blocks = rng.integers(0, 256, (h // 16 + 1, w // 16 + 1, 3))
    img = np.repeat(np.repeat(blocks, 16, axis=0), 16, axis=1)[:h, :w] + rng.integers(-30, 31, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def depth_png(rng, h, w, density):
    """uint16 [h,w]: depth * 256 of 1 .. 80 m at ``density`` of the pixels, the codes 1, 255, 256 and 65535 among them, plus points
    within 2 pixels of the crop's edges and of the scatter window's edges (in cropped coordinates)."""
    codes = rng.integers(256, 80 * 256, (h, w)).astype(np.uint16)
    out = np.where(rng.random((h, w)) < density, codes, 0).astype(np.uint16)
    i, j = h - CROP[0], int(round((w - CROP[1]) / 2.))
    rows = [0, 1, ROI[0] - 2, ROI[0] - 1, ROI[0], ROI[0] + 1, ROI[1] - 2, ROI[1] - 1, ROI[1], CROP[0] - 1]
    cols = [0, 1, ROI[2], ROI[2] + 1, ROI[3] - 2, ROI[3] - 1, ROI[3], CROP[1] - 1]
    for r in rows:
        for c in rng.integers(0, CROP[1], 6):
            out[i + r, j + c] = codes[i + r, j + c]
    for c in cols:
        for r in rng.integers(0, CROP[0], 6):
            out[i + r, j + c] = codes[i + r, j + c]
    out[i + 200, j + 300:j + 304] = (1, 255, 256, 65535)
    return out


def _save(path, array):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(array).save(path)


def make_tree(root, seed=99):
    """Writes the tree under ``root`` (the ``data_folder`` of ``completion_paths``)."""
    rng = np.random.default_rng(seed)
    for split, drives in (("train", TRAIN_FRAMES), ("val", {VAL_DRIVE: VAL_FRAMES})):
        for drive, frames in drives.items():
            h, w = SIZES.get(drive, VAL_SIZE)
            for n in range(min(frames) - 1, max(frames) + 2):    # colour frames include the neighbours of the first and last
                _save(os.path.join(root, "data_rgb", split, drive, "image_02/data/%010d.png" % n), image(rng, h, w))
            for n in frames:
                sparse = depth_png(rng, h, w, 0.03)
                if split == "val" and n == EIGHT_BIT_FRAME:
                    sparse = np.minimum(sparse, 255).astype(np.uint16)
                _save(os.path.join(root, "data_depth_velodyne", split, drive, "proj_depth/velodyne_raw/image_02/%010d.png" % n), sparse)
                _save(os.path.join(root, "data_depth_annotated", split, drive, "proj_depth/groundtruth/image_02/%010d.png" % n),
                      depth_png(rng, h, w, 0.10))
    sel = os.path.join(root, "depth_selection/val_selection_cropped")
    for drive, n, (h, w) in SELECT:
        name = "%s_%s_%010d_image_02.png"
        _save(os.path.join(sel, "image", name % (drive, "image", n)), image(rng, h, w))
        _save(os.path.join(sel, "velodyne_raw", name % (drive, "velodyne_raw", n)), depth_png(rng, h, w, 0.03))
        _save(os.path.join(sel, "groundtruth_depth", name % (drive, "groundtruth_depth", n)), depth_png(rng, h, w, 0.10))
    tst = os.path.join(root, "depth_selection/test_depth_completion_anonymous")
    for n, (h, w) in TEST:
        _save(os.path.join(tst, "image/%010d.png" % n), image(rng, h, w))
        _save(os.path.join(tst, "velodyne_raw/%010d.png" % n), depth_png(rng, h, w, 0.03))
    return root


def options(**kw):
    """The options the completion loader reads, with the reference's defaults."""
    import types
    o = dict(completion_not_full_res=False, completion_test=False, completion_need2channel="false", need_4beam=True, eval_gdc=False,
             need_path=False, inf=False)
    o.update(kw)
    return types.SimpleNamespace(**o)
