"""A synthetic KITTI object-detection tree for tests/test_gpu_detection.py, next to a raw-layout tree that holds the SAME files: the raw
tree comes from ``kitti_tree.make_tree`` (``<date>/<drive>`` folders, 10-digit names), the object tree copies its frames into ONE
folder under 6-digit names (``training/image_02/data/000003.png`` ...) and its calibration into ``<root>/<date>``.  A helper, not a test."""
import os
import shutil

import kitti_tree

# date -> image size: two of the five sizes ``detec_calib_date`` knows
DATES = [("2011_09_26", "2011_09_26_drive_0001_sync", (375, 1242)), ("2011_09_28", "2011_09_28_drive_0002_sync", (370, 1224))]
FOLDER = "training"


def make_trees(raw_root, obj_root, frames_per_date=2, down=0.35, seed=77):
    """-> (raw lines, object lines, dates): line i of either list names the same image and scans; object frame indices run over the
    dates' frames in order."""
    kitti_tree.make_tree(raw_root, [(date, drive, size, (1.0, 1.0)) for date, drive, size in DATES], frames=frames_per_date, down=down, seed=seed)
    raw_lines, obj_lines, dates = [], [], []
    for sub in ("image_02/data", "4beam", "velodyne_points/data"):
        os.makedirs(os.path.join(obj_root, FOLDER, sub))
    k = 0
    for date, drive, _ in DATES:
        shutil.copytree(os.path.join(raw_root, date), os.path.join(obj_root, date), ignore=lambda d, names: [n for n in names if "drive" in n])
        for i in range(frames_per_date):
            src = os.path.join(raw_root, date, drive)
            for sub, ext in (("image_02/data", ".png"), ("4beam", ".bin"), ("velodyne_points/data", ".bin")):
                shutil.copyfile(os.path.join(src, sub, "%010d%s" % (i, ext)), os.path.join(obj_root, FOLDER, sub, "%06d%s" % (k, ext)))
            raw_lines.append("%s/%s %d l" % (date, drive, i))
            obj_lines.append("%s %d l" % (FOLDER, k))
            dates.append(date)
            k += 1
    return raw_lines, obj_lines, dates
