"""``python -m fusiondepth_amd.inf_gdc``: the Refiner's ``inf_gdc`` targets, inf_gdc.py of the reference on the GPU.

For every split line ``<date>/<drive> <frame> <side>``:
  1. the stage-1 disparity ``inf_depth_{n}beam/{frame}_{side}.npy`` (``inf_depth_r{N}`` with --random_sample N) -> [0][0],
  2. ``disp_to_depth(., 0.1, 100)`` -> scaled disparity, resized to the LiDAR map's size (OpenCV's INTER_LINEAR rule), 1 / x,
  3. Eigen mask + Garg crop, median ratio np.median(lidar) / np.median(depth) (float64), depth * ratio rounded to float32,
  4. LiDAR map: ``{n}beam/{frame:010d}.bin`` (``random{N}``) rasterised like generate_depth_map(calib_dir, scan, 2, True),
     0 -> -1,
  5. ``GDC(depth, lidar, Calibration(calib_cam_to_cam.txt), W_tol=3e-5, recon_tol=5e-4, k=10, method='cg')`` with the pitch
     range (-0.1, 4.0) for beams and (-1.5, 9) for random samples,
  6. ``np.save(inf_gdc_{n}beam/{frame}_{side}.npy)`` (``inf_gdc_r{N}``): float32 [H, W].
A frame whose GDC fails keeps the scaled depth, as in the reference.  Frames run one after another on one GPU; file reading
and writing overlap the GPU work on a small thread pool.
"""
import argparse
import concurrent.futures
import os
import time

import numpy as np
import torch

from . import functional as FD
from .evaluate_depth import _median, garg_crop
from .gdc import GDC
from .kitti_utils import Calibration, load_velodyne_points, velo_to_image

DEFAULT_SPLITS = ("splits/eigen_zhou/train_files.txt", "splits/eigen/test_files.txt")     # inf_gdc.py:20-28


def parse_args(argv=None):
    p = argparse.ArgumentParser("python -m fusiondepth_amd.inf_gdc", description="Graph-based depth correction of stage-1 depth "
                                "against sparse LiDAR: writes the inf_gdc_* maps the Refiner trains against")
    p.add_argument("--data_path", default="kitti_data/", help="KITTI raw root")
    p.add_argument("--split_files", nargs="+", default=list(DEFAULT_SPLITS), help="split files whose lines are processed")
    p.add_argument("--nbeams", type=int, default=4)
    p.add_argument("--random_sample", type=int, default=-1)
    p.add_argument("--workers", type=int, default=8, help="file-reading / writing threads (at most 16)")
    return p.parse_args(argv)


def frame_paths(args, line):
    folder, idx, side = line.split()[:3]
    idx = int(idx)
    tag = "r{}".format(args.random_sample) if args.random_sample > 0 else "{}beam".format(args.nbeams)
    scan_dir = "random{}".format(args.random_sample) if args.random_sample > 0 else "{}beam".format(args.nbeams)
    base = os.path.join(args.data_path, folder)
    calib_dir = os.path.join(args.data_path, folder.split("/")[0])
    return dict(calib_dir=calib_dir, scan=os.path.join(base, scan_dir, "{:010d}.bin".format(idx)),
                disp=os.path.join(base, "inf_depth_" + tag, "{}_{}.npy".format(idx, side)),
                out_dir=os.path.join(base, "inf_gdc_" + tag), out=os.path.join(base, "inf_gdc_" + tag, "{}_{}.npy".format(idx, side)))


def load_frame(paths):
    """Host part of one frame: calibration, the scan, the disparity (runs on the thread pool)."""
    P, (im_h, im_w) = velo_to_image(paths["calib_dir"], 2)
    calib = Calibration(os.path.join(paths["calib_dir"], "calib_cam_to_cam.txt"))
    scan = load_velodyne_points(paths["scan"])
    disp = np.load(paths["disp"])[0][0]
    return P, (im_h, im_w), calib, scan, disp


def scaled_depth(disp, lidar):
    """Steps 2-3: [h,w] disparity (device) and the float64 LiDAR map -> the median-scaled float32 depth at the LiDAR's size."""
    gh, gw = lidar.shape
    scaled, _ = FD.disp_to_depth(FD.f32(disp), 0.1, 100.0)
    depth = 1.0 / FD.resize_linear_cv(scaled[None, None], (gh, gw))[0, 0]
    mask = (lidar > 1e-3) & (lidar < 80)
    c = garg_crop(gh, gw)
    crop = torch.zeros_like(mask)
    crop[c[0]:c[1], c[2]:c[3]] = True
    mask = mask & crop
    ratio = _median(lidar[mask]) / _median(depth[mask]).double()
    return (depth.double() * ratio).float()


def correct_frame(frame, random_sample=-1, device="cuda"):
    """Steps 2-5 on the device for one loaded frame -> (float32 [H,W] device map, GDCInfo or None when the frame failed)."""
    P, (im_h, im_w), calib, scan, disp = frame
    lidar = FD.velo_rasterize(torch.from_numpy(scan).to(device), P, im_h, im_w, None, return_full=True, vel_depth=True, beam=False)
    depth = scaled_depth(torch.as_tensor(disp).to(device), lidar)
    lidar[lidar == 0] = -1
    consider_range = (-0.1, 4.0) if random_sample == -1 else (-1.5, 9)
    out, info = GDC(depth, lidar, calib, W_tol=3e-5, recon_tol=5e-4, k=10, method="cg", consider_range=consider_range,
                    return_info=True)
    return out, info


def main(argv=None):
    args = parse_args(argv)
    lines = []
    for f in args.split_files:
        with open(f) as fh:
            lines += [ln for ln in fh.read().splitlines() if ln.strip()]
    torch.cuda.set_device(0)
    workers = max(1, min(16, args.workers))
    failed = 0
    t0 = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
        loads = [pool.submit(load_frame, frame_paths(args, ln)) for ln in lines[:workers]]
        saves = []
        for i, line in enumerate(lines):
            paths = frame_paths(args, line)
            frame = loads[i].result()
            if i + workers < len(lines):
                loads.append(pool.submit(load_frame, frame_paths(args, lines[i + workers])))
            loads[i] = None
            out, info = correct_frame(frame, args.random_sample)
            if info.status == "failed":
                failed += 1
                print("GDC failed: %s" % line)
            os.makedirs(paths["out_dir"], exist_ok=True)
            saves.append(pool.submit(np.save, paths["out"], out.cpu().numpy()))
        for s in saves:
            s.result()
    dt = time.perf_counter() - t0
    print("inf_gdc: %d frames in %.2f s (%.2f frames/s), %d failed" % (len(lines), dt, len(lines) / max(dt, 1e-9), failed))
    return failed


if __name__ == "__main__":
    main()
