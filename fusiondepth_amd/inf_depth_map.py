"""``python -m fusiondepth_amd.inf_depth_map``: the stage-1 disparity maps ``python -m fusiondepth_amd.inf_gdc`` corrects,
inf_depth_map.py of the reference on the GPU.

For every split line ``<date>/<drive> <frame> <side>`` the frozen stage-1 networks of ``--load_weights_folder`` (``Trainer.save_model``
output) run on the item ``KITTIRAWBatches`` builds for it (frame 0 alone, no augmentation, ``4beam`` / ``2channel`` / ``path`` keys), and
``outputs[("disp", 0)]`` of the item is saved as float32 [1, 1, H, W] to ``inf_depth_{n}beam/{frame}_{side}.npy`` (``inf_depth_r{N}``
with --random_sample N) in the drive's folder under ``--data_path`` (the reference writes under a hardcoded ``kitti_data/``).  The
whole chain from a KITTI raw tree and a checkpoint:

    python -m fusiondepth_amd.inf_depth_map --load_weights_folder log/mdp/models/weights_19 --data_path kitti_data
    python -m fusiondepth_amd.inf_gdc --data_path kitti_data
    Refiner(opts).train(KITTIRefinerBatches(...))

Batches are built and consumed on one GPU; the ``.npy`` files are written on a small thread pool beside the GPU work.
"""
import argparse
import collections
import concurrent.futures
import os
import time
import types

import numpy as np
import torch

from .inf_gdc import DEFAULT_SPLITS


def parse_args(argv=None):
    p = argparse.ArgumentParser("python -m fusiondepth_amd.inf_depth_map", description="Stage-1 disparity of every split line: writes the "
                                "inf_depth_* maps that python -m fusiondepth_amd.inf_gdc reads")
    p.add_argument("--load_weights_folder", required=True, help="folder with encoder.pth, beam_encoder.pth, depth.pth")
    p.add_argument("--data_path", default="kitti_data/", help="KITTI raw root")
    p.add_argument("--split_files", nargs="+", default=list(DEFAULT_SPLITS), help="split files whose lines are processed")
    p.add_argument("--nbeams", type=int, default=4)
    p.add_argument("--random_sample", type=int, default=-1)
    p.add_argument("--png", action="store_true", help="frames are .png (default .jpg)")
    p.add_argument("--num_layers", type=int, default=50, choices=[18, 34, 50, 101, 152])
    p.add_argument("--height", type=int, default=192)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--batch_size", type=int, default=1, help="items per forward pass (the reference: 1)")
    p.add_argument("--workers", type=int, default=8, help="decoding / file-writing threads (at most 16)")
    p.add_argument("--lidar_source", default="files", choices=["files", "raw"],
                   help="files: the sparse scans an offline sparsifier wrote; raw: sparsify velodyne_points on the device")
    return p.parse_args(argv)


def read_lines(split_files):
    lines = []
    for f in split_files:
        with open(f) as fh:
            lines += [ln for ln in fh.read().splitlines() if ln.strip()]
    return lines


def out_path(args, line):
    """inf_depth_map.py:140-153 under ``--data_path``; the path ``inf_gdc.frame_paths`` reads."""
    folder, idx, side = line.split()[:3]
    tag = "r{}".format(args.random_sample) if args.random_sample > 0 else "{}beam".format(args.nbeams)
    return os.path.join(args.data_path, folder, "inf_depth_" + tag, "{}_{}.npy".format(int(idx), side))


def loader_options(args):
    """The dataset options inf_depth_map.py runs with (its command line: --need_path; need_4beam / need_2_channel default on)."""
    return types.SimpleNamespace(need_4beam=True, need_2_channel=True, need_path=True, need_full_res_4beam=False, need_inf_gdc=False,
                                 clone_gdc=False, nbeams=args.nbeams, random_sample=args.random_sample)


def _save(path, array):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.save(path, array)


def main(argv=None):
    args = parse_args(argv)
    if args.height % 32 or args.width % 32:
        raise ValueError("'height' / 'width' must be multiples of 32")
    from .datasets import KITTIRAWBatches
    from .predict import Predictor
    lines = read_lines(args.split_files)
    torch.cuda.set_device(0)
    predictor = Predictor(args.load_weights_folder, num_layers=args.num_layers)
    workers = max(1, min(16, args.workers))
    loader = KITTIRAWBatches(args.data_path, lines, args.height, args.width, [0], 4, is_train=False, img_ext=".png" if args.png else ".jpg",
                             opt=loader_options(args), batch_size=args.batch_size, workers=workers, lidar_source=args.lidar_source,
                             drop_last=False)
    t0 = time.perf_counter()
    done = 0
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
        saves = collections.deque()
        for batch in loader:
            disp = predictor.predict(batch)[("disp", 0)].cpu().numpy()
            for k, line in enumerate(batch["path"]):
                saves.append(pool.submit(_save, out_path(args, line), np.ascontiguousarray(disp[k:k + 1], dtype=np.float32)))
            done += len(batch["path"])
            while len(saves) > 4 * workers:                      # bounded: slow storage holds the loop back instead of queueing
                saves.popleft().result()                         # every map in memory, and a failed save ends the run here
        for s in saves:
            s.result()
    loader.close()
    dt = time.perf_counter() - t0
    print("inf_depth_map: %d frames in %.2f s (%.2f frames/s)" % (done, dt, done / max(dt, 1e-9)))
    return 0


if __name__ == "__main__":
    main()
