"""Raw Velodyne scans -> the sparse ``{n}beam/`` and ``random{N}/`` scans the reference trains on, on the GPU: the reference's
``sparsify/sparsify.py`` as a library call and as a drop-in command line.

    python -m fusiondepth_amd.sparsify --W 1024 --H 64 --line_spec 2 7 12 16 --split_file splits/eigen_zhou/train_files.txt

takes the ``sparsify.py`` lines of the reference's ``prepare_*beam*.sh`` / ``prepare_r{100,200}.sh`` scripts as they are and writes the
same folders and file names (``<output_path><folder>/{nbeams}beam/%010d.bin`` or ``.../random{N}/%010d.bin``).  Files are read and
written on a host thread pool (``--threads``, at most 16); the scans go to the device in batches (``--batch``) and each batch is one
``fd_sparsify_scans`` call.

Arithmetic: numpy 2's evaluation of the reference (``data_ops.sparsify_scans``); only ``arcsin`` is not matched bit for bit, so a point
within a few float32 spacings of a bin edge may land in the neighbouring cell.  ``--random_sample`` draws from the
library's counter-based generator keyed by (``--seed``, folder, frame index): the reference's ``np.random`` draws depend on the
order its process pool happens to work in and are not reproduced; their distribution is.

Refused: ``--fill_in_map_dir`` / ``--fill_in_spec`` / ``--fill_in_slice`` (the line maps they paste in come from ``--store_line_map_dir``
runs of the reference, float64 ``.npy`` files this tool does not write), ``--store_line_map_dir`` (a debugging dump of the full
angular grid; no consumer in the training path) and ``--visualize`` (needs open3d and a display).
"""
import argparse
import concurrent.futures
import hashlib
import os

import numpy as np
import torch

from . import data_ops

REFUSED = {
    "fill_in_map_dir": "line maps are float64 .npy dumps of the reference's --store_line_map_dir runs, which this tool does not write",
    "fill_in_spec": "it pastes rows of a --fill_in_map_dir line map into the grid, and line maps are not covered",
    "fill_in_slice": "it pastes rows of a --fill_in_map_dir line map into the grid, and line maps are not covered",
    "store_line_map_dir": "the full angular grid is a debugging dump nothing in training or evaluation reads",
    "visualize": "it needs open3d and a display; this tool writes files only",
}


def scan_key(folder, frame_index):
    """The 64-bit key of a scan for the random-sample generator: a function of its folder and frame index alone."""
    digest = hashlib.blake2b(("%s %d" % (folder, int(frame_index))).encode(), digest_size=8).digest()
    return int.from_bytes(digest, "little")


def load_scan(path):
    """A KITTI Velodyne file -> float32 [n,4]."""
    return np.fromfile(path, dtype=np.float32).reshape(-1, 4)


def sparsify(points, H=64, W=1024, line_spec=None, slice=1, random_sample=0, uniforms=None, seed=0, key=0):
    """One scan ([n,4], CUDA tensor or numpy array) -> the compacted [m,4] float32 CUDA tensor ``gen_sparse_points`` returns."""
    if not torch.is_tensor(points):
        points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).cuda()
    slab, counts = data_ops.sparsify_scans([points], H, W, line_spec, slice, random_sample,
                                     None if uniforms is None else [uniforms], seed, [key])
    return slab[0, :int(counts[0])].clone()


def build_parser():
    """The reference's flags (sparsify.py:192-218) plus --seed and --batch."""
    p = argparse.ArgumentParser("Generate sparse pseudo-LiDAR points on the GPU")
    p.add_argument("--calib_path", type=str, help="accepted for compatibility; unused, as in the reference")
    p.add_argument("--image_path", type=str, help="accepted for compatibility; unused, as in the reference")
    p.add_argument("--ptc_path", type=str, default="../kitti_data/", help="path to point cloud files")
    p.add_argument("--output_path", type=str, default="../kitti_data/", help="path to sparsed point cloud files")
    p.add_argument("--slice", default=1, type=int)
    p.add_argument("--H", default=64, type=int)
    p.add_argument("--W", default=512, type=int)
    p.add_argument("--D", default=700, type=int, help="accepted for compatibility; unused, as in the reference")
    p.add_argument("--store_line_map_dir", type=str, default=None)
    p.add_argument("--line_spec", type=int, nargs="+", default=None)
    p.add_argument("--fill_in_map_dir", type=str, default=None)
    p.add_argument("--fill_in_spec", type=int, nargs="+", default=None)
    p.add_argument("--fill_in_slice", type=int, default=None)
    p.add_argument("--split_file", type=str)
    p.add_argument("--threads", type=int, default=20, help="host threads for file reads and writes (capped at 16)")
    p.add_argument("--random_sample", type=int, default=0)
    p.add_argument("--visualize", action="store_true")
    p.add_argument("--nbeams", default=4, type=int)
    p.add_argument("--seed", type=int, default=0, help="seed of the random-sample generator (with the scan's folder and frame index)")
    p.add_argument("--batch", type=int, default=32, help="scans per device call")
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    for name, why in REFUSED.items():
        if getattr(args, name):
            raise NotImplementedError("--%s is not covered: %s" % (name, why))
    if not args.split_file:
        raise ValueError("--split_file is required")
    args.threads = max(1, min(int(args.threads), 16))
    return args


def output_folder(args, folder):
    """sparsify.py:129-132."""
    sub = "{}beam/".format(args.nbeams) if args.random_sample == 0 else "random{}/".format(args.random_sample)
    return args.output_path + folder + "/" + sub


def split_entries(split_file):
    """[(folder, frame index)] of the non-empty lines."""
    with open(split_file) as f:
        return [(l.split()[0], int(l.split()[1])) for l in f.readlines() if len(l.strip()) > 0]


def input_path(args, folder, frame_index):
    return os.path.join(args.ptc_path + folder + "/velodyne_points/data", "{:010d}.bin".format(frame_index))


def _write(path, array):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    array.tofile(path)


def run(args, device="cuda"):
    """Process every line of the split file; returns the number of scans written."""
    entries = split_entries(args.split_file)
    os.makedirs(args.output_path, exist_ok=True)
    batch = max(1, int(args.batch))
    done = 0
    with concurrent.futures.ThreadPoolExecutor(max_workers=args.threads) as pool:
        chunks = [entries[i:i + batch] for i in range(0, len(entries), batch)]
        reads = [pool.submit(load_scan, input_path(args, *e)) for e in chunks[0]] if chunks else []
        writes = []
        for ci, chunk in enumerate(chunks):
            scans = [r.result() for r in reads]
            if ci + 1 < len(chunks):                             # the next batch's files are read while this one is on the device
                reads = [pool.submit(load_scan, input_path(args, *e)) for e in chunks[ci + 1]]
            dev = [torch.from_numpy(s).to(device, non_blocking=True) for s in scans]
            slab, counts = data_ops.sparsify_scans(dev, args.H, args.W, args.line_spec, args.slice, args.random_sample, None, args.seed,
                                             [scan_key(*e) for e in chunk])
            counts = counts.cpu().numpy()
            slab = slab[:, :max(int(counts.max()), 1)].cpu().numpy()
            for w in writes:
                w.result()
            writes = [pool.submit(_write, output_folder(args, folder) + "%010d.bin" % frame, slab[k, :counts[k]].copy())
                      for k, (folder, frame) in enumerate(chunk)]
            done += len(chunk)
        for w in writes:
            w.result()
    return done


def main(argv=None):
    args = parse_args(argv)
    n = run(args)
    print("%d scans -> %s" % (n, "random%d/" % args.random_sample if args.random_sample else "%dbeam/" % args.nbeams))


if __name__ == "__main__":
    main()
