"""The reference's ``export_detection.py`` on the device: the depth maps of a saved model over the KITTI 3-D object detection set, scored
like ``evaluate_depth`` scores the Eigen split and saved as the 16-bit PNGs a monocular 3-D detector is trained on.

    python -m fusiondepth_amd.export_detection --splits_dir splits --data_path kitti_data --load_weights_folder <folder> \\
        --eval_mono --png --det_name <name> [--refine_2d ...] [--post_process] [--eval_gdc] [--pl_name <name> [--pl_max_high 1.0]]

``evaluate(opt, splits_dir)`` (:77-413): lines from ``<splits_dir>/detection/test.txt``, ``Predictor`` exactly as
``evaluate_depth.evaluate`` constructs it, ``detection.KITTIDetecBatches`` as the loader, ``evaluate_depth.predict_disps`` for the
disparities, ground truth ``<splits_dir>/detection/gt_depths.npz`` (``detection.export_gt_depths_detec`` writes it).
``--post_process``, ``--refine_2d``, ``--save_pred_disps``, ``--no_eval``, ``--ext_disp_to_eval``, ``--eval_stereo`` and
``--eval_split benchmark`` behave as in ``evaluate_depth``, and ``evaluate_depth._refuse_uncovered`` refuses the same options.

  * without ``--eval_gdc``: ``evaluate_depth.eigen_scores`` gives the metrics and the per-image ratios, and ``detection.depth_export``
    is called with THOSE ratios - the saved map and the scored map cannot disagree.
  * with ``--eval_gdc``: batch size 1 as in the reference, beams from ``4beam.npz`` (``r{N}.npz`` with ``--random_sample N``), the camera
    from ``<data_path>/<date>/calib_cam_to_cam.txt``; scoring goes through ``evaluate_depth.evaluate_predictions`` and its ``on_depth``
    callback quantises each corrected map (``detection.quantize_u16``).
  * the maps go to ``<data_path>/<folder of the line>/<det_name>/{:06d}.png``, written with PIL on a pool of at most 16 host threads
    while the next chunk runs on the device.  ``--png_encoder device`` (this script's flag; ``evaluate(..., png_encoder="device")``;
    default ``pil``): the uint16 payload stays on the device and ``image_codecs.encode_png_batch`` encodes it there, chunk by chunk (one
    map at a time with ``--eval_gdc``); the pool writes the files from the encoder's pinned buffer.  The files differ from Pillow's in
    their bytes, not in a single decoded value; maps, scores and clouds are untouched.  As in the reference (:388), the map is saved BEFORE the [1e-3, 80] clamp of the scorer.

  * ``--pl_name NAME [--pl_max_high F]`` (this script's flags, taken off the command line like ``--splits_dir``): next to each PNG a
    pseudo-LiDAR cloud ``<data_path>/<folder of the line>/<pl_name>/{:06d}.bin`` (float32 x, y, z, 1 in the Velodyne frame, the input
    of a LiDAR-based detector), by ``detection.points_export`` and the point rule stated there - from the SAME float32 map the PNG is
    quantised from (``depth_export(want_depth=True)`` of the chunk; with ``--eval_gdc`` the corrected map rounded to float32 once),
    with the calibration of the line's recording date.  PNG, score and cloud cannot disagree.  Refused with ``--no_eval`` and
    ``--eval_split benchmark``.

Returns ``(mean_errors[7], ratios, per_image[N,7] or None with --eval_gdc, paths)``, with ``--pl_name`` a fifth element, the ``.bin``
paths; ``None`` after ``--no_eval`` and for the ``benchmark`` split.

Deviations from the reference, on purpose (next to those of ``evaluate_depth`` and ``detection``)
  * the file name is the LINE'S FRAME INDEX.  The reference names the PNG after the loop counter and uses the counter for the GDC
    calibration lookup too; on a split that lists the frames 0, 1, 2, ... in order the two are the same, on any other the reference
    saves frame k under another frame's name.
  * the output folder is ``<data_path>/<folder of the line>/<det_name>`` (the reference hardcodes ``kitti_data/kitti_detect/training``),
    and a missing ``--det_name`` raises ``ValueError`` (the reference writes into a folder called ``None``).
  * values the 16-bit payload cannot hold are defined instead of left to the C cast: NaN and negative -> 0, >= 65535 -> 65535.
  * the clouds are not in the reference at all (its ``project_image_to_velo`` calls a method that is commented out); their two
    deviations from Pseudo-LiDAR - the date's calibration, this project's product order - are stated in ``detection``.
"""
import concurrent.futures
import os
import sys

import numpy as np
import torch

from . import detection
from . import evaluate_depth as ED
from .datasets import parse_line

EXPORT_CHUNK = 64            # images per fd_depth_export call (and per pinned download)


def png_path(data_path, line, det_name):
    folder, frame_index, _ = parse_line(line)
    return os.path.join(data_path, folder, det_name, "{:06d}.png".format(frame_index))


def bin_path(data_path, line, pl_name):
    folder, frame_index, _ = parse_line(line)
    return os.path.join(data_path, folder, pl_name, "{:06d}.bin".format(frame_index))


def _save_bin(path, cloud):
    cloud.tofile(path)
    return path


def _save_png(path, depth_u16):
    from PIL import Image
    Image.fromarray(depth_u16).save(path)
    return path


def _save_bytes(path, data):
    with open(path, "wb") as fh:
        fh.write(data)                                           # a view into the encoder's pinned buffer
    return path


def evaluate(opt, splits_dir="splits", pl_name=None, pl_max_high=1.0, png_encoder="pil"):
    """See the module docstring."""
    from . import image_codecs
    image_codecs.check_png_encoder(png_encoder, "export_detection: --png_encoder")
    on_device = png_encoder == "device"
    ED._refuse_uncovered(opt)
    if not opt.det_name:
        raise ValueError("export_detection: --det_name is required (the folder the depth PNGs are written to)")
    if pl_name and (opt.no_eval or opt.eval_split == "benchmark"):
        raise ValueError("export_detection: --pl_name needs the scaled depth maps; it cannot be combined with --no_eval or "
                         "--eval_split benchmark")
    filenames = ED._read_lines(os.path.join(splits_dir, "detection", "test.txt"))
    dates = []
    if opt.ext_disp_to_eval is None:
        from .predict import Predictor
        if opt.load_weights_folder is None:
            raise ValueError("export_detection: --load_weights_folder is required")
        opt.load_weights_folder = folder = os.path.expanduser(opt.load_weights_folder)
        if not os.path.isdir(folder):
            raise FileNotFoundError("Cannot find a folder at {}".format(folder))
        print("-> Loading weights from {}".format(folder))
        enc = torch.load(os.path.join(folder, "encoder.pth"), map_location="cpu")
        height, width = int(enc.get("height", opt.height)), int(enc.get("width", opt.width))
        del enc
        if opt.eval_gdc:
            opt.eval_batch_size = 1
        predictor = Predictor(folder, num_layers=opt.num_layers, scales=tuple(opt.scales), cat_4beam_to_color=opt.cat_4beam_to_color,
                              cat2start=opt.cat2start, cat2end=opt.cat2end, refine_2d=opt.refine_2d, catxy=(opt.catxy == "true"),
                              refine2d_deep=(opt.refine2d_deep == "true"), refine_a0=(opt.refine_a0 == "true"),
                              refine_iter=opt.refine_iter, refine_offset=opt.refine_offset,
                              refine_depthnet_with_beam=(opt.refine_depthnet_with_beam == "true"), height=height, width=width,
                              min_depth=opt.min_depth, max_depth=opt.max_depth)
        loader = detection.KITTIDetecBatches(opt.data_path, filenames, height, width, [0], 4, is_train=False, img_ext=".png", opt=opt,
                                             batch_size=opt.eval_batch_size, drop_last=False)
        print("-> Computing predictions with size {}x{}".format(width, height))
        pred_disps = []
        for batch in loader:
            dates += batch["date"]
            pred_disps.append(ED.predict_disps(predictor, batch, opt))
        loader.close()
        pred_disps = np.concatenate(pred_disps)
    else:
        print("-> Loading predictions from {}".format(opt.ext_disp_to_eval))
        pred_disps = np.load(opt.ext_disp_to_eval)

    if opt.save_pred_disps:
        output_path = os.path.join(opt.load_weights_folder, "disps_{}_split.npy".format(opt.eval_split))
        print("-> Saving predicted disparities to ", output_path)
        np.save(output_path, pred_disps)
    if opt.no_eval:
        print("-> Evaluation disabled. Done.")
        return None
    if opt.eval_split == "benchmark":
        ED.save_benchmark_predictions(opt, pred_disps)
        return None

    gt_depths = list(np.load(os.path.join(splits_dir, "detection", "gt_depths.npz"), fix_imports=True, encoding="latin1",
                             allow_pickle=True)["data"])
    N = len(gt_depths)
    if len(pred_disps) != N or len(filenames) != N:
        raise ValueError("export_detection: %d predictions and %d split lines for %d ground-truth maps" % (len(pred_disps), len(filenames), N))
    print("-> Evaluating")
    if opt.eval_stereo:
        print("   Stereo evaluation - disabling median scaling, scaling by {}".format(ED.STEREO_SCALE_FACTOR))
        opt.disable_median_scaling = True
        opt.pred_depth_scale_factor = ED.STEREO_SCALE_FACTOR
    else:
        print("   Mono evaluation - using median scaling")

    paths = [png_path(opt.data_path, line, opt.det_name) for line in filenames]
    pl_paths, pl_calibs = [], []
    if pl_name:
        from . import kitti_utils
        pl_paths = [bin_path(opt.data_path, line, pl_name) for line in filenames]
        if not dates:                                            # the loader did not run (--ext_disp_to_eval)
            for line in filenames:
                folder, frame_index, _ = parse_line(line)
                image = os.path.join(opt.data_path, folder, "image_02/data/{:06d}.png".format(frame_index))
                dates.append(detection.detec_calib_date(*detection.image_size(image)))
        by_date = {d: (kitti_utils.Calibration(os.path.join(opt.data_path, d, "calib_cam_to_cam.txt")),)
                      + kitti_utils.rect_to_velo(os.path.join(opt.data_path, d)) for d in sorted(set(dates))}
        pl_calibs = [by_date[d] for d in dates]
    for d in sorted(set(os.path.dirname(p) for p in paths + pl_paths)):
        os.makedirs(d, exist_ok=True)
    writes = []
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, max(1, os.cpu_count() or 1))) as pool:
        if opt.eval_gdc:
            from . import kitti_utils
            if opt.random_sample == -1:
                beam_path = os.path.join(splits_dir, "detection", "4beam.npz")
            else:
                beam_path = os.path.join(splits_dir, "detection", "r{}.npz".format(opt.random_sample))
            beam_depths = np.load(beam_path, fix_imports=True, encoding="latin1", allow_pickle=True)["data"]
            calibs = [kitti_utils.Calibration(os.path.join(opt.data_path, d, "calib_cam_to_cam.txt")) for d in dates]

            def on_depth(i, depth):                              # after scaling and GDC, before the clamp (:388)
                if on_device:
                    (data,), _ = image_codecs.encode_png_batch([detection.quantize_u16(depth, want_device=True)], pool)
                    writes.append(pool.submit(_save_bytes, paths[i], data))
                else:
                    writes.append(pool.submit(_save_png, paths[i], detection.quantize_u16(depth)))
                if pl_name:                                      # the corrected map, rounded to float32 once (as --visualize does)
                    cloud, = detection.points_export([depth.detach().to(torch.float32)], [pl_calibs[i]], pl_max_high)
                    writes.append(pool.submit(_save_bin, pl_paths[i], cloud))

            mean_errors, ratios = ED.evaluate_predictions(pred_disps, gt_depths, opt.eval_split, opt.pred_depth_scale_factor,
                                                          opt.disable_median_scaling, True, beam_depths, calibs, opt.random_sample, opt.nbeams,
                                                          on_depth=on_depth)
            per_image = None
        else:
            per_image, ratios, _ = ED.eigen_scores(pred_disps, gt_depths, opt.eval_split, opt.pred_depth_scale_factor,
                                                   opt.disable_median_scaling)
            mean_errors = per_image.mean(0)
            sizes = [np.asarray(g).shape for g in gt_depths]
            for a in range(0, N, EXPORT_CHUNK):                  # the pool writes chunk k while the device runs chunk k + 1
                b = min(a + EXPORT_CHUNK, N)
                chunk_ratios = None if opt.disable_median_scaling else ratios[a:b]
                if not pl_name:
                    maps = detection.depth_export(pred_disps[a:b], sizes[a:b], chunk_ratios, opt.pred_depth_scale_factor, chunk=EXPORT_CHUNK,
                                                  want_device=on_device)
                else:                                            # the cloud from the float32 map the PNG is quantised from
                    maps, _, (pack,) = detection.depth_export(pred_disps[a:b], sizes[a:b], chunk_ratios, opt.pred_depth_scale_factor,
                                                              want_depth=True, chunk=EXPORT_CHUNK, want_packed=True,
                                                              want_device=on_device)
                    clouds = detection.points_export(None, pl_calibs[a:b], pl_max_high, packed=pack)
                    writes += [pool.submit(_save_bin, pl_paths[a + k], c) for k, c in enumerate(clouds)]
                if on_device:                                    # the payload never leaves the device unencoded
                    files, _ = image_codecs.encode_png_batch(maps, pool)
                    writes += [pool.submit(_save_bytes, paths[a + k], f) for k, f in enumerate(files)]
                else:
                    writes += [pool.submit(_save_png, paths[a + k], m) for k, m in enumerate(maps)]
        for w in writes:
            w.result()                                           # a failed write raises here
    print("-> Saved {} depth maps to <data_path>/<folder>/{}".format(N, opt.det_name))
    if pl_name:
        print("-> Saved {} pseudo-LiDAR clouds to <data_path>/<folder>/{}".format(N, pl_name))
    if not opt.disable_median_scaling:
        med = np.median(ratios)
        print(" Scaling ratios | med: {:0.3f} | std: {:0.3f}".format(med, np.std(ratios / med)))
    print("\n  " + ("{:>8} | " * 7).format(*ED.METRICS))
    print(("&{: 8.3f}  " * 7).format(*mean_errors.tolist()) + "\\\\")
    print("\n-> Done!")
    if pl_name:
        return mean_errors, ratios, per_image, paths, pl_paths
    return mean_errors, ratios, per_image, paths


# the flags of this script that are not among the reference's options (``evaluate_depth.split_off_flags``), with their defaults
SCRIPT_FLAGS = {"splits_dir": "splits", "pl_name": None, "pl_max_high": "1.0", "png_encoder": "pil"}


def main(argv=None):
    from .options import MonodepthOptions
    found, rest = ED.split_off_flags(sys.argv[1:] if argv is None else argv, SCRIPT_FLAGS)
    opt = MonodepthOptions().parse(rest)
    extra = {} if found["png_encoder"] == "pil" else {"png_encoder": found["png_encoder"]}
    if found["pl_name"] is None:                                 # the call of a command line without the new flags, as before
        return evaluate(opt, found["splits_dir"], **extra)
    return evaluate(opt, found["splits_dir"], pl_name=found["pl_name"], pl_max_high=float(found["pl_max_high"]), **extra)


if __name__ == "__main__":
    main()
