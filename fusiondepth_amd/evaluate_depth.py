"""The reference's ``evaluate_depth.py`` on the device: the Eigen-split metrics of a saved model.

  * ``compute_errors(gt, pred)``                      evaluate_depth.py:42-60   (fd_depth_errors)
  * ``batch_post_process_disparity(l_disp, r_disp)``  evaluate_depth.py:62-70   (fd_post_process_disparity, float64 like numpy)
  * ``evaluate_predictions(pred_disps, gt_depths, ...)``  the per-image loop of ``evaluate`` (evaluate_depth.py:344-478), one image
    at a time: resize the predicted disparity to the ground-truth size, invert, Eigen mask + Garg crop, ``pred_depth_scale_factor``,
    median scaling, optional GDC (--eval_gdc, gdc.py), clamp to [1e-3, 80], metrics, mean over images.  The path of ``--eval_gdc``,
    which needs the dense map between median scaling and scoring.
  * ``pack_gt_depths`` / ``eigen_scores(pred_disps, gt_depths, ...)``  the same loop without GDC as one library call per chunk of
    images (fd_eigen_scores, csrc/eigen_eval.hip): the resize is evaluated at the selected ground-truth pixels only, numpy's medians
    come from a radix select over the compacted pairs, float32 terms, float64 sums in a fixed order (bitwise reproducible).
  * ``pack_labels`` / ``eigen_class_scores(pred_disps, gt_depths, sem_masks, ...)`` / ``semantic_summary``: ``--per_semantic``
    (:330-334, :451-467, :491-496), the metrics of every image per semantic class - 34 boolean selections and ``compute_errors`` calls
    per image in the reference - from the same library call per chunk (fd_eigen_class_scores, csrc/eigen_class.hip): each selected
    pixel's label rides beside its (gt, pred) pair, one workgroup per (class, image) sums its class over the compact list.  With
    ``--eval_gdc`` the classes are scored per image from the dense map (``functional.class_errors``, fd_class_errors).
  * ``--visualize`` (:252-261, :407-449): the two pictures per test image - the disparity in magma colours, the error through a hue ramp
    at the evaluation mask - from one library call per chunk (``visualize.render``, fd_vis_render, csrc/visualize.hip), and the
    ``.npy`` dumps beside them, under ``--vis_dir``.
  * ``evaluate(opt, splits_dir, semantic_dir, semantic_out, vis_dir)`` / ``python -m fusiondepth_amd.evaluate_depth``: the script
    (:74-496), on ``Predictor`` (with ``--refine_2d``: the stage-2 refine decoder) and ``KITTIRAWBatches``.

Deviations from the reference, on purpose
  * disparities are scored as float32.  ``--post_process`` yields float64 (numpy's promotion in ``batch_post_process_disparity``), which
    the reference hands to ``cv2.resize`` as float64; here they are rounded to float32 once, as ``evaluate_predictions`` always did.
  * ``--post_process`` feeds the mirrored colour image next to the UNMIRRORED LiDAR maps (and a batch of B maps next to 2 B images,
    which fails for B > 1); here the second pass gets the mirrored ``2channel`` / ``4beam`` maps, as ``evaluate_completion`` does.
  * the splits folder is an argument (``--splits_dir``, taken off the command line before ``MonodepthOptions`` parses the rest; default
    ``splits``) instead of a folder beside the script; ``--eval_gdc`` reads the calibration under ``--data_path`` instead of ``kitti_data/``,
    and the beam file is read only then (the reference loads it always and uses it only with ``--eval_gdc``).
  * ``--per_semantic`` reads ``pred_mask{i}.png`` from ``--semantic_dir`` and writes ``<run_name>.npy`` and ``pixel_count.npy`` under
    ``--semantic_out`` (default ``.``), both taken off the command line like ``--splits_dir``, instead of
    ``../semantic-segmentation/kitti/results`` and the working directory; without ``--semantic_dir`` the flag is refused.  The
    arrays have one column per image of the split, not the reference's fixed 697; ``--run_name`` unset names the file ``per_semantic.npy``.
  * ``--no_eval`` and ``--eval_split benchmark`` return ``None`` instead of ending the interpreter; the benchmark PNGs are written with
    PIL; no wandb run, no ``visualization/dates.npy``, no input statistics printout.
  * ``--visualize`` writes under ``--vis_dir`` (taken off the command line like ``--splits_dir``; ``prediction/`` and ``npy/`` are
    created there) instead of ``visualization/`` in the working directory; without ``--vis_dir`` the flag is refused.  The PNGs are
    written with PIL, not OpenCV.  ``{idx}rgb.png`` is written for EVERY item of a batch (the reference writes item 0 of each batch
    under the batch's index), resized with ``FD.resize_linear_cv`` and rounded half to even.  The error picture's default colours
    are an analytic hue ramp (``visualize.hue_lut``), NOT OpenCV's ``COLORMAP_HSV`` bit for bit: cv2 is not available to pin it.
    After ``--eval_gdc`` the map is rounded to float32 once before it is drawn and dumped (the reference keeps GDC's float64);
    ``beam_depth.npy`` is written only then, and holds the beam map as loaded.  No ``dates.npy``.
  * not covered, refused with the reason: ``--visualize`` without ``--vis_dir``, ``--per_semantic`` without ``--semantic_dir``, ``--save_sample``, ``--demo``, the odometry splits, a model
    without the beam encoder, ``--cat2end`` with ``--refine_2d`` (the reference's refine branch reads ``beam_features``, which ``--cat2end``
    never computes), ``--eval_gdc`` with ``--ext_disp_to_eval`` (the reference's ``dates`` are undefined there).
No CPU fallback: tensors must live on the GPU.
"""
import os
import sys

import numpy as np
import torch

from . import functional as FD
from ._lib import _need_cuda, call, query, stream

MIN_DEPTH = 1e-3          # evaluate_depth.py:28-29
MAX_DEPTH = 80
STEREO_SCALE_FACTOR = 5.4 # :32
METRICS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
NUM_CLASSES = 34          # :331, :455 - the label ids of the segmentation masks
# numpy mirror of ``fd_eigen_desc`` (40 bytes, as ``_lib.EigenDesc``)
EIGEN_DESC = np.dtype([("offset", np.int64), ("H", np.int32), ("W", np.int32), ("pred", np.int32), ("y0", np.int32), ("y1", np.int32),
                       ("x0", np.int32), ("x1", np.int32), ("reserved", np.int32)])


def compute_errors(gt, pred):
    """evaluate_depth.py:42-60 on matched device tensors -> (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3) as floats."""
    return tuple(float(v) for v in FD.depth_errors(gt, pred))


def batch_post_process_disparity(l_disp, r_disp):
    """evaluate_depth.py:62-70: [B,H,W] float32 device tensors -> [B,H,W] float64 device tensor."""
    l_disp, r_disp = FD.f32(l_disp), FD.f32(r_disp)
    _need_cuda(l_disp, r_disp)
    assert l_disp.shape == r_disp.shape and l_disp.dim() == 3
    out = torch.empty(l_disp.shape, device=l_disp.device, dtype=torch.float64)
    call("fd_post_process_disparity", l_disp.data_ptr(), r_disp.data_ptr(), out.data_ptr(), l_disp.shape[0], l_disp.shape[1],
         l_disp.shape[2], stream())
    return out


def _median(v):
    """np.median (mean of the two middle values for an even count; torch.median would take the lower one)."""
    s, _ = torch.sort(v.reshape(-1))
    n = s.numel()
    return s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])


def garg_crop(gt_height, gt_width):
    """evaluate_depth.py:361-363."""
    return np.array([0.40810811 * gt_height, 0.99189189 * gt_height, 0.03594771 * gt_width, 0.96405229 * gt_width]).astype(np.int32)


def gdc_range(random_sample=-1, nbeams=4):
    """evaluate_depth.py:391-396: the pitch range (degrees) GDC considers for the sparse input."""
    if random_sample == -1:
        return (-0.1, 4.0)
    if nbeams > 4:
        return (-10, 10)
    return (-1.5, 9)


def evaluate_predictions(pred_disps, gt_depths, eval_split="eigen", pred_depth_scale_factor=1.0, disable_median_scaling=False,
                         eval_gdc=False, beam_depths=None, calibs=None, random_sample=-1, nbeams=4, on_depth=None, sem_masks=None,
                         num_classes=NUM_CLASSES):
    """evaluate_depth.py:344-478.  ``pred_disps``: [N,h,w] device tensor (or list); ``gt_depths``: list of [H_i,W_i] arrays /
    tensors (KITTI ground truth has per-drive sizes).  Returns (mean of the 7 metrics over the images, per-image scaling ratios).
    ``eval_gdc`` (--eval_gdc, evaluate_depth.py:387-405): after median scaling, correct each prediction with GDC against
    ``beam_depths[i]`` (the sparse LiDAR map at ground-truth size, 0 = no point) and ``calibs[i]`` (``kitti_utils.Calibration``),
    with the reference's settings and pitch range (``gdc_range(random_sample, nbeams)``).  ``on_depth``: an optional callback
    ``(i, depth)`` that sees image i's dense [H_i,W_i] device map after scaling and GDC, before the clamp (export_detection.py:388
    saves it there); the default changes nothing.  ``sem_masks`` (--per_semantic, :451-467): N [H_i,W_i] uint8 label maps; the
    classes of every image are then scored on ``gt[mask]``, the clamped ``pred[mask]`` and ``sem[mask]`` (``FD.class_errors``) and
    the result is ``(mean, ratios, class_metrics[N,K,7] float64, class_counts[N,K] int64)``."""
    if sem_masks is not None and len(sem_masks) != len(gt_depths):
        raise ValueError("evaluate_predictions: %d label masks for %d ground-truth maps" % (len(sem_masks), len(gt_depths)))
    classes = []
    if eval_gdc:
        from .gdc import GDC
        if beam_depths is None or calibs is None:
            raise ValueError("evaluate_predictions: eval_gdc needs beam_depths and calibs")
    errors, ratios = [], []
    for i in range(len(gt_depths)):
        gt = torch.as_tensor(gt_depths[i], dtype=torch.float32).cuda()
        gh, gw = gt.shape
        disp = FD.f32(torch.as_tensor(pred_disps[i])).cuda()[None, None]
        # cv2.resize(pred_disp, (gt_width, gt_height)): OpenCV's float32 INTER_LINEAR rule on the device (fd_resize_linear_cv; parity
        # unpinned - no OpenCV in the build image - and restated from its source, like oracle/evaluate.py::resize_bilinear)
        disp = FD.resize_linear_cv(disp, (gh, gw))
        pred_depth = 1.0 / disp[0, 0]
        if eval_split in ("eigen", "demo"):
            mask = (gt > MIN_DEPTH) & (gt < MAX_DEPTH)
            c = garg_crop(gh, gw)
            crop = torch.zeros_like(mask)
            crop[c[0]:c[1], c[2]:c[3]] = True
            mask = mask & crop
        else:
            mask = gt > 0
        pred_depth = pred_depth * pred_depth_scale_factor
        if not disable_median_scaling:
            ratio = _median(gt[mask]) / _median(pred_depth[mask])
            ratios.append(float(ratio))
            pred_depth = pred_depth * ratio
        if eval_gdc:
            gtd = torch.as_tensor(beam_depths[i], dtype=torch.float64).cuda().clone()
            gtd[gtd == 0] = -1
            pred_depth = GDC(pred_depth, gtd, calibs[i], W_tol=3e-5, recon_tol=5e-4, k=10, method="cg",
                             consider_range=gdc_range(random_sample, nbeams), idx=i)
        if on_depth is not None:
            on_depth(i, pred_depth)
        pred, g = torch.clamp(pred_depth[mask], MIN_DEPTH, MAX_DEPTH), gt[mask]
        errors.append(compute_errors(g, pred))
        if sem_masks is not None:
            sem = torch.from_numpy(_label_plane(sem_masks[i], i, gh, gw, "evaluate_predictions")).cuda()
            classes.append(FD.class_errors(g, pred, sem[mask], num_classes))
    if sem_masks is not None:
        rows = torch.stack(classes).cpu().numpy() if classes else np.zeros((0, num_classes, 8))
        return np.array(errors).mean(0), np.array(ratios), rows[:, :, :7].copy(), rows[:, :, 7].astype(np.int64)
    return np.array(errors).mean(0), np.array(ratios)


# ---------------------------------------------------------------------------------------------------------------- the batched scorer
def split_window(eval_split, gt_height, gt_width):
    """The mask window (y0, y1, x0, x1) of one ground-truth map: the Garg crop for ``eigen`` / ``demo`` (evaluate_depth.py:358-365),
    the whole map for every other split (:367-368)."""
    if eval_split in ("eigen", "demo"):
        return tuple(int(v) for v in garg_crop(gt_height, gt_width))
    return 0, int(gt_height), 0, int(gt_width)


def split_bounds(eval_split):
    """(gt_lo, gt_hi) of the strict comparisons that select ground truth: (1e-3, 80) for ``eigen`` / ``demo``, (0, inf) otherwise."""
    return (MIN_DEPTH, float(MAX_DEPTH)) if eval_split in ("eigen", "demo") else (0.0, float("inf"))


def pack_gt_depths(gt_depths, eval_split):
    """Ground-truth maps of different sizes -> (flat float32 tensor holding them back to back, ``EIGEN_DESC`` array with one
    descriptor per map: plane offset, size, the index of its prediction (its position in ``gt_depths``) and the split's mask window,
    computed as the reference does: float64 products, ``astype(np.int32)``, clamped to the map like the slice they feed).  Pure host
    code; the tensor is pinned where a GPU is present, so that its upload can overlap."""
    maps = [np.ascontiguousarray(np.asarray(g), dtype=np.float32) for g in gt_depths]
    desc = np.zeros(len(maps), dtype=EIGEN_DESC)
    at = 0
    for i, g in enumerate(maps):
        if g.ndim != 2 or not g.size:
            raise ValueError("pack_gt_depths: ground truth %d has shape %s, expected a non-empty [H,W] map" % (i, g.shape))
        H, W = g.shape
        y0, y1, x0, x1 = split_window(eval_split, H, W)
        y1, x1 = min(max(y1, 0), H), min(max(x1, 0), W)
        y0, x0 = min(max(y0, 0), y1), min(max(x0, 0), x1)
        desc[i] = (at, H, W, i, y0, y1, x0, x1, 0)
        at += H * W
    packed = torch.empty((max(at, 1),), dtype=torch.float32, pin_memory=torch.cuda.is_available())
    flat = packed.numpy()
    for d, g in zip(desc, maps):
        flat[d["offset"]:d["offset"] + g.size] = g.reshape(-1)
    return packed[:at] if at else packed[:0], desc


def _upload_chunk(who, disp, gt_depths, eval_split):
    """One chunk of ``eigen_scores`` / ``eigen_class_scores`` on its way to the device -> (disparities [n,h,w] on the device, the pinned
    packed ground truth, its descriptors, both on the device, the tallest window, the sum of the window areas)."""
    disp = disp if torch.is_tensor(disp) else torch.as_tensor(np.asarray(disp))
    disp = FD.f32(disp).cuda()
    if disp.dim() != 3:
        raise ValueError("%s: pred_disps must be [N,h,w], got %s" % (who, tuple(disp.shape)))
    packed, desc = pack_gt_depths(gt_depths, eval_split)
    packed_d = packed.to(disp.device, non_blocking=True)
    desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to(disp.device)
    max_rows = int((desc["y1"] - desc["y0"]).max())
    cap = int(((desc["y1"] - desc["y0"]).astype(np.int64) * (desc["x1"] - desc["x0"])).sum())
    return disp, packed, desc, packed_d, desc_d, max_rows, cap


def eigen_scores(pred_disps, gt_depths, eval_split="eigen", pred_depth_scale_factor=1.0, disable_median_scaling=False, chunk=64):
    """evaluate_depth.py:344-478 without GDC, ``chunk`` images per ``fd_eigen_scores`` call (so that pinned and device memory stay
    bounded).  ``pred_disps``: [N,h,w] device tensor or host array (float64 is rounded to float32 once); ``gt_depths``: N [H_i,W_i]
    maps.  Returns ``(per_image[N,7] float64, ratios[N] float32 - empty without median scaling -, counts[N] int64)``."""
    if not torch.cuda.is_available():
        raise RuntimeError("fusiondepth_amd.evaluate_depth.eigen_scores needs an MI355X: there is no CPU path (use oracle/ for CPU checks)")
    N = len(gt_depths)
    if len(pred_disps) != N:
        raise ValueError("eigen_scores: %d predictions for %d ground-truth maps" % (len(pred_disps), N))
    if chunk < 1 or chunk > 4096:
        raise ValueError("eigen_scores: chunk must be 1 .. 4096")
    gt_lo, gt_hi = split_bounds(eval_split)
    rows = []
    for a in range(0, N, chunk):
        b = min(a + chunk, N)
        disp, _, desc, packed_d, desc_d, max_rows, cap = _upload_chunk("eigen_scores", pred_disps[a:b], gt_depths[a:b], eval_split)
        dev = disp.device
        ws = torch.empty((max(query("fd_eigen_scores_ws_bytes", b - a, max_rows, cap), 8),), device=dev, dtype=torch.uint8)
        out = torch.empty((b - a, 9), device=dev, dtype=torch.float64)
        call("fd_eigen_scores", disp.data_ptr(), disp.shape[0], disp.shape[1], disp.shape[2], packed_d.data_ptr(), packed_d.numel(),
             desc_d.data_ptr(), b - a, max_rows, cap, float(gt_lo), float(gt_hi), float(pred_depth_scale_factor),
             0 if disable_median_scaling else 1, MIN_DEPTH, float(MAX_DEPTH), out.data_ptr(), ws.data_ptr(), stream())
        rows.append(out.cpu().numpy())                           # synchronises: the pinned buffer is free to go afterwards
    out = np.concatenate(rows) if rows else np.zeros((0, 9))
    ratios = np.zeros((0,), np.float32) if disable_median_scaling else out[:, 7].astype(np.float32)
    return out[:, :7].copy(), ratios, out[:, 8].astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- per semantic class
def _label_plane(mask, i, H, W, who):
    """Label mask ``i`` as a contiguous [H,W] uint8 array; ValueError when it is not of its ground truth's size or holds a value that
    uint8 cannot hold without change."""
    m = np.asarray(mask)
    if m.shape != (H, W):
        raise ValueError("%s: label mask %d has shape %s, its ground truth is %s" % (who, i, m.shape, (H, W)))
    with np.errstate(invalid="ignore"):
        u = m.astype(np.uint8)
    if not np.array_equal(u, m):
        raise ValueError("%s: label mask %d holds values that are not integers in 0 .. 255" % (who, i))
    return np.ascontiguousarray(u)


def pack_labels(sem_masks, desc):
    """Label masks beside ``pack_gt_depths``' planes: a uint8 tensor of as many BYTES as the packed ground truth has floats, mask n at
    byte ``desc[n]["offset"]`` (so a plane starts at any address: a 17x90 one is followed by one at an odd byte).  Pure host code;
    pinned where a GPU is present.  ValueError, naming the image, when a mask is not [H,W] of its ground truth or cannot be held
    as uint8 without change."""
    if len(sem_masks) != len(desc):
        raise ValueError("pack_labels: %d label masks for %d ground-truth maps" % (len(sem_masks), len(desc)))
    total = int(sum(int(d["H"]) * int(d["W"]) for d in desc))
    packed = torch.empty((max(total, 1),), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    flat = packed.numpy()
    for i, (d, m) in enumerate(zip(desc, sem_masks)):
        u = _label_plane(m, i, int(d["H"]), int(d["W"]), "pack_labels")
        flat[d["offset"]:d["offset"] + u.size] = u.reshape(-1)
    return packed[:total]


def eigen_class_scores(pred_disps, gt_depths, sem_masks, num_classes=NUM_CLASSES, eval_split="eigen", pred_depth_scale_factor=1.0,
                       disable_median_scaling=False, chunk=64):
    """``eigen_scores`` and, from the same call (fd_eigen_class_scores), evaluate_depth.py:451-467: the metrics of every image per
    label of ``sem_masks`` (N [H_i,W_i] uint8 maps; a label >= ``num_classes`` belongs to no class).  One upload of the labels and one
    download per chunk.  Returns ``(per_image[N,7], ratios, counts`` - ``eigen_scores``' own, bit for bit - ``, class_metrics[N,K,7]
    float64 (zeros where a class has no pixel), class_counts[N,K] int64)``."""
    if not torch.cuda.is_available():
        raise RuntimeError("fusiondepth_amd.evaluate_depth.eigen_class_scores needs an MI355X: there is no CPU path (use oracle/ for CPU checks)")
    N, K = len(gt_depths), int(num_classes)
    if len(pred_disps) != N or len(sem_masks) != N:
        raise ValueError("eigen_class_scores: %d predictions and %d label masks for %d ground-truth maps" % (len(pred_disps), len(sem_masks), N))
    if chunk < 1 or chunk > 4096:
        raise ValueError("eigen_class_scores: chunk must be 1 .. 4096")
    gt_lo, gt_hi = split_bounds(eval_split)
    rows, class_rows = [], []
    for a in range(0, N, chunk):
        b = min(a + chunk, N)
        n = b - a
        disp, _, desc, packed_d, desc_d, max_rows, cap = _upload_chunk("eigen_class_scores", pred_disps[a:b], gt_depths[a:b], eval_split)
        dev = disp.device
        labels = pack_labels(sem_masks[a:b], desc)
        labels_d = labels.to(dev, non_blocking=True)
        ws = torch.empty((max(query("fd_eigen_class_scores_ws_bytes", n, max_rows, cap, K), 8),), device=dev, dtype=torch.uint8)
        both = torch.empty((n * 9 + n * max(K, 0) * 8,), device=dev, dtype=torch.float64)       # out, then class_out: one download
        call("fd_eigen_class_scores", disp.data_ptr(), disp.shape[0], disp.shape[1], disp.shape[2], packed_d.data_ptr(), packed_d.numel(),
             desc_d.data_ptr(), n, max_rows, cap, float(gt_lo), float(gt_hi), float(pred_depth_scale_factor),
             0 if disable_median_scaling else 1, MIN_DEPTH, float(MAX_DEPTH), labels_d.data_ptr(), K, both.data_ptr(),
             both.data_ptr() + n * 9 * 8, ws.data_ptr(), stream())
        host = both.cpu().numpy()                                # synchronises: the pinned buffers are free to go afterwards
        rows.append(host[:n * 9].reshape(n, 9))
        class_rows.append(host[n * 9:].reshape(n, K, 8))
    out = np.concatenate(rows) if rows else np.zeros((0, 9))
    cls = np.concatenate(class_rows) if class_rows else np.zeros((0, max(K, 0), 8))
    ratios = np.zeros((0,), np.float32) if disable_median_scaling else out[:, 7].astype(np.float32)
    return out[:, :7].copy(), ratios, out[:, 8].astype(np.int64), cls[:, :, :7].copy(), cls[:, :, 7].astype(np.int64)


def semantic_summary(class_metrics, class_counts):
    """evaluate_depth.py:492-494 on the host: abs_rel of class c over the split, every image weighted by its pixels of the class,
    ``sum_i(abs_rel[i, c] * count[i, c]) / (sum_i count[i, c] + 1e-16)`` -> [K] float64 (0 for a class without pixels anywhere)."""
    abs_rel = np.asarray(class_metrics, np.float64)[:, :, 0].T            # [K, N], the reference's sem_errors[:, :, 0]
    counts = np.asarray(class_counts, np.float64).T
    return (abs_rel * counts).sum(1) / (counts.sum(1) + 0.0000000000000001)


def semantic_mask_paths(semantic_dir, n):
    """``<semantic_dir>/pred_mask{i}.png`` for the n images of the split, in scoring order (:452)."""
    return [os.path.join(semantic_dir, "pred_mask{}.png".format(i)) for i in range(n)]


def _require_masks(semantic_dir, n):
    for path in semantic_mask_paths(semantic_dir, n):
        if not os.path.isfile(path):
            raise FileNotFoundError("evaluate_depth: --per_semantic needs the label mask {}".format(path))


# ---------------------------------------------------------------------------------------------------------------- the script
def benchmark_depth_png(disp_resized):
    """evaluate_depth.py:299-301 on disparities already resized to 352x1216: ``5.4 / disp``, clip to 0 .. 80, ``uint16(depth * 256)``."""
    depth = STEREO_SCALE_FACTOR / np.asarray(disp_resized, dtype=np.float32)
    depth = np.clip(depth, 0, 80)
    return np.uint16(depth * 256)


def split_off_flags(argv, valued, switches=()):
    """Flags that are not among the reference's options (tests/golden/options_surface.json pins that surface) are taken off the
    command line before ``MonodepthOptions`` parses the rest.  ``valued``: {name: default} of the flags ``--name X`` / ``--name=X``;
    ``switches``: names of flags without a value.  Returns ({name: value - a string as typed, or the default -, switch: bool}, the
    remaining arguments); a flag that is in neither list stays in the rest and fails in argparse as before."""
    found = dict(valued)
    found.update({name: False for name in switches})
    rest, i, argv = [], 0, list(argv)
    while i < len(argv):
        arg = argv[i]
        name = arg[2:].split("=", 1)[0] if arg.startswith("--") else None
        if name in valued and "=" in arg:
            found[name] = arg.split("=", 1)[1]
        elif name in valued:
            if i + 1 >= len(argv):
                raise ValueError("--%s needs a value" % name)
            found[name] = argv[i + 1]
            i += 1
        elif name in switches and "=" not in arg:
            found[name] = True
        else:
            rest.append(arg)
        i += 1
    return found, rest


def split_off_splits_dir(argv, default="splits"):
    """``--splits_dir X`` / ``--splits_dir=X`` taken off the command line (``split_off_flags``) -> (splits_dir, the remaining
    arguments)."""
    found, rest = split_off_flags(argv, {"splits_dir": default})
    return found["splits_dir"], rest


# the flags of this script that are not among the reference's options (``split_off_flags``), with their defaults
SCRIPT_FLAGS = {"splits_dir": "splits", "semantic_dir": None, "semantic_out": ".", "vis_dir": None}


def _refuse_uncovered(opt, semantic_dir=None, vis_dir=None):
    """Everything ``evaluate`` does not cover, before anything touches the GPU.  ``--per_semantic`` is covered where the caller names
    the folder of the masks, ``--visualize`` where the caller names the folder the pictures go to."""
    if sum((bool(opt.eval_mono), bool(opt.eval_stereo))) != 1:
        raise ValueError("Please choose mono or stereo evaluation by setting either --eval_mono or --eval_stereo")
    named = {"per_semantic": semantic_dir, "visualize": vis_dir}  # covered where the caller names the folder
    for flag, why in (("visualize", "it writes OpenCV colour maps and .npy dumps to fixed relative folders; name yours with --vis_dir"),
                      ("per_semantic", "it reads masks of an external segmentation run from a fixed relative folder; name theirs with --semantic_dir"),
                      ("demo", "the demo split and its visualisation folders are not part of this package")):
        if getattr(opt, flag) and named.get(flag) is None:
            raise NotImplementedError("evaluate_depth: --%s is not covered (%s)" % (flag, why))
    if opt.save_sample != -1:
        raise NotImplementedError("evaluate_depth: --save_sample is not covered (a matplotlib plot saved to a path on the author's machine)")
    if opt.eval_split in ("odom_9", "odom_10"):
        raise NotImplementedError("evaluate_depth: the odometry splits are not covered (the reference's script has no ground truth for them)")
    if opt.ext_disp_to_eval is None:
        if not opt.beam_encoder:
            raise NotImplementedError("evaluate_depth: a model without the beam encoder is not covered (Predictor always runs it)")
        if opt.cat2end and opt.refine_2d:
            raise NotImplementedError("evaluate_depth: --cat2end with --refine_2d is not covered (the reference's refine branch reads "
                                      "beam_features, which its --cat2end branch never computes)")
    elif opt.eval_gdc:
        raise NotImplementedError("evaluate_depth: --eval_gdc with --ext_disp_to_eval is not covered (the reference's dates are undefined there)")


def _read_lines(path):
    with open(path) as fh:
        return [ln for ln in fh.read().splitlines() if ln.strip()]


def predict_disps(predictor, batch, opt):
    """evaluate_depth.py:166-242 for one batch -> [B,192,640] host array of scaled disparities (float32; float64 with --post_process)."""
    keys = ["2channel", "4beam"] + [("inv_K", s) for s in opt.scales]
    color = batch["color", 0, 0]
    B = color.shape[0]
    if opt.post_process:                                         # two passes per image, the second mirrored (LiDAR maps included)
        inputs = {("color_aug", 0, 0): torch.cat((color, torch.flip(color, [3])), 0)}
        for k in keys:
            if k in batch:
                second = torch.flip(batch[k], [3]) if isinstance(k, str) else batch[k]
                inputs[k] = torch.cat((batch[k], second), 0)
    else:
        inputs = {("color_aug", 0, 0): color}
        inputs.update({k: batch[k] for k in keys if k in batch})
    disp = predictor.predict(inputs)[("disp", 0)]
    if tuple(disp.shape[2:]) != (192, 640):                      # :235-236, the reference's fixed size
        disp = FD.bilinear_upsample(disp, (192, 640)) if disp.shape[2] <= 192 and disp.shape[3] <= 640 else \
            torch.nn.functional.interpolate(disp, [192, 640], mode="bilinear", align_corners=False)
    pred_disp = FD.disp_to_depth(disp, opt.min_depth, opt.max_depth)[0][:, 0]
    if opt.post_process:
        pred_disp = batch_post_process_disparity(pred_disp[:B].contiguous(), torch.flip(pred_disp[B:], [2]).contiguous())
    return pred_disp.cpu().numpy()


def selection_mask(gt, eval_split):
    """evaluate_depth.py:358-368 on the host: the boolean [H,W] mask of the pixels ``eval_split`` scores (``mask.npy`` of --visualize)."""
    gt = np.asarray(gt, dtype=np.float32)
    y0, y1, x0, x1 = split_window(eval_split, *gt.shape)
    lo, hi = split_bounds(eval_split)
    mask = gt > np.float32(lo)
    if np.isfinite(hi):
        mask &= gt < np.float32(hi)
    crop = np.zeros(gt.shape, dtype=bool)
    crop[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = True
    return mask & crop


def save_rgb_pngs(vis_dir, first, color):
    """evaluate_depth.py:252-261 for every item of a batch: ``color`` [B,3,h,w] in 0 .. 1 on the device, resized to 375x1242 by
    OpenCV's INTER_LINEAR rule, ``* 255``, rounded half to even -> ``<vis_dir>/prediction/{first + k}rgb.png``."""
    from PIL import Image
    os.makedirs(os.path.join(vis_dir, "prediction"), exist_ok=True)
    rgb = torch.round(FD.resize_linear_cv(color, (375, 1242)) * 255.0).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    for k, img in enumerate(rgb):
        Image.fromarray(np.ascontiguousarray(img)).save(os.path.join(vis_dir, "prediction", "{}rgb.png".format(first + k)))


def save_visuals(vis_dir, vis_name, first, gt_depths, eval_split, pred_disps=None, ratios=None, pred_depth_scale_factor=1.0, depths=None,
                 beam_depths=None):
    """evaluate_depth.py:407-449 for images ``first`` .. of the scored list, one ``visualize.render`` call: the error picture
    ``prediction/{i}{vis_name}.png``, the colour picture ``prediction/{i}{vis_name}depth.png`` and ``npy/{i}{vis_name}pred_depth.npy``,
    ``..diff.npy``, ``..mask.npy`` (``..beam_depth.npy`` where ``beam_depths`` are given) under ``vis_dir``.  The map comes from
    ``pred_disps`` with the scorer's ``ratios``, or from ``depths`` (dense device maps, after GDC)."""
    from PIL import Image
    from .visualize import render
    pics, dumps = os.path.join(vis_dir, "prediction"), os.path.join(vis_dir, "npy")
    os.makedirs(pics, exist_ok=True)
    os.makedirs(dumps, exist_ok=True)
    gt_depths = list(gt_depths)
    colors, errors, maps = render(pred_disps, gt_depths, ratios, eval_split, pred_depth_scale_factor, depths=depths, want_depth=True,
                                  chunk=max(1, min(len(gt_depths), 64)))
    for k, gt in enumerate(gt_depths):
        stem = "{}{}".format(first + k, vis_name)
        pred = maps[k].cpu().numpy()
        Image.fromarray(errors[k]).save(os.path.join(pics, stem + ".png"))
        Image.fromarray(colors[k]).save(os.path.join(pics, stem + "depth.png"))
        np.save(os.path.join(dumps, stem + "pred_depth.npy"), pred)
        np.save(os.path.join(dumps, stem + "diff.npy"), np.abs(pred - np.asarray(gt, dtype=np.float32)))
        np.save(os.path.join(dumps, stem + "mask.npy"), selection_mask(gt, eval_split))
        if beam_depths is not None:
            np.save(os.path.join(dumps, stem + "beam_depth.npy"), np.asarray(beam_depths[k]))


def save_benchmark_predictions(opt, pred_disps):
    """evaluate_depth.py:291-311: the ``benchmark`` split has no ground truth; its predictions go to 352x1216 16-bit PNGs under
    ``<load_weights_folder>/benchmark_predictions``."""
    from PIL import Image
    save_dir = os.path.join(opt.load_weights_folder, "benchmark_predictions")
    print("-> Saving out benchmark predictions to {}".format(save_dir))
    os.makedirs(save_dir, exist_ok=True)
    for a in range(0, len(pred_disps), 64):
        resized = FD.resize_linear_cv(FD.f32(torch.as_tensor(pred_disps[a:a + 64])).cuda(), (352, 1216)).cpu().numpy()
        for k, depth in enumerate(benchmark_depth_png(resized)):
            Image.fromarray(depth).save(os.path.join(save_dir, "{:010d}.png".format(a + k)))
    print("-> No ground truth is available for the KITTI benchmark, so not evaluating. Done.")


def evaluate(opt, splits_dir="splits", semantic_dir=None, semantic_out=".", vis_dir=None):
    """evaluate_depth.py:74-496: the disparities of a saved model over ``<splits_dir>/<eval_split>/test_files.txt`` (or those of
    ``--ext_disp_to_eval``), scored against ``gt_depths.npz`` of the split.  Returns ``(mean[7], ratios, per_image[N,7])``
    (``per_image`` is None with ``--eval_gdc``, which scores through ``evaluate_predictions``); None after ``--no_eval`` and for the
    ``benchmark`` split, which has no ground truth.  With ``--per_semantic`` and a ``semantic_dir`` holding ``pred_mask{i}.png`` for
    image i of the scored list: one line per class that has pixels, ``<semantic_out>/<run_name>.npy`` ([34] abs_rel per class) and
    ``<semantic_out>/pixel_count.npy`` ([34, N]) as the reference writes them, and a fourth element
    ``{"abs_rel": [34], "pixel_count": [34, N], "metrics": [N, 34, 7]}``.  With ``--visualize`` and a ``vis_dir``: the pictures and
    dumps of ``save_visuals`` for every scored image (with the scorer's own ratios; the scores are what they are without the flag)
    and, when the predictions are computed here, ``save_rgb_pngs`` for every item; the returned tuple keeps its length."""
    _refuse_uncovered(opt, semantic_dir, vis_dir)
    per_semantic = bool(opt.per_semantic) and not opt.no_eval and opt.eval_split != "benchmark"
    if per_semantic:
        _require_masks(semantic_dir, 1)                          # a missing folder fails here, before anything is loaded
    dates = []
    if opt.ext_disp_to_eval is None:
        from .datasets import KITTIRAWBatches
        from .predict import Predictor
        if opt.load_weights_folder is None:
            raise ValueError("evaluate_depth: --load_weights_folder is required")
        opt.load_weights_folder = folder = os.path.expanduser(opt.load_weights_folder)
        if not os.path.isdir(folder):
            raise FileNotFoundError("Cannot find a folder at {}".format(folder))
        print("-> Loading weights from {}".format(folder))
        filenames = _read_lines(os.path.join(splits_dir, opt.eval_split, "test_files.txt"))
        if per_semantic:
            _require_masks(semantic_dir, len(filenames))
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
        loader = KITTIRAWBatches(opt.data_path, filenames, height, width, [0], 4, is_train=False, img_ext=".png" if opt.png else ".jpg",
                                 opt=opt, batch_size=opt.eval_batch_size, drop_last=False)
        print("-> Computing predictions with size {}x{}".format(width, height))
        pred_disps, idx = [], 0
        for batch in loader:
            dates += batch["date"]
            pred_disps.append(predict_disps(predictor, batch, opt))
            if opt.visualize:
                save_rgb_pngs(vis_dir, idx, batch["color", 0, 0])
            idx += len(pred_disps[-1])
        loader.close()
        pred_disps = np.concatenate(pred_disps)
    else:
        print("-> Loading predictions from {}".format(opt.ext_disp_to_eval))
        pred_disps = np.load(opt.ext_disp_to_eval)
        if opt.eval_eigen_to_benchmark:
            pred_disps = pred_disps[np.load(os.path.join(splits_dir, "benchmark", "eigen_to_benchmark_ids.npy"))]
        if per_semantic:
            _require_masks(semantic_dir, len(pred_disps))

    if opt.save_pred_disps:
        output_path = os.path.join(opt.load_weights_folder, "disps_{}_split.npy".format(opt.eval_split))
        print("-> Saving predicted disparities to ", output_path)
        np.save(output_path, pred_disps)

    if opt.no_eval:
        print("-> Evaluation disabled. Done.")
        return None
    if opt.eval_split == "benchmark":
        save_benchmark_predictions(opt, pred_disps)
        return None

    gt_depths = np.load(os.path.join(splits_dir, opt.eval_split, "gt_depths.npz"), fix_imports=True, encoding="latin1", allow_pickle=True)["data"]
    print("-> Evaluating")
    if opt.eval_stereo:
        print("   Stereo evaluation - disabling median scaling, scaling by {}".format(STEREO_SCALE_FACTOR))
        opt.disable_median_scaling = True
        opt.pred_depth_scale_factor = STEREO_SCALE_FACTOR
    else:
        print("   Mono evaluation - using median scaling")
    sem_masks, classes = None, None
    if per_semantic:
        from PIL import Image
        sem_masks = [np.asarray(Image.open(path)) for path in semantic_mask_paths(semantic_dir, len(gt_depths))]
    if opt.eval_gdc:
        from . import kitti_utils
        if opt.random_sample == -1:
            print("using {} beams LiDAR".format(opt.nbeams))
            beam_path = os.path.join(splits_dir, opt.eval_split, "{}beam.npz".format(opt.nbeams))
        else:
            beam_path = os.path.join(splits_dir, opt.eval_split, "r{}.npz".format(opt.random_sample))
        beam_depths = np.load(beam_path, fix_imports=True, encoding="latin1", allow_pickle=True)["data"]
        calibs = [kitti_utils.Calibration(os.path.join(opt.data_path, d, "calib_cam_to_cam.txt")) for d in dates]
        held = []                                                # dense maps after GDC, rounded to float32 once, 64 per render call

        def flush(upto):
            if held:
                first = upto - len(held)
                save_visuals(vis_dir, opt.vis_name, first, gt_depths[first:upto], opt.eval_split, depths=held, beam_depths=beam_depths[first:upto])
                del held[:]

        def on_depth(i, depth):
            held.append(depth.detach().to(torch.float32))
            if len(held) == 64:
                flush(i + 1)

        scored = evaluate_predictions(pred_disps, gt_depths, opt.eval_split, opt.pred_depth_scale_factor, opt.disable_median_scaling,
                                      True, beam_depths, calibs, opt.random_sample, opt.nbeams, sem_masks=sem_masks,
                                      on_depth=on_depth if opt.visualize else None)
        flush(len(gt_depths))
        mean_errors, ratios, classes = scored[0], scored[1], scored[2:]
        per_image = None
    elif per_semantic:
        per_image, ratios, _, *classes = eigen_class_scores(pred_disps, list(gt_depths), sem_masks, NUM_CLASSES, opt.eval_split,
                                                            opt.pred_depth_scale_factor, opt.disable_median_scaling)
        mean_errors = per_image.mean(0)
    else:
        per_image, ratios, _ = eigen_scores(pred_disps, list(gt_depths), opt.eval_split, opt.pred_depth_scale_factor,
                                            opt.disable_median_scaling)
        mean_errors = per_image.mean(0)
    if opt.visualize and not opt.eval_gdc:
        for a in range(0, len(gt_depths), 64):
            b = min(a + 64, len(gt_depths))
            save_visuals(vis_dir, opt.vis_name, a, gt_depths[a:b], opt.eval_split, pred_disps[a:b],
                         None if opt.disable_median_scaling else ratios[a:b], opt.pred_depth_scale_factor)
    if not opt.disable_median_scaling:
        med = np.median(ratios)
        print(" Scaling ratios | med: {:0.3f} | std: {:0.3f}".format(med, np.std(ratios / med)))
    print("\n  " + ("{:>8} | " * 7).format(*METRICS))
    print(("&{: 8.3f}  " * 7).format(*mean_errors.tolist()) + "\\\\")
    print("\n-> Done!")
    if not per_semantic:
        return mean_errors, ratios, per_image
    class_metrics, class_counts = classes
    abs_rel = semantic_summary(class_metrics, class_counts)
    pixel_count = class_counts.T.astype(np.float64)              # [34, N], float64 like the reference's np.zeros([34, 697])
    print("\n  {:>5} | {:>8} | {:>10}".format("class", "abs_rel", "pixels"))
    for c in np.nonzero(pixel_count.sum(1) > 0)[0]:
        print("  {:5d} | {: 8.3f} | {:10d}".format(c, abs_rel[c], int(pixel_count[c].sum())))
    os.makedirs(semantic_out, exist_ok=True)
    np.save(os.path.join(semantic_out, "{}.npy".format(opt.run_name if opt.run_name is not None else "per_semantic")), abs_rel)
    np.save(os.path.join(semantic_out, "pixel_count.npy"), pixel_count)
    return mean_errors, ratios, per_image, {"abs_rel": abs_rel, "pixel_count": pixel_count, "metrics": class_metrics}


def main(argv=None):
    from .options import MonodepthOptions
    found, rest = split_off_flags(sys.argv[1:] if argv is None else argv, SCRIPT_FLAGS)
    folders = (found["splits_dir"], found["semantic_dir"], found["semantic_out"])
    if found["vis_dir"] is not None:                              # a call without --vis_dir stays the call it was
        folders += (found["vis_dir"],)
    return evaluate(MonodepthOptions().parse(rest), *folders)


if __name__ == "__main__":
    main()
