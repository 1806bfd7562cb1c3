"""Timing of the Eigen-split scorer: ``evaluate_depth.eigen_scores`` (fd_eigen_scores, csrc/eigen_eval.hip) at N = 1, 64 and 697 images
against the per-image ATen loop ``evaluate_depth.evaluate_predictions`` on the same inputs, on the same box.  Inputs: 192x640
disparities, synthetic 375x1242 ground truth with 5 % valid pixels (8 distinct maps, cycled), the ``eigen`` split with median scaling.

    python scripts/bench_eval.py [--reps 10] [--out profiles/eigen_eval_time.log]
    python scripts/bench_eval.py --step detection [--reps 10] [--out profiles/detection_export_time.log]
    python scripts/bench_eval.py --step val [--reps 5] [--out profiles/val_time.log]
    python scripts/bench_eval.py --step completion_val [--reps 5] [--out profiles/completion_val_time.log]
    python scripts/bench_eval.py --step semantic [--reps 10] [--out profiles/eigen_class_time.log]
    python scripts/bench_eval.py --step visualize [--reps 10] [--out profiles/visualize_time.log]
    python scripts/bench_eval.py --step log_images [--reps 10] [--out profiles/log_images_time.log]
    python scripts/bench_eval.py --step pseudo_lidar [--reps 10] [--out profiles/pseudo_lidar_time.log]
    python scripts/bench_eval.py --step png_encode [--reps 5] [--out profiles/png_encode_time.log]

Per N: the library call alone between device events with everything resident (median, min, max), the upload of the packed ground
truth, the whole ``eigen_scores`` (packing on the host, uploads, calls in chunks of 64, the read-back) and the loop, both as wall time
around a synchronise.  The call's traffic bound: the ground truth inside the windows once, four taps per selected pixel, the compact
(gt, pred) lists written once and read once; at 6.3 TB/s (achievable HBM, as elsewhere in profiles/).

``--step detection``: the dense part of the detection export, ``detection.depth_export`` (fd_depth_export, csrc/detection.hip), at N = 1 and
64 maps of 375x1242 from 192x640 disparities with per-image ratios, against the recipe that was available before it: one
``FD.resize_linear_cv`` per image, the reciprocal and two multiplies in torch, ``.cpu()``, ``(x * 256).astype(np.uint16)``.  Both on the
same box in the same run, alternating, after the two were compared bit for bit.  Per N: the library call alone between device events
(uint16 output only, as the script calls it) with its traffic bound - the bytes written plus the source read once, at 6.3 TB/s -, the
recipe's device part between events, and both end to end (uploads of descriptors and ratios, the download) as wall time.

``--step val``: one in-training validation, ``Trainer.val`` (ResNet-18 at 192x640, batch 1, eval mode), over 64 and over 697 synthetic
batches (``synthetic.make_batch``; 8 distinct ones, cycled) with 375x1242 ground truth of which 5 % is valid: the fused route
(``trainer.val_gt`` = a resident ``validation.ValGroundTruth``: depths gathered on the device, ``fd_val_scores`` once per 64 images, one
download) against the route without it (``compute_depth_losses`` per batch: a boolean selection, two ``torch.median`` sorts, seven
``.cpu()`` copies), alternating in one run, wall time around a synchronise; median (min, max) of the rounds after one warm-up round.  Also
the scorer alone between device events with everything resident.  No loader runs here: the batches are in memory.

``--step completion_val``: the same for ``Completor.val`` (ResNet-18 at 352x1216, batch 1) over 64 and over 1000 synthetic batches with
352x1216 ground truth of which 15 % is valid: the fused route (``completor.val_scorer`` = a ``validation.CompletionValScorer``:
``fd_completion_val_scores`` once per 64 images, one download) against ``Completor.compute_depth_losses`` per batch, alternating; and the
scorer alone between device events for 1 and for 64 images.

``--step semantic``: ``--per_semantic``, the metrics per semantic class (34 classes, labels 0 .. 39 drawn uniformly, 8 distinct masks,
cycled) at N = 1 and 64 on the inputs of the first step.  The library call ``fd_eigen_class_scores`` against the plain
``fd_eigen_scores`` call on the same resident inputs, alternating, between device events: the increment is the price of the classes.
Beside it the class kernel's traffic: each of the 34 workgroups of an image reads the image's three compact lists whole (label, gt
and pred: 9 bytes per pair; the pairs of one class lie one in 40, so every cache line of the two float lists would be touched
anyway, and reading them unconditionally keeps the loads of 16 steps in flight together) - L2 traffic, the lists were written
just before; what reaches HBM is the plain call's bound plus 2 bytes per selected pixel (its label read from the plane, written to
the list).  Then ``eigen_class_scores`` end to end (host
packing, uploads of ground truth and labels, the call, one download) against the recipe it replaces - per image the ATen code of
``evaluate_predictions`` and 34 boolean selections with a ``compute_errors`` call each - alternating, wall time.

``--step visualize``: the two pictures of ``--visualize``, ``visualize.render`` (fd_vis_render, csrc/visualize.hip), at N = 1 and 64 maps of
375x1242 on the inputs of the first step with per-image ratios, against the device recipe it replaces - per image one
``FD.resize_linear_cv``, ``torch.sort`` for the percentile, a gather per table and ``max_pool2d`` - alternating in one run after the two
were compared byte for byte.  Per N: the library call alone between device events with its traffic bound (the source and the ground
truth read once, the pictures written once), the recipe's device part, both end to end with their downloads as wall time, and - for
orientation, once - the reference's host code for the colour picture (``np.percentile``, ``Normalize``, ``magma``) on 16 threads.

``--step log_images``: the image summaries of ``train --log_images``, ``log_images.render`` (fd_log_sheets, csrc/log_images.hip), at the
shape of a real run - 192x640, scales 0-3, frames [0, -1, 1], automask on - for J = 1 (the default ``eval_batch_size``) and J = 4 items,
against the ATen recipe it replaces: per tile a multiply, clamp, cast, permute and copy into the sheet, ``FD.bilinear_upsample`` of the
disparity, ``disp_to_depth``, back-projection, projection and ``F.grid_sample`` per source frame, a max and a min per disparity.  The two
alternate in one run after their sheets were compared (byte for byte outside the colour predictions, within one level inside).  Per J:
the library call alone between device events with its traffic bound (every source read once, the disparities twice, the sheets written
once), the recipe's device part, both end to end with their download as wall time - what a log event holds the step loop for - and
the PNG encoding of one sheet, which the default sink does on its background thread.

``--step pseudo_lidar``: the pseudo-LiDAR clouds of ``export_detection --pl_name``, ``detection.points_export`` (fd_points_export,
csrc/pseudo_lidar.hip), at N = 1 and 16 maps of 375x1242 with a KITTI camera, against the ATen recipe it replaces - per image a
meshgrid, the float64 expression of the point rule in torch, a boolean index per coordinate, a concatenation and a cast -
alternating in one run after the two were compared byte for byte.  Per N: the library call alone between device events with its
traffic bound (8 B x pixels: the depth read by the count and by the write pass; 16 B x kept points), the recipe's device part (also
with its meshgrid hoisted out of the loop), and both end to end with their downloads as wall time - ``points_export`` from a list of
maps and from the packed tensor ``depth_export`` hands over."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fusiondepth_amd import evaluate_depth as ED          # noqa: E402
from fusiondepth_amd import functional as FD              # noqa: E402
from fusiondepth_amd._lib import call, query, stream       # noqa: E402

HBM = 6.3e12


def inputs(n, rng):
    gts = []
    for _ in range(min(n, 8)):
        gt = rng.uniform(1.5, 90.0, (375, 1242)).astype(np.float32)
        gt[rng.rand(375, 1242) > 0.05] = 0.0
        gts.append(gt)
    gts = [gts[i % len(gts)] for i in range(n)]
    disps = torch.from_numpy(rng.uniform(0.02, 0.6, (min(n, 64), 192, 640)).astype(np.float32)).cuda()
    disps = disps[torch.arange(n, device="cuda") % disps.shape[0]].contiguous()
    return disps, gts


def events(fn, reps):
    ts = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts = np.array(ts[1:])
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def wall(fn, reps):
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts[1:]))


def library_call(disps, gts):
    """One resident fd_eigen_scores call over at most 64 images -> (callable, packed host tensor, bound in bytes, selected pixels)."""
    packed, desc = ED.pack_gt_depths(gts, "eigen")
    packed_d = packed.cuda()
    desc_d = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    rows = int((desc["y1"] - desc["y0"]).max())
    area = ((desc["y1"] - desc["y0"]).astype(np.int64) * (desc["x1"] - desc["x0"]))
    cap = int(area.sum())
    n = len(gts)
    ws = torch.empty((query("fd_eigen_scores_ws_bytes", n, rows, cap),), device="cuda", dtype=torch.uint8)
    out = torch.empty((n, 9), device="cuda", dtype=torch.float64)

    def run():
        call("fd_eigen_scores", disps.data_ptr(), disps.shape[0], 192, 640, packed_d.data_ptr(), packed_d.numel(), desc_d.data_ptr(), n, rows,
             cap, 1e-3, 80.0, 1.0, 1, 1e-3, 80.0, out.data_ptr(), ws.data_ptr(), stream())

    run()
    selected = int(out[:, 8].sum().item())
    bound = 4 * cap + 16 * selected + 16 * selected
    return run, packed, bound, selected


def alternate(fns, reps, timer):
    """The callables in turn, ``reps`` rounds after one warm-up round -> per callable (median, min, max) of ``timer(fn)`` [ms]."""
    ts = [[] for _ in fns]
    for _ in range(reps + 1):
        for k, fn in enumerate(fns):
            ts[k].append(timer(fn))
    return [(float(np.median(t[1:])), float(min(t[1:])), float(max(t[1:]))) for t in ts]


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def detection_step(a):
    from fusiondepth_amd import detection as D
    from fusiondepth_amd import functional as FD
    H, W, h, w = 375, 1242, 192, 640
    rng = np.random.RandomState(5)
    lines = ["Detection depth export, %dx%d disparities -> %dx%d uint16 maps with per-image ratios; median of %d (min, max) after one "
             "warm-up round, exporter and recipe alternating" % (h, w, H, W, a.reps)]
    for n in (1, 64):
        disps = torch.from_numpy(rng.uniform(0.02, 0.6, (n, h, w)).astype(np.float32)).cuda()
        ratios = rng.uniform(1.2, 1.4, n).astype(np.float32)
        ratios_t = [torch.tensor(r, dtype=torch.float32, device="cuda") for r in ratios]
        sizes = [(H, W)] * n
        desc, total = D.pack_export_sizes(sizes)
        desc_d = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
        ratio_d = torch.from_numpy(ratios).cuda()
        out = torch.empty((total,), device="cuda", dtype=torch.int16)

        def kernel():
            call("fd_depth_export", disps.data_ptr(), n, h, w, desc_d.data_ptr(), n, total, H, W, 1.0, ratio_d.data_ptr(), None, out.data_ptr(),
                 stream())

        def recipe_device():
            return [(1.0 / FD.resize_linear_cv(disps[i][None, None], (H, W))[0, 0]) * 1.0 * ratios_t[i] for i in range(n)]

        def recipe():
            return [((1.0 / FD.resize_linear_cv(disps[i][None, None], (H, W))[0, 0]) * 1.0 * ratios_t[i]).cpu().numpy() * 256 for i in range(n)]

        def recipe_all():
            return [x.astype(np.uint16) for x in recipe()]

        def exporter_all():
            return D.depth_export(disps, sizes, ratios=ratios)

        got, want = exporter_all(), recipe_all()                 # in range the recipe's cast is defined: the two agree bit for bit
        assert all(np.array_equal(g, x) for g, x in zip(got, want)), "exporter and recipe disagree"
        t_k, t_rd = alternate([kernel, recipe_device], a.reps, _event_ms)
        t_e, t_r = alternate([exporter_all, recipe_all], a.reps, _wall_ms)
        bound = 2 * total + 4 * n * h * w
        t_bound = 1e3 * bound / HBM
        lines.append("  N = %2d: fd_depth_export, resident, uint16 only: %.3f ms (%.3f, %.3f) = %.1f us / image; traffic bound %.2f MB = %.2f us "
                     "at 6.3 TB/s -> %.1fx the bound; the recipe's device part (%d launches): %.3f ms (%.3f, %.3f) -> %.2fx"
                     % (n, t_k[0], t_k[1], t_k[2], 1e3 * t_k[0] / n, bound / 1e6, 1e3 * t_bound, t_k[0] / t_bound, 4 * n, t_rd[0], t_rd[1], t_rd[2],
                        t_rd[0] / t_k[0]))
        lines.append("          depth_export end to end (descriptor and ratio uploads, 1 call, pinned download of %.1f MB): %.3f ms (%.3f, %.3f) "
                     "= %.3f ms / image; recipe end to end (float32 download, host * 256 and cast): %.3f ms (%.3f, %.3f) = %.3f ms / image -> %.2fx"
                     % (2 * total / 1e6, t_e[0], t_e[1], t_e[2], t_e[0] / n, t_r[0], t_r[1], t_r[2], t_r[0] / n, t_r[0] / t_e[0]))
    return lines


def pseudo_lidar_step(a):
    import types
    from fusiondepth_amd import detection as D
    H, W = 375, 1242
    rng = np.random.RandomState(5)
    # the camera and the Velodyne transform of a KITTI recording date (2011_09_26, rounded as published)
    cam = types.SimpleNamespace(c_u=609.5593, c_v=172.854, f_u=721.5377, f_v=721.5377, b_x=44.85728 / -721.5377, b_y=0.2163791 / -721.5377)
    R = np.array([[7.533745e-03, -9.999714e-01, -6.166020e-04], [1.480249e-02, 7.280733e-04, -9.998902e-01],
                  [9.998621e-01, 7.523790e-03, 1.480755e-02]])
    T = np.array([-4.069766e-03, -7.631618e-02, -2.717806e-01])
    R0 = np.array([[9.999239e-01, 9.837760e-03, -7.445048e-03], [-9.869795e-03, 9.999421e-01, -4.278459e-03],
                   [7.402527e-03, 4.351614e-03, 9.999631e-01]])
    A, t = R.T @ np.linalg.inv(R0), -(R.T @ T)
    calib = (cam, A, t)
    Ad, td = [[float(v) for v in row] for row in A], [float(v) for v in t]
    lines = ["Pseudo-LiDAR clouds, %dx%d float32 depth maps (uniform 2 .. 80 m), max_high 1.0; median of %d (min, max) after one warm-up round, "
             "the call and the ATen recipe alternating" % (H, W, a.reps)]
    vv, uu = torch.meshgrid(torch.arange(H, dtype=torch.float64, device="cuda"), torch.arange(W, dtype=torch.float64, device="cuda"), indexing="ij")

    def recipe_one(depth, grid=None):
        v, u = grid if grid is not None else torch.meshgrid(torch.arange(H, dtype=torch.float64, device="cuda"),
                                                            torch.arange(W, dtype=torch.float64, device="cuda"), indexing="ij")
        z = depth.to(torch.float64)
        x = ((u - cam.c_u) * z) / cam.f_u + cam.b_x
        y = ((v - cam.c_v) * z) / cam.f_v + cam.b_y
        X, Y, Z = (((Ad[r][0] * x + Ad[r][1] * y) + Ad[r][2] * z) + td[r] for r in range(3))
        keep = (X >= 0) & (Z < 1.0)
        return torch.cat([X[keep][:, None], Y[keep][:, None], Z[keep][:, None], torch.ones_like(X[keep])[:, None]], 1).to(torch.float32)

    for n in (1, 16):
        maps = [torch.from_numpy(rng.uniform(2.0, 80.0, (H, W)).astype(np.float32)).cuda() for _ in range(n)]
        calibs = [calib] * n
        desc, total = D.pack_export_sizes([(H, W)] * n)
        depth = torch.cat([m.reshape(-1) for m in maps])
        table = torch.from_numpy(np.concatenate([desc.view(np.uint8).reshape(-1),
                                                 np.stack([D.points_calib_row(*c) for c in calibs]).view(np.uint8).reshape(-1)])).cuda()
        ws = torch.empty((query("fd_points_export_ws_bytes", n, H),), device="cuda", dtype=torch.uint8)
        points = torch.empty((4 * total,), device="cuda", dtype=torch.float32)
        starts = torch.empty((n + 1,), device="cuda", dtype=torch.int64)

        def kernel():
            call("fd_points_export", depth.data_ptr(), table.data_ptr(), table.data_ptr() + desc.nbytes, n, total, H, W, 1.0, ws.data_ptr(),
                 points.data_ptr(), starts.data_ptr(), stream())

        def recipe_device():
            return [recipe_one(m) for m in maps]

        def recipe_device_grid():                                # the recipe with its meshgrid hoisted out: what a careful caller would write
            return [recipe_one(m, (vv, uu)) for m in maps]

        def recipe_all():
            return [c.cpu().numpy() for c in recipe_device()]

        def export_all():
            return D.points_export(maps, calibs, 1.0, chunk=16)

        def export_packed():                                     # as export_detection calls it: the maps already lie packed
            return D.points_export(None, calibs, 1.0, packed=(depth, desc))

        got, want = export_all(), recipe_all()
        assert all(g.shape == x.shape and np.array_equal(g.view(np.uint32), x.view(np.uint32)) for g, x in zip(got, want)), \
            "the call and the recipe disagree"
        assert all(np.array_equal(g, x) for g, x in zip(export_packed(), got))
        kept = sum(len(g) for g in got)
        t_k, t_rd, t_rg = alternate([kernel, recipe_device, recipe_device_grid], a.reps, _event_ms)
        t_e, t_p, t_r = alternate([export_all, export_packed, recipe_all], a.reps, _wall_ms)
        bound = 8 * total + 16 * kept
        t_bound = 1e3 * bound / HBM
        lines.append("  N = %2d (%d of %d pixels kept = %.2f; equal bytes): fd_points_export, resident, 3 launches: %.3f ms (%.3f, %.3f) = %.1f us / image; "
                     "traffic bound 8 B x pixels + 16 B x kept = %.2f MB = %.2f us at 6.3 TB/s -> %.1fx the bound; the recipe's device part: "
                     "%.3f ms (%.3f, %.3f) -> %.1fx, with the meshgrid hoisted %.3f ms (%.3f, %.3f) -> %.1fx"
                     % (n, kept, total, kept / total, t_k[0], t_k[1], t_k[2], 1e3 * t_k[0] / n, bound / 1e6, 1e3 * t_bound, t_k[0] / t_bound,
                        t_rd[0], t_rd[1], t_rd[2], t_rd[0] / t_k[0], t_rg[0], t_rg[1], t_rg[2], t_rg[0] / t_k[0]))
        lines.append("          points_export end to end (pack, table upload, 1 call, starts read-back, pinned download of %.1f MB, host split): "
                     "%.3f ms (%.3f, %.3f) = %.3f ms / image; from the packed tensor: %.3f ms (%.3f, %.3f); recipe end to end (a download per "
                     "image): %.3f ms (%.3f, %.3f) = %.3f ms / image -> %.2fx (packed: %.2fx)%s"
                     % (16 * kept / 1e6, t_e[0], t_e[1], t_e[2], t_e[0] / n, t_p[0], t_p[1], t_p[2], t_r[0], t_r[1], t_r[2], t_r[0] / n,
                        t_r[0] / t_e[0], t_r[0] / t_p[0], "" if t_r[0] > t_e[0] else "  THE RECIPE WINS HERE"))
    return lines


def visualize_step(a):
    from concurrent.futures import ThreadPoolExecutor
    from fusiondepth_amd import visualize as V
    H, W, h, w = 375, 1242, 192, 640
    rng = np.random.RandomState(5)
    lut_disp, lut_err = V.magma_lut(), V.hue_lut()
    luts = torch.from_numpy(np.concatenate([lut_disp, lut_err])).cuda()
    lut_d, lut_e = luts[:256], luts[256:]
    lines = ["evaluate_depth --visualize, %dx%d disparities -> %dx%d colour and %dx%d error pictures, eigen split, per-image ratios, 5 %% "
             "valid ground truth; median of %d (min, max) after one warm-up round, renderer and recipe alternating"
             % (h, w, H, W, (H + 1) // 2, (W + 1) // 2, a.reps)]
    y0, y1, x0, x1 = ED.split_window("eigen", H, W)
    for n in (1, 64):
        disps, gts = inputs(n, rng)
        ratios = rng.uniform(1.2, 1.4, n).astype(np.float32)
        ratios_t = [torch.tensor(r, dtype=torch.float32, device="cuda") for r in ratios]
        packed, desc = ED.pack_gt_depths(gts, "eigen")
        total = packed.numel()
        packed_d, desc_d, ratio_d = packed.cuda(), torch.from_numpy(desc.view(np.uint8).copy()).cuda(), torch.from_numpy(ratios).cuda()
        gts_d = [packed_d[int(d["offset"]):int(d["offset"]) + H * W].view(H, W) for d in desc]
        err_pixels = n * ((H + 1) // 2) * ((W + 1) // 2)
        out = torch.empty((3 * total + 3 * err_pixels,), device="cuda", dtype=torch.uint8)
        ws = torch.empty((query("fd_vis_render_ws_bytes", n, total),), device="cuda", dtype=torch.uint8)

        def kernel():
            call("fd_vis_render", disps.data_ptr(), n, h, w, 1.0, ratio_d.data_ptr(), None, packed_d.data_ptr(), total, desc_d.data_ptr(), n,
                 H * W, 1e-3, 80.0, lut_d.data_ptr(), lut_e.data_ptr(), out.data_ptr(), out.data_ptr() + 3 * total, err_pixels, None, None,
                 ws.data_ptr(), stream())

        def recipe_device():
            """The pictures from what the package offered before: one resize per image, a sort for the percentile, gathers, a pool."""
            res = []
            for i in range(n):
                depth = (1.0 / FD.resize_linear_cv(disps[i][None, None], (H, W))[0, 0]) * 1.0 * ratios_t[i]
                d = 1.0 / depth
                s, _ = torch.sort(d.reshape(-1))
                m = s.numel()
                pos = np.float32(m - 1) * (np.float32(95.0) / np.float32(100.0))
                k = int(np.floor(pos))
                g = float(np.float32(pos - np.float32(k)))
                lo, hi = s[k], s[min(k + 1, m - 1)]
                vmax = hi - (hi - lo) * (1.0 - g) if g >= 0.5 else lo + (hi - lo) * g
                vmax = torch.where(lo == hi, lo, vmax)
                xn = ((d - s[0]).double() / (vmax.double() - s[0].double())).float()
                xa = xn * 256.0
                color = lut_d[torch.where(xa >= 256.0, torch.full_like(xa, 255.0), xa).clamp_(0, 255).long()]
                gt = gts_d[i]
                mask = (gt > ED.MIN_DEPTH) & (gt < ED.MAX_DEPTH)
                crop = torch.zeros_like(mask)
                crop[y0:y1, x0:x1] = True
                mask = mask & crop
                v = (80.0 - torch.clamp(torch.abs(depth - gt), 0, 2) * 40.0).long().clamp_(0, 255)
                col = lut_e[v] * mask[:, :, None]
                small = torch.nn.functional.max_pool2d(col.permute(2, 0, 1)[None].float(), 2, ceil_mode=True)[0].permute(1, 2, 0)
                small = torch.where((small == 0).all(2, keepdim=True), torch.full_like(small, 220.0), small).to(torch.uint8)
                res.append((color, small))
            return res

        def recipe_all():
            return [(c.cpu().numpy(), e.cpu().numpy()) for c, e in recipe_device()]

        def render_all():
            return V.render(disps, gts, ratios, "eigen")

        def host_all():
            """The reference's host code per image (:437-441), 16 threads; the depth maps are given."""
            def one(depth):
                disp = 1 / depth
                mapper = cm.ScalarMappable(norm=mpl.colors.Normalize(vmin=disp.min(), vmax=np.percentile(disp, 95)), cmap="magma")
                return (mapper.to_rgba(disp)[:, :, :3] * 255).astype(np.uint8)

            with ThreadPoolExecutor(16) as ex:
                return list(ex.map(one, host_depths))

        got, want = render_all(), recipe_all()                   # same bytes before anything is timed
        for i in range(n):
            assert np.array_equal(got[0][i], want[i][0]) and np.array_equal(got[1][i], want[i][1]), "renderer and recipe disagree at image %d" % i
        t_k, t_rd = alternate([kernel, recipe_device], a.reps if n == 1 else max(3, a.reps // 3), _event_ms)
        t_e, t_r = alternate([render_all, recipe_all], a.reps if n == 1 else max(3, a.reps // 3), _wall_ms)
        try:
            import matplotlib as mpl
            from matplotlib import cm
            cm.ScalarMappable(cmap="magma").to_rgba(np.zeros((2, 2), np.float32))      # first use builds the table: not timed
            host_depths =[m.cpu().numpy() for m in V.render(disps, gts, ratios, "eigen", want_depth=True)[2]]
            t0 = time.perf_counter()
            host = host_all()
            t_h = 1e3 * (time.perf_counter() - t0)
            assert all(np.array_equal(a_, b_) for a_, b_ in zip(host, got[0])), "matplotlib and the renderer disagree"
            host_text = "host numpy + matplotlib for the colour picture alone, 16 threads, maps given: %.1f ms = %.2f ms / image" % (t_h, t_h / n)
        except ImportError:
            host_text = "matplotlib is not installed: no host figure"
        bound = 4 * n * h * w + 4 * total + 3 * total + 3 * err_pixels
        t_bound = 1e3 * bound / HBM
        lines.append("  N = %2d: fd_vis_render, resident, both pictures (9 launches): %.3f ms (%.3f, %.3f) = %.1f us / image; traffic bound (source and "
                     "ground truth read once, pictures written once) %.2f MB = %.2f us at 6.3 TB/s -> %.1fx the bound; the recipe's device part: "
                     "%.3f ms (%.3f, %.3f) -> %.2fx"
                     % (n, t_k[0], t_k[1], t_k[2], 1e3 * t_k[0] / n, bound / 1e6, 1e3 * t_bound, t_k[0] / t_bound, t_rd[0], t_rd[1], t_rd[2],
                        t_rd[0] / t_k[0]))
        lines.append("          render end to end (host packing, upload of %.1f MB ground truth, 1 call, pinned download of %.1f MB): %.2f ms (%.2f, "
                     "%.2f) = %.3f ms / image; recipe end to end (two downloads per image): %.2f ms (%.2f, %.2f) = %.3f ms / image -> %.2fx; %s"
                     % (4 * total / 1e6, out.numel() / 1e6, t_e[0], t_e[1], t_e[2], t_e[0] / n, t_r[0], t_r[1], t_r[2], t_r[0] / n,
                        t_r[0] / t_e[0], host_text))
    return lines


def log_images_step(a):
    import ctypes
    import torch.nn.functional as F
    from fusiondepth_amd import log_images as L
    from fusiondepth_amd import synthetic
    from fusiondepth_amd.layers import disp_to_depth
    H, W, B = 192, 640, 4
    frame_ids, scales = [0, -1, 1], [0, 1, 2, 3]
    inputs_ = synthetic.make_scene_batch(B, H, W, frame_ids=frame_ids, seed=5)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(6)
    outputs = {}
    for s in scales:
        coarse = torch.rand(B, 1, 6, 20, device="cuda", generator=gen)
        outputs[("disp", s)] = (0.02 + 0.6 * F.interpolate(coarse, size=(H >> s, W >> s), mode="bilinear", align_corners=False)).contiguous()
        outputs[("sel", s)] = (torch.randint(0, 4, (B, H, W), device="cuda", dtype=torch.uint8, generator=gen), 2)
    Ts = {f: inputs_[("T_gt", f)].contiguous() for f in frame_ids[1:]}
    K, inv_K = inputs_[("K", 0)], inputs_[("inv_K", 0)]
    lines = ["train --log_images, %dx%d, scales 0-3, frames [0, -1, 1], automask: one contact sheet per item; median of %d (min, max) after "
             "one warm-up round, renderer and recipe alternating" % (H, W, a.reps)]

    def q8(x):
        return (x * 255.0).clamp_(0, 255).to(torch.uint8)

    for J in (1, 4):
        lay = L.layout(frame_ids, scales, H, W, J=J)
        per = len(lay.tiles) // J

        def recipe_device():
            """The sheets from what the package offered before: a few small ATen launches per tile."""
            sheets = torch.zeros((J, lay.Hs, lay.Ws, 3), device="cuda", dtype=torch.uint8)
            disp0 = FD.bilinear_upsample(outputs[("disp", 0)][:J], (H, W))
            depth = disp_to_depth(disp0, 0.1, 100.0)[1]
            cam = FD.backproject_depth(depth, inv_K[:J])
            pred = {f: F.grid_sample(inputs_[("color", f, 0)][:J], FD.project_3d(cam, K[:J], Ts[f][:J], H, W, 1e-7), padding_mode="border",
                                     align_corners=False) for f in frame_ids[1:]}
            for t in lay.tiles:
                j = t.item
                if t.kind == L.KIND_COLOR:
                    tile = q8(inputs_[("color", t.frame, t.scale)][j]).permute(1, 2, 0)
                elif t.kind == L.KIND_PRED:
                    tile = q8(pred[t.frame][j]).permute(1, 2, 0)
                elif t.kind == L.KIND_DISP:
                    x = outputs[("disp", t.scale)][j, 0]
                    ma, mi = x.max(), x.min()
                    d = torch.where(ma == mi, torch.full_like(ma, 1e5), (ma.double() - mi.double()).float())
                    tile = q8((x - mi) / d)[:, :, None]
                else:
                    sel, n_id = outputs[("sel", t.scale)]
                    tile = q8((sel[j] > n_id - 1).float())[:, :, None]
                sheets[j, t.y:t.y + t.h, t.x:t.x + t.w] = tile
            return sheets

        def recipe_all():
            with torch.no_grad():
                return recipe_device().cpu().numpy()

        def render_all():
            return L.render(inputs_, outputs, frame_ids, scales, J, Ts=Ts)

        # the resident call: the table render builds, kept on the device
        key = (tuple(frame_ids), tuple(scales), H, W, J, True, False, False, (H, W))
        _, cfg, template, NT = L._plan(key, 0.1, 100.0)
        table = type(template)()
        ctypes.memmove(table, template, ctypes.sizeof(table))
        for j in range(J):
            for i, t in enumerate(lay.tiles[:per]):
                e = table[j * NT + i]
                if t.kind in (L.KIND_COLOR, L.KIND_PRED):
                    e.p0 = inputs_[("color", t.frame, t.scale)][j].data_ptr()
                if t.kind == L.KIND_PRED:
                    e.p1, e.p2, e.p3, e.p4 = outputs[("disp", 0)][j].data_ptr(), K[j].data_ptr(), inv_K[j].data_ptr(), Ts[t.frame][j].data_ptr()
                elif t.kind == L.KIND_DISP:
                    e.p0 = outputs[("disp", t.scale)][j].data_ptr()
                elif t.kind == L.KIND_AUTOMASK:
                    e.p0, e.aux = outputs[("sel", t.scale)][0][j].data_ptr(), 2
        table_d = torch.from_numpy(np.frombuffer(table, dtype=np.uint8).copy()).cuda()
        ws = torch.empty((query("fd_log_sheets_ws_bytes", J, cfg.n_disp),), device="cuda", dtype=torch.uint8)
        out = torch.empty((J, lay.Hs, lay.Ws, 3), device="cuda", dtype=torch.uint8)

        def kernel():
            call("fd_log_sheets", ctypes.addressof(table), table_d.data_ptr(), J, NT, ctypes.addressof(cfg), out.data_ptr(), ws.data_ptr(), stream())

        got, want = render_all()[0], recipe_all()                # the same pictures before anything is timed
        kernel()
        assert np.array_equal(out.cpu().numpy(), got), "the resident call and render disagree"
        warp_diff = 0
        for t in lay.tiles:
            g, w_ = got[t.item, t.y:t.y + t.h, t.x:t.x + t.w], want[t.item, t.y:t.y + t.h, t.x:t.x + t.w]
            if t.kind == L.KIND_PRED:
                d = np.abs(g.astype(np.int32) - w_.astype(np.int32))
                assert d.max() <= 1, "renderer and recipe disagree at %s" % t.tag
                warp_diff = max(warp_diff, float((d != 0).mean()))
                want[t.item, t.y:t.y + t.h, t.x:t.x + t.w] = g
        assert np.array_equal(got, want), "renderer and recipe disagree outside the colour predictions"
        t_k, t_rd = alternate([kernel, recipe_device], a.reps, _event_ms)
        t_e, t_r = alternate([render_all, recipe_all], a.reps, _wall_ms)
        with tempfile.TemporaryDirectory() as tmp:
            t0 = time.perf_counter()
            L.write_png(os.path.join(tmp, "sheet.png"), got[0])
            t_png = 1e3 * (time.perf_counter() - t0)
        read = 0
        for t in lay.tiles:
            read += {L.KIND_COLOR: 12, L.KIND_PRED: 16, L.KIND_DISP: 8, L.KIND_AUTOMASK: 1}[t.kind] * t.h * t.w
        bound = read + out.numel()
        t_bound = 1e3 * bound / HBM
        lines.append("  J = %d (%d tiles, sheets %dx%d): fd_log_sheets, resident (2 launches + 1 memset): %.3f ms (%.3f, %.3f); traffic bound (sources "
                     "read once, disparities twice, sheets written once) %.2f MB = %.2f us at 6.3 TB/s -> %.1fx the bound; the recipe's device "
                     "part: %.3f ms (%.3f, %.3f) -> %.2fx; colour-prediction bytes that differ from the recipe's grid_sample: %.5f"
                     % (J, len(lay.tiles), lay.Hs, lay.Ws, t_k[0], t_k[1], t_k[2], bound / 1e6, 1e3 * t_bound, t_k[0] / t_bound, t_rd[0], t_rd[1],
                        t_rd[2], t_rd[0] / t_k[0], warp_diff))
        lines.append("          render end to end (checks, table upload, 1 call, pinned download of %.1f MB) = what a log event holds the step loop for: "
                     "%.2f ms (%.2f, %.2f); recipe end to end (one download): %.2f ms (%.2f, %.2f) -> %.2fx; PNG encoding of one sheet "
                     "(PIL, the sink's background thread): %.1f ms"
                     % (out.numel() / 1e6, t_e[0], t_e[1], t_e[2], t_r[0], t_r[1], t_r[2], t_r[0] / t_e[0], t_png))
    return lines


def semantic_step(a):
    K = 34
    rng = np.random.RandomState(5)
    lines = ["Per-class Eigen-split scores (--per_semantic), 192x640 disparities, 375x1242 ground truth with 5 %% valid pixels, %d classes "
             "(labels 0 .. 39), eigen split, median scaling; median (min, max) of %d rounds (3 for the recipe at N = 64) after one warm-up "
             "round, the two routes alternating" % (K, a.reps)]
    masks = [rng.randint(0, 40, (375, 1242)).astype(np.uint8) for _ in range(8)]
    for n in (1, 64):
        disps, gts = inputs(n, rng)
        sems = [masks[i % 8] for i in range(n)]
        plain, packed, bound, selected = library_call(disps, gts)
        _, desc = ED.pack_gt_depths(gts, "eigen")
        packed_d, desc_d = packed.cuda(), torch.from_numpy(desc.view(np.uint8).copy()).cuda()
        labels = ED.pack_labels(sems, desc)
        labels_d = labels.cuda()
        rows = int((desc["y1"] - desc["y0"]).max())
        cap = int(((desc["y1"] - desc["y0"]).astype(np.int64) * (desc["x1"] - desc["x0"])).sum())
        ws = torch.empty((query("fd_eigen_class_scores_ws_bytes", n, rows, cap, K),), device="cuda", dtype=torch.uint8)
        out = torch.empty((n, 9), device="cuda", dtype=torch.float64)
        class_out = torch.empty((n, K, 8), device="cuda", dtype=torch.float64)

        def classes():
            call("fd_eigen_class_scores", disps.data_ptr(), disps.shape[0], 192, 640, packed_d.data_ptr(), packed_d.numel(), desc_d.data_ptr(), n,
                 rows, cap, 1e-3, 80.0, 1.0, 1, 1e-3, 80.0, labels_d.data_ptr(), K, out.data_ptr(), class_out.data_ptr(), ws.data_ptr(), stream())

        def recipe():
            """evaluate_depth.py:344-478 with :451-467 in ATen, as ``evaluate_predictions`` spells the loop."""
            res = []
            for i in range(n):
                gt = torch.as_tensor(gts[i], dtype=torch.float32).cuda()
                sem = torch.as_tensor(sems[i]).cuda()
                gh, gw = gt.shape
                pred = 1.0 / FD.resize_linear_cv(disps[i][None, None], (gh, gw))[0, 0]
                mask = (gt > ED.MIN_DEPTH) & (gt < ED.MAX_DEPTH)
                c = ED.garg_crop(gh, gw)
                crop = torch.zeros_like(mask)
                crop[c[0]:c[1], c[2]:c[3]] = True
                mask = mask & crop
                pred = pred * (ED._median(gt[mask]) / ED._median(pred[mask]))
                per_class = []
                for k in range(K):
                    final = mask & (sem == k)
                    if int(final.sum()) > 0:
                        per_class.append(ED.compute_errors(gt[final], torch.clamp(pred[final], ED.MIN_DEPTH, ED.MAX_DEPTH)))
                    else:
                        per_class.append((0.0,) * 7)
                res.append(per_class)
                ED.compute_errors(gt[mask], torch.clamp(pred[mask], ED.MIN_DEPTH, ED.MAX_DEPTH))
            return np.array(res)

        def whole():
            return ED.eigen_class_scores(disps, gts, sems, K)

        got, want = whole()[3], recipe()
        worst = float(np.abs(got[:, :, 0] - want[:, :, 0]).max() / np.abs(want[:, :, 0]).max())
        assert worst < 1e-4, "eigen_class_scores and the recipe disagree: %g" % worst
        t_c, t_p = alternate([classes, plain], a.reps, _event_ms)
        in_classes = int(class_out[:, :, 7].sum().item())
        class_bytes = K * selected * 9 + n * K * 64
        t_e, t_r = alternate([whole, recipe], a.reps if n == 1 else 3, _wall_ms)
        lines.append("  N = %2d: fd_eigen_class_scores, resident (%d selected pixels, %d of them in a class): %.3f ms (%.3f, %.3f); fd_eigen_scores on "
                     "the same inputs: %.3f ms (%.3f, %.3f) -> the classes cost %.3f ms = %.1f us / image (%.2fx the plain call); the class kernel's "
                     "%d workgroups read %.2f MB from the L2, %.2f TB/s over the increment; HBM bound of the call %.2f MB = %.2f us at 6.3 TB/s"
                     % (n, selected, in_classes, t_c[0], t_c[1], t_c[2], t_p[0], t_p[1], t_p[2], t_c[0] - t_p[0], 1e3 * (t_c[0] - t_p[0]) / n,
                        t_c[0] / t_p[0], n * K, class_bytes / 1e6, class_bytes / (1e9 * (t_c[0] - t_p[0])), (bound + 2 * selected) / 1e6,
                        1e6 * (bound + 2 * selected) / HBM))
        lines.append("          eigen_class_scores end to end (host packing, uploads of %.1f MB ground truth and %.1f MB labels, 1 call, 1 download): "
                     "%.2f ms (%.2f, %.2f) = %.3f ms / image; the recipe (per image the ATen loop, %d selections and compute_errors calls): "
                     "%.2f ms (%.2f, %.2f) = %.3f ms / image -> %.2fx; abs_rel per class differs by at most %.1e of the largest"
                     % (packed.numel() * 4 / 1e6, labels.numel() / 1e6, t_e[0], t_e[1], t_e[2], t_e[0] / n, K, t_r[0], t_r[1], t_r[2], t_r[0] / n,
                        t_r[0] / t_e[0], worst))
    return lines


def val_step(a):
    from fusiondepth_amd import synthetic
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.trainer import Trainer
    from fusiondepth_amd.validation import ValGroundTruth
    rng = np.random.RandomState(5)
    torch.manual_seed(1)
    opt = MonodepthOptions().parse(["--num_layers", "18", "--weights_init", "scratch", "--log_dir", tempfile.mkdtemp(prefix="fd_bench_val_")])
    tr = Trainer(opt, verbose=False)
    distinct = []
    for k in range(8):
        b = synthetic.make_batch(1, 192, 640, frame_ids=(0,), seed=40 + k)
        gt = rng.uniform(1.5, 80.0, (375, 1242)).astype(np.float32)
        gt[rng.rand(375, 1242) > 0.05] = 0.0
        b["depth_gt"] = torch.from_numpy(gt).cuda()[None, None]
        distinct.append((b, gt))
    lines = ["In-training validation, Trainer.val (ResNet-18 at 192x640, batch 1, eval mode) over N in-memory synthetic batches, 375x1242 "
             "ground truth with 5 % valid pixels; fused route (val_gt) and compute_depth_losses route alternating in one run, wall time; "
             "median (min, max) of the rounds after one warm-up round"]
    for n in (64, 697):
        reps = a.reps if n <= 64 else max(2, a.reps // 2)
        batches = [distinct[i % 8][0] for i in range(n)]
        vg = ValGroundTruth([distinct[i % 8][1] for i in range(n)])

        def fused():
            tr.val_gt = vg
            return tr.val(batches, save_best=False)

        def plain():
            tr.val_gt = None
            return tr.val(batches, save_best=False)

        f, p = fused(), plain()
        worst = max(abs(float(f[m]) - float(p[m])) / abs(float(p[m])) for m in tr.depth_metric_names)
        (t_f, t_p) = alternate([fused, plain], reps, _wall_ms)
        depths = tr._val_depths
        t_s = alternate([lambda: vg.score(depths)], reps, _event_ms)[0]
        selected = int(vg.out[:, 8].sum().item())
        lines.append("  N = %3d, %d rounds: fused %.1f ms (%.1f, %.1f) = %.3f ms / image; compute_depth_losses route %.1f ms (%.1f, %.1f) = %.3f ms "
                     "/ image -> %.2fx (medians); the two routes' mean metrics differ by at most %.1e relative"
                     % (n, reps, t_f[0], t_f[1], t_f[2], t_f[0] / n, t_p[0], t_p[1], t_p[2], t_p[0] / n, t_p[0] / t_f[0], worst))
        lines.append("           fd_val_scores alone, resident ground truth (%.0f MB), %d call(s), %d selected pixels: %.3f ms (%.3f, %.3f) = "
                     "%.1f us / image" % (vg.packed.numel() * 4 / 1e6, len(vg.chunks), selected, t_s[0], t_s[1], t_s[2], 1e3 * t_s[0] / n))
        tr.val_gt = None
        del vg
    return lines


def completion_val_step(a):
    from fusiondepth_amd import synthetic
    from fusiondepth_amd.completor import Completor
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.validation import CompletionValScorer
    H, W = 352, 1216
    rng = np.random.RandomState(5)
    torch.manual_seed(1)
    opt = MonodepthOptions().parse(["--num_layers", "18", "--completion_num_layers", "18", "--completion_pose_num_layers", "18",
                                    "--weights_init", "scratch", "--log_dir", tempfile.mkdtemp(prefix="fd_bench_cval_")])
    cp = Completor(opt, verbose=False)
    distinct = []
    for k in range(8):
        b = synthetic.make_batch(1, H, W, frame_ids=(0,), seed=40 + k)
        gt = rng.uniform(1.5, 80.0, (H, W)).astype(np.float32)
        gt[rng.rand(H, W) > 0.15] = 0.0
        b["depth_gt"] = torch.from_numpy(gt).cuda()[None, None]
        distinct.append(b)
    lines = ["In-training validation, Completor.val (ResNet-18 at %dx%d, batch 1, eval mode) over N in-memory synthetic batches, ground "
             "truth with 15 %% valid pixels; fused route (val_scorer) and compute_depth_losses route alternating in one run, wall time; "
             "median (min, max) of the rounds after one warm-up round" % (H, W)]
    for n in (64, 1000):
        reps = a.reps if n <= 64 else max(3, a.reps // 3)
        batches = [distinct[i % 8] for i in range(n)]
        scorer = CompletionValScorer(n, (H, W), (H, W))

        def fused():
            cp.val_scorer = scorer
            return cp.val(batches, save_best=False)[0]

        def plain():
            cp.val_scorer = None
            return cp.val(batches, save_best=False)[0]

        f, p = fused(), plain()
        worst = max(abs(float(f[m]) - float(p[m])) / abs(float(p[m])) for m in cp.depth_metric_names)
        (t_f, t_p) = alternate([fused, plain], reps, _wall_ms)
        spread = max(t_f[2] - t_f[1], t_p[2] - t_p[1])
        lines.append("  N = %4d, %d rounds: fused %.1f ms (%.1f, %.1f) = %.3f ms / image; compute_depth_losses route %.1f ms (%.1f, %.1f) = %.3f ms "
                     "/ image -> %.2fx (medians); difference of the medians %.1f ms against the larger spread %.1f ms; the two routes' mean "
                     "metrics differ by at most %.1e relative"
                     % (n, reps, t_f[0], t_f[1], t_f[2], t_f[0] / n, t_p[0], t_p[1], t_p[2], t_p[0] / n, t_p[0] / t_f[0], t_p[0] - t_f[0], spread,
                        worst))
        cp.val_scorer = None
        del scorer
    for n in (1, 64):                                            # the scorer alone, everything resident: one library call
        scorer = CompletionValScorer(n, (H, W), (H, W))
        depth = torch.from_numpy(rng.uniform(1.0, 80.0, (n, 1, H, W)).astype(np.float32)).cuda()
        gts = torch.cat([distinct[i % 8]["depth_gt"] for i in range(n)])
        scorer.begin()
        scorer.add(depth, gts)
        scorer.finish()
        selected = int(scorer.out[:, 8].sum().item())

        def call_only():
            scorer.filled, scorer.seen = n, n
            scorer._flush()

        t_s = alternate([call_only], a.reps, _event_ms)[0]
        lines.append("  fd_completion_val_scores alone, %d image(s) resident, 1 call, %d selected pixels: %.3f ms (%.3f, %.3f) = %.1f us / image"
                     % (n, selected, t_s[0], t_s[1], t_s[2], 1e3 * t_s[0] / n))
    return lines


def png_encode_step(a):
    """Batch PNG encoding: image_codecs.encode_png_batch against Pillow on 16 threads, the routes alternating, after a decode-and-compare
    of both outputs.  Maps: fd_depth_export's uint16 payload of textured synthetic disparities; sheets: 768x4480 RGB contact sheets
    with a black background (textured tiles and a flat grey one)."""
    import concurrent.futures
    import ctypes
    import io
    from PIL import Image
    from fusiondepth_amd import image_codecs as DO
    from fusiondepth_amd import detection as D
    H, W, h, w = 375, 1242, 192, 640
    rng = np.random.RandomState(5)
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=16)
    lines = ["PNG encoding, image_codecs.encode_png_batch (3 launches) against Image.save on 16 threads after the download; median of %d "
             "(min, max) after one warm-up round, the routes alternating" % a.reps]

    def pil_one(arr):
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, format="PNG")
        return buf.getvalue()

    def case(name, images):
        n = len(images)
        total_px = sum(int(x.numel()) * x.element_size() for x in images)

        def device_all():
            return DO.encode_png_batch(images, pool)

        def pil_all():
            host = [x.cpu().numpy() for x in images]
            return list(pool.map(pil_one, host))

        files, stats = device_all()
        theirs = pil_all()
        for x, f, g in zip(images, files, theirs):               # both routes decode to the input
            want = x.cpu().numpy()
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(bytes(f)))), want), "the device's file does not decode to its input"
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(g))), want)
        back, st = DO.decode_png_batch([bytes(f) for f in files], mode="gray16" if images[0].dim() == 2 else "rgb")
        assert st["fallback"] == 0 and all(torch.equal(b, x) for b, x in zip(back, images)), "decode_png_batch of the files differs"
        # the launches alone: the two library calls on resident buffers, with the plan of the first run
        job = DO.PngEncodeJob(images, pool)
        words = job.stats_words()
        blocks = torch.empty((job.sizes.blocks * ctypes.sizeof(DO._lib.PngEncBlock),), dtype=torch.uint8, pin_memory=True)
        _, total = DO.png_enc_plan(job.table, n, words, blocks.data_ptr())
        room = (total + 3) // 4 * 4 + 4
        out = torch.empty((room,), dtype=torch.uint8, device="cuda")

        def launches():
            call("fd_png_enc_filter", job.work.data_ptr(), job.sizes.work_bytes, ctypes.addressof(job.table), n, stream())
            call("fd_png_enc_emit", job.work.data_ptr(), job.sizes.work_bytes, ctypes.addressof(job.table), n, blocks.data_ptr(), out.data_ptr(),
                 room, stream())

        t_k, = alternate([launches], a.reps, _event_ms)
        for run in (1, 2):
            t_d, t_p = alternate([device_all, pil_all], a.reps, _wall_ms)
            lines.append("  %s, run %d: encode_png_batch end to end %.2f ms (%.2f, %.2f) = %.2f ms / image; Pillow on 16 threads (download, "
                         "Image.save) %.2f ms (%.2f, %.2f) = %.2f ms / image -> %.2fx"
                         % (name, run, t_d[0], t_d[1], t_d[2], t_d[0] / n, t_p[0], t_p[1], t_p[2], t_p[0] / n, t_p[0] / t_d[0]))
        raw = stats["raw_bytes"]
        bound = total_px + 3 * raw + 2 * stats["bytes"]             # pixels read; workspace written, read twice; output cleared, written
        lines.append("      the three launches with their clears and uploads, resident: %.3f ms (%.3f, %.3f); traffic bound %.1f MB = %.1f us at "
                     "6.3 TB/s -> %.0fx the bound.  File bytes: device %d, Pillow %d (%+.1f %%), raw scanlines %d"
                     % (t_k[0], t_k[1], t_k[2], bound / 1e6, 1e6 * bound / HBM, t_k[0] / (1e3 * bound / HBM), stats["bytes"],
                        sum(len(g) for g in theirs), 100.0 * (stats["bytes"] / sum(len(g) for g in theirs) - 1.0), raw))

    for n in (1, 16, 64):
        base = rng.uniform(0.02, 0.6, (n, h // 8, w // 8)).astype(np.float32)
        disp = torch.nn.functional.interpolate(torch.from_numpy(base)[:, None], size=(h, w), mode="bicubic", align_corners=False)[:, 0]
        disp = (disp + torch.from_numpy(rng.uniform(-0.004, 0.004, (n, h, w)).astype(np.float32))).clamp_(0.01, 1.0).cuda()
        maps = D.depth_export(disp, [(H, W)] * n, want_device=True)
        case("%2d maps of %dx%d uint16" % (n, H, W), maps)
    for n in (1, 4):
        sheet = np.zeros((n, 768, 4480, 3), np.uint8)
        for j in range(n):
            for ty in range(4):
                for tx in range(6):
                    tile = rng.randint(0, 256, (24, 80, 3)).astype(np.float32)
                    big = torch.nn.functional.interpolate(torch.from_numpy(tile).permute(2, 0, 1)[None], size=(192, 640), mode="bilinear")[0]
                    noise = torch.from_numpy(rng.randint(-6, 7, (3, 192, 640)).astype(np.float32))
                    sheet[j, 192 * ty:192 * ty + 192, 640 * tx:640 * tx + 640] = (big + noise).clamp(0, 255).permute(1, 2, 0).numpy().astype(np.uint8)
            sheet[j, 576:768, 1280:1920] = 220
        sheets = torch.from_numpy(sheet).cuda()
        case("%d sheets of 768x4480 RGB" % n, [sheets[j] for j in range(n)])
    pool.shutdown()
    return lines + png_encode_commands(a)


def _verdict(name, unit, runs, higher_is_better):
    """The recommendation rule: ``--png_encoder device`` is recommended for a command only if its gain exceeds the larger run-to-run
    spread (max - min of either route) in BOTH runs; otherwise the line says that it lost or tied, and by how much."""
    gains, spreads = [], []
    for pil, dev in runs:
        gains.append((dev[0] - pil[0]) if higher_is_better else (pil[0] - dev[0]))
        spreads.append(max(pil[2] - pil[1], dev[2] - dev[1]))
    text = ", ".join("%+.3g against a spread of %.3g" % (g, s) for g, s in zip(gains, spreads))
    if all(g > s for g, s in zip(gains, spreads)):
        return "  %s: gain of device over pil per run [%s]: %s -> --png_encoder device is RECOMMENDED" % (name, unit, text)
    if all(-g > s for g, s in zip(gains, spreads)):
        return "  %s: gain of device over pil per run [%s]: %s -> --png_encoder device LOST; not recommended" % (name, unit, text)
    return "  %s: gain of device over pil per run [%s]: %s -> inside the spread in at least one run; NOT recommended" % (name, unit, text)


def png_encode_commands(a):
    """The two commands that write PNGs, each with ``--png_encoder pil`` and ``device``, twice, the routes alternating, after a
    decode-and-compare of both outputs.  ``export_detection``: wall time of the command on a synthetic object tree (tests/
    detection_tree.py, 32 images of two KITTI sizes) from saved disparities (``--ext_disp_to_eval``: scoring, export, encoding and
    writing; the network does not run).  ``Trainer``: ``Trainer.step`` counts per second over one epoch of 250 optimiser steps (500 micro-batches of 6 resident
    synthetic scene batches, the workload of bench.py) with ``log_images`` at the default ``--log_frequency 250``: two log events of
    one 768x4480 sheet each."""
    from PIL import Image
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]      # the synthetic trees the tests use
    import detection_tree
    from fusiondepth_amd import detection as D
    from fusiondepth_amd import export_detection as X
    from fusiondepth_amd import log_images as L
    from fusiondepth_amd import synthetic
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.trainer import Trainer
    import contextlib
    import io
    lines, reps = [], max(2, min(a.reps, 3))
    quiet = contextlib.redirect_stdout(io.StringIO())
    with tempfile.TemporaryDirectory() as tmp, quiet:
        # ---- export_detection
        raw_root, obj_root, splits = (os.path.join(tmp, d) for d in ("raw", "object", "splits"))
        _, obj_lines, _ = detection_tree.make_trees(raw_root, obj_root, frames_per_date=16)
        os.makedirs(os.path.join(splits, "detection"))
        with open(os.path.join(splits, "detection", "test.txt"), "w") as f:
            f.write("\n".join(obj_lines) + "\n")
        D.export_gt_depths_detec(obj_root, obj_lines, "detec", os.path.join(splits, "detection", D.detec_output_name("detec")))
        rng = np.random.RandomState(5)
        n = len(obj_lines)
        base = torch.from_numpy(rng.uniform(0.02, 0.6, (n, 24, 80)).astype(np.float32))
        disp = torch.nn.functional.interpolate(base[:, None], size=(192, 640), mode="bicubic", align_corners=False)[:, 0]
        disp = (disp + torch.from_numpy(rng.uniform(-0.004, 0.004, (n, 192, 640)).astype(np.float32))).clamp_(0.01, 1.0)
        saved = os.path.join(tmp, "disps.npy")
        np.save(saved, disp.numpy())
        flags = ["--splits_dir", splits, "--eval_mono", "--ext_disp_to_eval", saved, "--data_path", obj_root]

        def export_pil():
            return X.main(flags + ["--det_name", "bench_pil"])

        def export_dev():
            return X.main(flags + ["--det_name", "bench_dev", "--png_encoder", "device"])

        rp, rd = export_pil(), export_dev()
        assert np.array_equal(rp[0], rd[0]) and np.array_equal(rp[1], rd[1])
        sizes = [0, 0]
        for p, d in zip(rp[3], rd[3]):
            assert np.array_equal(np.asarray(Image.open(p)), np.asarray(Image.open(d))), "the two encoders' maps differ: %s" % p
            sizes[0] += os.path.getsize(p)
            sizes[1] += os.path.getsize(d)
        runs = [alternate([export_pil, export_dev], reps, _wall_ms) for _ in (1, 2)]
        for k, (tp, td) in enumerate(runs):
            lines.append("  export_detection, %d maps (ext_disp_to_eval; scoring + export + encoding + writing), run %d: pil %.1f ms (%.1f, %.1f); "
                         "device %.1f ms (%.1f, %.1f) -> %.2fx; file bytes pil %d, device %d"
                         % (n, k + 1, tp[0], tp[1], tp[2], td[0], td[1], td[2], tp[0] / td[0], sizes[0], sizes[1]))
        lines.append(_verdict("export_detection", "ms", runs, False))

        # ---- Trainer steps per second with log_images
        opt = MonodepthOptions().parse(["--num_layers", "18", "--weights_init", "scratch", "--batch_size", "12", "--height", "192", "--width",
                                        "640", "--log_dir", os.path.join(tmp, "logs"), "--save_frequency", "1000"])
        torch.manual_seed(5)
        tr = Trainer(opt, verbose=False)
        tr.opt.num_epochs = 1
        tr.log_images = True
        pool_ = []
        for i in range(8):
            mb = synthetic.make_scene_batch(tr.batch_size, 192, 640, seed=1234 + i, clutter=0.5)
            mb.pop("depth_gt", None)
            for f in (-1, 1):
                mb.pop(("T_gt", f), None)
            pool_.append(mb)
        loader = [pool_[i % 8] for i in range(250 * tr.accumulate_step)]
        steps = [0]

        def epoch(encoder):
            def run():
                tr.png_encoder = encoder
                tr.train(loader)                                 # one epoch; returns after the sink's thread has written everything
                steps[0] = tr.step
            return run

        epoch("pil")()                                           # warm-up, and the decode-and-compare on its last batch
        caught = []
        sink, tr.image_sink = tr.image_sink, (lambda mode, step, sheets, tiles: caught.append(sheets))
        tr.log_pictures("train", *tr._last_io)
        tr.image_sink, tr.png_encoder = sink, "device"
        tr.log_pictures("train", *tr._last_io)
        tr.close()
        written = np.asarray(Image.open(L.PngSink.path(tr.log_path, "train", tr.step, 0)))
        assert np.array_equal(written, caught[0][0]), "the device-encoded sheet does not decode to the rendered one"
        runs = [alternate([epoch("pil"), epoch("device")], reps, _wall_ms) for _ in (1, 2)]
        rate = lambda ms: 1e3 * steps[0] / ms                    # noqa: E731
        rates = []
        for k, (tp, td) in enumerate(runs):
            rp_, rd_ = (rate(tp[0]), rate(tp[2]), rate(tp[1])), (rate(td[0]), rate(td[2]), rate(td[1]))
            rates.append((rp_, rd_))
            lines.append("  Trainer, %d micro-batch steps of 6 images (Trainer.step; 250 optimiser steps of 12) with log_images at --log_frequency 250 (2 events, one %dx%d sheet each), run %d: "
                         "pil %.2f steps/s (%.2f, %.2f); device %.2f steps/s (%.2f, %.2f) -> %.3fx"
                         % (steps[0], written.shape[0], written.shape[1], k + 1, rp_[0], rp_[1], rp_[2], rd_[0], rd_[1], rd_[2], rd_[0] / rp_[0]))
        lines.append(_verdict("train --log_images", "steps/s", rates, True))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step", choices=("eigen", "detection", "val", "completion_val", "semantic", "visualize", "log_images", "pseudo_lidar",
                                       "png_encode"),
                    default="eigen")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", {"eigen": "eigen_eval_time.log", "detection": "detection_export_time.log",
                                                "val": "val_time.log", "completion_val": "completion_val_time.log",
                                                "semantic": "eigen_class_time.log", "visualize": "visualize_time.log",
                                                "log_images": "log_images_time.log", "pseudo_lidar": "pseudo_lidar_time.log",
                                                "png_encode": "png_encode_time.log"}[a.step])
    if a.step in ("detection", "val", "completion_val", "semantic", "visualize", "log_images", "pseudo_lidar", "png_encode"):
        text = "\n".join({"detection": detection_step, "val": val_step, "completion_val": completion_val_step,
                          "semantic": semantic_step, "visualize": visualize_step, "log_images": log_images_step,
                          "pseudo_lidar": pseudo_lidar_step, "png_encode": png_encode_step}[a.step](a))
        print(text)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")
        return
    rng = np.random.RandomState(5)
    lines = ["Eigen-split scorer, 192x640 disparities, 375x1242 ground truth with 5 %% valid pixels, eigen split, median scaling; "
             "median of %d (min, max) after one warm-up" % a.reps]
    for n in (1, 64, 697):
        disps, gts = inputs(n, rng)
        reps = a.reps if n <= 64 else 3
        m = min(n, 64)
        run, packed, bound, selected = library_call(disps[:m].contiguous(), gts[:m])
        t_call = events(run, reps)
        t_up = events(lambda: packed.cuda(non_blocking=True), reps)
        t_bound = 1e3 * bound / HBM
        t_all = wall(lambda: ED.eigen_scores(disps, gts), reps)
        t_loop = wall(lambda: ED.evaluate_predictions(disps, gts), 1 if n > 64 else 3)
        lines.append("  N = %3d: fd_eigen_scores, %d images resident (%d selected pixels): %.3f ms (%.3f, %.3f) = %.1f us / image; traffic bound "
                     "%.2f MB = %.2f us at 6.3 TB/s -> %.3f of the bound's rate; upload of the packed ground truth (%.1f MB pinned): %.3f ms"
                     % (n, m, selected, t_call[0], t_call[1], t_call[2], 1e3 * t_call[0] / m, bound / 1e6, 1e3 * t_bound, t_bound / t_call[0],
                        packed.numel() * 4 / 1e6, t_up[0]))
        lines.append("           eigen_scores end to end (host packing, uploads, %d call(s), read-back): %.2f ms = %.3f ms / image; "
                     "evaluate_predictions loop: %.2f ms = %.3f ms / image -> %.2fx"
                     % ((n + 63) // 64, t_all, t_all / n, t_loop, t_loop / n, t_loop / t_all))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
