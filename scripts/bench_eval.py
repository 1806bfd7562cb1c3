"""Timing of the Eigen-split scorer: ``evaluate_depth.eigen_scores`` (fd_eigen_scores, csrc/eigen_eval.hip) at N = 1, 64 and 697 images
against the per-image ATen loop ``evaluate_depth.evaluate_predictions`` on the same inputs, on the same box.  Inputs: 192x640
disparities, synthetic 375x1242 ground truth with 5 % valid pixels (8 distinct maps, cycled), the ``eigen`` split with median scaling.

    python scripts/bench_eval.py [--reps 10] [--out profiles/eigen_eval_time.log]

Per N: the library call alone between device events with everything resident (median, min, max), the upload of the packed ground
truth, the whole ``eigen_scores`` (packing on the host, uploads, calls in chunks of 64, the read-back) and the loop, both as wall time
around a synchronise.  The call's traffic bound: the ground truth inside the windows once, four taps per selected pixel, the compact
(gt, pred) lists written once and read once; at 6.3 TB/s (achievable HBM, as elsewhere in profiles/)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fusiondepth_amd import evaluate_depth as ED          # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eigen_eval_time.log"))
    a = ap.parse_args()
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
