"""GDC timing at 375x1242 on the synthetic KITTI-calibrated scene of tests/test_gpu_gdc.py, both pitch-range rules:
GPU time per stage (hipEvents: masks = fd_gdc_prepare, build = k-NN + weights + transpose + CG set-up, CG per iteration, finish),
the float64 numpy / scipy restatement's wall time on the same frame, and the inf_gdc driver's frames/s on a temporary tree.
The split of the build stage into its kernels comes from a kernel trace of this script (rocprofv3 --kernel-trace --stats).

    python scripts/time_gdc.py [--reps 5] [--frames 16]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import test_gpu_gdc as T                      # noqa: E402  (the scene and the float64 restatement)
from fusiondepth_amd import gdc as G          # noqa: E402


def gpu_stages(pred, gt, rng, reps):
    cam = T.camera()
    p, g = T.dev(pred), T.dev(gt)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    rows = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        ev[0].record()
        pix, N_PL, N_L = G.prepare(p, g, cam, rng)       # includes the one host read of the counts
        ev[1].record()
        ws = G.build(p, g, cam, pix, N_PL, N_L, 10, 5e-4)
        ev[2].record()
        st = G.solve(ws, N_PL, N_L, 10, 10 * N_PL)
        ev[3].record()
        out = torch.empty_like(p)
        from fusiondepth_amd._lib import call, stream
        call("fd_gdc_finish", p.data_ptr(), g.data_ptr(), pix.data_ptr(), N_PL, N_L, 10, p.shape[0], p.shape[1], ws.data_ptr(),
             out.data_ptr(), stream())
        ev[4].record()
        torch.cuda.synchronize()
        rows.append([ev[i].elapsed_time(ev[i + 1]) for i in range(4)] + [st.iterations])
    r = np.median(np.array(rows[1:]), 0)
    return N_PL, N_L, r


def restatement_time(pred, gt, rng):
    t0 = time.perf_counter()
    ref = T.ref_gdc(pred, gt, T.camera(), rng=rng)
    return time.perf_counter() - t0, ref["its"]


def driver_fps(frames):
    from fusiondepth_amd import inf_gdc
    import inputs as gin
    velo, _ = gin.lidar_scan(11, n_points=60000)
    cal = gin.lidar_scan.calib
    fmt = lambda a: " ".join(repr(float(v)) for v in np.asarray(a).reshape(-1))
    with tempfile.TemporaryDirectory() as tmp:
        date, drive = "2011_09_26", "2011_09_26_drive_0001_sync"
        ddir = os.path.join(tmp, date)
        os.makedirs(os.path.join(ddir, drive, "4beam"))
        os.makedirs(os.path.join(ddir, drive, "inf_depth_4beam"))
        P3 = cal["P_rect_02"].copy()
        P3[0, 3] = -339.5242
        with open(os.path.join(ddir, "calib_cam_to_cam.txt"), "w") as fh:
            fh.write("S_rect_02: %s\nR_rect_00: %s\nP_rect_02: %s\nP_rect_03: %s\n"
                     % (fmt(cal["S_rect_02"]), fmt(cal["R_rect_00"]), fmt(cal["P_rect_02"]), fmt(P3)))
        with open(os.path.join(ddir, "calib_velo_to_cam.txt"), "w") as fh:
            fh.write("R: %s\nT: %s\n" % (fmt(cal["R"]), fmt(cal["T"])))
        yy, xx = np.meshgrid(np.arange(192), np.arange(640), indexing="ij")
        lines = []
        for f in range(frames):
            velo.tofile(os.path.join(ddir, drive, "4beam", "%010d.bin" % f))
            disp = 0.03 + 0.02 * np.sin(xx / 70.0 + f) * np.cos(yy / 40.0) + 0.0005 * np.random.RandomState(f).randn(192, 640)
            np.save(os.path.join(ddir, drive, "inf_depth_4beam", "%d_l.npy" % f), disp.astype(np.float32)[None, None])
            lines.append("%s/%s %d l" % (date, drive, f))
        split = os.path.join(tmp, "split.txt")
        with open(split, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        inf_gdc.main(["--data_path", tmp, "--split_files", split])          # warm-up (library load, first launches)
        t0 = time.perf_counter()
        failed = inf_gdc.main(["--data_path", tmp, "--split_files", split])
        dt = time.perf_counter() - t0
    return frames / dt, failed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--no-restatement", action="store_true")
    a = ap.parse_args()
    torch.set_num_threads(16)
    truth, pred, gt = T.scene(375, 1242, seed=375)
    print("GDC at 375x1242, k = 10, W_tol = 3e-5, recon_tol = 5e-4 (median of %d runs after one warm-up)" % a.reps)
    for name, rng in (("beams (-0.1, 4.0)", T.BEAMS), ("random sample (-1.5, 9)", T.RANDOM)):
        N_PL, N_L, (t_prep, t_build, t_cg, t_fin, its) = gpu_stages(pred, gt, rng, a.reps)
        total = t_prep + t_build + t_cg + t_fin
        print("  %-24s N_PL %6d  N_L %5d | masks %.3f ms  build %.3f ms  CG %.3f ms (%d iterations, %.1f us / iteration incl. "
              "state reads)  finish %.3f ms | total %.2f ms"
              % (name, N_PL, N_L, t_prep, t_build, t_cg, its, 1e3 * t_cg / max(its, 1), t_fin, total))
        if not a.no_restatement:
            wall, rits = restatement_time(pred, gt, rng)
            print("  %-24s float64 numpy / scipy restatement (16 threads): %.2f s (%d CG iterations)" % ("", wall, rits))
    fps, failed = driver_fps(a.frames)
    print("inf_gdc driver: %.2f frames/s over %d frames (%d failed)" % (fps, a.frames, failed))


if __name__ == "__main__":
    main()
