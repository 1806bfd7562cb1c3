#!/usr/bin/env python
"""What the GPU batch builder (fusiondepth_amd.datasets.KITTIRAWBatches) costs and what it replaces.  Real sizes: 1242x375 frames
-> 640x192, four scales, batch 12 (36 frames).  Run on the MI355X box:

    python scripts/bench_loader.py [--out profiles/loader_time.log]

runs, each GPU step as a child process under its own ``timeout -k 10`` and chained so that a failing step ends the run:

  1. ``colour``   device time per batch of the colour path alone (FD.image_pyramid on resident uint8 frames, half the items jittered),
                  device events around synchronised work; bytes moved over time against the compulsory traffic at 6.3 TB/s.
     ``trace``    the same under ``rocprofv3 --kernel-trace --stats`` (a run of its own): kernel names and times.
  2. ``pil``      the reference's recipe (PIL Lanczos pyramid + ToTensor, ColorJitter on half the items) on 16 fresh worker
                  processes that import numpy and PIL only - the number the feature exists to beat.
  3. ``builder``  items/s of KITTIRAWBatches from PNG files, JPEG files and pre-decoded frames (synthetic KITTI tree in a temp dir).
  4. ``trainer``  Trainer images/s fed by the builder (pre-decoded frames) beside the same trainer fed make_scene_batch batches,
                  alternating windows; and the condition: (1) <= 10 % of the synthetic-fed step time.

The worker pool is 16, never ``os.cpu_count()``.  Nothing here is imported by the package; bench.py is untouched.
"""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H0, W0, HEIGHT, WIDTH, SCALES, BATCH, FRAMES = 375, 1242, 192, 640, 4, 12, 3
WORKERS = 16
HBM_BPS = 6.3e12
JITTER = ((1.13, 0.87, 1.1, 0.06), [2, 0, 3, 1])


def frame(seed, h=H0, w=W0):
    rng = np.random.default_rng(seed)
    base = np.repeat(np.repeat(rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3)), 8, axis=0), 8, axis=1)[:h, :w]
    return np.clip(base + rng.integers(-24, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def say(*a):
    print(*a, flush=True)


# ---------------------------------------------------------------------------------------------------- 2. the PIL recipe
def pil_item(frames, jitter):
    """mono_dataset.py:85-104 for one item: chained Lanczos pyramid of every frame, ToTensor of every image, ColorJitter (one draw per
    item) + ToTensor again for a jittered item."""
    from PIL import Image, ImageEnhance

    def to_tensor(img):
        return np.ascontiguousarray((np.asarray(img).astype(np.float32) / np.float32(255)).transpose(2, 0, 1))

    def hue(img, h):
        hh, ss, vv = img.convert("HSV").split()
        arr = (np.asarray(hh).astype(np.int32) + int(np.trunc(h * 255.0)) % 256).astype(np.uint8)
        return Image.merge("HSV", (Image.fromarray(arr, "L"), ss, vv)).convert("RGB")

    def aug(img):
        fac, order = JITTER
        for op in order:
            img = (ImageEnhance.Brightness(img).enhance(fac[0]) if op == 0 else ImageEnhance.Contrast(img).enhance(fac[1]) if op == 1
                   else ImageEnhance.Color(img).enhance(fac[2]) if op == 2 else hue(img, fac[3]))
        return img

    n = 0
    for arr in frames:
        cur = Image.fromarray(arr)
        for s in range(SCALES):
            cur = cur.resize((WIDTH >> s, HEIGHT >> s), Image.LANCZOS)
            n += to_tensor(cur).size
            n += to_tensor(aug(cur) if jitter else cur).size
    return n


def step_pil_worker(args):
    frames = [frame(100 + i) for i in range(FRAMES)]
    pil_item(frames, True)                                          # warm-up
    t = time.perf_counter()
    for i in range(args.items):
        pil_item(frames, bool(i % 2))
    say(json.dumps({"items": args.items, "seconds": time.perf_counter() - t}))


def step_pil(args):
    per = args.items
    t = time.perf_counter()
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--step", "pil_worker", "--items", str(per)], stdout=subprocess.PIPE,
                              text=True) for _ in range(WORKERS)]
    outs = [json.loads(p.communicate()[0].strip().splitlines()[-1]) for p in procs]
    wall = time.perf_counter() - t
    if any(p.returncode for p in procs):
        sys.exit("a PIL worker failed")
    busy = max(o["seconds"] for o in outs)
    say("[2] PIL recipe, %d worker processes x %d items (half jittered): %.1f items/s over the workers' timed loops (slowest %.2f s; "
        "%.1f items/s incl. process start, wall %.2f s); one worker alone: %.1f ms / item"
        % (WORKERS, per, WORKERS * per / busy, busy, WORKERS * per / wall, wall, 1e3 * np.mean([o["seconds"] for o in outs]) / per))


# ---------------------------------------------------------------------------------------------------- 1. colour path on the device
def colour_traffic(n_frames):
    """(compulsory bytes, bytes the passes actually move) per batch.  Passes: per scale a horizontal (read source, write the uint8
    intermediate) and a vertical resample (read it, write the level); the contrast statistics read the jittered levels; the apply pass
    reads every level once and writes each float32 plane of ``color`` and ``color_aug`` once."""
    sizes = [(HEIGHT >> s, WIDTH >> s) for s in range(SCALES)]
    lv = [h * w * 3 for h, w in sizes]
    compulsory = n_frames * (H0 * W0 * 3 + 2 * 4 * sum(lv))
    moved, hin, win = 0, H0, W0
    for (h, w), b in zip(sizes, lv):
        moved += hin * win * 3 + 2 * hin * w * 3 + b
        hin, win = h, w
    moved += sum(lv) * 0.5 + sum(lv) + 2 * 4 * sum(lv)
    return compulsory, n_frames * moved


def step_colour(args):
    import torch
    sys.path.insert(0, ROOT)
    from fusiondepth_amd import functional as FD
    n = BATCH * FRAMES
    frames = torch.from_numpy(np.stack([frame(i % 6) for i in range(n)])).cuda()
    flip = [bool((i // 2) % 2) for i in range(n)]
    jitter = [JITTER if i % 2 else None for i in range(n)]
    for _ in range(3):
        FD.image_pyramid(frames, HEIGHT, WIDTH, SCALES, flip, jitter)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        FD.image_pyramid(frames, HEIGHT, WIDTH, SCALES, flip, jitter)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    ms = float(np.median(times))
    comp, moved = colour_traffic(n)
    say("[1] colour path, batch %d (%d frames %dx%d -> %dx%d, %d scales, half jittered): %.3f ms / batch (median of %d, min %.3f, max %.3f; "
        "device events, includes the two small table uploads)" % (BATCH, n, W0, H0, WIDTH, HEIGHT, SCALES, ms, len(times), min(times), max(times)))
    say("    10 launches; compulsory traffic %.1f MB = %.1f us at 6.3 TB/s; the passes move %.1f MB -> %.2f TB/s achieved; %.1fx the bound"
        % (comp / 1e6, 1e6 * comp / HBM_BPS, moved / 1e6, moved / (ms * 1e-3) / 1e12, ms * 1e-3 / (comp / HBM_BPS)))
    say(json.dumps({"colour_ms_per_batch": ms}))


def step_trace_report(args):
    """Per-kernel times from the rocprofv3 results database of the traced colour run (the query of scripts/rocprof_summary.py)."""
    import sqlite3
    files = sorted(glob.glob(os.path.join(args.trace_dir, "**", "*_results.db"), recursive=True))
    if not files:
        sys.exit("no rocprofv3 results database under %s" % args.trace_dir)
    db = sqlite3.connect(files[-1])
    rows = list(db.execute("select name, count(*), sum(end-start)/1e3, avg(end-start)/1e3 from kernels group by name order by 3 desc"))
    batches = args.iters + 3
    ours = [r for r in rows if any(k in r[0] for k in ("k_lanczos", "k_jitter", "k_u8_to_planes"))]
    say("    rocprofv3 --kernel-trace --stats, %d batches (3 warm-up + %d): the library's kernels take %.1f us / batch of %.1f us of device "
        "kernel time / batch" % (batches, args.iters, sum(r[2] for r in ours) / batches, sum(r[2] for r in rows) / batches))
    say("      %-50s %8s %12s %10s" % ("kernel", "calls", "us / batch", "avg us"))
    for r in rows[:12]:
        name = r[0].replace("(anonymous namespace)::", "").split("(")[0]
        say("      %-50s %8d %12.1f %10.2f" % (name[-50:], r[1], r[2] / batches, r[3]))


# ---------------------------------------------------------------------------------------------------- 3 / 4. a synthetic KITTI tree
def write_tree(root, n_frames, exts):
    from PIL import Image
    date, drive = "2011_09_26", "2011_09_26_drive_0001_sync"
    fmt = lambda a: " ".join("%.17g" % v for v in np.asarray(a, dtype=np.float64).reshape(-1))
    K = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
    Rv = np.array([[7.533745e-03, -9.999714e-01, -6.166020e-04], [1.480249e-02, 7.280733e-04, -9.998902e-01], [9.998621e-01, 7.523790e-03, 1.480755e-02]])
    os.makedirs(os.path.join(root, date), exist_ok=True)
    with open(os.path.join(root, date, "calib_cam_to_cam.txt"), "w") as f:
        f.write("S_rect_02: %s\nR_rect_00: %s\nP_rect_02: %s\n" % (fmt([W0, H0]), fmt(np.eye(3)), fmt(K)))
    with open(os.path.join(root, date, "calib_velo_to_cam.txt"), "w") as f:
        f.write("R: %s\nT: %s\n" % (fmt(Rv), fmt([-4.069766e-03, -7.631618e-02, -2.717806e-01])))
    folder = os.path.join(root, date, drive)
    for sub in ("image_02/data", "4beam"):
        os.makedirs(os.path.join(folder, sub), exist_ok=True)
    rng = np.random.default_rng(5)
    sizes = {e: 0 for e in exts}
    for i in range(n_frames):
        img = Image.fromarray(frame(1000 + i))
        for e in exts:
            p = os.path.join(folder, "image_02/data/%010d%s" % (i, e))
            img.save(p, quality=92) if e == ".jpg" else img.save(p)
            sizes[e] += os.path.getsize(p)
        fwd = np.where(rng.random(1500) < 0.5, rng.uniform(4.0, 7.0, 1500), rng.uniform(2.0, 70.0, 1500))
        pts = np.stack([fwd, rng.uniform(-0.45, 0.45, 1500) * fwd, rng.uniform(-0.2, 0.12, 1500) * fwd, rng.random(1500)], 1).astype(np.float32)
        pts.tofile(os.path.join(folder, "4beam/%010d.bin" % i))
    lines = ["%s/%s %d l" % (date, drive, i) for i in range(1, n_frames - 1)]
    return lines, {e: s / n_frames for e, s in sizes.items()}


def _opt(batch):
    from fusiondepth_amd.options import MonodepthOptions
    return MonodepthOptions().parse(["--num_layers", "18", "--weights_init", "scratch", "--batch_size", str(batch), "--height", str(HEIGHT),
                                     "--width", str(WIDTH)])


def _cached_loader():
    from fusiondepth_amd.datasets import pil_loader
    cache = {}

    def load(path):
        if path not in cache:
            cache[path] = pil_loader(path)
        return cache[path]
    return load


def step_builder(args):
    import concurrent.futures
    import torch
    sys.path.insert(0, ROOT)
    from fusiondepth_amd.datasets import KITTIRAWBatches, pil_loader
    with tempfile.TemporaryDirectory() as root:
        lines, mean_size = write_tree(root, 50, (".png", ".jpg"))
        opt = _opt(BATCH)
        say("[3] KITTIRAWBatches, batch %d, %d items per epoch, %d decode threads, 4beam + 2channel keys included; files: PNG %.0f KB, JPEG %.0f KB "
            "each (noise-textured frames: larger than KITTI's)" % (BATCH, len(lines), WORKERS, mean_size[".png"] / 1e3, mean_size[".jpg"] / 1e3))

        def run(ext, loader=None, epochs=3):
            b = KITTIRAWBatches(root, lines, HEIGHT, WIDTH, [0, -1, 1], SCALES, is_train=True, img_ext=ext, opt=opt, batch_size=BATCH, shuffle=True,
                                seed=1, workers=WORKERS, loader=loader)
            for _ in b:                                                # warm-up epoch (fills the cache of the pre-decoded run)
                pass
            torch.cuda.synchronize()
            t = time.perf_counter()
            n = 0
            for _ in range(epochs):
                for batch in b:
                    n += batch[("color", 0, 0)].shape[0]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            b.close()
            return n / dt

        for ext, name in ((".png", "PNG files"), (".jpg", "JPEG files")):
            paths = sorted(glob.glob(os.path.join(root, "*", "*", "image_02", "data", "*" + ext)))
            with concurrent.futures.ThreadPoolExecutor(WORKERS) as pool:
                t = time.perf_counter()
                list(pool.map(pil_loader, paths * 2))
                dec = 2 * len(paths) / (time.perf_counter() - t)
            rate = run(ext)
            say("    from %-11s %7.1f items/s  (decode alone on the same %d threads: %.0f frames/s = %.1f items/s of 3 frames)"
                % (name + ":", rate, WORKERS, dec, dec / 3))
        say("    pre-decoded:     %7.1f items/s  (uint8 frames from host memory: upload + kernels + LiDAR files)" % run(".png", _cached_loader()))


def step_trainer(args):
    import torch
    sys.path.insert(0, ROOT)
    from fusiondepth_amd import synthetic
    from fusiondepth_amd.datasets import KITTIRAWBatches
    from fusiondepth_amd.trainer import Trainer
    torch.manual_seed(1)
    with tempfile.TemporaryDirectory() as root:
        lines, _ = write_tree(root, 50, (".png",))
        opt = _opt(BATCH)
        tr = Trainer(opt, verbose=False)
        per_step = tr.batch_size * tr.accumulate_step
        b = KITTIRAWBatches(root, lines, HEIGHT, WIDTH, [0, -1, 1], SCALES, is_train=True, img_ext=".png", opt=opt, batch_size=tr.batch_size,
                            shuffle=True, seed=1, workers=WORKERS, loader=_cached_loader())

        def endless():
            while True:
                for batch in b:
                    yield batch
        real = endless()
        pool = []
        for i in range(8):
            mbs = [synthetic.make_scene_batch(tr.batch_size, HEIGHT, WIDTH, seed=1234 + 17 * i + j, clutter=0.5) for j in range(tr.accumulate_step)]
            for mb in mbs:
                mb.pop("depth_gt", None)
                for f in (-1, 1):
                    mb.pop(("T_gt", f), None)
            pool.append(mbs)
        k = [0]

        def step_real():
            tr.train_step([next(real) for _ in range(tr.accumulate_step)])

        def step_syn():
            k[0] += 1
            tr.train_step(pool[k[0] % len(pool)])

        def window(fn, n):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / n

        for _ in range(4):
            step_syn()
            step_real()
        res = {"builder": [], "synthetic": []}
        for _ in range(args.windows):
            res["synthetic"].append(window(step_syn, args.steps))
            res["builder"].append(window(step_real, args.steps))
        b.close()
        syn, rl = float(np.median(res["synthetic"])), float(np.median(res["builder"]))
        say("[4] Trainer (ResNet-18, %dx%d, --batch_size %d = %d images / step), %d alternating windows of %d steps:" % (WIDTH, HEIGHT, BATCH, per_step,
                                                                                                                        args.windows, args.steps))
        say("    fed make_scene_batch batches:            %.1f images/s (%.2f ms / step; windows %s)"
            % (per_step / syn, 1e3 * syn, " ".join("%.2f" % (1e3 * v) for v in res["synthetic"])))
        say("    fed by KITTIRAWBatches (pre-decoded):    %.1f images/s (%.2f ms / step; windows %s)"
            % (per_step / rl, 1e3 * rl, " ".join("%.2f" % (1e3 * v) for v in res["builder"])))
        if args.colour_ms > 0:
            share = args.colour_ms * (per_step / BATCH) / (1e3 * syn)
            say("    condition: colour path %.3f ms per %d items = %.1f %% of the synthetic-fed step time (%.2f ms): %s the 10 %% limit"
                % (args.colour_ms * per_step / BATCH, per_step, 100 * share, 1e3 * syn, "within" if share <= 0.10 else "ABOVE"))


def drive(args):
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    scratch = tempfile.mkdtemp(prefix="bench_loader_")          # the profiler's database and the hand-over of step 1's figure
    trace_dir = os.path.join(scratch, "trace")
    me = "%s %s" % (sys.executable, os.path.abspath(__file__))
    colour_json = os.path.join(scratch, "colour.json")
    steps = [
        "timeout -k 10 240 %s --step colour --iters 30 | tee %s.tmp" % (me, colour_json),
        "timeout -k 10 300 rocprofv3 --kernel-trace --stats -d %s -- %s --step colour --iters 10 > /dev/null 2>&1" % (trace_dir, me),
        "%s --step trace_report --iters 10 --trace_dir %s" % (me, trace_dir),
        "timeout -k 10 300 %s --step pil --items 12" % me,
        "timeout -k 10 420 %s --step builder" % me,
        "timeout -k 10 540 %s --step trainer --colour_ms $(tail -1 %s.tmp | python -c 'import json,sys; print(json.load(sys.stdin)[\"colour_ms_per_batch\"])')"
        % (me, colour_json),
    ]
    cmd = "set -o pipefail; (" + " && ".join(steps) + ") 2>&1 | grep --line-buffered -v '^{' | tee %s" % out
    sys.exit(subprocess.call(["bash", "-c", cmd], cwd=ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="all", choices=["all", "colour", "trace_report", "pil", "pil_worker", "builder", "trainer"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loader_time.log"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--items", type=int, default=12)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--colour_ms", type=float, default=0.0)
    ap.add_argument("--trace_dir", default="")
    args = ap.parse_args()
    {"all": drive, "colour": step_colour, "trace_report": step_trace_report, "pil": step_pil, "pil_worker": step_pil_worker,
     "builder": step_builder, "trainer": step_trainer}[args.step](args)


if __name__ == "__main__":
    main()
