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

``--step raw [--out profiles/sparsify_time.log]`` measures the raw-scan LiDAR path (``lidar_source="raw"``, fd_sparsify_scans +
fd_velo_rasterize_batch) the same way, as a run of its own:

  5. ``sparsify``     device time per batch (36 scans of about 128 k points) of the new kernels against their compulsory traffic at
                      8 TB/s, and the upload time of the batch's pinned staging buffer.
  6. ``raw_builder``  items/s of KITTIRAWBatches in raw mode beside file mode (pre-decoded frames, the same tree, alternating).
  7. ``raw_trainer``  Trainer images/s fed by raw mode, by file mode and by make_scene_batch batches, alternating windows.
  8. ``offline``      scans/s of ``python -m fusiondepth_amd.sparsify`` beside the numpy restatement (tests/sparsify_ref.py) on 16
                      worker processes.

``--step refiner`` measures the Refiner's loader (``KITTIRefinerBatches``, fd_resize_bilinear_batch) and appends to ``--out``:

  9. ``inf_gdc_key``      the ``inf_gdc`` key at batch 6, 375x1242 -> 192x640: upload of the pinned staging buffer and the library call, each
                          on its own (device events), then the kernel's own time under ``rocprofv3 --kernel-trace --stats`` (a run of its
                          own) against its compulsory traffic (maps read once, key written once) at 8 TB/s.
 10. ``refiner_trainer``  Refiner images/s fed by KITTIRefinerBatches (pre-decoded frames, maps from .npy files) beside the same Refiner
                          fed synthetic batches, alternating windows; and the condition: colour path (step 1 at batch 6) + the key <=
                          10 % of the synthetic-fed Refiner step (file mode's LiDAR keys are not in that sum, as in step 4).

``--step completion [--out profiles/completion_time.log]`` measures the depth-completion loader and scorer (``KITTICompletionBatches``,
``evaluate_completion``):

 11. ``completion_keys``  batch 4 x 3 frames of 375x1242 sources in full-res mode: upload of the pinned staging buffer, each
                          ``fd_depth_png_keys`` call (beam planes, depth_gt, full_res_4beam) against its compulsory traffic (uint16 read once,
                          float32 written once) at 6.3 TB/s (achievable HBM), the colour path at 352x1216, and the two scoring kernels at N = 8 and N = 1 beside the
                          ``torch.sort``-based median recipe of evaluate_depth.py on the same tensors (device events); then the kernels' own
                          times under ``rocprofv3 --kernel-trace --stats`` (a run of its own).

 12. ``jpeg``             ``--step jpeg`` (a run of its own, ``| tee profiles/jpeg_decode_time.log``): 36 JPEG frames of 1242x375 (4:2:2, quality
                          92) through ``image_codecs.decode_jpeg_batch`` and through pil_loader on 16 threads + np.stack + upload, alternating; the
                          host Huffman phase, the upload and the two kernels against their traffic bound; the entropy decoder against
                          Pillow's whole decode on one thread; ``KITTIRAWBatches`` items/s and Trainer images/s fed by either ``decoder=``.
                          The kernels' own times: ``rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_loader.py --step
                          jpeg_kernels``, then ``--step jpeg_trace_report --trace_dir DIR``.

 13. ``png``              ``--step png`` (a run of its own, ``| tee profiles/png_decode_time.log``): step 12's workload as PNG files written by
                          Pillow with its default settings, through ``image_codecs.decode_png_batch`` and through pil_loader on 16 threads +
                          np.stack + upload, alternating; the host inflate phase, the upload and the two kernels against their traffic bound
                          and as a share of the batch; ``fd_png_inflate`` against ``zlib.decompress`` and Pillow's whole decode on one
                          thread; the completion loader's 16 depth planes by either route; ``KITTIRAWBatches`` items/s and Trainer
                          images/s fed by either ``png_decoder=``.
 14. ``jpeg_enc``         ``--step jpeg_enc`` (a run of its own, ``| tee -a profiles/jpeg_encode_time.log``): 36 frames of step 12's content
                          through ``image_codecs.encode_jpeg_batch`` against Pillow's ``save`` on 16 threads, ``fd_jpeg_enc_encode`` alone against
                          its traffic bound, and ``convert_frames`` end to end against ``--encoder pil --png_decoder pil``.

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
    n = args.items * FRAMES
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
        "device events, includes the two small table uploads)" % (args.items, n, W0, H0, WIDTH, HEIGHT, SCALES, ms, len(times), min(times), max(times)))
    say("    10 launches; compulsory traffic %.1f MB = %.1f us at 6.3 TB/s; the passes move %.1f MB -> %.2f TB/s achieved; %.1fx the bound"
        % (comp / 1e6, 1e6 * comp / HBM_BPS, moved / 1e6, moved / (ms * 1e-3) / 1e12, ms * 1e-3 / (comp / HBM_BPS)))
    say(json.dumps({"colour_ms_per_batch": ms, "batch": args.items}))


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


# ---------------------------------------------------------------------------------------------------- 12. JPEG frames on the device
def write_jpeg_tree(root, n_frames):
    """write_tree's layout with 4:2:2 JPEG frames at quality 92 (KITTI's own sampling) -> (split lines, frame paths, mean file bytes)."""
    from PIL import Image
    lines, _ = write_tree(root, n_frames, ())
    folder = os.path.join(root, "2011_09_26", "2011_09_26_drive_0001_sync", "image_02/data")
    paths = []
    for i in range(n_frames):
        paths.append(os.path.join(folder, "%010d.jpg" % i))
        Image.fromarray(frame(1000 + i)).save(paths[-1], quality=92, subsampling=1)
    return lines, paths, sum(os.path.getsize(p) for p in paths) / n_frames


def _spread(v):
    return "median %.2f, %.2f .. %.2f" % (float(np.median(v)), min(v), max(v))


def step_jpeg(args):
    """[12] ``image_codecs.decode_jpeg_batch`` against the parent route (pil_loader on 16 threads + np.stack + upload), its phases, the
    builder and the trainer fed by either route.  The routes alternate inside this one run."""
    import concurrent.futures
    import ctypes
    import torch
    sys.path.insert(0, ROOT)
    from fusiondepth_amd import _lib, image_codecs
    from fusiondepth_amd.datasets import KITTIRAWBatches, pil_loader
    N = 36
    with tempfile.TemporaryDirectory() as root:
        lines, paths, mean_size = write_jpeg_tree(root, N + 14)
        batch_paths = paths[:N]
        say("[12] JPEG frames: %d frames of %dx%d, 4:2:2, quality 92, written by Pillow from textured synthetic content; %.0f KB per file "
            "(entropy-decode time follows the file size; not a KITTI frame)" % (N, W0, H0, mean_size / 1e3))
        pool = concurrent.futures.ThreadPoolExecutor(WORKERS)

        def route_device():
            frames, stats = image_codecs.decode_jpeg_batch(batch_paths, pool=pool)
            torch.cuda.synchronize()
            assert stats["fallback"] == 0, stats
            return frames

        def route_pil():
            stack = torch.from_numpy(np.stack(list(pool.map(pil_loader, batch_paths)))).to("cuda", non_blocking=True)
            torch.cuda.synchronize()
            return stack

        got, want = route_device(), route_pil()
        assert all(torch.equal(g, w) for g, w in zip(got, want)), "the routes disagree"
        t = {"device": [], "pil": []}
        for _ in range(args.iters):
            for name, fn in (("device", route_device), ("pil", route_pil)):
                t0 = time.perf_counter()
                fn()
                t[name].append(1e3 * (time.perf_counter() - t0))
        for name, label in (("device", "decode_jpeg_batch (host Huffman on %d threads + one upload + fd_jpeg_reconstruct)" % WORKERS),
                            ("pil", "pil_loader on %d threads + np.stack + upload (the parent's route)" % WORKERS)):
            med = float(np.median(t[name]))
            say("    %-88s %7.1f frames/s, ms per batch of %d: %s  (%d alternating runs)" % (label + ":", 1e3 * N / med, N, _spread(t[name]), args.iters))

        # one thread, per frame: the entropy decoder alone against Pillow's whole decode
        datas = [open(p, "rb").read() for p in batch_paths]
        info = image_codecs.jpeg_probe(datas[0])[1]
        coef, qt = np.empty(info.coef_count, np.int16), np.empty(192, np.uint16)
        one = {"entropy": [], "pillow": []}
        for _ in range(3):
            t0 = time.perf_counter()
            for d in datas:
                assert image_codecs.jpeg_entropy_decode(d, coef, qt)[0] == 0
            one["entropy"].append(1e3 * (time.perf_counter() - t0) / N)
            t0 = time.perf_counter()
            for p in batch_paths:
                pil_loader(p)
            one["pillow"].append(1e3 * (time.perf_counter() - t0) / N)
        e1, p1 = min(one["entropy"]), min(one["pillow"])
        say("    one thread, per frame: fd_jpeg_entropy_decode %.2f ms, Pillow's whole decode %.2f ms -> the hand-written entropy decoder is %s "
            "than Pillow's whole decode (%.2fx)" % (e1, p1, "SLOWER" if e1 > p1 else "faster", p1 / e1))

        # inside the batch
        host_ms, up_ms, k_ms = [], [], []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            job = image_codecs.JpegBatchJob(batch_paths, pool)
            lay = job.wait_host()
            host_ms.append(1e3 * (time.perf_counter() - t0))
            job.finish("cuda")                                   # writes the descriptor table into the staging buffer
            torch.cuda.synchronize()
            total = lay["total_bytes"]
            dev = torch.empty((total,), dtype=torch.uint8, device="cuda")
            out = torch.empty((N * 3 * H0 * W0 + 64,), dtype=torch.uint8, device="cuda")
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            dev[:lay["upload_bytes"]].copy_(lay["staging"], non_blocking=True)
            ev[1].record()
            ev[2].record()
            _lib.call("fd_jpeg_reconstruct", dev.data_ptr(), total, dev.data_ptr(), N, out.data_ptr(), N * 3 * H0 * W0, _lib.stream())
            ev[3].record()
            torch.cuda.synchronize()
            up_ms.append(ev[0].elapsed_time(ev[1]))
            k_ms.append(ev[2].elapsed_time(ev[3]))
        up_bytes, rgb_bytes = lay["upload_bytes"], N * 3 * H0 * W0
        coef_bytes, plane_bytes = 2 * N * info.coef_count, N * info.coef_count
        traffic = coef_bytes + 2 * plane_bytes + rgb_bytes
        bound_ms = 1e3 * traffic / HBM_BPS
        km = float(np.median(k_ms))
        say("    inside the batch: host phase (read + probe + Huffman, %d threads) %s ms" % (WORKERS, _spread(host_ms)))
        say("                      upload %.1f MB (int16 coefficients = %.2fx the RGB bytes) %s ms = %.1f GB/s"
            % (up_bytes / 1e6, coef_bytes / rgb_bytes, _spread(up_ms), up_bytes / 1e6 / float(np.median(up_ms))))
        say("                      the two kernels (device events around fd_jpeg_reconstruct) %s ms; traffic bound %.1f MB (coefficients in, "
            "planes out and in, RGB out) at %.1f TB/s = %.4f ms -> %.1fx the bound" % (_spread(k_ms), traffic / 1e6, HBM_BPS / 1e12, bound_ms, km / bound_ms))

        # the builder from the JPEG tree, both routes, alternating
        opt = _opt(BATCH)

        def run(decoder, epochs=2):
            b = KITTIRAWBatches(root, lines, HEIGHT, WIDTH, [0, -1, 1], SCALES, is_train=True, img_ext=".jpg", opt=opt, batch_size=BATCH, shuffle=True,
                                seed=1, workers=WORKERS, decoder=decoder)
            for _ in b:
                pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for _ in range(epochs):
                for batch in b:
                    n += batch[("color", 0, 0)].shape[0]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            b.close()
            return n / dt

        rates = {"pil": [], "device": []}
        for _ in range(5):
            for name in ("pil", "device"):
                rates[name].append(run(name, epochs=6))
        sp = {k: max(v) - min(v) for k, v in rates.items()}
        mp, md = float(np.median(rates["pil"])), float(np.median(rates["device"]))
        say("    KITTIRAWBatches from the JPEG tree, batch %d, %d items per epoch, 5 alternating runs of 6 epochs each:" % (BATCH, len(lines)))
        say("        decoder='pil':    %7.1f items/s (runs %s; spread %.1f)" % (mp, " ".join("%.1f" % v for v in rates["pil"]), sp["pil"]))
        say("        decoder='device': %7.1f items/s (runs %s; spread %.1f)" % (md, " ".join("%.1f" % v for v in rates["device"]), sp["device"]))
        say("        difference %+.1f items/s against the larger spread %.1f: the device route %s"
            % (md - mp, max(sp.values()), "WINS" if md - mp > max(sp.values()) else ("LOSES" if mp - md > max(sp.values()) else "is within the spread")))
        pool.shutdown()

        if args.windows > 0:
            from fusiondepth_amd.trainer import Trainer
            torch.manual_seed(1)
            tr = Trainer(opt, verbose=False)
            per_step = tr.batch_size * tr.accumulate_step
            feeds = {}
            for name in ("pil", "device"):
                b = KITTIRAWBatches(root, lines, HEIGHT, WIDTH, [0, -1, 1], SCALES, is_train=True, img_ext=".jpg", opt=opt, batch_size=tr.batch_size,
                                    shuffle=True, seed=1, workers=WORKERS, decoder=name)

                def endless(b=b):
                    while True:
                        for batch in b:
                            yield batch
                feeds[name] = (b, endless())
            res = {"pil": [], "device": []}
            for name in feeds:
                for _ in range(3):
                    tr.train_step([next(feeds[name][1]) for _ in range(tr.accumulate_step)])
            for _ in range(args.windows):
                for name in ("pil", "device"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        tr.train_step([next(feeds[name][1]) for _ in range(tr.accumulate_step)])
                    torch.cuda.synchronize()
                    res[name].append((time.perf_counter() - t0) / args.steps)
            for name in feeds:
                feeds[name][0].close()
                m = float(np.median(res[name]))
                say("    Trainer (ResNet-18, %dx%d, %d images / step) fed by decoder='%s': %s %.1f images/s (%.2f ms / step; windows %s)"
                    % (WIDTH, HEIGHT, per_step, name, " " * (6 - len(name)), per_step / m, 1e3 * m, " ".join("%.2f" % (1e3 * v) for v in res[name])))
        say("    not measured: a real KITTI tree; JPEG files written by other encoders")


def step_jpeg_kernels(args):
    """3 + ``--iters`` batches of 36 frames through ``decode_jpeg_batch``, for ``rocprofv3 --kernel-trace --stats -d DIR -- ...``."""
    import torch
    sys.path.insert(0, ROOT)
    from fusiondepth_amd import image_codecs
    with tempfile.TemporaryDirectory() as root:
        _, paths, _ = write_jpeg_tree(root, 36)
        for _ in range(3 + args.iters):
            image_codecs.decode_jpeg_batch(paths)
            torch.cuda.synchronize()


def step_jpeg_trace_report(args):
    """The two kernels' own times from the rocprofv3 results database of a traced ``--step jpeg_kernels`` run."""
    import sqlite3
    files = sorted(glob.glob(os.path.join(args.trace_dir, "**", "*_results.db"), recursive=True))
    if not files:
        sys.exit("no rocprofv3 results database under %s" % args.trace_dir)
    db = sqlite3.connect(files[-1])
    rows = list(db.execute("select name, count(*), sum(end-start)/1e3, avg(end-start)/1e3 from kernels group by name order by 3 desc"))
    say("    rocprofv3 --kernel-trace --stats, %d batches of 36 frames (a run of its own):" % (3 + args.iters))
    for r in rows:
        if "k_jpeg" in r[0]:
            say("      %-30s %6d calls, %8.1f us / batch" % (r[0].replace("(anonymous namespace)::", "").split("(")[0], r[1], r[3]))


# ---------------------------------------------------------------------------------------------------- 13. PNG frames on the device
def write_png_tree(root, n_frames):
    """write_tree's layout with PNG frames written by Pillow with its default settings -> (split lines, frame paths, mean file bytes)."""
    lines, _ = write_tree(root, n_frames, (".png",))
    folder = os.path.join(root, "2011_09_26", "2011_09_26_drive_0001_sync", "image_02/data")
    paths = [os.path.join(folder, "%010d.png" % i) for i in range(n_frames)]
    return lines, paths, sum(os.path.getsize(p) for p in paths) / n_frames


def step_png(args):
    """[13] ``image_codecs.decode_png_batch`` against the parent route (pil_loader on 16 threads + np.stack + upload), its phases, the
    inflate alone against zlib and Pillow on one thread, the builder and the trainer fed by either route, and the completion loader's
    depth planes.  The routes alternate inside this one run."""
    import concurrent.futures
    import ctypes
    import zlib
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from fusiondepth_amd import _lib, completion_data as CD, image_codecs
    from fusiondepth_amd.datasets import KITTIRAWBatches, pil_loader
    import png_ref
    N = 36
    with tempfile.TemporaryDirectory() as root:
        lines, paths, mean_size = write_png_tree(root, N + 14)
        batch_paths = paths[:N]
        datas = [open(p, "rb").read() for p in batch_paths]
        filters = np.bincount(np.concatenate([png_ref.scanlines(d)[1][:, 0] for d in datas[:4]]), minlength=5)
        say("[13] PNG frames: %d frames of %dx%d, 8-bit RGB, written by Pillow with its default settings from textured synthetic content; "
            "%.0f KB per file; filter types of the first four files' rows (None Sub Up Average Paeth): %s (not a KITTI frame: KITTI's own "
            "PNGs come from another encoder)" % (N, W0, H0, mean_size / 1e3, " ".join(str(int(v)) for v in filters)))
        pool = concurrent.futures.ThreadPoolExecutor(WORKERS)

        def route_device():
            frames, stats = image_codecs.decode_png_batch(batch_paths, pool=pool)
            torch.cuda.synchronize()
            assert stats["fallback"] == 0, stats
            return frames

        def route_pil():
            stack = torch.from_numpy(np.stack(list(pool.map(pil_loader, batch_paths)))).to("cuda", non_blocking=True)
            torch.cuda.synchronize()
            return stack

        got, want = route_device(), route_pil()
        assert all(torch.equal(g, w) for g, w in zip(got, want)), "the routes disagree"
        t = {"device": [], "pil": []}
        for _ in range(args.iters):
            for name, fn in (("device", route_device), ("pil", route_pil)):
                t0 = time.perf_counter()
                fn()
                t[name].append(1e3 * (time.perf_counter() - t0))
        for name, label in (("device", "decode_png_batch (host inflate on %d threads + one upload + fd_png_unfilter)" % WORKERS),
                            ("pil", "pil_loader on %d threads + np.stack + upload (the parent's route)" % WORKERS)):
            med = float(np.median(t[name]))
            say("    %-88s %7.1f frames/s, ms per batch of %d: %s  (%d alternating runs)" % (label + ":", 1e3 * N / med, N, _spread(t[name]), args.iters))

        # one thread, per frame: the inflate alone against zlib's and against Pillow's whole decode
        info = image_codecs.png_probe(datas[0])[1]
        dst = np.empty(info.raw_bytes, np.uint8)
        streams = [png_ref.idat(d) for d in datas]
        one = {"inflate": [], "zlib": [], "pillow": []}
        for _ in range(3):
            t0 = time.perf_counter()
            for d in datas:
                assert image_codecs.png_inflate(d, dst)[0] == 0
            one["inflate"].append(1e3 * (time.perf_counter() - t0) / N)
            t0 = time.perf_counter()
            for s in streams:
                zlib.decompress(s)
            one["zlib"].append(1e3 * (time.perf_counter() - t0) / N)
            t0 = time.perf_counter()
            for p in batch_paths:
                pil_loader(p)
            one["pillow"].append(1e3 * (time.perf_counter() - t0) / N)
        i1, z1, p1 = min(one["inflate"]), min(one["zlib"]), min(one["pillow"])
        say("    one thread, per frame: fd_png_inflate (chunk walk, inflate, Adler-32, filter bytes) %.2f ms, zlib.decompress of the joined "
            "IDAT data (zlib %s) %.2f ms, Pillow's whole decode %.2f ms -> the inflate written here is %s than zlib's (%.2fx) and %.2fx "
            "Pillow's whole decode" % (i1, zlib.ZLIB_RUNTIME_VERSION, z1, p1, "SLOWER" if i1 > z1 else "faster", z1 / i1, p1 / i1))

        # inside the batch
        host_ms, up_ms, k_ms = [], [], []
        rgb_bytes = N * 3 * H0 * W0
        for _ in range(args.iters):
            t0 = time.perf_counter()
            job = image_codecs.PngBatchJob(batch_paths, pool)
            lay = job.wait_host()
            host_ms.append(1e3 * (time.perf_counter() - t0))
            table, _, _, _, out_bytes = job.layout()
            lay["staging"].numpy()[:N * ctypes.sizeof(_lib.PngDesc)] = np.frombuffer(table, dtype=np.uint8)
            dev = torch.empty((lay["upload_bytes"],), dtype=torch.uint8, device="cuda")
            out = torch.empty((out_bytes,), dtype=torch.uint8, device="cuda")
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            dev.copy_(lay["staging"], non_blocking=True)
            ev[1].record()
            ev[2].record()
            _lib.call("fd_png_unfilter", dev.data_ptr(), lay["upload_bytes"], ctypes.addressof(table), N, out.data_ptr(), out_bytes, _lib.stream())
            ev[3].record()
            torch.cuda.synchronize()
            up_ms.append(ev[0].elapsed_time(ev[1]))
            k_ms.append(ev[2].elapsed_time(ev[3]))
        up_bytes, raw_bytes = lay["upload_bytes"], N * info.raw_bytes
        traffic = raw_bytes + rgb_bytes                          # the filtered bytes read once, the RGB bytes written once
        bound_ms = 1e3 * traffic / HBM_BPS
        km, batch_ms = float(np.median(k_ms)), float(np.median(t["device"]))
        say("    inside the batch: host phase (read + probe + inflate, %d threads) %s ms" % (WORKERS, _spread(host_ms)))
        say("                      upload %.1f MB (filtered scanlines = %.3fx the RGB bytes) %s ms = %.1f GB/s"
            % (up_bytes / 1e6, raw_bytes / rgb_bytes, _spread(up_ms), up_bytes / 1e6 / float(np.median(up_ms))))
        say("                      the two kernels (device events around fd_png_unfilter) %s ms = %.1f %% of the batch; traffic bound %.1f MB "
            "(filtered bytes in, RGB out) at %.1f TB/s = %.4f ms -> %.1fx the bound"
            % (_spread(k_ms), 100 * km / batch_ms, traffic / 1e6, HBM_BPS / 1e12, bound_ms, km / bound_ms))

        # the completion loader's depth planes: --step completion's workload (batch 4 x 3 frames + 4 ground-truth maps, 5 % dense)
        rng = np.random.default_rng(5)
        from PIL import Image
        depth_paths = []
        for k in range(COMPLETION_BATCH * FRAMES + COMPLETION_BATCH):
            codes = rng.integers(256, 80 * 256, (H0, W0)).astype(np.uint16)
            codes[rng.random(codes.shape) >= 0.05] = 0
            depth_paths.append(os.path.join(root, "depth_%02d.png" % k))
            Image.fromarray(codes).save(depth_paths[-1])
        plane = (H0 * W0 + 3) // 4 * 4

        def depth_pil():
            staging = torch.empty((2 * plane * len(depth_paths),), dtype=torch.uint8, pin_memory=True)
            data = staging.numpy().view(np.uint16)
            for f in [pool.submit(CD._depth_into, p, data[k * plane:k * plane + H0 * W0].reshape(H0, W0)) for k, p in enumerate(depth_paths)]:
                f.result()
            dev = staging.to("cuda", non_blocking=True)
            torch.cuda.synchronize()
            return dev.view(torch.int16).view(len(depth_paths), plane)[:, :H0 * W0]

        def depth_device():
            frames, stats = image_codecs.decode_png_batch(depth_paths, pool=pool, mode="gray16")
            high = torch.stack([f.view(torch.uint8).view(-1)[1::2].amax() for f in frames]).cpu()          # the loader's 16-bit assertion
            assert stats["fallback"] == 0 and bool((high > 0).all())
            return frames

        a, b = depth_pil(), depth_device()
        assert all(torch.equal(x.view(torch.int16).view(-1), y) for x, y in zip(b, a)), "the depth routes disagree"
        td = {"device": [], "pil": []}
        for _ in range(args.iters):
            for name, fn in (("device", depth_device), ("pil", depth_pil)):
                t0 = time.perf_counter()
                fn()
                td[name].append(1e3 * (time.perf_counter() - t0))
        say("    completion depth planes (%d 16-bit PNGs of %dx%d, 5 %% dense, %.0f KB per file), ms per batch until the planes are on the device:"
            % (len(depth_paths), W0, H0, sum(os.path.getsize(p) for p in depth_paths) / len(depth_paths) / 1e3))
        say("        png_decoder='device' (inflate + upload + fd_png_unfilter + the 16-bit check's download): %s" % _spread(td["device"]))
        say("        png_decoder='pil'    (Pillow + copy into the pinned buffer + upload):                   %s" % _spread(td["pil"]))

        # the builder from the PNG tree, both routes, alternating
        opt = _opt(BATCH)

        def run(decoder, epochs=2):
            b = KITTIRAWBatches(root, lines, HEIGHT, WIDTH, [0, -1, 1], SCALES, is_train=True, img_ext=".png", opt=opt, batch_size=BATCH, shuffle=True,
                                seed=1, workers=WORKERS, png_decoder=decoder)
            for _ in b:
                pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for _ in range(epochs):
                for batch in b:
                    n += batch[("color", 0, 0)].shape[0]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            b.close()
            return n / dt

        rates = {"pil": [], "device": []}
        for _ in range(5):
            for name in ("pil", "device"):
                rates[name].append(run(name, epochs=4))
        sp = {k: max(v) - min(v) for k, v in rates.items()}
        mp, md = float(np.median(rates["pil"])), float(np.median(rates["device"]))
        say("    KITTIRAWBatches from the PNG tree, batch %d, %d items per epoch, 5 alternating runs of 4 epochs each:" % (BATCH, len(lines)))
        say("        png_decoder='pil':    %7.1f items/s (runs %s; spread %.1f)" % (mp, " ".join("%.1f" % v for v in rates["pil"]), sp["pil"]))
        say("        png_decoder='device': %7.1f items/s (runs %s; spread %.1f)" % (md, " ".join("%.1f" % v for v in rates["device"]), sp["device"]))
        say("        difference %+.1f items/s against the larger spread %.1f: the device route %s"
            % (md - mp, max(sp.values()), "WINS" if md - mp > max(sp.values()) else ("LOSES" if mp - md > max(sp.values()) else "is within the spread")))
        pool.shutdown()

        if args.windows > 0:
            from fusiondepth_amd.trainer import Trainer
            torch.manual_seed(1)
            tr = Trainer(opt, verbose=False)
            per_step = tr.batch_size * tr.accumulate_step
            feeds = {}
            for name in ("pil", "device"):
                b = KITTIRAWBatches(root, lines, HEIGHT, WIDTH, [0, -1, 1], SCALES, is_train=True, img_ext=".png", opt=opt, batch_size=tr.batch_size,
                                    shuffle=True, seed=1, workers=WORKERS, png_decoder=name)

                def endless(b=b):
                    while True:
                        for batch in b:
                            yield batch
                feeds[name] = (b, endless())
            res = {"pil": [], "device": []}
            for name in feeds:
                for _ in range(3):
                    tr.train_step([next(feeds[name][1]) for _ in range(tr.accumulate_step)])
            for _ in range(args.windows):
                for name in ("pil", "device"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        tr.train_step([next(feeds[name][1]) for _ in range(tr.accumulate_step)])
                    torch.cuda.synchronize()
                    res[name].append((time.perf_counter() - t0) / args.steps)
            for name in feeds:
                feeds[name][0].close()
                m = float(np.median(res[name]))
                say("    Trainer (ResNet-18, %dx%d, %d images / step) fed by png_decoder='%s': %s %.1f images/s (%.2f ms / step; windows %s)"
                    % (WIDTH, HEIGHT, per_step, name, " " * (6 - len(name)), per_step / m, 1e3 * m, " ".join("%.2f" % (1e3 * v) for v in res[name])))
        say("    not measured: a real KITTI tree (another encoder: other filter choices and compression); more than one rank sharing the "
            "host's %d threads; the completion loader end to end" % WORKERS)


# ---------------------------------------------------------------------------------------------------- 5-8. raw Velodyne scans
PEAK_BPS = 8.0e12
LINE_SPEC = [2, 7, 12, 16]


def _ref():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sparsify_ref
    return sparsify_ref


def write_raw_tree(root, n_frames):
    """write_tree plus 64-ring raw scans (about 128 k points, 2 MB each); ``4beam/`` is then rewritten from them by the offline tool, so
    that file mode and raw mode build the same batches."""
    from fusiondepth_amd import sparsify as SP
    SR = _ref()
    lines, _ = write_tree(root, n_frames, (".png",))
    folder = lines[0].split()[0]
    os.makedirs(os.path.join(root, folder, "velodyne_points/data"), exist_ok=True)
    for i in range(n_frames):
        SR.synthetic_scan(500 + i).tofile(os.path.join(root, folder, "velodyne_points/data/%010d.bin" % i))
    split = os.path.join(root, "scans.txt")
    with open(split, "w") as f:
        f.write("".join("%s %d l\n" % (folder, i) for i in range(n_frames)))
    SP.main(["--W", "1024", "--H", "64", "--line_spec"] + [str(r) for r in LINE_SPEC] + ["--ptc_path", root + "/", "--output_path", root + "/",
                                                                                        "--split_file", split])
    return lines, split


def step_sparsify(args):
    import torch
    sys.path.insert(0, ROOT)
    from fusiondepth_amd import functional as FD
    SR = _ref()
    S = BATCH * FRAMES
    scans = [SR.synthetic_scan(700 + i % 6) for i in range(S)]
    ends = np.cumsum([0] + [len(p) for p in scans])
    packed = torch.from_numpy(np.concatenate(scans)).cuda()
    offsets = torch.tensor(ends, dtype=torch.int32).cuda()
    K = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
    V = np.array([[7.533745e-03, -9.999714e-01, -6.166020e-04, -4.069766e-03], [1.480249e-02, 7.280733e-04, -9.998902e-01, -7.631618e-02],
                  [9.998621e-01, 7.523790e-03, 1.480755e-02, -2.717806e-01], [0.0, 0.0, 0.0, 1.0]])
    descs = [(K @ V, H0, W0, bool(i % 2)) for i in range(S)]
    table = torch.frombuffer(bytearray(bytes(FD.raster_desc_table(descs))), dtype=torch.uint8).cuda()
    staging = torch.empty((packed.numel() * 4,), dtype=torch.uint8, pin_memory=True)
    cap = len(LINE_SPEC) * 1024

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        return float(np.median(times)), min(times), max(times)

    keep = {}

    def sparsify():
        keep["slab"] = FD.sparsify_scans(packed, 64, 1024, LINE_SPEC, offsets=offsets)[0]

    def random100():
        FD.sparsify_scans(packed, 64, 1024, random_sample=100, keys=list(range(S)), offsets=offsets)

    def beams():
        FD.velo_rasterize_batch(keep["slab"], descs, (2 * HEIGHT, 2 * WIDTH), desc_table=table)

    def depth_gt():
        FD.velo_rasterize_batch(packed, descs[:BATCH], (375, 1242), return_full=True, beam=False, offsets=offsets[:BATCH + 1],
                                n_max=max(len(p) for p in scans[:BATCH]), desc_table=table[:BATCH * 112])

    say("[5] raw-scan LiDAR path, batch %d: %d scans, %d points (%.1f MB), device events, median of %d (min, max)"
        % (BATCH, S, ends[-1], 16 * ends[-1] / 1e6, args.iters))
    comp = 16 * ends[-1] + 16 * S * cap
    ms = timed(sparsify)
    say("    fd_sparsify_scans, rows %s (4 launches + 1 memset): %.3f ms (%.3f, %.3f); compulsory traffic (points read once, slab written once) "
        "%.1f MB = %.1f us at 8 TB/s -> %.1fx the bound, %.2f TB/s" % (LINE_SPEC, ms[0], ms[1], ms[2], comp / 1e6, 1e6 * comp / PEAK_BPS,
                                                                       ms[0] * 1e-3 / (comp / PEAK_BPS), comp / (ms[0] * 1e-3) / 1e12))
    comp_r = 16 * ends[-1] + 16 * S * 64 * 1024
    ms = timed(random100)
    say("    fd_sparsify_scans, random 100 over all 64 rows (7 launches + 1 memset; the table upload of the keys included): %.3f ms (%.3f, %.3f); "
        "compulsory %.1f MB = %.1f us -> %.1fx" % (ms[0], ms[1], ms[2], comp_r / 1e6, 1e6 * comp_r / PEAK_BPS, ms[0] * 1e-3 / (comp_r / PEAK_BPS)))
    ms = timed(beams)
    say("    fd_velo_rasterize_batch, %d slabs of %d rows -> beam maps %dx%d (4 launches): %.3f ms (%.3f, %.3f)"
        % (S, cap, WIDTH, HEIGHT, ms[0], ms[1], ms[2]))
    ms = timed(depth_gt)
    say("    fd_velo_rasterize_batch, %d raw scans -> depth_gt 1242x375 float64 (4 launches): %.3f ms (%.3f, %.3f)" % (BATCH, ms[0], ms[1], ms[2]))
    ms = timed(lambda: staging.to("cuda", non_blocking=True))
    say("    upload of the batch's pinned staging buffer (%.1f MB, one copy): %.3f ms (%.3f, %.3f) = %.1f GB/s; the 4-beam files of a batch are "
        "%.0f KB" % (staging.numel() / 1e6, ms[0], ms[1], ms[2], staging.numel() / (ms[0] * 1e-3) / 1e9, S * 2000 * 16 / 1e3))


def _raw_pair(root, lines, opt, batch_size):
    from fusiondepth_amd.datasets import KITTIRAWBatches
    load = _cached_loader()
    mk = lambda source: KITTIRAWBatches(root, lines, HEIGHT, WIDTH, [0, -1, 1], SCALES, is_train=True, img_ext=".png", opt=opt,
                                        batch_size=batch_size, shuffle=True, seed=1, workers=WORKERS, loader=load, lidar_source=source)
    return mk("files"), mk("raw")


def step_raw_builder(args):
    import torch
    sys.path.insert(0, ROOT)
    with tempfile.TemporaryDirectory() as root:
        lines, _ = write_raw_tree(root, 50)
        files, raw = _raw_pair(root, lines, _opt(BATCH), BATCH)

        def epochs(b, n):
            torch.cuda.synchronize()
            t = time.perf_counter()
            k = 0
            for _ in range(n):
                for batch in b:
                    k += batch[("color", 0, 0)].shape[0]
            torch.cuda.synchronize()
            return k / (time.perf_counter() - t)

        for b in (files, raw):
            epochs(b, 1)                                              # warm-up: the frame cache, the page cache, code objects
        res = {"files": [], "raw": []}
        for _ in range(args.windows):
            res["files"].append(epochs(files, 2))
            res["raw"].append(epochs(raw, 2))
        files.close()
        raw.close()
        say("[6] KITTIRAWBatches, batch %d, pre-decoded frames, 4beam + 2channel + depth_gt keys, %d alternating windows of 2 epochs (%d items each):"
            % (BATCH, args.windows, len(lines) // BATCH * BATCH))
        for name, what in (("files", "file mode (4beam/*.bin + the raw scan for depth_gt)"), ("raw", "raw mode (velodyne_points only)")):
            say("    %-55s %7.1f items/s (windows %s)" % (what + ":", float(np.median(res[name])), " ".join("%.1f" % v for v in res[name])))


def step_raw_trainer(args):
    import torch
    sys.path.insert(0, ROOT)
    from fusiondepth_amd import synthetic
    from fusiondepth_amd.trainer import Trainer
    torch.manual_seed(1)
    with tempfile.TemporaryDirectory() as root:
        lines, _ = write_raw_tree(root, 50)
        opt = _opt(BATCH)
        tr = Trainer(opt, verbose=False)
        per_step = tr.batch_size * tr.accumulate_step
        files, raw = _raw_pair(root, lines, opt, tr.batch_size)

        def endless(b):
            while True:
                for batch in b:
                    batch.pop("depth_gt", None)                        # as for the synthetic batches: the step itself stays the same
                    yield batch
        feeds = {"files": endless(files), "raw": endless(raw)}
        pool = []
        for i in range(8):
            mbs = [synthetic.make_scene_batch(tr.batch_size, HEIGHT, WIDTH, seed=1234 + 17 * i + j, clutter=0.5) for j in range(tr.accumulate_step)]
            for mb in mbs:
                mb.pop("depth_gt", None)
                for f in (-1, 1):
                    mb.pop(("T_gt", f), None)
            pool.append(mbs)
        k = [0]

        def step_syn():
            k[0] += 1
            tr.train_step(pool[k[0] % len(pool)])

        steps = {"synthetic": step_syn, "files": lambda: tr.train_step([next(feeds["files"]) for _ in range(tr.accumulate_step)]),
                 "raw": lambda: tr.train_step([next(feeds["raw"]) for _ in range(tr.accumulate_step)])}

        def window(fn, n):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / n

        for _ in range(4):
            for fn in steps.values():
                fn()
        res = {name: [] for name in steps}
        for _ in range(args.windows):
            for name, fn in steps.items():
                res[name].append(window(fn, args.steps))
        files.close()
        raw.close()
        say("[7] Trainer (ResNet-18, %dx%d, --batch_size %d = %d images / step), %d alternating windows of %d steps; the builders also make "
            "depth_gt (dropped before the step):" % (WIDTH, HEIGHT, BATCH, per_step, args.windows, args.steps))
        for name, what in (("synthetic", "fed make_scene_batch batches"), ("files", "fed by KITTIRAWBatches, file mode (pre-decoded)"),
                           ("raw", "fed by KITTIRAWBatches, raw mode (pre-decoded)")):
            v = float(np.median(res[name]))
            say("    %-50s %.1f images/s (%.2f ms / step; windows %s)" % (what + ":", per_step / v, 1e3 * v, " ".join("%.2f" % (1e3 * w) for w in res[name])))


def step_offline_worker(args):
    SR = _ref()
    t = time.perf_counter()
    n = 0
    for line in open(args.split_file).read().split("\n")[args.worker::WORKERS]:
        if not line.strip():
            continue
        folder, frame = line.split()[0], int(line.split()[1])
        scan = np.fromfile(os.path.join(args.root, folder, "velodyne_points/data/%010d.bin" % frame), dtype=np.float32).reshape(-1, 4)
        out = scan[SR.sparsify_indices(scan, W=1024, line_spec=LINE_SPEC)]
        os.makedirs(os.path.join(args.root, folder, "4beam_numpy"), exist_ok=True)
        out.tofile(os.path.join(args.root, folder, "4beam_numpy/%010d.bin" % frame))
        n += 1
    say(json.dumps({"scans": n, "seconds": time.perf_counter() - t}))


def step_offline(args):
    import torch
    sys.path.insert(0, ROOT)
    from fusiondepth_amd import sparsify as SP
    n = 192
    with tempfile.TemporaryDirectory() as root:
        lines, split = write_raw_tree(root, n)                       # runs the tool once: warm-up (code objects, page cache)
        argv = ["--W", "1024", "--H", "64", "--line_spec"] + [str(r) for r in LINE_SPEC] + ["--ptc_path", root + "/", "--output_path", root + "/",
                                                                                           "--split_file", split]
        gpu, cpu = [], []
        for _ in range(args.windows):
            t = time.perf_counter()
            SP.run(SP.parse_args(argv))
            torch.cuda.synchronize()
            gpu.append(n / (time.perf_counter() - t))
            t = time.perf_counter()
            procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--step", "offline_worker", "--root", root, "--split_file", split,
                                       "--worker", str(w)], stdout=subprocess.PIPE, text=True) for w in range(WORKERS)]
            outs = [json.loads(p.communicate()[0].strip().splitlines()[-1]) for p in procs]
            wall = time.perf_counter() - t
            if any(p.returncode for p in procs):
                sys.exit("a numpy worker failed")
            cpu.append((n / max(o["seconds"] for o in outs), n / wall))
        say("[8] offline tool, %d scans of about 128 k points (2 MB files, page cache warm), rows %s, %d alternating runs:" % (n, LINE_SPEC, args.windows))
        say("    python -m fusiondepth_amd.sparsify (16 file threads, 32 scans per call): %.0f scans/s (runs %s)"
            % (float(np.median(gpu)), " ".join("%.0f" % v for v in gpu)))
        say("    numpy restatement on %d processes:                                      %.0f scans/s over the workers' loops (runs %s); %.0f scans/s "
            "incl. process start" % (WORKERS, float(np.median([c[0] for c in cpu])), " ".join("%.0f" % c[0] for c in cpu),
                                     float(np.median([c[1] for c in cpu]))))

# ---------------------------------------------------------------------------------------------------- 9 / 10. the Refiner's loader
GDC_BATCH = 6


def step_inf_gdc_key(args):
    import torch
    sys.path.insert(0, ROOT)
    from fusiondepth_amd import functional as FD
    B = GDC_BATCH
    rng = np.random.default_rng(3)
    descs = [(k * H0 * W0, H0, W0, bool(k % 2)) for k in range(B)]
    table = np.frombuffer(FD.resize_desc_table(descs), dtype=np.uint8)
    base = (table.size + 15) // 16 * 16
    staging = torch.empty((base + 4 * B * H0 * W0,), dtype=torch.uint8, pin_memory=True)
    staging.numpy()[:table.size] = table
    staging.numpy()[base:].view(np.float32)[:] = rng.uniform(0.05, 80.0, B * H0 * W0).astype(np.float32)
    dev = staging.cuda()

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        return float(np.median(times)), min(times), max(times)

    read, write = 4 * B * H0 * W0, 4 * B * HEIGHT * WIDTH
    say("[9] inf_gdc key, batch %d, %dx%d -> %dx%d, device events, median of %d (min, max)" % (B, W0, H0, WIDTH, HEIGHT, args.iters))
    up = timed(lambda: staging.to("cuda", non_blocking=True))
    say("    upload of the batch's pinned staging buffer (%.1f MB, one copy): %.3f ms (%.3f, %.3f) = %.1f GB/s"
        % (staging.numel() / 1e6, up[0], up[1], up[2], staging.numel() / (up[0] * 1e-3) / 1e9))
    ms = timed(lambda: FD.resize_bilinear_batch(dev[base:].view(torch.float32), descs, (HEIGHT, WIDTH), desc_table=dev[:table.size]))
    comp = read + write
    say("    fd_resize_bilinear_batch (1 launch; the output allocation included): %.3f ms (%.3f, %.3f); compulsory traffic read %.1f MB + "
        "write %.1f MB = %.2f us at 8 TB/s -> %.1fx the bound, %.2f TB/s"
        % (ms[0], ms[1], ms[2], read / 1e6, write / 1e6, 1e6 * comp / PEAK_BPS, ms[0] * 1e-3 / (comp / PEAK_BPS), comp / (ms[0] * 1e-3) / 1e12))
    say(json.dumps({"gdc_key_ms_per_batch": up[0] + ms[0], "batch": B}))


def step_gdc_trace_report(args):
    """The kernel's own time from the rocprofv3 results database of a traced ``inf_gdc_key`` run."""
    import sqlite3
    files = sorted(glob.glob(os.path.join(args.trace_dir, "**", "*_results.db"), recursive=True))
    if not files:
        sys.exit("no rocprofv3 results database under %s" % args.trace_dir)
    db = sqlite3.connect(files[-1])
    rows = list(db.execute("select count(*), avg(end-start)/1e3, min(end-start)/1e3, max(end-start)/1e3 from kernels where name like "
                           "'%k_resize_bilinear_batch%'"))
    n, avg, lo, hi = rows[0]
    if not n:
        sys.exit("k_resize_bilinear_batch is not in the trace")
    comp = 4 * GDC_BATCH * (H0 * W0 + HEIGHT * WIDTH)
    say("    rocprofv3 --kernel-trace --stats (a run of its own), k_resize_bilinear_batch, %d launches: avg %.2f us (min %.2f, max %.2f) = %.1fx the "
        "%.2f us traffic bound, %.2f TB/s (bound by HBM bytes; the arithmetic is 13 float operations per output pixel)"
        % (n, avg, lo, hi, avg * 1e-6 / (comp / PEAK_BPS), 1e6 * comp / PEAK_BPS, comp / (avg * 1e-6) / 1e12))


def step_refiner_trainer(args):
    import torch
    sys.path.insert(0, ROOT)
    from fusiondepth_amd import synthetic
    from fusiondepth_amd.datasets import KITTIRefinerBatches
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.refiner import Refiner
    from fusiondepth_amd.trainer import Trainer
    torch.manual_seed(1)
    with tempfile.TemporaryDirectory() as root:
        lines, _ = write_tree(root, 50, (".png",))
        rng = np.random.default_rng(9)
        for line in lines:
            folder, frame, side = line.split()
            os.makedirs(os.path.join(root, folder, "inf_gdc_4beam"), exist_ok=True)
            np.save(os.path.join(root, folder, "inf_gdc_4beam", "%d_%s.npy" % (int(frame), side)), rng.uniform(0.05, 80.0, (H0, W0)).astype(np.float32))
        base = ["--num_layers", "18", "--weights_init", "scratch", "--batch_size", str(BATCH), "--height", str(HEIGHT), "--width", str(WIDTH)]
        tr = Trainer(MonodepthOptions().parse(base + ["--log_dir", os.path.join(root, "log"), "--model_name", "stage1"]), verbose=False)
        weights = tr.save_model("stage1")
        del tr
        rf = Refiner(MonodepthOptions().parse(base + ["--refine_load_weights_folder", weights]), verbose=False)
        B = rf.batch_size
        b = KITTIRefinerBatches(root, lines, HEIGHT, WIDTH, [0, -1, 1], SCALES, is_train=True, img_ext=".png", opt=rf.opt, batch_size=B, shuffle=True,
                                seed=1, workers=WORKERS, loader=_cached_loader())

        def endless():
            while True:
                for batch in b:
                    yield batch
        real = endless()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(5)
        pool = []
        for i in range(3):
            inp = synthetic.make_batch(B, HEIGHT, WIDTH, seed=77 + i)
            inp["inf_gdc"] = torch.empty(B, 1, HEIGHT, WIDTH, device="cuda").uniform_(0.05, 1.5, generator=gen)
            pool.append(inp)
        k = [0]
        cur = [next(real)]

        def step_syn():                                            # bench.py's refiner configuration: the next batch is announced
            k[0] += 1
            rf.train_step(pool[k[0] % 3], pool[(k[0] + 1) % 3])

        def step_real():                                           # Refiner.run_epoch reads one batch ahead in the same way
            nxt = next(real)
            rf.train_step(cur[0], nxt)
            cur[0] = nxt

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
        say("[10] Refiner (ResNet-18, %dx%d, --batch_size %d = %d images / step), %d alternating windows of %d steps:" % (WIDTH, HEIGHT, BATCH, B,
                                                                                                                        args.windows, args.steps))
        say("    fed synthetic batches (bench.py's refiner configuration): %.1f images/s (%.2f ms / step; windows %s)"
            % (B / syn, 1e3 * syn, " ".join("%.2f" % (1e3 * v) for v in res["synthetic"])))
        say("    fed by KITTIRefinerBatches (pre-decoded frames, inf_gdc maps from .npy files): %.1f images/s (%.2f ms / step; windows %s)"
            % (B / rl, 1e3 * rl, " ".join("%.2f" % (1e3 * v) for v in res["builder"])))
        if args.colour_ms > 0 or args.gdc_ms > 0:
            if B != GDC_BATCH:
                sys.exit("steps 1 and 9 were measured at batch %d, the Refiner's batch is %d" % (GDC_BATCH, B))
            dev_ms = args.colour_ms + args.gdc_ms
            share = dev_ms / (1e3 * syn)
            say("    condition: colour path %.3f ms + inf_gdc key (upload + library call) %.3f ms, both measured at batch %d = %.3f ms = %.1f %% of "
                "the synthetic-fed Refiner step (%.2f ms): %s the 10 %% limit.  As in step 4, file mode's LiDAR keys (per-item scan uploads, "
                "rasterisation and scatter launches) are NOT in this sum: the figure is the builder's colour path and the new key, not all "
                "of its device work" % (args.colour_ms, args.gdc_ms, B, dev_ms, 100 * share, 1e3 * syn, "within" if share <= 0.10 else "ABOVE"))


# ---------------------------------------------------------------------------------------------------- 11. depth completion
COMPLETION_BATCH = 4


def step_completion_keys(args):
    import torch
    sys.path.insert(0, ROOT)
    from fusiondepth_amd import completion_data as CD, data_ops, evaluate_completion as EC
    from fusiondepth_amd.evaluate_depth import _median
    B, F = COMPLETION_BATCH, FRAMES
    rng = np.random.default_rng(5)
    n_planes = F * B + B                                         # sparse planes frame-major, then ground truth
    plane = (H0 * W0 + 3) // 4 * 4
    beam = [CD.depth_desc(k * plane, H0, W0, bool(k % 2), True, False) for k in range(F * B)]
    gt = [CD.depth_desc((F * B + k) * plane, H0, W0, bool(k % 2), True, False) for k in range(B)]
    full = [CD.depth_desc(k * plane, H0, W0, bool(k % 2), True, True) for k in range(B)]
    tables = [np.frombuffer(data_ops.depth_png_desc_table([d for d, _ in t]), dtype=np.uint8) for t in (beam, gt, full)]
    at, pos = [], 0
    for t in tables:
        at.append((pos, pos + t.size))
        pos = (pos + t.size + 15) // 16 * 16
    staging = torch.empty((pos + 2 * n_planes * plane,), dtype=torch.uint8, pin_memory=True)
    host = staging.numpy()
    for t, (a, b) in zip(tables, at):
        host[a:b] = t
    codes = rng.integers(256, 80 * 256, n_planes * plane).astype(np.uint16)
    codes[rng.random(codes.size) >= 0.05] = 0
    host[pos:].view(np.uint16)[:] = codes
    dev = staging.cuda()
    packed = dev[pos:].view(torch.int16)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        return float(np.median(times)), min(times), max(times)

    say("[11] depth-completion keys, batch %d x %d frames, %dx%d sources, full-res mode; device events, median of %d (min, max)" % (B, F, W0, H0, args.iters))
    up = timed(lambda: staging.to("cuda", non_blocking=True))
    say("    upload of the batch's pinned staging buffer (%.1f MB, one copy): %.3f ms (%.3f, %.3f) = %.1f GB/s"
        % (staging.numel() / 1e6, up[0], up[1], up[2], staging.numel() / (up[0] * 1e-3) / 1e9))
    total = up[0]
    for name, descs, k, channels, div1 in (("beam planes -> (2channel, f, 0), 4beam", beam, 0, 2, 100.0), ("depth_gt", gt, 1, 1, 1.0),
                                           ("full_res_4beam", full, 2, 1, 1.0)):
        canvas = descs[0][1]
        ms = timed(lambda: data_ops.depth_png_keys(packed, [d for d, _ in descs], canvas, 1, channels, 256.0, div1,
                                                   desc_table=dev[at[k][0]:at[k][1]]))
        read = 2 * len(descs) * 352 * 1216                       # the cropped rectangle of every plane
        write = 4 * len(descs) * channels * canvas[0] * canvas[1]
        comp = read + write
        total += ms[0]
        say("    fd_depth_png_keys, %s (%d planes, 1 launch; the output allocation included): %.3f ms (%.3f, %.3f); compulsory traffic read "
            "%.1f MB + write %.1f MB = %.2f us at 6.3 TB/s (achievable HBM) -> %.1fx the bound, %.2f TB/s"
            % (name, len(descs), ms[0], ms[1], ms[2], read / 1e6, write / 1e6, 1e6 * comp / HBM_BPS, ms[0] * 1e-3 / (comp / HBM_BPS),
               comp / (ms[0] * 1e-3) / 1e12))
    frames = torch.from_numpy(np.stack([frame(i % 6)[H0 - 352:, 13:13 + 1216] for i in range(F * B)])).cuda()
    flip = [bool((i // 2) % 2) for i in range(F * B)]
    jitter = [JITTER if i % 2 else None for i in range(F * B)]
    ms = timed(lambda: data_ops.image_pyramid(frames, 352, 1216, SCALES, flip, jitter))
    total += ms[0]
    say("    colour path at 352x1216 (%d cropped frames, %d scales, half jittered, 10 launches): %.3f ms (%.3f, %.3f)" % (F * B, SCALES, ms[0], ms[1], ms[2]))
    say("    the batch's device work (upload + three key calls + colour): %.3f ms" % total)
    # the scorer, per image, beside the torch.sort-based median recipe of evaluate_depth.py on the same tensors
    N = 8
    v, u = np.meshgrid(np.arange(352, dtype=np.float32), np.arange(1216, dtype=np.float32), indexing="ij")
    truth = np.stack([5.0 + n + 40.0 * (1.0 - v / 352) + 3.0 * np.sin(u / 80.0) for n in range(N)]).astype(np.float32)
    g = torch.from_numpy(np.where(rng.random(truth.shape) < 0.15, truth, 0.0).astype(np.float32)).cuda()
    p = torch.from_numpy((truth * 0.5 + rng.normal(0, 0.1, truth.shape)).astype(np.float32)).cuda()
    med = timed(lambda: EC.completion_medians(p, g))
    ratio = EC.completion_medians(p, g)[:, 0].contiguous()
    err = timed(lambda: EC.completion_errors(p, g, ratio))

    def recipe():
        out = []
        for n in range(N):
            m = g[n] > 0.1
            gs, ps = g[n][m], p[n][m]
            ps = torch.clamp(ps * (_median(gs) / _median(ps)), 1e-3, 80)
            d, di = gs * 1000.0 - ps * 1000.0, 1.0 / (gs * 0.001) - 1.0 / (ps * 0.001)
            out.append(torch.stack([(d * d).double().mean().sqrt(), d.abs().double().mean(), (di * di).double().mean().sqrt(), di.abs().double().mean()]))
        return torch.stack(out)

    rec = timed(recipe)
    p1, g1, r1 = p[:1].contiguous(), g[:1].contiguous(), ratio[:1].contiguous()
    med1, err1 = timed(lambda: EC.completion_medians(p1, g1)), timed(lambda: EC.completion_errors(p1, g1, r1))
    N_all, N = N, 1
    rec1 = timed(recipe)
    N = N_all
    assert np.allclose(recipe().cpu().numpy(), EC.completion_errors(p, g, ratio)[:, :4].cpu().numpy(), rtol=1e-6)
    say("    scorer, %d images of 352x1216, 15 %% ground truth: fd_completion_medians %.3f ms (%.3f, %.3f) = %.1f us / image; "
        "fd_completion_errors %.3f ms (%.3f, %.3f) = %.1f us / image" % (N, med[0], med[1], med[2], 1e3 * med[0] / N, err[0], err[1], err[2], 1e3 * err[0] / N))
    say("    the same scores with boolean selection + torch.sort medians (evaluate_depth._median), ATen: %.3f ms (%.3f, %.3f) = %.1f us / image "
        "-> %.1fx the two kernels" % (rec[0], rec[1], rec[2], 1e3 * rec[0] / N, rec[0] / (med[0] + err[0])))
    say("    ONE image (latency: the medians run two workgroups, nothing beside them): fd_completion_medians %.3f ms (%.3f, %.3f), "
        "fd_completion_errors %.3f ms (%.3f, %.3f); the ATen recipe %.3f ms (%.3f, %.3f) -> %.2fx the two kernels"
        % (med1[0], med1[1], med1[2], err1[0], err1[1], err1[2], rec1[0], rec1[1], rec1[2], rec1[0] / (med1[0] + err1[0])))


def step_completion_trace_report(args):
    """The kernels' own times from the rocprofv3 results database of a traced ``completion_keys`` run."""
    import sqlite3
    files = sorted(glob.glob(os.path.join(args.trace_dir, "**", "*_results.db"), recursive=True))
    if not files:
        sys.exit("no rocprofv3 results database under %s" % args.trace_dir)
    db = sqlite3.connect(files[-1])
    say("    rocprofv3 --kernel-trace --stats (a run of its own), kernel times:")
    for name in ("k_depth_png_keys", "k_completion_median", "k_completion_ratio", "k_completion_errors", "k_completion_finish"):
        n, avg, lo, hi = list(db.execute("select count(*), avg(end-start)/1e3, min(end-start)/1e3, max(end-start)/1e3 from kernels where name like "
                                         "'%%%s%%'" % name))[0]
        if not n:
            sys.exit("%s is not in the trace" % name)
        say("      %-22s %4d launches: avg %8.2f us (min %.2f, max %.2f)" % (name, n, avg, lo, hi))


def drive_completion(args):
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    scratch = tempfile.mkdtemp(prefix="bench_loader_")
    me = "%s %s" % (sys.executable, os.path.abspath(__file__))
    trace_dir = os.path.join(scratch, "trace")
    steps = ["timeout -k 10 240 %s --step completion_keys --iters 30" % me,
             "timeout -k 10 300 rocprofv3 --kernel-trace --stats -d %s -- %s --step completion_keys --iters 10 > /dev/null 2>&1" % (trace_dir, me),
             "%s --step completion_trace_report --trace_dir %s" % (me, trace_dir)]
    cmd = "set -o pipefail; (" + " && ".join(steps) + ") 2>&1 | tee -a %s" % out
    sys.exit(subprocess.call(["bash", "-c", cmd], cwd=ROOT))


def drive_refiner(args):
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    scratch = tempfile.mkdtemp(prefix="bench_loader_")
    me = "%s %s" % (sys.executable, os.path.abspath(__file__))
    last = "$(tail -1 %s | python -c 'import json,sys; print(json.load(sys.stdin)[\"%s\"])')"
    colour_json, gdc_json = os.path.join(scratch, "colour.json"), os.path.join(scratch, "gdc.json")
    trace_dir = os.path.join(scratch, "trace")
    steps = ["timeout -k 10 240 %s --step colour --iters 30 --items %d | tee %s" % (me, GDC_BATCH, colour_json),
             "timeout -k 10 240 %s --step inf_gdc_key --iters 30 | tee %s" % (me, gdc_json),
             "timeout -k 10 300 rocprofv3 --kernel-trace --stats -d %s -- %s --step inf_gdc_key --iters 10 > /dev/null 2>&1" % (trace_dir, me),
             "%s --step gdc_trace_report --trace_dir %s" % (me, trace_dir),
             "timeout -k 10 540 %s --step refiner_trainer --colour_ms %s --gdc_ms %s"
             % (me, last % (colour_json, "colour_ms_per_batch"), last % (gdc_json, "gdc_key_ms_per_batch"))]
    cmd = "set -o pipefail; (" + " && ".join(steps) + ") 2>&1 | grep --line-buffered -v '^{' | tee -a %s" % out
    sys.exit(subprocess.call(["bash", "-c", cmd], cwd=ROOT))


def drive_raw(args):
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    me = "%s %s" % (sys.executable, os.path.abspath(__file__))
    steps = ["timeout -k 10 240 %s --step sparsify --iters 30" % me,
             "timeout -k 10 420 %s --step raw_builder" % me,
             "timeout -k 10 540 %s --step raw_trainer" % me,
             "timeout -k 10 420 %s --step offline" % me]
    cmd = "set -o pipefail; (" + " && ".join(steps) + ") 2>&1 | grep --line-buffered -v '^{' | tee %s" % out
    sys.exit(subprocess.call(["bash", "-c", cmd], cwd=ROOT))


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


# ---------------------------------------------------------------------------------------------------- 14. JPEG outputs on the device
def step_jpeg_enc(args):
    """[14] ``image_codecs.encode_jpeg_batch`` against Pillow's ``save`` on 16 threads, the library call alone against its traffic bound, and
    ``convert_frames`` end to end on a synthetic PNG tree against ``--encoder pil --png_decoder pil``.  The routes alternate inside
    this one run, after a byte comparison; run it twice for the run-to-run spread."""
    import concurrent.futures
    import ctypes
    import io
    import torch
    from PIL import Image
    sys.path.insert(0, ROOT)
    from fusiondepth_amd import _lib, convert_frames, image_codecs
    N, Q, S = 36, 92, "2x2"
    note = say

    frames = [frame(1000 + i) for i in range(N)]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    pool = concurrent.futures.ThreadPoolExecutor(WORKERS)

    def route_device():
        return image_codecs.encode_jpeg_batch(dev, quality=Q, sampling=S, pool=pool)[0]

    def pil_one(a):
        f = io.BytesIO()
        Image.fromarray(a).save(f, "JPEG", quality=Q, subsampling=2)
        return f.getvalue()

    def route_pil():
        host = [d.cpu().numpy() for d in dev]                    # the frames are on the device in both routes: Pillow's pays the download
        return list(pool.map(pil_one, host))

    got, want = route_device(), route_pil()
    assert [bytes(g) for g in got] == want, "the routes disagree"
    total = sum(len(w) for w in want)
    note("[14] JPEG outputs: %d frames of %dx%d, quality %d, %s, textured synthetic content (step 12's); %.0f KB per file; the two routes' "
         "files are equal byte for byte" % (N, W0, H0, Q, S, total / N / 1e3))
    iters = max(3, min(args.iters, 15))
    t = {"device": [], "pil": []}
    for _ in range(iters):
        for name, fn in (("device", route_device), ("pil", route_pil)):
            t0 = time.perf_counter()
            fn()
            t[name].append(1e3 * (time.perf_counter() - t0))
    for name, label in (("device", "encode_jpeg_batch (one library call + two downloads + the headers)"),
                        ("pil", "download + Pillow's save on %d threads" % WORKERS)):
        med = float(np.median(t[name]))
        note("    %-72s %8.1f frames/s, ms per batch of %d: %s  (%d alternating runs)" % (label + ":", 1e3 * N / med, N, _spread(t[name]), iters))

    # the library call alone: the two small uploads, the clear and the seven launches
    table, sizes = image_codecs.jpeg_enc_layout([(W0, H0, 2, 2)] * N)
    for d, x in zip(table, dev):
        d.src = x.data_ptr()
    work = torch.empty((sizes.work_bytes,), dtype=torch.uint8, device="cuda")
    out = torch.empty((sizes.out_bytes,), dtype=torch.uint8, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for k in range(iters + 2):
        ev[0].record()
        _lib.call("fd_jpeg_enc_encode", work.data_ptr(), sizes.work_bytes, ctypes.addressof(table), N, Q, out.data_ptr(), sizes.out_bytes,
                  _lib.stream())
        ev[1].record()
        torch.cuda.synchronize()
        if k >= 2:
            ms.append(ev[0].elapsed_time(ev[1]))
    blocks = sizes.blocks
    traffic = N * 3 * H0 * W0 + 3 * 128 * blocks + 12 * blocks + sizes.raw_bytes + 3 * total
    note("    fd_jpeg_enc_encode alone (clear of %.1f MB of worst-case stream room + seven launches): ms per batch %s; its traffic (pixels once, "
         "coefficients written once and read twice, the clear, the stream written, read and written stuffed) = %.1f MB = %.3f ms at %.1f "
         "TB/s -> %.1fx the bound" % (sizes.raw_bytes / 1e6, _spread(ms), traffic / 1e6, 1e3 * traffic / HBM_BPS, HBM_BPS / 1e12,
                                       float(np.median(ms)) / (1e3 * traffic / HBM_BPS)))

    # convert_frames end to end
    n_tree = 72
    with tempfile.TemporaryDirectory() as root:
        src = os.path.join(root, "png", "2011_09_26", "image_02", "data")
        os.makedirs(src)
        for i in range(n_tree):
            Image.fromarray(frame(2000 + i)).save(os.path.join(src, "%010d.png" % i))
        runs = {"device": [], "pil": []}
        files = {}
        for rep in range(-1, 3):                                 # rep -1: one conversion per route that is not timed (library load, first allocations)
            for enc in ("device", "pil"):
                dst = os.path.join(root, "out_%s_%d" % (enc, rep))
                t0 = time.perf_counter()
                res = convert_frames.convert(os.path.join(root, "png"), dst, encoder=enc, png_decoder=enc, workers=WORKERS)
                if rep >= 0:
                    runs[enc].append(n_tree / (time.perf_counter() - t0))
                assert res["converted"] == n_tree and (res["device"] == n_tree) == (enc == "device"), res
                files[enc] = [open(os.path.join(dst, "2011_09_26", "image_02", "data", "%010d.jpg" % i), "rb").read() for i in range(n_tree)]
            assert files["device"] == files["pil"], "convert_frames: the routes disagree"
        for enc in ("device", "pil"):
            note("    convert_frames --encoder %s --png_decoder %s on %d PNG frames (temporary directory): files/s %s  (3 alternating runs after one "
                 "untimed conversion per route)" % (enc, enc, n_tree, _spread(runs[enc])))
        gain = float(np.median(runs["device"])) / float(np.median(runs["pil"]))
        diff = float(np.median(runs["device"])) - float(np.median(runs["pil"]))
        spread = max(max(v) - min(v) for v in runs.values())
        note("    convert_frames: device over pil = %.2fx by the medians; gain %.1f files/s, larger spread %.1f files/s -> the gain %s the spread"
             % (gain, diff, spread, "EXCEEDS" if diff > spread else "does NOT exceed"))
    note("    NOT measured: a real KITTI tree (real frames compress differently from synthetic content), file-system write time on a real "
         "disk, ImageMagick itself")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="all", choices=["all", "colour", "trace_report", "pil", "pil_worker", "builder", "trainer", "raw", "sparsify",
                                                      "raw_builder", "raw_trainer", "offline", "offline_worker", "refiner", "inf_gdc_key", "gdc_trace_report",
                                                      "refiner_trainer", "completion", "completion_keys", "completion_trace_report", "jpeg", "jpeg_kernels",
                                                      "jpeg_trace_report", "png", "jpeg_enc"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default="")
    ap.add_argument("--split_file", default="")
    ap.add_argument("--worker", type=int, default=0)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--items", type=int, default=12)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--colour_ms", type=float, default=0.0)
    ap.add_argument("--gdc_ms", type=float, default=0.0)
    ap.add_argument("--trace_dir", default="")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", {"raw": "sparsify_time.log", "completion": "completion_time.log"}.get(args.step, "loader_time.log"))
    {"completion": drive_completion, "completion_keys": step_completion_keys, "completion_trace_report": step_completion_trace_report,
     "refiner": drive_refiner, "inf_gdc_key": step_inf_gdc_key, "gdc_trace_report": step_gdc_trace_report,
     "refiner_trainer": step_refiner_trainer, "raw": drive_raw, "sparsify": step_sparsify, "raw_builder": step_raw_builder,
     "raw_trainer": step_raw_trainer, "offline": step_offline, "offline_worker": step_offline_worker, "all": drive, "colour": step_colour,
     "trace_report": step_trace_report, "pil": step_pil, "pil_worker": step_pil_worker, "builder": step_builder,
     "trainer": step_trainer, "jpeg": step_jpeg, "jpeg_kernels": step_jpeg_kernels,
     "jpeg_trace_report": step_jpeg_trace_report, "png": step_png, "jpeg_enc": step_jpeg_enc}[args.step](args)


if __name__ == "__main__":
    main()
