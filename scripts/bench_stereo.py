"""The --use_stereo optimiser step on one GPU, ResNet-18, 640x192, --batch_size 12, synthetic scene batches with the stereo partner
"s" resident in HBM: frame_ids [0, -1, 1] (three source frames) and [0] (stereo only).  Two routes of the loss, alternated round by
round inside ONE run so that both see the same machine state:
    fused      the all-scales kernel at one / three source frames (csrc/photometric_ms.hip: fd_photo_ms_fwd / _bwd)
    per-scale  ``tuning.host.photo_ms = False``: four fd_photo_fwd_ex + four fd_photo_bwd_ex launches - the only route these
               configurations had before that kernel took them (a tree from before prints this column only)
Per configuration: the step's wall clock (bracketed by synchronize, like bench.py) per round, and the device time between two
HIP events around the loss path alone - forward + backward on resident inputs, many iterations back to back.  The spread is what
the script itself observes between its rounds; a difference smaller than that is not a difference.
    python scripts/bench_stereo.py [--batch_size 12] [--steps 10] [--warmup 3] [--rounds 5]        (run on the GPU box)"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
from fusiondepth_amd import functional as FD
from fusiondepth_amd import synthetic, tuning
from fusiondepth_amd.options import MonodepthOptions

ap = argparse.ArgumentParser()
ap.add_argument("--batch_size", type=int, default=12)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--loss_iters", type=int, default=200)
ap.add_argument("--height", type=int, default=192)
ap.add_argument("--width", type=int, default=640)
args = ap.parse_args()
HAS_FUSED = FD.photo_ms_supported(FD.PhotoOptions(), 3)          # False on a tree whose all-scales kernel takes two frames only
ROUTES = [("fused", True), ("per-scale", False)] if HAS_FUSED else [("per-scale", False)]


def timed(step, n, w):
    for _ in range(w):
        step()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds_ms": [round(v, 4) for v in ms]}


def loss_alone(tr, inp, fused):
    """Device time of the loss path alone: the arguments ``generate_images_pred`` forms, forward + backward, ``loss_iters`` times."""
    o = tr.opt
    fids = list(o.frame_ids[1:])
    B, _, H, W = inp[("color", 0, 0)].shape
    G = B // tr.batch_size
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    disps = [torch.empty(B, 1, H >> s, W >> s, device="cuda").uniform_(0.03, 0.13, generator=gen).requires_grad_(True) for s in o.scales]
    Ts = []
    for f in fids:
        if f == "s":
            Ts.append(inp["stereo_T"])
        else:
            T = torch.eye(4, device="cuda").repeat(B, 1, 1)
            T[:, 2, 3] = 0.02 if f < 0 else -0.02
            Ts.append(T.requires_grad_(True))
    srcs, target = [inp[("color", f, 0)] for f in fids], inp[("color", 0, 0)]
    ident = torch.cat([FD.reprojection_loss_map(s, target, True) for s in srcs], 1)
    noise = torch.randn((len(o.scales), B, len(fids), H, W), device="cuda", generator=gen)
    K, inv_K, beam, po = inp[("K", 0)], inp[("inv_K", 0)], inp["4beam"], tr.photo_options

    def once():
        if fused:
            photo, si, _ = FD.photo_loss_ms(disps, Ts, K, inv_K, srcs, target, ident, list(noise), beam, list(range(len(disps))), po, G)
        else:
            res = [FD.photo_loss(d, Ts, K, inv_K, srcs, target, ident, noise[s], beam, po, False, G) for s, d in enumerate(disps)]
            photo, si = [r[0] for r in res], [r[1] for r in res]
        total = sum(photo) + sum(si)
        torch.autograd.grad(total, disps + [T for T in Ts if T.requires_grad])

    for _ in range(10):
        once()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(args.loss_iters):
        once()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.loss_iters


def config_line(frame_ids):
    from fusiondepth_amd.trainer import Trainer
    opt = MonodepthOptions().parse(["--num_layers", "18", "--weights_init", "scratch", "--batch_size", str(args.batch_size), "--height",
                                    str(args.height), "--width", str(args.width), "--use_stereo", "--frame_ids"] + [str(f) for f in frame_ids])
    torch.manual_seed(1)
    tr = Trainer(opt, verbose=False)
    fids = list(tr.opt.frame_ids)
    # stereo only has no pose network, and such a step runs its micro-batches one after the other (Trainer.stack_microbatches)
    pool = []
    for i in range(3):
        mbs = [synthetic.make_scene_batch(tr.batch_size, args.height, args.width, frame_ids=fids, seed=4321 + 17 * i + j, clutter=0.5)
               for j in range(tr.accumulate_step)]
        pool.append(tr.stack_micro_batches(mbs) if tr.stack_microbatches else mbs)
    one_pass = pool[0] if tr.stack_microbatches else pool[0][0]          # what one loss launch sees
    k = [0]

    def step():
        k[0] += 1
        return tr.train_step(pool[k[0] % len(pool)])

    steps = {name: [] for name, _ in ROUTES}
    default = tuning.host.photo_ms
    try:
        for r in range(args.rounds):
            for name, on in ROUTES:                              # alternate the routes; only the first round pays the long warm-up
                tuning.host.photo_ms = on
                steps[name].append(1e3 * timed(step, args.steps, args.warmup if r else max(args.warmup, 5)))
        alone = {}
        for r in range(3):
            for name, on in ROUTES:
                alone.setdefault(name, []).append(loss_alone(tr, one_pass, on))
    finally:
        tuning.host.photo_ms = default
    final = {k: float(v.detach()) for k, v in step().items() if torch.is_tensor(v) and v.numel() == 1}
    imgs = tr.batch_size * tr.accumulate_step
    out = {"metric": "--use_stereo optimiser step, frame_ids %s (%d source frame%s), %dx%d, ResNet-18, %d images per step"
                     % (fids, len(fids) - 1, "" if len(fids) == 2 else "s", args.width, args.height, imgs),
           "unit": "ms", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "data": "synthetic", "final_losses": final,
           "passes_per_step": 1 if tr.stack_microbatches else tr.accumulate_step, "images_per_loss_launch": int(one_pass[("color", 0, 0)].shape[0]),
           "step": {name: summary(v) for name, v in steps.items()},
           "loss_path_alone_device": {name: summary(v) for name, v in alone.items()}}
    if HAS_FUSED:
        f, p = out["step"]["fused"], out["step"]["per-scale"]
        spread = max(f["max_ms"] - f["min_ms"], p["max_ms"] - p["min_ms"])
        out["step_gain_ms"] = p["median_ms"] - f["median_ms"]
        out["step_spread_ms"] = spread
        out["fused_is_faster_beyond_spread"] = bool(out["step_gain_ms"] > spread)
        out["images_per_s"] = {"fused": 1e3 * imgs / f["median_ms"], "per-scale": 1e3 * imgs / p["median_ms"]}
    return out


for frame_ids in ([0, -1, 1], [0]):
    print(json.dumps(config_line(frame_ids)), flush=True)
    torch.cuda.empty_cache()
