"""The reference's ``python trainer.py`` as a command: options -> loaders -> ``Trainer.train`` with in-training validation.

    python -m fusiondepth_amd.train [reference flags] [--splits_dir D] [--seed N] [--lidar_source files|raw] [--val_limit N] [--no_val]
                                    [--log_images] [--image_decoder pil|device] [--png_decoder pil|device]
                                    [--png_encoder pil|device] [--resume PATH|latest] [--pretrained_path FILE|DIR] [--shard_val]
                                    [--grad_guard off|skip] [--clip_grad_norm X] [--max_skipped_steps N]
    python -m torch.distributed.run --nproc-per-node 8 -m fusiondepth_amd.train ...          # data parallel, one rank per GPU

  * ``build_loaders(opt, splits_dir, rank, world_size, ...)``  trainer.py:142-174: the training lines of
    ``<splits_dir>/<opt.split>/train_files.txt`` (shuffled, ``drop_last``, this rank's shard: datasets.py, "Rank sharding"), the Eigen
    test lines of ``<splits_dir>/eigen/test_files.txt`` for validation (frame 0 only, ``--eval_batch_size``, in order, nothing
    dropped) and the per-image ground truth of ``<splits_dir>/eigen/gt_depths.npz``.
  * ``main(argv)``  ``dp.init_from_env()``, ``torch.manual_seed(seed)``, ``Trainer(opt, rank=, world_size=)``, the loaders,
    ``trainer.val_gt = ValGroundTruth(gt_depths)`` (validation.py: the fused scorer; about 1.3 GB of device memory for the 697 Eigen
    maps), ``trainer.train(train_loader, val_loader)``; on exit every rank writes ``<log_path>/train_summary.rank<k>.json``.

Ranks.  Every rank trains on its own batches; rank 0 alone validates, logs and saves, as ``Trainer`` always did, and the other ranks
wait for it in the next gradient exchange.  ``--shard_val`` (off by default) shares the validation instead: rank r walks test lines
``r::world_size`` against their own maps, ``Trainer.val_metrics`` gathers the per-image rows of all ranks and puts them back in image
order, so every rank forms the one-rank mean and the same ``best``; rank 0 alone still logs and saves.

Continuing a run.  ``--resume PATH|latest`` loads every network, ``adam.pth`` and this rank's ``run_state.rank<k>.pth`` of an epoch
checkpoint (``Trainer.resume``; ``latest``: the highest-numbered complete ``weights_<n>`` under ``<log_path>/models``) and runs the
remaining epochs; the result is bit for bit the uninterrupted run's (resume.py).  It is refused beside
``--train_load_weights_folder`` / ``--load_weights_folder`` and for a run that differs in ``world_size``, batch sizes, seed or an
option that fixes shapes or the data order.  The summary gains ``"resumed_from"`` (the finished epochs of the checkpoint, or null).

Guarding the optimiser step (off by default).  ``--grad_guard skip``: a step whose gradient holds a NaN or an
inf is not taken - parameters, moments and the Adam step count stay, the gradient is cleared, the batch counts as consumed - instead
of writing NaN into every parameter.  ``--clip_grad_norm X`` scales the gradient by ``min(1, X / (norm + 1e-6))`` first
(``torch.nn.utils.clip_grad_norm_`` over all trained parameters, the norm taken in float64) and turns the guard on by itself;
beside ``--grad_guard off`` it is refused.  The train scalars gain ``grad_norm``, ``grad_norm/<network>``, ``clip_coef``,
``nonfinite`` and the skip counters, the summary ``"grad_guard"``; more than ``--max_skipped_steps N`` (default 10) skipped steps
stop the run with the first and last skipped optimiser step in the message.

``--weights_init pretrained`` reads torchvision's ``resnet{n}-*.pth`` from ``--pretrained_path`` (a file or a directory), then
``$TORCH_HOME/hub/checkpoints``, then ``~/.cache/torch/hub/checkpoints``; it never downloads (networks/resnet_encoder.py).

Deviations from the reference, on purpose
  * the splits folder is an argument (``--splits_dir``, default ``splits``) instead of a folder beside the script, as in
    ``evaluate_depth``; ``--seed`` (default 0) seeds the networks, the epoch order and the per-item draws, so that a run can be
    repeated; ``--lidar_source raw`` sparsifies the Velodyne scans in the loader instead of reading ``{n}beam/`` files;
    ``--image_decoder device`` decodes the JPEG frames on the device (datasets.py, ``decoder=``; same batches bit for bit; with
    ``--png`` it changes nothing); ``--png_decoder device`` does the same for the PNG frames of a ``--png`` tree (``png_decoder=``;
    without ``--png`` it changes nothing).
  * ``--val_limit N`` validates on the first N test lines (the reference validates on all 697 at every log event), ``--no_val``
    not at all.
  * the reference overwrites ``--num_epochs`` with ``(8 * 17) // batch_size`` (trainer.py:28).  So does ``Trainer`` - unless the
    flag is spelled out on this command line, which then holds: a short run must be possible without a batch size of 136.
  * ``--dataset`` other than ``kitti`` is refused: the reference's ``KITTIOdomDataset`` has no LiDAR keys, and nothing here reads the
    odometry layout.
  * no tensorboard / wandb: the scalars go to ``<log_path>/{train,val}/scalars.jsonl`` (``Trainer.log``).  ``--log_images`` adds the
    reference's image summaries (trainer.py:656-681) at every log event: one contact sheet per item, rendered on the device
    (log_images.py), as ``<log_path>/{train,val}/images/{step:07d}_{j}.png``; ``Trainer.image_sink`` takes a tensorboard or wandb
    writer instead.  Rank 0 alone logs, so the switch is set on rank 0 alone.  ``--png_encoder device`` (default ``pil``) encodes
    the sheets on the device (``image_codecs.encode_png_batch``) instead of with PIL on the sink's thread: the default sink then receives
    and writes encoded files, which decode to the same pixels; a sink of your own keeps receiving arrays and tiles; the training
    state is not touched either way.
"""
import json
import os
import sys

import numpy as np
import torch

from . import dp
from . import resume as run_state
from .evaluate_depth import split_off_flags

EXTRA_VALUED = {"splits_dir": "splits", "seed": "0", "lidar_source": "files", "val_limit": None, "image_decoder": None, "png_decoder": None,
                "png_encoder": None, "resume": None, "pretrained_path": None, "grad_guard": None, "clip_grad_norm": None,
                "max_skipped_steps": None}
EXTRA_SWITCHES = ("no_val", "log_images", "shard_val")


def split_off_extra(argv):
    """The flags of this command that ``MonodepthOptions`` does not know, typed -> ({splits_dir, seed, lidar_source, val_limit,
    no_val}, the remaining arguments); ``log_images: True`` joins the dict where ``--log_images`` is given, and only there, and so
    do ``image_decoder``, ``png_decoder`` and ``png_encoder`` ('pil' or 'device'), ``resume`` ('latest' or a folder),
    ``pretrained_path`` and ``shard_val: True``, and ``grad_guard`` / ``clip_grad_norm`` / ``max_skipped_steps`` (``take_guard_flags``).
    ``--resume`` beside a weights folder of the command line is a ``ValueError``."""
    found, rest = split_off_flags(argv, EXTRA_VALUED, EXTRA_SWITCHES)
    if not found["log_images"]:
        del found["log_images"]
    take_image_decoder(found)
    run_state.take_flags(found)
    run_state.check_flags(found, rest)
    take_guard_flags(found)
    found["seed"] = int(found["seed"])
    if found["val_limit"] is not None:
        found["val_limit"] = int(found["val_limit"])
        if found["val_limit"] < 1:
            raise ValueError("--val_limit must be positive (use --no_val to skip validation)")
    if found["lidar_source"] not in ("files", "raw"):
        raise ValueError("--lidar_source must be 'files' or 'raw', got %r" % (found["lidar_source"],))
    return found, rest


def take_image_decoder(found):
    """``--image_decoder pil|device``, ``--png_decoder pil|device`` and ``--png_encoder pil|device``: validated where given, dropped
    from ``found`` where not (the default of each is 'pil')."""
    for name in ("image_decoder", "png_decoder", "png_encoder"):
        if found.get(name) is None:
            found.pop(name, None)
        elif found[name] not in ("pil", "device"):
            raise ValueError("--%s must be 'pil' or 'device', got %r" % (name, found[name]))


def take_guard_flags(found):
    """``--grad_guard off|skip``, ``--clip_grad_norm X`` and ``--max_skipped_steps N``: typed and validated
    where given, dropped from ``found`` where not.  ``--clip_grad_norm X`` with X > 0 sets ``grad_guard`` to 'skip' by itself;
    beside ``--grad_guard off`` it is a ``ValueError``, and so are another mode name, a negative or non-finite X and a negative N -
    all before a GPU is touched."""
    from .optim import check_guard
    for name in ("grad_guard", "clip_grad_norm", "max_skipped_steps"):
        if found.get(name) is None:
            found.pop(name, None)
    if "clip_grad_norm" in found:
        try:
            found["clip_grad_norm"] = float(found["clip_grad_norm"])
        except ValueError:
            raise ValueError("--clip_grad_norm must be a number, got %r" % (found["clip_grad_norm"],)) from None
        if found["clip_grad_norm"] > 0 and "grad_guard" not in found:
            found["grad_guard"] = "skip"
    if "grad_guard" in found or "clip_grad_norm" in found:
        try:
            check_guard(found.get("grad_guard", "off"), found.get("clip_grad_norm", 0.0))
        except ValueError as e:
            raise ValueError("--grad_guard / --clip_grad_norm: %s" % e) from None
    if "max_skipped_steps" in found:
        found["max_skipped_steps"] = int(found["max_skipped_steps"])
        if found["max_skipped_steps"] < 0:
            raise ValueError("--max_skipped_steps must be >= 0, got %d" % found["max_skipped_steps"])


def apply_guard_flags(trainer, extra):
    """The guard flags of the command line -> the attributes ``Trainer.optimizer_step`` reads."""
    for name in ("grad_guard", "clip_grad_norm", "max_skipped_steps"):
        if name in extra:
            setattr(trainer, name, extra[name])


def _read_lines(path):
    with open(path) as fh:
        return [ln for ln in fh.read().splitlines() if ln.strip()]


def decode_workers(num_workers, local_world_size):
    """Threads of one rank's decode pool: ``--num_workers``, but the ranks of one host share 16 CPUs."""
    return max(1, min(int(num_workers), 16 // max(int(local_world_size), 1)))


def build_loaders(opt, splits_dir="splits", rank=0, world_size=1, seed=0, lidar_source="files", val_limit=None, no_val=False,
                  batch_size=None, local_world_size=None, device="cuda", image_decoder="pil", png_decoder="pil", shard_val=False):
    """trainer.py:142-174 -> ``(train_loader, val_loader, gt_depths)``; the last two are None with ``no_val``.  ``batch_size``: the
    per-process micro-batch (``Trainer.batch_size``; default ``opt.batch_size``).  ``local_world_size``: ranks on this host (default
    ``world_size``).  The validation loader walks all of the (limited) test lines unless ``shard_val``: then it and ``gt_depths``
    hold lines ``rank::world_size`` (``shard_val_lines``), for a ``Trainer`` whose ``shard_val`` is set."""
    from .datasets import KITTIRAWBatches, KITTIStereoBatches
    if opt.dataset != "kitti":
        raise NotImplementedError("fusiondepth_amd.train: --dataset %s is not covered (the reference's KITTIOdomDataset has no LiDAR keys, "
                                  "which every network here reads; only the KITTI raw layout is built)" % opt.dataset)
    gt_depths = None
    if not no_val:
        gt_path = os.path.join(splits_dir, "eigen", "gt_depths.npz")
        if not os.path.isfile(gt_path):
            raise FileNotFoundError("%s is missing; fusiondepth_amd.kitti_utils.export_gt_depths(data_path, lines, 'eigen', output_path) "
                                    "writes it from the Velodyne scans of <splits_dir>/eigen/test_files.txt" % gt_path)
    train_lines = _read_lines(os.path.join(splits_dir, opt.split, "train_files.txt"))
    img_ext = ".png" if opt.png else ".jpg"
    frame_ids = list(opt.frame_ids)
    if opt.use_stereo and "s" not in frame_ids:                  # trainer.py:63-64 (Trainer has done it already when it came first)
        frame_ids.append("s")
    builder = KITTIStereoBatches if opt.use_stereo else KITTIRAWBatches
    workers = decode_workers(opt.num_workers, world_size if local_world_size is None else local_world_size)
    common = dict(img_ext=img_ext, opt=opt, seed=seed, device=device, workers=workers, lidar_source=lidar_source, decoder=image_decoder,
                  png_decoder=png_decoder)
    train_loader = builder(opt.data_path, train_lines, opt.height, opt.width, frame_ids, 4, is_train=True,
                           batch_size=opt.batch_size if batch_size is None else batch_size, shuffle=True, drop_last=True, rank=rank,
                           world_size=world_size, **common)
    val_loader = None
    if not no_val:
        val_lines = _read_lines(os.path.join(splits_dir, "eigen", "test_files.txt"))
        gt_depths = list(np.load(gt_path, fix_imports=True, encoding="latin1", allow_pickle=True)["data"])
        if len(gt_depths) != len(val_lines):
            raise ValueError("%s holds %d maps for the %d lines of eigen/test_files.txt" % (gt_path, len(gt_depths), len(val_lines)))
        if val_limit is not None:
            val_lines, gt_depths = val_lines[:val_limit], gt_depths[:val_limit]
        if shard_val:
            val_lines, gt_depths = shard_val_lines(val_lines, gt_depths, rank, world_size)
        val_loader = builder(opt.data_path, val_lines, opt.height, opt.width, [0], 4, is_train=False, batch_size=opt.eval_batch_size,
                             shuffle=False, drop_last=False, **common)
    return train_loader, val_loader, gt_depths


def shard_val_lines(val_lines, gt_depths, rank, world_size):
    """``--shard_val``: rank r validates lines ``r::world_size`` against their own maps (the shares differ by at most one)."""
    if len(val_lines) < world_size:
        raise ValueError("--shard_val: %d validation lines cannot be shared among %d ranks" % (len(val_lines), world_size))
    return val_lines[rank::world_size], gt_depths[rank::world_size]


def start_epoch_of(trainer, extra, train_loader):
    """``--resume PATH|latest`` -> ``Trainer.resume`` of that folder -> the epoch ``Trainer.train`` starts at (0 without the flag)."""
    if extra.get("resume") is None:
        return 0
    folder = run_state.resolve(extra["resume"], trainer.log_path, list(trainer.models), trainer.world_size)
    return trainer.resume(folder, train_loader)


def param_checksum(trainer):
    """[sum, sum of magnitudes] of the flat parameter buffer in float64: the form ``bench.py`` prints."""
    flat64 = trainer.flat.flat_param.double()
    return [float(flat64.sum()), float(flat64.abs().sum())]


def write_summary(trainer, train_loader, rank, loss_scale=None):
    """``<log_path>/train_summary.rank<k>.json``: what this rank did.  ``loss_scale``: what turns the latest step's ``loss`` into the
    value the log prints (default ``1 / accumulate_step``: ``Trainer.train_step`` sums over its stacked micro-batches)."""
    last = trainer.last_losses
    scale = 1.0 / trainer.accumulate_step if loss_scale is None else loss_scale
    loss = float(last["loss"]) * scale if last is not None else None
    res = {"rank": rank, "world_size": trainer.world_size, "steps": trainer.step, "epochs": len(train_loader.served),
           "batches_per_epoch": len(train_loader), "batch_size": train_loader.batch_size, "last_loss": loss,
           "param_checksum": param_checksum(trainer), "best": float(trainer.best), "resumed_from": trainer.resumed_from,
           "grad_guard": trainer.guard_summary(),
           "items": [order for _, order in train_loader.served]}
    os.makedirs(trainer.log_path, exist_ok=True)
    path = os.path.join(trainer.log_path, "train_summary.rank%d.json" % rank)
    with open(path, "w") as f:
        json.dump(res, f)
    return path


def main(argv=None):
    from .options import MonodepthOptions
    from .trainer import Trainer
    rank, world, _ = dp.init_from_env()
    extra, rest = split_off_extra(sys.argv[1:] if argv is None else argv)
    opt = MonodepthOptions().parse(rest)
    epochs_given = opt.num_epochs if any(a == "--num_epochs" or a.startswith("--num_epochs=") for a in rest) else None
    if extra.get("pretrained_path"):                             # where --weights_init pretrained looks first (resnet_encoder.py)
        opt.pretrained_path = extra["pretrained_path"]
    torch.manual_seed(extra["seed"])
    trainer = Trainer(opt, rank=rank, world_size=world)
    trainer.shard_val = bool(extra.get("shard_val")) and world > 1
    apply_guard_flags(trainer, extra)
    if epochs_given is not None:
        trainer.opt.num_epochs = epochs_given
    if extra.get("log_images") and rank == 0:                    # the other ranks do not log
        trainer.log_images = True
    if extra.get("png_encoder") == "device":                     # the sheets of --log_images, encoded on the device
        trainer.png_encoder = "device"
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    train_loader, val_loader, gt_depths = build_loaders(opt, extra["splits_dir"], rank, world, seed=extra["seed"],
                                                        lidar_source=extra["lidar_source"], val_limit=extra["val_limit"],
                                                        no_val=extra["no_val"] or (rank != 0 and not trainer.shard_val),
                                                        batch_size=trainer.batch_size, local_world_size=local_world,
                                                        device=trainer.device, image_decoder=extra.get("image_decoder", "pil"),
                                                        png_decoder=extra.get("png_decoder", "pil"), shard_val=trainer.shard_val)
    if val_loader is not None:
        from .validation import ValGroundTruth
        trainer.val_gt = ValGroundTruth(gt_depths, device=trainer.device)
    try:
        trainer.train(train_loader, val_loader, start_epoch=start_epoch_of(trainer, extra, train_loader))
        write_summary(trainer, train_loader, rank)
    finally:
        trainer.close()
        train_loader.close()
        if val_loader is not None:
            val_loader.close()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return trainer


if __name__ == "__main__":
    main()
