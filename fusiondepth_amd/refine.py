"""The reference's ``python refiner.py`` as a command: options -> loaders -> ``Refiner.train`` with in-training validation.

    python -m fusiondepth_amd.refine [reference flags] [--splits_dir D] [--seed N] [--lidar_source files|raw] [--val_limit N] [--no_val]
                                     [--image_decoder pil|device] [--png_decoder pil|device] [--resume PATH|latest] [--shard_val]
                                     [--grad_guard off|skip] [--clip_grad_norm X] [--max_skipped_steps N]   (fusiondepth_amd/train.py)
    python -m torch.distributed.run --nproc-per-node 8 -m fusiondepth_amd.refine ...         # data parallel, one rank per GPU

  * ``build_loaders(opt, splits_dir, rank, world_size, ...)``  refiner.py:168-200: the training lines of
    ``<splits_dir>/<opt.split>/train_files.txt`` through ``KITTIRefinerBatches`` (shuffled, ``drop_last``, this rank's shard), the
    Eigen test lines of ``<splits_dir>/eigen/test_files.txt`` for validation (frame 0 only, ``--eval_batch_size``, in order, nothing
    dropped) and the per-image ground truth of ``<splits_dir>/eigen/gt_depths.npz``.
  * ``main(argv)``  ``dp.init_from_env()``, ``torch.manual_seed(seed)``, ``Refiner(opt, rank=, world_size=)`` (which reads
    ``--refine_load_weights_folder``), the loaders (which read the ``inf_gdc`` maps ``python -m fusiondepth_amd.inf_gdc`` wrote),
    ``refiner.val_gt = ValGroundTruth(gt_depths)``, ``refiner.train(train_loader, val_loader)``; on exit every rank writes
    ``<log_path>/train_summary.rank<k>.json`` with ``train.py``'s fields.

The Refiner's validation rule is the trainer's (``Trainer.val_metrics`` / ``Trainer.val``), so the ranks, the fused scorer and the
checkpoint names (``weights_best``, ``weights_absrel<N>``) are ``train.py``'s; so are the deviations from the reference listed there:
``--splits_dir``, ``--seed``, ``--lidar_source``, ``--val_limit``, ``--no_val``, a ``--num_epochs`` spelled out on the command line
wins over the derived ``(8 * 17) // batch_size``, ``--dataset`` other than ``kitti`` is refused, scalars go to
``<log_path>/{train,val}/scalars.jsonl``.  ``--resume`` and ``--shard_val`` are ``train.py``'s too: a continued run loads every network
of the epoch checkpoint, the frozen ones included, and ends on the bits of the uninterrupted run.
"""
import os
import sys

import numpy as np
import torch

from . import dp
from .train import _read_lines, apply_guard_flags, decode_workers, shard_val_lines, split_off_extra, start_epoch_of, write_summary


def build_loaders(opt, splits_dir="splits", rank=0, world_size=1, seed=0, lidar_source="files", val_limit=None, no_val=False,
                  batch_size=None, local_world_size=None, device="cuda", image_decoder="pil", png_decoder="pil", shard_val=False):
    """refiner.py:168-200 -> ``(train_loader, val_loader, gt_depths)``; the last two are None with ``no_val``.  The arguments are
    ``train.build_loaders``'.  ``opt`` should be the ``Refiner``'s own options (its constructor sets ``clone_gdc``, which makes the
    training loader add ``inf_gdc``)."""
    from .datasets import KITTIRefinerBatches
    if opt.dataset != "kitti":
        raise NotImplementedError("fusiondepth_amd.refine: --dataset %s is not covered (the reference's KITTIOdomDataset has no LiDAR keys, "
                                  "which every network here reads; only the KITTI raw layout is built)" % opt.dataset)
    gt_depths = None
    if not no_val:
        gt_path = os.path.join(splits_dir, "eigen", "gt_depths.npz")
        if not os.path.isfile(gt_path):
            raise FileNotFoundError("%s is missing; fusiondepth_amd.kitti_utils.export_gt_depths(data_path, lines, 'eigen', output_path) "
                                    "writes it from the Velodyne scans of <splits_dir>/eigen/test_files.txt" % gt_path)
    train_lines = _read_lines(os.path.join(splits_dir, opt.split, "train_files.txt"))
    workers = decode_workers(opt.num_workers, world_size if local_world_size is None else local_world_size)
    common = dict(img_ext=".png" if opt.png else ".jpg", opt=opt, seed=seed, device=device, workers=workers, lidar_source=lidar_source,
                  decoder=image_decoder, png_decoder=png_decoder)
    train_loader = KITTIRefinerBatches(opt.data_path, train_lines, opt.height, opt.width, list(opt.frame_ids), 4, is_train=True,
                                       batch_size=opt.batch_size if batch_size is None else batch_size, shuffle=True, drop_last=True,
                                       rank=rank, world_size=world_size, **common)
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
        val_loader = KITTIRefinerBatches(opt.data_path, val_lines, opt.height, opt.width, [0], 4, is_train=False,
                                         batch_size=opt.eval_batch_size, shuffle=False, drop_last=False, **common)
    return train_loader, val_loader, gt_depths


def main(argv=None):
    from .options import MonodepthOptions
    from .refiner import Refiner
    rank, world, _ = dp.init_from_env()
    extra, rest = split_off_extra(sys.argv[1:] if argv is None else argv)
    opt = MonodepthOptions().parse(rest)
    epochs_given = opt.num_epochs if any(a == "--num_epochs" or a.startswith("--num_epochs=") for a in rest) else None
    torch.manual_seed(extra["seed"])
    refiner = Refiner(opt, rank=rank, world_size=world)
    refiner.shard_val = bool(extra.get("shard_val")) and world > 1
    apply_guard_flags(refiner, extra)
    if epochs_given is not None:
        refiner.opt.num_epochs = epochs_given
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    train_loader, val_loader, gt_depths = build_loaders(refiner.opt, extra["splits_dir"], rank, world, seed=extra["seed"],
                                                        lidar_source=extra["lidar_source"], val_limit=extra["val_limit"],
                                                        no_val=extra["no_val"] or (rank != 0 and not refiner.shard_val),
                                                        batch_size=refiner.batch_size, local_world_size=local_world,
                                                        device=refiner.device, image_decoder=extra.get("image_decoder", "pil"),
                                                        png_decoder=extra.get("png_decoder", "pil"), shard_val=refiner.shard_val)
    if val_loader is not None:
        from .validation import ValGroundTruth
        refiner.val_gt = ValGroundTruth(gt_depths, device=refiner.device)
    try:
        refiner.train(train_loader, val_loader, start_epoch=start_epoch_of(refiner, extra, train_loader))
        write_summary(refiner, train_loader, rank, loss_scale=1.0)     # the Refiner never accumulates (refiner.py:272-278)
    finally:
        train_loader.close()
        if val_loader is not None:
            val_loader.close()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return refiner


if __name__ == "__main__":
    main()
