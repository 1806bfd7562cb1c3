"""The reference's ``python completor.py`` as a command: options -> loaders -> ``Completor.train`` with in-training validation.

    python -m fusiondepth_amd.complete [reference flags] [--seed N] [--val_limit N] [--no_val] [--val_route fused|per_batch]
                                       [--image_decoder pil|device] [--png_decoder pil|device] [--resume PATH|latest]
                                       [--pretrained_path FILE|DIR] [--grad_guard off|skip] [--clip_grad_norm X]
                                       [--max_skipped_steps N]          (the guard flags: fusiondepth_amd/train.py)
    python -m torch.distributed.run --nproc-per-node 8 -m fusiondepth_amd.complete ...       # data parallel, one rank per GPU

  * ``build_loaders(opt, rank, world_size, ...)``  completor.py:132-152: both loaders are ``KITTICompletionBatches`` over
    ``<data_path>/completion`` (the tree ``evaluate_completion`` reads).  Training: ``opt.frame_ids``, ``--batch_size``, shuffled,
    ``drop_last``, this rank's shard.  Validation: ``--completion_val_split`` (the 1000 images of ``val_selection_cropped`` by
    default), frame 0 only, ``--eval_batch_size``, in order, nothing dropped.
  * ``main(argv)``  ``dp.init_from_env()``, ``torch.manual_seed(seed)``, ``Completor(opt, rank=, world_size=)``, the loaders,
    ``completor.val_scorer = CompletionValScorer(...)`` (validation.py: the fused scorer, device memory bounded by its chunk of 64
    images) unless ``--val_route per_batch``, ``completor.train(train_loader, val_loader)``; on exit every rank writes
    ``<log_path>/train_summary.rank<k>.json`` with ``train.py``'s fields - ``best`` is the best ``de/rms`` in millimetres.

Ranks.  Every rank trains on its own batches; rank 0 alone validates, logs and saves (``weights_rms<N>``, ``Completor.val``), and
the other ranks wait for it in the next gradient exchange.  Validation is not sharded.

Deviations from the reference, on purpose
  * ``--seed`` (default 0) seeds the networks, the epoch order and the per-item draws; ``--val_limit N`` validates on the first N
    validation files (the reference validates on the whole split at every log event), ``--no_val`` not at all.
  * the reference always loads ``--load_weights_folder`` (completor.py:125-126, 850-880: ``models_to_load``, the two LiDAR encoders
    and ``adam.pth``), whose default is a path on its author's machine.  Here the folder is loaded - through ``Trainer.load_model``,
    the ``--train_load_weights_folder`` path - only when the flag is spelled out on the command line; without it the networks start
    from ``--weights_init``.
  * ``--val_route``: ``fused`` scores every image on its own with ``fd_completion_val_scores`` and downloads once per validation,
    ``per_batch`` is ``Completor.compute_depth_losses`` per batch (seven downloads each).  At ``--eval_batch_size 1``, the reference's
    default, both are the reference's mean over batches; at a larger batch the fused route still averages per image.
  * ``--dataset`` is not read: the completion tree has one layout.  ``--completion_amp`` is not covered.
  * no tensorboard / wandb: the scalars go to ``<log_path>/{train,val}/scalars.jsonl`` (``Trainer.log``).
  * ``--resume PATH|latest`` continues a run from an epoch checkpoint and ``--pretrained_path`` names torchvision's ImageNet file for
    ``--weights_init pretrained``, both as in ``train.py``; ``--shard_val`` is not offered here (the scorer's chunks are rank 0's).
"""
import os
import sys

import torch

from . import dp
from .evaluate_completion import canvas_size
from .evaluate_depth import split_off_flags
from . import resume as run_state
from .train import apply_guard_flags, decode_workers, start_epoch_of, take_guard_flags, take_image_decoder, write_summary

DEFAULT_VAL_ROUTE = "fused"            # decided by profiles/completion_val_time.log
EXTRA_VALUED = {"seed": "0", "val_limit": None, "val_route": DEFAULT_VAL_ROUTE, "image_decoder": None, "png_decoder": None,
                "resume": None, "pretrained_path": None, "grad_guard": None, "clip_grad_norm": None, "max_skipped_steps": None}
EXTRA_SWITCHES = ("no_val",)


def split_off_extra(argv):
    """The flags of this command that ``MonodepthOptions`` does not know, typed -> ({seed, val_limit, val_route, no_val,
    load_weights_given}, the remaining arguments).  ``load_weights_given``: ``--load_weights_folder`` is spelled out in ``argv`` (it
    stays among the remaining arguments).  ``image_decoder`` ('pil' or 'device') joins the dict only where ``--image_decoder`` is
    given; the completion tree's colour frames are PNG files, so both values decode with Pillow.  ``png_decoder`` likewise joins only
    where ``--png_decoder`` is given: 'device' unfilters the 16-bit depth PNGs of every batch on the device (the colour frames, whose
    crop, pad and mirror run on the host threads, stay with Pillow)."""
    found, rest = split_off_flags(argv, EXTRA_VALUED, EXTRA_SWITCHES)
    take_image_decoder(found)
    run_state.take_flags(found)
    run_state.check_flags(found, rest)
    take_guard_flags(found)
    found["seed"] = int(found["seed"])
    if found["val_limit"] is not None:
        found["val_limit"] = int(found["val_limit"])
        if found["val_limit"] < 1:
            raise ValueError("--val_limit must be positive (use --no_val to skip validation)")
    if found["val_route"] not in ("fused", "per_batch"):
        raise ValueError("--val_route must be 'fused' or 'per_batch', got %r" % (found["val_route"],))
    found["load_weights_given"] = any(a == "--load_weights_folder" or a.startswith("--load_weights_folder=") for a in rest)
    return found, rest


def build_loaders(opt, rank=0, world_size=1, seed=0, val_limit=None, no_val=False, local_world_size=None, device="cuda",
                  image_decoder="pil", png_decoder="pil"):
    """completor.py:132-152 -> ``(train_loader, val_loader)``; the second is None with ``no_val``.  ``opt`` should be the
    ``Completor``'s own options (its constructor sets the full-resolution size).  The validation loader is never sharded."""
    from .completion_data import KITTICompletionBatches
    tree = os.path.join(opt.data_path, "completion")
    workers = decode_workers(opt.num_workers, world_size if local_world_size is None else local_world_size)
    common = dict(val_split=opt.completion_val_split, opt=opt, seed=seed, device=device, workers=workers, decoder=image_decoder,
                  png_decoder=png_decoder)
    train_loader = KITTICompletionBatches(tree, opt.height, opt.width, list(opt.frame_ids), 4, is_train=True, batch_size=opt.batch_size,
                                          shuffle=True, drop_last=True, rank=rank, world_size=world_size, **common)
    val_loader = None
    if not no_val:
        val_loader = KITTICompletionBatches(tree, opt.height, opt.width, [0], 4, is_train=False, batch_size=opt.eval_batch_size,
                                            shuffle=False, drop_last=False, **common)
        if val_limit is not None:
            val_loader.filenames = val_loader.filenames[:val_limit]      # the sorted paths: the first N files
    return train_loader, val_loader


def val_scorer_for(opt, val_loader, device="cuda"):
    """The resident ``CompletionValScorer`` of ``val_loader``'s images for a ``Completor`` with options ``opt``."""
    from .validation import CompletionValScorer
    return CompletionValScorer(len(val_loader.filenames), canvas_size(opt), (opt.height, opt.width),
                               eigen_crop=bool(opt.completion_eigen_crop), device=device)


def main(argv=None):
    from .completor import Completor
    from .options import MonodepthOptions
    rank, world, _ = dp.init_from_env()
    extra, rest = split_off_extra(sys.argv[1:] if argv is None else argv)
    opt = MonodepthOptions().parse(rest)
    if opt.completion_amp:
        raise NotImplementedError("fusiondepth_amd.complete: --completion_amp is not covered")
    if extra["load_weights_given"]:
        opt.train_load_weights_folder = opt.load_weights_folder
    if extra.get("pretrained_path"):
        opt.pretrained_path = extra["pretrained_path"]
    torch.manual_seed(extra["seed"])
    completor = Completor(opt, rank=rank, world_size=world)
    apply_guard_flags(completor, extra)
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    train_loader, val_loader = build_loaders(completor.opt, rank, world, seed=extra["seed"], val_limit=extra["val_limit"],
                                             no_val=extra["no_val"] or rank != 0, local_world_size=local_world, device=completor.device,
                                             image_decoder=extra.get("image_decoder", "pil"),
                                             png_decoder=extra.get("png_decoder", "pil"))
    if val_loader is not None and extra["val_route"] == "fused":
        completor.val_scorer = val_scorer_for(completor.opt, val_loader, completor.device)
    try:
        completor.train(train_loader, val_loader, start_epoch=start_epoch_of(completor, extra, train_loader))
        write_summary(completor, train_loader, rank)
    finally:
        train_loader.close()
        if val_loader is not None:
            val_loader.close()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return completor


if __name__ == "__main__":
    main()
