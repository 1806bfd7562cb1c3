"""Host side of ``--resume``: the run-state file beside an epoch checkpoint, its compatibility check and the ``latest`` lookup.

After every epoch checkpoint (``Trainer.train``: every ``save_frequency`` epochs) every rank writes
``models/weights_<epoch>/run_state.rank<k>.pth`` - last, through a temporary name and a rename: the file is the commit marker of
its folder.  It holds what ``adam.pth`` and the network files do not: the counters of the driver loop, the StepLR count, the
loader's epoch counter, both random generators, and the facts a continued run must share with the one that wrote it.  Nothing
here touches a GPU; ``Trainer.save_run_state`` / ``Trainer.resume`` add the device generator's state.
"""
import os
import re

import torch

VERSION = 1
FILE = "run_state.rank%d.pth"
# the options that fix tensor shapes and the data order (the number of training lines joins them in ``fingerprint``)
FINGERPRINT_OPTIONS = ("num_layers", "height", "width", "scales", "frame_ids", "use_stereo", "pose_model_type", "split")
# what must be equal between the run that wrote the file and the run that continues it, in the order it is checked
IDENTITY_FIELDS = ("world_size", "micro_batch", "accumulate_step", "seed")
# optional: the skip counters of the optimiser's guard, written only by a run whose guard is on
GUARD_KEYS = ("skipped_steps", "first_skipped_step", "last_skipped_step")


def _plain(v):
    return list(v) if isinstance(v, (list, tuple)) else v


def fingerprint(opt, train_lines):
    """{field: value} of ``FINGERPRINT_OPTIONS`` + ``train_lines`` (how many lines the training split has)."""
    fp = {k: _plain(getattr(opt, k)) for k in FINGERPRINT_OPTIONS}
    fp["train_lines"] = None if train_lines is None else int(train_lines)
    return fp


def state_path(folder, rank):
    return os.path.join(folder, FILE % rank)


def write_state(state, folder, rank):
    """``torch.save`` under a temporary name, then a rename: a reader never sees half a file."""
    os.makedirs(folder, exist_ok=True)
    path = state_path(folder, rank)
    tmp = path + ".tmp"
    torch.save(dict(state, version=VERSION), tmp)
    os.replace(tmp, path)
    return path


def read_state(folder, rank):
    path = state_path(folder, rank)
    if not os.path.isfile(path):
        raise FileNotFoundError("--resume: %s is missing (the folder is no finished epoch checkpoint of rank %d)" % (path, rank))
    state = torch.load(path, map_location="cpu")
    if state.get("version") != VERSION:
        raise ValueError("--resume: %s has format version %r, this code reads version %d" % (path, state.get("version"), VERSION))
    return state


def check_compatible(saved, current):
    """``ValueError`` naming the first field in which the saved run and the current one differ, with both values.  Both arguments
    carry ``IDENTITY_FIELDS`` and ``fingerprint``."""
    for k in IDENTITY_FIELDS:
        if saved.get(k) != current.get(k):
            raise ValueError("--resume: %s differs: the checkpoint was written with %r, this run has %r" % (k, saved.get(k), current.get(k)))
    for k, now in current["fingerprint"].items():
        was = saved["fingerprint"].get(k)
        if _plain(was) != _plain(now):
            raise ValueError("--resume: %s differs: the checkpoint was written with %r, this run has %r" % (k, was, now))


def is_complete(folder, network_names, world_size):
    """Every network file, ``adam.pth`` and one run-state file per rank."""
    names = ["%s.pth" % n for n in network_names] + ["adam.pth"] + [FILE % k for k in range(world_size)]
    return all(os.path.isfile(os.path.join(folder, n)) for n in names)


def latest(models_dir, network_names, world_size):
    """The highest-numbered complete ``weights_<n>`` under ``models_dir``, or ``FileNotFoundError``."""
    found = []
    if os.path.isdir(models_dir):
        for name in os.listdir(models_dir):
            m = re.fullmatch(r"weights_(\d+)", name)
            if m and is_complete(os.path.join(models_dir, name), network_names, world_size):
                found.append((int(m.group(1)), name))
    if not found:
        raise FileNotFoundError("--resume latest: no weights_<n> under %s holds every network file, adam.pth and the run state of "
                                "%d rank(s)" % (models_dir, world_size))
    return os.path.join(models_dir, max(found)[1])


def resolve(where, log_path, network_names, world_size):
    """``--resume PATH|latest`` -> the folder."""
    if where == "latest":
        return latest(os.path.join(log_path, "models"), network_names, world_size)
    folder = os.path.expanduser(where)
    if not os.path.isdir(folder):
        raise FileNotFoundError("--resume: cannot find the folder %s" % folder)
    return folder


def check_flags(extra, rest):
    """``--resume`` loads every network itself: it is refused beside a weights folder of the command line."""
    if extra.get("resume") is None:
        return
    for flag in ("--train_load_weights_folder", "--load_weights_folder"):
        if any(a == flag or a.startswith(flag + "=") for a in rest):
            raise ValueError("--resume cannot be combined with %s: the checkpoint it continues holds every network" % flag)


def take_flags(found):
    """``--resume``, ``--pretrained_path`` (valued) and ``--shard_val`` (a switch) join ``found`` only where they are given."""
    for name in ("resume", "pretrained_path"):
        if name in found and found[name] is None:
            del found[name]
    if "shard_val" in found and not found["shard_val"]:
        del found["shard_val"]
