"""Host side of ``--resume``: the ``latest`` lookup, the compatibility check, ``KITTIRAWBatches.set_epoch``, the run-state file and the
flags of the three commands.  No GPU is touched: the device generator's state, the one part that needs one, is left out of the round
trip here and covered by tests/test_gpu_resume.py."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

NETWORKS = ["encoder", "depth", "pose"]


def _folder(models, n, networks=NETWORKS, adam=True, ranks=(0, 1)):
    from fusiondepth_amd import resume as RS
    folder = os.path.join(str(models), "weights_%s" % n)
    os.makedirs(folder)
    for name in networks:
        open(os.path.join(folder, name + ".pth"), "wb").close()
    if adam:
        open(os.path.join(folder, "adam.pth"), "wb").close()
    for k in ranks:
        open(RS.state_path(folder, k), "wb").close()
    return folder


# --------------------------------------------------------------------------------------------- latest
def test_latest_skips_what_is_not_a_finished_checkpoint(tmp_path):
    from fusiondepth_amd import resume as RS
    models = tmp_path / "log" / "models"
    with pytest.raises(FileNotFoundError, match="no weights_<n>"):
        RS.latest(str(models), NETWORKS, 2)                      # no folder at all
    good = _folder(models, 1)
    _folder(models, 2, networks=NETWORKS[:2])                    # a network file is missing
    _folder(models, 3, ranks=(0,))                               # rank 1 never committed
    _folder(models, 4, adam=False)
    _folder(models, "best")                                      # model exports carry no number
    _folder(models, "absrel71")
    assert RS.latest(str(models), NETWORKS, 2) == good
    assert RS.latest(str(models), NETWORKS, 1) == os.path.join(str(models), "weights_3")       # one rank needs rank 0's marker alone
    ten = _folder(models, 10)
    assert RS.latest(str(models), NETWORKS, 2) == ten            # by number, not by name: 10 > 4 > 3
    assert RS.resolve("latest", str(tmp_path / "log"), NETWORKS, 2) == ten
    assert RS.resolve(good, str(tmp_path / "log"), NETWORKS, 2) == good
    with pytest.raises(FileNotFoundError, match="cannot find the folder"):
        RS.resolve(str(models / "weights_77"), str(tmp_path / "log"), NETWORKS, 2)


# --------------------------------------------------------------------------------------------- compatibility
def _opt(**over):
    base = dict(num_layers=18, height=192, width=640, scales=[0, 1, 2, 3], frame_ids=[0, -1, 1], use_stereo=False,
                pose_model_type="separate_resnet", split="eigen_zhou")
    base.update(over)
    return SimpleNamespace(**base)


def _identity(lines=40, **over):
    from fusiondepth_amd import resume as RS
    ident = {"world_size": 2, "micro_batch": 6, "accumulate_step": 1, "seed": 0}
    opt = {k: over.pop(k) for k in list(over) if k not in ident}
    ident.update(over)
    ident["fingerprint"] = RS.fingerprint(_opt(**opt), lines)
    return ident


def test_every_mismatch_raises_and_names_its_field():
    from fusiondepth_amd import resume as RS
    assert set(RS.fingerprint(_opt(), 40)) == set(RS.FINGERPRINT_OPTIONS) | {"train_lines"}
    assert set(RS.FINGERPRINT_OPTIONS) == {"num_layers", "height", "width", "scales", "frame_ids", "use_stereo", "pose_model_type", "split"}
    RS.check_compatible(_identity(), _identity())
    RS.check_compatible(_identity(scales=(0, 1, 2, 3)), _identity())     # a tuple in the file is the list of the options
    changed = dict(world_size=1, micro_batch=3, accumulate_step=2, seed=4, num_layers=50, height=320, width=1024, scales=[0, 1],
                   frame_ids=[0, -1, 1, "s"], use_stereo=True, pose_model_type="shared", split="eigen_full")
    for field, value in changed.items():
        with pytest.raises(ValueError) as e:
            RS.check_compatible(_identity(), _identity(**{field: value}))
        assert field in str(e.value) and repr(value) in str(e.value) and repr(_identity().get(field, getattr(_opt(), field, None))) in str(e.value)
    with pytest.raises(ValueError, match="train_lines.*40.*41"):
        RS.check_compatible(_identity(), _identity(lines=41))


# --------------------------------------------------------------------------------------------- the loader's epoch counter
def _loader(cls=None, **kw):
    from fusiondepth_amd.datasets import KITTIRAWBatches
    lines = ["2011_09_26/2011_09_26_drive_0001_sync %d l" % i for i in range(11)]
    ld = (cls or KITTIRAWBatches)("/nowhere", lines, 64, 96, [0, -1, 1], 4, is_train=True, opt=None, batch_size=2, shuffle=True, seed=7,
                                  device="cpu", prefetch=False, **kw)
    ld._start_host = lambda epoch, indices: (epoch, list(indices))       # no files, no device: the order is what is under test
    ld._finish_batch = lambda items: items
    return ld


def test_set_epoch_serves_that_epochs_order():
    from fusiondepth_amd.datasets import KITTIRefinerBatches, KITTIStereoBatches
    ld = _loader()
    assert [b for b in ld] and ld.served == [(0, ld.epoch_order(0))]
    ld.set_epoch(5)
    batches = list(ld)
    assert ld.served[-1] == (5, ld.epoch_order(5)) and ld.epoch_order(5) != ld.epoch_order(1)
    assert [i for _, idx in batches for i in idx] == ld.epoch_order(5) and all(e == 5 for e, _ in batches)       # the draws' epoch too
    list(ld)
    assert ld.served[-1] == (6, ld.epoch_order(6))               # and counts on from there
    assert ld.epoch_order(5) == [int(i) for i in np.random.default_rng([7, 5]).permutation(11)[:10]]
    for cls in (KITTIStereoBatches, KITTIRefinerBatches):        # inherited by every builder
        sub = _loader(cls, rank=1, world_size=2)
        sub.set_epoch(3)
        list(sub)
        assert sub.served == [(3, sub.epoch_order(3))]
    with pytest.raises(ValueError, match="negative"):
        ld.set_epoch(-1)


def test_set_epoch_is_refused_while_an_iteration_is_open():
    ld = _loader()
    it = iter(ld)
    ld.set_epoch(2)                                              # nothing is open before the first batch is asked for
    next(it)
    with pytest.raises(RuntimeError, match="iteration is open"):
        ld.set_epoch(4)
    assert ld.served == [(2, ld.epoch_order(2))]
    for _ in it:
        pass
    ld.set_epoch(4)                                              # exhausted
    it = iter(ld)
    next(it)
    it.close()                                                   # dropped
    ld.set_epoch(0)
    assert [e for e, _ in ld.served] == [2, 4]


# --------------------------------------------------------------------------------------------- the file
def test_run_state_round_trip(tmp_path):
    from fusiondepth_amd import resume as RS
    torch.manual_seed(123)
    torch.rand(5)
    state = dict(_identity(), rank=1, epochs_done=2, step=34, batch_idx=34, best=0.07421875, scheduler_epochs=2, loader_epoch=2,
                 torch_rng=torch.get_rng_state(), cuda_rng=None)
    want = torch.rand(7)
    folder = str(tmp_path / "weights_1")
    path = RS.write_state(state, folder, 1)
    assert path == RS.state_path(folder, 1) == os.path.join(folder, "run_state.rank1.pth")
    assert os.listdir(folder) == ["run_state.rank1.pth"]         # the temporary name is gone
    back = RS.read_state(folder, 1)
    assert back["version"] == RS.VERSION == 1
    for k, v in state.items():
        if k != "torch_rng":
            assert back[k] == v and type(back[k]) is type(v), k
    RS.check_compatible(back, _identity())
    torch.manual_seed(9)
    torch.set_rng_state(back["torch_rng"])
    assert torch.equal(torch.rand(7), want)                      # the host generator goes on where it was
    with pytest.raises(FileNotFoundError, match="run_state.rank0.pth"):
        RS.read_state(folder, 0)
    torch.save(dict(state, version=99), RS.state_path(folder, 1))
    with pytest.raises(ValueError, match="version 99"):
        RS.read_state(folder, 1)


# --------------------------------------------------------------------------------------------- the flags
def test_flags_of_the_three_commands():
    from fusiondepth_amd import complete as C, refine as R, train as T
    from fusiondepth_amd.options import MonodepthOptions
    assert R.split_off_extra is T.split_off_extra
    for mod in (T, R, C):                                        # train, refine and complete accept the flag
        assert "resume" not in mod.split_off_extra([])[0]
        extra, rest = mod.split_off_extra(["--png", "--resume", "latest", "--seed", "3"])
        assert extra["resume"] == "latest" and rest == ["--png"]
        assert mod.split_off_extra(["--resume=/log/m/models/weights_4"])[0]["resume"] == "/log/m/models/weights_4"
        with pytest.raises(ValueError, match="needs a value"):
            mod.split_off_extra(["--resume"])
        for other in (["--train_load_weights_folder", "/w"], ["--load_weights_folder=/w"]):
            with pytest.raises(ValueError, match="--resume cannot be combined with --(train_)?load_weights_folder"):
                mod.split_off_extra(["--resume", "latest"] + other)
            mod.split_off_extra(other)                           # fine without --resume
        assert mod.split_off_extra(["--pretrained_path", "/hub"])[0]["pretrained_path"] == "/hub"
    assert T.split_off_extra(["--shard_val"])[0]["shard_val"] is True and "shard_val" not in T.split_off_extra([])[0]
    assert C.split_off_extra(["--shard_val"])[1] == ["--shard_val"]      # complete's scorer is not sharded: the flag is not its own
    with pytest.raises(SystemExit):                              # the options surface stays the reference's
        MonodepthOptions().parse(["--resume", "latest"])
    with pytest.raises(ValueError, match="cannot be shared among 3 ranks"):
        T.shard_val_lines(["a", "b"], [0, 1], 0, 3)
    assert T.shard_val_lines(list("abcde"), [0, 1, 2, 3, 4], 1, 2) == (["b", "d"], [1, 3])
    assert T.shard_val_lines(list("abcde"), [0, 1, 2, 3, 4], 0, 2) == (["a", "c", "e"], [0, 2, 4])
