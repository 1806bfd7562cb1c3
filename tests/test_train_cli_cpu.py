"""Host side of ``python -m fusiondepth_amd.train``: rank sharding of the KITTI loaders, ``build_loaders``, the extra flags, and the
numpy restatement of the training-time metrics (tests/val_ref.py) pinned to the reference's own torch expression.  No GPU is touched."""
import os

import numpy as np
import pytest

import val_ref

N_LINES, BATCH = 53, 2


def _opt(*flags):
    from fusiondepth_amd.options import MonodepthOptions
    return MonodepthOptions().parse(list(flags))


def _lines(n=N_LINES):
    return ["2011_09_26/2011_09_26_drive_0001_sync %d l" % i for i in range(n)]


def _loader(cls=None, **kw):
    from fusiondepth_amd.datasets import KITTIRAWBatches
    kw.setdefault("batch_size", BATCH)
    kw.setdefault("shuffle", True)
    kw.setdefault("seed", 11)
    return (cls or KITTIRAWBatches)("/nowhere", _lines(), 64, 96, [0, -1, 1], 4, is_train=True, opt=None, **kw)


def _batches(order, B=BATCH):
    return [tuple(order[i:i + B]) for i in range(0, len(order), B)]


# --------------------------------------------------------------------------------------------- sharding
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_ranks_take_disjoint_equal_shares_of_the_global_batches(world):
    whole = _loader()
    for epoch in (0, 3):
        perm = [int(i) for i in np.random.default_rng([11, epoch]).permutation(N_LINES)]
        global_batches = _batches(perm)[:(N_LINES // (BATCH * world)) * world]
        shares = []
        for rank in range(world):
            ld = _loader(rank=rank, world_size=world)
            assert len(ld) == N_LINES // (BATCH * world)
            mine = _batches(ld.epoch_order(epoch))
            assert len(mine) == len(ld)
            assert mine == global_batches[rank::world]           # global batch k goes to rank k % world
            shares.append(mine)
        flat = [b for s in shares for b in s]
        assert len(set(flat)) == len(flat) and set(flat) == set(global_batches)
        items = [i for b in flat for i in b]
        assert len(set(items)) == len(items)
        if world == 1:
            assert shares[0] == _batches(whole.epoch_order(epoch))


def test_defaults_keep_the_epoch_order():
    """rank / world_size omitted: the order of the parent commit, restated - permutation(n) cut to whole batches."""
    for shuffle in (True, False):
        for drop_last in (True, False):
            ld = _loader(shuffle=shuffle, drop_last=drop_last, seed=5)
            assert (ld.rank, ld.world_size) == (0, 1)
            for epoch in (0, 1, 7):
                order = np.random.default_rng([5, epoch]).permutation(N_LINES) if shuffle else np.arange(N_LINES)
                want = [int(i) for i in order[:(N_LINES // BATCH) * BATCH if drop_last else N_LINES]]
                assert ld.epoch_order(epoch) == want
            assert len(ld) == (N_LINES // BATCH if drop_last else (N_LINES + BATCH - 1) // BATCH)


def test_sharding_refuses_a_partial_batch_and_a_bad_rank():
    with pytest.raises(ValueError, match="drop_last"):
        _loader(rank=0, world_size=2, drop_last=False)
    with pytest.raises(ValueError, match="rank"):
        _loader(rank=2, world_size=2)


def test_item_draws_do_not_depend_on_the_rank():
    a, b, c = _loader(), _loader(rank=1, world_size=3), _loader(rank=2, world_size=8)
    for epoch, index in ((0, 0), (2, 17), (5, 52)):
        assert a.item_draws(epoch, index) == b.item_draws(epoch, index) == c.item_draws(epoch, index)


def test_subclasses_inherit_the_sharding():
    from fusiondepth_amd.datasets import KITTIRefinerBatches, KITTIStereoBatches
    for cls in (KITTIStereoBatches, KITTIRefinerBatches):
        ld = _loader(cls, rank=1, world_size=2)
        assert _batches(ld.epoch_order(0)) == _batches(_loader().epoch_order(0))[1:26:2]


# --------------------------------------------------------------------------------------------- build_loaders and the flags
def _splits(tmp_path, gt=True):
    d = tmp_path / "splits"
    for sub, name, n in (("eigen_zhou", "train_files.txt", 9), ("eigen_full", "train_files.txt", 5), ("eigen", "test_files.txt", 3)):
        os.makedirs(d / sub, exist_ok=True)
        (d / sub / name).write_text("\n".join(_lines(n)) + "\n")
    if gt:
        data = np.array([np.zeros((4, 5), np.float32), np.zeros((3, 5), np.float32), np.ones((4, 6), np.float32)], dtype=object)
        np.savez_compressed(str(d / "eigen" / "gt_depths.npz"), data=data)
    return str(d)


def test_build_loaders(tmp_path):
    from fusiondepth_amd import train as T
    from fusiondepth_amd.datasets import KITTIRAWBatches, KITTIStereoBatches
    splits = _splits(tmp_path)
    tr, va, gt = T.build_loaders(_opt("--height", "64", "--width", "96", "--batch_size", "2", "--num_workers", "12"), splits, 1, 2, seed=9,
                                 local_world_size=2)
    assert type(tr) is KITTIRAWBatches and type(va) is KITTIRAWBatches
    assert (tr.rank, tr.world_size, tr.seed, tr.shuffle, tr.drop_last, tr.is_train, tr.batch_size) == (1, 2, 9, True, True, True, 2)
    assert tr.frame_idxs == [0, -1, 1] and len(tr.filenames) == 9 and tr.img_ext == ".jpg" and (tr.height, tr.width) == (64, 96)
    assert tr.workers == 8                                       # min(12, 16 // 2)
    assert va.frame_idxs == [0] and va.drop_last is False and not va.is_train and not va.shuffle and va.batch_size == 1
    assert (va.rank, va.world_size) == (0, 1) and len(va.filenames) == 3 and len(va) == 3
    assert [g.shape for g in gt] == [(4, 5), (3, 5), (4, 6)]
    # --use_stereo, --png, the split, --eval_batch_size, --val_limit, --no_val
    tr, va, gt = T.build_loaders(_opt("--use_stereo", "--png", "--split", "eigen_full", "--eval_batch_size", "2"), splits, 0, 1, val_limit=2)
    assert type(tr) is KITTIStereoBatches and type(va) is KITTIStereoBatches
    assert tr.frame_idxs == [0, -1, 1, "s"] and va.frame_idxs == [0] and tr.img_ext == va.img_ext == ".png"
    assert len(tr.filenames) == 5 and len(va.filenames) == 2 and len(gt) == 2 and va.batch_size == 2 and tr.workers == 4
    tr, va, gt = T.build_loaders(_opt(), splits, 0, 1, no_val=True, lidar_source="raw", batch_size=3)
    assert va is None and gt is None and tr.lidar_source == "raw" and tr.batch_size == 3
    assert T.decode_workers(4, 8) == 2 and T.decode_workers(4, 32) == 1 and T.decode_workers(0, 1) == 1


def test_build_loaders_refusals(tmp_path):
    from fusiondepth_amd import train as T
    with pytest.raises(NotImplementedError, match="KITTIOdomDataset has no LiDAR keys"):
        T.build_loaders(_opt("--dataset", "kitti_odom"), _splits(tmp_path), 0, 1)
    with pytest.raises(FileNotFoundError, match="export_gt_depths"):
        T.build_loaders(_opt(), _splits(tmp_path / "b", gt=False), 0, 1)
    T.build_loaders(_opt(), _splits(tmp_path / "c", gt=False), 0, 1, no_val=True)      # not needed without validation


def test_extra_flags_are_taken_off_the_command_line():
    from fusiondepth_amd import train as T
    from fusiondepth_amd.options import MonodepthOptions
    argv = ["--png", "--splits_dir", "/d/splits", "--seed=7", "--batch_size", "2", "--no_val", "--lidar_source", "raw", "--val_limit", "5"]
    extra, rest = T.split_off_extra(argv)
    assert extra == {"splits_dir": "/d/splits", "seed": 7, "lidar_source": "raw", "val_limit": 5, "no_val": True}
    assert rest == ["--png", "--batch_size", "2"]
    o = MonodepthOptions().parse(rest)
    assert o.png and o.batch_size == 2 and not any(hasattr(o, k) for k in extra)
    assert T.split_off_extra([])[0] == {"splits_dir": "splits", "seed": 0, "lidar_source": "files", "val_limit": None, "no_val": False}
    for bad, word in ((["--seed"], "needs a value"), (["--lidar_source", "disk"], "lidar_source"), (["--val_limit", "0"], "val_limit")):
        with pytest.raises(ValueError, match=word):
            T.split_off_extra(bad)
    extra, rest = T.split_off_extra(["--no_validation", "--seed", "1"])
    assert rest == ["--no_validation"]
    with pytest.raises(SystemExit):                              # an unknown flag still fails in argparse
        MonodepthOptions().parse(rest)
    with pytest.raises(SystemExit):                              # and the options surface does not know the extra ones
        MonodepthOptions().parse(["--seed", "1"])


def test_binding_of_the_scorer():
    import ctypes
    from fusiondepth_amd import _lib, validation as V
    assert _lib.ABI_VERSION == 8
    assert _lib.SIGNATURES["fd_val_scores_ws_bytes"] == ("iil", "l")
    args, res = _lib.SIGNATURES["fd_val_scores"]
    assert res == "i" and len(args) == 15 and args[-1] == "p"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "fd_val_scores") and hasattr(lib, "fd_val_scores_ws_bytes")
    header = open(os.path.join(__import__("conftest").ROOT, "include", "fdhip.h")).read()
    assert "#define FD_ABI_VERSION 8" in header and "int fd_val_scores(" in header
    desc, total = V.plan_gt([np.zeros((375, 1242)), np.zeros((128, 192)), np.zeros((40, 100))], gap=3)
    assert [tuple(d[["y0", "y1", "x0", "x1"]]) for d in desc] == [(153, 371, 44, 1197), (128, 128, 44, 192), (40, 40, 44, 100)]
    assert [int(d["offset"]) for d in desc] == [3, 3 + 465750 + 3, 465756 + 128 * 192 + 3] and total == 465756 + 128 * 192 + 3 + 4000
    assert [int(d["pred"]) for d in desc] == [0, 1, 2]
    assert V.val_window(40, 100, (5, 37, 4, 90)) == (5, 37, 4, 90) and V.val_window(30, 50, (5, 37, 4, 90)) == (5, 30, 4, 50)


# --------------------------------------------------------------------------------------------- the restatement against torch
def _bits(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


@pytest.mark.parametrize("size,odd", [((375, 1242), False), ((370, 1226), True)], ids=["375x1242-even", "370x1226-odd"])
def test_restatement_equals_the_reference_expression_on_the_cpu(size, odd):
    """Counts, both (lower) medians, the ratio and the three threshold counts bit for bit; the metrics to float32 summation accuracy."""
    rng = np.random.default_rng(size[0])
    depth = val_ref.depth_pred(rng)
    gt = val_ref.sparse_gt(rng, *size, odd=odd)
    want = val_ref.torch_reference(depth, gt)
    got = val_ref.val_scores(depth[None], [gt])
    n = int(got["counts"][0])
    assert n == want["count"] and n % 2 == int(odd) and n > 5000
    assert np.array_equal(_bits(got["med_gt"][0]), _bits(want["med_gt"]))
    assert np.array_equal(_bits(got["med_pred"][0]), _bits(want["med_pred"]))
    assert np.array_equal(_bits(got["ratios"][0]), _bits(want["ratio"]))
    assert got["thresh_counts"][0].tolist() == want["thresh_counts"]
    # the lower median is what was tested: numpy's differs for the even count
    win = gt[153:371, 44:1197]
    assert (np.median(win[win > 0]) != got["med_gt"][0]) == (not odd)
    # torch's float32 means (pairwise float32 sums, float32 logs) against float64 sums of the float32 terms
    np.testing.assert_allclose(got["metrics"][0], want["metrics"], rtol=2e-5)


def test_restatement_edges():
    depths, gts, res = val_ref.six_case()
    assert res["counts"][0] % 2 == 0 and res["counts"][1] % 2 == 1
    assert res["counts"][2] == 0 and res["counts"][3] == 0 and res["counts"][5] == 218 * 1153 == 251354
    assert np.isnan(res["metrics"][2]).all() and np.isnan(res["metrics"][3]).all() and np.isnan(res["ratios"][2:4]).all()
    assert np.isnan(res["metrics"][4][:4]).all() and (res["metrics"][4][4:] == 0).all() and np.isnan(res["ratios"][4])
    assert np.isfinite(res["metrics"][[0, 1, 5]]).all()
