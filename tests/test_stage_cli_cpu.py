"""Host side of ``python -m fusiondepth_amd.refine`` and ``python -m fusiondepth_amd.complete``: the extra flags, ``build_loaders`` of
both, the binding of the Completor's scorer, and the numpy restatement of the Completor's validation metrics
(tests/completion_val_ref.py) pinned to the reference's own torch expression.  No GPU is touched."""
import os

import numpy as np
import pytest

import completion_tree as CT
import completion_val_ref as CV
import conftest


def _opt(*flags):
    from fusiondepth_amd.options import MonodepthOptions
    return MonodepthOptions().parse(list(flags))


def _lines(n):
    return ["2011_09_26/2011_09_26_drive_0001_sync %d l" % i for i in range(n)]


# --------------------------------------------------------------------------------------------- flags
def test_refine_flags_are_train_flags():
    from fusiondepth_amd import refine as R, train as T
    assert R.split_off_extra is T.split_off_extra and R.write_summary is T.write_summary and R.decode_workers is T.decode_workers
    extra, rest = R.split_off_extra(["--png", "--splits_dir", "/d/s", "--seed=7", "--num_epochs", "2", "--no_val", "--lidar_source", "raw",
                                     "--val_limit", "5"])
    assert extra == {"splits_dir": "/d/s", "seed": 7, "lidar_source": "raw", "val_limit": 5, "no_val": True}
    assert rest == ["--png", "--num_epochs", "2"] and _opt(*rest).num_epochs == 2
    for bad, word in ((["--seed"], "needs a value"), (["--lidar_source", "disk"], "lidar_source"), (["--val_limit", "0"], "val_limit")):
        with pytest.raises(ValueError, match=word):
            R.split_off_extra(bad)


def test_complete_flags():
    from fusiondepth_amd import complete as C
    extra, rest = C.split_off_extra(["--png", "--seed=7", "--batch_size", "2", "--no_val", "--val_limit", "5", "--val_route", "per_batch",
                                     "--load_weights_folder", "/w/rms900"])
    assert extra == {"seed": 7, "val_limit": 5, "val_route": "per_batch", "no_val": True, "load_weights_given": True}
    assert rest == ["--png", "--batch_size", "2", "--load_weights_folder", "/w/rms900"]
    o = _opt(*rest)
    assert o.load_weights_folder == "/w/rms900" and o.train_load_weights_folder is None and not any(hasattr(o, k) for k in extra)
    assert C.split_off_extra(["--load_weights_folder=/w"])[0]["load_weights_given"]
    assert C.split_off_extra([])[0] == {"seed": 0, "val_limit": None, "val_route": C.DEFAULT_VAL_ROUTE, "no_val": False,
                                        "load_weights_given": False}
    assert C.DEFAULT_VAL_ROUTE in ("fused", "per_batch")
    for bad, word in ((["--seed"], "needs a value"), (["--val_route", "gpu"], "val_route"), (["--val_limit", "0"], "val_limit"),
                      (["--val_limit", "-3"], "val_limit")):
        with pytest.raises(ValueError, match=word):
            C.split_off_extra(bad)
    with pytest.raises(ValueError):
        C.split_off_extra(["--seed", "x"])
    with pytest.raises(SystemExit):                              # the options surface does not know the extra ones
        _opt("--val_route", "fused")


# --------------------------------------------------------------------------------------------- refine.build_loaders
def _splits(tmp_path, gt=True):
    d = tmp_path / "splits"
    for sub, name, n in (("eigen_zhou", "train_files.txt", 9), ("eigen_full", "train_files.txt", 5), ("eigen", "test_files.txt", 3)):
        os.makedirs(d / sub, exist_ok=True)
        (d / sub / name).write_text("\n".join(_lines(n)) + "\n")
    if gt:
        data = np.array([np.zeros((4, 5), np.float32), np.zeros((3, 5), np.float32), np.ones((4, 6), np.float32)], dtype=object)
        np.savez_compressed(str(d / "eigen" / "gt_depths.npz"), data=data)
    return str(d)


def test_refine_build_loaders(tmp_path):
    from fusiondepth_amd import refine as R
    from fusiondepth_amd.datasets import KITTIRefinerBatches
    splits = _splits(tmp_path)
    opt = _opt("--height", "64", "--width", "96", "--batch_size", "2", "--num_workers", "12", "--eval_batch_size", "2")
    opt.clone_gdc = True                                         # what Refiner.__init__ sets
    both = [R.build_loaders(opt, splits, rank, 2, seed=9, local_world_size=2, no_val=rank != 0, device="cpu") for rank in range(2)]
    tr, va, gt = both[0]
    assert type(tr) is KITTIRefinerBatches and type(va) is KITTIRefinerBatches
    assert (tr.rank, tr.world_size, tr.seed, tr.shuffle, tr.drop_last, tr.is_train, tr.batch_size) == (0, 2, 9, True, True, True, 2)
    assert tr.frame_idxs == [0, -1, 1] and len(tr.filenames) == 9 and tr.img_ext == ".jpg" and (tr.height, tr.width) == (64, 96)
    assert tr.workers == 8 and tr.need_gdc and tr.lidar_source == "files"
    assert va.frame_idxs == [0] and va.drop_last is False and not va.is_train and not va.shuffle and va.batch_size == 2
    assert (va.rank, va.world_size) == (0, 1) and len(va.filenames) == 3 and len(va) == 2 and not va.need_gdc
    assert [g.shape for g in gt] == [(4, 5), (3, 5), (4, 6)]
    assert both[1][1] is None and both[1][2] is None             # rank 0 alone validates
    # the shards of two ranks: disjoint, equal in length, the global batches of the epoch in turns
    a, b = both[0][0].epoch_order(0), both[1][0].epoch_order(0)
    perm = [int(i) for i in np.random.default_rng([9, 0]).permutation(9)]
    assert len(a) == len(b) == 4 and not set(a) & set(b) and a == perm[0:2] + perm[4:6] and b == perm[2:4] + perm[6:8]
    # the split, --png, --val_limit, lidar_source, batch_size
    tr, va, gt = R.build_loaders(_opt("--png", "--split", "eigen_full"), splits, 0, 1, val_limit=2, lidar_source="raw", batch_size=3,
                                 device="cpu")
    assert len(tr.filenames) == 5 and len(va.filenames) == 2 and len(gt) == 2 and va.batch_size == 1 and tr.img_ext == va.img_ext == ".png"
    assert tr.lidar_source == "raw" and tr.batch_size == 3 and tr.workers == 4


def test_refine_build_loaders_refusals(tmp_path):
    from fusiondepth_amd import refine as R
    with pytest.raises(NotImplementedError, match="KITTIOdomDataset has no LiDAR keys"):
        R.build_loaders(_opt("--dataset", "kitti_odom"), _splits(tmp_path), 0, 1, device="cpu")
    with pytest.raises(FileNotFoundError, match="export_gt_depths"):
        R.build_loaders(_opt(), _splits(tmp_path / "b", gt=False), 0, 1, device="cpu")
    tr, va, gt = R.build_loaders(_opt(), _splits(tmp_path / "c", gt=False), 0, 1, no_val=True, device="cpu")
    assert va is None and gt is None
    data = np.array([np.zeros((4, 5), np.float32), np.zeros((3, 5), np.float32)], dtype=object)
    np.savez_compressed(os.path.join(_splits(tmp_path / "d"), "eigen", "gt_depths.npz"), data=data)
    with pytest.raises(ValueError, match="holds 2 maps for the 3 lines"):
        R.build_loaders(_opt(), str(tmp_path / "d" / "splits"), 0, 1, device="cpu")


# --------------------------------------------------------------------------------------------- complete.build_loaders
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    data = tmp_path_factory.mktemp("data")
    CT.make_tree(str(data / "completion"))
    return str(data)


def test_complete_build_loaders(tree):
    from fusiondepth_amd import complete as C
    from fusiondepth_amd.completion_data import KITTICompletionBatches
    opt = _opt("--data_path", tree, "--batch_size", "2", "--eval_batch_size", "2", "--num_workers", "12")
    opt.height, opt.width = 352, 1216                            # what Completor.__init__ sets in full-resolution mode
    n_train = sum(len(v) for v in CT.TRAIN_KEPT.values())
    both = [C.build_loaders(opt, rank, 2, seed=4, no_val=rank != 0, local_world_size=2, device="cpu") for rank in range(2)]
    tr, va = both[0]
    assert type(tr) is KITTICompletionBatches and type(va) is KITTICompletionBatches
    assert (tr.split, tr.is_train, tr.shuffle, tr.drop_last, tr.batch_size, tr.seed, tr.workers) == ("train", True, True, True, 2, 4, 8)
    assert tr.frame_idxs == [0, -1, 1] and tr.frames == [0, -1, 1] and len(tr.filenames) == n_train == 8 and tr.full_res
    assert (tr.height, tr.width) == (352, 1216) and (tr.rank, tr.world_size) == (0, 2)
    assert (va.split, va.val_split, va.is_train, va.shuffle, va.drop_last, va.batch_size) == ("val", "select", False, False, False, 2)
    assert va.frame_idxs == [0] and len(va.filenames) == len(CT.SELECT) and len(va) == 2 and (va.rank, va.world_size) == (0, 1)
    assert all("val_selection_cropped" in p for p in va.filenames) and va.filenames == sorted(va.filenames)
    assert both[1][1] is None
    a, b = both[0][0].epoch_order(0), both[1][0].epoch_order(0)
    assert len(a) == len(b) == 4 and not set(a) & set(b) and len(both[0][0]) == len(both[1][0]) == 2
    # --val_limit: the first N files; --completion_val_split full; --completion_not_full_res; --no_val
    opt = _opt("--data_path", tree, "--completion_val_split", "full", "--completion_not_full_res")
    tr, va = C.build_loaders(opt, val_limit=2, device="cpu")
    assert va.val_split == "full" and len(va.filenames) == 2 and len(va) == 2 and va.batch_size == 1 and not va.full_res
    full = C.build_loaders(opt, device="cpu")[1]
    assert len(full.filenames) == len(CT.VAL_FRAMES) and va.filenames == full.filenames[:2]
    assert tr.frame_idxs == [0, -1, 1] and (tr.height, tr.width) == (192, 640) and tr.batch_size == opt.batch_size and tr.workers == 4
    assert C.build_loaders(opt, no_val=True, device="cpu")[1] is None
    with pytest.raises(RuntimeError, match="Found 0 images"):
        C.build_loaders(_opt("--data_path", os.path.join(tree, "nowhere")), device="cpu")


# --------------------------------------------------------------------------------------------- the binding
def test_binding_of_the_completion_scorer():
    import ctypes
    import re
    from fusiondepth_amd import _lib, validation as V
    assert _lib.ABI_VERSION == 8
    assert _lib.SIGNATURES["fd_completion_val_scores_ws_bytes"] == ("iil", "l")
    args, res = _lib.SIGNATURES["fd_completion_val_scores"]
    assert res == "i" and args == "piii" "pl" "pi" "il" "fff" "p" "pp"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "fd_completion_val_scores") and hasattr(lib, "fd_completion_val_scores_ws_bytes")
    header = open(os.path.join(conftest.ROOT, "include", "fdhip.h")).read()
    assert "#define FD_ABI_VERSION 8" in header
    for name in ("fd_completion_val_scores_ws_bytes", "fd_completion_val_scores"):      # the header's arity
        proto = re.search(r"\b(?:int|long) %s\(([^;]*)\);" % name, header).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name][0]), name
    table = open(os.path.join(conftest.ROOT, "fusiondepth_amd", "csrc", "replay_table.inc")).read()
    assert '{"fd_completion_val_scores", "piiiplpiilfffppp"},' in table
    # the window of each mode, as slicing clips it
    assert V.val_window(352, 1216, V.completion_window(False)) == (0, 352, 0, 1216)
    assert V.val_window(352, 1216, V.completion_window(True)) == (153, 352, 44, 1197)
    assert V.val_window(128, 192, V.completion_window(True)) == (128, 128, 44, 192)
    desc, total = V.plan_gt([np.zeros((40, 100)), np.zeros((375, 1242))], window=[V.WHOLE_MAP, V.VAL_CROP])
    assert [tuple(d[["y0", "y1", "x0", "x1"]]) for d in desc] == [(0, 40, 0, 100), (153, 371, 44, 1197)] and total == 4000 + 375 * 1242
    assert np.float32(V.COMPLETION_GT_MIN) == CV.GT_MIN


# --------------------------------------------------------------------------------------------- the restatement against torch
def _bits(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


CASES = [((352, 1216), (352, 1216), False, False), ((352, 1216), (352, 1216), False, True), ((352, 1216), (352, 1216), True, False),
         ((352, 1216), (352, 1216), True, True), ((384, 1280), (192, 640), False, None)]


@pytest.mark.parametrize("gt_size,pred_size,crop,odd", CASES,
                         ids=["352x1216-even", "352x1216-odd", "352x1216-crop-even", "352x1216-crop-odd", "192x640-to-384x1280"])
def test_restatement_equals_the_reference_expression_on_the_cpu(gt_size, pred_size, crop, odd):
    """Counts, both (lower) medians, the ratio and the three threshold counts bit for bit; the selection agrees on float32(0.1) and
    its neighbours; the metrics to float32 summation accuracy (the observed distance is reported, DESIGN.md section 18 records it)."""
    rng = np.random.default_rng(gt_size[0] + 2 * int(crop) + int(bool(odd)))
    depth = CV.depth_pred(rng, pred_size)
    gt = CV.sparse_gt(rng, *gt_size, odd=odd, eigen_crop=crop)
    inside = gt[153:371, 44:1197] if crop else gt
    assert all((inside == v).any() for v in CV.EDGE)             # float32(0.1) and its two neighbours are among the pixels
    want = CV.torch_reference(depth, gt, eigen_crop=crop)
    got = CV.completion_val_scores(depth[None], [gt], eigen_crop=crop)
    n = int(got["counts"][0])
    assert n == want["count"] and n > 5000 and (odd is None or n % 2 == int(odd))
    assert n == int((inside > 0.2).sum()) + 1                    # of the three edge values only the upper neighbour is selected
    assert np.array_equal(_bits(got["med_gt"][0]), _bits(want["med_gt"]))
    assert np.array_equal(_bits(got["med_pred"][0]), _bits(want["med_pred"]))
    assert np.array_equal(_bits(got["ratios"][0]), _bits(want["ratio"]))
    assert got["thresh_counts"][0].tolist() == want["thresh_counts"]
    rel = np.abs(got["metrics"][0] - want["metrics"]) / np.abs(want["metrics"])
    conftest.report("completion restatement vs torch float32 .mean(), gt %dx%d%s (n = %d), worst of 7 (rel)" %
                    (gt_size + (" crop" if crop else "", n)), rel.max(), 2e-5)
    # torch's float32 means (pairwise float32 sums, float32 logs) against float64 sums of the float32 terms: the bound
    # tests/test_train_cli_cpu.py holds tests/val_ref.py to for the same construction
    np.testing.assert_allclose(got["metrics"][0], want["metrics"], rtol=2e-5)
    assert 100.0 < got["metrics"][0][2] < 80000.0                # the RMSE is in millimetres


def test_restatement_edges():
    depths, gts, crops, res = CV.mixed_case()
    c = res["counts"]
    assert c[0] % 2 == 0 and c[1] % 2 == 1 and c[2] == 96 * 128 > 8192 and c[3] == 0 and c[5] == 0 and c[6] == 4000
    assert (c[[0, 1, 2, 4, 6, 7, 8]] > 100).all()
    assert np.isnan(res["metrics"][[3, 5]]).all() and np.isnan(res["ratios"][[3, 5]]).all()
    assert np.isnan(res["metrics"][6][:4]).all() and (res["metrics"][6][4:] == 0).all() and np.isnan(res["ratios"][6])
    assert np.isfinite(res["metrics"][[0, 1, 2, 4, 7, 8]]).all()
    win = gts[4][153:352, 44:1197]
    assert c[4] == int((win > CV.GT_MIN).sum()) and (gts[4][:153] > CV.GT_MIN).any()      # clipped to rows 153:352, others ignored
