"""``python -m fusiondepth_amd.train`` on a synthetic KITTI tree: ``Trainer.val`` through the fused scorer (``val_gt``), the command in
one process, and the command as two data-parallel ranks that share the test box's GPU over gloo (the launch of tests/test_gpu_dp.py).

The network runs at 192 x 640: the date's images are 375 x 1242 (the size at which the fixed crop ``153:371, 44:1197`` is the Garg crop),
and the loader rasterises ``4beam`` at twice the network's size, which must not be narrower than the image - 640 is the smallest width
that ``KITTIRAWBatches`` accepts for this date."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import kitti_tree
import val_ref
from conftest import ROOT, assert_close

pytestmark = pytest.mark.gpu
H, W = 192, 640


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """One date at 375 x 1242, six frames: four lines that serve as the training split and as the Eigen test split, and the
    ``gt_depths.npz`` ``export_gt_depths`` writes for them."""
    from fusiondepth_amd import kitti_utils as KU
    root = str(tmp_path_factory.mktemp("kitti"))
    lines = kitti_tree.make_tree(root, [("2011_09_26", "2011_09_26_drive_0001_sync", (375, 1242), (1.0, 1.0))], frames=6, down=0.35)
    assert len(lines) == 4
    splits = str(tmp_path_factory.mktemp("splits"))
    for name, file in (("eigen_zhou", "train_files.txt"), ("eigen", "test_files.txt")):
        os.makedirs(os.path.join(splits, name))
        with open(os.path.join(splits, name, file), "w") as f:
            f.write("\n".join(lines) + "\n")
    gts = KU.export_gt_depths(root, lines, "eigen", os.path.join(splits, "eigen", "gt_depths.npz"))
    assert [g.shape for g in gts] == [(375, 1242)] * 4
    return root, splits, lines, gts


def _flags(root, log_dir, batch=2):
    return ["--num_layers", "18", "--weights_init", "scratch", "--height", str(H), "--width", str(W), "--batch_size", str(batch),
            "--data_path", root, "--png", "--log_dir", str(log_dir), "--num_workers", "4"]


def test_val_with_resident_ground_truth(tree, tmp_path):
    from fusiondepth_amd import train as T
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.trainer import Trainer
    from fusiondepth_amd.validation import ValGroundTruth
    root, splits, lines, gts = tree
    torch.manual_seed(3)
    tr = Trainer(MonodepthOptions().parse(_flags(root, tmp_path)), verbose=False)
    assert tr.val_gt is None                                     # the default: val_metrics / val / run_epoch as before
    _, val_loader, gt_depths = T.build_loaders(tr.opt, splits, batch_size=tr.batch_size)
    assert len(val_loader) == 4 and val_loader.batch_size == 1
    tr.val_gt = ValGroundTruth(gt_depths)
    losses = tr.val(val_loader)
    depths = tr._val_depths.cpu().numpy()                        # the ("depth", 0, 0) maps the scorer saw
    assert depths.shape == (4, H, W)
    tr.set_eval()
    with torch.no_grad():                                        # ... are the network's, in the loader's order
        for k, batch in enumerate(val_loader):
            out, _ = tr.process_batch(batch, val=True)
            assert_close(out[("depth", 0, 0)][0, 0].cpu().numpy(), depths[k], rtol=1e-5, atol=0, what="depth of image %d" % k)
    tr.set_train()
    want = val_ref.val_scores(depths, gts)
    assert (want["counts"] > 100).all() and np.array_equal(tr.last_val_rows[:, 8].astype(np.int64), want["counts"])
    assert np.array_equal(tr.last_val_rows[:, 7].astype(np.float32).view(np.uint32), want["ratios"].view(np.uint32))
    got = np.array([losses[m] for m in tr.depth_metric_names], np.float64)
    assert_close(got, want["metrics"].mean(0), rtol=1e-9, atol=0, what="mean validation metrics")
    assert list(losses) == tr.depth_metric_names
    # the bookkeeping of val is unchanged: a new best is remembered and saved
    assert tr.best == float(losses["de/abs_rel"]) < 10.0
    assert tr.last_saved and tr.last_saved[0].endswith("weights_best") and os.path.isfile(os.path.join(tr.last_saved[0], "encoder.pth"))
    val_loader.close()


def test_command_one_process(tree, tmp_path):
    from fusiondepth_amd import train as T
    root, splits, lines, gts = tree
    tr = T.main(_flags(root, tmp_path) + ["--model_name", "one", "--num_epochs", "1", "--log_frequency", "1", "--splits_dir", splits,
                                          "--seed", "5"])
    log = os.path.join(str(tmp_path), "one")
    summary = json.load(open(os.path.join(log, "train_summary.rank0.json")))
    assert summary["epochs"] == 1 and summary["steps"] == 2 and summary["batches_per_epoch"] == 2 and summary["world_size"] == 1
    assert np.isfinite(summary["last_loss"]) and np.isfinite(summary["param_checksum"]).all()
    assert len(summary["items"]) == 1 and sorted(summary["items"][0]) == [0, 1, 2, 3]          # each training item once
    assert summary["items"][0] == [int(i) for i in np.random.default_rng([5, 0]).permutation(4)]
    val = [json.loads(l) for l in open(os.path.join(log, "val", "scalars.jsonl"))]
    assert len(val) == 2 and all(np.isfinite(v["de/abs_rel"]) for v in val)
    assert summary["best"] == min(v["de/abs_rel"] for v in val) == tr.best
    assert os.path.isdir(os.path.join(log, "models", "weights_best")) and os.path.isdir(os.path.join(log, "models", "weights_0"))
    assert len(tr.val_gt) == 4


def test_command_two_ranks_over_gloo(tree, tmp_path):
    root, splits, lines, gts = tree
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, FD_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", "fusiondepth_amd.train"] + _flags(root, tmp_path) + \
          ["--model_name", "two", "--num_epochs", "1", "--log_frequency", "1", "--splits_dir", splits, "--seed", "5", "--val_limit", "2"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:]
    log = os.path.join(str(tmp_path), "two")
    s0, s1 = [json.load(open(os.path.join(log, "train_summary.rank%d.json" % k))) for k in range(2)]
    assert s0["param_checksum"] == s1["param_checksum"] and s0["steps"] == s1["steps"] == 1 and s0["world_size"] == 2
    assert np.isfinite(s0["last_loss"]) and np.isfinite(s1["last_loss"])
    perm = [int(i) for i in np.random.default_rng([5, 0]).permutation(4)]
    assert s0["items"] == [perm[:2]] and s1["items"] == [perm[2:]]       # disjoint, and together the global batches of the epoch
    val = [json.loads(l) for l in open(os.path.join(log, "val", "scalars.jsonl"))]
    assert len(val) == 1 and np.isfinite(val[0]["de/abs_rel"])         # rank 0 alone validated
