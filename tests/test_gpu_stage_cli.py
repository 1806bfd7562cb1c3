"""``python -m fusiondepth_amd.complete`` and ``python -m fusiondepth_amd.refine`` on synthetic trees, ResNet-18 throughout: the commands
in one process, ``Completor.train`` with a validation loader on the per-batch route, ``--load_weights_folder``, and ``refine`` as two
data-parallel ranks that share the test box's GPU over gloo (the launch of tests/test_gpu_train_cli.py)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import completion_tree as CT
import completion_val_ref as CV
import kitti_tree
from conftest import ROOT, assert_close

pytestmark = pytest.mark.gpu


def _scalars(log, mode="val"):
    return [json.loads(l) for l in open(os.path.join(log, mode, "scalars.jsonl"))]


# ---------------------------------------------------------------------------------------------- complete
@pytest.fixture(scope="module")
def completion(tmp_path_factory):
    data = tmp_path_factory.mktemp("data")
    CT.make_tree(str(data / "completion"))
    return str(data), str(tmp_path_factory.mktemp("log"))


def _complete_flags(data, log_dir, name):
    return ["--num_layers", "18", "--completion_num_layers", "18", "--completion_pose_num_layers", "18", "--weights_init", "scratch",
            "--data_path", data, "--png", "--completion_not_full_res", "--log_dir", log_dir, "--model_name", name, "--batch_size", "2",
            "--log_frequency", "1", "--num_workers", "4"]


@pytest.fixture(scope="module")
def first_run(completion):
    """``complete.main`` for one epoch of 4 batches with a validation at every log event -> (the Completor, its log folder, its
    final parameters)."""
    from fusiondepth_amd import complete as C
    data, log_dir = completion
    cp = C.main(_complete_flags(data, log_dir, "c1") + ["--completion_num_epochs", "1", "--seed", "3"])
    torch.cuda.synchronize()
    return cp, os.path.join(log_dir, "c1"), cp.flat.flat_param.clone()


def test_complete_command_one_process(first_run, completion):
    from fusiondepth_amd import complete as C
    cp, log, _ = first_run
    assert C.DEFAULT_VAL_ROUTE == "fused" and cp.val_scorer is not None and len(cp.val_scorer) == len(CT.SELECT)
    summary = json.load(open(os.path.join(log, "train_summary.rank0.json")))
    assert summary["epochs"] == 1 and summary["steps"] == 4 and summary["batches_per_epoch"] == 4 and summary["world_size"] == 1
    assert np.isfinite(summary["last_loss"]) and np.isfinite(summary["param_checksum"]).all() and np.isfinite(summary["best"])
    assert sorted(summary["items"][0]) == list(range(8))
    val = _scalars(log)
    assert len(val) == 4 and len(_scalars(log, "train")) == 4 and all(np.isfinite(v["de/rms"]) for v in val)      # one per log event
    assert summary["best"] == min(v["de/rms"] for v in val) == cp.best
    assert os.path.isdir(os.path.join(log, "models", "weights_0"))
    # the fused route's mean metrics are the restatement's over the depths the scorer saw (3 images: one chunk, still in the staging)
    sc = cp.val_scorer
    assert sc.calls == 1 and sc.pred_size == (192, 640) and sc.gt_size == (384, 1280)
    depths, gts = sc.pred.cpu().numpy(), sc.gt.cpu().numpy()
    want = CV.completion_val_scores(depths, gts)
    assert (want["counts"] > 100).all() and np.array_equal(cp.last_val_rows[:, 8].astype(np.int64), want["counts"])
    assert np.array_equal(cp.last_val_rows[:, 7].astype(np.float32).view(np.uint32), want["ratios"].view(np.uint32))
    got = np.array([val[-1][m] for m in cp.depth_metric_names], np.float64)
    assert_close(got, want["metrics"].mean(0), rtol=1e-9, atol=0, what="mean validation metrics of the last log event")
    # ... and the per-batch compute_depth_losses route on the same model (nothing was trained after the last validation), within the
    # distance tests/test_stage_cli_cpu.py holds the restatement to against torch's float32 means
    loader = C.build_loaders(cp.opt, device=cp.device)[1]
    assert len(loader) == 3 and loader.batch_size == 1
    fused = cp.val_metrics(loader)
    assert_close([fused[m] for m in cp.depth_metric_names], got, rtol=1e-6, atol=0, what="the fused route, run again")
    cp.val_scorer = None
    try:
        plain = cp.val_metrics(loader)
    finally:
        cp.val_scorer = sc
        loader.close()
    for m in cp.depth_metric_names:
        print("%s: fused %.9g, per batch %.9g" % (m, fused[m], float(plain[m])))
    np.testing.assert_allclose([float(plain[m]) for m in cp.depth_metric_names], got, rtol=2e-5)


def test_completor_train_logs_validation_on_the_per_batch_route(completion, tmp_path):
    """``Completor.train(train_loader, val_loader)`` called directly, ``val_scorer = None``: ``run_epoch`` logs the losses of
    ``Completor.val``'s ``(losses, saved)``."""
    from fusiondepth_amd import complete as C
    from fusiondepth_amd.completor import Completor
    from fusiondepth_amd.options import MonodepthOptions
    data, _ = completion
    opt = MonodepthOptions().parse(_complete_flags(data, str(tmp_path), "direct") + ["--completion_num_epochs", "1"])
    torch.manual_seed(3)
    cp = Completor(opt, verbose=False)
    assert cp.val_scorer is None
    train_loader, val_loader = C.build_loaders(cp.opt, seed=2, device=cp.device)
    train_loader.filenames = train_loader.filenames[:2]          # one epoch of 1 batch
    try:
        cp.train(train_loader, val_loader)
        torch.cuda.synchronize()
    finally:
        train_loader.close()
        val_loader.close()
    val = _scalars(os.path.join(str(tmp_path), "direct"))
    assert cp.step == 1 and len(val) == 1 and all(np.isfinite(val[0][m]) for m in cp.depth_metric_names)
    assert val[0]["de/rms"] == cp.best > 100.0                   # millimetres
    losses, saved = cp.val([], save_best=False)                  # Completor.val keeps returning the pair
    assert isinstance(losses, dict) and saved is None


def test_complete_loads_the_weights_folder(first_run, completion, tmp_path):
    from fusiondepth_amd import complete as C
    data, _ = completion
    _, log, params = first_run
    folder = os.path.join(log, "models", "weights_0")
    assert os.path.isfile(os.path.join(folder, "adam.pth")) and os.path.isfile(os.path.join(folder, "beam_encoder_pose.pth"))
    flags = _complete_flags(data, str(tmp_path), "c2") + ["--completion_num_epochs", "0", "--no_val", "--seed", "9"]
    loaded = C.main(flags + ["--load_weights_folder", folder])
    assert loaded.opt.train_load_weights_folder == folder and loaded.step == 0
    assert torch.equal(loaded.flat.flat_param, params) and loaded.adam_step_count == 4
    for name in ("encoder", "depth"):                            # buffers too: the BatchNorm statistics
        saved = torch.load(os.path.join(folder, name + ".pth"), map_location="cpu")
        for k, v in loaded.models[name].state_dict().items():
            assert torch.equal(v.cpu(), saved[k]), (name, k)
    # without the flag the networks start from --weights_init, whatever the option's default names
    fresh = C.main(flags)
    assert fresh.opt.train_load_weights_folder is None and fresh.adam_step_count == 0
    assert not torch.equal(fresh.flat.flat_param, params)


# ---------------------------------------------------------------------------------------------- refine
H, W = 96, 320


@pytest.fixture(scope="module")
def refine_tree(tmp_path_factory):
    """tests/test_gpu_refiner_data.py's chain up to the Refiner: one date of native 192 x 640 frames, a stage-1 checkpoint, the maps
    ``inf_depth_map`` and ``inf_gdc`` write, the split files and the ``gt_depths.npz`` of ``export_gt_depths``."""
    from fusiondepth_amd import inf_depth_map, inf_gdc, kitti_utils as KU
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.trainer import Trainer
    root = str(tmp_path_factory.mktemp("kitti"))
    lines = kitti_tree.make_tree(root, [("2011_09_26", "2011_09_26_drive_0001_sync", (192, 640), (640 / 1242.0, 192 / 375.0))], frames=6,
                                 down=0.35)
    assert len(lines) == 4
    splits = str(tmp_path_factory.mktemp("splits"))
    for name, file in (("eigen_zhou", "train_files.txt"), ("eigen", "test_files.txt")):
        os.makedirs(os.path.join(splits, name))
        with open(os.path.join(splits, name, file), "w") as f:
            f.write("\n".join(lines) + "\n")
    gts = KU.export_gt_depths(root, lines, "eigen", os.path.join(splits, "eigen", "gt_depths.npz"))
    assert [g.shape for g in gts] == [(192, 640)] * 4
    assert all(int((g[153:, 44:] > 0).sum()) > 100 for g in gts)        # the Garg crop, clipped to 192 rows, is not empty
    o = MonodepthOptions().parse(["--num_layers", "18", "--weights_init", "scratch", "--batch_size", "2", "--height", str(H), "--width", str(W),
                                  "--log_dir", str(tmp_path_factory.mktemp("stage1"))])
    torch.manual_seed(5)
    tr = Trainer(o, verbose=False)
    folder = tr.save_model("init")
    del tr
    split = os.path.join(splits, "eigen", "test_files.txt")
    assert inf_depth_map.main(["--load_weights_folder", folder, "--data_path", root, "--split_files", split, "--png", "--num_layers", "18",
                               "--height", str(H), "--width", str(W), "--batch_size", "2"]) == 0
    inf_gdc.main(["--data_path", root, "--split_files", split])
    return root, splits, lines, folder


def _refine_flags(root, splits, folder, log_dir, name):
    return ["--num_layers", "18", "--weights_init", "scratch", "--batch_size", "2", "--height", str(H), "--width", str(W), "--png",
            "--data_path", root, "--log_dir", str(log_dir), "--model_name", name, "--log_frequency", "1", "--num_epochs", "1",
            "--refine_load_weights_folder", folder, "--num_workers", "4", "--splits_dir", splits, "--seed", "5"]


def test_refine_command_one_process(refine_tree, tmp_path):
    from fusiondepth_amd import refine as R
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.refiner import Refiner
    root, splits, lines, folder = refine_tree
    flags = _refine_flags(root, splits, folder, tmp_path, "r1")
    rf = R.main(flags)
    torch.cuda.synchronize()
    log = os.path.join(str(tmp_path), "r1")
    summary = json.load(open(os.path.join(log, "train_summary.rank0.json")))
    assert summary["epochs"] == 1 and summary["steps"] == 2 and summary["batches_per_epoch"] == 2 and summary["world_size"] == 1
    assert np.isfinite(summary["last_loss"]) and np.isfinite(summary["param_checksum"]).all()
    assert summary["items"] == [[int(i) for i in np.random.default_rng([5, 0]).permutation(4)]]
    val = _scalars(log)
    assert len(val) == 2 and all(np.isfinite(v["de/abs_rel"]) for v in val)
    assert summary["best"] == min(v["de/abs_rel"] for v in val) == rf.best
    assert len(rf.val_gt) == 4 and (rf.last_val_rows[:, 8] > 100).all()                     # validation through val_gt
    assert os.path.isfile(os.path.join(log, "models", "weights_best", "refine2d_decoder.pth"))
    # only refine2d_decoder's parameters changed: the frozen networks are the checkpoint's, the decoder is not its initialisation
    for name, net in rf.models.items():
        if name == "refine2d_decoder":
            continue
        saved = torch.load(os.path.join(folder, name + ".pth"), map_location="cpu")
        for k, v in net.state_dict().items():
            assert torch.equal(v.cpu(), saved[k]), (name, k)
    rest = R.split_off_extra(flags)[1]
    torch.manual_seed(5)
    init = Refiner(MonodepthOptions().parse(rest), verbose=False)
    assert rf.trained == ["refine2d_decoder"] and init.flat.flat_param.numel() == rf.flat.flat_param.numel()
    assert not torch.equal(init.flat.flat_param, rf.flat.flat_param) and torch.isfinite(rf.flat.flat_param).all()


def test_refine_command_two_ranks_over_gloo(refine_tree, tmp_path):
    root, splits, lines, folder = refine_tree
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, FD_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", "fusiondepth_amd.refine"] + _refine_flags(root, splits, folder, tmp_path, "two") + \
          ["--val_limit", "2"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:]
    log = os.path.join(str(tmp_path), "two")
    s0, s1 = [json.load(open(os.path.join(log, "train_summary.rank%d.json" % k))) for k in range(2)]
    assert s0["param_checksum"] == s1["param_checksum"] and s0["steps"] == s1["steps"] == 1 and s0["world_size"] == 2
    assert np.isfinite(s0["last_loss"]) and np.isfinite(s1["last_loss"])
    perm = [int(i) for i in np.random.default_rng([5, 0]).permutation(4)]
    assert s0["items"] == [perm[:2]] and s1["items"] == [perm[2:]]       # disjoint, and together the global batches of the epoch
    val = _scalars(log)
    assert len(val) == 1 and np.isfinite(val[0]["de/abs_rel"])         # rank 0 alone validated
