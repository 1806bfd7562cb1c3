"""``--resume``, ``--shard_val`` and ``--weights_init pretrained`` on the GPU.  The acceptance of ``--resume`` has no tolerance: a run
that is stopped after an epoch checkpoint and continued in a fresh process ends on the bits of the run that was never stopped - every
tensor of the last checkpoint and of ``adam.pth``, the learning rate, ``best``, ``step``, the parameter checksum and the item order.

Trees, sizes and flags are those of tests/test_gpu_train_cli.py and tests/test_gpu_stage_cli.py (imported); the training split repeats
the tree's four lines so that an epoch has more than one step.  Every run is a child process under its own time limit."""
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import imagenet_file as IF
import test_gpu_stage_cli as SC
import test_gpu_train_cli as TC
from conftest import ROOT

pytestmark = pytest.mark.gpu
tree, completion, refine_tree = TC.tree, SC.completion, SC.refine_tree         # the fixtures of those files, built once for this one


# --------------------------------------------------------------------------------------------- helpers
def _run(module, flags, ranks=1, limit=240):
    """``python -m fusiondepth_amd.<module> flags`` in a fresh child process (``ranks`` of them over gloo on the one GPU)."""
    env = dict(os.environ, FD_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable]
    if ranks > 1:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
                "--master-port", str(port)]
    t0 = time.time()
    r = subprocess.run(cmd + ["-m", "fusiondepth_amd." + module] + flags, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=limit)
    print("%s x%d: %.1f s" % (module, ranks, time.time() - t0))
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def _summary(log, rank=0):
    return json.load(open(os.path.join(log, "train_summary.rank%d.json" % rank)))


def _same_bits(a, b, what):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape, what
        if a.dtype == torch.float32:
            a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
        assert torch.equal(a, b), what
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), what
        for k in a:
            _same_bits(a[k], b[k], "%s[%r]" % (what, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same_bits(x, y, "%s[%d]" % (what, i))
    else:
        assert a == b and type(a) is type(b), what


def _same_checkpoint(a, b, networks):
    """Every tensor of every network file and all of ``adam.pth`` (moments, step counts, ``lr``), bit for bit."""
    for name in list(networks) + ["adam"]:
        _same_bits(torch.load(os.path.join(a, name + ".pth"), map_location="cpu"), torch.load(os.path.join(b, name + ".pth"), map_location="cpu"), name)


def _same_end(a, b, epoch, resumed_from, ranks=1, initial_best=10.0):
    """Summaries of an uninterrupted run ``a`` and a continued run ``b`` that both finished ``epoch``."""
    for k in range(ranks):
        sa, sb = _summary(a, k), _summary(b, k)
        assert sa["resumed_from"] is None and sb["resumed_from"] == resumed_from
        assert sa["param_checksum"] == sb["param_checksum"] and sa["best"] == sb["best"] and sa["steps"] == sb["steps"] > 0
        assert len(sa["items"]) == epoch + 1 and len(sb["items"]) == epoch + 1 - resumed_from
        assert sa["items"][resumed_from:] == sb["items"]         # the item order of the continued epochs
        assert np.isfinite(sa["param_checksum"]).all() and (k > 0 or sa["best"] < initial_best)       # rank 0's validations set it


def _adam(log, epoch):
    return torch.load(os.path.join(log, "models", "weights_%d" % epoch, "adam.pth"), map_location="cpu")


TRAINER_NETWORKS = ["encoder", "beam_encoder", "beam_encoder_pose", "depth", "pose_encoder", "pose"]


@pytest.fixture(scope="module")
def splits12(tree, tmp_path_factory):
    """The tree of tests/test_gpu_train_cli.py with a training split of 12 lines (its four, three times) and an Eigen test split of
    5 (its four and the first again: shares of 3 + 2 for two ranks)."""
    root, splits, lines, gts = tree
    d = str(tmp_path_factory.mktemp("splits12"))
    os.makedirs(os.path.join(d, "eigen_zhou"))
    os.makedirs(os.path.join(d, "eigen"))
    with open(os.path.join(d, "eigen_zhou", "train_files.txt"), "w") as f:
        f.write("\n".join(lines * 3) + "\n")
    with open(os.path.join(d, "eigen", "test_files.txt"), "w") as f:
        f.write("\n".join(lines + lines[:1]) + "\n")
    data = np.empty(5, dtype=object)
    for i, g in enumerate(list(gts) + [gts[0]]):
        data[i] = g
    np.savez_compressed(os.path.join(d, "eigen", "gt_depths.npz"), data=data)
    return d


# --------------------------------------------------------------------------------------------- (a) train, one process
@pytest.fixture(scope="module")
def train_runs(tree, splits12, tmp_path_factory):
    """Run A: epochs 0..2 in one process.  Run B: epochs 0..1, then ``--resume latest --num_epochs 3`` in a fresh process.
    --batch_size 6 --scheduler_step_size 1 derives a StepLR period of int(1 * 8 / 6) = 1 epoch: the rate drops after every epoch,
    before and after the point of resumption.  12 lines: 2 steps per epoch."""
    root, tmp_path = tree[0], tmp_path_factory.mktemp("train_runs")
    common = TC._flags(root, tmp_path, batch=6) + ["--scheduler_step_size", "1", "--log_frequency", "1", "--save_frequency", "1",
                                                    "--val_limit", "2", "--splits_dir", splits12, "--seed", "5"]
    _run("train", common + ["--model_name", "A", "--num_epochs", "3"])
    _run("train", common + ["--model_name", "B", "--num_epochs", "2"])
    a, b = os.path.join(str(tmp_path), "A"), os.path.join(str(tmp_path), "B")
    assert _summary(b)["steps"] == 4 and _summary(b)["resumed_from"] is None
    for k in (0, 1):                                             # the commit marker, in epoch checkpoints only
        assert os.path.isfile(os.path.join(b, "models", "weights_%d" % k, "run_state.rank0.pth"))
    assert os.path.isdir(os.path.join(b, "models", "weights_best")) and not os.path.exists(os.path.join(b, "models", "weights_best", "run_state.rank0.pth"))
    _run("train", common + ["--model_name", "B", "--num_epochs", "3", "--resume", "latest"])
    return a, b, common


def test_train_resumed_equals_uninterrupted(train_runs):
    a, b, _ = train_runs
    _same_checkpoint(os.path.join(a, "models", "weights_2"), os.path.join(b, "models", "weights_2"), TRAINER_NETWORKS)
    _same_end(a, b, 2, 2)
    assert _summary(a)["steps"] == 6 and _summary(b)["epochs"] == 1
    lrs = [_adam(a, k)["param_groups"][0]["lr"] for k in range(3)]
    assert lrs[2] < 0.11 * lrs[1] < 0.0111 * lrs[0] and lrs[2] == _adam(b, 2)["param_groups"][0]["lr"]     # dropped before and after
    assert float(_adam(a, 2)["state"][0]["step"]) == 6.0
    val_a = [json.loads(l) for l in open(os.path.join(a, "val", "scalars.jsonl"))]
    val_b = [json.loads(l) for l in open(os.path.join(b, "val", "scalars.jsonl"))]
    assert len(val_a) == len(val_b) == 6 and val_a == val_b      # every validation of the continued run, the rate it logged included


def test_resume_with_nothing_left_and_with_another_batch_size(train_runs, tree, splits12, tmp_path):
    a, b, common = train_runs
    root = tree[0]
    before = _summary(b)
    # nothing left to do: no step, and the summary is still written
    os.remove(os.path.join(b, "train_summary.rank0.json"))
    _run("train", common + ["--model_name", "B", "--num_epochs", "3", "--resume", os.path.join(b, "models", "weights_2")])
    s = _summary(b)
    assert s["resumed_from"] == 3 and s["epochs"] == 0 and s["items"] == [] and s["last_loss"] is None
    assert s["steps"] == 6 and s["param_checksum"] == before["param_checksum"] and s["best"] == before["best"]
    # a run that differs is refused before the first step, and the field is named
    r = subprocess.run([sys.executable, "-m", "fusiondepth_amd.train"] + TC._flags(root, os.path.dirname(b), batch=3) +
                       ["--model_name", "B", "--splits_dir", splits12, "--seed", "5", "--no_val", "--resume", "latest"],
                       env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert r.returncode != 0 and "ValueError: --resume: micro_batch differs" in r.stdout and "6" in r.stdout.split("micro_batch differs")[1]


# --------------------------------------------------------------------------------------------- (b) train, two ranks
def test_train_resumed_on_two_ranks(tree, splits12, tmp_path):
    root = tree[0]
    common = TC._flags(root, tmp_path) + ["--log_frequency", "1", "--save_frequency", "1", "--val_limit", "2", "--splits_dir", splits12,
                                          "--seed", "5"]
    _run("train", common + ["--model_name", "A", "--num_epochs", "2"], ranks=2)
    _run("train", common + ["--model_name", "B", "--num_epochs", "1"], ranks=2)
    a, b = os.path.join(str(tmp_path), "A"), os.path.join(str(tmp_path), "B")
    assert sorted(n for n in os.listdir(os.path.join(b, "models", "weights_0")) if n.startswith("run_state")) == \
        ["run_state.rank0.pth", "run_state.rank1.pth"]
    _run("train", common + ["--model_name", "B", "--num_epochs", "2", "--resume", "latest"], ranks=2)
    _same_checkpoint(os.path.join(a, "models", "weights_1"), os.path.join(b, "models", "weights_1"), TRAINER_NETWORKS)
    _same_end(a, b, 1, 1, ranks=2)
    s0, s1 = _summary(b, 0), _summary(b, 1)
    assert s0["param_checksum"] == s1["param_checksum"] and s0["steps"] == s1["steps"] == 6 and s0["world_size"] == 2
    assert not set(s0["items"][0]) & set(s1["items"][0])


# --------------------------------------------------------------------------------------------- (c) complete
def test_complete_resumed_equals_uninterrupted(completion, tmp_path):
    data, _ = completion
    def flags(name, epochs):
        return SC._complete_flags(data, str(tmp_path), name) + ["--completion_num_epochs", str(epochs), "--seed", "3", "--val_limit", "2",
                                                                "--save_frequency", "1"]
    _run("complete", flags("A", 2))
    _run("complete", flags("B", 1))
    _run("complete", flags("B", 2) + ["--resume", "latest"])
    a, b = os.path.join(str(tmp_path), "A"), os.path.join(str(tmp_path), "B")
    _same_checkpoint(os.path.join(a, "models", "weights_1"), os.path.join(b, "models", "weights_1"), TRAINER_NETWORKS)
    _same_end(a, b, 1, 1, initial_best=100000.0)
    assert _summary(a)["steps"] == 8


# --------------------------------------------------------------------------------------------- (d) refine
def test_refine_resumed_equals_uninterrupted(refine_tree, tmp_path):
    root, splits, lines, folder = refine_tree
    def flags(name, epochs):
        return SC._refine_flags(root, splits, folder, tmp_path, name) + ["--num_epochs", str(epochs), "--val_limit", "2",
                                                                          "--save_frequency", "1"]
    _run("refine", flags("A", 2))
    _run("refine", flags("B", 1))
    _run("refine", flags("B", 2) + ["--resume", "latest"])
    a, b = os.path.join(str(tmp_path), "A"), os.path.join(str(tmp_path), "B")
    last_a, last_b = os.path.join(a, "models", "weights_1"), os.path.join(b, "models", "weights_1")
    _same_checkpoint(last_a, last_b, TRAINER_NETWORKS + ["refine2d_decoder"])
    _same_end(a, b, 1, 1)
    assert _summary(a)["steps"] == 4
    for name in TRAINER_NETWORKS:                                # only refine2d_decoder changes: the frozen networks are stage 1's
        saved, kept = torch.load(os.path.join(folder, name + ".pth"), map_location="cpu"), torch.load(os.path.join(last_b, name + ".pth"), map_location="cpu")
        for k, v in kept.items():
            if torch.is_tensor(v):
                assert torch.equal(v, saved[k]), (name, k)
    first = torch.load(os.path.join(b, "models", "weights_0", "refine2d_decoder.pth"), map_location="cpu")
    final = torch.load(os.path.join(last_b, "refine2d_decoder.pth"), map_location="cpu")
    assert any(not torch.equal(first[k], final[k]) for k in first)


# --------------------------------------------------------------------------------------------- (e) --shard_val
def test_sharded_validation_equals_one_process(tree, splits12, tmp_path):
    """Two ranks validate 5 images as 3 + 2.  The last log event follows the last step of the epoch, so its validation saw the
    weights of ``weights_0``: one process that loads them and walks all 5 images must get the same bits for every metric."""
    from fusiondepth_amd import train as T
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.trainer import Trainer
    from fusiondepth_amd.validation import ValGroundTruth
    root = tree[0]
    flags = TC._flags(root, tmp_path) + ["--model_name", "S", "--num_epochs", "1", "--log_frequency", "1", "--save_frequency", "1"]
    _run("train", flags + ["--splits_dir", splits12, "--seed", "5", "--shard_val"], ranks=2)
    log = os.path.join(str(tmp_path), "S")
    s0, s1 = _summary(log, 0), _summary(log, 1)
    val = [json.loads(l) for l in open(os.path.join(log, "val", "scalars.jsonl"))]
    assert len(val) == 3                                         # rank 0 alone logged: one line per log event
    assert s0["best"] == s1["best"] == min(v["de/abs_rel"] for v in val) < 10.0
    assert s0["param_checksum"] == s1["param_checksum"]
    opt = MonodepthOptions().parse(flags + ["--train_load_weights_folder", os.path.join(log, "models", "weights_0")])
    tr = Trainer(opt, verbose=False)
    _, val_loader, gt_depths = T.build_loaders(tr.opt, splits12, batch_size=tr.batch_size)
    assert len(val_loader) == 5 and val_loader.batch_size == 1
    tr.val_gt = ValGroundTruth(gt_depths)
    try:
        whole = tr.val_metrics(val_loader)
    finally:
        val_loader.close()
    assert tr.last_val_rows.shape == (5, 9)
    for m in tr.depth_metric_names:
        print("%s: two ranks %r, one process %r" % (m, val[-1][m], float(whole[m])))
    for m in tr.depth_metric_names:
        assert val[-1][m] == float(whole[m]), m


# --------------------------------------------------------------------------------------------- (f) --weights_init pretrained
def test_pretrained_from_a_file(tree, tmp_path):
    from fusiondepth_amd import train as T
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.trainer import Trainer
    root, splits, lines, gts = tree
    hub = str(tmp_path / "hub")
    _, sd = IF.write(hub, 18)
    flags = TC._flags(root, tmp_path) + ["--model_name", "P"]

    def first_batch(tr):
        loader = T.build_loaders(tr.opt, splits, seed=5, no_val=True, batch_size=tr.batch_size)[0]
        it = iter(loader)
        try:
            return next(it)
        finally:
            it.close()
            loader.close()

    opt = MonodepthOptions().parse(flags + ["--weights_init", "pretrained"])
    opt.pretrained_path = hub                                    # what --pretrained_path sets
    torch.manual_seed(3)
    tr = Trainer(opt, verbose=False)
    flat = tr.flat.flat_param
    seen = 0
    for name in ("encoder", "beam_encoder", "beam_encoder_pose", "pose_encoder"):
        trunk = tr.models[name].encoder
        for key, p in trunk.named_parameters():
            lo = (p.data_ptr() - flat.data_ptr()) // 4
            assert 0 <= lo and lo + p.numel() <= flat.numel(), (name, key)       # a view of the flat buffer
            held = flat[lo:lo + p.numel()].view(p.shape).cpu()
            want = sd[key]
            if key == "conv1.weight" and name == "pose_encoder":
                want = torch.cat([want] * 2, 1) / 2
            if key == "conv1.weight" and name.startswith("beam"):
                assert held.shape == (64, 4 if name.endswith("pose") else 2, 7, 7) and float(held.std()) > 0
                continue
            assert torch.equal(held.view(torch.int32), want.contiguous().view(torch.int32)), (name, key)
            seen += 1
        for key, buf in trunk.named_buffers():
            assert torch.equal(buf.cpu(), sd[key]), (name, key)
    assert seen == 4 * 62 - 2                                    # 62 parameters per ResNet-18, two replaced stems
    folder = tr.save_model("init")
    losses = tr.train_step([first_batch(tr)])
    assert np.isfinite(float(losses["loss"]))
    after = flat.clone()
    assert torch.isfinite(after).all()
    del tr, flat
    # a scratch Trainer into which the same tensors are copied through load_model takes the same step
    opt = MonodepthOptions().parse(flags + ["--train_load_weights_folder", folder])
    torch.manual_seed(3)
    tr = Trainer(opt, verbose=False)
    tr.train_step([first_batch(tr)])
    assert torch.equal(tr.flat.flat_param.view(torch.int32), after.view(torch.int32))
