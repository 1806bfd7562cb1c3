"""The host side of the Eigen-split evaluation (fusiondepth_amd/evaluate_depth.py): ground-truth packing, what the script refuses, its
command line, the benchmark PNG values and the ABI 8 binding.  No GPU is touched."""
import ctypes

import numpy as np
import pytest


def _opt(*flags):
    from fusiondepth_amd.options import MonodepthOptions
    return MonodepthOptions().parse(list(flags))


def test_pack_gt_depths_mixed_sizes():
    from fusiondepth_amd import _lib
    from fusiondepth_amd import evaluate_depth as ED
    assert ED.EIGEN_DESC.itemsize == ctypes.sizeof(_lib.EigenDesc) == 40
    for name in ED.EIGEN_DESC.names:
        assert ED.EIGEN_DESC.fields[name][1] == getattr(_lib.EigenDesc, name).offset, name
    rng = np.random.RandomState(3)
    sizes = [(375, 1242), (370, 1226), (17, 90), (375, 1242)]
    gts = [rng.uniform(0, 90, s).astype(np.float32 if i % 2 else np.float64) for i, s in enumerate(sizes)]
    packed, desc = ED.pack_gt_depths(gts, "eigen")
    assert packed.dtype.is_floating_point and packed.element_size() == 4 and packed.numel() == sum(h * w for h, w in sizes)
    assert not packed.is_cuda and len(desc) == 4
    at = 0
    for i, ((h, w), g) in enumerate(zip(sizes, gts)):
        d = desc[i]
        assert (d["offset"], d["H"], d["W"], d["pred"]) == (at, h, w, i)
        assert (d["y0"], d["y1"], d["x0"], d["x1"]) == tuple(ED.garg_crop(h, w))
        assert np.array_equal(packed[at:at + h * w].numpy().reshape(h, w), g.astype(np.float32))
        at += h * w
    assert tuple(desc[2][["y0", "y1", "x0", "x1"]]) == (6, 16, 3, 86) and desc[2]["offset"] % 4 != 0      # off 16-byte alignment
    assert tuple(desc[0][["y0", "y1", "x0", "x1"]]) == (153, 371, 44, 1197)
    # every other split: the whole map, gt > 0 with no upper bound
    _, whole = ED.pack_gt_depths(gts, "eigen_benchmark")
    for (h, w), d in zip(sizes, whole):
        assert (d["y0"], d["y1"], d["x0"], d["x1"]) == (0, h, 0, w)
    assert ED.split_bounds("eigen") == (1e-3, 80.0) and ED.split_bounds("eigen_benchmark") == (0.0, float("inf"))
    with pytest.raises(ValueError, match="non-empty"):
        ED.pack_gt_depths([np.zeros((3,))], "eigen")


def test_evaluate_refuses_what_it_does_not_cover(monkeypatch):
    import torch
    from fusiondepth_amd import evaluate_depth as ED

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the refusal")

    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    monkeypatch.setattr(torch.Tensor, "cuda", no_gpu)
    for flags in ([], ["--eval_mono", "--eval_stereo"]):
        with pytest.raises(ValueError, match="eval_mono or --eval_stereo"):
            ED.evaluate(_opt(*flags))
    for flags, word in ((["--visualize"], "visualize"), (["--per_semantic"], "per_semantic"), (["--save_sample", "3"], "save_sample"),
                        (["--demo"], "demo"), (["--eval_split", "odom_9"], "odometry"), (["--eval_split", "odom_10"], "odometry"),
                        (["--beam_encoder"], "beam encoder"), (["--cat2end", "--refine_2d"], "cat2end"),
                        (["--ext_disp_to_eval", "x.npy", "--eval_gdc"], "eval_gdc")):
        with pytest.raises(NotImplementedError, match=word):
            ED.evaluate(_opt("--eval_mono", *flags))
    # evaluate_completion keeps its own refusal of --refine_2d
    from fusiondepth_amd import evaluate_completion as EC
    with pytest.raises(NotImplementedError, match="refine_2d"):
        EC.evaluate(_opt("--eval_mono", "--refine_2d"))


def test_splits_dir_is_taken_off_the_command_line():
    from fusiondepth_amd import evaluate_depth as ED
    from fusiondepth_amd.options import MonodepthOptions
    argv = ["--eval_mono", "--splits_dir", "/data/splits", "--png", "--eval_split", "eigen_benchmark"]
    d, rest = ED.split_off_splits_dir(argv)
    assert d == "/data/splits" and rest == ["--eval_mono", "--png", "--eval_split", "eigen_benchmark"]
    o = MonodepthOptions().parse(rest)
    assert o.eval_mono and o.png and o.eval_split == "eigen_benchmark" and not hasattr(o, "splits_dir")
    assert ED.split_off_splits_dir(["--splits_dir=s2", "--eval_stereo"]) == ("s2", ["--eval_stereo"])
    assert ED.split_off_splits_dir(["--eval_stereo"]) == ("splits", ["--eval_stereo"])
    with pytest.raises(ValueError, match="needs a value"):
        ED.split_off_splits_dir(["--eval_mono", "--splits_dir"])
    with pytest.raises(SystemExit):                              # the options surface itself does not know the flag
        MonodepthOptions().parse(argv)


def test_benchmark_png_values():
    from fusiondepth_amd import evaluate_depth as ED
    disp = np.array([[5.4, 0.54, 0.0675, 0.01, 1e9, 2.7]], np.float32)
    got = ED.benchmark_depth_png(disp)
    assert got.dtype == np.uint16 and got.shape == disp.shape
    # 5.4 / disp, clipped to 0 .. 80, * 256, truncated: 1 m, 10 m, 80 m, 540 m -> 80 m, ~0, 2 m
    want = np.uint16(np.clip(np.float32(5.4) / disp, 0, 80) * 256)
    assert np.array_equal(got, want)
    assert got[0, 0] in (255, 256) and got[0, 2] == 20480 and got[0, 3] == 20480 and got[0, 4] == 0 and got[0, 5] == 512


def test_abi_8_binding():
    from fusiondepth_amd import _lib
    assert _lib.ABI_VERSION == 8
    assert _lib.SIGNATURES["fd_eigen_scores_ws_bytes"] == ("iil", "l")
    args, res = _lib.SIGNATURES["fd_eigen_scores"]
    assert res == "i" and len(args) == 19 and args[-1] == "p"
    header = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "fdhip.h")).read()
    assert "#define FD_ABI_VERSION 8" in header and "fd_eigen_desc" in header
