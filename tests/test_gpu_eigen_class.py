"""``evaluate_depth --per_semantic`` on the device: the per-class scorer (``fd_eigen_class_scores`` through
``evaluate_depth.eigen_class_scores``, ``fd_class_errors`` through ``functional.class_errors``) against its numpy restatement
(tests/eigen_class_ref.py), against the plain scorer it rides on, at its class-size and class-count edges, and the script end to end
on a synthetic KITTI tree.

Bounds, as in tests/test_gpu_eigen_eval.py: counts and threshold counts exactly; abs_rel, sq_rel and rmse within 1e-9 (float64 sums of
the same float32 terms in another order: n * 2^-53 at n <= 465 750 is 5.2e-11); rmse_log against the float64-logarithm restatement
within twice the error the float32 numpy restatement shows against it on the same classes (both printed in the terminal summary).

Measured on the MI355X: rmse_log per class 5.3e-08 (abs) from the float64-logarithm restatement for ``fd_eigen_class_scores`` against
3.4e-07 for the float32 numpy restatement (277 classes with pixels), 1.0e-07 against 1.8e-07 for ``fd_class_errors`` (138 classes);
``fd_class_errors`` on one image's host-rebuilt pairs equals the batched call's rows bit for bit - DESIGN.md section 19."""
import os

import numpy as np
import pytest
import torch

import conftest
import eigen_class_ref as CREF
import kitti_tree
from conftest import assert_close

pytestmark = pytest.mark.gpu

MODES = {"eigen-median": ("eigen", 1.0, False), "eigen-stereo": ("eigen", 5.4, True), "benchmark-median": ("eigen_benchmark", 1.0, False)}
K = 34
T = 256                                                          # the class kernel's thread count (CLASS_THREADS, csrc/score_lists.h)
F32 = np.float32


def _gt(rng, h, w, density=0.05):
    gt = rng.uniform(1.5, 90.0, (h, w)).astype(np.float32)
    if density < 1:
        gt[rng.rand(h, w) > density] = 0.0
    return gt


def _disp(rng, h, w):
    return rng.uniform(0.02, 0.6, (h, w)).astype(np.float32)


def _labels(rng, h, w):
    return rng.randint(0, 40, (h, w)).astype(np.uint8)           # some fall outside K = 34


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _class_scores(disps, gts, sems, mode, num_classes=K, **kw):
    from fusiondepth_amd import evaluate_depth as ED
    split, factor, no_median = MODES[mode]
    return ED.eigen_class_scores(torch.from_numpy(np.stack(disps)).cuda(), gts, sems, num_classes, split, factor, no_median, **kw)


def _plain_scores(disps, gts, mode):
    from fusiondepth_amd import evaluate_depth as ED
    split, factor, no_median = MODES[mode]
    return ED.eigen_scores(torch.from_numpy(np.stack(disps)).cuda(), gts, split, factor, no_median)


def _restate(disps, gts, sems, mode, num_classes=K):
    split, factor, no_median = MODES[mode]
    return CREF.restate_classes(disps, gts, sems, num_classes, split, factor, no_median)


@pytest.fixture(scope="module")
def mixed():
    """N = 4 maps of different sizes under 192x640 disparities: 17x90 (odd, down-sampled; every plane behind it starts off 4-byte
    alignment), 8x8, 370x1226 at 5 % and one fully valid 375x1242 plane (every row band, the longest lists).  The restatement of
    every mode is computed once and shared."""
    rng = np.random.RandomState(4321)
    gts = [_gt(rng, 17, 90), _gt(rng, 8, 8), _gt(rng, 370, 1226), _gt(rng, 375, 1242, 1.0)]
    disps = [_disp(rng, 192, 640) for _ in gts]
    sems = [_labels(rng, *g.shape) for g in gts]
    return {"disps": disps, "gts": gts, "sems": sems, "want": {mode: _restate(disps, gts, sems, mode) for mode in MODES}}


def _check_rows(cm, cc, want_counts, want_tc, want_m, what):
    """[.., K, 7] metrics and [.., K] counts against the restatement: counts and threshold counts exactly, the three order-only sums
    within 1e-9, zero rows where a class has no pixel."""
    assert cm.dtype == np.float64 and cc.dtype == np.int64 and cm.shape == want_m.shape and cc.shape == want_counts.shape
    assert np.array_equal(cc, want_counts), (what, cc, want_counts)
    scaled = cm[..., 4:] * cc[..., None]
    got_tc = np.rint(scaled).astype(np.int64)
    assert np.array_equal(got_tc, want_tc), (what, got_tc, want_tc)
    assert np.abs(scaled - got_tc).max(initial=0) < 1e-6
    assert (cm[cc == 0] == 0).all(), what
    assert_close(cm[..., :3], want_m[..., :3], rtol=1e-9, atol=0, what=what + ": abs_rel / sq_rel / rmse vs float64 sums of the float32 terms")


def _log_errors(cm, cc, want, log_errs):
    """(count, |mine - float64-log restatement|, |float32 numpy restatement - float64-log restatement|) of every class with pixels."""
    for idx in zip(*np.nonzero(cc > 0)):
        log_errs.append((cc[idx], abs(cm[idx][3] - want["metrics64"][idx][3]), abs(want["metrics"][idx][3] - want["metrics64"][idx][3])))


def _assert_log_rule(log_errs, what):
    assert len(log_errs) >= 10, (what, len(log_errs))
    mine, numpy32 = max(e[1] for e in log_errs), max(e[2] for e in log_errs)
    conftest.report("%s rmse_log per class vs the float64-log restatement (abs)" % what, mine, 2 * numpy32,
                    "(float32 numpy restatement %.2e, %d classes)" % (numpy32, len(log_errs)))
    assert mine <= 2 * numpy32, (what, mine, numpy32)


def test_class_scores_match_the_restatement(mixed):
    log_errs = []
    for mode in MODES:
        want = mixed["want"][mode]
        per, ratios, counts, cm, cc = _class_scores(mixed["disps"], mixed["gts"], mixed["sems"], mode)
        plain = _plain_scores(mixed["disps"], mixed["gts"], mode)
        for mine, theirs in zip((per, ratios, counts), plain):   # out is fd_eigen_scores' out, bit for bit
            assert mine.dtype == theirs.dtype and np.array_equal(_bits(mine), _bits(theirs)), mode
        assert cm.shape == (4, K, 7) and cc.shape == (4, K)
        _check_rows(cm, cc, want["counts"], want["thresh_counts"], want["metrics"], "mixed N=4 " + mode)
        _log_errors(cm, cc, want, log_errs)
        # per image, the classes partition the selected pixels whose label is below K
        assert np.array_equal(cc.sum(1), counts - want["outside"]) and (want["outside"][2:] > 0).all()
        got_tc = np.rint(cm[..., 4:] * cc[..., None]).astype(np.int64).sum(1)
        for i in range(4):
            th, out = want["image"]["terms"][i]["thresh"], want["labels"][i] >= K
            outside_tc = [int((th[out] < F32(1.25 ** k)).sum()) for k in (1, 2, 3)]
            assert np.array_equal(got_tc[i], want["image"]["thresh_counts"][i] - outside_tc), (mode, i)
    assert (mixed["want"]["eigen-median"]["counts"][3] > 1000).all()          # the long lists: every class of the dense plane
    _assert_log_rule(log_errs, "fd_eigen_class_scores")


def test_class_size_edges():
    """One 8x8 fully valid image, labels by hand: a class with 0 pixels (eight zeros), one with 1, one with 2, one with all the rest, and
    one pixel labelled 255 - outside K = 34, a class of its own at K = 256."""
    rng = np.random.RandomState(8)
    gt = rng.uniform(2.0, 70.0, (8, 8)).astype(np.float32)
    disp = _disp(rng, 8, 8)
    sem = np.full((8, 8), 1, np.uint8)
    sem[4, 2] = 3
    sem[3, 0], sem[6, 6] = 7, 7
    sem[5, 5] = 255
    for mode, total in (("eigen-median", 28), ("benchmark-median", 64)):      # the Garg window of 8x8: rows [3, 7), columns [0, 7)
        for num_classes in (K, 256):
            want = _restate([disp], [gt], [sem], mode, num_classes)
            per, ratios, counts, cm, cc = _class_scores([disp], [gt], [sem], mode, num_classes)
            assert counts.tolist() == [total]
            assert cc[0, 5] == 0 and (cm[0, 5] == 0).all() and cc[0, 3] == 1 and cc[0, 7] == 2 and cc[0, 1] == total - 4
            assert cc[0].sum() == total - (1 if num_classes == K else 0) and (num_classes == K or cc[0, 255] == 1)
            assert np.isfinite(cm).all()
            _check_rows(cm, cc, want["counts"], want["thresh_counts"], want["metrics"], "8x8 edges %s K=%d" % (mode, num_classes))
            assert_close(cm[..., 3], want["metrics64"][..., 3], rtol=0, atol=1e-6, what="8x8 edges: rmse_log")
            # one pixel: abs_rel is that pixel's term
            one = want["labels"][0] == 3
            assert cm[0, 3, 0] == np.float64(want["image"]["terms"][0]["abs_rel"][one][0])


@pytest.fixture(scope="module")
def small():
    """17x90, fully valid, under a 33x41 disparity; labels 0 .. 39 with a few 200s and 255s."""
    rng = np.random.RandomState(17)
    gt, disp, sem = _gt(rng, 17, 90, 1.0), _disp(rng, 33, 41), _labels(rng, 17, 90)
    sem[rng.rand(17, 90) < 0.02] = 200
    sem[rng.rand(17, 90) < 0.02] = 255
    return [disp], [gt], [sem]


@pytest.mark.parametrize("num_classes", [1, 34, 256])
def test_class_count_edges(small, num_classes):
    want = _restate(*small, "eigen-median", num_classes)
    per, ratios, counts, cm, cc = _class_scores(*small, "eigen-median", num_classes)
    assert cm.shape == (1, num_classes, 7) and cc.shape == (1, num_classes) and cc[0, 0] > 0
    _check_rows(cm, cc, want["counts"], want["thresh_counts"], want["metrics"], "17x90 K=%d" % num_classes)
    assert np.array_equal(cc.sum(1), counts - want["outside"])
    if num_classes == 256:
        assert want["outside"][0] == 0 and cc[0, 200] > 0 and cc[0, 255] > 0 and (cc[0, 40:200] == 0).all()
    plain = _plain_scores(small[0], small[1], "eigen-median")
    assert np.array_equal(_bits(per), _bits(plain[0]))


@pytest.mark.parametrize("num_classes", [0, 257])
def test_class_count_is_refused(small, num_classes):
    from fusiondepth_amd import functional as FD
    with pytest.raises(RuntimeError, match="fd_eigen_class_scores"):
        _class_scores(*small, "eigen-median", num_classes)
    g = torch.ones(5, device="cuda")
    with pytest.raises(RuntimeError, match="fd_class_errors"):
        FD.class_errors(g, g, torch.zeros(5, dtype=torch.uint8, device="cuda"), num_classes)


def test_nan_disparity_stays_in_its_image():
    rng = np.random.RandomState(21)
    gts = [_gt(rng, 20, 30, 0.5) for _ in range(3)]
    disps = [_disp(rng, 12, 16) for _ in range(3)]
    sems = [_labels(rng, 20, 30) for _ in range(3)]
    clean = _class_scores(disps, gts, sems, "eigen-median")
    bad = [d.copy() for d in disps]
    bad[1][:] = np.nan
    per, ratios, counts, cm, cc = _class_scores(bad, gts, sems, "eigen-median")
    assert np.array_equal(cc, clean[4]) and np.array_equal(counts, clean[2]) and (cc[1] > 0).sum() >= 10
    for i in (0, 2):
        assert np.array_equal(_bits(cm[i]), _bits(clean[3][i])) and np.array_equal(_bits(per[i]), _bits(clean[0][i]))
    some = cc[1] > 0
    assert np.isnan(cm[1][some][:, :4]).all() and (cm[1][some][:, 4:] == 0).all() and (cm[1][~some] == 0).all()
    assert np.isnan(per[1, :4]).all() and (per[1, 4:] == 0).all()


def test_two_calls_are_bitwise_equal(mixed):
    a = _class_scores(mixed["disps"], mixed["gts"], mixed["sems"], "eigen-median")
    b = _class_scores(mixed["disps"], mixed["gts"], mixed["sems"], "eigen-median")
    c = _class_scores(mixed["disps"], mixed["gts"], mixed["sems"], "eigen-median", chunk=3)     # 3 + 1 images per call: the same rows
    for x, y, z in zip(a, b, c):
        assert np.array_equal(_bits(x), _bits(y)) and np.array_equal(_bits(x), _bits(z))


# ---------------------------------------------------------------------------------------------------------------- fd_class_errors
def _list_errors(g, p, labels, num_classes=K, lo=1e-3, hi=80):
    from fusiondepth_amd import functional as FD
    out = FD.class_errors(torch.from_numpy(g).cuda(), torch.from_numpy(p).cuda(), torch.from_numpy(labels).cuda(), num_classes, lo, hi)
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (num_classes, 8)
    return out.cpu().numpy()


def test_class_errors_on_lists():
    """n = 0, 1, 2 and around the thread count T (a thread with no pair, one pair each, a second pair for thread 0), then 70 001:
    about 270 pairs per thread.  Predictions reach past both clamps."""
    rng = np.random.RandomState(5)
    log_errs = []
    for n in (0, 1, 2, T - 1, T, T + 1, 70001):
        g = rng.uniform(1.5, 79.0, n).astype(np.float32)
        p = rng.uniform(0.0005, 100.0, n).astype(np.float32)
        labels = rng.randint(0, 40, n).astype(np.uint8)
        counts, tcs, rows, rows64 = CREF.class_rows(CREF.pair_terms(g, p), labels, K)
        got = _list_errors(g, p, labels)
        cm, cc = got[:, :7].copy(), got[:, 7].astype(np.int64)
        assert np.array_equal(got[:, 7], cc)
        _check_rows(cm, cc, counts, tcs, rows, "lists n=%d" % n)
        _log_errors(cm, cc, {"metrics": rows, "metrics64": rows64}, log_errs)
        again = _list_errors(g, p, labels)
        assert np.array_equal(_bits(got), _bits(again))
        if n == 0:
            assert (got == 0).all()
    assert (p < 1e-3).any() and (p > 80).any()
    _assert_log_rule(log_errs, "fd_class_errors")
    # a NaN prediction: NaN in the first four columns of its class, 0 in a1-a3, every other class untouched
    at = int(np.nonzero(labels < K)[0][100])
    p_nan = p.copy()
    p_nan[at] = np.nan
    bad = _list_errors(g, p_nan, labels)
    c = int(labels[at])
    assert np.isnan(bad[c, :4]).all() and bad[c, 7] == got[c, 7] and np.isfinite(bad[c, 4:7]).all()
    rest = np.arange(K) != c
    assert np.array_equal(_bits(bad[rest]), _bits(got[rest]))


def test_class_errors_equal_the_image_rows_bit_for_bit(mixed):
    """The pairs of one image (370x1226, 5 %), rebuilt on the host as the restatement forms them - ``gt[mask]`` and
    ``(pred * ratio)[mask]``, each step one float32 rounding, the operations the compact kernel and the class kernel make on the device -
    and handed to ``fd_class_errors`` with ``lo`` and ``hi``: the same workgroup shape, thread stride and tree, so the same bits as the
    image's rows from ``fd_eigen_class_scores``."""
    i = 2
    per, ratios, counts, cm, cc = _class_scores(mixed["disps"], mixed["gts"], mixed["sems"], "eigen-median")
    want = mixed["want"]["eigen-median"]
    assert np.array_equal(ratios.view(np.uint32), want["image"]["ratios"].view(np.uint32))
    g, p = CREF.scaled_pairs(mixed["disps"][i], mixed["gts"][i], ratios[i], "eigen", 1.0)
    assert g.size == counts[i] and g.size > 10000
    got = _list_errors(g, p, want["labels"][i])
    assert np.array_equal(got[:, 7].astype(np.int64), cc[i])
    rel = np.abs(got[:, :7] - cm[i]) / np.maximum(np.abs(cm[i]), 1e-300)
    conftest.report("fd_class_errors vs fd_eigen_class_scores on one image's pairs (rel; 0 = bit-equal)", rel.max(), 0.0)
    assert np.array_equal(_bits(got[:, :7]), _bits(cm[i]))


# ---------------------------------------------------------------------------------------------------------------- the script
H, W = 192, 640
SIZES = {"2011_09_26": (375, 1242), "2011_09_30": (370, 1226)}


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """A ``Trainer.save_model`` folder from a seeded random ResNet-18 (the recipe of tests/test_gpu_eigen_eval.py)."""
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.trainer import Trainer
    tmp = tmp_path_factory.mktemp("eigen_class_models")
    common = ["--num_layers", "18", "--weights_init", "scratch", "--batch_size", "2", "--height", str(H), "--width", str(W)]
    torch.manual_seed(5)
    net = Trainer(MonodepthOptions().parse(common + ["--log_dir", str(tmp / "stage1")]), verbose=False)
    saved = net.save_model("init")
    del net
    return saved


def _write_split(splits, lines, root, beams=False):
    from fusiondepth_amd import kitti_utils as KU
    os.makedirs(os.path.join(splits, "eigen"))
    with open(os.path.join(splits, "eigen", "test_files.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    gts = KU.export_gt_depths(root, lines, "eigen", os.path.join(splits, "eigen", "gt_depths.npz"))
    if beams:
        KU.export_gt_depths(root, lines, "4beam", os.path.join(splits, "eigen", "4beam.npz"))
    return gts


def _write_masks(folder, gts, seed):
    from PIL import Image
    rng = np.random.RandomState(seed)
    sems = [_labels(rng, *g.shape) for g in gts]
    for i, s in enumerate(sems):
        Image.fromarray(s).save(os.path.join(folder, "pred_mask%d.png" % i))
    return sems


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    """A two-drive tree with different image sizes; its split file and ``gt_depths.npz``; a second split of one frame per drive with
    the ``4beam.npz`` that --eval_gdc reads; label masks as PNGs for both."""
    root = str(tmp_path_factory.mktemp("kitti"))
    lines = kitti_tree.make_tree(root, [("2011_09_26", "2011_09_26_drive_0001_sync", SIZES["2011_09_26"], (1.0, 1.0)),
                                        ("2011_09_30", "2011_09_30_drive_0016_sync", SIZES["2011_09_30"], (1.0, 1.0))], frames=4, down=0.35)
    assert len(lines) == 4
    out = {"root": root, "lines": lines}
    for name, sel, beams in (("all", lines, False), ("gdc", [lines[0], lines[3]], True)):
        splits, masks = str(tmp_path_factory.mktemp("splits_" + name)), str(tmp_path_factory.mktemp("masks_" + name))
        gts = _write_split(splits, sel, root, beams)
        assert [g.shape for g in gts] == [SIZES[l.split("/")[0]] for l in sel]
        out[name] = {"splits": splits, "masks": masks, "gts": gts, "sems": _write_masks(masks, gts, 99)}
    return out


def _eval_opt(root, folder, *extra):
    from fusiondepth_amd.options import MonodepthOptions
    return MonodepthOptions().parse(["--num_layers", "18", "--data_path", root, "--png", "--load_weights_folder", folder, "--eval_mono",
                                     "--eval_batch_size", "3"] + list(extra))


def _check_files(out_dir, run_name, result, n):
    from fusiondepth_amd import evaluate_depth as ED
    sem = result[3]
    assert set(sem) == {"abs_rel", "pixel_count", "metrics"}
    saved, pixels = np.load(os.path.join(out_dir, run_name + ".npy")), np.load(os.path.join(out_dir, "pixel_count.npy"))
    assert saved.shape == (34,) and pixels.shape == (34, n) and sem["metrics"].shape == (n, 34, 7)
    assert np.array_equal(saved, sem["abs_rel"]) and np.array_equal(pixels, sem["pixel_count"])
    assert np.array_equal(_bits(saved), _bits(ED.semantic_summary(sem["metrics"], sem["pixel_count"].T.astype(np.int64))))
    assert_close(saved, CREF.summary(sem["metrics"], sem["pixel_count"].T), rtol=1e-12, atol=0, what="the summary of :492-494")
    return sem, pixels


def test_script_end_to_end(folder, split, tmp_path, capsys):
    from fusiondepth_amd import evaluate_depth as ED
    root, s = split["root"], split["all"]
    N = len(s["gts"])
    plain = ED.evaluate(_eval_opt(root, folder, "--save_pred_disps"), s["splits"])
    assert len(plain) == 3
    capsys.readouterr()
    out_dir = str(tmp_path / "out")
    got = ED.evaluate(_eval_opt(root, folder, "--per_semantic", "--run_name", "r"), s["splits"], s["masks"], out_dir)
    printed = capsys.readouterr().out
    assert len(got) == 4
    for a, b in zip(got[:3], plain):                             # the flag changes nothing it does not add
        assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))
    sem, pixels = _check_files(out_dir, "r", got, N)
    want_counts = np.stack([[int((m[CREF.split_mask(g, "eigen")] == c).sum()) for c in range(34)] for g, m in zip(s["gts"], s["sems"])])
    assert np.array_equal(pixels, want_counts.T) and (pixels.sum(1) > 0).sum() >= 10
    assert np.isfinite(sem["metrics"]).all() and (sem["abs_rel"][pixels.sum(1) > 0] > 0).all()
    lines = [ln for ln in printed.splitlines() if ln.strip() and ln.split("|")[0].strip().isdigit()]
    assert [int(ln.split("|")[0]) for ln in lines] == np.nonzero(pixels.sum(1) > 0)[0].tolist()        # one line per class with pixels
    # the command line: the two folders are taken off before the options are parsed; --run_name unset names the file per_semantic.npy
    saved = os.path.join(folder, "disps_eigen_split.npy")
    cli_dir = str(tmp_path / "cli")
    cli = ED.main(["--splits_dir", s["splits"], "--semantic_dir", s["masks"], "--semantic_out", cli_dir, "--eval_mono", "--per_semantic",
                   "--ext_disp_to_eval", saved])
    assert np.array_equal(_bits(cli[2]), _bits(plain[2])) and np.array_equal(_bits(cli[3]["metrics"]), _bits(sem["metrics"]))
    _check_files(cli_dir, "per_semantic", cli, N)


def test_script_with_gdc(folder, split, tmp_path):
    """--eval_gdc on two images: the classes are scored from the corrected dense map (``functional.class_errors``); the mask does not
    depend on GDC, so the counts are the restatement's."""
    from fusiondepth_amd import evaluate_depth as ED
    root, s = split["root"], split["gdc"]
    out_dir = str(tmp_path / "out")
    got = ED.evaluate(_eval_opt(root, folder, "--eval_gdc", "--per_semantic", "--run_name", "g"), s["splits"], s["masks"], out_dir)
    assert len(got) == 4 and got[2] is None and len(got[1]) == 2 and np.isfinite(got[0]).all()
    sem, pixels = _check_files(out_dir, "g", got, 2)
    want_counts = np.stack([[int((m[CREF.split_mask(g, "eigen")] == c).sum()) for c in range(34)] for g, m in zip(s["gts"], s["sems"])])
    assert np.array_equal(pixels, want_counts.T) and (want_counts > 0).any()
    assert np.isfinite(sem["metrics"]).all() and (sem["metrics"][want_counts > 0][:, :4] > 0).all() and (sem["metrics"][want_counts == 0] == 0).all()
