"""The Eigen-split evaluation on the device: the batched scorer (``fd_eigen_scores`` through ``evaluate_depth.eigen_scores``) against its
numpy restatement (tests/eigen_eval_ref.py) and against the per-image loop it stands beside, its edges, stage-2 prediction
(``Predictor(refine_2d=True)``) against the Refiner, and the script end to end on a synthetic KITTI tree.

rmse_log, measured on the MI355X (printed in the terminal summary): the worst absolute error over the images of the restatement test
against the float64-logarithm restatement, beside the error the float32 numpy restatement shows on the same inputs - DESIGN.md
section 14 records both."""
import os

import numpy as np
import pytest
import torch

import conftest
import eigen_eval_ref as REF
import inputs as gin
import kitti_tree
from conftest import assert_close

pytestmark = pytest.mark.gpu

MODES = {"eigen-median": ("eigen", 1.0, False), "eigen-stereo": ("eigen", 5.4, True), "benchmark-median": ("eigen_benchmark", 1.0, False)}


def _gt(rng, h, w, density=0.05):
    gt = rng.uniform(1.5, 90.0, (h, w)).astype(np.float32)
    if density < 1:
        gt[rng.rand(h, w) > density] = 0.0
    return gt


def _disp(rng, h, w):
    return rng.uniform(0.02, 0.6, (h, w)).astype(np.float32)


@pytest.fixture(scope="module")
def cases():
    """One call takes disparities of ONE size and ground truth of any sizes.  ``mixed``: N = 5 maps of different sizes (17x90: odd,
    down-sampled, its plane and the one behind it off 16-byte alignment; 8x8; the two KITTI sizes; one fully valid 375x1242 plane,
    ~251 k selected pixels: every row band and every partial sum) under 192x640 disparities.  ``alone``: the N = 1 calls, each
    with the disparity size named for it (33x41 -> 17x90, 8x8 -> 8x8 the identity, 192x640 -> the KITTI sizes).  5 % of the
    ground truth is valid; ``dense`` adds the two small pairs fully valid, where 5 % leaves a handful of pixels."""
    rng = np.random.RandomState(1234)
    c = {"mixed": ([_disp(rng, 192, 640) for _ in range(5)],
                   [_gt(rng, 17, 90), _gt(rng, 375, 1242), _gt(rng, 8, 8), _gt(rng, 370, 1226), _gt(rng, 375, 1242, 1.0)])}
    c["alone"] = [([_disp(rng, 33, 41)], [_gt(rng, 17, 90)]), ([_disp(rng, 8, 8)], [_gt(rng, 8, 8)]),
                  ([_disp(rng, 192, 640)], [_gt(rng, 375, 1242)]), ([_disp(rng, 192, 640)], [_gt(rng, 370, 1226)]),
                  ([_disp(rng, 192, 640)], [_gt(rng, 375, 1242, 1.0)])]
    c["dense"] = [([_disp(rng, 33, 41)], [_gt(rng, 17, 90, 1.0)]), ([_disp(rng, 8, 8)], [_gt(rng, 8, 8, 1.0)])]
    return c


def _score(disps, gts, mode, **kw):
    from fusiondepth_amd import evaluate_depth as ED
    split, factor, no_median = MODES[mode]
    return ED.eigen_scores(torch.from_numpy(np.stack(disps)).cuda(), gts, split, factor, no_median, **kw)


def _check_against_restatement(disps, gts, mode, what, log_errs):
    split, factor, no_median = MODES[mode]
    want = REF.restate(disps, gts, split, factor, no_median)
    per, ratios, counts = _score(disps, gts, mode)
    assert per.shape == (len(gts), 7) and per.dtype == np.float64 and counts.dtype == np.int64
    assert np.array_equal(counts, want["counts"]), (what, counts, want["counts"])
    if no_median:
        assert ratios.shape == (0,)
    else:
        assert ratios.dtype == np.float32 and np.array_equal(ratios.view(np.uint32), want["ratios"].view(np.uint32)), (what, ratios, want["ratios"])
    some = counts > 0
    got_tc = np.rint(per[some, 4:] * counts[some, None]).astype(np.int64)
    assert np.array_equal(got_tc, want["thresh_counts"][some]), (what, got_tc, want["thresh_counts"][some])
    assert np.abs(per[some, 4:] * counts[some, None] - got_tc).max(initial=0) < 1e-6
    assert np.isnan(per[~some]).all()
    assert_close(per[:, :3], want["metrics"][:, :3], rtol=1e-9, atol=0, what=what + ": abs_rel / sq_rel / rmse vs float64 sums of the float32 terms")
    for i in np.nonzero(some)[0]:
        log_errs.append((counts[i], abs(per[i, 3] - want["metrics64"][i, 3]), abs(want["metrics"][i, 3] - want["metrics64"][i, 3])))
    return per, ratios, counts


def test_scorer_matches_the_restatement(cases):
    """Counts, ratios and threshold counts exactly; the three sums that differ from the restatement by summation order alone within
    1e-9 (n * 2^-53 at n <= 465 750 is 5.2e-11); rmse_log against the float64-logarithm restatement within twice the error the float32
    numpy restatement shows against it on the same images - over all images, and over those with >= 1000 pixels alone."""
    log_errs = []
    for mode in MODES:
        _check_against_restatement(*cases["mixed"], mode, "mixed N=5 " + mode, log_errs)
    for k, (disps, gts) in enumerate(cases["alone"] + cases["dense"]):
        _check_against_restatement(disps, gts, "eigen-median", "alone %d" % k, log_errs)
        _check_against_restatement(disps, gts, "eigen-stereo", "alone %d stereo" % k, log_errs)
    for name, sel in (("all images", [e for e in log_errs]), ("images of >= 1000 pixels", [e for e in log_errs if e[0] >= 1000])):
        assert len(sel) >= 10
        mine, numpy32 = max(e[1] for e in sel), max(e[2] for e in sel)
        conftest.report("fd_eigen_scores rmse_log vs the float64-log restatement, %s (abs)" % name, mine, 2 * numpy32,
                        "(float32 numpy restatement %.2e)" % numpy32)
        assert mine <= 2 * numpy32, (name, mine, numpy32)


@pytest.mark.parametrize("mode", list(MODES))
def test_scorer_matches_the_per_image_loop(mode):
    """Against ``evaluate_predictions`` (the ATen loop that stays for --eval_gdc) at the bounds that loop is held to against the oracle."""
    from fusiondepth_amd import evaluate_depth as ED
    split, factor, no_median = MODES[mode]
    rng = np.random.RandomState(77)
    gts = [_gt(rng, h, w) for h, w in ((375, 1242), (370, 1226), (375, 1242))]
    disps = [_disp(rng, 192, 640) for _ in gts]
    want, want_r = ED.evaluate_predictions(torch.from_numpy(np.stack(disps)).cuda(), gts, split, factor, no_median)
    per, ratios, _ = _score(disps, gts, mode)
    got = per.mean(0)
    assert_close(got[:4], want[:4], rtol=5e-5, atol=0, what="mean abs_rel / sq_rel / rmse / rmse_log")
    assert_close(got[4:], want[4:], rtol=0, atol=3e-4, what="mean a1 / a2 / a3")
    assert_close(ratios, want_r, rtol=1e-5, atol=0, what="ratios")
    assert (len(ratios) == 3) == (not no_median)


# a 20 x 30 map: Garg window rows [8, 19), columns [1, 28)
EH, EW, EY0, EY1, EX0, EX1 = 20, 30, 8, 19, 1, 28


def _edge(points):
    gt = np.zeros((EH, EW), np.float32)
    for (y, x), v in points.items():
        gt[y, x] = v
    return gt


def _edge_call(gts, disps=None, mode="eigen-median"):
    rng = np.random.RandomState(9)
    disps = [_disp(rng, 12, 16) for _ in gts] if disps is None else disps
    split, factor, no_median = MODES[mode]
    return _score(disps, gts, mode), REF.restate(disps, gts, split, factor, no_median), disps


def test_window_is_the_garg_crop():
    from fusiondepth_amd import evaluate_depth as ED
    assert tuple(ED.garg_crop(EH, EW)) == (EY0, EY1, EX0, EX1)


def test_edge_zero_one_and_two_pixels():
    """No pixel: a NaN row, count 0; one: the odd median is the pixel; two: the even median is the float32 mean of two different values."""
    gts = [_edge({}), _edge({(10, 5): 7.5}), _edge({(10, 5): 7.5, (15, 20): 31.0})]
    (per, ratios, counts), want, _ = _edge_call(gts)
    assert counts.tolist() == [0, 1, 2]
    assert np.isnan(per[0]).all() and np.isnan(ratios[0]) and np.isfinite(per[1:]).all()
    assert np.array_equal(ratios.view(np.uint32), want["ratios"].view(np.uint32))
    assert want["terms"][2]["thresh"].size == 2
    assert_close(per[:, :3], want["metrics"][:, :3], rtol=1e-9, atol=0, what="0 / 1 / 2 pixels")
    assert np.array_equal(np.rint(per[1:, 4:] * counts[1:, None]), want["thresh_counts"][1:])


def test_edge_strict_ground_truth_bounds():
    """gt == float32(1e-3) and gt == 80 are excluded by the strict comparisons; their float32 neighbours inside are selected."""
    lo, hi = np.float32(1e-3), np.float32(80)
    gts = [_edge({(10, 5): lo, (10, 6): hi, (12, 7): 20.0}),
           _edge({(10, 5): np.nextafter(lo, np.float32(1)), (10, 6): np.nextafter(hi, np.float32(0)), (12, 7): 20.0})]
    (per, ratios, counts), want, _ = _edge_call(gts)
    assert counts.tolist() == [1, 3] and want["counts"].tolist() == [1, 3]
    assert np.array_equal(ratios.view(np.uint32), want["ratios"].view(np.uint32))
    # the other splits select gt > 0 with no upper bound
    (per, ratios, counts), want, _ = _edge_call([_edge({(0, 0): 1e-4, (19, 29): 500.0, (3, 3): 0.0})], mode="benchmark-median")
    assert counts.tolist() == [2] and want["counts"].tolist() == [2]


def test_edge_window_rows_and_columns():
    """Rows y0 and y1 - 1 and columns x0 and x1 - 1 are inside; rows y0 - 1 and y1 and columns x0 - 1 and x1 are outside."""
    inside = {(EY0, 10): 5.0, (EY1 - 1, 11): 6.0, (12, EX0): 7.0, (13, EX1 - 1): 8.0, (EY0, EX0): 9.0, (EY1 - 1, EX1 - 1): 10.0}
    outside = {(EY0 - 1, 10): 11.0, (EY1, 11): 12.0, (12, EX0 - 1): 13.0, (13, EX1): 14.0, (EY1, EX1): 15.0, (0, 0): 16.0, (EH - 1, EW - 1): 17.0}
    d = _disp(np.random.RandomState(10), 12, 16)               # images 0 and 2 share a disparity: only the outside pixels differ
    (per, ratios, counts), want, _ = _edge_call([_edge({**inside, **outside}), _edge(outside), _edge(inside)], [d, d + np.float32(0.1), d])
    assert counts.tolist() == [6, 0, 6] and want["counts"].tolist() == [6, 0, 6]
    assert np.array_equal(per[0].view(np.uint64), per[2].view(np.uint64)) and np.isnan(per[1]).all()
    assert np.array_equal(ratios.view(np.uint32), want["ratios"].view(np.uint32))
    assert_close(per[:, :3], want["metrics"][:, :3], rtol=1e-9, atol=0, what="window borders")


def test_edge_predictions_clamp_at_both_ends():
    """Without median scaling: a disparity of 1e5 is 1e-5 m -> 1e-3; one of 1e-3 is 1000 m -> 80."""
    gts = [_edge({(10, 5): 10.0, (15, 20): 10.0}), _edge({(10, 5): 10.0, (15, 20): 10.0})]
    disps = [np.full((12, 16), 1e5, np.float32), np.full((12, 16), 1e-3, np.float32)]
    split, factor, no_median = "eigen", 1.0, True
    from fusiondepth_amd import evaluate_depth as ED
    per, ratios, counts = ED.eigen_scores(torch.from_numpy(np.stack(disps)).cuda(), gts, split, factor, no_median)
    want = REF.restate(disps, gts, split, factor, no_median)
    assert counts.tolist() == [2, 2] and ratios.size == 0
    assert_close(per[:, :3], want["metrics"][:, :3], rtol=1e-9, atol=0, what="clamped predictions")
    assert_close(per[:, 3], want["metrics64"][:, 3], rtol=1e-7, atol=0, what="clamped predictions, rmse_log")
    assert_close(per[:, 2], [10.0 - np.float64(np.float32(1e-3)), 70.0], rtol=1e-6, atol=0, what="rmse at the clamps")
    assert (per[:, 4:] == 0).all()


def test_edge_nan_disparity_stays_in_its_image():
    rng = np.random.RandomState(21)
    gts = [_gt(rng, EH, EW, 0.5) for _ in range(3)]
    disps = [_disp(rng, 12, 16) for _ in range(3)]
    clean, _, _ = _edge_call(gts, disps)
    bad = [d.copy() for d in disps]
    bad[1][:] = np.nan                                          # every tap of every selected pixel of image 1
    (per, ratios, counts), want, _ = _edge_call(gts, bad)
    assert counts.tolist() == clean[2].tolist() and counts[1] > 0
    assert np.isnan(per[1, :4]).all() and np.isnan(ratios[1]) and (per[1, 4:] == 0).all()
    assert np.array_equal(np.isnan(per), np.isnan(want["metrics"]))
    for i in (0, 2):
        assert np.array_equal(per[i].view(np.uint64), clean[0][i].view(np.uint64)) and ratios[i] == clean[1][i]
    # one NaN tap: still that image alone
    one = [d.copy() for d in disps]
    y, x = [int(v[0]) for v in np.nonzero((gts[1] > 1e-3) & (gts[1] < 80) & (np.arange(EH)[:, None] >= EY0) & (np.arange(EH)[:, None] < EY1)
                                          & (np.arange(EW)[None] >= EX0) & (np.arange(EW)[None] < EX1))]
    one[1][min(int((y + 0.5) * 12 / EH), 11), min(int((x + 0.5) * 16 / EW), 15)] = np.nan
    (per1, ratios1, _), want1, _ = _edge_call(gts, one)
    assert np.array_equal(np.isnan(per1), np.isnan(want1["metrics"])) and np.isnan(per1[1, 0])
    assert np.array_equal(per1[0].view(np.uint64), clean[0][0].view(np.uint64)) and np.array_equal(per1[2].view(np.uint64), clean[0][2].view(np.uint64))


def test_two_calls_are_bitwise_equal(cases):
    a = _score(*cases["mixed"], "eigen-median")
    b = _score(*cases["mixed"], "eigen-median")
    c = _score(*cases["mixed"], "eigen-median", chunk=2)        # 2 + 2 + 1 images per call: the same rows
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)) and np.array_equal(x.view(np.uint8), z.view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------- stage-2 prediction
H, W = 192, 640


def _save(o, cls, name):
    net = cls(o, verbose=False)
    folder = net.save_model(name)
    del net
    return folder


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """A ``Trainer.save_model`` folder from a seeded random ResNet-18 and ``Refiner.save_model`` folders on top of it, by refine variant."""
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.refiner import Refiner
    from fusiondepth_amd.trainer import Trainer
    tmp = tmp_path_factory.mktemp("eigen_eval_models")
    common = ["--num_layers", "18", "--weights_init", "scratch", "--batch_size", "2", "--height", str(H), "--width", str(W)]
    torch.manual_seed(5)
    stage1 = _save(MonodepthOptions().parse(common + ["--log_dir", str(tmp / "stage1")]), Trainer, "init")
    out = {"stage1": stage1}
    for catxy in ("true", "false"):
        torch.manual_seed(6)
        o = MonodepthOptions().parse(common + ["--log_dir", str(tmp / ("refine_" + catxy)), "--refine_load_weights_folder", stage1, "--catxy", catxy])
        out["refine", catxy] = _save(o, Refiner, "init")
    return out


def _batch(seed=808, B=2):
    inp, _ = gin.refiner_inputs(seed, B, H, W)
    return {k: v.cuda() for k, v in inp.items()}


def _host(t):
    return t.detach().cpu().numpy()


def test_predictor_defaults_are_unchanged(folders):
    """Without ``refine_2d`` the new arguments are not read: ``predict`` gives the stage-1 decoder's output bit for bit, from either folder."""
    from fusiondepth_amd.predict import Predictor
    batch = _batch()
    a = Predictor(folders["stage1"], num_layers=18).predict(batch)
    b = Predictor(folders["refine", "true"], num_layers=18, catxy=False, refine_iter=3, refine_offset=True, height=64).predict(batch)
    p = Predictor(folders["stage1"], num_layers=18)
    with torch.no_grad():                                        # today's predict, spelled out
        want = dict(p.frozen.run("depth", *p.frozen.run("encoder", batch["color_aug", 0, 0].contiguous()),
                                 *p.frozen.run("beam_encoder", batch["2channel"].contiguous())))
    assert set(a) == set(b) == {("disp", s) for s in range(4)}
    for s in range(4):
        assert torch.equal(a[("disp", s)], b[("disp", s)]) and torch.equal(a[("disp", s)], want[("disp", s)])
    with pytest.raises(FileNotFoundError, match="refine2d_decoder"):
        Predictor(folders["stage1"], num_layers=18, refine_2d=True)


@pytest.mark.parametrize("catxy", ["true", "false"])
def test_refined_prediction_matches_the_refiner(folders, catxy):
    """``Predictor(refine_2d=True).predict`` against ``Refiner.process_batch(batch, val=True)``: two routes through the same kernels."""
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.predict import Predictor
    from fusiondepth_amd.refiner import Refiner
    folder = folders["refine", catxy]
    o = MonodepthOptions().parse(["--num_layers", "18", "--weights_init", "scratch", "--batch_size", "2", "--height", str(H), "--width", str(W),
                                  "--refine_load_weights_folder", folder, "--catxy", catxy, "--refine_a0", "true"])
    rf = Refiner(o, verbose=False)
    batch = _batch()
    want, _ = rf.process_batch(dict(batch), val=True)
    p = Predictor(folder, num_layers=18, refine_2d=True, catxy=(catxy == "true"), refine_a0=True, refine_depthnet_with_beam=False,
                  height=H, width=W, min_depth=o.min_depth, max_depth=o.max_depth)
    got = p.predict(batch)
    coarse = Predictor(folder, num_layers=18).predict(batch)
    for s in range(4):
        a, b = _host(got[("disp", s)]), _host(want[("disp", s)])
        conftest.report("Predictor(refine_2d) vs Refiner.process_batch, catxy %s, disp %d (abs)" % (catxy, s), np.abs(a - b).max(), 2e-6)
        assert_close(a, b, rtol=2e-5, atol=2e-6, what="refined disp %d" % s)
        assert not np.array_equal(a, _host(coarse[("disp", s)]))
    del rf


def test_refine_iter_two_matches_the_oracle_applied_twice(folders):
    from fusiondepth_amd.predict import Predictor
    from oracle import refiner as OR
    folder = folders["refine", "true"]
    oopt = OR.default_opt(batch_size=2, height=H, width=W)
    om = OR.build_models(oopt, 0)
    for k in ("encoder", "beam_encoder", "depth", "refine2d_decoder"):
        sd = torch.load(os.path.join(folder, k + ".pth"), map_location="cpu")
        om[k].load_state_dict({n: v for n, v in sd.items() if n in om[k].state_dict()})
        om[k].eval()
    inp, _ = gin.refiner_inputs(808, 2, H, W)
    with torch.no_grad():
        features, beam_features = om["encoder"](inp[("color_aug", 0, 0)]), om["beam_encoder"](inp["2channel"])
        outputs = dict(om["depth"](features))
        for _ in range(2):
            outputs.update(OR.refine_inputs(oopt, inp, outputs))
            offset = om["refine2d_decoder"](features, beam_features=beam_features, depth_maps=outputs, tanh=False)
            for s in oopt.scales:
                outputs[("disp", s)] = offset[("disp", s)]
    batch = {k: v.cuda() for k, v in inp.items()}
    p = Predictor(folder, num_layers=18, refine_2d=True, refine_iter=2, refine_depthnet_with_beam=False, height=H, width=W,
                  min_depth=oopt.min_depth, max_depth=oopt.max_depth)
    got = p.predict(batch)
    once = Predictor(folder, num_layers=18, refine_2d=True, refine_iter=1, refine_depthnet_with_beam=False, height=H, width=W,
                     min_depth=oopt.min_depth, max_depth=oopt.max_depth).predict(batch)
    for s in range(4):
        assert_close(_host(got[("disp", s)]), outputs[("disp", s)].numpy(), rtol=1e-3, atol=1e-4, what="twice-refined disp %d" % s)
    assert not torch.equal(got[("disp", 0)], once[("disp", 0)])


# ---------------------------------------------------------------------------------------------------------------- the script
SIZES = {"2011_09_26": (375, 1242), "2011_09_30": (370, 1226)}


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    """A two-drive tree with different image sizes, its split file and the ``gt_depths.npz`` ``export_gt_depths`` writes for it."""
    from fusiondepth_amd import kitti_utils as KU
    root = str(tmp_path_factory.mktemp("kitti"))
    lines = kitti_tree.make_tree(root, [("2011_09_26", "2011_09_26_drive_0001_sync", SIZES["2011_09_26"], (1.0, 1.0)),
                                        ("2011_09_30", "2011_09_30_drive_0016_sync", SIZES["2011_09_30"], (1.0, 1.0))], frames=4, down=0.35)
    assert len(lines) == 4
    splits = str(tmp_path_factory.mktemp("splits"))
    for name in ("eigen", "benchmark"):
        os.makedirs(os.path.join(splits, name))
        with open(os.path.join(splits, name, "test_files.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    gts = KU.export_gt_depths(root, lines, "eigen", os.path.join(splits, "eigen", "gt_depths.npz"))
    assert [g.shape for g in gts] == [SIZES[l.split("/")[0]] for l in lines]
    return root, splits, lines, gts


def _eval_opt(root, folder, *extra):
    from fusiondepth_amd.options import MonodepthOptions
    return MonodepthOptions().parse(["--num_layers", "18", "--data_path", root, "--png", "--load_weights_folder", folder, "--eval_mono",
                                     "--eval_batch_size", "3"] + list(extra))


def test_script_end_to_end(folders, split, capsys):
    from PIL import Image
    from fusiondepth_amd import evaluate_depth as ED
    root, splits, lines, gts = split
    N = len(lines)
    stage1, refined = folders["stage1"], folders["refine", "true"]
    mean, ratios, per = ED.evaluate(_eval_opt(root, stage1, "--save_pred_disps"), splits)
    printed = capsys.readouterr().out
    assert "Scaling ratios | med:" in printed and "abs_rel |" in printed and "-> Done!" in printed
    assert per.shape == (N, 7) and ratios.shape == (N,) and np.isfinite(per).all() and np.isfinite(ratios).all()
    saved = os.path.join(stage1, "disps_eigen_split.npy")
    disps = np.load(saved)
    assert disps.shape == (N, 192, 640) and disps.dtype == np.float32
    want, want_r = ED.evaluate_predictions(torch.from_numpy(disps).cuda(), gts, "eigen")
    assert_close(mean[:4], want[:4], rtol=5e-5, atol=0, what="script: mean abs_rel / sq_rel / rmse / rmse_log")
    assert_close(mean[4:], want[4:], rtol=0, atol=3e-4, what="script: mean a1 / a2 / a3")
    assert_close(ratios, want_r, rtol=1e-5, atol=0, what="script: ratios")
    # the saved disparities through --ext_disp_to_eval: the same numbers, bit for bit (no network is loaded)
    from fusiondepth_amd.options import MonodepthOptions
    again = ED.evaluate(MonodepthOptions().parse(["--eval_mono", "--ext_disp_to_eval", saved]), splits)
    assert np.array_equal(again[0].view(np.uint64), mean.view(np.uint64)) and np.array_equal(again[2].view(np.uint64), per.view(np.uint64))
    assert np.array_equal(again[1].view(np.uint32), ratios.view(np.uint32))
    # stereo: no median scaling, factor 5.4
    st = ED.evaluate(MonodepthOptions().parse(["--eval_stereo", "--ext_disp_to_eval", saved]), splits)
    assert st[1].size == 0 and np.isfinite(st[0]).all() and not np.array_equal(st[0], mean)
    # the command line: --splits_dir is taken off before the options are parsed
    cli = ED.main(["--splits_dir", splits, "--eval_mono", "--ext_disp_to_eval", saved])
    assert np.array_equal(cli[0].view(np.uint64), mean.view(np.uint64))
    # --refine_2d: other disparities, still finite scores
    r_mean, r_ratios, r_per = ED.evaluate(_eval_opt(root, refined, "--refine_2d", "--save_pred_disps"), splits)
    r_disps = np.load(os.path.join(refined, "disps_eigen_split.npy"))
    assert r_disps.shape == disps.shape and not np.array_equal(r_disps, disps) and np.isfinite(r_per).all() and np.isfinite(r_mean).all()
    # --post_process: float64 disparities of the reference's fixed size
    pp = ED.evaluate(_eval_opt(root, refined, "--refine_2d", "--post_process", "--save_pred_disps", "--no_eval"), splits)
    pp_disps = np.load(os.path.join(refined, "disps_eigen_split.npy"))
    assert pp is None and pp_disps.shape == (N, 192, 640) and pp_disps.dtype == np.float64 and np.isfinite(pp_disps).all()
    assert not np.array_equal(pp_disps.astype(np.float32), r_disps)
    pp_mean = ED.evaluate(_eval_opt(root, stage1, "--post_process"), splits)[0]
    assert np.isfinite(pp_mean).all()
    # --eval_split benchmark: N uint16 352 x 1216 PNGs
    assert ED.evaluate(_eval_opt(root, stage1, "--eval_split", "benchmark"), splits) is None
    out = os.path.join(stage1, "benchmark_predictions")
    assert sorted(os.listdir(out)) == ["%010d.png" % i for i in range(N)]
    for i in range(N):
        png = np.array(Image.open(os.path.join(out, "%010d.png" % i)))
        assert png.dtype == np.uint16 and png.shape == (352, 1216) and png.max() <= 80 * 256
    from fusiondepth_amd import functional as FD
    want0 = ED.benchmark_depth_png(FD.resize_linear_cv(torch.from_numpy(disps[:1]).cuda(), (352, 1216)).cpu().numpy())[0]
    assert np.array_equal(np.array(Image.open(os.path.join(out, "%010d.png" % 0))), want0)
