"""The float64 references and seeded inputs of tests/glue_ref.py without a GPU: every reference against the float32 CPU oracle
(``oracle.layers`` / plain torch / ``torch.optim.Adam``) on the same inputs - the measured difference is the yardstick the GPU tests
scale their bounds by (tests/test_gpu_glue_edges.py) - and the input conditions that keep those GPU tests from hiding or inventing
failures, for every case they run."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_ref as R
from conftest import report
from oracle import layers as OL

F32, F64 = torch.float32, torch.float64
AGREE = 2e-4          # float32 against float64 of these formulas: 4.8e-5 at worst (pose-vector gradient, 1 - cos at 3e-4 rad)


def yardsticks(what, fn, *args, exact=()):
    """rel_err of the float32 oracle against the float64 reference per output; both are returned for further checks."""
    ref, ora = fn(*args[:1], F64, *args[1:]), fn(*args[:1], F32, *args[1:])
    for k in ref:
        if not torch.is_tensor(ref[k]) or ref[k].dtype != F64:
            continue
        assert ora[k].dtype == F32, "%s %s: the oracle is not float32" % (what, k)
        if not bool(torch.isfinite(ref[k]).all()):
            assert R.same_values(ora[k].to(F64), ref[k]), "%s %s: non-finite pattern" % (what, k)
            continue
        y = R.rel_err(ora[k], ref[k])
        report("yardstick %s %s" % (what, k), y, AGREE)
        assert y <= AGREE, "%s %s: float32 oracle and float64 reference differ by %.3g of scale" % (what, k, y)
        if k in exact:
            # a copy, a selection or one correctly rounded addition: the float32 result is the rounded float64 one
            assert torch.equal(ora[k], ref[k].to(F32)), "%s %s must be exact in float32, differs by %.3g" % (what, k, y)
    return ref, ora


def test_rel_err_and_bound():
    ref = torch.tensor([1.0, -4.0, 0.0], dtype=F64)
    assert R.rel_err(ref, ref) == 0.0
    assert R.rel_err(torch.tensor([1.0, -4.0, 0.002]), ref) == pytest.approx(5e-4, rel=1e-3)      # a small entry errs at the scale of the tensor
    assert R.rel_err(torch.zeros(3), torch.zeros(3)) == 0.0
    assert R.rel_err(torch.full((3,), 1e-20), torch.zeros(3)) > 1.0                                  # tiny keeps 0 / 0 out, not errors
    assert R.bound(0.0) == 1e-6 and R.bound(1e-5) == 4e-5 and R.bound(1e-5, cap=2e-5) == 2e-5 and R.bound(1e-9, cap=2e-5) == 1e-6
    nan = float("nan")
    assert R.same_values(torch.tensor([1.0, nan]), torch.tensor([1.0, nan])) and not R.same_values(torch.tensor([1.0, nan]), torch.tensor([1.0, 2.0]))


@pytest.mark.parametrize("n", R.D2D_N)
def test_disp_to_depth(n):
    inp = R.d2d_inputs(n)
    for use_gs, use_gd in ((True, True), (True, False), (False, True), (False, False)):
        ref, _ = yardsticks("disp_to_depth n=%d gs=%d gd=%d" % (n, use_gs, use_gd), R.d2d_ref, inp, use_gs, use_gd)
        if not (use_gs or use_gd):
            assert not ref["d_disp"].any()
    assert float(ref["depth"].min()) >= R.MIN_DEPTH * (1 - 1e-6) and float(ref["depth"].max()) <= R.MAX_DEPTH


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("B", R.POSE_B)
def test_pose_matrix(B, invert):
    inp = R.pose_inputs(B)
    norms = inp["aa"].to(F64).norm(dim=2).reshape(-1)
    want = sorted(set(R.POSE_NORMS)) if B >= 8 else None
    if want:
        for w in want:           # every norm of the list is in the batch (to float32 rounding of the vector)
            assert bool(((norms - w).abs() <= 1e-6 * max(w, 1e-30) + 1e-30).any()), "no item with rotation norm %g" % w
    ref, ora = yardsticks("pose_matrix B=%d invert=%d" % (B, invert), R.pose_ref, inp, invert)
    for d in (ref, ora):
        assert all(bool(torch.isfinite(v).all()) for v in d.values())


def test_pose_head():
    inp = R.pose_head_inputs()
    G, nf, Bq, npred = R.POSE_HEAD
    assert G * nf * Bq == 66
    ref, _ = yardsticks("pose_head", R.pose_head_ref, inp)
    assert not ref["g_pose"][:, 6:].any() and ref["g_pose"][:, :6].abs().min() > 0


@pytest.mark.parametrize("B", R.PROJMAT_B)
def test_proj_matrix(B):
    yardsticks("proj_matrix B=%d" % B, R.projmat_ref, R.projmat_inputs(B))
    assert (B * 12 > 64) == (B >= 6) and (B * 16 > 64) == (B >= 5)


@pytest.mark.parametrize("B,H,W", R.BACKPROJECT_SHAPES)
def test_backproject_and_cat_xy(B, H, W):
    inp = R.backproject_inputs(B, H, W)
    yardsticks("backproject %dx%dx%d" % (B, H, W), R.backproject_ref, inp)
    assert B == 1 or not torch.equal(inp["inv_K"][0], inp["inv_K"][1])
    assert 1.0 <= float(inp["depth"].min()) and float(inp["depth"].max()) <= 21.0


@pytest.mark.parametrize("B,H,W", R.PROJECT_SHAPES)
def test_project3d(B, H, W):
    inp = R.project_inputs(B, H, W)
    z = R.project_cam_z(inp)
    report("project3d %dx%dx%d min |cam_z + eps|" % (B, H, W), float(z.abs().min()), 0.5, "(must be >= the bound)")
    assert float(z.abs().min()) >= 0.5
    assert B == 1 or not (torch.equal(inp["K"][0], inp["K"][1]) or torch.equal(inp["T"][0], inp["T"][1]))
    Rm, t = inp["T"][:, :3, :3].to(F64), inp["T"][:, :3, 3].to(F64)
    angle = torch.acos(((Rm.diagonal(dim1=1, dim2=2).sum(-1) - 1) / 2).clamp(-1, 1))
    assert float(angle.max()) <= 0.05 + 1e-6 and float(t.norm(dim=1).max()) <= 0.3 + 1e-6
    yardsticks("project3d %dx%dx%d" % (B, H, W), R.project_ref, inp)


@pytest.mark.parametrize("kind", R.MAXPOOL_KINDS)
@pytest.mark.parametrize("N,C,H,W", R.MAXPOOL_SHAPES)
def test_maxpool(N, C, H, W, kind):
    inp = R.maxpool_inputs(N, C, H, W, kind)
    x = inp["x"]
    assert R.maxpool_unintended_ties(x) == 0, "a tie between values that are not exact repeats"
    ref, ora = yardsticks("maxpool %s %dx%dx%dx%d" % (kind, N, C, H, W), R.maxpool_ref, inp, exact=("y",))
    assert R.same_values(ora["y"].to(F64), ref["y"])
    # float32 and float64 route every gradient to the same input pixel, ties, -inf and NaN included
    assert torch.equal(ora["gx"] != 0, ref["gx"] != 0)
    if kind == "negative":
        assert float(x.max()) < 0 and float(ref["y"].max()) < 0
    if kind == "neginf":
        assert bool(torch.isinf(ref["y"]).any()), "no window is all -inf"
    if kind == "nan":
        assert bool(torch.isnan(ref["y"]).any()) and not bool(torch.isnan(ref["gx"]).any())
    if kind == "const":
        assert float(x.reshape(N * C, -1)[-1].max()) == float(x.reshape(N * C, -1)[-1].min()) == -1.5


@pytest.mark.parametrize("combo", R.UPCAT_COMBOS)
@pytest.mark.parametrize("h,w", R.UPCAT_HW)
def test_upsample_concat(h, w, combo):
    inp = R.upcat_inputs(h, w)
    ref, _ = yardsticks("upcat %dx%d %s" % (h, w, combo), R.upcat_ref, inp, combo, exact=("y", "g_skip", "g_skip_add", "g_extra"))
    N, Ca, Cs, C3 = inp["dims"]
    assert ref["y"].shape == (N, Ca + Cs * combo[0] + C3 * combo[2], 2 * h, 2 * w)


@pytest.mark.parametrize("act", R.ACT_NAMES[1:])
def test_upsample_concat_activation_gradient_equals_autograd(act):
    """The gradient written through the activation's output is the autograd gradient of cat([up2(act(pre)), skip]) in pre."""
    fn = {"relu": torch.relu, "elu": F.elu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}[act]
    pre = torch.randn(2, 3, 5, 7, dtype=F64, generator=torch.Generator().manual_seed(3)).requires_grad_(True)
    a = fn(pre)
    cot = torch.randn(2, 3, 10, 14, dtype=F64, generator=torch.Generator().manual_seed(4))
    (want,) = torch.autograd.grad(OL.upsample(a), pre, cot)
    (plain,) = torch.autograd.grad(OL.upsample(a), a, cot)
    assert R.rel_err(plain * R.act_deriv_from_output(a.detach(), act), want) < 1e-14
    for h, w in ((6, 8), (5, 7)):
        v = R.upcat_inputs(h, w, act)["a"]
        lo, hi = {"relu": (0, 1e9), "elu": (-1, 1e9), "sigmoid": (0, 1), "tanh": (-1, 1)}[act]
        assert float(v.min()) >= lo and float(v.max()) <= hi and (act != "relu" or bool((v == 0).any()))
        yardsticks("upcat act %s %dx%d" % (act, h, w), R.upcat_ref, R.upcat_inputs(h, w, act), (1, 0, 0), act)


@pytest.mark.parametrize("N,C,h,w", R.UP2_CASES)
def test_upsample_nearest2x(N, C, h, w):
    yardsticks("upsample2x %dx%dx%dx%d" % (N, C, h, w), R.up2_ref, R.up2_inputs(N, C, h, w), exact=("y",))


@pytest.mark.parametrize("n", R.EW_N)
def test_elementwise(n):
    inp = R.ew_inputs(n)
    for act in R.ACT_NAMES:
        y = R.act_output_values(np.random.RandomState(n % 1000), (n,), act)
        r = yardsticks("act_bwd %s n=%d" % (act, n), lambda d, dt: {"g": R.act_bwd_ref(d["y"], d["gy"], act, dt)}, {"y": y, "gy": inp["b"]})[0]
        assert r["g"].shape == (n,)
    yardsticks("axpby n=%d" % n, lambda d, dt: {"out": R.axpby_ref(d["a"], d["b"], 0.7, -1.3, dt)}, inp)
    norm = R.input_normalize_f32(inp["img"])
    assert norm.dtype == F32 and R.rel_err(norm, (inp["img"].to(F64) - 0.45) / 0.225) < 1e-6


@pytest.mark.parametrize("planes", R.MEAN_PLANES)
@pytest.mark.parametrize("plane_size", R.MEAN_PLANE_SIZES)
def test_spatial_mean(plane_size, planes):
    inp = R.mean_inputs(planes, plane_size)
    assert inp["x"].shape[0] * inp["x"].shape[1] == planes and inp["x"].shape[2] * inp["x"].shape[3] == plane_size
    yardsticks("spatial_mean %dx%d" % (planes, plane_size), R.mean_ref, inp)


@pytest.mark.parametrize("n", R.DEPTH_ERR_N)
def test_depth_errors(n):
    inp = R.depth_err_inputs(n)
    for k in ("gt", "pred"):
        assert inp[k].shape == (n,) and 0.5 <= float(inp[k].min()) and float(inp[k].max()) <= 80.0
    margin = R.depth_err_margin(inp)
    report("depth_errors n=%d distance of max(gt/pred, pred/gt) from a threshold" % n, margin, 1e-4, "(must be >= the bound)")
    assert margin >= 1e-4
    (ref, counts), (ora, counts32) = R.depth_err_ref(inp, F64), R.depth_err_ref(inp, F32)
    assert counts == counts32 and counts[0] <= counts[1] <= counts[2] <= n
    if n >= 256:
        assert 0 < counts[0] < counts[1] < counts[2] < n, "every threshold must separate some samples"
    for i, name in enumerate(("abs_rel", "sq_rel", "rmse", "rmse_log")):
        y = R.rel_err(ora[i], ref[i])
        report("yardstick depth_errors n=%d %s" % (n, name), y, AGREE)
        assert y <= AGREE


@pytest.mark.parametrize("n", R.ADAM_N)
def test_adam_restatement(n):
    for name, sc in R.adam_scenarios(n).items():
        ref = R.adam_ref(sc)
        t64, _ = R.adam_torch(sc, F64)
        t32, _ = R.adam_torch(sc, F32)
        for k in ref:
            assert R.rel_err(t64[k], ref[k]) < 1e-12, "%s %s: the restatement is not torch.optim.Adam" % (name, k)
            y = R.rel_err(t32[k], ref[k])
            report("yardstick adam n=%d %s: %s" % (n, name, k), y, 1e-4)
            assert y <= 1e-4
        assert float(ref["p"].abs().max()) > 0
    sc = R.adam_scenarios(n)["five steps from zero"]
    if n >= 257:
        split, _ = R.adam_torch(sc, F64, shapes=[(n - 100,), (10, 10)])
        assert R.rel_err(split["p"], R.adam_ref(sc)["p"]) < 1e-12
