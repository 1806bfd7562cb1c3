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


# ================================================================================================ the loss-map kernels' references
def finite_yardsticks(what, fn, *args):
    """rel_err of the float32 oracle against the float64 reference per output, reported; it has to be a number, its size is the GPU
    test's business (the SSIM gradients lose more than AGREE to the cancellation in E[x^2] - mu^2)."""
    ref, ora = fn(*args[:1], F64, *args[1:]), fn(*args[:1], F32, *args[1:])
    for k in ref:
        assert ref[k].dtype == F64 and ora[k].dtype == F32, "%s %s: dtypes %s, %s" % (what, k, ref[k].dtype, ora[k].dtype)
        assert bool(torch.isfinite(ref[k]).all()) and bool(torch.isfinite(ora[k]).all()), "%s %s is not finite" % (what, k)
        y = R.rel_err(ora[k], ref[k])
        report("yardstick %s %s" % (what, k), y, float("inf"), "(must be finite)")
        assert np.isfinite(y), "%s %s: yardstick %r" % (what, k, y)
    return ref, ora


@pytest.mark.parametrize("BC,Hin,Win,Hout,Wout", R.BILINEAR_CASES)
def test_bilinear(BC, Hin, Win, Hout, Wout):
    inp = R.bilinear_inputs(BC, Hin, Win, Hout, Wout)
    assert inp["x"].shape == (1, BC, Hin, Win) and inp["cot"].shape == (1, BC, Hout, Wout) and Hout >= Hin and Wout >= Win
    ref, _ = finite_yardsticks("bilinear %dx%dx%d -> %dx%d" % (BC, Hin, Win, Hout, Wout), R.bilinear_ref, inp)
    assert ref["y"].shape == inp["cot"].shape and ref["gx"].shape == inp["x"].shape
    if Hin * Win > R.BILINEAR_DENSE_MAX:
        return
    # the adjoint, independently of autograd: the forward reference as a dense matrix, transposed
    M = R.bilinear_matrix(Hin, Win, Hout, Wout)
    assert R.rel_err((M @ inp["x"].to(F64).reshape(BC, -1).t()).t().reshape(ref["y"].shape), ref["y"]) < 1e-12
    assert float((M.sum(1) - 1).abs().max()) < 1e-12 and float(M.min()) >= 0
    want = (M.t() @ inp["cot"].to(F64).reshape(BC, -1).t()).t().reshape(ref["gx"].shape)
    e = R.rel_err(ref["gx"], want)
    report("bilinear %dx%dx%d -> %dx%d gradient reference against M^T cot" % (BC, Hin, Win, Hout, Wout), e, 1e-12)
    assert e <= 1e-12


def test_bilinear_cases_cover_their_edges():
    dense = [c for c in R.BILINEAR_CASES if c[1] * c[2] <= R.BILINEAR_DENSE_MAX]
    assert len(dense) == len(R.BILINEAR_CASES) - 3
    assert {c[1] * c[2] for c in R.BILINEAR_CASES} >= {255, 256, 257}
    assert any(c[3] * c[4] > 2048 * 256 for c in R.BILINEAR_CASES) and any(c[1] * c[2] > 2048 * 256 for c in R.BILINEAR_CASES)
    frac = [c for c in R.BILINEAR_CASES if c[3] % c[1] or c[4] % c[2]]
    assert (1, 6, 6, 7, 7) in frac and len(frac) == 7 and R.BILINEAR_OFFSET_CASE in frac


def _ssim_cases():
    return [(p, H, W, "smooth") for H, W in R.SSIM_HW for p in R.SSIM_PLANES] + [R.SSIM_UNIFORM_CASE + ("uniform",)]


@pytest.mark.parametrize("planes,H,W,kind", _ssim_cases())
def test_ssim(planes, H, W, kind):
    inp = R.ssim_inputs(planes, H, W, kind)
    what = "ssim %s %dx%dx%d" % (kind, planes, H, W)
    diff = R.ssim_window_difference(inp)
    report("%s min over windows of max |x - y|" % what, diff, 1e-3, "(must be >= the bound)")
    assert diff >= 1e-3, "a 3x3 window in which the two images are all but equal"
    pre = R.ssim_preclamp(inp["x"].to(F64), inp["y"].to(F64))
    margin = min(float(pre.min()), 1.0 - float(pre.max()))
    report("%s distance of the float64 pre-clamp value from 0 and 1" % what, margin, 1e-4, "(must be >= the bound)")
    assert margin >= 1e-4
    ref, _ = finite_yardsticks(what, R.ssim_ref, inp)
    assert torch.equal(ref["ssim"], pre), "no pixel is clamped, so the clamp changes nothing"
    assert float(ref["gx"].abs().max()) > 0 and float(ref["gy"].abs().max()) > 0
    only_x, only_y = R.ssim_ref(inp, F64, True, False), R.ssim_ref(inp, F64, False, True)
    assert "gy" not in only_x and "gx" not in only_y and torch.equal(only_x["gx"], ref["gx"]) and torch.equal(only_y["gy"], ref["gy"])


def test_ssim_of_equal_windows_is_zero():
    planes, H, W = R.SSIM_EQUAL_CASE
    inp = R.ssim_inputs(planes, H, W, "equal")
    assert torch.equal(inp["x"][..., H - 8:, W - 8:], inp["y"][..., H - 8:, W - 8:]) and H - 8 < 16 < H and W - 8 < 64 < W
    for dt in (F64, F32):
        s = R.ssim_ref(inp, dt)["ssim"]
        assert bool(torch.isfinite(s).all())
        assert not s[..., H - 7:, W - 7:].any(), "windows inside the block (the reflection keeps the last row and column inside)"
        assert float(s[..., :H - 9, :W - 9].min()) > 0


@pytest.mark.parametrize("use_ssim", [True, False])
@pytest.mark.parametrize("B", R.REPROJ_B)
@pytest.mark.parametrize("H,W", R.SSIM_HW)
def test_reprojection_map(H, W, B, use_ssim):
    inp = R.reproj_inputs(B, H, W)
    ref, _ = finite_yardsticks("reproj map %dx%dx%d ssim=%d" % (B, H, W, use_ssim), R.reproj_ref, inp, use_ssim)
    assert ref["map"].shape == (B, 1, H, W) and float(ref["map"].min()) > 0


def test_reprojection_map_is_the_oracle_trainers():
    from oracle import trainer as OT
    inp = R.reproj_inputs(3, 17, 65)
    for use_ssim in (True, False):
        want = OT.reprojection_loss(OT.default_opt(no_ssim=not use_ssim), inp["pred"], inp["target"])
        assert torch.equal(R.reproj_ref(inp, F32, use_ssim)["map"], want)


def _smooth_cases():
    return [(B, H, W, n) for H, W in R.SMOOTH_SHAPES for B in R.SMOOTH_B for n in (False, True)] + list(R.SMOOTH_EXTRA)


@pytest.mark.parametrize("B,H,W,normalize", _smooth_cases())
def test_smooth_loss(B, H, W, normalize):
    inp = R.smooth_inputs(B, H, W)
    d = inp["disp"]
    assert d.shape == (B, 1, H, W) and 0.01 < float(d.min()) and float(d.max()) <= 1.0
    assert torch.equal(d.to(F64) / inp["step"], (d.to(F64) / inp["step"]).round()) and d.unique().numel() == d.numel()
    gap = R.smooth_min_neighbour_difference(inp)
    # one step of 2^-e >= 2^-19 between any two disparities <= 1: at least 16 float32 roundings of either, divided by the mean or not
    report("smooth %dx%dx%d min |d_p - d_q| over the edges" % (B, H, W), gap, inp["step"], "(must be >= the bound)")
    assert gap >= inp["step"] >= 2.0 ** -19
    what = "smooth %dx%dx%d normalize=%d" % (B, H, W, normalize)
    ref, ora = finite_yardsticks(what, R.smooth_ref, inp, normalize)
    assert ref["g_disp"].shape == d.shape and float(ref["loss"]) > 0 and float(ref["g_disp"].abs().min()) > 0


def test_smooth_cases_cover_their_edges():
    px = [H * W for H, W in R.SMOOTH_SHAPES]
    assert px[1:4] == [1023, 1024, 1025] and [p // 4 for p in px[4:]] == [3072, 3073, 4096, 4097] and all(p % 4 == 0 for p in px[4:])
    assert 2 * -(-330 * 400 // 1024) == 258 and -(-513 * 513 // 256) > 1024


@pytest.mark.parametrize("si_mode", R.COMBINE_SI)
@pytest.mark.parametrize("n", R.COMBINE_N)
def test_combine_losses(n, si_mode):
    inp = R.combine_inputs(n, si_mode)
    assert [s is not None for s in inp["si"]] == [si_mode == "all" or (si_mode == "scale0" and s == 0) for s in range(n)]
    ref, _ = finite_yardsticks("combine n=%d si=%s" % (n, si_mode), R.combine_ref, inp)
    # against autograd through the same formula in float64
    leaves = [t.to(F64).clone().requires_grad_(True) for t in inp["photo"] + inp["smooth"] + [s for s in inp["si"] if s is not None]]
    photo, smooth, si = leaves[:n], leaves[n:2 * n], iter(leaves[2 * n:])
    total = sum(photo[s] + float(np.float32(inp["w"])) * smooth[s] / 2 ** s for s in range(n)) + sum(next(si) for s in inp["si"] if s is not None)
    g = torch.autograd.grad(total / n, leaves, torch.tensor(float(np.float32(inp["cot"])), dtype=F64))
    assert abs(float((total / n).detach()) - float(ref["total"])) <= 1e-14
    assert R.rel_err(torch.stack(g[:n]), ref["g_photo"]) < 1e-14 and R.rel_err(torch.stack(g[n:2 * n]), ref["g_smooth"]) < 1e-14
    for gs in g[2 * n:]:
        assert abs(float(gs) - float(ref["g_si"][0])) <= 1e-15


def test_combine_reference_equals_the_oracle_trainers_totals():
    """oracle.trainer.compute_losses on one seeded batch: with the smoothness weight 0 its loss/s are the photometric terms alone
    (x + 0 is x), the smoothness terms are recomputed as it computes them, the SI terms are its own - and the float32 restatement must
    then give its loss/s and its total bit for bit."""
    import inputs as gin
    from oracle import trainer as OT
    B, H, W = 2, 64, 96
    inp, rng = gin.batch_inputs(404, B, H, W)
    disp = gin.disp_pyramid(rng, B, H, W)
    Ts = {f: OL.transformation_from_parameters(*gin.small_poses(rng, B), invert=(f < 0)) for f in (-1, 1)}
    noise = [torch.from_numpy(np.random.RandomState(7 + s).randn(B, 2, H, W).astype(np.float32)) for s in range(4)]

    def run(**over):
        opt = OT.default_opt(height=H, width=W, **over)
        outputs = dict(disp)
        for f in (-1, 1):
            outputs[("cam_T_cam", 0, f)] = Ts[f]
        OT.generate_images_pred(opt, inp, outputs)
        return opt, OT.compute_losses(opt, inp, outputs, noise)

    opt, want = run()
    _, bare = run(disparity_smoothness=0.0)
    n = len(opt.scales)
    smooth = []
    for s in opt.scales:
        d = disp[("disp", s)]
        smooth.append(OL.get_smooth_loss(d / (d.mean(2, True).mean(3, True) + 1e-7), inp[("color", 0, s)]))
    case = {"photo": [bare["loss/%d" % s] for s in opt.scales], "smooth": smooth,
            "si": [want.get("loss/si_loss%d" % s) for s in opt.scales], "w": opt.disparity_smoothness, "cot": 1.0}
    assert all(s is not None for s in case["si"]) and n == 4
    got = R.combine_ref(case, F32)
    assert got["total"].dtype == F32 and torch.equal(got["total"], want["loss"])
    for s in opt.scales:
        assert torch.equal(got["loss"][s], want["loss/%d" % s])
    case["si"] = [case["si"][0], None, None, None]
    _, want0 = run(trainer_siloss_all_scale=False)
    assert "loss/si_loss1" not in want0 and torch.equal(R.combine_ref(case, F32)["total"], want0["loss"])
