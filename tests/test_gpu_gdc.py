"""Graph-based depth correction (fusiondepth_amd/gdc.py, csrc/gdc.hip) against a float64 restatement of gdc_old.py's GDC
written here on numpy, scipy.spatial.cKDTree, scipy.sparse and scipy.sparse.linalg.cg(rtol=..., atol=0).

Fixtures are generated: a KITTI-calibrated scene (ground plane 1.65 m below the camera, boxes, a far wall), LiDAR on 4 rows of
constant pitch inside (0, 4) degrees every 2-3 columns with 2 cm noise, and a prediction = truth * (1 + smooth +-10 %) + noise."""
import os
import sys
import types

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch
from scipy.spatial import cKDTree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEAMS = (-0.1, 4.0)          # inf_gdc.py:76-79 / evaluate_depth.py:391-396
RANDOM = (-1.5, 9)
# tests/golden/inputs.py::lidar_scan's P_rect_02
K = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])


def camera():
    return types.SimpleNamespace(c_u=K[0, 2], c_v=K[1, 2], f_u=K[0, 0], f_v=K[1, 1], b_x=K[0, 3] / -K[0, 0], b_y=K[1, 3] / -K[1, 1])


def scene(H, W, seed=0):
    """-> (truth float64, pred float32, lidar float64 with -1 where there is no point)."""
    rng = np.random.RandomState(seed)
    cam = camera()
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dx, dy = (u - cam.c_u) / cam.f_u, (v - cam.c_v) / cam.f_v
    depth = np.full((H, W), 60.0) + 3.0 * np.sin(u / 97.0)                 # far wall
    with np.errstate(divide="ignore"):
        ground = np.where(dy > 1e-4, 1.65 / dy, np.inf)
    depth = np.minimum(depth, ground)
    for x0, x1, y0, z0 in ((-6.0, -2.0, -0.3, 14.0), (1.5, 4.5, 0.2, 24.0), (-14.0, -8.0, -1.2, 35.0), (6.0, 12.0, -0.5, 45.0)):
        x, y = dx * z0, dy * z0
        hit = (x >= x0) & (x < x1) & (y >= y0) & (y < 1.65)
        depth = np.where(hit, np.minimum(depth, z0), depth)
    distort = 1.0 + 0.1 * np.sin(u / 180.0 + 0.7) * np.cos(v / 90.0)
    pred = (depth * distort + rng.randn(H, W) * 0.02 * np.sqrt(depth)).astype(np.float32)
    lidar = np.full((H, W), -1.0)
    for pitch in (0.5, 1.5, 2.5, 3.5):
        row = int(round(cam.c_v + cam.f_v * np.tan(np.radians(pitch))))
        cols, c = [], 0
        while c < W:
            cols.append(c)
            c += 2 + (len(cols) % 2)
        cols = np.array(cols)
        lidar[row, cols] = depth[row, cols] + rng.randn(cols.size) * 0.02
    return depth, pred, lidar


# ----------------------------------------------------------------------------------------- restatement (float64 numpy/scipy) --
def cloud(depth, cam):
    H, W = depth.shape
    c, r = np.meshgrid(np.arange(W), np.arange(H))
    pts = np.stack([c, r, depth]).reshape((3, -1)).T
    x = ((pts[:, 0] - cam.c_u) * pts[:, 2]) / cam.f_u + cam.b_x
    y = ((pts[:, 1] - cam.c_v) * pts[:, 2]) / cam.f_v + cam.b_y
    return np.stack([x, y, pts[:, 2]], 1)


def region(p):
    return (p[:, 2] < 80) & (p[:, 2] > 1) & (p[:, 0] < 40) & (p[:, 0] >= -40) & (p[:, 1] < 2.5) & (p[:, 1] >= -1)


def pitch(p):
    return np.arcsin(p[:, 1] / np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2 + p[:, 2] ** 2))


def ref_masks(pred, gt, cam, rng):
    pc, pg = cloud(pred, cam), cloud(gt, cam)
    th = pitch(pc)
    lo, hi = np.radians(rng[0]), np.radians(rng[1])
    consider = region(pc) & (th >= lo) & (th < hi)
    gtm = consider & region(pg)
    gtm[gtm] &= np.abs(pred.reshape(-1)[gtm] - gt.reshape(-1)[gtm]) < 2
    predm = consider & ~gtm
    near = np.minimum(np.abs(th - lo), np.abs(th - hi)) < 1e-12
    return predm, gtm, pc, near


def ref_weights(x_info, nbr, k, W_tol):
    n = x_info.shape[0]
    A = np.zeros((n, k + 2, k + 2))
    b = np.zeros((n, k + 2))
    A[:, :k, :k] = np.eye(k) * (1 + W_tol)
    A[:, k + 1, :k] = 1
    A[:, :k, k + 1] = 1
    b[:, k + 1] = 1
    b[:, k] = x_info
    A[:, k, :k] = x_info[nbr]
    A[:, :k, k] = x_info[nbr]
    return np.linalg.solve(A, b[..., None])[..., 0][:, :k]


def ref_system(nbr, Wt, N_PL, g):
    """A = [I - W_PLPL ; W_PLL], b = [W_LPL g ; g - W_LL g] as CSR matrices built row by row from the neighbour lists."""
    N, k = nbr.shape
    rows = np.repeat(np.arange(N), k)
    cols, vals = nbr.reshape(-1), Wt.reshape(-1)
    pl = cols < N_PL
    Wfull_pl = sp.csr_matrix((vals[pl], (rows[pl], cols[pl])), shape=(N, N_PL))
    Wfull_l = sp.csr_matrix((vals[~pl], (rows[~pl], cols[~pl] - N_PL)), shape=(N, max(N - N_PL, 0)))
    A = sp.vstack((sp.eye(N_PL) - Wfull_pl[:N_PL], Wfull_pl[N_PL:])).tocsr()
    b = np.concatenate((Wfull_l[:N_PL].dot(g), g - Wfull_l[N_PL:].dot(g)))
    return A, b


def ref_cg(A, b, x0, rtol, maxiter):
    its = [0]

    def cb(_):
        its[0] += 1
    ATA = spla.LinearOperator((A.shape[1], A.shape[1]), matvec=lambda v: A.T.dot(A.dot(v)))
    x, info = spla.cg(ATA, A.T.dot(b), x0=x0.copy(), rtol=rtol, atol=0.0, maxiter=maxiter, callback=cb)
    return x, its[0], info


def ref_gdc(pred, gt, cam, k=10, W_tol=3e-5, recon_tol=5e-4, rng=BEAMS, maxiter=None):
    predm, gtm, pc, _ = ref_masks(pred, gt, cam, rng)
    x_info = np.concatenate((pred.reshape(-1)[predm], pred.reshape(-1)[gtm])).astype(np.float64)
    g = gt.reshape(-1)[gtm]
    N_PL, N_L = int(predm.sum()), int(gtm.sum())
    pts = np.concatenate((pc[predm], pc[gtm]))
    _, ind = cKDTree(pts).query(pts, k=k + 1)
    nbr = ind[:, 1:]
    Wt = ref_weights(x_info, nbr, k, W_tol)
    A, b = ref_system(nbr, Wt, N_PL, g)
    x, its, info = ref_cg(A, b, x_info[:N_PL], recon_tol, 10 * N_PL if maxiter is None else maxiter)
    out = pred.copy()
    out.reshape(-1)[predm] = x
    out[gt > 0] = gt[gt > 0]
    return dict(out=out, N_PL=N_PL, N_L=N_L, x=x, its=its, predm=predm, gtm=gtm, A=A, b=b)


# ------------------------------------------------------------------------------------------------------------------ helpers --
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def G():
    from fusiondepth_amd import gdc
    return gdc


@pytest.fixture(scope="module", params=[(375, 1242), (370, 1224)], ids=["375x1242", "370x1224"])
def frame(request):
    H, W = request.param
    return scene(H, W, seed=H)


def gpu_stage(G, pred, gt, rng, k=10, recon_tol=5e-4):
    p, g = dev(pred), dev(gt)
    pix, N_PL, N_L = G.prepare(p, g, camera(), rng)
    ws = G.build(p, g, camera(), pix, N_PL, N_L, k, recon_tol)
    torch.cuda.synchronize()
    return pix, N_PL, N_L, ws


# -------------------------------------------------------------------------------------------------------------------- tests --
@pytest.mark.parametrize("rng", [BEAMS, RANDOM], ids=["beams", "random"])
def test_masks_and_compaction(G, frame, rng):
    _, pred, gt = frame
    predm, gtm, _, near = ref_masks(pred, gt, camera(), rng)
    pix, N_PL, N_L = G.prepare(dev(pred), dev(gt), camera(), rng)
    pix = pix.cpu().numpy()
    got_pl, got_l = np.zeros_like(predm), np.zeros_like(gtm)
    got_pl[pix[:N_PL]] = True
    got_l[pix[N_PL:N_PL + N_L]] = True
    bad = (got_pl != predm) | (got_l != gtm)
    print("N_PL %d N_L %d, mismatches %d (all within 1e-12 rad of a pitch bound: %s)" % (N_PL, N_L, bad.sum(), bool(near[bad].all())))
    assert near[bad].all()
    assert N_L > 100 and N_PL > 1000
    if not bad.any():
        assert (N_PL, N_L) == (predm.sum(), gtm.sum())
        np.testing.assert_array_equal(pix[:N_PL], np.flatnonzero(predm))
        np.testing.assert_array_equal(pix[N_PL:N_PL + N_L], np.flatnonzero(gtm))
    assert np.all(np.diff(pix[:N_PL]) > 0) and np.all(np.diff(pix[N_PL:N_PL + N_L]) > 0)


def _points(G, pred, pix, N_PL, N_L):
    pc = cloud(pred, camera())
    sel = pix.cpu().numpy()[:N_PL + N_L]
    return pc[sel], pred.reshape(-1)[sel].astype(np.float64)


@pytest.mark.parametrize("rng", [BEAMS, RANDOM], ids=["beams", "random"])
def test_knn_exact(G, frame, rng):
    _, pred, gt = frame
    k = 10
    pix, N_PL, N_L, ws = gpu_stage(G, pred, gt, rng, k)
    pts, _ = _points(G, pred, pix, N_PL, N_L)
    got = G.ws_view(ws, N_PL, N_L, k, "nbr").cpu().numpy().reshape(-1, k)
    np.testing.assert_array_equal(G.ws_view(ws, N_PL, N_L, k, "px").cpu().numpy(), pts[:, 0])      # bit-identical positions
    dist, ind = cKDTree(pts).query(pts, k=k + 1)
    dref = dist[:, 1:] ** 2
    dgot = ((pts[got] - pts[:, None, :]) ** 2).sum(-1)
    assert np.all(np.diff(dgot, axis=1) >= 0)
    rel = np.abs(dgot - dref) / np.maximum(dref, 1e-300)
    print("N = %d, max rel distance difference %.3e" % (pts.shape[0], rel.max()))
    assert rel.max() <= 1e-12
    assert np.array_equal(np.sort(got, 1), np.sort(ind[:, 1:], 1))


def test_weights(G, frame):
    _, pred, gt = frame
    k = 10
    pix, N_PL, N_L, ws = gpu_stage(G, pred, gt, BEAMS, k)
    _, x_info = _points(G, pred, pix, N_PL, N_L)
    nbr = G.ws_view(ws, N_PL, N_L, k, "nbr").cpu().numpy().reshape(-1, k)
    w = G.ws_view(ws, N_PL, N_L, k, "w").cpu().numpy().reshape(-1, k)
    ref = ref_weights(x_info, nbr, k, 3e-5)
    xn = x_info[nbr]
    det = k * (xn * xn).sum(1) - xn.sum(1) ** 2
    ok = det > 1e-6 * xn.sum(1) ** 2            # the 2x2 Schur block is not near-singular
    rel = np.abs(w - ref).max(1) / np.abs(ref).max(1)
    print("rows %d, well-conditioned %d, max rel weight difference there %.3e" % (w.shape[0], ok.sum(), rel[ok].max()))
    assert ok.mean() > 0.9
    assert rel[ok].max() <= 1e-9
    assert np.abs(w.sum(1) - 1).max() <= 1e-9
    assert (np.abs((w * xn).sum(1) - x_info) / x_info).max() <= 1e-9


@pytest.mark.parametrize("rng", [BEAMS, RANDOM], ids=["beams", "random"])
def test_cg_fixed_iterations(G, frame, rng):
    """maxiter = 50, recon_tol = 0: the iterate against scipy's cg on the same A and b (built from the GPU's neighbours and
    weights, so that only the solver is compared).  The gate is norm-wise: ||x - x_scipy|| / ||x_scipy|| <= 1e-8, or at most
    4x the distance between two scipy runs that differ only in the order of the A^T sums (rows of A permuted), where scipy's
    own rounding spread is larger than 1e-8.  Measured on MI355X: 4.6e-9 (scipy vs scipy 9.5e-9), 6.3e-10 (3.9e-10),
    2.3e-7 (1.1e-7: the 370x1224 beam scene is the worst conditioned), 1.1e-9 (1.1e-9).  Element-wise the iterate is
    rounding-sensitive for both (largest entry differences 2e-7 ... 2e-5, printed)."""
    _, pred, gt = frame
    k = 10
    pix, N_PL, N_L, ws = gpu_stage(G, pred, gt, rng, k, recon_tol=0.0)
    _, x_info = _points(G, pred, pix, N_PL, N_L)
    nbr = G.ws_view(ws, N_PL, N_L, k, "nbr").cpu().numpy().reshape(-1, k)
    w = G.ws_view(ws, N_PL, N_L, k, "w").cpu().numpy().reshape(-1, k)
    g = gt.reshape(-1)[pix.cpu().numpy()[N_PL:N_PL + N_L]]
    A, b = ref_system(nbr, w, N_PL, g)
    np.testing.assert_allclose(G.ws_view(ws, N_PL, N_L, k, "b").cpu().numpy(), b, rtol=1e-13, atol=1e-12)
    xr, its, info = ref_cg(A, b, x_info[:N_PL], 0.0, 50)
    st = G.solve(ws, N_PL, N_L, k, 50)
    x = G.ws_view(ws, N_PL, N_L, k, "x").cpu().numpy()
    perm = np.random.RandomState(0).permutation(A.shape[0])
    xp, _, _ = ref_cg(A[perm], b[perm], x_info[:N_PL], 0.0, 50)
    rel = np.linalg.norm(x - xr) / np.linalg.norm(xr)
    print("N_PL %d: iterations %d / %d, ||x - x_scipy|| / ||x_scipy|| %.3e (scipy reordered: %.3e); element-wise max %.3e "
          "(scipy reordered: %.3e)" % (N_PL, st.iterations, its, rel, np.linalg.norm(xp - xr) / np.linalg.norm(xr),
                                       (np.abs(x - xr) / np.abs(xr)).max(), (np.abs(xp - xr) / np.abs(xr)).max()))
    assert st.iterations == 50 == its and info == 50
    assert rel <= max(1e-8, 4 * np.linalg.norm(xp - xr) / np.linalg.norm(xr))


@pytest.mark.parametrize("rng", [BEAMS, RANDOM], ids=["beams", "random"])
def test_default_settings_end_to_end(G, frame, rng):
    """W_tol = 3e-5, recon_tol = 5e-4.  The stopping iteration is rounding-sensitive: scipy against itself with only the order of
    the A^T sums changed stops at 71 / 76 (375x1242, beams) and 71 / 75 (370x1224, random sample) on these scenes, so the device's
    count is held to scipy's +-5, not +-2 (measured on MI355X: +1, -2, +3, -1)."""
    truth, pred, gt = frame
    ref = ref_gdc(pred, gt, camera(), rng=rng)
    out, info = G.GDC(dev(pred), dev(gt), camera(), W_tol=3e-5, recon_tol=5e-4, k=10, method="cg", consider_range=rng,
                      return_info=True)
    out = out.cpu().numpy()
    assert out.dtype == np.float32
    assert (info.N_PL, info.N_L) == (ref["N_PL"], ref["N_L"])
    print("iterations %d (scipy %d), rel residual %.3e, status %s" % (info.iterations, ref["its"], info.rel_residual, info.status))
    assert info.status == "converged" and abs(info.iterations - ref["its"]) <= 5
    assert info.rel_residual < 5e-4
    outside = ~ref["predm"].reshape(out.shape)
    assert np.array_equal(out[outside].view(np.uint32), ref["out"][outside].view(np.uint32))
    d = np.abs(out[~outside].astype(np.float64) - ref["out"][~outside])
    print("|d depth| at pred_mask pixels: max %.3e m, 99.9th pct %.3e m; mean |correction| %.3f m"
          % (d.max(), np.percentile(d, 99.9), np.abs(out[~outside] - pred[~outside]).mean()))
    assert d.max() < 0.5
    e0, e1 = np.abs(pred[~outside] - truth[~outside]).mean(), np.abs(out[~outside] - truth[~outside]).mean()
    print("mean |depth - truth| at pred_mask pixels: %.3f m before, %.3f m after" % (e0, e1))


def test_no_lidar_in_range(G):
    _, pred, gt = scene(375, 1242, seed=3)
    gt = np.full_like(gt, -1.0)
    ref = ref_gdc(pred, gt, camera())
    out, info = G.GDC(dev(pred), dev(gt), camera(), W_tol=3e-5, recon_tol=5e-4, k=10, method="cg", consider_range=BEAMS,
                      return_info=True)
    out = out.cpu().numpy()
    assert info.N_L == 0 and info.status == "converged" and info.iterations == 0
    assert np.all(ref["x"] == 0)
    assert np.array_equal(out.view(np.uint32), ref["out"].view(np.uint32))


def test_no_pseudo_lidar_points(G):
    _, pred, _ = scene(375, 1242, seed=4)
    gt = pred.astype(np.float64)                       # every considered pixel has a LiDAR point at its own depth
    out, info = G.GDC(dev(pred), dev(gt), camera(), W_tol=3e-5, recon_tol=5e-4, k=10, method="cg", consider_range=BEAMS,
                      return_info=True)
    out = out.cpu().numpy()
    assert info.N_PL == 0 and info.N_L > 100 and info.status == "converged"
    want = pred.copy()
    want[gt > 0] = gt[gt > 0]
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


def test_too_few_points_fails(G):
    _, pred, gt = scene(375, 1242, seed=5)
    pred = np.full_like(pred, 100.0)                   # outside z < 80 everywhere ...
    row = int(round(camera().c_v + 20))
    pred[row, 600:605] = 30.0                          # ... but for 5 pixels
    out, info = G.GDC(dev(pred), dev(gt), camera(), k=10, method="cg", consider_range=BEAMS, return_info=True)
    assert info.status == "failed" and info.N_PL + info.N_L == 5
    assert np.array_equal(out.cpu().numpy(), pred)


def test_deterministic(G):
    _, pred, gt = scene(375, 1242, seed=6)
    runs = [G.GDC(dev(pred), dev(gt), camera(), W_tol=3e-5, recon_tol=5e-4, method="cg", consider_range=RANDOM, return_info=True)
            for _ in range(2)]
    assert runs[0][1] == runs[1][1]
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))


def test_errors_and_options(G):
    _, pred, gt = scene(375, 1242, seed=7)
    with pytest.raises(NotImplementedError):
        G.GDC(dev(pred), dev(gt), camera(), subsample=True)
    with pytest.raises(NotImplementedError):
        G.GDC(dev(pred), dev(gt), camera(), verbose=True)


def _metrics(gt, pred):
    thresh = np.maximum(gt / pred, pred / gt)
    a1, a2, a3 = (thresh < 1.25).mean(), (thresh < 1.25 ** 2).mean(), (thresh < 1.25 ** 3).mean()
    rmse = np.sqrt(((gt - pred) ** 2).mean())
    rmse_log = np.sqrt(((np.log(gt) - np.log(pred)) ** 2).mean())
    return np.array([np.mean(np.abs(gt - pred) / gt), np.mean((gt - pred) ** 2 / gt), rmse, rmse_log, a1, a2, a3])


def test_evaluate_predictions_eval_gdc(G):
    from fusiondepth_amd import evaluate_depth as E
    from fusiondepth_amd import functional as FD
    truth, pred, lidar = scene(375, 1242, seed=8)
    gt = truth.astype(np.float32)
    disp = torch.nn.functional.interpolate(dev(1.0 / pred)[None, None], size=(192, 640), mode="bilinear", align_corners=False)[0]
    beam = np.where(lidar > 0, lidar, 0.0)
    base, _ = E.evaluate_predictions(disp, [gt])
    same, _ = E.evaluate_predictions(disp, [gt], eval_gdc=False, beam_depths=[beam], calibs=[camera()])
    assert np.array_equal(base, same)
    got, ratios = E.evaluate_predictions(disp, [gt], eval_gdc=True, beam_depths=[beam], calibs=[camera()])
    # restatement: the same resized disparity (OpenCV's rule, on the device), numpy median scaling, GDC, clamp, metrics
    pd = (1.0 / FD.resize_linear_cv(disp[None], (375, 1242))[0, 0]).cpu().numpy()
    mask = (gt > 1e-3) & (gt < 80)
    c = E.garg_crop(375, 1242)
    crop = np.zeros_like(mask)
    crop[c[0]:c[1], c[2]:c[3]] = True
    mask &= crop
    pd = pd * np.float32(np.median(gt[mask]) / np.median(pd[mask]))
    gtd = beam.copy()
    gtd[gtd == 0] = -1
    # GDC's own parity is the business of the tests above (its CG iterate is rounding-sensitive: the float64 restatement's
    # solution moves the metrics by ~1e-4 relative); here the restatement of the evaluation path takes the device's GDC of
    # the restated median-scaled depth, so what is compared is where and how evaluate_predictions applies it
    corrected, info = G.GDC(dev(pd), dev(gtd), camera(), W_tol=3e-5, recon_tol=5e-4, k=10, method="cg", consider_range=BEAMS,
                            return_info=True)
    assert info.status == "converged"
    corrected = corrected.cpu().numpy()
    want = _metrics(gt[mask].astype(np.float64), np.clip(corrected[mask], 1e-3, 80).astype(np.float64))
    full = ref_gdc(pd.astype(np.float32), gtd, camera(), rng=BEAMS)["out"]
    want_ref = _metrics(gt[mask].astype(np.float64), np.clip(full[mask], 1e-3, 80).astype(np.float64))
    print("metrics with GDC", got, "restatement", want, "with the scipy GDC", want_ref, "without", base)
    np.testing.assert_allclose(got, want, rtol=1e-4)
    np.testing.assert_allclose(got, want_ref, rtol=2e-3)
    assert not np.allclose(got, base, rtol=1e-3)


def test_inf_gdc_driver(G, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import inputs as gin
    from fusiondepth_amd import evaluate_depth as E
    from fusiondepth_amd import functional as FD
    from fusiondepth_amd import inf_gdc
    from fusiondepth_amd.kitti_utils import Calibration, velo_to_image
    velo, _ = gin.lidar_scan(11)
    cal = gin.lidar_scan.calib
    date, drive, frame_id = "2011_09_26", "2011_09_26_drive_0001_sync", 7
    ddir = tmp_path / date
    (ddir / drive / "4beam").mkdir(parents=True)
    (ddir / drive / "inf_depth_4beam").mkdir()
    P3 = cal["P_rect_02"].copy()
    P3[0, 3] = -339.5242
    fmt = lambda a: " ".join(repr(float(v)) for v in np.asarray(a).reshape(-1))
    (ddir / "calib_cam_to_cam.txt").write_text("calib_time: 09-Jan-2012 13:57:47\nS_rect_02: %s\nR_rect_00: %s\nP_rect_02: %s\n"
                                               "P_rect_03: %s\n" % (fmt(cal["S_rect_02"]), fmt(cal["R_rect_00"]),
                                                                     fmt(cal["P_rect_02"]), fmt(P3)))
    (ddir / "calib_velo_to_cam.txt").write_text("R: %s\nT: %s\n" % (fmt(cal["R"]), fmt(cal["T"])))
    velo.tofile(str(ddir / drive / "4beam" / ("%010d.bin" % frame_id)))
    yy, xx = np.meshgrid(np.arange(192), np.arange(640), indexing="ij")
    disp = (0.03 + 0.02 * np.sin(xx / 70.0) * np.cos(yy / 40.0) + 0.0005 * np.random.RandomState(2).randn(192, 640))
    disp = disp.astype(np.float32)[None, None]
    np.save(str(ddir / drive / "inf_depth_4beam" / ("%d_l.npy" % frame_id)), disp)
    split = tmp_path / "split.txt"
    split.write_text("%s/%s %d l\n" % (date, drive, frame_id))
    assert inf_gdc.main(["--data_path", str(tmp_path), "--split_files", str(split)]) == 0
    got = np.load(str(ddir / drive / "inf_gdc_4beam" / ("%d_l.npy" % frame_id)))
    assert got.dtype == np.float32 and got.shape == (375, 1242)
    # the same frame through GDC directly
    P, (im_h, im_w) = velo_to_image(str(ddir), 2)
    scan = velo.copy()
    scan[:, 3] = 1
    lidar = FD.velo_rasterize(dev(scan), P, im_h, im_w, None, return_full=True, vel_depth=True, beam=False)
    scaled, _ = FD.disp_to_depth(dev(disp[0, 0]), 0.1, 100.0)
    depth = 1.0 / FD.resize_linear_cv(scaled[None, None], (375, 1242))[0, 0]
    m = (lidar > 1e-3) & (lidar < 80)
    c = E.garg_crop(375, 1242)
    crop = torch.zeros_like(m)
    crop[c[0]:c[1], c[2]:c[3]] = True
    m &= crop
    depth = (depth.double() * (E._median(lidar[m]) / E._median(depth[m]).double())).float()
    lidar[lidar == 0] = -1
    want = G.GDC(depth, lidar, Calibration(str(ddir / "calib_cam_to_cam.txt")), W_tol=3e-5, recon_tol=5e-4, k=10, method="cg",
                 consider_range=(-0.1, 4.0)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # what a Refiner loader does with the file: bilinear resize to the network size
    small = torch.nn.functional.interpolate(dev(got)[None, None], size=(192, 640), mode="bilinear", align_corners=False)
    assert torch.isfinite(small).all()
