"""numpy restatement of the Completor's validation metrics (the reference's ``compute_depth_losses``, completor.py:728-762, plus
``compute_depth_errors``, layers.py:284-302) per image, for the tests of the fused scorer (``fd_completion_val_scores``), and the same
chain in torch on the CPU, to which the restatement is pinned (tests/test_stage_cli_cpu.py).  A helper, not a test.

What differs from tests/val_ref.py: the mask is ``gt > float32(0.1)`` over the whole map (inside the Garg crop only with
``eigen_crop``), and after the second clamp both sides are multiplied by ``float32(1000)`` - one rounding each - before the seven
terms.  As there, the sums of the float32 terms run in float64 and the log term is ``float32(log(float64(g')) - log(float64(p')))``."""
import functools

import numpy as np

from val_ref import CROP, F32, _clamp, clip_window, lower_median, resize_rule

GT_MIN = F32(0.1)
MM = F32(1000.0)
EDGE = (np.nextafter(GT_MIN, F32(0)), GT_MIN, np.nextafter(GT_MIN, F32(1)))      # float32(0.1) and its two neighbours
WHOLE = (0, 1 << 30, 0, 1 << 30)


def window_of(eigen_crop):
    return CROP if eigen_crop else WHOLE


def completion_val_scores(depths, gt_depths, eigen_crop=False, window=None, lo=1e-3, hi=80):
    """-> dict of per-image results: ``counts`` [N], ``med_gt`` / ``med_pred`` / ``ratios`` [N] float32, ``thresh_counts`` [N,3] and
    ``metrics`` [N,7] float64 (float64 sums of the float32 terms; NaN rows where nothing is selected)."""
    window = window_of(eigen_crop) if window is None else window
    res = {k: [] for k in ("counts", "med_gt", "med_pred", "ratios", "thresh_counts", "metrics")}
    with np.errstate(all="ignore"):
        for depth, gt in zip(depths, gt_depths):
            gt = np.asarray(gt, F32)
            H, W = gt.shape
            y0, y1, x0, x1 = clip_window(H, W, window)
            mask = np.zeros(gt.shape, bool)
            mask[y0:y1, x0:x1] = gt[y0:y1, x0:x1] > GT_MIN
            g = gt[mask]
            p = _clamp(resize_rule(depth, (H, W))[mask], lo, hi)
            mg, mp = lower_median(g), lower_median(p)
            ratio = F32(mg) / F32(mp)
            p = _clamp(p * ratio, lo, hi)
            g, p = g * MM, p * MM                                # millimetres
            thresh = np.maximum(g / p, p / g)
            d = g - p
            sq = d * d
            dl = (np.log(g.astype(np.float64)) - np.log(p.astype(np.float64))).astype(F32)
            terms = [np.abs(d) / g, sq / g, sq, dl * dl]
            assert all(t.dtype == F32 for t in terms) and thresh.dtype == F32
            n = np.float64(g.size)
            s = [t.sum(dtype=np.float64) for t in terms]
            tc = [int((thresh < F32(1.25 ** k)).sum()) for k in (1, 2, 3)]
            res["metrics"].append([s[0] / n, s[1] / n, np.sqrt(s[2] / n), np.sqrt(s[3] / n)] + [c / n for c in tc])
            res["counts"].append(g.size)
            res["med_gt"].append(mg)
            res["med_pred"].append(mp)
            res["ratios"].append(ratio)
            res["thresh_counts"].append(tc)
    res["counts"] = np.array(res["counts"], np.int64)
    res["thresh_counts"] = np.array(res["thresh_counts"], np.int64).reshape(-1, 3)
    res["metrics"] = np.array(res["metrics"], np.float64).reshape(-1, 7)
    for k in ("med_gt", "med_pred", "ratios"):
        res[k] = np.array(res[k], F32)
    return res


def torch_reference(depth, gt, eigen_crop=False):
    """The same chain in torch on the CPU, operation for operation as completor.py:730-762 and layers.py:284-302 form it, for one
    image with a non-empty selection -> dict with the count, both medians, the ratio, the three threshold counts and the seven
    metrics (torch's own float32 ``.mean()`` values)."""
    import torch
    import torch.nn.functional as F
    p = torch.from_numpy(np.array(depth, F32))[None, None]
    g = torch.from_numpy(np.array(gt, F32))[None, None]
    if tuple(p.shape[2:]) != tuple(g.shape[2:]):
        p = F.interpolate(p, list(g.shape[2:]), mode="bilinear", align_corners=False)
    p = torch.clamp(p, 1e-3, 80)
    mask = g > 0.1
    if eigen_crop:
        crop = torch.zeros_like(mask)
        crop[:, :, 153:371, 44:1197] = 1
        mask = mask * crop
    g, p = g[mask], p[mask]
    med_g, med_p = torch.median(g), torch.median(p)
    p = torch.clamp(p * (med_g / med_p), min=1e-3, max=80)
    g, p = g * 1000.0, p * 1000.0
    worse = torch.max(g / p, p / g)
    below = [worse < 1.25 ** k for k in (1, 2, 3)]
    diff = g - p
    means = [torch.mean(diff.abs() / g), torch.mean(diff ** 2 / g), torch.sqrt(torch.mean(diff ** 2)),
             torch.sqrt(torch.mean((torch.log(g) - torch.log(p)) ** 2))] + [b.float().mean() for b in below]
    return {"count": int(g.numel()), "med_gt": med_g.numpy(), "med_pred": med_p.numpy(), "ratio": (med_g / med_p).numpy(),
            "thresh_counts": [int(b.sum()) for b in below], "metrics": np.array([float(v) for v in means])}


# ------------------------------------------------------------------------------------------------ shared cases
def sparse_gt(rng, H, W, valid=0.15, odd=None, eigen_crop=False, edge=True):
    """A float32 [H,W] map, ``valid`` of it in (0.5, 80), the rest 0 - except, with ``edge``, three pixels inside every window that
    hold float32(0.1) and its two neighbours (only the upper one is selected).  ``odd``: make the selected count odd / even."""
    gt = np.where(rng.random((H, W)) < valid, rng.uniform(0.5, 80.0, (H, W)), 0.0).astype(F32)
    y0, y1, x0, x1 = clip_window(H, W, window_of(eigen_crop))
    win = gt[y0:y1, x0:x1]
    if edge and win.size >= 8:
        cy, cx = (y1 - y0) // 2, (x1 - x0) // 2
        win[cy, cx:cx + 3] = EDGE
    if odd is not None and (int((win > GT_MIN).sum()) % 2 == 1) != odd:
        ys, xs = np.nonzero(win > F32(0.2))
        win[ys[0], xs[0]] = 0.0
    return gt


def depth_pred(rng, shape):
    """Predicted depths, log-uniform in (0.5, 120): some leave the clamp range above."""
    return np.exp(rng.uniform(np.log(0.5), np.log(120.0), shape)).astype(F32)


PRED_SIZE = (48, 160)


@functools.lru_cache(maxsize=None)
def mixed_case():
    """The images of tests/test_gpu_completion_val.py's single call -> (depths [9,48,160], ground-truth maps, windows' flag,
    the restatement's result).  All are scored with ``eigen_crop`` windows or whole maps as ``crops`` says.  Computed once per
    process; callers must leave it unchanged."""
    rng = np.random.default_rng(1812)
    depths = depth_pred(rng, (9,) + PRED_SIZE)
    gts, crops = [], []
    gts.append(sparse_gt(rng, 37, 101, valid=0.3, odd=False)); crops.append(False)           # 0: even; 101 % 64, 37 % 4 != 0
    gts.append(sparse_gt(rng, 37, 101, valid=0.3, odd=True)); crops.append(False)            # 1: odd
    gts.append(rng.uniform(0.5, 80.0, (96, 128)).astype(F32)); crops.append(False)           # 2: fully valid, 12288 pairs
    nothing = np.where(rng.random((40, 100)) < 0.5, GT_MIN, 0.0).astype(F32)                 # 3: all gt <= 0.1
    nothing[5, 5:8] = (EDGE[0], EDGE[1], 0.05)
    gts.append(nothing); crops.append(False)
    gts.append(sparse_gt(rng, 352, 1216, valid=0.02, eigen_crop=True)); crops.append(True)   # 4: the crop clipped to rows 153:352
    gts.append(sparse_gt(rng, 128, 192, valid=0.5, eigen_crop=True)); crops.append(True)     # 5: the crop clipped away entirely
    gts.append(sparse_gt(rng, 40, 100, valid=0.4, edge=False)); crops.append(False)          # 6: a NaN prediction inside the selection
    gts.append(sparse_gt(rng, *PRED_SIZE, valid=0.3)); crops.append(False)                   # 7: equal sizes
    gts.append(sparse_gt(rng, 96, 320, valid=0.1)); crops.append(False)                      # 8: pred 48x160 against gt 96x320
    gts[6][:] = np.where(gts[6] > 0, gts[6], F32(3.0))           # every pixel selected, so the NaN's bilinear footprint is too
    depths[6, 20, 70] = np.nan
    depths.setflags(write=False)
    for g in gts:
        g.setflags(write=False)
    want = [completion_val_scores(depths[i:i + 1], [g], eigen_crop=c) for i, (g, c) in enumerate(zip(gts, crops))]
    res = {k: np.concatenate([w[k] for w in want]) for k in want[0]}
    return depths, gts, crops, res
