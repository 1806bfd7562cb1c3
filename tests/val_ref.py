"""numpy restatement of the trainer's validation metrics (the reference's ``compute_depth_losses``, trainer.py:598-630, plus
``compute_depth_errors``, layers.py:284-302) per image, for the tests of the fused scorer (``fd_val_scores``), and the same chain in
torch on the CPU, to which the restatement is pinned (tests/test_train_cli_cpu.py).  A helper, not a test.

Every element-wise step is one float32 operation; the fused multiply-adds of ATen's bilinear rule are formed in float64 and rounded
once (the product of two float32 values is exact in float64).  The reference takes ``.mean()`` of float32 tensors; here the sums of
the float32 terms run in float64, which is what the kernel does and the tighter statement.  The log term is the kernel's:
``float32(log(float64(gt)) - log(float64(pred)))`` squared in float32 (a float32 ``log`` cannot be restated bit for bit)."""
import functools

import numpy as np

F32 = np.float32
CROP = (153, 371, 44, 1197)
PRED_SIZE = (64, 96)


# ------------------------------------------------------------------------------------------------ ATen's bilinear rule (fdhip.h)
def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _axis(n_in, n_out):
    scale = F32(n_in) / F32(n_out)
    d = np.arange(n_out, dtype=F32) + F32(0.5)
    src = _fma(np.full(n_out, scale, F32), d, np.full(n_out, -0.5, F32))
    src = np.maximum(src, F32(0))
    i0 = np.minimum(src.astype(np.int32), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(F32)
    return i0, i1, F32(1.0) - l1, l1


def resize_rule(x, size):
    """F.interpolate(x, size, mode="bilinear", align_corners=False) on the CPU, float32: width first, then height."""
    x = np.asarray(x, dtype=F32)
    y0, y1, hy, ly = _axis(x.shape[0], size[0])
    x0, x1, hx, lx = _axis(x.shape[1], size[1])
    hx, lx, hy, ly = hx[None, :], lx[None, :], hy[:, None], ly[:, None]
    top = _fma(hx, x[y0][:, x0], lx * x[y0][:, x1])
    bot = _fma(hx, x[y1][:, x0], lx * x[y1][:, x1])
    return _fma(hy, top, ly * bot)


def clip_window(H, W, window=None):
    y0, y1, x0, x1 = CROP if window is None else window
    y1, x1 = min(max(y1, 0), H), min(max(x1, 0), W)
    return min(max(y0, 0), y1), y1, min(max(x0, 0), x1), x1


def _clamp(p, lo, hi):
    p = np.where(p < F32(lo), F32(lo), p)                        # a NaN stays
    return np.where(p > F32(hi), F32(hi), p).astype(F32)


def lower_median(v):
    """torch.median of a 1-D float32 array: the element of rank (n - 1) // 2; NaN when one is present or nothing is selected."""
    if not v.size or np.isnan(v).any():
        return F32(np.nan)
    return np.sort(v)[(v.size - 1) // 2]


# ------------------------------------------------------------------------------------------------ the restatement
def val_scores(depths, gt_depths, window=None, lo=1e-3, hi=80):
    """-> dict of per-image results: ``counts`` [N], ``med_gt`` / ``med_pred`` / ``ratios`` [N] float32, ``thresh_counts`` [N,3] and
    ``metrics`` [N,7] float64 (float64 sums of the float32 terms; NaN rows where nothing is selected)."""
    res = {k: [] for k in ("counts", "med_gt", "med_pred", "ratios", "thresh_counts", "metrics")}
    with np.errstate(all="ignore"):
        for depth, gt in zip(depths, gt_depths):
            gt = np.asarray(gt, F32)
            H, W = gt.shape
            y0, y1, x0, x1 = clip_window(H, W, window)
            mask = np.zeros(gt.shape, bool)
            mask[y0:y1, x0:x1] = gt[y0:y1, x0:x1] > 0
            g = gt[mask]
            p = _clamp(resize_rule(depth, (H, W))[mask], lo, hi)
            mg, mp = lower_median(g), lower_median(p)
            ratio = F32(mg) / F32(mp)
            p = _clamp(p * ratio, lo, hi)
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


# ------------------------------------------------------------------------------------------------ the reference's expression
def torch_reference(depth, gt):
    """The same chain in torch on the CPU, operation for operation as the reference's trainer forms it (``F.interpolate``, clamp, mask
    and crop, ``torch.median`` of both selections, scale, clamp, then the seven float32 ``.mean()`` metrics), for one image with a
    non-empty selection -> dict with the count, both medians, the ratio, the three threshold counts and the seven metrics."""
    import torch
    import torch.nn.functional as F
    p = torch.from_numpy(np.array(depth, F32))[None, None]               # copies: the shared cases are read-only
    g = torch.from_numpy(np.array(gt, F32))[None, None]
    p = torch.clamp(F.interpolate(p, list(g.shape[2:]), mode="bilinear", align_corners=False), 1e-3, 80)
    inside = torch.zeros_like(g, dtype=torch.bool)
    inside[:, :, CROP[0]:CROP[1], CROP[2]:CROP[3]] = True
    sel = (g > 0) & inside
    g, p = g[sel], p[sel]
    med_g, med_p = torch.median(g), torch.median(p)
    p = torch.clamp(p * (med_g / med_p), min=1e-3, max=80)
    worse = torch.max(g / p, p / g)
    below = [worse < 1.25 ** k for k in (1, 2, 3)]
    diff = g - p
    means = [torch.mean(diff.abs() / g), torch.mean(diff ** 2 / g), torch.sqrt(torch.mean(diff ** 2)),
             torch.sqrt(torch.mean((torch.log(g) - torch.log(p)) ** 2))] + [b.float().mean() for b in below]
    return {"count": int(g.numel()), "med_gt": med_g.numpy(), "med_pred": med_p.numpy(), "ratio": (med_g / med_p).numpy(),
            "thresh_counts": [int(b.sum()) for b in below], "metrics": np.array([float(v) for v in means])}


# ------------------------------------------------------------------------------------------------ shared cases
def sparse_gt(rng, H, W, valid=0.05, odd=None):
    """A float32 [H,W] map, ``valid`` of it in (0.5, 80), the rest 0.  ``odd``: make the selected count inside the Garg crop odd
    (True) or even (False) by clearing one selected pixel if need be."""
    gt = np.where(rng.random((H, W)) < valid, rng.uniform(0.5, 80.0, (H, W)), 0.0).astype(F32)
    if odd is not None:
        y0, y1, x0, x1 = clip_window(H, W)
        win = gt[y0:y1, x0:x1]
        if (int((win > 0).sum()) % 2 == 1) != odd:
            ys, xs = np.nonzero(win > 0)
            win[ys[0], xs[0]] = 0.0
    return gt


def depth_pred(rng, n=None):
    """Predicted depths at ``PRED_SIZE``, log-uniform in (0.5, 120): some leave the clamp range above."""
    shape = PRED_SIZE if n is None else (n,) + PRED_SIZE
    return np.exp(rng.uniform(np.log(0.5), np.log(120.0), shape)).astype(F32)


@functools.lru_cache(maxsize=None)
def six_case():
    """The six images of tests/test_gpu_val_scores.py -> (depths [6,64,96], ground-truth maps, the restatement's result).  Computed
    once per process; callers must leave it unchanged."""
    rng = np.random.default_rng(2024)
    depths = depth_pred(rng, 6)
    gts = [sparse_gt(rng, 375, 1242, odd=False), sparse_gt(rng, 370, 1226, odd=True)]
    nothing = sparse_gt(rng, 375, 1242)
    nothing[153:371, 44:1197] = 0.0                              # valid pixels, but none inside the crop
    gts.append(nothing)
    gts.append(sparse_gt(rng, 128, 192, valid=0.5))              # the clipped crop is empty
    gts.append(sparse_gt(rng, 375, 1242))
    depths[4, 30, 40] = np.nan                                   # a NaN in the prediction of image 4
    gts.append(rng.uniform(0.5, 80.0, (375, 1242)).astype(F32))  # valid everywhere: 218 * 1153 = 251 354 pairs
    depths.setflags(write=False)
    for g in gts:
        g.setflags(write=False)
    return depths, gts, val_scores(depths, gts)
