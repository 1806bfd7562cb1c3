"""numpy restatement of the per-image loop of the reference's ``evaluate_depth.py`` (:344-478, without GDC) for the tests of the batched
scorer (``fd_eigen_scores``): every intermediate the kernel's result can be held against.  A helper, not a test.

The resize is ``oracle.evaluate.resize_bilinear``; every element-wise step is a float32 numpy operation, as in the reference.  The
reference then takes ``.mean()`` of float32 arrays (numpy's pairwise float32 sum); here the sums of the float32 terms run in float64,
which is what the kernel does and the tighter statement.  ``metrics64`` takes the two logarithms in float64 as well."""
import numpy as np

from oracle import evaluate as OE

F32 = np.float32


def restate(pred_disps, gt_depths, eval_split="eigen", pred_depth_scale_factor=1.0, disable_median_scaling=False, lo=1e-3, hi=80):
    """-> dict of per-image results: ``counts`` [N], ``thresh_counts`` [N,3], ``ratios`` [N] float32 (NaN without median scaling),
    ``metrics`` [N,7] (float64 sums of the float32 terms), ``metrics64`` [N,7] (the same with float64 logarithms) and ``terms``:
    a list of dicts of the float32 per-pixel terms (abs_rel, sq_rel, sq, log_sq, thresh) plus ``log_sq64``."""
    res = {"counts": [], "thresh_counts": [], "ratios": [], "metrics": [], "metrics64": [], "terms": []}
    with np.errstate(all="ignore"):
        for disp, gt in zip(pred_disps, gt_depths):
            gt = np.asarray(gt, F32)
            gh, gw = gt.shape
            pred = F32(1) / OE.resize_bilinear(np.asarray(disp, F32), gh, gw)
            if eval_split in ("eigen", "demo"):
                mask = np.logical_and(gt > F32(1e-3), gt < F32(80))
                c = np.array([0.40810811 * gh, 0.99189189 * gh, 0.03594771 * gw, 0.96405229 * gw]).astype(np.int32)
                crop = np.zeros(mask.shape, bool)
                crop[c[0]:c[1], c[2]:c[3]] = True
                mask = np.logical_and(mask, crop)
            else:
                mask = gt > 0
            pred = pred * F32(pred_depth_scale_factor)
            ratio = F32(np.nan)
            g = gt[mask]
            if not disable_median_scaling:
                if g.size:
                    ratio = F32(np.median(g)) / F32(np.median(pred[mask]))
                pred = pred * ratio
            p = pred[mask]
            p[p < F32(lo)] = F32(lo)
            p[p > F32(hi)] = F32(hi)
            thresh = np.maximum(g / p, p / g)
            d = g - p
            sq = d * d
            t = {"abs_rel": np.abs(d) / g, "sq_rel": sq / g, "sq": sq, "log_sq": (np.log(g) - np.log(p)) ** 2, "thresh": thresh}
            t["log_sq64"] = (np.log(g.astype(np.float64)) - np.log(p.astype(np.float64))) ** 2
            assert all(v.dtype == F32 for k, v in t.items() if k != "log_sq64")
            n = np.float64(g.size)
            tc = [int((thresh < F32(1.25 ** k)).sum()) for k in (1, 2, 3)]
            s = lambda v: v.sum(dtype=np.float64)
            row = [s(t["abs_rel"]) / n, s(t["sq_rel"]) / n, np.sqrt(s(t["sq"]) / n), np.sqrt(s(t["log_sq"]) / n)] + [c / n for c in tc]
            row64 = list(row)
            row64[3] = np.sqrt(s(t["log_sq64"]) / n)
            res["counts"].append(g.size)
            res["thresh_counts"].append(tc)
            res["ratios"].append(ratio)
            res["metrics"].append(row)
            res["metrics64"].append(row64)
            res["terms"].append(t)
    for k in ("counts", "thresh_counts"):
        res[k] = np.array(res[k], np.int64).reshape(len(res["terms"]), -1 if k == "thresh_counts" else 1)
    res["counts"] = res["counts"].reshape(-1)
    res["ratios"] = np.array(res["ratios"], F32)
    res["metrics"], res["metrics64"] = np.array(res["metrics"], np.float64).reshape(-1, 7), np.array(res["metrics64"], np.float64).reshape(-1, 7)
    return res
