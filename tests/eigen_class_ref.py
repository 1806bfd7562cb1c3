"""numpy restatement of the reference's ``--per_semantic`` loop (``evaluate_depth.py`` :451-467) and of its summary (:491-496) for the
tests of the per-class scorer (``fd_eigen_class_scores``, ``fd_class_errors``).  A helper, not a test.

Built on ``eigen_eval_ref.restate``: the mask is recomputed as the reference forms it, ``labels[mask]`` lies beside restate's float32
per-pixel ``terms`` (both in row-major order), and a class's row is made of the float64 sums of its terms - what the kernel does and
the tighter statement, as in ``eigen_eval_ref``.  ``metrics64`` takes the two logarithms in float64 as well.  The ratio is the whole
image's: only the selection differs between classes."""
import numpy as np

import eigen_eval_ref as REF

F32 = np.float32


def split_mask(gt, eval_split):
    """evaluate_depth.py:358-368."""
    gt = np.asarray(gt, F32)
    gh, gw = gt.shape
    if eval_split in ("eigen", "demo"):
        mask = np.logical_and(gt > F32(1e-3), gt < F32(80))
        c = np.array([0.40810811 * gh, 0.99189189 * gh, 0.03594771 * gw, 0.96405229 * gw]).astype(np.int32)
        crop = np.zeros(mask.shape, bool)
        crop[c[0]:c[1], c[2]:c[3]] = True
        return np.logical_and(mask, crop)
    return gt > 0


def class_rows(terms, labels, num_classes):
    """One image: restate's ``terms`` and the labels of the same pixels -> (counts [K], thresh_counts [K,3], metrics [K,7],
    metrics64 [K,7]); a class without pixels gives zeros, the reference's ``np.zeros(7)``."""
    K = num_classes
    counts, tcs = np.zeros(K, np.int64), np.zeros((K, 3), np.int64)
    rows, rows64 = np.zeros((K, 7)), np.zeros((K, 7))
    s = lambda v: v.sum(dtype=np.float64)
    with np.errstate(all="ignore"):
        for c in range(K):
            sel = labels == c
            n = int(sel.sum())
            counts[c] = n
            if n == 0:
                continue
            th = terms["thresh"][sel]
            tcs[c] = [int((th < F32(1.25 ** k)).sum()) for k in (1, 2, 3)]
            head = [s(terms["abs_rel"][sel]) / n, s(terms["sq_rel"][sel]) / n, np.sqrt(s(terms["sq"][sel]) / n)]
            tail = [t / np.float64(n) for t in tcs[c]]
            rows[c] = head + [np.sqrt(s(terms["log_sq"][sel]) / n)] + tail
            rows64[c] = head + [np.sqrt(s(terms["log_sq64"][sel]) / n)] + tail
    return counts, tcs, rows, rows64


def restate_classes(pred_disps, gt_depths, sem_masks, num_classes=34, eval_split="eigen", pred_depth_scale_factor=1.0,
                    disable_median_scaling=False, lo=1e-3, hi=80):
    """-> dict: ``image`` (``eigen_eval_ref.restate``'s result), ``labels`` (list of ``sem_mask[mask]``, uint8), ``counts`` [N,K],
    ``thresh_counts`` [N,K,3], ``metrics`` [N,K,7] (float64 sums of the float32 terms), ``metrics64`` [N,K,7] (the same with float64
    logarithms) and ``outside`` [N]: the selected pixels whose label is >= num_classes."""
    image = REF.restate(pred_disps, gt_depths, eval_split, pred_depth_scale_factor, disable_median_scaling, lo, hi)
    res = {"image": image, "labels": [], "counts": [], "thresh_counts": [], "metrics": [], "metrics64": [], "outside": []}
    for gt, sem, terms in zip(gt_depths, sem_masks, image["terms"]):
        sem = np.asarray(sem)
        assert sem.shape == np.asarray(gt).shape and sem.dtype == np.uint8
        labels = sem[split_mask(gt, eval_split)]
        assert labels.size == terms["thresh"].size
        counts, tcs, rows, rows64 = class_rows(terms, labels, num_classes)
        res["labels"].append(labels)
        res["counts"].append(counts)
        res["thresh_counts"].append(tcs)
        res["metrics"].append(rows)
        res["metrics64"].append(rows64)
        res["outside"].append(int((labels >= num_classes).sum()))
    N, K = len(res["labels"]), num_classes
    res["counts"] = np.array(res["counts"], np.int64).reshape(N, K)
    res["thresh_counts"] = np.array(res["thresh_counts"], np.int64).reshape(N, K, 3)
    res["metrics"], res["metrics64"] = np.array(res["metrics"]).reshape(N, K, 7), np.array(res["metrics64"]).reshape(N, K, 7)
    res["outside"] = np.array(res["outside"], np.int64)
    return res


def scaled_pairs(disp, gt, ratio, eval_split="eigen", pred_depth_scale_factor=1.0):
    """The matched lists of one image before the clamp, as the reference holds them at :455: ``gt[mask]`` and ``(pred * ratio)[mask]``
    in float32 (``ratio`` None: no median scaling), every step one float32 rounding as in ``eigen_eval_ref.restate``."""
    from oracle import evaluate as OE
    gt = np.asarray(gt, F32)
    with np.errstate(all="ignore"):
        pred = F32(1) / OE.resize_bilinear(np.asarray(disp, F32), *gt.shape)
        pred = pred * F32(pred_depth_scale_factor)
        if ratio is not None:
            pred = pred * F32(ratio)
    mask = split_mask(gt, eval_split)
    return gt[mask], pred[mask]


def pair_terms(g, p, lo=1e-3, hi=80):
    """``eigen_eval_ref.restate``'s per-pixel ``terms`` for matched float32 lists that are already scaled: the clamp, then every step a
    float32 numpy operation (what ``fd_class_errors`` is held against)."""
    g, p = np.asarray(g, F32), np.array(p, F32)
    with np.errstate(all="ignore"):
        p[p < F32(lo)] = F32(lo)
        p[p > F32(hi)] = F32(hi)
        d = g - p
        sq = d * d
        t = {"abs_rel": np.abs(d) / g, "sq_rel": sq / g, "sq": sq, "log_sq": (np.log(g) - np.log(p)) ** 2, "thresh": np.maximum(g / p, p / g)}
        t["log_sq64"] = (np.log(g.astype(np.float64)) - np.log(p.astype(np.float64))) ** 2
    assert all(v.dtype == F32 for k, v in t.items() if k != "log_sq64")
    return t


def summary(class_metrics, class_counts):
    """evaluate_depth.py:492-494 from [N,K,7] metrics and [N,K] counts -> [K]."""
    sem_errors = np.transpose(np.asarray(class_metrics, np.float64), (1, 0, 2))[:, :, 0]
    valid = np.asarray(class_counts, np.float64).T
    return (sem_errors * valid).sum(1) / (valid.sum(1) + 0.0000000000000001)
