"""numpy restatement of the reference's ``evaluate_depth.py --visualize`` branch (:407-449) for the tests of ``fd_vis_render``, and the
fixture inputs those tests share.  A helper, not a test.

Every element-wise step is one float32 numpy operation.  The percentile is numpy 2's ``np.percentile(x, 95)`` for float32 input
restated step by step (float32 virtual index, its ``_lerp``); the normalisation and the lookup are matplotlib's ``Normalize`` and
``Colormap.__call__``; ``block_reduce`` is ``skimage.measure.block_reduce(.., (2, 2, 1), np.max)`` (zero padding at an odd edge).  The
colour tables are arguments.  tests/test_visualize_cpu.py holds this file against numpy and matplotlib themselves."""
import numpy as np

import detection_ref as DR

F32 = np.float32

# (H, W): a single pixel; 1x2 (g = 0.95: the g >= 0.5 branch); 2x3 (g = 0.75); 1x21 and 1x41 (g = 0 with k + 1 in range); 7x5; 37x41
# (odd both ways, rows of 123 bytes)
SIZES = [(1, 1), (1, 2), (2, 3), (1, 21), (1, 41), (7, 5), (37, 41)]
SRC = (6, 20)
BIG = (375, 1242)                                                 # n = 465 750: k = 442 461 and g = 0.53125, not 0.55
BIG_SRC = (192, 640)


def percentile95(x):
    """``np.percentile(x, 95)`` of a float32 array as numpy 2 computes it -> float32 scalar."""
    s = np.sort(np.asarray(x, F32).reshape(-1))
    n = s.size
    q = F32(95.0) / F32(100.0)
    pos = F32(n - 1) * q
    k = int(np.floor(pos))
    g = F32(pos - F32(k))
    a, b = s[k], s[min(k + 1, n - 1)]
    with np.errstate(all="ignore"):
        diff = F32(b - a)
        out = F32(a + F32(diff * g))
        if g >= F32(0.5):
            out = F32(b - F32(diff * F32(F32(1.0) - g)))
    if a == b:
        out = a
    return F32(out)


def virtual_index(n):
    """(k, g) of the recipe above for n values."""
    pos = F32(n - 1) * (F32(95.0) / F32(100.0))
    k = int(np.floor(pos))
    return k, float(F32(pos - F32(k)))


def normalize(d, vmin, vmax):
    """``mpl.colors.Normalize(vmin, vmax)(d)`` for a float32 array and float32 limits -> float32 array.  Normalize holds the limits as
    float64 scalars: ``resdat -= vmin`` is exact in float64 and rounds to float32 once, ``resdat /= (vmax - vmin)`` divides in float64
    and rounds to float32 once."""
    if vmin == vmax:
        return np.zeros(d.shape, F32)
    with np.errstate(all="ignore"):
        return ((d - F32(vmin)).astype(np.float64) / (np.float64(vmax) - np.float64(vmin))).astype(F32)


def colorize(depth, lut):
    """:437-441 -> ([H,W,3] uint8, (vmin, vmax) float32)."""
    depth = np.asarray(depth, F32)
    with np.errstate(all="ignore"):
        d = F32(1.0) / depth
        vmin, vmax = F32(d.min()), percentile95(d)
        xn = normalize(d, vmin, vmax)
        xa = xn * F32(256.0)
        idx = np.zeros(d.shape, np.int64)
        hi = xa >= F32(256.0)
        ok = (xa > 0) & ~hi
        idx[ok] = xa[ok].astype(np.int64)
        idx[hi] = 255
        idx[~np.isfinite(d)] = 0
    assert xa.dtype == F32
    return np.asarray(lut, np.uint8)[idx], (vmin, vmax)


def block_reduce_max(img):
    """``skimage.measure.block_reduce(img, (2, 2, 1), np.max)`` of an [H,W,3] array."""
    H, W, C = img.shape
    pad = np.zeros((H + H % 2, W + W % 2, C), img.dtype)
    pad[:H, :W] = img
    return pad.reshape(pad.shape[0] // 2, 2, pad.shape[1] // 2, 2, C).max(axis=(1, 3))


def split_mask(gt, eval_split):
    """:358-368, through the package's own (host-only) window and bounds."""
    from fusiondepth_amd.evaluate_depth import split_bounds, split_window
    gt = np.asarray(gt, F32)
    H, W = gt.shape
    y0, y1, x0, x1 = split_window(eval_split, H, W)
    lo, hi = split_bounds(eval_split)
    mask = gt > F32(lo)
    if np.isfinite(hi):
        mask &= gt < F32(hi)
    crop = np.zeros(gt.shape, bool)
    crop[max(y0, 0):y1, max(x0, 0):x1] = True
    return mask & crop


def error_picture(depth, gt, mask, lut):
    """:408, :420-428 -> [ceil(H/2),ceil(W/2),3] uint8."""
    depth, gt = np.asarray(depth, F32), np.asarray(gt, F32)
    with np.errstate(all="ignore"):
        diff = np.abs(depth - gt)
        v = np.ones_like(diff) * F32(80) - np.clip(diff, 0, 2) * F32(40)
    assert v.dtype == F32
    v = np.where(mask, v, F32(0))                                 # outside the mask the value is never looked at
    colour = np.asarray(lut, np.uint8)[v.astype(np.uint8)]
    ones = np.zeros(colour.shape, np.uint8)
    ones[mask] = colour[mask]
    ones = block_reduce_max(ones)
    ones[(ones == 0).all(axis=2)] = 220
    return ones


def restate(depth, gt, eval_split, lut_disp, lut_err):
    """One image -> (colour picture, error picture, (vmin, vmax))."""
    color, stats = colorize(depth, lut_disp)
    return color, error_picture(depth, gt, split_mask(gt, eval_split), lut_err), stats


def depth_of(disp, size, scale=1.0, ratio=None):
    """The depth chain of ``fd_depth_export`` (tests/detection_ref.py)."""
    return DR.restate(disp, size, scale, ratio)[0]


def random_luts(seed=11):
    """Two random tables with no zero byte in ``lut_err`` - a selected pixel never looks unscored - and distinct channels."""
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (256, 3)).astype(np.uint8), rng.randint(1, 256, (256, 3)).astype(np.uint8)


def ground_truth(rng, depth, eval_split):
    """Ground truth near the prediction with 40 % holes; a few values at and past the split's bounds."""
    H, W = depth.shape
    gt = (depth * rng.uniform(0.5, 1.5, (H, W)).astype(F32) + rng.uniform(-1.5, 1.5, (H, W)).astype(F32)).astype(F32)
    gt = np.abs(gt) + F32(0.01)
    gt[rng.rand(H, W) < 0.4] = 0.0
    if H * W > 20:
        flat = gt.reshape(-1)
        flat[rng.choice(flat.size, 4, replace=False)] = [F32(80.0), F32(1e-3), F32(95.0), F32(79.5)]
    return gt
