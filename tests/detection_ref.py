"""numpy restatement of the dense part of the reference's ``export_detection.py`` (:322-325, 344-348, 388) for the tests of
``fd_depth_export`` / ``fd_depth_quantize_u16``, and the fixture inputs those tests share.  A helper, not a test.

The resize is ``oracle.evaluate.resize_bilinear``; every element-wise step is one float32 numpy operation, as in the reference:
``F32(1) / .``, ``* F32(scale)``, ``* ratio``, ``* F32(256)``.  In range the cast is ``astype(np.uint16)`` (truncation toward zero); out
of range numpy's cast is undefined and the rule of include/fdhip.h is applied instead: NaN and negative -> 0, ``>= 65535`` -> 65535."""
import numpy as np

from oracle import evaluate as OE

F32 = np.float32

# (H, W) of the maps one call exports from 6x20 disparities: a single pixel; widths that are no multiple of 8, so that the planes
# behind them start at odd element offsets; 5x64 (rows of whole 16-byte groups); 37x130 and 33x66 (more rows than a wave takes, several
# row classes); 12x257 (a width that is odd and leaves a one-pixel tail); 3x20 (down-sampling in y); 6x20 (the identity)
SIZES = [(1, 1), (2, 3), (7, 11), (5, 64), (37, 130), (12, 257), (33, 66), (3, 20), (6, 20)]
SRC = (6, 20)


def quantize(q):
    """The quantiser rule on a float32 / float64 array of ``depth * 256``."""
    q = np.asarray(q)
    out = np.zeros(q.shape, np.uint16)
    with np.errstate(invalid="ignore"):
        hi = q >= 65535
        ok = (q > 0) & ~hi
    out[hi] = 65535
    out[ok] = q[ok].astype(np.uint16)
    return out


def restate(disp, size, scale=1.0, ratio=None):
    """One map -> (float32 depth before the ``* 256``, the float32 product ``q``, the uint16 payload)."""
    with np.errstate(all="ignore"):
        p = F32(1) / OE.resize_bilinear(np.asarray(disp, F32), int(size[0]), int(size[1]))
        p = p * F32(scale)
        if ratio is not None:
            p = p * F32(ratio)
        q = p * F32(256)
    assert p.dtype == F32 and q.dtype == F32
    return p, q, quantize(q)


def fixture(seed=2024):
    """-> (disparities [9,6,20] float32 uniform in [0.02, 0.5], ground truth per map).  The ground truth is derived from the prediction
    - ``1.3 * pred * U(0.9, 1.1)`` with 40 % holes; ``1.3 * pred`` without noise or holes for maps of six pixels or fewer - so that the
    median-scaling ratios stay near 1.3 and the payload inside the uint16 range (independent ground truth gives ratios up to 8 and
    payloads past 65535, where equality would only test the saturation rule)."""
    rng = np.random.RandomState(seed)
    disps = rng.uniform(0.02, 0.5, (len(SIZES),) + SRC).astype(F32)
    gts = []
    for d, (H, W) in zip(disps, SIZES):
        pred = F32(1) / OE.resize_bilinear(d, H, W)
        if H * W <= 6:
            gt = (F32(1.3) * pred).astype(F32)
        else:
            gt = (F32(1.3) * pred * rng.uniform(0.9, 1.1, (H, W)).astype(F32)).astype(F32)
            gt[rng.rand(H, W) < 0.4] = 0.0
        gts.append(gt)
    return disps, gts


def special_plane():
    """A 6x20 disparity plane with the four out-of-range cases, and where they are: 0 (depth +inf), NaN, a negative value, 1e-4
    (10 000 m, payload 2 560 000).  Far enough apart that no output pixel of the identity resize mixes two of them."""
    rng = np.random.RandomState(7)
    d = rng.uniform(0.02, 0.5, SRC).astype(F32)
    where = {"zero": (1, 3), "nan": (3, 9), "negative": (4, 15), "far": (1, 17)}
    d[where["zero"]], d[where["nan"]], d[where["negative"]], d[where["far"]] = 0.0, np.nan, -0.25, 1e-4
    return d, where
