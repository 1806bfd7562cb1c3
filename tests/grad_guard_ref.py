"""The rules of the guarded optimiser step (include/fdhip.h: fd_grad_stats, fd_adam_step_guarded) restated in
numpy: ``x = grad * grad_scale`` formed in float32, squares and sums in float64, ``coef`` through one float32 rounding, the skip
decision and the counters.  No GPU, no torch."""
import numpy as np


def scaled(grad, grad_scale):
    """``x``: the float32 product the Adam kernel forms."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(grad, np.float32) * np.float32(grad_scale)).astype(np.float32)


def offsets_of(sizes):
    """Segment sizes -> the n_seg + 1 element offsets, 0 first."""
    return [0] + [int(v) for v in np.cumsum(np.asarray(sizes, np.int64))]


def grad_stats(grad, seg_offsets, grad_scale=1.0, max_norm=0.0, skip_nonfinite=True, counters=(0, -1, -1), adam_step=0):
    """-> (stats: float64 array [norm, count, coef, skip, segment norms ...], counters: [skipped, first, last]).  ``adam_step``: the
    Adam steps taken so far (``state[0]``); a skip is recorded as step ``adam_step + 1``, the step this call would have been."""
    x = scaled(grad, grad_scale).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = x * x
        sums = [float(np.sum(sq[a:b])) for a, b in zip(seg_offsets[:-1], seg_offsets[1:])]
        total = 0.0
        for s in sums:                                           # in segment order
            total += s
        norm = np.sqrt(total)
        count = int(np.count_nonzero(~np.isfinite(x)))
        skip = bool(skip_nonfinite) and count > 0
        coef = 1.0
        if max_norm > 0 and not skip:
            r = float(np.float32(max_norm)) / (norm + 1e-6)
            coef = float(np.float32(r if r < 1.0 else 1.0))      # a NaN ratio gives 1
    counters = [int(c) for c in counters]
    if skip:
        step = int(adam_step) + 1
        counters = [counters[0] + 1, step if counters[1] < 0 else counters[1], step]
    return np.array([norm, count, coef, 1.0 if skip else 0.0] + [np.sqrt(s) for s in sums], np.float64), counters


def clipped(grad, grad_scale, coef):
    """The gradient the guarded update uses: ``float32(float32(g * grad_scale) * coef)``."""
    return (scaled(grad, grad_scale) * np.float32(coef)).astype(np.float32)


def norm_bound(n):
    """Relative bound between two float64 sums of the same n non-negative terms taken in different orders (and their roots)."""
    return max(int(n), 1) * 2.0 ** -53
