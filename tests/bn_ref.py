"""Plain NumPy restatement of the BatchNorm entry points of csrc/norm.hip (fd_bn_*), in float64 as ground truth and in float32
two-pass arithmetic (``*_f32``) as the error baseline, plus the rounding floors and the input generator of tests/test_gpu_bn_edges.py.
No GPU, no project code.

Conventions: x [N, C, H, W]; the batch is ``groups`` consecutive sub-batches of N / groups samples, statistics are per (group, channel)
and laid out [groups * C]; the running statistics receive one momentum update per group, in group order, with the unbiased variance."""
import math

import numpy as np

U = 2.0 ** -24                     # unit roundoff of float32
MARGIN = 2.0 ** -14                # the generator's guarantee, as a fraction of |x a| + |b| + |r|
F32, F64 = np.float32, np.float64


def relu(v):
    """torch.relu: NaN stays NaN, everything not above zero becomes +0."""
    return np.where(v <= 0, np.zeros((), v.dtype), v)


def _grouped(t, groups):
    N = t.shape[0]
    assert N % groups == 0
    return t.reshape((groups, N // groups) + t.shape[1:])


def _bc(s):
    """[G, C] -> broadcastable against [G, Ng, C, H, W]."""
    return s[:, None, :, None, None]


def _vec(v, C, dt, default):
    return np.full((C,), default, dt) if v is None else np.asarray(v).astype(dt)


def _train_fwd(x, w, b, residual, groups, eps, momentum, relu_, running, dt):
    N, C, H, W = x.shape
    xg = _grouped(np.asarray(x).astype(dt), groups)
    M = (N // groups) * H * W
    w, b = _vec(w, C, dt, 1), _vec(b, C, dt, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = xg.sum(axis=(1, 3, 4), dtype=dt) / dt(M)                       # [G, C]
        dev = xg - _bc(mean)
        var = (dev * dev).sum(axis=(1, 3, 4), dtype=dt) / dt(M)
        invstd = dt(1) / np.sqrt(var + dt(eps))
        pre = dev * _bc(invstd) * w[None, None, :, None, None] + b[None, None, :, None, None]
        if residual is not None:
            pre = pre + _grouped(np.asarray(residual).astype(dt), groups)
        y = relu(pre) if relu_ else pre
        out = {"y": y.reshape(x.shape), "pre": pre.reshape(x.shape), "save_mean": mean.reshape(-1), "save_invstd": invstd.reshape(-1),
               "var": var.reshape(-1), "M": M}
        if running is not None:
            rm, rv = np.asarray(running[0]).astype(dt), np.asarray(running[1]).astype(dt)
            for g in range(groups):
                unbiased = var[g] * (dt(M) / dt(M - 1)) if M > 1 else var[g]
                rm = (dt(1) - dt(momentum)) * rm + dt(momentum) * mean[g]
                rv = (dt(1) - dt(momentum)) * rv + dt(momentum) * unbiased
            out["running_mean"], out["running_var"] = rm, rv
    return out


def train_fwd(x, w, b, residual, groups, eps, momentum, relu, running):
    """-> dict(y, save_mean, save_invstd, running_mean, running_var, var (biased), pre (before the ReLU), M), float64."""
    return _train_fwd(x, w, b, residual, groups, eps, momentum, relu, running, F64)


def train_fwd_f32(x, w, b, residual, groups, eps, momentum, relu, running):
    return _train_fwd(x, w, b, residual, groups, eps, momentum, relu, running, F32)


def _eval_fwd(x, w, b, residual, running_mean, running_var, eps, relu_, dt):
    C = x.shape[1]
    w, b = _vec(w, C, dt, 1), _vec(b, C, dt, 0)
    s = lambda v: np.asarray(v).astype(dt)[None, :, None, None]
    invstd = dt(1) / np.sqrt(s(running_var) + dt(eps))
    pre = (np.asarray(x).astype(dt) - s(running_mean)) * invstd * s(w) + s(b)
    if residual is not None:
        pre = pre + np.asarray(residual).astype(dt)
    return relu(pre) if relu_ else pre


def eval_fwd(x, w, b, residual, running_mean, running_var, eps, relu):
    return _eval_fwd(x, w, b, residual, running_mean, running_var, eps, relu, F64)


def eval_fwd_f32(x, w, b, residual, running_mean, running_var, eps, relu):
    return _eval_fwd(x, w, b, residual, running_mean, running_var, eps, relu, F32)


def _bwd_core(x, d, w, mean, invstd, groups, dt):
    """BatchNorm backward of the (already masked) gradient d; every intermediate the floors need is returned."""
    N, C, H, W = x.shape
    M = (N // groups) * H * W
    xg, dg = _grouped(np.asarray(x).astype(dt), groups), _grouped(d, groups)
    mean, invstd = np.asarray(mean).astype(dt).reshape(groups, C), np.asarray(invstd).astype(dt).reshape(groups, C)
    xh = (xg - _bc(mean)) * _bc(invstd)
    s1, s2 = dg.sum(axis=(1, 3, 4), dtype=dt), (dg * xh).sum(axis=(1, 3, 4), dtype=dt)
    k = w[None, :] * invstd
    m1, m2 = s1 / dt(M), s2 / dt(M)
    gx = _bc(k) * (dg - _bc(m1) - xh * _bc(m2))
    gw, gb = np.zeros((C,), dt), np.zeros((C,), dt)
    for g in range(groups):                                                   # in group order, as the kernels add them
        gw, gb = gw + s2[g], gb + s1[g]
    return {"gx": gx.reshape(x.shape), "gweight": gw, "gbias": gb, "d": d, "xhat": xh.reshape(x.shape), "k": k, "m1": m1, "m2": m2,
            "s1": s1, "s2": s2, "abs1": np.abs(dg).sum(axis=(1, 3, 4)), "abs2": np.abs(dg * xh).sum(axis=(1, 3, 4)), "M": M}


def _train_bwd(x, gy, w, b, mean, invstd, residual, relu_, groups, dt):
    C = x.shape[1]
    w, b = _vec(w, C, dt, 1), _vec(b, C, dt, 0)
    d = np.asarray(gy).astype(dt)
    if relu_:
        mg, ig = np.asarray(mean).astype(dt).reshape(groups, C), np.asarray(invstd).astype(dt).reshape(groups, C)
        pre = (_grouped(np.asarray(x).astype(dt), groups) - _bc(mg)) * _bc(ig) * w[None, None, :, None, None] + b[None, None, :, None, None]
        if residual is not None:
            pre = pre + _grouped(np.asarray(residual).astype(dt), groups)
        d = np.where(pre.reshape(x.shape) > 0, d, np.zeros((), dt))
    out = _bwd_core(x, d, w, mean, invstd, groups, dt)
    out["g_residual"] = d if residual is not None else None
    return out


def train_bwd(x, gy, w, b, mean, invstd, residual, relu, groups):
    """Backward of relu?(bn(x) + residual?) with the statistics (mean, invstd) of the forward.  ``residual`` is the forward's residual
    input (None = absent): the ReLU mask is the sign of the forward's pre-activation.  -> dict(gx, gweight, gbias, g_residual, ...)."""
    return _train_bwd(x, gy, w, b, mean, invstd, residual, relu, groups, F64)


def train_bwd_f32(x, gy, w, b, mean, invstd, residual, relu, groups):
    return _train_bwd(x, gy, w, b, mean, invstd, residual, relu, groups, F32)


# ---- the stem's tail: relu(bn(x)) -> features[0] -> MaxPool2d(3, stride 2, padding 1) ---------------------------------------------
def pool_out(n):
    return (n - 1) // 2 + 1


def _taps(f):
    """[9, N, C, Ho, Wo]: tap kh * 3 + kw of every window, -inf where the tap lies outside the plane."""
    N, C, H, W = f.shape
    Ho, Wo = pool_out(H), pool_out(W)
    p = np.full((N, C, 2 * Ho + 1, 2 * Wo + 1), -np.inf, f.dtype)
    p[:, :, 1:H + 1, 1:W + 1] = f
    return np.stack([p[:, :, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] for kh in range(3) for kw in range(3)])


def maxpool_fwd(f):
    """-> (pooled, argmax byte): the first maximum in raster order wins."""
    t = _taps(f)
    idx = np.argmax(t, axis=0)
    return np.take_along_axis(t, idx[None], 0)[0], idx.astype(np.uint8)


def maxpool_bwd(g_pooled, idx, H, W):
    N, C, Ho, Wo = g_pooled.shape
    p = np.zeros((N, C, 2 * Ho + 1, 2 * Wo + 1), g_pooled.dtype)
    for t in range(9):
        kh, kw = divmod(t, 3)
        p[:, :, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] += np.where(idx == t, g_pooled, np.zeros((), g_pooled.dtype))
    return p[:, :, 1:H + 1, 1:W + 1]


def _relu_maxpool_fwd(x, w, b, groups, eps, momentum, running, dt):
    out = _train_fwd(x, w, b, None, groups, eps, momentum, 1, running, dt)
    out["feat"] = out.pop("y")
    out["pooled"], out["idx"] = maxpool_fwd(out["feat"])
    return out


def relu_maxpool_fwd(x, w, b, groups, eps, momentum, running):
    return _relu_maxpool_fwd(x, w, b, groups, eps, momentum, running, F64)


def relu_maxpool_fwd_f32(x, w, b, groups, eps, momentum, running):
    return _relu_maxpool_fwd(x, w, b, groups, eps, momentum, running, F32)


def _relu_maxpool_bwd(x, g_pooled, idx, g_feat, w, b, mean, invstd, groups, dt):
    N, C, H, W = x.shape
    g = maxpool_bwd(np.asarray(g_pooled).astype(dt), idx, H, W)
    if g_feat is not None:
        g = g + np.asarray(g_feat).astype(dt)                                 # added before the mask
    return _train_bwd(x, g, w, b, mean, invstd, None, 1, groups, dt)


def relu_maxpool_bwd(x, g_pooled, idx, g_feat, w, b, mean, invstd, groups):
    return _relu_maxpool_bwd(x, g_pooled, idx, g_feat, w, b, mean, invstd, groups, F64)


def relu_maxpool_bwd_f32(x, g_pooled, idx, g_feat, w, b, mean, invstd, groups):
    return _relu_maxpool_bwd(x, g_pooled, idx, g_feat, w, b, mean, invstd, groups, F32)


def parts_from(x, S):
    """[N, C, S, 2] float32 = (sum, M2 about the slot's own mean) of the S slots of H * W / S consecutive pixels of every plane: what
    the convolution epilogue hands to fd_bn_train_fwd_parts.  Computed in float64, rounded once."""
    N, C, H, W = x.shape
    assert (H * W) % S == 0
    s = np.asarray(x).astype(F64).reshape(N, C, S, (H * W) // S)
    m = s.mean(-1, keepdims=True)
    return np.stack([s.sum(-1), ((s - m) ** 2).sum(-1)], -1).astype(F32)


# ---- rounding floors (see the docstring of tests/test_gpu_bn_edges.py) ---------------------------------------------------------
def lg(M):
    """Depth of a pairwise summation tree over M terms; one rounding at least."""
    return max(math.log2(M), 1.0)


def ab_of(ref, w, b, groups):
    """The apply pass's per-(group, channel) constants a = invstd * w, b' = b - mean * a, from the float64 statistics."""
    C = ref["save_mean"].size // groups
    w, b = _vec(w, C, F64, 1), _vec(b, C, F64, 0)
    a = ref["save_invstd"].reshape(groups, C) * w[None]
    return a, b[None] - ref["save_mean"].reshape(groups, C) * a


def floor_apply(x, a, bb, residual, groups):
    """y = fma(x, a, b') (+ r): 4 roundings' worth of the magnitudes that enter (a, b', the fma, the residual add)."""
    xg = _grouped(np.asarray(x).astype(F64), groups)
    f = np.abs(xg * _bc(a)) + np.abs(_bc(bb))
    if residual is not None:
        f = f + np.abs(_grouped(np.asarray(residual).astype(F64), groups))
    return (4 * U * f).reshape(x.shape)


def floor_sum(abs_terms_sum, M):
    """A sum of M float32 terms in a tree of depth log2(M)."""
    return U * lg(M) * abs_terms_sum


def floor_bwd(r, groups):
    """gx = k (d - m1 - xhat m2): 8 roundings of the terms, plus the summation error of the two means.  -> (gx, gweight, gbias)."""
    M = r["M"]
    k, m1, m2 = np.abs(r["k"]), np.abs(r["m1"]), np.abs(r["m2"])
    xh, d = np.abs(_grouped(r["xhat"], groups)), np.abs(_grouped(r["d"], groups))
    e1, e2 = floor_sum(r["abs1"], M) / M, floor_sum(r["abs2"], M) / M
    fx = 8 * U * _bc(k) * (d + _bc(m1) + xh * _bc(m2)) + _bc(k) * (_bc(e1) + xh * _bc(e2))
    # parameter gradients: the groups' sums, each with its summation floor, added in group order (one rounding per addition)
    fw = floor_sum(r["abs2"], M).sum(0) + U * np.abs(r["s2"]).sum(0)
    fb = floor_sum(r["abs1"], M).sum(0) + U * np.abs(r["s1"]).sum(0)
    return fx.reshape(r["gx"].shape), fw, fb


def shift_of(x, groups, path):
    """The shift of the kernels' single-pass sums, [G, C]: "small" (one-launch register kernels) the first element of the group's first
    plane, "large" (two-launch path, stem tail) the median of the nine samples ((2 j + 1) HW) / 18 of that plane."""
    N, C, H, W = x.shape
    xg = _grouped(np.asarray(x).astype(F64), groups)
    if path == "small":
        return xg[:, 0, :, 0, 0]
    HW = H * W
    return np.median(xg[:, 0].reshape(groups, C, HW)[:, :, [((2 * j + 1) * HW) // 18 for j in range(9)]], axis=-1)


def floor_stats(x, ref, groups, eps, momentum, running, path, S=None):
    """-> floors of save_mean, save_invstd, running_mean, running_var, from the documented form of the path that computes them.

    "small" / "large": mean = shift + m, m = sum(d) / M, var = sum(d^2) / M - m^2 with d = x - shift (bn_ref.shift_of).  The summation
    term u log2(M) sum|terms| / M over the terms d resp. d^2, one more rounding per term for forming d (three for d^2: d enters twice,
    and the square), the division and the final addition for the mean; for the variance also the error of m carried into m^2
    (2 |m| floor(m)), the roundings of m^2 and of the subtraction.  This is the documented loss u (mean - shift)^2 of the shifted form.
    The small path sums the deviations from the mean again when m^2 > 16 var; then (taken here at 16.01, so that a kernel which
    decides the other way within rounding of the threshold is held to the looser of the two) only the two-pass terms remain.
    "parts": the S float32 (sum, M2) partials per plane, E = N / groups * S of them merged by Chan's rule: mean = sum(sum_i) / M with
    one rounding per stored partial; var = sum(M2_i + cnt dm_i^2) / M with dm_i = sum_i / cnt - mean, whose rounding
    u (|sum_i / cnt| + |mean|) + floor(mean) enters as 2 cnt |dm_i| times itself.
    invstd = (var + eps)^-1/2 moves by invstd^3 / 2 per unit of variance, plus the square root's and the division's roundings; each
    momentum update adds the rounding of its two products and their sum."""
    N, C, H, W = x.shape
    M = ref["M"]
    xg = _grouped(np.asarray(x).astype(F64), groups)
    mean, var, inv = (ref[k].reshape(groups, C) for k in ("save_mean", "var", "save_invstd"))
    if path == "parts":
        cnt, E = (H * W) // S, (N // groups) * S
        sums = _grouped(np.asarray(x).astype(F64).reshape(N, C, S, cnt).sum(-1), groups)            # [G, Ng, C, S]
        f_mean = U * (lg(E) + 1) * np.abs(sums).sum(axis=(1, 3)) / M + U * np.abs(mean)
        dm = sums / cnt - mean[:, None, :, None]
        f_dm = U * (np.abs(sums / cnt) + np.abs(mean)[:, None, :, None]) + f_mean[:, None, :, None]
        f_var = U * (lg(E) + 2) * var + (2 * cnt * np.abs(dm) * f_dm).sum(axis=(1, 3)) / M
    else:
        shift = shift_of(x, groups, path)
        d, m = xg - _bc(shift), mean - shift
        f_m = U * (lg(M) + 1) * np.abs(d).sum(axis=(1, 3, 4)) / M + U * np.abs(m)
        f_mean = f_m + U * np.abs(mean)
        single = U * (lg(M) + 3) * (var + m * m) + 2 * np.abs(m) * f_m + U * (m * m + var)
        two = U * (lg(M) + 3) * var + U * var
        f_var = np.where((m * m > 16.01 * var) & (path == "small"), two, single)
    f_inv = 0.5 * inv ** 3 * f_var + 2 * U * inv
    out = {"save_mean": f_mean.reshape(-1), "save_invstd": f_inv.reshape(-1), "var": f_var.reshape(-1)}
    if running is not None:
        rm, rv = np.asarray(running[0]).astype(F64), np.asarray(running[1]).astype(F64)
        frm, frv = np.zeros(C), np.zeros(C)
        ub = M / (M - 1.0) if M > 1 else 1.0
        for g in range(groups):
            frm = (1 - momentum) * frm + momentum * f_mean[g] + 3 * U * (np.abs((1 - momentum) * rm) + np.abs(momentum * mean[g]))
            frv = (1 - momentum) * frv + momentum * ub * (f_var[g] + U * var[g]) + 3 * U * (np.abs((1 - momentum) * rv) + momentum * ub * var[g])
            rm = (1 - momentum) * rm + momentum * mean[g]
            rv = (1 - momentum) * rv + momentum * ub * var[g]
        out["running_mean"], out["running_var"] = frm, frv
    return out


def path_of(shape, aligned=True, parts=None, stem=False):
    """Which statistics path csrc/norm.hip takes (bn_small / bn_vec_ok): NT * SMALL_K = 1024 float4 per (group, channel), 16 groups."""
    N, C, H, W, G = shape
    if parts is not None:
        return "parts"
    small = not stem and aligned and (H * W) % 4 == 0 and G <= 16 and (N // G) * ((H * W) // 4) <= 1024
    return "small" if small else "large"


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
EPS, MOMENTUM = 1e-5, 0.1


def params(C, seed):
    """Weight and bias with both signs, running statistics away from their defaults."""
    rng = np.random.RandomState(7919 * seed + C)
    w = (rng.uniform(0.5, 1.5, C) * np.where(np.arange(C) % 2 == 0, 1.0, -1.0)).astype(F32)
    b = (rng.uniform(0.2, 0.8, C) * np.where(np.arange(C) % 3 == 0, -1.0, 1.0)).astype(F32)
    rm = rng.uniform(-0.5, 0.5, C).astype(F32)
    rv = rng.uniform(0.5, 2.0, C).astype(F32)
    return w, b, rm, rv


def _margin_miss(x, w, b, residual, groups):
    """Elements whose float64 pre-activation lies closer to 0 than MARGIN (|x a| + |b'| + |r|), and a per (group, channel)."""
    ref = train_fwd(x, w, b, residual, groups, EPS, MOMENTUM, 0, None)
    a, bb = ab_of(ref, w, b, groups)
    scale = floor_apply(x, a, bb, residual, groups) / (4 * U)
    return np.abs(ref["pre"]) < MARGIN * scale, np.broadcast_to(_bc(a), _grouped(x, groups).shape).reshape(x.shape), scale


def min_margin(x, w, b, residual, groups):
    """Smallest |pre-activation| / (|x a| + |b'| + |r|) over the tensor (the generator guarantees >= MARGIN)."""
    ref = train_fwd(x, w, b, residual, groups, EPS, MOMENTUM, 0, None)
    a, bb = ab_of(ref, w, b, groups)
    return float((np.abs(ref["pre"]) / (floor_apply(x, a, bb, residual, groups) / (4 * U))).min())


def _tap_gap(x, w, b, groups):
    """Per pooling window: gap between the best and the second-best tap of relu(bn(x)), the scale |x a| + |b'| of the best tap, the
    best tap's index, and whether the two best are both exactly 0."""
    ref = train_fwd(x, w, b, None, groups, EPS, MOMENTUM, 1, None)
    a, bb = ab_of(ref, w, b, groups)
    t = _taps(ref["y"])
    ts = _taps(floor_apply(x, a, bb, None, groups) / (4 * U))
    order = np.argsort(-t, axis=0, kind="stable")
    best, second = np.take_along_axis(t, order[:1], 0)[0], np.take_along_axis(t, order[1:2], 0)[0]
    scale = np.take_along_axis(ts, order[:1], 0)[0]
    both_zero = (best == 0) & (second == 0)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(second), best - second, np.inf)            # a window with one valid tap has no second-best
    return gap, scale, order[0], both_zero


def min_tap_gap(x, w, b, groups):
    gap, scale, _, both_zero = _tap_gap(x, w, b, groups)
    return float(np.where(both_zero, np.inf, gap / scale).min())


def make_case(shape, seed, stem=False):
    """(N, C, H, W, groups), seed -> dict of float32 x, gy, residual, w, b, running statistics (and, for the stem, g_pooled, g_feat).

    x = 2 randn + a per-channel offset.  Then every element whose float64 pre-activation, with or without the residual, lies within
    MARGIN (|x a| + |b'| + |r|) of zero is moved away from it (x += 8 MARGIN scale / a, towards the side it is on), and for the stem
    every best tap that leads the second-best by less than MARGIN of its scale is raised likewise, until nothing is left to move:
    the kernels' masks and argmax bytes are then decided by margins 2^10 times their rounding error.  At most 1 % of x is moved."""
    N, C, H, W, groups = shape
    rng = np.random.RandomState(seed)
    w, b, rm, rv = params(C, seed)
    x = (2 * rng.randn(N, C, H, W) + rng.uniform(-1.5, 1.5, (1, C, 1, 1))).astype(F32)
    gy = rng.randn(N, C, H, W).astype(F32)
    residual = rng.randn(N, C, H, W).astype(F32)
    moved = np.zeros(x.shape, bool)
    for _ in range(20):
        clean = True
        for r in ((None,) if stem else (None, residual)):
            miss, a, scale = _margin_miss(x, w, b, r, groups)
            if miss.any():
                clean = False
                ref = train_fwd(x, w, b, r, groups, EPS, MOMENTUM, 0, None)
                step = 8 * MARGIN * scale / np.abs(a) * np.sign(a) * np.where(ref["pre"] >= 0, 1.0, -1.0)
                x = np.where(miss, (x + step).astype(F32), x)
                moved |= miss
        if stem:
            gap, scale, best, both_zero = _tap_gap(x, w, b, groups)
            tie = (gap < MARGIN * scale) & ~both_zero
            if tie.any():
                clean = False
                ref = train_fwd(x, w, b, None, groups, EPS, MOMENTUM, 0, None)
                a, _ = ab_of(ref, w, b, groups)
                a = np.broadcast_to(_bc(a), _grouped(x, groups).shape).reshape(x.shape)
                n, c, ho, wo = np.nonzero(tie)
                kh, kw = np.divmod(best[n, c, ho, wo], 3)
                h, ww = 2 * ho - 1 + kh, 2 * wo - 1 + kw
                x = x.copy()
                x[n, c, h, ww] = (x[n, c, h, ww] + 8 * MARGIN * scale[n, c, ho, wo] / a[n, c, h, ww]).astype(F32)
                moved[n, c, h, ww] = True
        if clean:
            break
    else:
        raise AssertionError("make_case%r: margins not reached in 20 rounds" % (shape,))
    assert moved.sum() <= max(1, 0.01 * x.size), "make_case%r moved %d of %d elements" % (shape, moved.sum(), x.size)
    case = {"shape": shape, "x": x, "gy": gy, "residual": residual, "w": w, "b": b, "rm": rm, "rv": rv, "moved": int(moved.sum())}
    if stem:
        case["g_pooled"] = rng.randn(N, C, pool_out(H), pool_out(W)).astype(F32)
        case["g_feat"] = rng.randn(N, C, H, W).astype(F32)
    return case


# the shapes of tests/test_gpu_bn_edges.py (N, C, H, W, groups); constants read from csrc/norm.hip: NT = 256 threads, SMALL_K = 4 float4
# slots per thread (small path: N/groups * HW/4 <= 1024 float4), slices of >= 1024 floats, at most 2048 / (C groups) and 64 of them,
# at most 64 workgroups per plane of 1024 floats each, at most 16 groups on the small and the parts path
SMALL = [(1, 3, 2, 2, 1), (1, 2, 1, 1024, 1), (1, 2, 1, 1028, 1), (2, 2, 4, 256, 1), (1, 2, 1, 2052, 1), (3, 2, 16, 64, 1),
         (1, 2, 1, 3076, 1), (4, 3, 16, 64, 1)]
PAST_SMALL = [(4, 3, 16, 68, 1)]
GROUPS = [(4, 5, 4, 8, 2), (16, 3, 2, 2, 16), (17, 3, 2, 2, 17)]
SCALAR = [(2, 3, 5, 7, 1), (1, 2, 33, 50, 1)]
OFFSET = (2, 3, 4, 8, 1)
RAGGED = [(2, 4, 33, 100, 1)]
CAPS = [(1, 1, 260, 256, 1)]
ONE_SPLIT = [(2, 1030, 6, 8, 2)]   # C groups > 2048; register kernels when aligned (test_channel_cap_of_the_slices_... reaches the two-launch path)
TRAIN_SHAPES = SMALL + PAST_SMALL + GROUPS + SCALAR + [OFFSET] + RAGGED + CAPS + ONE_SPLIT
PARTS = [((2, 3, 12, 20, 1), (1, 2, 15, 60)), ((4, 2, 12, 20, 2), (1, 2, 15, 60)), ((2, 3, 3, 5, 1), (1, 3, 5, 15))]
STEM = [(2, 3, 1, 4, 1), (1, 2, 7, 9, 1), (2, 2, 6, 8, 2), (1, 2, 5, 4, 1), (1, 1, 9, 12, 1), (1, 2, 6, 8, 1)]
STEM_BIG = (1, 1, 513, 1024, 1)
