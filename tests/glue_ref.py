"""float64 references, seeded inputs and the case lists for the memory-bound glue kernels of csrc/geometry.hip and csrc/pool.hip
(disparity -> depth, pose matrices, projection matrices, back-projection, projection, Cat_xy, max-pool, the decoder's input assembly,
nearest x2, activation backward, axpby, input normalisation, spatial mean, depth metrics, Adam) and for the stand-alone loss-map kernels
(bilinear resize and its adjoint, SSIM, the reprojection loss map, the edge-aware smoothness loss, the combination of the loss terms).

Every reference is dtype-generic: called with ``torch.float64`` it is the ground truth, called with ``torch.float32`` it is the CPU
oracle whose own distance from the ground truth is the *yardstick* of a comparison (``bound``).  ``oracle.layers`` is used wherever it
is dtype-generic; max-pool, concatenation, means and all gradients are plain torch; Adam is restated.
tests/test_glue_ref_cpu.py checks all of this without a GPU; tests/test_gpu_glue_edges.py holds the kernels to it.
Test helper: not imported by the package.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import layers as OL

F32, F64 = torch.float32, torch.float64
TINY = 1e-30
MIN_DEPTH, MAX_DEPTH = 0.1, 100.0

# ---------------------------------------------------------------------------------------------- the cases (smallest shapes per edge)
D2D_N = (1, 255, 256, 257, 524288 + 257)                       # ew_grid: 2048 blocks of 256, then the grid-stride loop
POSE_B = (1, 64, 65)                                           # one thread per item, blocks of 64
POSE_NORMS = (0.0, 1e-7, 1e-6, 3e-4, 1e-3, 1e-2, 0.3, 3.1)
POSE_HEAD = (11, 2, 3, 2)                                      # G, nf, Bq, predictions: 66 threads
PROJMAT_B = (1, 5, 6)                                          # B * 12 and B * 16 cross 64 between 5 and 6
PROJMAT_STRIDES = (12, 20)
BACKPROJECT_SHAPES = ((1, 1, 1), (3, 3, 5), (2, 16, 16), (1, 33, 31), (1, 513, 1025))
PROJECT_SHAPES = ((3, 2, 2), (3, 3, 5), (3, 16, 16), (3, 32, 32), (3, 33, 31), (3, 25, 41), (1, 513, 1025))
MAXPOOL_SHAPES = ((1, 1, 1, 7), (1, 1, 7, 1), (2, 3, 2, 2), (1, 2, 3, 4), (1, 2, 4, 3), (1, 2, 257, 259), (33, 1000, 2, 2))
MAXPOOL_KINDS = ("randn", "negative", "neginf", "nan", "const")
UPCAT_HW = ((6, 8), (3, 2), (5, 7), (129, 128))                # vector, vector, scalar, a plane above 16384 float4s
UPCAT_COMBOS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1))      # skip, skip_add, extra
ACT_NAMES = ("none", "relu", "elu", "sigmoid", "tanh")         # ids 0..4
UP2_CASES = ((2, 3, 1, 1), (2, 3, 5, 7), (1, 1, 129, 128), (33, 1000, 1, 1))
EW_N = (1, 255, 256, 257, 1048576 + 257)                       # ew_blocks: 4096 blocks of 256
MEAN_PLANE_SIZES = (1, 6, 63, 64, 65, 120, 4097)
MEAN_PLANES = (1, 36)
DEPTH_ERR_N = (1, 7, 256, 65536 + 13, 375 * 1242 // 3)         # 256 partial sums of 256 threads = 65536
ADAM_N = (1, 257, 1048576 + 257)
ADAM_BETAS, ADAM_EPS, ADAM_LR = (0.9, 0.999), 1e-8, 1.5e-4
# bilinear resize (BC, Hin, Win, Hout, Wout), forward and adjoint; the adjoint runs one thread per input pixel in blocks of 256
BILINEAR_CASES = (
    (1, 1, 1, 1, 1), (1, 1, 1, 3, 5),                              # a single input pixel: every output is its copy
    (2, 1, 7, 4, 7),                                               # one axis only
    (3, 5, 7, 5, 7),                                               # identity
    (6, 3, 5, 6, 10), (2, 6, 20, 24, 80), (2, 3, 10, 24, 80),      # integer ratios 2, 4 and 8: the pyramid
    (2, 2, 3, 24, 36),                                             # ratio 12: interior windows wider than MAXW = 24 (scalar branch), border windows unrolled
    (1, 6, 6, 7, 7),                                               # fractional ratios; the smallest shape at which the ceiling-ratio window lost a row
    (2, 8, 12, 9, 13), (2, 5, 7, 8, 11), (1, 16, 20, 24, 31), (1, 7, 9, 9, 16),
    (1, 4, 6, 8, 7),                                               # integer in y, fractional in x
    (1, 192, 640, 375, 1242),                                      # the evaluation size, one plane
    (1, 15, 17, 30, 34), (1, 16, 16, 32, 32), (1, 1, 257, 2, 514),  # input planes of 255, 256 and 257 pixels
    (1, 257, 1025, 514, 2050),                                     # forward: 1053700 outputs, past ew_grid's 2048 blocks of 256
    (1, 513, 1025, 513, 1025),                                     # adjoint: 525825 inputs, past ew_grid's 2048 blocks of 256
)
BILINEAR_OFFSET_CASE = (2, 5, 7, 8, 11)                            # operands one float off 16-byte alignment
BILINEAR_DENSE_MAX = 4096                                          # input pixels up to which the CPU test builds the dense matrix
# SSIM and the reprojection map: tiles of 64 x 16 with a halo of 1 (2 in the backward); the reflect fold acts on rows / columns 1 and n - 2
SSIM_HW = ((4, 4),                                                 # the minimum: every pixel next to a fold
           (4, 64), (16, 64),                                      # one tile wide; exactly one tile
           (15, 63),                                               # one short of a tile both ways
           (17, 65), (18, 66),                                     # the folded row / column on either side of the tile seam
           (33, 129),                                              # three tiles each way, the last one pixel deep
           (5, 130))                                               # the fold in the third tile's second column
SSIM_PLANES = (1, 7)
SSIM_UNIFORM_CASE = (7, 33, 129)                                   # independent uniform images: the variance cancellation at its worst
SSIM_EQUAL_CASE = (1, 18, 66)                                      # x == y on the 8 x 8 block in the bottom right corner, across both tile seams
REPROJ_B = (1, 3)
REPROJ_GAP = 5                                                     # floats between the images of `out`
# smoothness (B, H, W): 1024 pixels per block; k_image_mean takes float4 loads, four in flight (4096 float4s a round), when P % 4 == 0
SMOOTH_SHAPES = ((2, 2),                                           # the minimum
                 (3, 341), (2, 512), (5, 205),                     # 1023, 1024 and 1025 pixels (1025: scalar mean)
                 (96, 128), (4, 3073),                             # n4 = 3072: the last unrolled round is not entered; 3073: it is
                 (128, 128), (4, 4097))                            # n4 = 4096: one full round, no tail; 4097: a tail of one
SMOOTH_B = (1, 3)
SMOOTH_OFFSET_CASE = (1, 128, 128)                                 # off alignment: the scalar mean
SMOOTH_EXTRA = ((2, 330, 400, False), (2, 330, 400, True),         # 2 x 129 = 258 partial sums for the 256 threads of k_smooth_fin
                (1, 513, 513, True))                               # 1029 blocks of 256 wanted by k_sub_per_image, 1024 launched
SMOOTH_COT = 1.7
COMBINE_N = (1, 2, 3, 4)
COMBINE_SI = ("all", "none", "scale0")
COMBINE_WEIGHT, COMBINE_COT = 1e-3, 1.3


# ---------------------------------------------------------------------------------------------- error measure
def rel_err(got, ref):
    """max|got - ref| / max(max|ref|, tiny): the error at the scale of the tensor."""
    got = torch.as_tensor(got).detach().cpu().to(F64)
    ref = torch.as_tensor(ref).detach().cpu().to(F64)
    assert got.shape == ref.shape, "shape %s vs %s" % (tuple(got.shape), tuple(ref.shape))
    if ref.numel() == 0:
        return 0.0
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), TINY)


def bound(yardstick, cap=None):
    """max(4 x yardstick, 1e-6), never above ``cap`` (what an existing test of the same quantity allows, as a fraction of scale)."""
    b = max(4.0 * yardstick, 1e-6)
    return b if cap is None else min(b, cap)


def same_values(a, b):
    """Exact equality that also wants NaN where NaN is (torch.equal says NaN != NaN)."""
    a, b = torch.as_tensor(a).detach().cpu(), torch.as_tensor(b).detach().cpu()
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _rng(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 12345) % (2 ** 31 - 1)
    return np.random.RandomState(seed)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _grad(outs, cots, leaves):
    """d sum_i <outs[i], cots[i]> / d leaves, zeros for a leaf no output depends on."""
    pairs = [(o, c) for o, c in zip(outs, cots) if c is not None]
    if not pairs:
        return [torch.zeros_like(l) for l in leaves]
    gs = torch.autograd.grad([o for o, _ in pairs], leaves, [c.to(o.dtype) for o, c in pairs], allow_unused=True)
    return [torch.zeros_like(l) if g is None else g for g, l in zip(gs, leaves)]


# ---------------------------------------------------------------------------------------------- disp_to_depth
def d2d_inputs(n):
    rng = _rng(1, n)
    return {"disp": _t(rng.uniform(0.01, 0.99, n)), "g_scaled": _t(rng.randn(n)), "g_depth": _t(rng.randn(n))}


def d2d_ref(inp, dtype, use_gs=True, use_gd=True):
    disp = inp["disp"].to(dtype).clone().requires_grad_(True)
    scaled, depth = OL.disp_to_depth(disp, MIN_DEPTH, MAX_DEPTH)
    (g,) = _grad([scaled, depth], [inp["g_scaled"] if use_gs else None, inp["g_depth"] if use_gd else None], [disp])
    return {"scaled": scaled.detach(), "depth": depth.detach(), "d_disp": g}


# ---------------------------------------------------------------------------------------------- pose vector -> 4x4
def pose_inputs(B):
    """Rotation norms POSE_NORMS spread over the batch (item b has norm number b mod 8; a single item has 3e-4, where 1 - cos loses most in float32), random axes, translations of KITTI size."""
    rng = _rng(2, B)
    axis = rng.randn(B, 3)
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    norms = np.array([POSE_NORMS[(b + (3 if B == 1 else 0)) % len(POSE_NORMS)] for b in range(B)])
    return {"aa": _t(axis * norms[:, None]).view(B, 1, 3), "tr": _t(0.1 * rng.randn(B, 1, 3)), "cot": _t(rng.randn(B, 4, 4))}


def pose_ref(inp, dtype, invert):
    aa, tr = (inp[k].to(dtype).clone().requires_grad_(True) for k in ("aa", "tr"))
    T = OL.transformation_from_parameters(aa, tr, invert=invert)
    g_aa, g_tr = _grad([T], [inp["cot"]], [aa, tr])
    return {"T": T.detach(), "g_aa": g_aa, "g_tr": g_tr}


def pose_head_inputs():
    G, nf, Bq, npred = POSE_HEAD
    rng = _rng(3, G, nf, Bq)
    return {"pose": _t(0.05 * rng.randn(G * nf * Bq, 6 * npred)), "cots": [_t(rng.randn(G * Bq, 4, 4)) for _ in range(nf)],
            "inverts": [k % 2 == 0 for k in range(nf)]}


def pose_head_ref(inp, dtype):
    """trainer.py:338-360: rows ordered (micro-batch, frame pair, sample); prediction 0 (columns 0..5) makes the matrix."""
    G, nf, Bq, npred = POSE_HEAD
    pose = inp["pose"].to(dtype).clone().requires_grad_(True)
    Ts = []
    for k in range(nf):
        rows = torch.cat([pose[(g * nf + k) * Bq:(g * nf + k + 1) * Bq] for g in range(G)], 0)
        Ts.append(OL.transformation_from_parameters(rows[:, None, 0:3], rows[:, None, 3:6], invert=inp["inverts"][k]))
    (g,) = _grad(Ts, inp["cots"], [pose])
    out = {"T%d" % k: T.detach() for k, T in enumerate(Ts)}
    out["g_pose"] = g
    return out


# ---------------------------------------------------------------------------------------------- cameras
K_NORM = np.array([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)


def cameras(B, H, W, seed):
    """A different K / inv_K / T per batch item: KITTI's normalised intrinsics with focal lengths and principal point moved by a few
    percent, rotations <= 0.05 rad, translations <= 0.3."""
    rng = _rng(4, B, H, W, seed)
    Ks, iKs = [], []
    for b in range(B):
        K = K_NORM.copy()
        K[0, 0] *= 1 + 0.05 * b
        K[1, 1] *= 1 - 0.04 * b
        K[0, 2] += 0.02 * b
        K[1, 2] -= 0.03 * b
        K[0, :] *= W
        K[1, :] *= H
        Ks.append(K)
        iKs.append(np.linalg.pinv(K))
    axis = rng.randn(B, 3)
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    aa = torch.from_numpy(axis * rng.uniform(0.01, 0.05, (B, 1))).view(B, 1, 3)
    tr = torch.from_numpy(rng.uniform(-0.3, 0.3, (B, 1, 3)) / math.sqrt(3.0))
    T = OL.transformation_from_parameters(aa, tr, invert=False)
    return _t(np.stack(Ks)), _t(np.stack(iKs)), T.to(F32)


@functools.lru_cache(maxsize=None)
def backproject_inputs(B, H, W):
    rng = _rng(5, B, H, W)
    _, inv_K, _ = cameras(B, H, W, 0)
    return {"depth": _t(rng.uniform(1.0, 21.0, (B, 1, H, W))), "inv_K": inv_K, "cot": _t(rng.randn(B, 4, H * W)),
            "B": B, "H": H, "W": W}


def backproject_ref(inp, dtype):
    depth = inp["depth"].to(dtype).clone().requires_grad_(True)
    inv_K = inp["inv_K"].to(dtype)
    pts = OL.backproject_depth(depth, inv_K)
    (g,) = _grad([pts], [inp["cot"]], [depth])
    return {"points": pts.detach(), "g_depth": g, "cat_xy": OL.cat_xy(depth.detach(), inv_K)}


@functools.lru_cache(maxsize=None)
def project_inputs(B, H, W):
    """Points = the float32 oracle's back-projection of depths in [1, 21] (the kernel's real input), per-item K and T."""
    rng = _rng(6, B, H, W)
    K, inv_K, T = cameras(B, H, W, 1)
    depth = _t(rng.uniform(1.0, 21.0, (B, 1, H, W)))
    return {"points": OL.backproject_depth(depth, inv_K), "K": K, "T": T, "cot": _t(rng.randn(B, H, W, 2)), "B": B, "H": H, "W": W}


def project_cam_z(inp, eps=1e-7):
    """cam_z + eps of the float64 reference: the denominator whose smallness would make any comparison meaningless."""
    P = torch.matmul(inp["K"].to(F64), inp["T"].to(F64))[:, :3, :]
    return torch.matmul(P, inp["points"].to(F64))[:, 2, :] + eps


def project_ref(inp, dtype, eps=1e-7):
    pts, T = (inp[k].to(dtype).clone().requires_grad_(True) for k in ("points", "T"))
    grid = OL.project_3d(pts, inp["K"].to(dtype), T, inp["H"], inp["W"], eps)
    g_pts, gT = _grad([grid], [inp["cot"]], [pts, T])
    return {"grid": grid.detach(), "g_points": g_pts, "gT": gT}


def projmat_inputs(B):
    rng = _rng(7, B)
    K, _, T = cameras(B, 192, 640, 2)
    return {"K": K, "T": T, "gP": _t(rng.randn(B, 3, 4))}


def projmat_ref(inp, dtype):
    """P = (K @ T)[:3] (layers.py:217) and its adjoint in T."""
    K, T = inp["K"].to(dtype), inp["T"].to(dtype).clone().requires_grad_(True)
    P = torch.matmul(K, T)[:, :3, :]
    (gT,) = _grad([P], [inp["gP"]], [T])
    return {"P": P.detach(), "gT": gT}


# ---------------------------------------------------------------------------------------------- max-pool 3x3 / 2 / 1
@functools.lru_cache(maxsize=None)
def maxpool_inputs(N, C, H, W, kind):
    """``randn``; ``negative``: every value < 0 (a padded tap competing as 0 would win); ``neginf``: -inf in most of plane 0, so that
    whole windows are -inf; ``nan``: scattered NaN in plane 0; ``const``: the last plane is one negative constant (every tap ties)."""
    rng = _rng(8, N, C, H, W, MAXPOOL_KINDS.index(kind))
    x = rng.randn(N * C, H, W).astype(np.float32)
    if kind == "negative":
        x = -np.abs(x) - 0.1
    elif kind == "neginf":
        x[0][rng.rand(H, W) < 0.7] = -np.inf
        x[0][:2, :2] = -np.inf                                      # window (0, 0) sees nothing else
    elif kind == "nan":
        x[0][rng.rand(H, W) < 0.15] = np.nan
        x[0].flat[-1] = np.nan
    elif kind == "const":
        x[-1] = -1.5
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return {"x": _t(x).view(N, C, H, W), "cot": _t(rng.randn(N, C, Ho, Wo))}


def maxpool_ref(inp, dtype):
    x = inp["x"].to(dtype).clone().requires_grad_(True)
    y = F.max_pool2d(x, 3, 2, 1)
    (gx,) = torch.autograd.grad(y, x, inp["cot"].to(dtype))
    return {"y": y.detach(), "gx": gx}


def maxpool_unintended_ties(x):
    """Number of windows whose maximum is attained more than once by values that are NOT exact repeats of an intended kind
    (-inf, or a constant plane): 0 means torch's routing (first maximum in raster order) is the only sensible answer."""
    x = x.to(F64)
    N, C, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1), value=float("-inf"))
    win = xp.unfold(2, 3, 2).unfold(3, 3, 2).reshape(N, C, -1, 9)      # [N, C, Ho*Wo, 9]
    mx = torch.nan_to_num(win, nan=float("inf")).max(-1, keepdim=True).values
    ties = (win == mx).sum(-1) > 1
    const_plane = (x.reshape(N, C, -1).min(-1).values == x.reshape(N, C, -1).max(-1).values)[..., None]
    intended = (mx[..., 0] == float("-inf")) | (const_plane & (H * W > 1))
    return int((ties & ~intended).sum())


# ---------------------------------------------------------------------------------------------- decoder input assembly
def act_output_values(rng, shape, act):
    """Values an activation can OUTPUT (the kernels differentiate through the output): ReLU >= 0 with exact zeros, ELU > -1,
    sigmoid in (0, 1), tanh in (-1, 1)."""
    v = rng.randn(*shape)
    if act == "relu":
        v = np.maximum(v, 0)
    elif act == "elu":
        v = np.where(v > 0, v, np.expm1(v))
    elif act == "sigmoid":
        v = 1 / (1 + np.exp(-v))
    elif act == "tanh":
        v = np.tanh(v)
    return _t(v)


def act_deriv_from_output(v, act):
    """act'(pre-activation) written through the activation's output ``v`` (fd_act_bwd's convention)."""
    if act == "relu":
        return (v > 0).to(v.dtype)
    if act == "elu":
        return torch.where(v > 0, torch.ones_like(v), v + 1)
    if act == "sigmoid":
        return v * (1 - v)
    if act == "tanh":
        return 1 - v * v
    return torch.ones_like(v)


@functools.lru_cache(maxsize=None)
def upcat_inputs(h, w, act="none"):
    N, Ca, Cs, C3 = (1, 1, 1, 1) if h * w > 4096 else (2, 3, 2, 2)
    rng = _rng(9, h, w, ACT_NAMES.index(act))
    mk = lambda *s: _t(rng.randn(*s))
    return {"a": act_output_values(rng, (N, Ca, h, w), act), "skip": mk(N, Cs, 2 * h, 2 * w), "skip_add": mk(N, Cs, 2 * h, 2 * w),
            "extra": mk(N, C3, 2 * h, 2 * w), "cot": mk(N, Ca + Cs + C3, 2 * h, 2 * w), "dims": (N, Ca, Cs, C3)}


def upcat_ref(inp, dtype, combo, act="none"):
    """cat([up2(a), skip (+ skip_add), extra], 1) and its gradients; with ``act`` the gradient of ``a`` is taken w.r.t. the
    pre-activation whose output ``a`` is."""
    use_skip, use_add, use_extra = combo
    N, Ca, Cs, C3 = inp["dims"]
    a, s1, s2, s3 = (inp[k].to(dtype).clone().requires_grad_(True) for k in ("a", "skip", "skip_add", "extra"))
    parts = [OL.upsample(a)]
    if use_skip:
        parts.append(s1 + s2 if use_add else s1)
    if use_extra:
        parts.append(s3)
    y = torch.cat(parts, 1)
    cot = torch.cat([inp["cot"][:, :Ca]] + ([inp["cot"][:, Ca:Ca + Cs]] if use_skip else []) + ([inp["cot"][:, Ca + Cs:]] if use_extra else []), 1)
    ga, g1, g2, g3 = _grad([y], [cot], [a, s1, s2, s3])
    out = {"y": y.detach(), "cot": cot, "g_a": ga * act_deriv_from_output(a.detach(), act)}
    if use_skip:
        out["g_skip"] = g1
    if use_add:
        out["g_skip_add"] = g2
    if use_extra:
        out["g_extra"] = g3
    return out


def up2_inputs(N, C, h, w):
    rng = _rng(10, N, C, h, w)
    return {"x": _t(rng.randn(N, C, h, w)), "cot": _t(rng.randn(N, C, 2 * h, 2 * w))}


def up2_ref(inp, dtype):
    x = inp["x"].to(dtype).clone().requires_grad_(True)
    y = OL.upsample(x)
    (gx,) = _grad([y], [inp["cot"]], [x])
    return {"y": y.detach(), "gx": gx}


# ---------------------------------------------------------------------------------------------- element-wise
@functools.lru_cache(maxsize=None)
def ew_inputs(n):
    rng = _rng(11, n)
    return {"a": _t(rng.randn(n)), "b": _t(rng.randn(n)), "img": _t(rng.rand(n))}


def act_bwd_ref(y, gy, act, dtype):
    y, gy = y.to(dtype), gy.to(dtype)
    return gy * act_deriv_from_output(y, act)


def axpby_ref(a, b, alpha, beta, dtype):
    """alpha and beta reach the kernel as float32."""
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    return alpha * a.to(dtype) + beta * b.to(dtype)


def input_normalize_f32(x):
    """resnet_encoder.py:94 in float32 on the CPU, a true division: what the kernels must reproduce bit for bit."""
    return (x.to(F32).cpu() - 0.45) / 0.225


def mean_inputs(planes, plane_size):
    rng = _rng(12, planes, plane_size)
    N = 4 if planes % 4 == 0 else 1
    return {"x": _t(rng.randn(N, planes // N, 1, plane_size) + 0.5), "cot": _t(rng.randn(N, planes // N)), "scale": 0.01}


def mean_ref(inp, dtype):
    x = inp["x"].to(dtype).clone().requires_grad_(True)
    m = float(np.float32(inp["scale"])) * x.mean(3).mean(2)
    (gx,) = _grad([m], [inp["cot"]], [x])
    return {"mean": m.detach(), "gx": gx}


# ---------------------------------------------------------------------------------------------- depth metrics
DEPTH_THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)


@functools.lru_cache(maxsize=None)
def depth_err_inputs(n):
    """gt, pred in [0.5, 80] with max(gt / pred, pred / gt) spread over (1.02, 2.72); a sample whose ratio comes within 1e-3 of a
    threshold is given pred = gt instead, so that float32 rounding cannot move any of the three counts."""
    rng = _rng(13, n)
    gt = rng.uniform(1.4, 29.0, n).astype(np.float32)
    pred = (gt * np.exp(rng.choice([-1.0, 1.0], n) * rng.uniform(0.02, 1.0, n))).astype(np.float32)
    ratio = np.maximum(gt.astype(np.float64) / pred, pred.astype(np.float64) / gt)
    near = np.zeros(n, bool)
    for t in DEPTH_THRESHOLDS:
        near |= np.abs(ratio - t) < 1e-3
    pred[near] = gt[near]
    return {"gt": _t(gt), "pred": _t(pred)}


def depth_err_margin(inp):
    gt, pred = inp["gt"].to(F64), inp["pred"].to(F64)
    ratio = torch.max(gt / pred, pred / gt)
    return min(float((ratio - t).abs().min()) for t in DEPTH_THRESHOLDS)


def depth_err_ref(inp, dtype):
    """-> (the four continuous metrics [abs_rel, sq_rel, rmse, rmse_log], the three counts as integers)."""
    gt, pred = inp["gt"].to(dtype), inp["pred"].to(dtype)
    e = OL.compute_depth_errors(gt, pred)
    ratio = torch.max(gt / pred, pred / gt)
    counts = [int((ratio < t).sum()) for t in DEPTH_THRESHOLDS]
    return torch.stack([v.to(dtype) for v in e[:4]]), counts


# ---------------------------------------------------------------------------------------------- Adam
def adam_scenarios(n):
    """name -> dict(step0, m0, v0, grads, lrs (one per step, as the device state holds them), grad_scale).  p starts at 0, so p itself
    is the accumulated update."""
    rng = _rng(14, n)
    grads = [_t(rng.randn(n)) for _ in range(5)]
    zero = torch.zeros(n)
    lr32 = lambda v: float(np.float32(v))
    base = dict(step0=0, m0=zero, v0=zero, grads=grads, lrs=[lr32(ADAM_LR)] * 5, grad_scale=1.0)
    out = {"five steps from zero": base,
           "lr drops after step 3": dict(base, lrs=[lr32(ADAM_LR)] * 3 + [lr32(ADAM_LR * 0.1)] * 2),
           "grad_scale 0.5": dict(base, grad_scale=0.5),
           "resumed at step 100000": dict(base, step0=100000, m0=_t(0.3 * rng.randn(n)), v0=_t(rng.uniform(0.05, 2.0, n)), grads=grads[:2],
                                          lrs=[lr32(ADAM_LR)] * 2)}
    return out


def adam_ref(sc, dtype=F64):
    """torch.optim.Adam (betas (0.9, 0.999), eps 1e-8, no weight decay) restated: bias corrections from Python doubles, the gradient
    pre-multiplied by grad_scale.  -> p, exp_avg, exp_avg_sq after the scenario's steps, from p = 0."""
    b1, b2 = ADAM_BETAS
    m, v = sc["m0"].to(dtype).clone(), sc["v0"].to(dtype).clone()
    p = torch.zeros_like(m)
    for i, (g, lr) in enumerate(zip(sc["grads"], sc["lrs"])):
        t = sc["step0"] + i + 1
        g = g.to(dtype) * sc["grad_scale"]
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        p = p - (lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + ADAM_EPS))
    return {"p": p, "exp_avg": m, "exp_avg_sq": v}


def adam_torch(sc, dtype, shapes=None):
    """The same scenario through torch.optim.Adam itself, on one tensor or on tensors of ``shapes`` (flattened and concatenated on return)."""
    n = sc["m0"].numel()
    shapes = shapes or [(n,)]
    sizes = [int(np.prod(s)) for s in shapes]
    params = [torch.nn.Parameter(torch.zeros(s, dtype=dtype)) for s in shapes]
    opt = torch.optim.Adam(params, lr=sc["lrs"][0], betas=ADAM_BETAS, eps=ADAM_EPS)
    if sc["step0"]:
        for p, m0, v0 in zip(params, sc["m0"].split(sizes), sc["v0"].split(sizes)):
            opt.state[p] = {"step": torch.tensor(float(sc["step0"])), "exp_avg": m0.to(dtype).view(p.shape).clone(),
                            "exp_avg_sq": v0.to(dtype).view(p.shape).clone()}
    for g, lr in zip(sc["grads"], sc["lrs"]):
        opt.param_groups[0]["lr"] = lr
        for p, gp in zip(params, g.split(sizes)):
            p.grad = (gp.to(dtype) * sc["grad_scale"]).view(p.shape)
        opt.step()
    cat = lambda key: torch.cat([opt.state[p][key].reshape(-1) for p in params])
    return {"p": torch.cat([p.detach().reshape(-1) for p in params]), "exp_avg": cat("exp_avg"), "exp_avg_sq": cat("exp_avg_sq")}, opt


# ---------------------------------------------------------------------------------------------- bilinear resize and its adjoint
def smooth_images(rng, *shape):
    """Uniform noise box-filtered twice (3 x 3, edge-replicated) over the last two axes: values in (0, 1), neighbours ~0.03 apart."""
    a = rng.rand(*shape)
    for _ in range(2):
        p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(1, 1), (1, 1)], mode="edge")
        a = sum(p[..., dy:dy + shape[-2], dx:dx + shape[-1]] for dy in range(3) for dx in range(3)) / 9.0
    return a


@functools.lru_cache(maxsize=None)
def bilinear_inputs(BC, Hin, Win, Hout, Wout):
    """x: a smooth image, as the disparity and depth maps are that the project resizes; cot: white noise.  ATen's float32 rule, which the
    kernel follows, rounds the source coordinate to float32: at 640 -> 1242 columns that moves a weight by up to ~1e-4, and on a
    white-noise x (neighbours up to 1 apart) the float32 CPU oracle itself is then 4.8e-5 of scale from float64, above the 1.1e-5 that
    the forward comparison may allow.  On the smooth x the same coordinate error costs ~30 times less, while a wrong tap or a swapped
    weight still costs ~0.03 / 0.5 of scale.  The adjoint sees the white-noise cotangent at every shape."""
    rng = _rng(15, BC, Hin, Win, Hout, Wout)
    return {"x": _t(smooth_images(rng, 1, BC, Hin, Win)), "cot": _t(rng.randn(1, BC, Hout, Wout)), "size": (Hout, Wout)}


def bilinear_ref(inp, dtype):
    x = inp["x"].to(dtype).clone().requires_grad_(True)
    y = F.interpolate(x, inp["size"], mode="bilinear", align_corners=False)
    (gx,) = _grad([y], [inp["cot"]], [x])
    return {"y": y.detach(), "gx": gx}


def bilinear_matrix(Hin, Win, Hout, Wout):
    """The forward reference as a dense float64 matrix [Hout * Wout, Hin * Win], one unit image per column."""
    eye = torch.eye(Hin * Win, dtype=F64).view(Hin * Win, 1, Hin, Win)
    return F.interpolate(eye, (Hout, Wout), mode="bilinear", align_corners=False).reshape(Hin * Win, Hout * Wout).t()


# ---------------------------------------------------------------------------------------------- SSIM, reprojection loss map
SSIM_KINDS = ("smooth", "uniform", "equal")


@functools.lru_cache(maxsize=None)
def ssim_inputs(planes, H, W, kind="smooth"):
    """``smooth``: a smooth image and the same plus noise of 0.05, clipped to [0, 1] (tests/test_gpu_losspath.py::test_ssim_fwd_bwd);
    ``uniform``: two independent uniform images; ``equal``: smooth, with y == x on the 8 x 8 block in the bottom right corner."""
    rng = _rng(16, planes, H, W, SSIM_KINDS.index(kind))
    if kind == "uniform":
        x, y = rng.rand(1, planes, H, W), rng.rand(1, planes, H, W)
    else:
        x = smooth_images(rng, 1, planes, H, W)
        y = np.clip(x + 0.05 * rng.randn(1, planes, H, W), 0, 1)
    x, y = _t(x), _t(y)
    if kind == "equal":
        y[..., H - 8:, W - 8:] = x[..., H - 8:, W - 8:]
    return {"x": x, "y": y, "cot": _t(rng.rand(1, planes, H, W))}


def ssim_preclamp(x, y):
    """(1 - SSIM) / 2 before the clamp to [0, 1] (oracle.layers.ssim without its last step): where this leaves [0, 1] the gradient is cut."""
    xp, yp = F.pad(x, (1, 1, 1, 1), mode="reflect"), F.pad(y, (1, 1, 1, 1), mode="reflect")
    mu_x, mu_y = F.avg_pool2d(xp, 3, 1), F.avg_pool2d(yp, 3, 1)
    sig_x = F.avg_pool2d(xp ** 2, 3, 1) - mu_x ** 2
    sig_y = F.avg_pool2d(yp ** 2, 3, 1) - mu_y ** 2
    sig_xy = F.avg_pool2d(xp * yp, 3, 1) - mu_x * mu_y
    num = (2 * mu_x * mu_y + OL.SSIM_C1) * (2 * sig_xy + OL.SSIM_C2)
    den = (mu_x ** 2 + mu_y ** 2 + OL.SSIM_C1) * (sig_x + sig_y + OL.SSIM_C2)
    return (1 - num / den) / 2


def ssim_window_difference(inp):
    """min over the 3 x 3 windows (reflect-padded) of max |x - y| inside the window: > 0 means no window sees two equal images."""
    d = F.pad((inp["x"].to(F64) - inp["y"].to(F64)).abs(), (1, 1, 1, 1), mode="reflect")
    return float(F.max_pool2d(d, 3, 1).min())


def ssim_ref(inp, dtype, use_gx=True, use_gy=True):
    """oracle.layers.ssim (dtype-generic) and the gradients of <ssim, cot>; a gradient nobody asks for is left out."""
    x, y = (inp[k].to(dtype).clone().requires_grad_(True) for k in ("x", "y"))
    s = OL.ssim(x, y)
    gx, gy = _grad([s], [inp["cot"]], [x, y])
    out = {"ssim": s.detach()}
    if use_gx:
        out["gx"] = gx
    if use_gy:
        out["gy"] = gy
    return out


@functools.lru_cache(maxsize=None)
def reproj_inputs(B, H, W):
    rng = _rng(17, B, H, W)
    pred = smooth_images(rng, B, 3, H, W)
    return {"pred": _t(pred), "target": _t(np.clip(pred + 0.05 * rng.randn(B, 3, H, W), 0, 1))}


def reproj_ref(inp, dtype, use_ssim):
    """trainer.py:476-488: 0.85 * ssim.mean(1, True) + 0.15 * |target - pred|.mean(1, True), or the L1 term alone."""
    pred, target = inp["pred"].to(dtype), inp["target"].to(dtype)
    l1 = (target - pred).abs().mean(1, True)
    return {"map": 0.85 * OL.ssim(pred, target).mean(1, True) + 0.15 * l1 if use_ssim else l1}


# ---------------------------------------------------------------------------------------------- edge-aware smoothness
def smooth_step(n):
    """The spacing 2^-e of n distinct disparities in (0.01, 1): the largest power of two with 0.01 + (n + 1) steps < 1."""
    return 2.0 ** -math.ceil(math.log2(n / 0.98))


@functools.lru_cache(maxsize=None)
def smooth_inputs(B, H, W):
    """Disparities: a random permutation of B * H * W consecutive multiples of smooth_step, the first one just above 0.01 - all of them
    exact in float32, no two equal, so that |d_p - d_q| has no kink and sgn(d_p - d_q) no choice at any edge, in any precision, with or
    without the division by the image's mean.  Image: uniform noise, so that every edge has its own weight exp(-|dI|)."""
    n = B * H * W
    step = smooth_step(n)
    k0 = int(0.01 / step) + 1
    assert k0 + n < 2 ** 24 and (k0 + n) * step < 1.0
    rng = _rng(18, B, H, W)
    disp = (k0 + rng.permutation(n)).astype(np.float64) * step
    return {"disp": _t(disp.reshape(B, 1, H, W)), "img": _t(rng.rand(B, 3, H, W)), "step": step}


def smooth_min_neighbour_difference(inp):
    d = inp["disp"].to(F64)
    return min(float((d[..., :, 1:] - d[..., :, :-1]).abs().min()), float((d[..., 1:, :] - d[..., :-1, :]).abs().min()))


def smooth_ref(inp, dtype, normalize):
    """oracle.layers.get_smooth_loss on d, or on d / (d.mean(2, True).mean(3, True) + 1e-7) (trainer.py:569-571), and SMOOTH_COT times its
    gradient in d."""
    d = inp["disp"].to(dtype).clone().requires_grad_(True)
    n = d / (d.mean(2, True).mean(3, True) + 1e-7) if normalize else d
    loss = OL.get_smooth_loss(n, inp["img"].to(dtype))
    (g,) = _grad([loss], [torch.tensor(SMOOTH_COT)], [d])
    return {"loss": loss.detach(), "g_disp": g}


# ---------------------------------------------------------------------------------------------- combination of the loss terms
def combine_inputs(n, si_mode):
    """n scales of (photometric, smoothness, SI) scalars of the sizes the trainer sees; SI at every scale, at none or at scale 0 only."""
    rng = _rng(19, n, COMBINE_SI.index(si_mode))
    has_si = [si_mode == "all" or (si_mode == "scale0" and s == 0) for s in range(n)]
    draw = lambda lo, hi: _t(rng.uniform(lo, hi, 1)).reshape(())
    return {"photo": [draw(0.05, 0.2) for _ in range(n)], "smooth": [draw(1.0, 60.0) for _ in range(n)],
            "si": [draw(0.01, 0.3) if h else None for h in has_si], "w": COMBINE_WEIGHT, "cot": COMBINE_COT}


def combine_ref(inp, dtype):
    """trainer.py:569-596 in the operation order of k_combine_losses, which is the reference's: loss_s = photo_s + w * smooth_s / 2^s,
    total += loss_s, total += si_s where there is one, total / n.  The weight and the cotangent reach the kernels as float32.
    -> loss [n], total, and the gradients of cot * total in photo_s, smooth_s, si_s (the last for every scale, as the kernel writes it)."""
    n = len(inp["photo"])
    w, cot = float(np.float32(inp["w"])), float(np.float32(inp["cot"]))
    total, losses = torch.zeros((), dtype=dtype), []
    for s in range(n):
        loss = inp["photo"][s].to(dtype) + w * inp["smooth"][s].to(dtype) / (2 ** s)
        total = total + loss
        losses.append(loss)
        if inp["si"][s] is not None:
            total = total + inp["si"][s].to(dtype)
    gt = torch.tensor(cot, dtype=dtype) / n
    return {"loss": torch.stack(losses), "total": total / n, "g_photo": torch.stack([gt] * n),
            "g_smooth": torch.stack([gt * w / (2 ** s) for s in range(n)]), "g_si": torch.stack([gt] * n)}
