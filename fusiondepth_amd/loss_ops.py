"""The loss path over the libfdhip C ABI: geometry (disparity -> depth, poses, back-projection, projection), SSIM, the smoothness
term, the per-scale and the all-scales fused photometric / LiDAR losses and their combination.  One ``torch.autograd.Function`` per
C-ABI forward / backward pair; nothing here touches the convolution stack."""
import ctypes

import torch

from . import _lib
from ._lib import _empty, _need_cuda, call, f32, ptr, query, stream

PROJECT_EPS = 1e-7


# ------------------------------------------------------------------------------------ geometry ---
class _DispToDepth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, min_depth, max_depth):
        disp = f32(disp)
        _need_cuda(disp)
        scaled, depth = torch.empty_like(disp), torch.empty_like(disp)
        call("fd_disp_to_depth_fwd", ptr(disp), ptr(scaled), ptr(depth), disp.numel(), float(min_depth),
             float(max_depth), stream())
        ctx.save_for_backward(disp)
        ctx.rng = (float(min_depth), float(max_depth))
        return scaled, depth

    @staticmethod
    def backward(ctx, g_scaled, g_depth):
        (disp,) = ctx.saved_tensors
        gs = f32(g_scaled) if g_scaled is not None else None
        gd = f32(g_depth) if g_depth is not None else None
        out = torch.empty_like(disp)
        call("fd_disp_to_depth_bwd", ptr(disp), ptr(gs), ptr(gd), ptr(out), disp.numel(), ctx.rng[0], ctx.rng[1],
             stream())
        return out, None, None


def disp_to_depth(disp, min_depth, max_depth):
    return _DispToDepth.apply(disp, min_depth, max_depth)


class _PoseMatrix(torch.autograd.Function):
    @staticmethod
    def forward(ctx, axisangle, translation, invert):
        B = axisangle.shape[0]
        aa = f32(axisangle).reshape(B, 3)
        tr = f32(translation).reshape(B, 3)
        _need_cuda(aa, tr)
        T = _empty((B, 4, 4), aa)
        call("fd_pose_matrix_fwd", ptr(aa), ptr(tr), ptr(T), B, int(bool(invert)), stream())
        ctx.save_for_backward(aa, tr)
        ctx.invert = int(bool(invert))
        ctx.shapes = (axisangle.shape, translation.shape)
        return T

    @staticmethod
    def backward(ctx, gT):
        aa, tr = ctx.saved_tensors
        B = aa.shape[0]
        gT = f32(gT)
        gaa, gtr = torch.empty_like(aa), torch.empty_like(tr)
        call("fd_pose_matrix_bwd", ptr(aa), ptr(tr), ptr(gT), ptr(gaa), ptr(gtr), B, ctx.invert, stream())
        return gaa.reshape(ctx.shapes[0]), gtr.reshape(ctx.shapes[1]), None


def transformation_from_parameters(axisangle, translation, invert=False):
    """layers.py:23-40.  axisangle / translation: [B,1,3] -> [B,4,4]."""
    return _PoseMatrix.apply(axisangle, translation, invert)


class _PoseHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pose, G, nf, Bq, invert_mask):
        import ctypes
        pose = f32(pose)
        _need_cuda(pose)
        N, ld = pose.shape
        if N != G * nf * Bq or ld % 6 != 0 or not 1 <= nf <= 4:
            raise ValueError("pose_head: pose must be [G * nf * Bq, 6 * predictions] with 1..4 frame pairs, got %s for G=%d nf=%d Bq=%d"
                             % (tuple(pose.shape), G, nf, Bq))
        Ts = [_empty((G * Bq, 4, 4), pose) for _ in range(nf)]
        aas = [_empty((G * Bq, ld // 6, 1, 3), pose) for _ in range(nf)]
        trs = [_empty((G * Bq, ld // 6, 1, 3), pose) for _ in range(nf)]
        arr = ctypes.c_void_p * nf
        call("fd_pose_head_fwd", ptr(pose), arr(*[ptr(t) for t in Ts]), arr(*[ptr(t) for t in aas]), arr(*[ptr(t) for t in trs]),
             G, nf, Bq, ld, int(invert_mask), stream())
        ctx.save_for_backward(pose)
        ctx.cfg = (G, nf, Bq, ld, int(invert_mask))
        ctx.mark_non_differentiable(*aas, *trs)
        return tuple(Ts) + tuple(aas) + tuple(trs)

    @staticmethod
    def backward(ctx, *grads):
        import ctypes
        (pose,) = ctx.saved_tensors
        G, nf, Bq, ld, invert_mask = ctx.cfg
        gTs = [None if g is None else f32(g) for g in grads[:nf]]
        g_pose = torch.empty_like(pose)
        call("fd_pose_head_bwd", ptr(pose), (ctypes.c_void_p * nf)(*[ptr(g) for g in gTs]), ptr(g_pose), G, nf, Bq, ld, invert_mask,
             stream())
        return g_pose, None, None, None, None


def pose_head(pose, groups, n_pairs, batch, inverts):
    """trainer.py:338-360 for the stacked pose network in ONE launch each way (fd_pose_head_fwd / _bwd): ``pose`` [groups * n_pairs *
    batch, 6 * predictions] = the pose decoder's output with rows ordered (micro-batch, frame pair, sample) -> per frame pair
    (cam_T_cam [groups * batch, 4, 4], axisangle, translation [groups * batch, predictions, 1, 3]).  ``inverts[k]``: trainer.py:352
    ``invert=(f_i < 0)``.  The axisangle / translation entries are what the reference's outputs dictionary holds; here they carry
    no gradient (the reference's only differentiable use of them is the matrix, except for --pose_model_type posecnn, which does not
    take this path)."""
    mask = 0
    for k, inv in enumerate(inverts):
        mask |= (1 << k) if inv else 0
    out = _PoseHead.apply(pose, int(groups), int(n_pairs), int(batch), mask)
    nf = int(n_pairs)
    return [(out[k], out[nf + k], out[2 * nf + k]) for k in range(nf)]


class _Backproject(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, inv_K):
        depth, inv_K = f32(depth), f32(inv_K)
        _need_cuda(depth, inv_K)
        B, _, H, W = depth.shape
        pts = _empty((B, 4, H * W), depth)
        call("fd_backproject_fwd", ptr(depth), ptr(inv_K), ptr(pts), B, H, W, stream())
        ctx.save_for_backward(inv_K)
        ctx.shape = depth.shape
        return pts

    @staticmethod
    def backward(ctx, g):
        (inv_K,) = ctx.saved_tensors
        B, _, H, W = ctx.shape
        out = _empty(ctx.shape, g)
        call("fd_backproject_bwd", ptr(f32(g)), ptr(inv_K), ptr(out), B, H, W, stream())
        return out, None


def backproject_depth(depth, inv_K):
    return _Backproject.apply(depth, inv_K)


class _Project3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, K, T, H, W, eps):
        points, K, T = f32(points), f32(K), f32(T)
        _need_cuda(points, K, T)
        B = points.shape[0]
        grid = _empty((B, H, W, 2), points)
        call("fd_project3d_fwd", ptr(points), ptr(K), ptr(T), ptr(grid), B, H, W, float(eps), stream())
        ctx.save_for_backward(points, K, T)
        ctx.dims = (B, H, W, float(eps))
        return grid

    @staticmethod
    def backward(ctx, g):
        points, K, T = ctx.saved_tensors
        B, H, W, eps = ctx.dims
        g = f32(g)
        gpts = torch.empty_like(points)
        gT = _empty((B, 4, 4), points)
        ws = _empty((query("fd_project3d_bwd_ws_floats", B, H, W),), points)
        call("fd_project3d_bwd", ptr(points), ptr(K), ptr(T), ptr(g), ptr(gpts), ptr(gT), ptr(ws), B, H, W, eps,
             stream())
        return gpts, None, gT, None, None, None


def project_3d(points, K, T, height, width, eps=PROJECT_EPS):
    return _Project3D.apply(points, K, T, height, width, eps)


def cat_xy(depth, inv_K):
    depth, inv_K = f32(depth.detach()), f32(inv_K)
    _need_cuda(depth, inv_K)
    B, _, H, W = depth.shape
    out = _empty((B, 3, H, W), depth)
    call("fd_cat_xy_fwd", ptr(depth), ptr(inv_K), ptr(out), B, H, W, stream())
    return out


class _BilinearUp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Hout, Wout):
        x = f32(x)
        _need_cuda(x)
        B, C, Hin, Win = x.shape
        y = _empty((B, C, Hout, Wout), x)
        call("fd_bilinear_up_fwd", ptr(x), ptr(y), B * C, Hin, Win, Hout, Wout, stream())
        ctx.dims = (B, C, Hin, Win, Hout, Wout)
        return y

    @staticmethod
    def backward(ctx, g):
        B, C, Hin, Win, Hout, Wout = ctx.dims
        gx = _empty((B, C, Hin, Win), g)
        call("fd_bilinear_up_bwd", ptr(f32(g)), ptr(gx), B * C, Hin, Win, Hout, Wout, stream())
        return gx, None, None


def bilinear_upsample(x, size):
    """F.interpolate(x, size, mode='bilinear', align_corners=False) of [B, C, Hin, Win], B * C < 65536.  The forward takes any size;
    the gradient exists for size[0] >= Hin and size[1] >= Win only (any ratio, integer or fractional, per axis) and a backward
    pass through a smaller size raises."""
    return _BilinearUp.apply(x, int(size[0]), int(size[1]))


# ------------------------------------------------------------------------------------ SSIM etc. ---
class _SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        x, y = f32(x), f32(y)
        _need_cuda(x, y)
        B, C, H, W = x.shape
        out = torch.empty_like(x)
        call("fd_ssim_fwd", ptr(x), ptr(y), ptr(out), B, C, H, W, stream())
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        B, C, H, W = x.shape
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        call("fd_ssim_bwd", ptr(x), ptr(y), ptr(f32(g)), ptr(gx), ptr(gy), B, C, H, W, stream())
        return gx, gy


def ssim(x, y):
    return _SSIM.apply(x, y)


def reprojection_loss_map(pred, target, use_ssim=True, out=None):
    """trainer.py:476-488 without autograd (used for the identity losses): [B,3,H,W]^2 -> [B,1,H,W]."""
    pred, target = f32(pred.detach()), f32(target.detach())
    _need_cuda(pred, target)
    B, C, H, W = pred.shape
    assert C == 3
    if out is None:
        out = _empty((B, 1, H, W), pred)
        stride = H * W
    else:
        stride = out.stride(0)
    call("fd_reproj_loss_map", ptr(pred), ptr(target), out.data_ptr(), stride, B, H, W, int(bool(use_ssim)), stream())
    return out


class _SmoothLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, img, normalize):
        disp, img = f32(disp), f32(img)
        _need_cuda(disp, img)
        B, _, H, W = disp.shape
        out = _empty((1,), disp)
        ws = _empty((query("fd_smooth_ws_floats", B, H, W),), disp)
        call("fd_smooth_fwd", ptr(disp), ptr(img), ptr(out), ptr(ws), B, H, W, int(normalize), stream())
        ctx.save_for_backward(disp, img)
        ctx.normalize = int(normalize)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        disp, img = ctx.saved_tensors
        B, _, H, W = disp.shape
        g = f32(g).reshape(1)
        d = torch.empty_like(disp)
        ws = _empty((query("fd_smooth_ws_floats", B, H, W),), disp)
        call("fd_smooth_bwd", ptr(disp), ptr(img), ptr(g), ptr(d), ptr(ws), B, H, W, ctx.normalize, stream())
        return d, None, None


def get_smooth_loss(disp, img):
    """layers.py:235-248."""
    return _SmoothLoss.apply(disp, img, False)


def normalized_smooth_loss(disp, img):
    """trainer.py:569-571: get_smooth_loss(disp / (disp.mean(2,3) + 1e-7), img)."""
    return _SmoothLoss.apply(disp, img, True)


class _CombineLosses(torch.autograd.Function):
    """trainer.py:569-596 on device scalars: (loss_0..loss_{n-1}, total) = f(photo_s, smooth_s, si_s)."""

    @staticmethod
    def forward(ctx, weight, n, *terms):
        photo, smooth, si = terms[:n], terms[n:2 * n], terms[2 * n:]
        P = ctypes.c_void_p * n
        arr = [P(*[ptr(f32(t).reshape(1)) if t is not None else None for t in group]) for group in (photo, smooth, si)]
        out = _empty((n + 1,), photo[0])
        call("fd_combine_losses_fwd", ctypes.addressof(arr[0]), ctypes.addressof(arr[1]), ctypes.addressof(arr[2]), n,
             float(weight), ptr(out), stream())
        ctx.n, ctx.weight = n, float(weight)
        ctx.has = [t is not None for t in terms]
        return tuple(out[i] for i in range(n + 1))

    @staticmethod
    def backward(ctx, *gs):
        n = ctx.n
        g_total = gs[n]
        grads = _empty((3 * n,), g_total)
        call("fd_combine_losses_bwd", ptr(f32(g_total).reshape(1)), n, ctx.weight, ptr(grads), stream())
        return (None, None) + tuple(grads[i] if ctx.has[i] else None for i in range(3 * n))


def combine_losses(photo, smooth, si, smooth_weight):
    """-> ([loss_s], total) for lists of 0-dim device tensors (``si`` entries may be None).  Only ``total`` carries a
    gradient (the per-scale values are logging outputs, as in the reference)."""
    n = len(photo)
    out = _CombineLosses.apply(float(smooth_weight), n, *(list(photo) + list(smooth) + list(si)))
    return [o.detach() for o in out[:n]], out[n]


# ------------------------------------------------------------------------------------ fused loss --
class PhotoOptions:
    """The option subset the fused loss reads (options.py:64-71,111-125,242-330)."""

    def __init__(self, min_depth=0.1, max_depth=100.0, no_ssim=False, avg_reprojection=False, si_threshold=2.0,
                 si_var=0.3, si_depth_scale=26.0, si_beam_scale=100.0, si_lo=1.0, si_mode=0):
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)
        self.no_ssim, self.avg_reprojection = bool(no_ssim), bool(avg_reprojection)
        self.si_threshold, self.si_var = float(si_threshold), float(si_var)
        self.si_depth_scale, self.si_beam_scale = float(si_depth_scale), float(si_beam_scale)
        self.si_lo = float(si_lo)
        self.si_mode = int(si_mode)       # 0 SI-log, 1 masked L1 (completor.py:718-723)


def _photo_cfg(po, B, H, W, Hs, Ws, NF, groups=1):
    c = _lib.PhotoCfg()
    c.groups = groups
    c.min_depth, c.max_depth = po.min_depth, po.max_depth
    c.B, c.H, c.W, c.Hs, c.Ws, c.NF = B, H, W, Hs, Ws, NF
    c.use_ssim = 0 if po.no_ssim else 1
    c.avg_reprojection = 1 if po.avg_reprojection else 0
    c.si_depth_scale, c.si_beam_scale = po.si_depth_scale, po.si_beam_scale
    c.si_threshold, c.si_var, c.eps = po.si_threshold, po.si_var, PROJECT_EPS
    c.si_lo = getattr(po, "si_lo", 1.0)
    c.si_mode = getattr(po, "si_mode", 0)
    return c


class _PhotoLoss(torch.autograd.Function):
    """One pyramid scale of generate_images_pred + the photometric / SI part of compute_losses (one to three source frames,
    optional predictive mask).

    Returns (to_optimise.mean(), si_loss, sel, depth, sample, color); the last four are
    non-differentiable by-products (``None`` unless requested)."""

    @staticmethod
    def forward(ctx, disp, T0, T1, T2, mask, K, inv_K, src0, src1, src2, target, ident, noise, beam, po, materialize, groups):
        disp, K, inv_K, target = f32(disp), f32(K), f32(inv_K), f32(target)
        _need_cuda(disp, K, inv_K, target, src0)
        srcs = [f32(t) for t in (src0, src1, src2) if t is not None]
        Ts = [f32(t) for t in (T0, T1, T2) if t is not None]
        NF = len(srcs)
        assert len(Ts) == NF
        B, _, Hs, Ws = disp.shape
        H, W = target.shape[2:]
        P = _empty((B, NF, 3, 4), disp)
        for f in range(NF):
            call("fd_proj_matrix_fwd", ptr(K), ptr(Ts[f]), P.data_ptr() + f * 48, NF * 12, B, stream())
        ident = f32(ident) if ident is not None else None
        noise = f32(noise) if noise is not None else None
        beam = f32(beam) if beam is not None else None
        mask = f32(mask) if mask is not None else None
        cfg = _photo_cfg(po, B, H, W, Hs, Ws, NF, groups)
        sel = _empty((B, H, W), disp, torch.uint8)
        depth = _empty((B, 1, H, W), disp) if materialize else None
        sample = _empty((NF, B, H, W, 2), disp) if materialize else None
        color = _empty((NF, B, 3, H, W), disp) if materialize else None
        reproj = _empty((B, NF, H, W), disp) if mask is not None else None
        ws = _empty((query("fd_photo_ws_floats", B, H, W),), disp)
        out = _empty((96,), disp)
        src_arr = (ctypes.c_void_p * 3)(*[ptr(srcs[min(f, NF - 1)]) for f in range(3)])
        call("fd_photo_fwd_ex", ctypes.addressof(cfg), ptr(disp), ptr(inv_K), ptr(P), ctypes.addressof(src_arr),
             ptr(target), ptr(ident), ptr(noise), ptr(beam), ptr(mask), ptr(sel), ptr(depth), ptr(sample), ptr(color),
             ptr(reproj), ptr(ws), ptr(out), stream())
        ctx.save_for_backward(disp, K, inv_K, P, target, beam, sel, out, mask, reproj, *srcs)
        ctx.cfg, ctx.NF, ctx.has_ident = cfg, NF, int(ident is not None)
        ctx.mark_non_differentiable(sel)
        extras = [t for t in (depth, sample, color) if t is not None]
        if extras:
            ctx.mark_non_differentiable(*extras)
        return out[0], out[4], sel, depth, sample, color

    @staticmethod
    def backward(ctx, g_photo, g_si, *_):
        disp, K, inv_K, P, target, beam, sel, stats, mask, reproj = ctx.saved_tensors[:10]
        srcs = ctx.saved_tensors[10:]
        cfg, NF = ctx.cfg, ctx.NF
        B, H, W = cfg.B, cfg.H, cfg.W
        g = _empty((2,), disp)
        g[0] = g_photo if g_photo is not None else 0.0
        g[1] = g_si if g_si is not None else 0.0
        d_disp = torch.empty_like(disp)
        gP = _empty((B, NF, 3, 4), disp)
        ws = _empty((query("fd_photo_bwd_ws_floats", B, H, W),), disp)
        src_arr = (ctypes.c_void_p * 3)(*[ptr(srcs[min(f, NF - 1)]) for f in range(3)])
        call("fd_photo_bwd_ex", ctypes.addressof(cfg), ptr(disp), ptr(inv_K), ptr(P), ctypes.addressof(src_arr),
             ptr(target), ptr(beam), ptr(mask), ptr(sel), ctx.has_ident, ptr(stats), ptr(g), ptr(d_disp), ptr(gP), ptr(ws),
             stream())
        gTs = []
        for f in range(3):
            if f < NF and ctx.needs_input_grad[1 + f]:
                gT = _empty((B, 4, 4), disp)
                call("fd_proj_matrix_bwd", ptr(K), gP.data_ptr() + f * 48, NF * 12, ptr(gT), B, stream())
                gTs.append(gT)
            else:
                gTs.append(None)
        g_mask = None
        if mask is not None and ctx.needs_input_grad[4]:
            # d mean(min_f mask_f r_f) / d mask_f = r_f / (B H W) where frame f won (everywhere / NF with avg_reprojection)
            if cfg.avg_reprojection and NF >= 2:
                g_mask = reproj * (g[0] / float(B * H * W * NF))
            else:
                won = sel.unsqueeze(1) == torch.arange(NF, device=sel.device, dtype=sel.dtype).view(1, NF, 1, 1)
                g_mask = reproj * won * (g[0] / float(B * H * W))
        return (d_disp, gTs[0], gTs[1], gTs[2], g_mask) + (None,) * 12


def photo_loss(disp, T_list, K, inv_K, src_list, target, ident=None, noise=None, beam=None, po=None,
               materialize=False, groups=1, mask=None):
    """Fused per-scale loss.  T_list / src_list: one to three source frames.  ``groups``: the batch is that many stacked
    micro-batches; the SI-log loss is evaluated per micro-batch and averaged.  ``mask`` [B,NF,H,W]: the predictive-mask
    baseline (trainer.py:530-541; needs ``ident is None``)."""
    po = po or PhotoOptions()
    assert 1 <= len(T_list) == len(src_list) <= 3
    Ts = list(T_list) + [None] * (3 - len(T_list))
    ss = list(src_list) + [None] * (3 - len(src_list))
    return _PhotoLoss.apply(disp, Ts[0], Ts[1], Ts[2], mask, K, inv_K, ss[0], ss[1], ss[2], target, ident, noise, beam, po,
                            materialize, int(groups))


def photo_ms_supported(po, n_src, materialize=False):
    """Configurations the multi-scale kernel covers (csrc/photometric_ms.hip, one to three source frames); the rest stays on the
    per-scale kernels."""
    return 1 <= n_src <= 3 and not po.no_ssim and not po.avg_reprojection and not materialize


class _PhotoLossMS(torch.autograd.Function):
    """All pyramid scales of generate_images_pred + the photometric / LiDAR part of compute_losses in ONE launch that also
    produces the unit-cotangent gradients (``fd_photo_ms_fwd``, csrc/photometric_ms.hip); the backward only scales them
    (``fd_photo_ms_bwd``).  One to three source frames (NF): with ``--use_stereo`` the stereo partner "s" is the only source
    frame, or the third.  A pose that requires no gradient (``stereo_T``) gets no ``fd_proj_matrix_bwd`` call and a ``None``
    gradient.

    Returns (photo_0..photo_{S-1}, si_0..si_{S-1}, sel[S,B,H,W])."""

    N_FIXED = 11                  # arguments before the NF poses, the NF source frames and the S disparities

    @staticmethod
    def forward(ctx, NF, K, inv_K, target, ident, noise, beam, po, groups, beam_scales, rows, *rest):
        Ts, srcs, disps = [f32(t) for t in rest[:NF]], [f32(t) for t in rest[NF:2 * NF]], [f32(d) for d in rest[2 * NF:]]
        S = len(disps)
        K, inv_K, target = f32(K), f32(inv_K), f32(target)
        _need_cuda(disps[0], K, inv_K, target, *srcs)
        B = disps[0].shape[0]
        H, W = target.shape[2:]
        P = _empty((B, NF, 3, 4), target)
        for f in range(NF):
            call("fd_proj_matrix_fwd", ptr(K), ptr(Ts[f]), P.data_ptr() + f * 48, NF * 12, B, stream())
        ident = f32(ident) if ident is not None else None
        beam = f32(beam) if beam is not None else None
        if noise is not None and ident is not None:
            noise = [f32(n) for n in noise]            # S tensors [B,NF,H,W] (or the S slices of one [S,B,NF,H,W] tensor)
        else:
            noise = None
        cfg = _lib.PhotoMsCfg()
        cfg.base = _photo_cfg(po, B, H, W, H, W, NF, groups)
        cfg.n_scales = S
        for s in range(S):
            cfg.Hs[s], cfg.Ws[s] = disps[s].shape[2], disps[s].shape[3]
        cfg.beam_mask = sum(1 << s for s in beam_scales if s < S) if beam is not None else 0
        cfg.rows_per_strip = int(rows)
        n0 = _PhotoLossMS.N_FIXED
        need_grad = any(ctx.needs_input_grad[n0:n0 + NF]) or any(ctx.needs_input_grad[n0 + 2 * NF:])
        sel = _empty((S, B, H, W), target, torch.uint8)
        d1 = _empty((S, B, H, W), target) if need_grad else None
        ws = _empty((query("fd_photo_ms_ws_floats", ctypes.addressof(cfg)),), target)
        out = _empty((S * _lib.PHOTO_OUT_FLOATS,), target)
        PP = ctypes.c_void_p * 4
        disp_arr = PP(*[ptr(d) for d in disps])
        noise_arr = PP(*[ptr(n) for n in noise]) if noise is not None else None
        src_arr = (ctypes.c_void_p * NF)(*[ptr(s) for s in srcs])
        call("fd_photo_ms_fwd", ctypes.addressof(cfg), ctypes.addressof(disp_arr), ptr(inv_K), ptr(P), ctypes.addressof(src_arr),
             ptr(target), ptr(ident), ctypes.addressof(noise_arr) if noise_arr is not None else None, ptr(beam), ptr(sel),
             ptr(d1), ptr(ws), ptr(out), stream())
        ctx.save_for_backward(K, out, ws, beam, *disps)
        ctx.d1, ctx.cfg, ctx.S, ctx.NF = d1, cfg, S, NF
        ctx.mark_non_differentiable(sel)
        photo = tuple(out[s * _lib.PHOTO_OUT_FLOATS] for s in range(S))
        si = tuple(out[s * _lib.PHOTO_OUT_FLOATS + 4] for s in range(S))
        return photo + si + (sel,)

    @staticmethod
    def backward(ctx, *grads):
        K, stats, ws, beam = ctx.saved_tensors[:4]
        disps = ctx.saved_tensors[4:]
        S, NF, cfg, d1 = ctx.S, ctx.NF, ctx.cfg, ctx.d1
        if d1 is None:
            raise RuntimeError("photo_loss_ms: backward called although no input required a gradient in forward")
        B = cfg.base.B
        PP = ctypes.c_void_p * 4
        keep = [f32(g).reshape(1) if g is not None else None for g in grads[:2 * S]]
        gp_arr = PP(*[ptr(g) for g in keep[:S]])
        gs_arr = PP(*[ptr(g) for g in keep[S:2 * S]])
        d_disps = [torch.empty_like(d) for d in disps]
        dd_arr = PP(*[ptr(d) for d in d_disps])
        disp_arr = PP(*[ptr(d) for d in disps])
        gP = _empty((B, NF, 3, 4), stats)
        call("fd_photo_ms_bwd", ctypes.addressof(cfg), ctypes.addressof(disp_arr), ptr(beam), ptr(stats), ctypes.addressof(gp_arr),
             ctypes.addressof(gs_arr), ptr(d1), ptr(ws), ctypes.addressof(dd_arr), ptr(gP), stream())
        gTs = []
        for f in range(NF):
            if ctx.needs_input_grad[_PhotoLossMS.N_FIXED + f]:
                gT = _empty((B, 4, 4), stats)
                call("fd_proj_matrix_bwd", ptr(K), gP.data_ptr() + f * 48, NF * 12, ptr(gT), B, stream())
                gTs.append(gT)
            else:
                gTs.append(None)
        return (None,) * _PhotoLossMS.N_FIXED + tuple(gTs) + (None,) * NF + tuple(d_disps)


def photo_loss_ms(disps, T_list, K, inv_K, src_list, target, ident=None, noise=None, beam=None, beam_scales=(), po=None,
                  groups=1, rows_per_strip=0):
    """Fused loss of ALL scales (``fd_photo_ms_*``) for one to three source frames (NF; one and three are the stereo
    configurations).  ``noise``: S tensors [B,NF,H,W] (or one [S,B,NF,H,W] tensor) or None; ``beam_scales``: the scales that
    carry the LiDAR term.  Returns ([photo_s], [si_s or None], sel[S,B,H,W])."""
    po = po or PhotoOptions()
    S = len(disps)
    if len(T_list) != len(src_list) or not photo_ms_supported(po, len(src_list)):
        raise RuntimeError("photo_loss_ms: unsupported configuration (use photo_loss per scale)")
    res = _PhotoLossMS.apply(len(src_list), K, inv_K, target, ident, noise, beam, po, int(groups), tuple(beam_scales),
                             int(rows_per_strip), *(list(T_list) + list(src_list) + list(disps)))
    photo, si, sel = list(res[:S]), list(res[S:2 * S]), res[2 * S]
    if beam is None:
        si = [None] * S
    else:
        si = [si[s] if s in beam_scales else None for s in range(S)]
    return photo, si, sel
