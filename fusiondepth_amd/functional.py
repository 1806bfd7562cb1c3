"""``torch.autograd.Function`` wrappers over the libfdhip C ABI for the network layers (layers.py ops): convolution plans, conv,
BatchNorm and pool, ``upsample_concat``, the refine inputs and Adam.  The loss path lives in loss_ops.py, batch preparation in
data_ops.py, the per-pass host state in pass_state.py and the weight-layout cache in weight_layouts.py; their public names are
re-exported here.

Host logic only: shape checks, workspace allocation from PyTorch's caching allocator, and the
forward/backward pairing.  All arithmetic happens in the HIP kernels; nothing here falls back to
torch ops on the data path.
"""
import ctypes
import weakref

import torch

from . import _lib
from . import tuning
from ._lib import _empty, _need_cuda, call, f32, ptr, query, stream
from .data_ops import (JITTER_OPS, SPARSIFY_BOX, SPARSIFY_LINE_SPEC, as_int64, color_jitter_u8, image_pyramid, lanczos_table,  # noqa: F401
                       padded_rows, raster_desc_table, resize_bilinear_batch, resize_desc_table, resize_lanczos_u8, scaled_roi,
                       scatter_2channel, sparsify_rows, sparsify_scans, u8_to_planes, velo_rasterize, velo_rasterize_batch)
from .loss_ops import (PROJECT_EPS, PhotoOptions, backproject_depth, bilinear_upsample, cat_xy, combine_losses, disp_to_depth,  # noqa: F401
                       get_smooth_loss, normalized_smooth_loss, photo_loss, photo_loss_ms, photo_ms_supported, pose_head, project_3d,
                       reprojection_loss_map, ssim, transformation_from_parameters)
from .pass_state import (add_grad_ready_callback, begin_forward_pass, bn_groups, bump_bn_counter, current_bn_groups,  # noqa: F401
                         defer_bn_counters, direct_grad_target, enable_direct_grad, enable_side_wgrad, grad_ready, has_side_wgrad,
                         join_wgrad_streams, keep_until_wgrad_join, note_use, param_uses, wgrad_stream)
from .visualize import colorize_disparity  # noqa: F401
from .weight_layouts import (build_weight_plan, bump_weights_epoch, enable_weight_cache, evict_dead_weight_layouts,  # noqa: F401
                             frozen_epoch, invalidate_frozen_layouts, refresh_weight_layouts, release_retired_layouts,
                             sync_late_layouts, unfreeze, weight_layout, weight_plan_needs_rebuild)


# ------------------------------------------------------------------------------------ conv stack --
ACT = {"none": 0, "relu": 1, "elu": 2, "sigmoid": 3, "tanh": 4}
PAD_MODE = {"zero": 0, "reflect": 1}


def _conv_desc(x, w, stride, pad, pad_mode, act, in_norm):
    d = _lib.ConvDesc()
    d.N, d.Cin, d.H, d.W = x.shape
    d.Cout, cin_w, d.KH, d.KW = w.shape
    if cin_w != d.Cin:
        raise RuntimeError("conv2d: input has %d channels, weight expects %d" % (d.Cin, cin_w))
    d.stride, d.pad, d.pad_mode, d.act, d.in_norm = stride, pad, pad_mode, act, int(in_norm)
    return d


def _conv_out_hw(d):
    return (d.H + 2 * d.pad - d.KH) // d.stride + 1, (d.W + 2 * d.pad - d.KW) // d.stride + 1


# Shape-keyed plans: the descriptor of a convolution and the workspace / layout sizes the library reports for it depend only on
# the shapes and flags, so they are asked for once per distinct layer shape instead of on every launch (a step launches ~220
# convolutions forward and as many backward; the size queries alone were ~1 300 library calls per step).
_CONV_PLANS = {}
_conv_plans_gen = 0       # tuning.generation() the plans were made under
_PLANS_EVER = []          # every descriptor ever created stays allocated (a few hundred bytes each; recorded call sequences hold their addresses)


class _ConvPlan:
    __slots__ = ("d", "dp", "Ho", "Wo", "fwd_ws", "fwd_wt", "bwd_data_ws", "bwd_data_wt", "bwd_weight_ws", "stat_slots", "bn_fused")

    def __init__(self, x, w, stride, pad, pad_mode, act, in_norm):
        self.d = _conv_desc(x, w, stride, pad, pad_mode, act, in_norm)
        self.dp = ctypes.addressof(self.d)
        _lib.HOST_PERSISTENT.add(self.dp)          # may appear as a literal in a recorded call sequence (replay.py)
        _PLANS_EVER.append(self)                   # ... so the descriptor must outlive a cleared plan table
        self.Ho, self.Wo = _conv_out_hw(self.d)
        self.fwd_ws = query("fd_conv2d_fwd_ws_floats", self.dp)
        self.fwd_wt = query("fd_conv2d_fwd_wt_floats", self.dp)
        self.stat_slots = query("fd_conv2d_fwd_stat_slots", self.dp)       # BatchNorm partial sums per (image, channel); 0: none
        self.bwd_data_ws = self.bwd_data_wt = self.bwd_weight_ws = None
        self.bn_fused = {}                 # BatchNorm groups -> fd_conv2d_fwd_bn_ok

    def fused_bn_ok(self, groups):
        ok = self.bn_fused.get(groups)
        if ok is None:
            ok = self.bn_fused[groups] = bool(query("fd_conv2d_fwd_bn_ok", self.dp, int(groups)))
        return ok

    def data_sizes(self):
        if self.bwd_data_ws is None:
            self.bwd_data_ws = max(query("fd_conv2d_bwd_data_ws_floats", self.dp), 1)
            self.bwd_data_wt = query("fd_conv2d_bwd_data_wt_floats", self.dp)
        return self.bwd_data_ws, self.bwd_data_wt

    def weight_ws(self):
        if self.bwd_weight_ws is None:
            self.bwd_weight_ws = max(query("fd_conv2d_bwd_weight_ws_floats", self.dp), 1)
        return self.bwd_weight_ws


# The library's kernel-selection thresholds (fd_tuning) change the split-K / slab workspace and weight-layout sizes, so the number of
# fd_set_tuning calls so far is part of the plan key (one integer compare; the tests and sweeps flip thresholds within a process).
def _conv_plan(x, w, stride, pad, pad_mode, act, in_norm):
    global _conv_plans_gen
    gen = tuning.generation()
    if gen != _conv_plans_gen:             # plans of an older fd_tuning can never be hit again: drop them (sweeps flip thresholds in loops)
        _CONV_PLANS.clear()
        _conv_plans_gen = gen
    key = (tuple(x.shape), tuple(w.shape), stride, pad, pad_mode, act, in_norm)
    plan = _CONV_PLANS.get(key)
    if plan is None:
        plan = _CONV_PLANS[key] = _ConvPlan(x, w, stride, pad, pad_mode, act, in_norm)
    return plan


# direct-equivalent convolution flops issued since the tally was switched on (bench.py: the MFMA fraction of the configurations that
# have no analytic table - Refiner / Completor steps); None = off, [0.0] = counting
CONV_FLOP_TALLY = None


def _tally(d, Ho, Wo, passes=1):
    if CONV_FLOP_TALLY is not None:
        CONV_FLOP_TALLY[0] += 2.0 * passes * d.N * d.Cout * Ho * Wo * d.Cin * d.KH * d.KW


def _conv_forward(ctx, x, w, bias, stride, pad, pad_mode, act, in_norm, want_stats=False):
    """-> (x as float32, y, part): ``part`` [N, Cout, S, 2] holds the per-channel (sum, M2 about the slot's own mean) of y per pixel slot,
    gathered in the convolution's epilogue for the BatchNorm that follows - or is None when ``want_stats`` is False or the
    kernel chosen for this shape has no statistics epilogue."""
    cache_id = getattr(w, "_fd_cache_id", None)
    ctx.params = (w, bias)
    note_use(w, bias)
    x, w = f32(x), f32(w)
    bias = f32(bias) if bias is not None else None
    _need_cuda(x, w)
    plan = _conv_plan(x, w, stride, pad, pad_mode, act, bool(in_norm))
    d, Ho, Wo, nws, nwt = plan.d, plan.Ho, plan.Wo, plan.fwd_ws, plan.fwd_wt
    y = _empty((d.N, d.Cout, Ho, Wo), x)
    _tally(d, Ho, Wo)
    ws = _empty((nws,), x) if nws > 0 else None
    wt, ready = weight_layout(w, cache_id, "f", nwt, d) if nwt > 0 else (None, 0)
    part = None
    # a view off a 16-byte boundary: some statistics epilogues need an aligned input, so BatchNorm makes its own pass instead
    if want_stats and plan.stat_slots > 0 and x.data_ptr() % 16 == 0:
        part = _empty((d.N, d.Cout, plan.stat_slots, 2), x)
        call("fd_conv2d_fwd_stats", plan.dp, ptr(x), ptr(w), ptr(bias), ptr(y), ptr(wt), ready, ptr(ws), ptr(part), stream())
    else:
        call("fd_conv2d_fwd", plan.dp, ptr(x), ptr(w), ptr(bias), ptr(y), ptr(wt), ready, ptr(ws), stream())
    ctx.save_for_backward(x, w, y if act != 0 else None)
    ctx.desc, ctx.has_bias, ctx.cache_id, ctx.plan = d, bias is not None, cache_id, plan
    return x, y, part


def _conv_backward(ctx, gy, gx_add=None):
    """-> (gx, gw, gb).  ``gx_add``: a second gradient arriving at the conv's input (see ``conv2d_tap``); it joins the data
    gradient in the kernel's epilogue (fd_conv2d_bwd_data_add)."""
    x, w, y = ctx.saved_tensors
    d = ctx.desc
    gx = gw = gb = None
    if gy is None:                   # only the tap was used downstream
        return (f32(gx_add) if gx_add is not None else None), None, None
    gy = f32(gy)
    if d.act != 0 and not getattr(ctx, "grad_preact", False):
        gpre = torch.empty_like(gy)
        call("fd_act_bwd", ptr(y), ptr(gy), ptr(gpre), gy.numel(), d.act, stream())
        gy = gpre
    plan = ctx.plan
    dp = plan.dp
    in_act = getattr(ctx, "in_act", 0)
    if in_act and ctx.needs_input_grad[0] and (gx_add is not None or d.in_norm):
        # the producer of x was built with grad_preact=True and has skipped its own act' pass: this layer MUST multiply by act'(x)
        # (the fallback branches below would drop it silently)
        raise RuntimeError("conv2d(in_act=...): the fused act' data gradient cannot be taken here (second incoming gradient or "
                           "normalised input) - build the producer without grad_preact")
    if ctx.needs_input_grad[0]:
        _tally(d, plan.Ho, plan.Wo)
        gx = torch.empty_like(x)
        n_ws, n_wt = plan.data_sizes()
        ws = _empty((n_ws,), x)
        wt, ready = weight_layout(w, ctx.cache_id, "d", n_wt, d)
        if in_act:
            # x is an activation output consumed by this layer alone: hand its producer the gradient w.r.t. the PRE-activation
            call("fd_conv2d_bwd_data_inact", dp, ptr(gy), ptr(w), ptr(x), in_act, ptr(gx), ptr(wt), ready, ptr(ws), stream())
        elif gx_add is not None and not d.in_norm:
            call("fd_conv2d_bwd_data_add", dp, ptr(gy), ptr(w), ptr(f32(gx_add)), ptr(gx), ptr(wt), ready, ptr(ws), stream())
        else:
            call("fd_conv2d_bwd_data", dp, ptr(gy), ptr(w), ptr(gx), ptr(wt), ready, ptr(ws), stream())
            if d.in_norm:   # d/dx of (x - 0.45) / 0.225
                call("fd_axpby", ptr(gx), ptr(gx), ptr(gx), gx.numel(), 1.0 / 0.225, 0.0, stream())
            if gx_add is not None:
                call("fd_axpby", ptr(gx), ptr(f32(gx_add)), ptr(gx), gx.numel(), 1.0, 1.0, stream())
    if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
        _tally(d, plan.Ho, plan.Wo)
        tw = direct_grad_target(ctx.params[0])
        tb = direct_grad_target(ctx.params[1]) if ctx.has_bias else None
        direct = tw is not None and (not ctx.has_bias or tb is not None)
        gw = tw if direct else torch.empty_like(w)
        gb = (tb if direct else _empty((d.Cout,), x)) if ctx.has_bias else None
        ws = _empty((plan.weight_ws(),), x)
        if direct and has_side_wgrad(ctx.params[0]):
            # a layer of the decoder's serial chain (enable_side_wgrad): its weight gradient is a leaf of the backward graph - it
            # runs on a side stream beside the data gradients of the following layers; the gradient-ready notification is given
            # with that stream current, so that a data-parallel bucket is ordered behind the kernel that really finishes it
            side = wgrad_stream()                      # ordered after everything queued so far (gy is complete)
            with torch.cuda.stream(side):
                call("fd_conv2d_bwd_weight", dp, ptr(x), ptr(gy), ptr(gw), ptr(gb), ptr(ws), 1, stream())
                grad_ready(ctx.params[0], ctx.params[1] if ctx.has_bias else None)
            keep_until_wgrad_join(x, gy, ws)
            return gx, None, None
        call("fd_conv2d_bwd_weight", dp, ptr(x), ptr(gy), ptr(gw), ptr(gb), ptr(ws), int(direct), stream())
        if direct:
            gw = gb = None          # already accumulated in place
            grad_ready(ctx.params[0], ctx.params[1] if ctx.has_bias else None)
    return gx, gw, gb


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, pad_mode, act, in_norm, grad_preact=False, in_act=0):
        ctx.grad_preact, ctx.in_act = bool(grad_preact), int(in_act)
        return _conv_forward(ctx, x, w, bias, stride, pad, pad_mode, act, in_norm)[1]

    @staticmethod
    def backward(ctx, gy):
        return _conv_backward(ctx, gy) + (None, None, None, None, None, None, None)


_NO_STATS = {}


def _no_stats(like):
    """Placeholder for "this convolution has no statistics epilogue" (autograd Functions return tensors)."""
    t = _NO_STATS.get(like.device)
    if t is None:
        t = _NO_STATS[like.device] = torch.empty((0,), device=like.device)
    return t


class _Conv2dStats(torch.autograd.Function):
    """conv2d that also returns the BatchNorm partial sums of its output (``fd_conv2d_fwd_stats``); an empty tensor when the
    kernel chosen for the shape cannot produce them."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, pad_mode, act, in_norm):
        _, y, part = _conv_forward(ctx, x, w, bias, stride, pad, pad_mode, act, in_norm, True)
        part = part if part is not None else _no_stats(y)
        ctx.mark_non_differentiable(part)
        ctx.set_materialize_grads(False)      # no zero-filled "gradient" of `part` (one fill launch per convolution otherwise)
        return y, part

    @staticmethod
    def backward(ctx, gy, _g_part):
        return _conv_backward(ctx, gy) + (None, None, None, None, None)


class _Conv2dTapStats(torch.autograd.Function):
    """``_Conv2dTap`` + the BatchNorm partial sums of ``_Conv2dStats``."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, pad_mode, act, in_norm):
        xf, y, part = _conv_forward(ctx, x, w, bias, stride, pad, pad_mode, act, in_norm, True)
        part = part if part is not None else _no_stats(y)
        ctx.mark_non_differentiable(part)
        ctx.set_materialize_grads(False)
        return y, xf.view_as(xf), part

    @staticmethod
    def backward(ctx, gy, g_tap, _g_part):
        return _conv_backward(ctx, gy, g_tap) + (None, None, None, None, None)


def conv2d_stats(x, weight, bias=None, stride=1, pad=0, pad_mode="zero", tap=False):
    """Convolution followed by a training-mode BatchNorm: -> (y, conv_stats[, x_tap]) where ``conv_stats`` goes to
    ``batch_norm(..., conv_stats=)`` (None when this shape's kernel cannot gather them: batch_norm then makes its own pass)."""
    args = (x, weight, bias, int(stride), int(pad), PAD_MODE[pad_mode], 0, False)
    if tap and torch.is_grad_enabled() and x.requires_grad:
        y, x_tap, part = _Conv2dTapStats.apply(*args)
    else:
        y, part = _Conv2dStats.apply(*args)
        x_tap = x
    part = part if part.numel() else None
    return (y, part, x_tap) if tap else (y, part)


class _Conv2dTap(torch.autograd.Function):
    """conv2d that also hands its input on: (y, x_tap) with x_tap == x.  A tensor that feeds a convolution and something else (the
    input of a ResNet block is also its residual branch) normally receives two gradients that autograd sums with an element-wise
    kernel; routing the second consumer through ``x_tap`` brings that gradient to THIS node instead, where it is added in the
    epilogue of the data-gradient kernel.  Same values, one pass over the tensor less, one launch less."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, pad_mode, act, in_norm):
        xf, y, _ = _conv_forward(ctx, x, w, bias, stride, pad, pad_mode, act, in_norm)
        return y, xf.view_as(xf)

    @staticmethod
    def backward(ctx, gy, g_tap):
        return _conv_backward(ctx, gy, g_tap) + (None, None, None, None, None)


def conv2d_tap(x, weight, bias=None, stride=1, pad=0, pad_mode="zero", act="none", in_norm=False):
    """-> (conv2d(x, ...), x): use the second value wherever ``x`` itself is needed again (see ``_Conv2dTap``)."""
    if not (torch.is_grad_enabled() and x.requires_grad):
        return conv2d(x, weight, bias, stride, pad, pad_mode, act, in_norm), x
    return _Conv2dTap.apply(x, weight, bias, int(stride), int(pad), PAD_MODE[pad_mode], ACT[act], bool(in_norm))


class _InputNormalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mean, std):
        x = f32(x)
        _need_cuda(x)
        y = torch.empty_like(x)
        call("fd_input_normalize", ptr(x), ptr(y), x.numel(), float(mean), float(std), stream())
        ctx.std = float(std)
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = f32(gy)
        gx = torch.empty_like(gy)
        call("fd_axpby", ptr(gy), ptr(gy), ptr(gx), gy.numel(), 1.0 / ctx.std, 0.0, stream())
        return gx, None, None


def stack_normalize(pieces, n_images, channels_total, normalize=True, mean=0.45, std=0.225):
    """One launch for ``torch.cat`` along batch and channels + the encoder's input normalisation: ``pieces`` = [(tensor [imgs, C, H, W]
    contiguous, first destination image, destination channel offset)]; all pieces have the same shape.  -> [n_images, channels_total,
    H, W] (fd_stack_normalize).  No gradient (network inputs)."""
    t0 = f32(pieces[0][0].detach())
    _need_cuda(t0)
    imgs, C, H, W = t0.shape
    out = _empty((n_images, channels_total, H, W), t0)
    for lo in range(0, len(pieces), 16):
        part = pieces[lo:lo + 16]
        ts = [f32(t.detach()) for t, _, _ in part]
        if any(t.shape != t0.shape for t in ts):
            raise RuntimeError("stack_normalize: pieces differ in shape")
        n = len(part)
        src = (ctypes.c_void_p * n)(*[ptr(t) for t in ts])
        di = (ctypes.c_int * n)(*[int(d) for _, d, _ in part])
        dc = (ctypes.c_int * n)(*[int(c) for _, _, c in part])
        call("fd_stack_normalize", src, di, dc, n, imgs, C, channels_total, H, W, ptr(out), int(bool(normalize)), float(mean), float(std), stream())
    return out


def input_normalize(x, mean=0.45, std=0.225):
    """``(x - mean) / std`` — the encoder's input normalisation (resnet_encoder.py:94) as its own pass, so that the stem
    convolution and its weight gradient gather plain values (the fused ``in_norm`` variant pays a division per tap)."""
    return _InputNormalize.apply(x, mean, std)


def conv2d(x, weight, bias=None, stride=1, pad=0, pad_mode="zero", act="none", in_norm=False, grad_preact=False, in_act="none"):
    """act(conv2d(pad(x)) + bias) on the MFMA implicit-GEMM kernels; ``in_norm`` folds the encoder's
    (x-0.45)/0.225 into the tap loads (resnet_encoder.py:94).

    A contract between a layer with an activation and the ONE consumer of its output, so that ``act'`` is applied where the
    gradient is produced instead of in an element-wise pass of its own (the depth decoder sets both ends, networks/depth_decoder.py):
    ``grad_preact``: the gradient this call receives already is the gradient w.r.t. its pre-activation (its consumer multiplied by
    act'(y) - ``upsample_concat(..., a_act=)`` or a ``conv2d(..., in_act=)``); ``in_act``: ``x`` is the output of that activation
    and feeds this call alone - the data gradient returned is multiplied by act'(x)."""
    if (grad_preact or ACT[in_act]) and torch.is_grad_enabled():
        return _Conv2d.apply(x, weight, bias, int(stride), int(pad), PAD_MODE[pad_mode], ACT[act], bool(in_norm), bool(grad_preact), ACT[in_act])
    return _Conv2d.apply(x, weight, bias, int(stride), int(pad), PAD_MODE[pad_mode], ACT[act], bool(in_norm))


def _bn_forward(ctx, x, weight, bias, residual, running_mean, running_var, training, momentum, eps, relu, groups, conv_stats=None):
    """Body of ``_BatchNorm.forward``; ``ctx`` is the Function's context or the BatchNorm half of a fused node (``_Part``)."""
    ctx.params = (weight, bias)
    note_use(weight, bias)
    ctx.groups = groups
    x = f32(x)
    _need_cuda(x)
    N, C, H, W = x.shape
    y = torch.empty_like(x)
    res = f32(residual) if residual is not None else None
    if training:
        mean, invstd = _empty((groups * C,), x), _empty((groups * C,), x)
        if conv_stats is not None and groups <= 16:
            # statistics gathered by the producing convolution's epilogue: one launch, no statistics pass over x
            assert conv_stats.shape[:2] == (N, C) and conv_stats.shape[3] == 2
            call("fd_bn_train_fwd_parts", ptr(x), ptr(weight), ptr(bias), ptr(res), ptr(y), ptr(running_mean), ptr(running_var),
                 ptr(mean), ptr(invstd), ptr(conv_stats), int(conv_stats.shape[2]), N, C, H, W, groups, float(eps),
                 float(momentum), int(relu), stream())
        else:
            ws = _empty((query("fd_bn_ws_floats", N, C, H, W, groups),), x)
            call("fd_bn_train_fwd", ptr(x), ptr(weight), ptr(bias), ptr(res), ptr(y), ptr(running_mean), ptr(running_var),
                 ptr(mean), ptr(invstd), ptr(ws), N, C, H, W, groups, float(eps), float(momentum), int(relu), stream())
        # ReLU without a residual input: the backward recomputes the mask from x (fd_bn_train_bwd_remask) and does not read y
        ctx.remask = bool(relu and residual is None and tuning.host.bn_remask)
        ctx.save_for_backward(x, (bias if ctx.remask else y) if relu else None, weight, mean, invstd)
    else:
        call("fd_bn_eval_fwd", ptr(x), ptr(weight), ptr(bias), ptr(res), ptr(y), ptr(running_mean), ptr(running_var),
             N, C, H, W, float(eps), int(relu), stream())
    ctx.training, ctx.relu, ctx.has_res = bool(training), int(relu), residual is not None
    return y


def _bn_backward(ctx, gy, need_res):
    """Body of ``_BatchNorm.backward`` -> (gx, gweight, gbias, gresidual)."""
    if not ctx.training:
        raise RuntimeError("BatchNorm backward is implemented for training mode only (frozen nets run under no_grad)")
    x, y, weight, mean, invstd = ctx.saved_tensors
    N, C, H, W = x.shape
    gy = f32(gy)
    gx = torch.empty_like(x)
    tw, tb = direct_grad_target(ctx.params[0]), direct_grad_target(ctx.params[1])
    direct = tw is not None and tb is not None
    gw, gb = (tw, tb) if direct else (_empty((C,), x), _empty((C,), x))
    gres = torch.empty_like(x) if ctx.has_res and need_res else None
    ws = _empty((query("fd_bn_ws_floats", N, C, H, W, ctx.groups),), x)
    if getattr(ctx, "remask", False):             # `y` holds the bias here (see _bn_forward)
        call("fd_bn_train_bwd_remask", ptr(x), ptr(gy), ptr(weight), ptr(y), ptr(mean), ptr(invstd), ptr(gx), ptr(gw), ptr(gb),
             ptr(ws), N, C, H, W, ctx.groups, int(direct), stream())
    else:
        call("fd_bn_train_bwd", ptr(x), ptr(y), ptr(gy), ptr(weight), ptr(mean), ptr(invstd), ptr(gx), ptr(gw), ptr(gb),
             ptr(gres), ptr(ws), N, C, H, W, ctx.groups, ctx.relu, int(direct), stream())
    if direct:
        gw = gb = None
        grad_ready(ctx.params[0], ctx.params[1])
    return gx, gw, gb, gres


class _BatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, training, momentum, eps, relu, groups, conv_stats=None):
        return _bn_forward(ctx, x, weight, bias, residual, running_mean, running_var, training, momentum, eps, relu, groups, conv_stats)

    @staticmethod
    def backward(ctx, gy):
        return _bn_backward(ctx, gy, ctx.needs_input_grad[3]) + (None, None, None, None, None, None, None, None)


class _Part:
    """Context of one half of a fused autograd node: what ``_conv_forward`` / ``_bn_forward`` keep between the passes.  The tensors go
    through the node's own ``save_for_backward`` (``_ConvBN``), so nothing here holds a reference to an output of the node."""
    saved_tensors = ()
    needs_input_grad = (True, True, True)

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors


def _conv_bn_fused_forward(c, b, x, w, bn_w, bn_b, residual, running_mean, running_var, stride, pad, momentum, eps, relu, groups):
    """``_conv_forward`` + ``_bn_forward`` as ONE library call where the convolution runs as F(2x2, 3x3) slabs and the BatchNorm is a
    small-plane one (ResNet layer3 / layer4): fd_conv2d_fwd_bn - the slab reduction happens inside the BatchNorm kernel.  Fills the
    two half-contexts exactly as the separate bodies do; -> (x as float32, conv output, BatchNorm output), or None when the pair does
    not qualify."""
    if groups > 16:
        return None
    xf, wf = f32(x), f32(w)
    plan = _conv_plan(xf, wf, stride, pad, 0, 0, False)
    if not plan.fused_bn_ok(groups):
        return None
    cache_id = getattr(w, "_fd_cache_id", None)
    c.params = (w, None)
    note_use(w, None)
    b.params = (bn_w, bn_b)
    note_use(bn_w, bn_b)
    d, nws, nwt = plan.d, plan.fwd_ws, plan.fwd_wt
    y = _empty((d.N, d.Cout, plan.Ho, plan.Wo), xf)
    out = torch.empty_like(y)
    _tally(d, plan.Ho, plan.Wo)
    ws = _empty((nws,), xf)
    wt, ready = weight_layout(wf, cache_id, "f", nwt, d)
    res = f32(residual) if residual is not None else None
    C = d.Cout
    mean, invstd = _empty((groups * C,), xf), _empty((groups * C,), xf)
    call("fd_conv2d_fwd_bn", plan.dp, ptr(xf), ptr(wf), ptr(y), ptr(wt), ready, ptr(ws), ptr(bn_w), ptr(bn_b), ptr(res), ptr(out),
         ptr(running_mean), ptr(running_var), ptr(mean), ptr(invstd), int(groups), float(eps), float(momentum), int(relu), stream())
    c.save_for_backward(xf, wf, None)
    c.desc, c.has_bias, c.cache_id, c.plan = d, False, cache_id, plan
    b.groups = groups
    b.remask = bool(relu and residual is None and tuning.host.bn_remask)
    b.save_for_backward(y, (bn_b if b.remask else out) if relu else None, bn_w, mean, invstd)
    b.training, b.relu, b.has_res = True, int(relu), residual is not None
    return xf, y, out


class _ConvBN(torch.autograd.Function):
    """Training-mode ``bn(conv(x)) [+ residual] [ReLU]`` of a ResNet block as ONE autograd node (bias-free convolution, zero padding,
    statistics from the convolution's epilogue where its kernel has one): the same C-ABI calls in the same order as ``_Conv2dStats``
    / ``_Conv2dTapStats`` followed by ``_BatchNorm`` - half the ``Function.apply`` calls and backward nodes for the 80 conv + BatchNorm
    pairs of the step (host time only; the launches are unchanged).  ``tap``: also return x for the block's second consumer, whose
    gradient then joins the data gradient in the kernel's epilogue (see ``_Conv2dTap``)."""

    @staticmethod
    def forward(ctx, x, w, bn_w, bn_b, residual, running_mean, running_var, stride, pad, momentum, eps, relu, groups, tap):
        c, b = _Part(), _Part()
        fused = None
        if tuning.host.fused_finish_bn and x.is_cuda:
            fused = _conv_bn_fused_forward(c, b, x, w, bn_w, bn_b, residual, running_mean, running_var, stride, pad, momentum, eps, relu, groups)
        if fused is not None:
            xf, y, out = fused
        else:
            xf, y, part = _conv_forward(c, x, w, None, stride, pad, 0, 0, False, True)
            out = _bn_forward(b, y, bn_w, bn_b, residual, running_mean, running_var, True, momentum, eps, relu, groups, part)
        ctx.n_conv = len(c.saved_tensors)
        ctx.save_for_backward(*(c.saved_tensors + b.saved_tensors))
        c.saved_tensors = b.saved_tensors = ()
        ctx.c, ctx.b = c, b
        ctx.set_materialize_grads(False)
        return (out, xf.view_as(xf)) if tap else out

    @staticmethod
    def backward(ctx, gout, g_tap=None):
        c, b = ctx.c, ctx.b
        saved = ctx.saved_tensors
        c.saved_tensors, b.saved_tensors = saved[:ctx.n_conv], saved[ctx.n_conv:]
        c.needs_input_grad = (ctx.needs_input_grad[0], ctx.needs_input_grad[1], False)
        if gout is None:                              # only the tap was used downstream
            return (f32(g_tap) if g_tap is not None else None,) + (None,) * 13
        gy, gbw, gbb, gres = _bn_backward(b, gout, ctx.needs_input_grad[4])
        gx, gw, _ = _conv_backward(c, gy, g_tap)
        c.saved_tensors = b.saved_tensors = ()
        return (gx, gw, gbw, gbb, gres) + (None,) * 9


_FOLDED = {}               # id(conv weight) -> [stamp, weakref(conv weight), folded weight, folded bias]


def folded_tensors():
    """The folded weight / bias tensors of ``conv_bn_frozen`` (persistent storage for a call recorder)."""
    return [t for e in _FOLDED.values() for t in e[2:4]]


def conv_bn_frozen(x, conv_weight, bn, stride=1, pad=0, relu=False):
    """Eval-mode ``relu?(bn(conv(x)))`` of a FROZEN network (the Refiner's stage-1 ResNets, refiner.py:56-60) with the BatchNorm folded
    into the convolution: w' = w * a[co], b' = bias - running_mean * a, a = weight / sqrt(running_var + eps) (the per-channel constants
    of k_bn_apply_eval), ReLU in the convolution's epilogue - the pass over the activation that applied them is gone.  The folded pair
    is derived once and kept until the weights / statistics change (their version counters, ``invalidate_frozen_layouts``).  The
    result differs from the two-launch form by the rounding of w * a (one ulp per weight)."""
    stamp = (conv_weight._version, frozen_epoch(), conv_weight.data_ptr(), bn.weight._version, bn.bias._version,
             bn.running_mean._version, bn.running_var._version)
    ent = _FOLDED.get(id(conv_weight))
    if ent is None or ent[0] != stamp or ent[1]() is not conv_weight:
        with torch.no_grad():
            a = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
            wf = (conv_weight.detach() * a.view(-1, 1, 1, 1)).contiguous()
            bf = (bn.bias.detach() - bn.running_mean * a).contiguous()
        enable_weight_cache([wf], frozen=True)
        key = id(conv_weight)
        ent = _FOLDED[key] = [stamp, weakref.ref(conv_weight, lambda _r, k=key: _FOLDED.pop(k, None)), wf, bf]
    return conv2d(x, ent[2], ent[3], stride, pad, "zero", "relu" if relu else "none")


def conv_bn(x, conv_weight, bn, stride=1, pad=0, residual=None, relu=False, tap=False):
    """``batch_norm(conv2d(x, w), bn, residual, relu)`` in training mode as one autograd node -> out, or (out, x_tap) with ``tap``."""
    groups = current_bn_groups()
    if bn.num_batches_tracked is not None:
        bump_bn_counter(bn.num_batches_tracked, groups)
    want_tap = bool(tap and x.requires_grad)
    res = _ConvBN.apply(x, conv_weight, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var, int(stride), int(pad),
                        bn.momentum, bn.eps, bool(relu), groups, want_tap)
    if tap:
        return res if want_tap else (res, x)
    return res


def batch_norm(x, bn, residual=None, relu=False, conv_stats=None):
    """nn.BatchNorm2d semantics (batch statistics + running-stat update in training mode) fused with the
    optional residual add and ReLU.  ``bn`` is an ``nn.BatchNorm2d`` used as the parameter/buffer holder.
    ``conv_stats``: the partial sums ``conv2d_stats`` returned for ``x`` (training mode only)."""
    training = bn.training
    groups = current_bn_groups() if training else 1
    if training and bn.num_batches_tracked is not None:
        bump_bn_counter(bn.num_batches_tracked, groups)                    # one multi-tensor add per step (trainer)
    return _BatchNorm.apply(x, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var, training, bn.momentum,
                            bn.eps, relu, groups, conv_stats if training else None)


class _BNReluPool(torch.autograd.Function):
    """Training-mode ``maxpool3x3s2(relu(bn(x)))`` of the ResNet stem as one node over fd_bn_relu_maxpool_fwd / _bwd (csrc/norm.hip):
    the full-resolution activation is written only when ``want_feat`` (features[0] has a reader) and never re-read; the backward
    recomputes the ReLU mask / normalised value from x.  Outputs: pooled, or (pooled, feat)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, groups, want_feat):
        ctx.params = (weight, bias)
        note_use(weight, bias)
        x = f32(x)
        _need_cuda(x)
        N, C, H, W = x.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        pooled = _empty((N, C, Ho, Wo), x)
        idx = _empty((N, C, Ho, Wo), x, torch.uint8)
        feat = torch.empty_like(x) if want_feat else None
        mean, invstd = _empty((groups * C,), x), _empty((groups * C,), x)
        ws = _empty((query("fd_bn_ws_floats", N, C, H, W, groups),), x)
        call("fd_bn_relu_maxpool_fwd", ptr(x), ptr(weight), ptr(bias), ptr(feat), ptr(pooled), ptr(idx), ptr(running_mean), ptr(running_var),
             ptr(mean), ptr(invstd), ptr(ws), N, C, H, W, groups, float(eps), float(momentum), stream())
        ctx.save_for_backward(x, weight, bias, mean, invstd, idx)
        ctx.groups = groups
        ctx.set_materialize_grads(False)
        return (pooled, feat) if want_feat else pooled

    @staticmethod
    def backward(ctx, g_pooled, g_feat=None):
        x, weight, bias, mean, invstd, idx = ctx.saved_tensors
        N, C, H, W = x.shape
        if g_pooled is None:                         # only features[0] was used downstream: a zero pooled gradient
            g_pooled = torch.zeros((N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), device=x.device, dtype=torch.float32)
        g_pooled = f32(g_pooled)
        g_feat = f32(g_feat) if g_feat is not None else None
        gx = torch.empty_like(x)
        tw, tb = direct_grad_target(ctx.params[0]), direct_grad_target(ctx.params[1])
        direct = tw is not None and tb is not None
        gw, gb = (tw, tb) if direct else (_empty((C,), x), _empty((C,), x))
        ws = _empty((query("fd_bn_ws_floats", N, C, H, W, ctx.groups),), x)
        call("fd_bn_relu_maxpool_bwd", ptr(x), ptr(g_pooled), ptr(idx), ptr(g_feat), ptr(weight), ptr(bias), ptr(mean), ptr(invstd), ptr(gx),
             ptr(gw), ptr(gb), ptr(ws), N, C, H, W, ctx.groups, int(direct), stream())
        if direct:
            gw = gb = None
            grad_ready(ctx.params[0], ctx.params[1])
        return gx, gw, gb, None, None, None, None, None, None


def bn_relu_maxpool(x, bn, want_feature=True):
    """``f0 = relu(bn(x)); pooled = max_pool3x3s2(f0)`` (resnet_encoder.py:95-98) -> (f0 or None, pooled).  Training mode: one fused
    node (``_BNReluPool``); eval mode: the two separate calls."""
    if not bn.training:
        f0 = batch_norm(x, bn, relu=True)
        return f0, max_pool3x3s2(f0)
    groups = current_bn_groups()
    if bn.num_batches_tracked is not None:
        bump_bn_counter(bn.num_batches_tracked, groups)
    out = _BNReluPool.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, groups, bool(want_feature))
    if not want_feature:
        return None, out
    out[1]._fd_fused_stem = True           # its backward only READS the gradient arriving at features[0] (see mark_single_consumer)
    return out[1], out[0]


def mark_single_consumer(*tensors):
    """The caller guarantees that each of these features[0] tensors of fused stem tails is consumed by ONE node (the depth
    decoder's upsample + concatenation).  ``_UpCat.backward`` then hands both encoders the same gradient tensor instead of cloning
    it: autograd passes a single incoming gradient on without accumulating into it, and ``_BNReluPool.backward`` only reads it."""
    for t in tensors:
        if t is not None and getattr(t, "_fd_fused_stem", False):
            t._fd_grad_readonly = True


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = f32(x)
        _need_cuda(x)
        N, C, H, W = x.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = _empty((N, C, Ho, Wo), x)
        idx = _empty((N, C, Ho, Wo), x, torch.uint8)
        call("fd_maxpool3x3s2_fwd", ptr(x), ptr(y), ptr(idx), N, C, H, W, stream())
        ctx.save_for_backward(idx)
        ctx.shape = x.shape
        return y

    @staticmethod
    def backward(ctx, gy):
        (idx,) = ctx.saved_tensors
        N, C, H, W = ctx.shape
        gx = _empty(ctx.shape, gy)
        call("fd_maxpool3x3s2_bwd", ptr(f32(gy)), ptr(idx), ptr(gx), N, C, H, W, stream())
        return gx


def max_pool3x3s2(x):
    """nn.MaxPool2d(kernel_size=3, stride=2, padding=1)."""
    return _MaxPool.apply(x)


class _UpCat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, s1, s2, s3, a_act=0, share_skip_grad=False):
        a = f32(a)
        ctx.a_act = int(a_act)
        if ctx.a_act:
            ctx.save_for_backward(a)
        _need_cuda(a)
        N, Ca, h, w = a.shape
        s1 = f32(s1) if s1 is not None else None
        s2 = f32(s2) if s2 is not None else None
        s3 = f32(s3) if s3 is not None else None
        Cs = s1.shape[1] if s1 is not None else 0
        C3 = s3.shape[1] if s3 is not None else 0
        out = _empty((N, Ca + Cs + C3, 2 * h, 2 * w), a)
        call("fd_upcat_fwd", ptr(a), ptr(s1), ptr(s2), ptr(s3), ptr(out), N, Ca, Cs, C3, h, w, stream())
        ctx.dims = (N, Ca, Cs, C3, h, w)
        ctx.has = (s1 is not None, s2 is not None, s3 is not None)
        ctx.share_skip_grad = bool(share_skip_grad)
        return out

    @staticmethod
    def backward(ctx, g):
        N, Ca, Cs, C3, h, w = ctx.dims
        g = f32(g)
        need_s = (ctx.has[0] and ctx.needs_input_grad[1]) or (ctx.has[1] and ctx.needs_input_grad[2])
        ga = _empty((N, Ca, h, w), g) if ctx.needs_input_grad[0] else None
        gs = _empty((N, Cs, 2 * h, 2 * w), g) if need_s else None
        g3 = _empty((N, C3, 2 * h, 2 * w), g) if ctx.has[2] and ctx.needs_input_grad[3] else None
        if ctx.a_act and ga is not None:
            (a_out,) = ctx.saved_tensors
            call("fd_upcat_bwd_act", ptr(g), ptr(a_out), ctx.a_act, ptr(ga), ptr(gs), ptr(g3), N, Ca, Cs, C3, h, w, stream())
        else:
            call("fd_upcat_bwd", ptr(g), ptr(ga), ptr(gs), ptr(g3), N, Ca, Cs, C3, h, w, stream())
        # skip and skip_add come from encoders that run their backward on DIFFERENT streams.  Handing both the same tensor is
        # a race: autograd may accumulate a second incoming gradient into it in place on one stream while the other stream's
        # kernels still read it (seen as run-to-run different encoder gradients under GPU contention).  One owner each.
        # ``share_skip_grad``: both skips are features[0] of fused stem tails (_BNReluPool): each has this node as its ONLY consumer, so
        # autograd hands the tensor on without accumulating into it, and the stem-tail backward kernels only read it - no copy.
        both = ctx.has[0] and ctx.has[1] and ctx.needs_input_grad[1] and ctx.needs_input_grad[2] and not ctx.share_skip_grad
        return ga, gs if ctx.has[0] else None, (gs.clone() if both else gs) if ctx.has[1] else None, g3, None, None


def upsample_concat(a, skip=None, skip_add=None, extra=None, a_act="none"):
    """cat([nearest_up2(a), skip (+ skip_add), extra], 1)  — depth_decoder.py:75-83 in one pass.  ``a_act``: ``a`` is the output of
    that activation, produced by a ``conv2d(..., grad_preact=True)`` and consumed here alone: its gradient is returned times act'(a)."""
    share = bool(getattr(skip, "_fd_grad_readonly", False) and getattr(skip_add, "_fd_grad_readonly", False))
    if ACT[a_act] and torch.is_grad_enabled() and a.requires_grad:
        return _UpCat.apply(a, skip, skip_add, extra, ACT[a_act], share)
    return _UpCat.apply(a, skip, skip_add, extra, 0, share)


class _Up2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = f32(x)
        _need_cuda(x)
        N, C, h, w = x.shape
        y = _empty((N, C, 2 * h, 2 * w), x)
        call("fd_upsample2x_fwd", ptr(x), ptr(y), N * C, h, w, stream())
        ctx.shape = x.shape
        return y

    @staticmethod
    def backward(ctx, g):
        N, C, h, w = ctx.shape
        gx = _empty(ctx.shape, g)
        call("fd_upsample2x_bwd", ptr(f32(g)), ptr(gx), N * C, h, w, stream())
        return gx


def upsample_nearest2x(x):
    return _Up2.apply(x)


class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = f32(a), f32(b)
        _need_cuda(a, b)
        out = torch.empty_like(a)
        call("fd_axpby", ptr(a), ptr(b), ptr(out), a.numel(), 1.0, 1.0, stream())
        return out

    @staticmethod
    def backward(ctx, g):
        # the two operands belong to encoders on different streams: separate gradient tensors (see _UpCat.backward)
        return g, (g.clone() if ctx.needs_input_grad[0] and ctx.needs_input_grad[1] else g)


def add(a, b):
    """Feature fusion a + b (depth_decoder.py:70, pose_decoder.py:31)."""
    return _Add.apply(a, b)


class _SpatialMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale):
        x = f32(x)
        _need_cuda(x)
        N, C, H, W = x.shape
        out = _empty((N, C), x)
        call("fd_spatial_mean_fwd", ptr(x), ptr(out), N * C, H * W, float(scale), stream())
        ctx.shape, ctx.scale = x.shape, float(scale)
        return out

    @staticmethod
    def backward(ctx, g):
        N, C, H, W = ctx.shape
        gx = _empty(ctx.shape, g)
        call("fd_spatial_mean_bwd", ptr(f32(g)), ptr(gx), N * C, H * W, ctx.scale, stream())
        return gx, None


def spatial_mean(x, scale=1.0):
    """scale * x.mean(3).mean(2)  (pose_decoder.py:44-46)."""
    return _SpatialMean.apply(x, scale)


def resize_linear_cv(x, size):
    """``cv2.resize(img, (size[1], size[0]))`` (INTER_LINEAR, float32) for every plane of ``x`` [..., H, W] -> [..., size[0], size[1]]
    (evaluate_depth.py:349; OpenCV's coefficient rule, see fd_resize_linear_cv)."""
    x = f32(x.detach())
    _need_cuda(x)
    H, W = x.shape[-2:]
    planes = x.numel() // (H * W)
    y = _empty(tuple(x.shape[:-2]) + (int(size[0]), int(size[1])), x)
    call("fd_resize_linear_cv", ptr(x), ptr(y), planes, H, W, int(size[0]), int(size[1]), stream())
    return y


def masked_median(x, gate, scale=1.0, window=None):
    """``torch.median(x[mask] * scale)`` with ``mask = gate > 0`` inside ``window`` = (y0, y1, x0, x1) of every plane (default: the
    whole plane), over the whole batch - refiner.py:327-331.  A 0-dim device tensor; no host round trip, no sort."""
    x, gate = f32(x.detach()), f32(gate.detach())
    _need_cuda(x, gate)
    if x.shape != gate.shape:
        raise RuntimeError("masked_median: x %s and gate %s differ in shape" % (tuple(x.shape), tuple(gate.shape)))
    H, W = x.shape[-2:]
    B = x.numel() // (H * W)
    y0, y1, x0, x1 = window if window is not None else (0, H, 0, W)
    out = _empty((2,), x)
    ws = torch.empty((query("fd_masked_median_ws_bytes", B, H, W),), device=x.device, dtype=torch.uint8)
    call("fd_masked_median", ptr(x), ptr(gate), float(scale), B, H, W, int(y0), int(y1), int(x0), int(x1), ptr(out), ws.data_ptr(), stream())
    return out[0]


def refine_inputs(disps, beam, two_cha, inv_Ks, height, width, min_depth, max_depth, catxy=True, pool_disp0=True,
                  crop=(78, 190, 23, 617), return_stats=False):
    """refiner.py:316-348 for all scales in four launches (csrc/refine.hip): -> list of [B, 1 + 3*catxy + 2, Hs, Ws] tensors, the
    ``depth_maps`` inputs of the refine decoder (scaled disparity | Cat_xy of the pooled depth | pooled 2-channel LiDAR map).
    ``disps``: ``outputs[("disp", s)]`` per scale (only ``disps[0]`` is read when ``pool_disp0`` = --refine_a0 true);
    ``inv_Ks``: ``inputs[("inv_K", s)]`` per scale.  No gradient (the reference computes all of it under no_grad)."""
    S = len(disps)
    d0 = f32(disps[0].detach())
    beam, two_cha = f32(beam.detach()), f32(two_cha.detach())
    _need_cuda(d0, beam, two_cha)
    B = d0.shape[0]
    cfg = _lib.RefineCfg()
    cfg.B, cfg.H, cfg.W, cfg.n_scales = B, int(height), int(width), S
    ds, ks = [], []
    for s in range(S):
        cfg.Hs[s], cfg.Ws[s] = (int(disps[s].shape[2]), int(disps[s].shape[3]))
        ds.append(d0 if s == 0 else (None if pool_disp0 else f32(disps[s].detach())))
        ks.append(f32(inv_Ks[s].detach()) if catxy else None)
    # the reference writes `crop_mask[:, :, 78:190, 23:617] = 1` (refiner.py:329): a slice, i.e. silently clamped to the plane - at 96x320 or
    # 128x416 the window shrinks, below 79 rows it is empty (medians NaN, as torch.median of an empty selection); ADVICE round 5
    y0, y1, x0, x1 = (int(v) for v in crop)
    y1, x1 = min(y1, int(height)), min(x1, int(width))
    y0, x0 = min(y0, y1), min(x0, x1)
    cfg.crop_y0, cfg.crop_y1, cfg.crop_x0, cfg.crop_x1 = y0, y1, x0, x1
    cfg.min_depth, cfg.max_depth, cfg.catxy, cfg.pool_disp0 = float(min_depth), float(max_depth), int(bool(catxy)), int(bool(pool_disp0))
    C = 1 + (3 if catxy else 0) + 2
    outs = [_empty((B, C, cfg.Hs[s], cfg.Ws[s]), d0) for s in range(S)]
    ws = torch.empty((query("fd_refine_inputs_ws_bytes", ctypes.byref(cfg)),), device=d0.device, dtype=torch.uint8)
    stats = _empty((S, 4), d0) if return_stats else None
    arr = lambda ts: (ctypes.c_void_p * 4)(*[ptr(t) for t in ts] + [None] * (4 - len(ts)))
    call("fd_refine_inputs", ctypes.byref(cfg), arr(ds), ptr(beam), ptr(two_cha), arr(ks), arr(outs), ptr(stats), ws.data_ptr(), stream())
    return (outs, stats) if return_stats else outs


def depth_errors(gt, pred):
    """layers.py:284-302 on matched 1-D tensors -> 7 scalars (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3)."""
    gt, pred = f32(gt.detach()).reshape(-1), f32(pred.detach()).reshape(-1)
    _need_cuda(gt, pred)
    out, ws = _empty((7,), gt), _empty((7 * 256,), gt)
    call("fd_depth_errors", ptr(gt), ptr(pred), gt.numel(), ptr(out), ptr(ws), stream())
    return tuple(out[i] for i in range(7))


def class_errors(gt, pred, labels, num_classes=34, lo=1e-3, hi=80):
    """evaluate_depth.py:455-467 on matched 1-D device tensors (float32, float32, uint8): for every class c < ``num_classes`` the
    metrics of the pairs whose label is c, ``pred`` clamped to [lo, hi] -> [K, 8] float64 device tensor (abs_rel, sq_rel, rmse,
    rmse_log, a1, a2, a3, count); a class without pairs gives eight zeros (fd_class_errors).  No CPU path."""
    _need_cuda(gt, pred, labels)
    if labels.dtype != torch.uint8:
        raise RuntimeError("class_errors: labels must be uint8, got %s" % labels.dtype)
    gt, pred, labels = f32(gt.detach()).reshape(-1), f32(pred.detach()).reshape(-1), labels.contiguous().reshape(-1)
    if not gt.numel() == pred.numel() == labels.numel():
        raise ValueError("class_errors: %d ground-truth values, %d predictions, %d labels" % (gt.numel(), pred.numel(), labels.numel()))
    out = _empty((max(int(num_classes), 0), 8), gt, torch.float64)
    call("fd_class_errors", ptr(gt), ptr(pred), ptr(labels), gt.numel(), int(num_classes), float(lo), float(hi), out.data_ptr(), stream())
    return out


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0):
    """One torch.optim.Adam update of a flat fp32 tensor, in place."""
    bc1, bc2 = 1.0 - betas[0] ** step, 1.0 - betas[1] ** step
    sync_late_layouts()
    bump_weights_epoch()
    call("fd_adam_step", ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), float(lr), betas[0],
         betas[1], float(eps), bc1, bc2, float(grad_scale), stream())
    refresh_weight_layouts()


def adam_step_dev(param, grad, exp_avg, exp_avg_sq, state, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, zero_grad=False):
    """Adam update whose step counter / lr live in ``state`` (device, [step, lr]) — hipGraph-replay safe.  ``zero_grad``: the same
    launch leaves ``grad`` all zeros (fd_adam_step_dev_zero)."""
    sync_late_layouts()
    bump_weights_epoch()
    call("fd_adam_step_dev_zero" if zero_grad else "fd_adam_step_dev", ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq),
         param.numel(), ptr(state), betas[0], betas[1], float(eps), float(grad_scale), stream())
    refresh_weight_layouts()


GUARD_MAX_SEGMENTS = 16      # FD_GUARD_MAX_SEGMENTS


def _guard_ptr(t, dtype, numel, what):
    """Device pointer of a contiguous ``dtype`` CUDA tensor of at least ``numel`` elements (the guard's small tables)."""
    _need_cuda(t)
    if t.dtype != dtype or not t.is_contiguous() or t.numel() < numel:
        raise RuntimeError("%s must be a contiguous %s tensor of at least %d elements, got %s[%d]" % (what, dtype, numel, t.dtype, t.numel()))
    return t.data_ptr()


def grad_stats_ws_bytes(n, n_seg):
    """Bytes of the ``ws`` that ``grad_stats`` of ``n`` gradient elements in ``n_seg`` segments needs (fd_grad_stats_ws_bytes)."""
    size = query("fd_grad_stats_ws_bytes", int(n), int(n_seg))
    if size < 0:
        raise ValueError("grad_stats: %d elements in %d segments (1 .. %d segments are covered)" % (n, n_seg, GUARD_MAX_SEGMENTS))
    return size


def grad_stats(grad, seg_offsets, ws, stats, counters, adam_state, grad_scale=1.0, max_norm=0.0, skip_nonfinite=True):
    """fd_grad_stats: the float64 norms (overall and per segment), the non-finite count, the clip factor and the skip decision of
    ``grad * grad_scale``, left in ``stats`` (float64, 4 + n_seg) and ``counters`` (int64, 3) on the device; no host read.
    ``seg_offsets``: int64 device tensor of n_seg + 1 element offsets, 0 first, ``grad.numel()`` last."""
    n_seg = seg_offsets.numel() - 1
    n = grad.numel()
    need = grad_stats_ws_bytes(n, n_seg)
    _need_cuda(ws)
    if not ws.is_contiguous() or ws.numel() * ws.element_size() < need or ws.data_ptr() % 8:
        raise RuntimeError("grad_stats: ws must be contiguous, 8-byte aligned and hold %d bytes" % need)
    call("fd_grad_stats", ptr(grad), n, _guard_ptr(seg_offsets, torch.int64, 2, "seg_offsets"), n_seg, float(grad_scale),
         float(max_norm), int(bool(skip_nonfinite)), ws.data_ptr(), _guard_ptr(stats, torch.float64, 4 + n_seg, "stats"),
         _guard_ptr(counters, torch.int64, 3, "counters"), ptr(adam_state), stream())


def adam_step_guarded(param, grad, exp_avg, exp_avg_sq, state, stats, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, zero_grad=False):
    """``adam_step_dev`` behind the decision ``grad_stats`` left in ``stats``: the gradient is also multiplied by ``stats[2]`` (the clip
    factor), and with ``stats[3]`` set neither the parameters, the moments nor the step count change (fd_adam_step_guarded).
    ``zero_grad`` clears the gradient in both cases."""
    sync_late_layouts()
    bump_weights_epoch()
    call("fd_adam_step_guarded", ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), ptr(state), betas[0], betas[1],
         float(eps), float(grad_scale), _guard_ptr(stats, torch.float64, 4, "stats"), int(bool(zero_grad)), stream())
    refresh_weight_layouts()
