"""Every routed convolution shape of tests/golden/make_conv_routes.py (the layers of the benchmarked networks at their real batch, plus
the grid around every routing threshold), run through the raw C ABI on exact data and compared with float64 bit for bit.

Exact data.  x, w and gy are integers in -2..2 (zero mean), bias, gx_add and the accumulation buffers integers as well.  Every kernel
family is then exact in fp32: the Winograd transforms are dyadic (0, +-1, 1/2, 1/4), bf16 limbs hold such integers exactly, the ring /
fold, split-K and slab reductions are plain additions.  The only condition is that no partial sum exceeds 2^24 units of its granularity
(1/4, what the transforms give), i.e. |partial| < 2^22.  _Data.budget() asserts that per case and direction from the nonzero counts and the
largest magnitudes, times a transform gain of 16 (F(2x2,3x3), a worst case); the weight gradient's reduction runs over up to 737 k
pixels, so gy is made sparser where it is long.

Reference.  Float64 on the CPU, through two independent random projections with nonzero integer entries (Freivalds): r over Cout for
y, s over Cin for gx, both for gw.  A projection of a GPU result is a float64 sum of integers, exact in any order.  Where a case is
small the whole result is compared element by element as well.

Not exact: the in_norm stems ((x - 0.45) / 0.225) and the ELU / sigmoid / tanh forward.  Their pre-activation runs as the same
convolution without activation (checked exact like the others); the activation output of the first, a middle and the last image is
compared with float64 within 4 fp32 ulp + 2^-22.  in_norm is compared on the same three images within 2^-18 * conv(|x_hat|, |w|).

Per case: forward (wt_ready 0, 1, and a layout written by fd_relayout_batch from fd_conv2d_relayout_jobs; + bias; statistics where
stat_slots > 0), data gradient (the same three layouts; _add; _inact with every activation id), weight gradient (accumulate 0 / 1,
bias gradient), and x / gy at a one-float storage offset (bitwise the same result, or the documented alignment error).  Then every
fd_tuning setting whose route-table row differs from the default row, plus the four settings that never change a row (selected by the
family fd_tuning.log names under the defaults), must give the default's exact results bit for bit."""
import ctypes
import os
import re
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fusiondepth_amd import functional as FD, tuning
from fusiondepth_amd._lib import ConvDesc, RelayoutJob, call, ptr, query, stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
try:
    import make_conv_routes as gen
finally:
    sys.path.remove(GOLDEN)

F64 = torch.float64
LIMIT = 1 << 22                  # |partial sum| < 2^24 units of 1/4
GAIN = 16                        # F(2x2,3x3) transform gain, worst case
FULL_MACS = 6e7                  # element-wise float64 comparison of a whole result below this many multiply-adds per direction
DOCUMENTED_MISALIGNED = "needs a 16-byte aligned input"
DOCUMENTED_IN_NORM = "in_norm is only built for the 7x7 stem"
ACT_NAMES = {v: k for k, v in gen.ACT.items()}

with np.load(os.path.join(GOLDEN, "conv_routes.npz")) as _npz:
    _Z = {k: _npz[k] for k in _npz.files}
DESCS = [tuple(int(v) for v in row) for row in gen.cases()]
SETTINGS = [str(s) for s in _Z["settings"]]
ROW_KEYS = ("sizes", "bn_ok", "njobs", "jobs")
N_NETWORK = len(set(gen.network_cases()))


_ROW_DIFF = np.zeros((len(SETTINGS), len(DESCS)), bool)          # [setting, case]: its route-table row differs from the default row
for _k in ROW_KEYS:
    _ROW_DIFF |= (_Z[_k] != _Z[_k][:1]).reshape(len(SETTINGS), len(DESCS), -1).any(2)


def _row_settings(ci):
    return [SETTINGS[si] for si in np.flatnonzero(_ROW_DIFF[:, ci])]


def _kw(setting):
    return dict((k, int(v)) for k, v in (p.split("=") for p in setting.split(",") if p))


def _log_only_settings(t, fams):
    """(setting, directions) of the row-neutral settings that can change this case's kernel: the 7x7 stems (fwd 'stem7', wgrad
    'stem'), reflect-padded data gradients on planes between 4 096 and 16 384 pixels (ring or padded grid), Winograd weight
    gradients (f32 or limb matrix loop)."""
    N, Cin, H, W, Cout, K = t[:6]
    out = []
    if fams.get("fwd") == "stem7" or fams.get("wgrad") == "stem":
        out.append(("stem7=0", "fw"))
    if t[9] == 1 and 4096 <= H * W < 16384:
        out.append(("reflect_ring=4096", "d"))
    if fams.get("wgrad") == "wino":
        out += [("wino_wgrad_limb=0", "w"), ("wino_wgrad_limb=1", "w")]
    return out


def _out_hw(t):
    N, Cin, H, W, Cout, K, _, s, p = t[:9]
    return (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1


def _case_id(ci):
    N, Cin, H, W, Cout, K, _, s, p, pm, act, inn = DESCS[ci]
    return "c%03d-n%d_%d-%d_%dx%d_k%ds%dp%d%s%s%s" % (ci, N, Cin, Cout, H, W, K, s, p, "_refl" if pm else "",
                                                     "_" + ACT_NAMES[act] if act else "", "_innorm" if inn else "")


# ---------------------------------------------------------------------------------------------------------------- reference (CPU)
def _pad(x, t):
    p = t[8]
    return F.pad(x, (1, 1, 1, 1), mode="reflect") if t[9] == 1 else F.pad(x, (p, p, p, p))


def _ref_fwd(x, w, t):
    """float64 conv(x [N,C,H,W], w [V,C,K,K]) with the case's stride / padding -> [N,V,Ho,Wo]: per tap a product over the channels of the
    padded grid, added at the tap's offset (a GEMM per image chunk; torch's float64 conv2d is an order of magnitude slower here)."""
    s, K = t[7], t[5]
    Ho, Wo = _out_hw(t)
    xp = _pad(x, t)
    N, C, Hp, Wp = xp.shape
    V = w.shape[0]
    wm = w.permute(2, 3, 0, 1).reshape(K * K * V, C)
    out = torch.zeros(N, V, Ho, Wo, dtype=F64)
    step = max(1, int(4e7 // (K * K * V * Hp * Wp)))
    for n0 in range(0, N, step):
        z = torch.matmul(wm, xp[n0:n0 + step].reshape(-1, C, Hp * Wp)).view(-1, K, K, V, Hp, Wp)
        for kh in range(K):
            for kw in range(K):
                out[n0:n0 + step] += z[:, kh, kw, :, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s]
    return out


def _ref_dgrad(gy, w, t):
    """float64 data gradient of gy [N,Co,Ho,Wo] through w [Co,V,K,K] (the adjoint of _ref_fwd, reflect fold included) -> [N,V,H,W]."""
    N, _, H, W = t[:4]
    K, s, p = t[5], t[7], t[8]
    Ho, Wo = _out_hw(t)
    pp = 1 if t[9] == 1 else p
    Hp, Wp = H + 2 * pp, W + 2 * pp
    Co, V = w.shape[:2]
    wm = w.permute(2, 3, 1, 0).reshape(K * K * V, Co)
    g = torch.zeros(N, V, Hp, Wp, dtype=F64)
    step = max(1, int(4e7 // (K * K * V * Ho * Wo)))
    for n0 in range(0, N, step):
        z = torch.matmul(wm, gy[n0:n0 + step].reshape(-1, Co, Ho * Wo)).view(-1, K, K, V, Ho, Wo)
        for kh in range(K):
            for kw in range(K):
                g[n0:n0 + step, :, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s] += z[:, kh, kw]
    if t[9] == 1:
        z = torch.zeros(N, V, H, W, dtype=F64, requires_grad=True)
        return torch.autograd.grad(F.pad(z, (1, 1, 1, 1), mode="reflect"), z, g)[0]
    return g[:, :, pp:pp + H, pp:pp + W].contiguous()


def _ref_wgrad(gy, x, t):
    """float64 weight gradient sum_{n,p} gy[n,a,p] * xpad[n,b,p+tap] for gy [N,A,Ho,Wo], x [N,B,H,W] -> [A,B,K,K]."""
    K, s = t[5], t[7]
    Ho, Wo = _out_hw(t)
    xp = _pad(x, t)
    N, A = gy.shape[:2]
    B = xp.shape[1]
    g2 = gy.permute(1, 0, 2, 3).reshape(A, -1)
    out = torch.empty(A, B, K, K, dtype=F64)
    for kh in range(K):
        for kw in range(K):
            xs = xp[:, :, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s].permute(1, 0, 2, 3).reshape(B, -1)
            out[:, :, kh, kw] = g2 @ xs.T
    return out


def _act64(a, act):
    return {1: torch.relu, 2: F.elu, 3: torch.sigmoid, 4: torch.tanh}[act](a)


def _act_grad_factor(xin, act):
    """act'(pre) written through the activation's OUTPUT xin (fd_act_bwd's convention), float64."""
    return {1: (xin > 0).to(F64), 2: torch.where(xin > 0, torch.ones_like(xin), xin + 1), 3: xin * (1 - xin), 4: 1 - xin * xin}[act]


# ---------------------------------------------------------------------------------------------------------------- data
class _Data:
    """Integer tensors of one case, on the GPU (float32) and the CPU (float64), and the two projection pairs (r over Cout, s over Cin)."""

    def __init__(self, ci, t):
        N, Cin, H, W, Cout, K = t[:6]
        Ho, Wo = _out_hw(t)
        g = torch.Generator(device="cuda").manual_seed(7919 * ci + 13)
        cpu = torch.Generator().manual_seed(7919 * ci + 17)
        ints = lambda shape, lo=-2, hi=3: torch.randint(lo, hi, shape, generator=g, device="cuda", dtype=torch.int8)
        x8, w8 = ints((N, Cin, H, W)), ints((Cout, Cin, K, K))
        gy8 = ints((N, Cout, Ho, Wo))
        # the weight gradient sums over N*Ho*Wo pixels: keep at most ~0.7 * LIMIT / (GAIN * 2 * 2) nonzeros per output channel
        dens = min(1.0, 0.7 * LIMIT / (GAIN * 4) / (0.8 * N * Ho * Wo))
        if dens < 1.0:
            gy8 *= (torch.rand(gy8.shape, generator=g, device="cuda") < dens).to(torch.int8)
        self.x, self.w, self.gy = x8.float(), w8.float(), gy8.float()
        self.bias = ints((Cout,)).float()
        self.gx_add = ints((N, Cin, H, W)).float()
        self.gw0, self.gb0 = ints((Cout, Cin, K, K)).float(), ints((Cout,)).float()
        self.x_in = ints((N, Cin, H, W), -3, 4).float() / 4          # dyadic: every act'(x_in) times an integer stays exact
        self.x_mis, self.gy_mis = _misaligned(self.x), _misaligned(self.gy)
        self.xc, self.wc, self.gyc = x8.cpu().to(F64), w8.cpu().to(F64), gy8.cpu().to(F64)
        pick = lambda n: (torch.randint(1, 4, (2, n), generator=cpu) * (1 - 2 * torch.randint(0, 2, (2, n), generator=cpu))).to(F64)
        self.r, self.s = pick(Cout), pick(Cin)
        self.nnz_gy = int((gy8 != 0).sum((0, 2, 3)).max())

    def budget(self, t):
        """largest possible |partial sum| of the forward, data-gradient and weight-gradient reductions (in units of 1)"""
        w = self.wc != 0
        fwd = int(w.sum((1, 2, 3)).max()) * 2 * 2 * GAIN + 2
        dgrad = int(w.sum((0, 2, 3)).max()) * 2 * 2 * GAIN + 2
        wgrad = self.nnz_gy * 2 * 2 * GAIN + 2
        return {"fwd": fwd, "dgrad": dgrad, "wgrad": wgrad}


def _misaligned(t):
    """a copy of t at a one-float storage offset (4-byte but not 16-byte aligned)"""
    buf = torch.empty(t.numel() + 4, device=t.device)
    m = buf[1:1 + t.numel()].view(t.shape)
    m.copy_(t)
    return m


def _nan(shape):
    return torch.full(shape if isinstance(shape, tuple) else (max(int(shape), 1),), float("nan"), device="cuda")


# ---------------------------------------------------------------------------------------------------------------- one run
def _try(name, *args):
    try:
        call(name, *args)
        return None
    except RuntimeError as e:
        return str(e)


def _batch_layout(dp, kind, w, n):
    """the weight layout of direction `kind` written by ONE fd_relayout_batch launch from fd_conv2d_relayout_jobs (NaN elsewhere)"""
    wt = _nan(n)
    jobs = (RelayoutJob * 4)()
    nj = query("fd_conv2d_relayout_jobs", dp, kind, ptr(w), ptr(wt), ctypes.addressof(jobs))
    if nj > 0:
        blocks = query("fd_relayout_plan", ctypes.addressof(jobs), nj)
        dev = torch.frombuffer(bytearray(bytes(memoryview(jobs))[: nj * ctypes.sizeof(RelayoutJob)]), dtype=torch.uint8).cuda()
        call("fd_relayout_batch", ptr(dev), nj, blocks, stream())
        torch.cuda.synchronize()
    return wt


def _run(t, D, dirs="fdw", full=True):
    """Every entry point of case t on data D under the current fd_tuning -> (outputs, errors).  NaN-filled outputs, layouts and
    workspaces: an element a kernel fails to write, or a NaN it reads, shows up.  full=False (the settings): without the wt_ready = 1
    repeats, and with _inact only where the one-channel stencil fuses it (elsewhere it is this data gradient + fd_act_bwd)."""
    d = ConvDesc(*t)
    dp = ctypes.addressof(d)
    N, Cin, H, W, Cout, K = t[:6]
    Ho, Wo = _out_hw(t)
    st = stream()
    o, err = {}, {}
    if "f" in dirs:
        wt, ws = _nan(query("fd_conv2d_fwd_wt_floats", dp)), _nan(query("fd_conv2d_fwd_ws_floats", dp))
        fwd = lambda x, b, lay, ready, y: _try("fd_conv2d_fwd", dp, ptr(x), ptr(D.w), ptr(b), ptr(y), ptr(lay), ready, ptr(ws), st)
        for key, x, b, lay, ready in (("y", D.x, None, wt, 0), ("y_ready", D.x, None, wt, 1), ("y_bias", D.x, D.bias, wt, 1),
                                      ("y_mis", D.x_mis, None, wt, 1)):
            if key == "y_ready" and not full:
                continue
            o[key] = _nan((N, Cout, Ho, Wo))
            err[key] = fwd(x, b, lay, ready, o[key])
        o["y_batch"] = _nan((N, Cout, Ho, Wo))
        err["y_batch"] = fwd(D.x, None, _batch_layout(dp, 0, D.w, wt.numel()), 1, o["y_batch"])
        slots = query("fd_conv2d_fwd_stat_slots", dp)
        if slots > 0:
            for key, x in (("y_stats", D.x), ("y_stats_mis", D.x_mis)):
                o[key], o[key + "_part"] = _nan((N, Cout, Ho, Wo)), _nan((N, Cout, slots, 2))
                err[key] = _try("fd_conv2d_fwd_stats", dp, ptr(x), ptr(D.w), None, ptr(o[key]), ptr(wt), 1, ptr(ws), ptr(o[key + "_part"]), st)
    if "d" in dirs:
        wt, ws = _nan(query("fd_conv2d_bwd_data_wt_floats", dp)), _nan(query("fd_conv2d_bwd_data_ws_floats", dp))
        for key, gy, lay, ready in (("gx", D.gy, wt, 0), ("gx_ready", D.gy, wt, 1), ("gx_mis", D.gy_mis, wt, 1),
                                    ("gx_batch", D.gy, _batch_layout(dp, 1, D.w, wt.numel()), 1)):
            if key == "gx_ready" and not full:
                continue
            o[key] = _nan((N, Cin, H, W))
            err[key] = _try("fd_conv2d_bwd_data", dp, ptr(gy), ptr(D.w), ptr(o[key]), ptr(lay), ready, ptr(ws), st)
        o["gx_add"] = _nan((N, Cin, H, W))
        err["gx_add"] = _try("fd_conv2d_bwd_data_add", dp, ptr(D.gy), ptr(D.w), ptr(D.gx_add), ptr(o["gx_add"]), ptr(wt), 1, ptr(ws), st)
        for a in (1, 2, 3, 4) if full or Cout == 1 else ():
            key = "gx_inact%d" % a
            o[key] = _nan((N, Cin, H, W))
            err[key] = _try("fd_conv2d_bwd_data_inact", dp, ptr(D.gy), ptr(D.w), ptr(D.x_in), a, ptr(o[key]), ptr(wt), 1, ptr(ws), st)
    if "w" in dirs:
        ws = _nan(query("fd_conv2d_bwd_weight_ws_floats", dp))
        for key, x, gy, acc in (("gw", D.x, D.gy, 0), ("gw_acc", D.x, D.gy, 1), ("gw_mis", D.x_mis, D.gy_mis, 0)):
            o[key] = D.gw0.clone() if acc else _nan((Cout, Cin, K, K))
            o[key + "_b"] = D.gb0.clone() if acc else _nan((Cout,))
            err[key] = _try("fd_conv2d_bwd_weight", dp, ptr(x), ptr(gy), ptr(o[key]), ptr(o[key + "_b"]), ptr(ws), acc, st)
    torch.cuda.synchronize()
    return o, err


# ---------------------------------------------------------------------------------------------------------------- checks
def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _first_diff(a, b):
    bad = (a.view(torch.int32) != b.view(torch.int32)).nonzero()
    i = tuple(bad[0].tolist())
    return "%d elements differ; first at %s: %r vs %r" % (len(bad), i, float(a[i]), float(b[i]))


def _expect_same(what, got, want):
    assert _same(got, want), "%s: %s" % (what, _first_diff(got, want))


def _exact_keys(t):
    """outputs that must be exact (and so identical under every setting and layout)"""
    act, inn = t[10], t[11]
    keys = ["gx", "gx_ready", "gx_mis", "gx_batch", "gx_add"] + ["gx_inact%d" % a for a in (1, 2, 3, 4)]
    if not inn:
        keys += ["gw", "gw_b", "gw_acc", "gw_acc_b", "gw_mis", "gw_mis_b"]
        if act in (0, 1):
            keys += ["y", "y_ready", "y_bias", "y_mis", "y_batch", "y_stats", "y_stats_mis"]
    else:
        keys += ["gw_b", "gw_acc_b", "gw_mis_b"]
    return keys


def _check_errors(t, err, ctx):
    """a call may fail only with a documented error: an input off 16-byte alignment where a kernel needs it, in_norm off the 7x7 stem"""
    for key, e in err.items():
        if e is None:
            continue
        if t[11] and t[5] != 7 and DOCUMENTED_IN_NORM in e and (key.startswith("y") or key.startswith("gw")) and not key.endswith("_b"):
            continue
        if key.endswith("_mis") and DOCUMENTED_MISALIGNED in e:
            continue
        raise AssertionError("%s: %s failed: %s" % (ctx, key, e))


def _check_internal(t, D, o, err, ctx):
    """the relations between the runs of one setting that hold bit for bit"""
    ok = lambda k: k in o and err.get(k) is None
    if ok("y") and t[10] in (0, 1) and not t[11]:        # (the non-exact outputs are each compared with float64 instead)
        for k in ("y_ready", "y_batch", "y_mis", "y_stats", "y_stats_mis"):
            if ok(k):
                _expect_same("%s: %s vs y" % (ctx, k), o[k], o["y"])
        if ok("y_stats") and ok("y_stats_mis"):
            _expect_same("%s: slot sums of the misaligned input" % ctx, o["y_stats_mis_part"][..., 0], o["y_stats_part"][..., 0])
        if t[10] == 0 and ok("y_bias"):
            _expect_same("%s: y + bias" % ctx, o["y_bias"], o["y"] + D.bias.view(1, -1, 1, 1))
    if ok("gx"):
        for k in ("gx_ready", "gx_batch", "gx_mis"):
            if ok(k):
                _expect_same("%s: %s vs gx" % (ctx, k), o[k], o["gx"])
        _expect_same("%s: gx + gx_add" % ctx, o["gx_add"], o["gx"] + D.gx_add)
        g64 = o["gx"].to(F64)
        for a in (1, 2, 3, 4):
            if not ok("gx_inact%d" % a):
                continue
            want = (g64 * _act_grad_factor(D.x_in.to(F64), a)).float()
            _expect_same("%s: gx * act%d'(x_in)" % (ctx, a), o["gx_inact%d" % a], want)
    if ok("gw") or ok("gw_acc"):
        _expect_same("%s: accumulated bias gradient" % ctx, o["gw_acc_b"], o["gw_b"] + D.gb0)
        _expect_same("%s: bias gradient (misaligned)" % ctx, o["gw_mis_b"], o["gw_b"])
        if ok("gw") and ok("gw_acc") and not t[11]:
            _expect_same("%s: accumulated weight gradient" % ctx, o["gw_acc"], o["gw"] + D.gw0)
        if ok("gw") and ok("gw_mis") and not t[11]:
            _expect_same("%s: weight gradient (misaligned)" % ctx, o["gw_mis"], o["gw"])


def _images(N):
    return sorted({0, N // 2, N - 1})


def _check_act(t, D, o, err, pre, ctx):
    """activation outputs against float64 act(pre-activation): ReLU bit for bit, ELU / sigmoid / tanh within 4 ulp + 2^-22 on the
    first, a middle and the last image"""
    act = t[10]
    for key, b in (("y", None), ("y_ready", None), ("y_batch", None), ("y_mis", None), ("y_bias", D.bias)):
        if key not in o or err.get(key) is not None:
            continue
        p = pre if b is None else pre + b.view(1, -1, 1, 1)
        if act == 1:
            _expect_same("%s: %s vs relu(pre)" % (ctx, key), o[key], torch.relu(p))
            continue
        idx = _images(t[0])
        ref = _act64(p[idx].cpu().to(F64), act)
        got = o[key][idx].cpu().to(F64)
        bound = 4 * 2.0 ** -24 * ref.abs() + 2.0 ** -22
        bad = (got - ref).abs() > bound
        assert not bad.any(), "%s: %s %s: %d elements off; worst |err| %.3g" % (ctx, key, ACT_NAMES[act], int(bad.sum()),
                                                                               float((got - ref).abs().max()))


def _check_in_norm(t, D, o, err, ctx):
    """in_norm stems against float64 (x - 0.45) / 0.225 on the in-bounds taps: |err| <= 2^-18 * conv(|x_hat|, |w|) (an fp32 sum of
    at most 7*7*7 products, each rounded, plus the normalisation's own rounding) + 2^-22"""
    xh = (D.xc - 0.45) / 0.225
    if err.get("y") is None:
        idx = _images(t[0])
        ref = _ref_fwd(xh[idx], D.wc, t)
        scale = _ref_fwd(xh[idx].abs(), D.wc.abs(), t)
        if t[10]:
            ref = _act64(ref, t[10])
        for key in ("y", "y_ready", "y_batch", "y_mis"):
            if key in o and err.get(key) is None:
                e = (o[key][idx].cpu().to(F64) - ref).abs()
                assert bool((e <= 2.0 ** -18 * scale + 2.0 ** -22).all()), "%s: %s in_norm forward |err| %.3g" % (ctx, key, float(e.max()))
    if err.get("gw") is None:
        ref = _ref_wgrad(D.gyc, xh, t)
        scale = _ref_wgrad(D.gyc.abs(), xh.abs(), t)
        for key in ("gw", "gw_mis"):
            if err.get(key) is None:
                e = (o[key].cpu().to(F64) - ref).abs()
                assert bool((e <= 2.0 ** -18 * scale + 2.0 ** -22).all()), "%s: %s in_norm weight gradient |err| %.3g" % (ctx, key, float(e.max()))
        e = (o["gw_acc"].cpu().to(F64) - ref - D.gw0.cpu().to(F64)).abs()
        assert bool((e <= 2.0 ** -18 * (scale + 2) + 2.0 ** -22).all()), "%s: accumulated in_norm weight gradient" % ctx


def _proj(r, a):
    """sum_c r[v, c] * a[n, c, ...] in float64 on the device of a (integers: exact in any order) -> CPU [N, V, ...]"""
    return torch.einsum("vc,nc...->nv...", r.to(a.device), a.to(F64)).cpu()


def _check_float64(t, D, pre, o, err, checks):
    """the exact results of the default run against float64: projections of every element, element-wise where cheap"""
    N, Cin, H, W, Cout, K = t[:6]
    Ho, Wo = _out_hw(t)
    if pre is not None:
        want = _ref_fwd(D.xc, torch.einsum("vo,oikl->vikl", D.r, D.wc), t)
        got = _proj(D.r, pre)
        assert torch.equal(got, want), "forward: projection differs from float64 at %d of %d positions" % (int((got != want).sum()), got.numel())
        checks.append("fwd")
        if N * Ho * Wo * Cin * Cout * K * K <= FULL_MACS:
            assert torch.equal(pre.cpu().to(F64), _ref_fwd(D.xc, D.wc, t)), "forward differs from float64 element-wise"
            checks.append("fwd full")
    if err.get("gx") is None:
        want = _ref_dgrad(D.gyc, torch.einsum("vi,oikl->ovkl", D.s, D.wc), t)
        got = _proj(D.s, o["gx"])
        assert torch.equal(got, want), "data gradient: projection differs from float64 at %d of %d positions" % (int((got != want).sum()), got.numel())
        checks.append("dgrad")
        if N * Ho * Wo * Cin * Cout * K * K <= FULL_MACS:
            assert torch.equal(o["gx"].cpu().to(F64), _ref_dgrad(D.gyc, D.wc, t)), "data gradient differs from float64 element-wise"
            checks.append("dgrad full")
    if err.get("gw") is None and not t[11]:
        gy_r = torch.einsum("vo,no...->nv...", D.r, D.gyc)
        x_s = torch.einsum("vi,ni...->nv...", D.s, D.xc)
        want = torch.stack([_ref_wgrad(gy_r[:, v:v + 1], x_s[:, v:v + 1], t)[0, 0] for v in range(2)])
        got = torch.einsum("vo,oikl,vi->vkl", D.r.cuda(), o["gw"].to(F64), D.s.cuda()).cpu()
        assert torch.equal(got, want), "weight gradient: r^T gw s differs from float64: %s vs %s" % (got.tolist(), want.tolist())
        checks.append("wgrad")
        if N * Ho * Wo * Cin * Cout * K * K <= FULL_MACS:
            assert torch.equal(o["gw"].cpu().to(F64), _ref_wgrad(D.gyc, D.xc, t)), "weight gradient differs from float64 element-wise"
            checks.append("wgrad full")
    if err.get("gw") is None:
        assert torch.equal(o["gw_b"].cpu().to(F64), D.gyc.sum((0, 2, 3))), "bias gradient differs from float64"
        checks.append("bias grad")
    if err.get("y_stats") is None and "y_stats_part" in o:
        part = o["y_stats_part"].to(F64)
        y64 = o["y_stats"].to(F64).flatten(2)
        S = part.shape[2]
        assert torch.equal(part[..., 0].sum(2), y64.sum(2)), "statistics: slot sums differ from float64"
        if (Ho * Wo) % S == 0:
            n = Ho * Wo // S
            mean_s = part[..., 0] / n
            mean = y64.mean(2, keepdim=True)
            m2 = part[..., 1].sum(2) + (n * (mean_s - mean) ** 2).sum(2)
            m2_ref = ((y64 - mean) ** 2).sum(2)
            tol = 1e-5 * m2_ref + 1e-5 * (y64.abs().amax(2) ** 2) + 1e-6
            assert bool(((m2 - m2_ref).abs() <= tol).all()), "statistics: M2 off by %.3g" % float((m2 - m2_ref).abs().max())
        checks.append("stats")


# ---------------------------------------------------------------------------------------------------------------- the tests
FAMILIES = {"fwd": set(), "dgrad": set(), "wgrad": set()}
RAN = set()
TOTALS = {"checks": 0, "runs": 0, "calls": 0}
_LOG = re.compile(r"^FDCONV (fwd|dgrad|wgrad) (.+?) N=(\d+) Cin=(\d+) H=(\d+) W=(\d+) Cout=(\d+) K=(\d+) s=(\d+) pad_mode=(\d+)$", re.M)


def _families(text, t):
    """{direction: family} that fd_tuning.log named first for descriptor t (the aligned call with no bias); every name is recorded"""
    out = {}
    for m in _LOG.finditer(text):
        key = tuple(int(v) for v in m.groups()[2:])
        if key == (t[0], t[1], t[2], t[3], t[4], t[5], t[7], t[9]):
            FAMILIES[m.group(1)].add(m.group(2))
            if m.group(2) != "c1 stencil * act'(input)" and m.group(1) not in out:
                out[m.group(1)] = m.group(2)
    return out


@pytest.fixture(scope="module", autouse=True)
def _log_on():
    prev = tuning.set_lib(log=1)
    t0 = time.time()
    yield
    tuning.set_lib(**prev)
    import conftest
    conftest.report("conv exact: wall seconds of the module", time.time() - t0, 120, "(%d case runs, %d entry-point calls, %d float64 "
                    "comparisons)" % (TOTALS["runs"], TOTALS["calls"], TOTALS["checks"]))


def test_case_list_matches_route_table():
    assert np.array_equal(np.array(DESCS, np.int32), _Z["desc"]) and N_NETWORK == 197 and len(DESCS) == 617
    assert sum(len(_row_settings(ci)) for ci in range(len(DESCS))) == 1078


@pytest.mark.parametrize("ci", range(len(DESCS)), ids=_case_id)
def test_conv_exact(ci, capfd):
    t = DESCS[ci]
    D = _Data(ci, t)
    bud = D.budget(t)
    assert max(bud.values()) < LIMIT, "exactness budget exceeded: %s" % bud
    ctx = "%s default" % _case_id(ci)
    capfd.readouterr()
    o, err = _run(t, D)
    fams = _families(capfd.readouterr().err, t)
    _check_errors(t, err, ctx)
    _check_internal(t, D, o, err, ctx)
    pre = None
    if t[10] != 0 and err.get("y") is None:
        # the pre-activation: the same convolution without activation, checked exact below
        tp = t[:10] + (0,) + t[11:]
        op, ep = _run(tp, D, "f")
        capfd.readouterr()
        _check_errors(tp, ep, ctx + " (no activation)")
        _check_internal(tp, D, op, ep, ctx + " (no activation)")
        pre = op["y"] if ep["y"] is None else None
        if not t[11] and pre is not None:
            _check_act(t, D, o, err, pre, ctx)
    elif t[10] == 0 and not t[11] and err.get("y") is None:
        pre = o["y"]
    checks = []
    _check_float64(t, D, pre if not t[11] else None, o, err, checks)
    if t[11]:
        _check_in_norm(t, D, o, err, ctx)
        checks.append("in_norm")
    TOTALS["checks"] += len(checks)
    TOTALS["runs"] += 1
    TOTALS["calls"] += sum(1 for e in err.values() if e is None)
    base = {k: o[k] for k in _exact_keys(t) if k in o and err.get(k[:-2] if k.endswith("_b") else k) is None}
    # every setting whose route-table row differs, and the row-neutral settings where the default family is theirs
    todo = [(s, "fdw") for s in _row_settings(ci)] + _log_only_settings(t, fams)
    for setting, dirs in todo:
        sctx = "%s %s" % (_case_id(ci), setting)
        with tuning.override(**_kw(setting)):
            os_, es = _run(t, D, dirs, full=False)
        _families(capfd.readouterr().err, t)
        _check_errors(t, es, sctx)
        _check_internal(t, D, os_, es, sctx)
        for k, v in base.items():
            if k in os_ and es.get(k[:-2] if k.endswith("_b") else k) is None:
                _expect_same("%s: %s vs the default" % (sctx, k), os_[k], v)
        if t[10] not in (0, 1) and pre is not None and not t[11] and "f" in dirs:
            _check_act(t, D, os_, es, pre, sctx)
        if t[11]:
            _check_in_norm(t, D, os_, es, sctx)
        TOTALS["runs"] += 1
        TOTALS["calls"] += sum(1 for e in es.values() if e is None)
    RAN.add(ci)


def _route_names():
    """every family name route_fwd / route_dgrad / route_wgrad (csrc/conv.hip) can print"""
    src = open(os.path.join(ROOT, "fusiondepth_amd", "csrc", "conv.hip")).read()
    body = lambda a, b: src[src.index(a):src.index(b)]
    names = lambda text: set(re.findall(r'r\.set\([^;"]*"([^"]+)"\)', text))
    return {"fwd": names(body("Route route_fwd(", "Route route_dgrad(")),
            "dgrad": names(body("Route route_dgrad(", "Route route_wgrad(")),
            "wgrad": names(body("Route route_wgrad(", "// The stand-alone"))}


def test_every_route_family_is_reached():
    """the cases above reach every family each route_* can print - a threshold change that orphans one shows up here"""
    if len(RAN) != len(DESCS):
        pytest.skip("needs the whole case list in this session (ran %d of %d cases)" % (len(RAN), len(DESCS)))
    names = _route_names()
    assert all(len(v) >= 5 for v in names.values()), names
    for direction, want in names.items():
        missing = want - FAMILIES[direction]
        assert not missing, "%s families never reached: %s (reached: %s)" % (direction, sorted(missing), sorted(FAMILIES[direction]))


def test_conv2d_stats_of_a_misaligned_view():
    """functional.conv2d_stats on a view 4 bytes past a 16-byte boundary (a shape whose statistics epilogue needs an aligned input,
    ResNet layer2 at 640x192: 480 tiles per image): the same y bit for bit, and statistics that batch_norm can use"""
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randint(-2, 3, (2, 128, 24, 80), generator=g, device="cuda").float()
    w = torch.randint(-2, 3, (128, 128, 3, 3), generator=g, device="cuda").float()
    xm = _misaligned(x)
    assert xm.data_ptr() % 16 == 4
    y, part = FD.conv2d_stats(x, w, None, 1, 1)
    ym, partm = FD.conv2d_stats(xm, w, None, 1, 1)
    torch.cuda.synchronize()
    _expect_same("conv2d_stats(misaligned view)", ym, y)
    if partm is not None:
        _expect_same("conv2d_stats(misaligned view) statistics", partm, part)
