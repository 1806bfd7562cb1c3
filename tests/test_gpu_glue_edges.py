"""The memory-bound glue kernels of csrc/geometry.hip and csrc/pool.hip at their launch edges (one element, a ragged last block, exactly
one block, one element into the next block, past every block cap and into the grid-stride loops), and the stand-alone loss-map kernels
(bilinear resize and its adjoint, SSIM, the reprojection map, smoothness, the combination of the loss terms) at their tile seams, reflect
folds, window branches and fractional ratios, against the float64 references of tests/glue_ref.py.

Copies and selections must be exact.  Everything else is held, per output tensor, to ``rel_err <= max(4 x yardstick, 1e-6)``, where the
yardstick is the float32 CPU oracle's own rel_err against the same float64 reference on the same inputs, computed here on the CPU - and
never looser than what the older test of the same quantity allows.  Adam is held to the project's 1e-4 of scale.  Outputs written
through raw pointers sit in sentinel-filled buffers, 64 floats in, and the sentinel must survive on both sides."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import glue_ref as R
from conftest import report

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SENTINEL = -7.25e9
PAD_BYTES = 256                   # 64 floats: the alignment of the output is that of the buffer


@pytest.fixture(scope="module")
def FD():
    from fusiondepth_amd import functional
    return functional


@pytest.fixture(scope="module")
def L():
    from fusiondepth_amd import _lib
    _lib.load()
    return _lib


def dev(t):
    return t.detach().to(F32).contiguous().cuda()


class Band:
    """``numel`` elements inside a sentinel-filled device buffer; ``.t`` is the tensor to hand out, ``.intact()`` the check."""

    def __init__(self, numel, dtype=F32, fill=None):
        self.pad = PAD_BYTES // torch.empty((), dtype=dtype).element_size()
        self.sentinel = SENTINEL if dtype == F32 else 0xA5
        self.buf = torch.full((2 * self.pad + numel,), self.sentinel, dtype=dtype, device="cuda")
        assert self.buf.data_ptr() % PAD_BYTES == 0
        self.t = self.buf[self.pad:self.pad + numel]
        if fill is not None:
            self.t.fill_(fill)

    def intact(self):
        return bool((self.buf[:self.pad] == self.sentinel).all()) and bool((self.buf[self.pad + self.t.numel():] == self.sentinel).all())

    def untouched(self):
        return bool((self.buf == self.sentinel).all())


def offset_view(t):
    """The same values as a contiguous view one float into a larger buffer: 4 mod 16 bytes."""
    buf = torch.empty(t.numel() + 1, device="cuda", dtype=F32)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def cap_of(rtol, atol, ref):
    """What a per-element test ``|d| <= atol + rtol |ref|`` allows at most, as a fraction of the tensor's scale."""
    return rtol + atol / max(float(ref.abs().max()), R.TINY)


class Checks:
    """Reports every measured error, then fails once with all of them that are out of bound."""

    def __init__(self, what):
        self.what, self.bad = what, []

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            assert not self.bad, "; ".join(self.bad)

    def close(self, name, got, ref, ora, cap=None):
        y = R.rel_err(ora, ref)
        b = R.bound(y, cap)
        e = R.rel_err(got, ref)
        report("%s %s" % (self.what, name), e, b, "(yardstick %.2e)" % y)
        if not (math.isfinite(e) and e <= b):
            self.bad.append("%s %s: %.3g of scale from float64, bound %.3g (float32 oracle: %.3g)" % (self.what, name, e, b, y))

    def fixed(self, name, got, ref, b):
        e = R.rel_err(got, ref)
        report("%s %s" % (self.what, name), e, b, "(fixed bound)")
        if not (math.isfinite(e) and e <= b):
            self.bad.append("%s %s: %.3g of scale from float64, bound %.3g" % (self.what, name, e, b))

    def exact(self, name, got, want):
        if not R.same_values(got.to(F32), want.to(F32)):
            g, w = got.detach().cpu().to(F32), want.detach().cpu().to(F32)
            n = int((~((g == w) | (torch.isnan(g) & torch.isnan(w)))).sum()) if g.shape == w.shape else -1
            self.bad.append("%s %s: %d of %d values differ (must be exact)" % (self.what, name, n, w.numel()))

    def guard(self, name, *bands):
        for i, bd in enumerate(bands):
            if not bd.intact():
                self.bad.append("%s %s: guard band %d overwritten" % (self.what, name, i))


# ================================================================================================ geometry.hip
@pytest.mark.parametrize("n", R.D2D_N)
def test_disp_to_depth(L, n):
    inp = R.d2d_inputs(n)
    disp, gs, gd = dev(inp["disp"]), dev(inp["g_scaled"]), dev(inp["g_depth"])
    ref, ora = R.d2d_ref(inp, F64), R.d2d_ref(inp, F32)
    with Checks("disp_to_depth n=%d" % n) as c:
        for want_s, want_d in ((True, True), (True, False), (False, True)):
            s, d = Band(n), Band(n)
            L.call("fd_disp_to_depth_fwd", L.ptr(disp), L.ptr(s.t) if want_s else None, L.ptr(d.t) if want_d else None, n, R.MIN_DEPTH, R.MAX_DEPTH, L.stream())
            c.guard("fwd", s, d)
            if want_s:
                c.close("scaled", s.t, ref["scaled"], ora["scaled"], cap=1e-6)
            else:
                assert s.untouched()
            if want_d:
                c.close("depth", d.t, ref["depth"], ora["depth"], cap=1e-6)
            else:
                assert d.untouched()
        for use_gs, use_gd in ((True, True), (True, False), (False, True), (False, False)):
            r, o = R.d2d_ref(inp, F64, use_gs, use_gd), R.d2d_ref(inp, F32, use_gs, use_gd)
            out = Band(n)
            L.call("fd_disp_to_depth_bwd", L.ptr(disp), L.ptr(gs) if use_gs else None, L.ptr(gd) if use_gd else None, L.ptr(out.t), n,
                   R.MIN_DEPTH, R.MAX_DEPTH, L.stream())
            c.guard("bwd", out)
            if use_gs or use_gd:
                c.close("d_disp gs=%d gd=%d" % (use_gs, use_gd), out.t, r["d_disp"], o["d_disp"], cap=cap_of(1e-5, 1e-6 * float(r["d_disp"].abs().max()), r["d_disp"]))
            else:
                assert not out.t.any(), "no incoming gradient: zeros"


def _pose_caps(ref):
    return {"T": cap_of(1e-5, 1e-7, ref["T"]), "g_aa": cap_of(1e-4, 1e-5, ref["g_aa"]), "g_tr": cap_of(1e-4, 1e-6, ref["g_tr"])}


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("B", R.POSE_B)
def test_pose_matrix(L, B, invert):
    inp = R.pose_inputs(B)
    ref, ora = R.pose_ref(inp, F64, invert), R.pose_ref(inp, F32, invert)
    aa, tr, cot = dev(inp["aa"].view(B, 3)), dev(inp["tr"].view(B, 3)), dev(inp["cot"])
    T, g_aa, g_tr = Band(B * 16), Band(B * 3), Band(B * 3)
    L.call("fd_pose_matrix_fwd", L.ptr(aa), L.ptr(tr), L.ptr(T.t), B, int(invert), L.stream())
    L.call("fd_pose_matrix_bwd", L.ptr(aa), L.ptr(tr), L.ptr(cot), L.ptr(g_aa.t), L.ptr(g_tr.t), B, int(invert), L.stream())
    caps = _pose_caps(ref)
    with Checks("pose_matrix B=%d invert=%d" % (B, invert)) as c:
        c.guard("outputs", T, g_aa, g_tr)
        for k, got in (("T", T.t.view(B, 4, 4)), ("g_aa", g_aa.t.view(B, 1, 3)), ("g_tr", g_tr.t.view(B, 1, 3))):
            assert bool(torch.isfinite(got).all()), "%s is not finite everywhere" % k
            c.close(k, got, ref[k], ora[k], cap=caps[k])


def test_pose_matrix_through_the_wrapper(FD):
    """The autograd wrapper hands the same buffers to the same kernels: equal to the float64 reference under the same bounds."""
    B, invert = 65, True
    inp = R.pose_inputs(B)
    ref, ora = R.pose_ref(inp, F64, invert), R.pose_ref(inp, F32, invert)
    aa, tr = dev(inp["aa"]).requires_grad_(True), dev(inp["tr"]).requires_grad_(True)
    T = FD.transformation_from_parameters(aa, tr, invert=invert)
    g_aa, g_tr = torch.autograd.grad(T, [aa, tr], dev(inp["cot"]))
    caps = _pose_caps(ref)
    with Checks("pose_matrix wrapper B=65") as c:
        for k, got in (("T", T), ("g_aa", g_aa), ("g_tr", g_tr)):
            c.close(k, got, ref[k], ora[k], cap=caps[k])


def test_pose_head_across_the_block_boundary(FD):
    G, nf, Bq, npred = R.POSE_HEAD
    inp = R.pose_head_inputs()
    ref, ora = R.pose_head_ref(inp, F64), R.pose_head_ref(inp, F32)
    pose = dev(inp["pose"]).requires_grad_(True)
    heads = FD.pose_head(pose, G, nf, Bq, inp["inverts"])
    (g,) = torch.autograd.grad([h[0] for h in heads], pose, [dev(ct) for ct in inp["cots"]])
    with Checks("pose_head %d threads" % (G * nf * Bq)) as c:
        for k in range(nf):
            c.close("T%d" % k, heads[k][0], ref["T%d" % k], ora["T%d" % k], cap=cap_of(1e-5, 1e-7, ref["T%d" % k]))
            rows = torch.cat([inp["pose"][(q * nf + k) * Bq:(q * nf + k + 1) * Bq] for q in range(G)], 0).view(G * Bq, npred, 1, 6)
            c.exact("axisangle %d" % k, heads[k][1], rows[..., :3])
            c.exact("translation %d" % k, heads[k][2], rows[..., 3:])
        c.close("g_pose", g, ref["g_pose"], ora["g_pose"], cap=cap_of(1e-4, 1e-5, ref["g_pose"]))
        assert not g[:, 6:].any(), "predictions the loss never uses take no gradient"


@pytest.mark.parametrize("stride", R.PROJMAT_STRIDES)
@pytest.mark.parametrize("B", R.PROJMAT_B)
def test_proj_matrix(L, B, stride):
    inp = R.projmat_inputs(B)
    ref, ora = R.projmat_ref(inp, F64), R.projmat_ref(inp, F32)
    K, T = dev(inp["K"]), dev(inp["T"])
    n = (B - 1) * stride + 12
    slot = (torch.arange(B)[:, None] * stride + torch.arange(12)[None, :]).reshape(-1).cuda()
    hole = torch.ones(n, dtype=torch.bool, device="cuda")
    hole[slot] = False
    P = Band(n)
    L.call("fd_proj_matrix_fwd", L.ptr(K), L.ptr(T), L.ptr(P.t), stride, B, L.stream())
    gP = torch.full((n,), float("nan"), device="cuda")             # a read from a gap poisons the result
    gP[slot] = dev(inp["gP"]).reshape(-1)
    gT = Band(B * 16)
    L.call("fd_proj_matrix_bwd", L.ptr(K), L.ptr(gP), stride, L.ptr(gT.t), B, L.stream())
    with Checks("proj_matrix B=%d stride=%d" % (B, stride)) as c:
        c.guard("outputs", P, gT)
        assert bool((P.t[hole] == SENTINEL).all()), "the gaps between the items' 12 floats were written"
        c.close("P", P.t[slot].view(B, 3, 4), ref["P"], ora["P"])
        c.close("gT", gT.t.view(B, 4, 4), ref["gT"], ora["gT"])


@pytest.mark.parametrize("B,H,W", R.BACKPROJECT_SHAPES)
def test_backproject_and_cat_xy(L, B, H, W):
    inp = R.backproject_inputs(B, H, W)
    ref, ora = R.backproject_ref(inp, F64), R.backproject_ref(inp, F32)
    depth, inv_K, cot = dev(inp["depth"]), dev(inp["inv_K"]), dev(inp["cot"])
    pts, gd, cat = Band(B * 4 * H * W), Band(B * H * W), Band(B * 3 * H * W)
    L.call("fd_backproject_fwd", L.ptr(depth), L.ptr(inv_K), L.ptr(pts.t), B, H, W, L.stream())
    L.call("fd_backproject_bwd", L.ptr(cot), L.ptr(inv_K), L.ptr(gd.t), B, H, W, L.stream())
    L.call("fd_cat_xy_fwd", L.ptr(depth), L.ptr(inv_K), L.ptr(cat.t), B, H, W, L.stream())
    with Checks("backproject %dx%dx%d" % (B, H, W)) as c:
        c.guard("outputs", pts, gd, cat)
        c.close("points", pts.t.view(B, 4, H * W), ref["points"], ora["points"], cap=cap_of(1e-5, 1e-6, ref["points"]))
        c.exact("points w", pts.t.view(B, 4, H * W)[:, 3], torch.ones(B, H * W))
        c.close("g_depth", gd.t.view(B, 1, H, W), ref["g_depth"], ora["g_depth"], cap=cap_of(1e-4, 1e-5, ref["g_depth"]))
        c.close("cat_xy", cat.t.view(B, 3, H, W), ref["cat_xy"], ora["cat_xy"], cap=cap_of(1e-5, 1e-6, ref["cat_xy"]))


@pytest.mark.parametrize("B,H,W", R.PROJECT_SHAPES)
def test_project3d(L, B, H, W):
    inp = R.project_inputs(B, H, W)
    ref, ora = R.project_ref(inp, F64), R.project_ref(inp, F32)
    pts, K, T, cot = dev(inp["points"]), dev(inp["K"]), dev(inp["T"]), dev(inp["cot"])
    n_ws = L.query("fd_project3d_bwd_ws_floats", B, H, W)
    assert n_ws == B * 12 * min(256, max(1, -(-H * W // 1024)))
    grid, gp, gT = Band(B * H * W * 2), Band(B * 4 * H * W), Band(B * 16)
    ws = Band(n_ws, fill=float("nan"))
    L.call("fd_project3d_fwd", L.ptr(pts), L.ptr(K), L.ptr(T), L.ptr(grid.t), B, H, W, 1e-7, L.stream())
    L.call("fd_project3d_bwd", L.ptr(pts), L.ptr(K), L.ptr(T), L.ptr(cot), L.ptr(gp.t), L.ptr(gT.t), L.ptr(ws.t), B, H, W, 1e-7, L.stream())
    with Checks("project3d %dx%dx%d" % (B, H, W)) as c:
        c.guard("outputs and workspace", grid, gp, gT, ws)
        assert bool(torch.isfinite(ws.t).all()), "the launcher uses less workspace than fd_project3d_bwd_ws_floats reports"
        c.close("grid", grid.t.view(B, H, W, 2), ref["grid"], ora["grid"], cap=cap_of(1e-4, 1e-5, ref["grid"]))
        c.close("g_points", gp.t.view(B, 4, H * W), ref["g_points"], ora["g_points"], cap=cap_of(1e-4, 1e-5, ref["g_points"]))
        c.close("gT", gT.t.view(B, 4, 4), ref["gT"], ora["gT"], cap=cap_of(1e-4, 1e-3, ref["gT"]))


# ================================================================================================ pool.hip
@pytest.mark.parametrize("N,C,H,W", R.MAXPOOL_SHAPES)
def test_maxpool(FD, L, N, C, H, W):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    with Checks("maxpool %dx%dx%dx%d" % (N, C, H, W)) as c:
        for kind in R.MAXPOOL_KINDS:
            inp = R.maxpool_inputs(N, C, H, W, kind)
            ref, ora = R.maxpool_ref(inp, F64), R.maxpool_ref(inp, F32)
            x, cot = dev(inp["x"]), dev(inp["cot"])
            y, idx, gx = Band(N * C * Ho * Wo), Band(N * C * Ho * Wo, torch.uint8), Band(N * C * H * W)
            L.call("fd_maxpool3x3s2_fwd", L.ptr(x), L.ptr(y.t), L.ptr(idx.t), N, C, H, W, L.stream())
            L.call("fd_maxpool3x3s2_bwd", L.ptr(cot), L.ptr(idx.t), L.ptr(gx.t), N, C, H, W, L.stream())
            c.guard(kind, y, idx, gx)
            c.exact("%s forward" % kind, y.t.view(N, C, Ho, Wo), ora["y"])
            assert bool((idx.t < 9).all()), "%s: a window without a winning tap" % kind
            c.close("%s gx" % kind, gx.t.view(N, C, H, W), ref["gx"], ora["gx"], cap=2e-6)
            c.exact("%s gradient routing" % kind, gx.t.view(N, C, H, W) != 0, ref["gx"] != 0)
        xg = dev(inp["x"]).requires_grad_(True)                      # the autograd wrapper, on the last kind
        yg = FD.max_pool3x3s2(xg)
        (gg,) = torch.autograd.grad(yg, xg, cot)
        c.exact("wrapper forward", yg, y.t.view(N, C, Ho, Wo))
        c.exact("wrapper backward", gg, gx.t.view(N, C, H, W))


def _upcat_raw(L, inp, combo, h, w):
    """fd_upcat_fwd / fd_upcat_bwd through raw pointers, every output in a guard band."""
    use_skip, use_add, use_extra = combo
    N, Ca, Cs, C3 = inp["dims"]
    Cs, C3 = Cs * use_skip, C3 * use_extra
    a, s1, s2, s3 = dev(inp["a"]), dev(inp["skip"]) if use_skip else None, dev(inp["skip_add"]) if use_add else None, dev(inp["extra"]) if use_extra else None
    plane = 4 * h * w
    out = Band(N * (Ca + Cs + C3) * plane)
    L.call("fd_upcat_fwd", L.ptr(a), L.ptr(s1), L.ptr(s2), L.ptr(s3), L.ptr(out.t), N, Ca, Cs, C3, h, w, L.stream())
    return out, (N, Ca, Cs, C3, plane)


@pytest.mark.parametrize("combo", R.UPCAT_COMBOS, ids=lambda c: "skip%d_add%d_extra%d" % c)
@pytest.mark.parametrize("h,w", R.UPCAT_HW)
def test_upsample_concat(L, h, w, combo):
    inp = R.upcat_inputs(h, w)
    ref, ora = R.upcat_ref(inp, F64, combo), R.upcat_ref(inp, F32, combo)
    out, (N, Ca, Cs, C3, plane) = _upcat_raw(L, inp, combo, h, w)
    gout = dev(ref["cot"])
    ga, gs, g3 = Band(N * Ca * h * w), Band(N * Cs * plane), Band(N * C3 * plane)
    L.call("fd_upcat_bwd", L.ptr(gout), L.ptr(ga.t), L.ptr(gs.t) if Cs else None, L.ptr(g3.t) if C3 else None, N, Ca, Cs, C3, h, w, L.stream())
    with Checks("upcat %dx%d skip/add/extra=%d%d%d" % ((h, w) + combo)) as c:
        c.guard("outputs", out, ga, gs, g3)
        c.exact("forward", out.t.view(ora["y"].shape), ora["y"])
        c.close("g_a", ga.t.view(N, Ca, h, w), ref["g_a"], ora["g_a"], cap=2e-6)
        if Cs:
            c.exact("g_skip", gs.t.view(ora["g_skip"].shape), ora["g_skip"])
        if C3:
            c.exact("g_extra", g3.t.view(ora["g_extra"].shape), ora["g_extra"])


def _upcat_api(FD, inp, combo, act, wrap=lambda name, t: t):
    """upsample_concat and its gradients through the autograd wrapper; ``wrap(name, tensor)`` may re-home an operand."""
    use_skip, use_add, use_extra = combo
    ts = {k: wrap(k, dev(inp[k])).requires_grad_(True) for k in ("a", "skip", "skip_add", "extra")}
    y = FD.upsample_concat(ts["a"], ts["skip"] if use_skip else None, ts["skip_add"] if use_add else None, ts["extra"] if use_extra else None, a_act=act)
    names = ["a"] + ["skip"] * use_skip + ["skip_add"] * use_add + ["extra"] * use_extra
    N, Ca, Cs, C3 = inp["dims"]
    cot = torch.cat([inp["cot"][:, :Ca]] + [inp["cot"][:, Ca:Ca + Cs]] * use_skip + [inp["cot"][:, Ca + Cs:]] * use_extra, 1)
    grads = torch.autograd.grad(y, [ts[k] for k in names], wrap("gout", dev(cot)))
    return y, dict(zip(names, grads))


@pytest.mark.parametrize("act", R.ACT_NAMES[1:])
@pytest.mark.parametrize("h,w", [(6, 8), (5, 7)], ids=["vector", "scalar"])
def test_upsample_concat_with_activation_gradient(FD, h, w, act):
    inp = R.upcat_inputs(h, w, act)
    combo = (1, 1, 1)
    ref, ora = R.upcat_ref(inp, F64, combo, act), R.upcat_ref(inp, F32, combo, act)
    y, g = _upcat_api(FD, inp, combo, act)
    with Checks("upcat a_act=%s %dx%d" % (act, h, w)) as c:
        c.exact("forward", y, ora["y"])
        c.close("g_a", g["a"], ref["g_a"], ora["g_a"], cap=2e-6 if act == "relu" else None)
        for k in ("skip", "skip_add", "extra"):
            c.exact("g_" + k, g[k], ora["g_" + k])


@pytest.mark.parametrize("which", ["a", "skip", "skip_add", "extra", "gout", "a_out"])
@pytest.mark.parametrize("h,w", [(6, 8), (3, 2)])
def test_upsample_concat_operand_off_alignment(FD, h, w, which):
    """An even width with one operand 4 bytes off 16-byte alignment (a contiguous view at a storage offset): the launcher must fall
    back to the scalar kernels, and the result is the aligned run's, bit for bit."""
    act = "elu" if which == "a_out" else "none"                     # a_out: `a` as saved for the backward pass (its 8-byte check)
    inp = R.upcat_inputs(h, w, act)
    target = "a" if which == "a_out" else which
    y0, g0 = _upcat_api(FD, inp, (1, 1, 1), act)
    y1, g1 = _upcat_api(FD, inp, (1, 1, 1), act, wrap=lambda name, t: offset_view(t) if name == target else t)
    ora = R.upcat_ref(inp, F32, (1, 1, 1), act)
    with Checks("upcat %dx%d, %s off alignment" % (h, w, which)) as c:
        c.exact("aligned forward", y0, ora["y"])
        c.exact("forward", y1, y0)
        for k in g0:
            c.exact("g_" + k, g1[k], g0[k])


@pytest.mark.parametrize("N,C,h,w", R.UP2_CASES)
def test_upsample_nearest2x(FD, N, C, h, w):
    inp = R.up2_inputs(N, C, h, w)
    ref, ora = R.up2_ref(inp, F64), R.up2_ref(inp, F32)
    x = dev(inp["x"]).requires_grad_(True)
    y = FD.upsample_nearest2x(x)
    (gx,) = torch.autograd.grad(y, x, dev(inp["cot"]))
    with Checks("upsample2x %dx%dx%dx%d" % (N, C, h, w)) as c:
        c.exact("forward", y, ora["y"])
        c.close("gx", gx, ref["gx"], ora["gx"], cap=2e-6)


@pytest.mark.parametrize("n", R.EW_N)
def test_act_bwd_axpby_input_normalize(L, n):
    inp = R.ew_inputs(n)
    a, b, img = dev(inp["a"]), dev(inp["b"]), dev(inp["img"])
    with Checks("elementwise n=%d" % n) as c:
        for act_id, act in enumerate(R.ACT_NAMES):
            yv = R.act_output_values(np.random.RandomState(n % 1000), (n,), act)
            out, yd = Band(n), dev(yv)
            L.call("fd_act_bwd", L.ptr(yd), L.ptr(b), L.ptr(out.t), n, act_id, L.stream())
            c.guard("act_bwd", out)
            c.close("act_bwd %s" % act, out.t, R.act_bwd_ref(yv, inp["b"], act, F64), R.act_bwd_ref(yv, inp["b"], act, F32))
        out = Band(n)
        L.call("fd_axpby", L.ptr(a), L.ptr(b), L.ptr(out.t), n, 0.7, -1.3, L.stream())
        c.guard("axpby", out)
        c.close("axpby", out.t, R.axpby_ref(inp["a"], inp["b"], 0.7, -1.3, F64), R.axpby_ref(inp["a"], inp["b"], 0.7, -1.3, F32))
        out = Band(n)
        L.call("fd_input_normalize", L.ptr(img), L.ptr(out.t), n, 0.45, 0.225, L.stream())
        c.guard("input_normalize", out)
        c.exact("input_normalize", out.t, R.input_normalize_f32(inp["img"]))


def test_stack_normalize_past_its_block_cap(FD):
    C, H, W = 3, 384, 1024                                          # 294912 float4s per image: 288 blocks of 1024 wanted, 256 launched
    rng = np.random.RandomState(5)
    pieces = [torch.from_numpy(rng.rand(1, C, H, W).astype(np.float32)) for _ in range(2)]
    got = FD.stack_normalize([(dev(pieces[0]), 0, 0), (dev(pieces[1]), 0, C)], 1, 2 * C)
    assert torch.equal(got.cpu(), R.input_normalize_f32(torch.cat(pieces, 1)))
    got = FD.stack_normalize([(dev(pieces[0]), 0, C), (dev(pieces[1]), 0, 0)], 1, 2 * C, normalize=False)
    assert torch.equal(got.cpu(), torch.cat(pieces[::-1], 1))


def test_stack_normalize_refuses_what_its_float4_kernel_cannot_take(L):
    def run(src, H, W, out):
        L.call("fd_stack_normalize", (ctypes.c_void_p * 1)(src), (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(0), 1, 1, 3, 3, H, W, L.ptr(out.t), 1, 0.45, 0.225, L.stream())

    src = torch.rand(3 * 8 * 8 + 4, device="cuda")
    out = Band(3 * 8 * 8)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        run(src.data_ptr(), 3, 5, out)                               # H * W % 4 != 0
    with pytest.raises(RuntimeError, match="bad piece"):
        run(src.data_ptr() + 4, 8, 8, out)                           # a piece 4 bytes off
    torch.cuda.synchronize()
    assert out.untouched(), "a refused call must launch nothing"
    run(src.data_ptr(), 8, 8, out)
    assert out.intact() and torch.equal(out.t.cpu(), R.input_normalize_f32(src[:192]))


@pytest.mark.parametrize("planes", R.MEAN_PLANES)
@pytest.mark.parametrize("plane_size", R.MEAN_PLANE_SIZES)
def test_spatial_mean(L, plane_size, planes):
    inp = R.mean_inputs(planes, plane_size)
    ref, ora = R.mean_ref(inp, F64), R.mean_ref(inp, F32)
    x, cot = dev(inp["x"]), dev(inp["cot"])
    m, gx = Band(planes), Band(planes * plane_size)
    L.call("fd_spatial_mean_fwd", L.ptr(x), L.ptr(m.t), planes, plane_size, inp["scale"], L.stream())
    L.call("fd_spatial_mean_bwd", L.ptr(cot), L.ptr(gx.t), planes, plane_size, inp["scale"], L.stream())
    with Checks("spatial_mean %d planes of %d" % (planes, plane_size)) as c:
        c.guard("outputs", m, gx)
        c.close("mean", m.t.view(ref["mean"].shape), ref["mean"], ora["mean"], cap=1.1e-5)
        c.close("gx", gx.t.view(ref["gx"].shape), ref["gx"], ora["gx"], cap=2e-6)


@pytest.mark.parametrize("n", R.DEPTH_ERR_N)
def test_depth_errors(L, n):
    inp = R.depth_err_inputs(n)
    (ref, counts), (ora, _) = R.depth_err_ref(inp, F64), R.depth_err_ref(inp, F32)
    out, ws = Band(7), Band(7 * 256)
    gt, pred = dev(inp["gt"]), dev(inp["pred"])
    L.call("fd_depth_errors", L.ptr(gt), L.ptr(pred), n, L.ptr(out.t), L.ptr(ws.t), L.stream())
    got = out.t.cpu()
    with Checks("depth_errors n=%d" % n) as c:
        c.guard("outputs and workspace", out, ws)
        for i, name in enumerate(("abs_rel", "sq_rel", "rmse", "rmse_log")):
            c.close(name, got[i], ref[i], ora[i], cap=1e-5)
        # counts below 2^24 are exact in float32, and so is their one division by n
        c.exact("a1 a2 a3", got[4:], torch.tensor(counts, dtype=F32) / torch.tensor(float(n), dtype=F32))


def _adam_state(sc):
    return torch.tensor([float(sc["step0"]), sc["lrs"][0]], device="cuda", dtype=F32)


@pytest.mark.parametrize("n", R.ADAM_N)
def test_adam_step_dev(L, n):
    b1, b2 = R.ADAM_BETAS
    with Checks("adam_step_dev n=%d" % n) as c:
        for name, sc in R.adam_scenarios(n).items():
            ref = R.adam_ref(sc)
            p, m, v = Band(n, fill=0.0), Band(n), Band(n)
            m.t.copy_(sc["m0"]); v.t.copy_(sc["v0"])
            state = _adam_state(sc)
            for i, (g, lr) in enumerate(zip(sc["grads"], sc["lrs"])):
                state[1] = lr                                         # what FlatAdam.scheduler_step writes between steps
                gd = dev(g)
                L.call("fd_adam_step_dev", L.ptr(p.t), L.ptr(gd), L.ptr(m.t), L.ptr(v.t), n, L.ptr(state), b1, b2, R.ADAM_EPS, sc["grad_scale"], L.stream())
                assert float(state[0]) == sc["step0"] + i + 1, "%s: the device step counter after %d calls" % (name, i + 1)
            c.guard(name, p, m, v)
            for k, got in (("p", p.t), ("exp_avg", m.t), ("exp_avg_sq", v.t)):
                c.fixed("%s: %s" % (name, k), got, ref[k], 1e-4)


def test_adam_step_dev_of_no_elements_still_counts_the_step(L):
    b1, b2 = R.ADAM_BETAS
    p, m, v = Band(4, fill=1.0), Band(4, fill=2.0), Band(4, fill=3.0)
    g = torch.ones(4, device="cuda")
    state = torch.tensor([7.0, R.ADAM_LR], device="cuda")
    L.call("fd_adam_step_dev", L.ptr(p.t), L.ptr(g), L.ptr(m.t), L.ptr(v.t), 0, L.ptr(state), b1, b2, R.ADAM_EPS, 1.0, L.stream())
    assert state.tolist() == [8.0, float(np.float32(R.ADAM_LR))]
    assert p.intact() and m.intact() and v.intact()
    assert bool((p.t == 1).all()) and bool((m.t == 2).all()) and bool((v.t == 3).all())


@pytest.mark.parametrize("n,tail", [(2, (1,)), (257, (10, 10)), (1048576 + 257, (10, 10))])
def test_flat_adam_against_torch_adam_in_float64(n, tail):
    """FlatAdam.step / scheduler_step / load_state_dict over a two-tensor dp.FlatParameters: what the trainer runs."""
    from fusiondepth_amd import dp, optim
    shapes = [(n - int(np.prod(tail)),), tail]
    sizes = [int(np.prod(s)) for s in shapes]
    with Checks("FlatAdam n=%d" % n) as c:
        for name, sc in R.adam_scenarios(n).items():
            ref, ref_opt = R.adam_torch(sc, F64, shapes)
            params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in shapes]
            flat = dp.FlatParameters(params)
            drop_at = next((i for i in range(1, len(sc["lrs"])) if sc["lrs"][i] != sc["lrs"][i - 1]), None)
            opt = optim.FlatAdam(flat, R.ADAM_LR, scheduler_step_size=1)
            if sc["step0"]:
                fresh, fresh_opt = R.adam_torch(dict(sc, grads=[], lrs=sc["lrs"][:1]), F64, shapes)      # the state before the scenario's steps
                st = fresh_opt.state_dict()
                st["param_groups"][0]["lr"] = R.ADAM_LR
                opt.load_state_dict(st)
                assert opt.step_count == sc["step0"] and float(opt.state[0]) == sc["step0"]
            for i, g in enumerate(sc["grads"]):
                if i == drop_at:
                    opt.scheduler_step()
                    assert float(opt.state[1]) == sc["lrs"][i], "StepLR's new learning rate must reach the device state"
                flat.flat_grad.copy_(g)
                opt.step(grad_scale=sc["grad_scale"])
            assert float(opt.state[0]) == sc["step0"] + len(sc["grads"]) == opt.step_count
            for k, got in (("p", flat.flat_param), ("exp_avg", opt.exp_avg), ("exp_avg_sq", opt.exp_avg_sq)):
                c.fixed("%s: %s" % (name, k), got, ref[k], 1e-4)
            for p, o, s in zip(params, flat.offsets, sizes):
                assert p.data_ptr() == flat.flat_param.data_ptr() + 4 * o and p.numel() == s


# ================================================================================================ the stand-alone loss-map kernels
# fd_bilinear_up_* (geometry.hip), fd_ssim_* and fd_reproj_loss_map (photometric.hip), fd_smooth_* and fd_combine_losses_* (smooth.hip).
# The caps are what tests/test_gpu_losspath.py allows for the same quantities against the float32 oracle.
@functools.lru_cache(maxsize=None)
def _bilinear_refs(case):
    inp = R.bilinear_inputs(*case)
    return inp, R.bilinear_ref(inp, F64), R.bilinear_ref(inp, F32)


def _case_name(case):
    return "%dx%dx%d -> %dx%d" % case


@pytest.mark.parametrize("case", R.BILINEAR_CASES, ids=_case_name)
def test_bilinear_forward(L, case):
    BC, Hin, Win, Hout, Wout = case
    inp, ref, ora = _bilinear_refs(case)
    x, y = dev(inp["x"]), Band(BC * Hout * Wout)
    L.call("fd_bilinear_up_fwd", L.ptr(x), L.ptr(y.t), BC, Hin, Win, Hout, Wout, L.stream())
    with Checks("bilinear " + _case_name(case)) as c:
        c.guard("forward", y)
        c.close("y", y.t.view(ref["y"].shape), ref["y"], ora["y"], cap=cap_of(1e-5, 1e-6, ref["y"]))
        if (Hin, Win) == (Hout, Wout):
            c.exact("y is a copy", y.t.view(ref["y"].shape), inp["x"])


@pytest.mark.parametrize("case", R.BILINEAR_CASES, ids=_case_name)
def test_bilinear_adjoint(L, case):
    """Every input pixel must collect from every output pixel that reads it, at integer and at fractional ratios alike."""
    BC, Hin, Win, Hout, Wout = case
    inp, ref, ora = _bilinear_refs(case)
    cot, gx = dev(inp["cot"]), Band(BC * Hin * Win)
    L.call("fd_bilinear_up_bwd", L.ptr(cot), L.ptr(gx.t), BC, Hin, Win, Hout, Wout, L.stream())
    with Checks("bilinear " + _case_name(case)) as c:
        c.guard("adjoint", gx)
        c.close("gx", gx.t.view(ref["gx"].shape), ref["gx"], ora["gx"], cap=cap_of(1e-4, 1e-5, ref["gx"]))
        if (Hin, Win) == (Hout, Wout):
            c.exact("gx is a copy", gx.t.view(ref["gx"].shape), inp["cot"])


def test_bilinear_through_the_wrapper_at_a_fractional_ratio(FD):
    case = R.BILINEAR_OFFSET_CASE
    BC, Hin, Win, Hout, Wout = case
    inp, ref, ora = _bilinear_refs(case)
    x = dev(inp["x"]).requires_grad_(True)
    y = FD.bilinear_upsample(x, (Hout, Wout))
    (gx,) = torch.autograd.grad(y, x, dev(inp["cot"]))
    with Checks("bilinear wrapper " + _case_name(case)) as c:
        c.close("y", y, ref["y"], ora["y"], cap=cap_of(1e-5, 1e-6, ref["y"]))
        c.close("gx", gx, ref["gx"], ora["gx"], cap=cap_of(1e-4, 1e-5, ref["gx"]))


def test_bilinear_operands_off_alignment(L):
    """Every operand one float off 16-byte alignment: bit for bit the aligned call's result."""
    case = R.BILINEAR_OFFSET_CASE
    BC, Hin, Win, Hout, Wout = case
    inp, _, _ = _bilinear_refs(case)
    x, cot = dev(inp["x"]), dev(inp["cot"])
    y0, g0 = Band(BC * Hout * Wout), Band(BC * Hin * Win)
    L.call("fd_bilinear_up_fwd", L.ptr(x), L.ptr(y0.t), BC, Hin, Win, Hout, Wout, L.stream())
    L.call("fd_bilinear_up_bwd", L.ptr(cot), L.ptr(g0.t), BC, Hin, Win, Hout, Wout, L.stream())
    y1, g1 = Band(BC * Hout * Wout + 1), Band(BC * Hin * Win + 1)
    assert y1.t[1:].data_ptr() % 16 == 4 and g1.t[1:].data_ptr() % 16 == 4
    x1, cot1 = offset_view(x), offset_view(cot)
    L.call("fd_bilinear_up_fwd", L.ptr(x1), y1.t[1:].data_ptr(), BC, Hin, Win, Hout, Wout, L.stream())
    L.call("fd_bilinear_up_bwd", L.ptr(cot1), g1.t[1:].data_ptr(), BC, Hin, Win, Hout, Wout, L.stream())
    with Checks("bilinear off alignment " + _case_name(case)) as c:
        c.guard("outputs", y0, g0, y1, g1)
        assert bool((y1.t[:1] == SENTINEL).all()) and bool((g1.t[:1] == SENTINEL).all()), "the float before an output was written"
        c.exact("y", y1.t[1:], y0.t)
        c.exact("gx", g1.t[1:], g0.t)


def test_bilinear_refuses_what_it_cannot_take(L):
    gy, gx = torch.rand(2 * 6 * 6, device="cuda"), Band(2 * 6 * 6)
    with pytest.raises(RuntimeError, match="only upsampling"):
        L.call("fd_bilinear_up_bwd", L.ptr(gy), L.ptr(gx.t), 2, 6, 6, 5, 6, L.stream())           # Hout < Hin
    with pytest.raises(RuntimeError, match="only upsampling"):
        L.call("fd_bilinear_up_bwd", L.ptr(gy), L.ptr(gx.t), 2, 6, 6, 6, 5, L.stream())           # Wout < Win
    # 65536 planes of one pixel: the plane index is blockIdx.y.  The buffers are real and large enough, the answer must come before any launch
    n = 65536
    src, dst = torch.rand(n, device="cuda"), Band(n)
    for fn in ("fd_bilinear_up_fwd", "fd_bilinear_up_bwd"):
        with pytest.raises(RuntimeError, match="at most 65535"):
            L.call(fn, L.ptr(src), L.ptr(dst.t), n, 1, 1, 1, 1, L.stream())
    torch.cuda.synchronize()
    assert gx.untouched() and dst.untouched(), "a refused call must launch nothing"
    L.call("fd_bilinear_up_bwd", L.ptr(src), L.ptr(dst.t), n - 1, 1, 1, 1, 1, L.stream())         # 65535 planes are taken
    assert dst.intact() and torch.equal(dst.t[:n - 1], src[:n - 1]) and bool((dst.t[n - 1:] == SENTINEL).all())


def _ssim_case(L, planes, H, W, kind):
    inp = R.ssim_inputs(planes, H, W, kind)
    ref, ora = R.ssim_ref(inp, F64), R.ssim_ref(inp, F32)
    x, y, cot = dev(inp["x"]), dev(inp["y"]), dev(inp["cot"])
    n = planes * H * W
    out = Band(n)
    L.call("fd_ssim_fwd", L.ptr(x), L.ptr(y), L.ptr(out.t), 1, planes, H, W, L.stream())
    gcap = lambda k: cap_of(1e-3, 1e-4 * float(ref["gx"].abs().max()), ref[k])
    with Checks("ssim %s %dx%dx%d" % (kind, planes, H, W)) as c:
        c.guard("forward", out)
        c.close("ssim", out.t.view(ref["ssim"].shape), ref["ssim"], ora["ssim"], cap=cap_of(1e-4, 2e-5, ref["ssim"]))
        both = None
        for want_x, want_y in ((True, True), (True, False), (False, True)):
            gx, gy = Band(n), Band(n)
            L.call("fd_ssim_bwd", L.ptr(x), L.ptr(y), L.ptr(cot), L.ptr(gx.t) if want_x else None, L.ptr(gy.t) if want_y else None,
                   1, planes, H, W, L.stream())
            c.guard("backward gx=%d gy=%d" % (want_x, want_y), gx, gy)
            if both is None:
                both = (gx, gy)
                c.close("gx", gx.t.view(ref["gx"].shape), ref["gx"], ora["gx"], cap=gcap("gx"))
                c.close("gy", gy.t.view(ref["gy"].shape), ref["gy"], ora["gy"], cap=gcap("gy"))
            elif want_x:
                assert gy.untouched(), "gy was not asked for"
                c.exact("gx alone", gx.t, both[0].t)
            else:
                assert gx.untouched(), "gx was not asked for"
                c.exact("gy alone", gy.t, both[1].t)


@pytest.mark.parametrize("planes", R.SSIM_PLANES)
@pytest.mark.parametrize("H,W", R.SSIM_HW)
def test_ssim(L, H, W, planes):
    _ssim_case(L, planes, H, W, "smooth")


def test_ssim_of_uniform_random_images(L):
    _ssim_case(L, *R.SSIM_UNIFORM_CASE, "uniform")


def test_ssim_of_equal_windows_is_exactly_zero(L):
    planes, H, W = R.SSIM_EQUAL_CASE
    inp = R.ssim_inputs(planes, H, W, "equal")
    ref, ora = R.ssim_ref(inp, F64), R.ssim_ref(inp, F32)
    x, y, out = dev(inp["x"]), dev(inp["y"]), Band(planes * H * W)
    L.call("fd_ssim_fwd", L.ptr(x), L.ptr(y), L.ptr(out.t), 1, planes, H, W, L.stream())
    got = out.t.view(ref["ssim"].shape)
    with Checks("ssim equal block %dx%dx%d" % (planes, H, W)) as c:
        c.guard("forward", out)
        c.close("ssim", got, ref["ssim"], ora["ssim"], cap=cap_of(1e-4, 2e-5, ref["ssim"]))
        c.exact("windows inside the block", got[..., H - 7:, W - 7:], torch.zeros(1, planes, 7, 7))


@pytest.mark.parametrize("B", R.REPROJ_B)
@pytest.mark.parametrize("H,W", R.SSIM_HW)
def test_reprojection_loss_map(L, H, W, B):
    inp = R.reproj_inputs(B, H, W)
    pred, target = dev(inp["pred"]), dev(inp["target"])
    P, stride = H * W, H * W + R.REPROJ_GAP
    with Checks("reproj map %dx%dx%d" % (B, H, W)) as c:
        for use_ssim in (True, False):
            ref, ora = R.reproj_ref(inp, F64, use_ssim), R.reproj_ref(inp, F32, use_ssim)
            out = Band((B - 1) * stride + P)
            L.call("fd_reproj_loss_map", L.ptr(pred), L.ptr(target), L.ptr(out.t), stride, B, H, W, int(use_ssim), L.stream())
            c.guard("ssim=%d" % use_ssim, out)
            for b in range(B - 1):
                assert bool((out.t[b * stride + P:(b + 1) * stride] == SENTINEL).all()), "the floats between images %d and %d were written" % (b, b + 1)
            got = torch.stack([out.t[b * stride:b * stride + P] for b in range(B)]).view(B, 1, H, W)
            c.close("ssim=%d" % use_ssim, got, ref["map"], ora["map"], cap=cap_of(1e-4, 2e-5, ref["map"]))


def _smooth_case(L, B, H, W, normalize, wrap=lambda t: t):
    inp = R.smooth_inputs(B, H, W)
    ref, ora = R.smooth_ref(inp, F64, normalize), R.smooth_ref(inp, F32, normalize)
    disp, img = wrap(dev(inp["disp"])), dev(inp["img"])
    g = torch.tensor([R.SMOOTH_COT], device="cuda")
    n_ws = L.query("fd_smooth_ws_floats", B, H, W)
    assert n_ws == 2 * B + 2 * B * (-(-H * W // 1024))
    out, d_disp = Band(1), Band(B * H * W)
    ws_f, ws_b = Band(n_ws, fill=float("nan")), Band(n_ws, fill=float("nan"))
    L.call("fd_smooth_fwd", L.ptr(disp), L.ptr(img), L.ptr(out.t), L.ptr(ws_f.t), B, H, W, int(normalize), L.stream())
    L.call("fd_smooth_bwd", L.ptr(disp), L.ptr(img), L.ptr(g), L.ptr(d_disp.t), L.ptr(ws_b.t), B, H, W, int(normalize), L.stream())
    with Checks("smooth %dx%dx%d normalize=%d" % (B, H, W, normalize)) as c:
        c.guard("outputs and workspaces", out, d_disp, ws_f, ws_b)
        c.close("loss", out.t.view(()), ref["loss"], ora["loss"], cap=cap_of(1e-5, 1e-8, ref["loss"]))
        c.close("g_disp", d_disp.t.view(ref["g_disp"].shape), ref["g_disp"], ora["g_disp"], cap=1e-3 + 1e-5)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("B", R.SMOOTH_B)
@pytest.mark.parametrize("H,W", R.SMOOTH_SHAPES)
def test_smooth_loss(L, H, W, B, normalize):
    _smooth_case(L, B, H, W, normalize)


@pytest.mark.parametrize("B,H,W,normalize", R.SMOOTH_EXTRA)
def test_smooth_loss_past_its_partial_sum_and_block_caps(L, B, H, W, normalize):
    _smooth_case(L, B, H, W, normalize)


def test_smooth_loss_with_the_disparity_off_alignment(L):
    """4 bytes off 16-byte alignment k_image_mean must take its scalar loop: the same bound holds."""
    _smooth_case(L, *R.SMOOTH_OFFSET_CASE, True, wrap=offset_view)


@pytest.mark.parametrize("si_mode", R.COMBINE_SI)
@pytest.mark.parametrize("n", R.COMBINE_N)
def test_combine_losses(L, n, si_mode):
    """One thread restating the reference's Python loop: the float32 restatement's values, bit for bit, both ways."""
    inp = R.combine_inputs(n, si_mode)
    want = R.combine_ref(inp, F32)
    terms = [[None if t is None else dev(t).reshape(1) for t in inp[k]] for k in ("photo", "smooth", "si")]
    P = ctypes.c_void_p * n
    arr = [P(*[L.ptr(t) for t in group]) for group in terms]
    out, grads = Band(n + 1), Band(3 * n)
    g = torch.tensor([inp["cot"]], device="cuda")
    L.call("fd_combine_losses_fwd", ctypes.addressof(arr[0]), ctypes.addressof(arr[1]), ctypes.addressof(arr[2]), n, inp["w"], L.ptr(out.t), L.stream())
    L.call("fd_combine_losses_bwd", L.ptr(g), n, inp["w"], L.ptr(grads.t), L.stream())
    with Checks("combine n=%d si=%s" % (n, si_mode)) as c:
        c.guard("outputs", out, grads)
        c.exact("loss/s", out.t[:n], want["loss"])
        c.exact("total", out.t[n], want["total"])
        c.exact("d total / d photo", grads.t[:n], want["g_photo"])
        c.exact("d total / d smooth", grads.t[n:2 * n], want["g_smooth"])
        c.exact("d total / d si", grads.t[2 * n:], want["g_si"])
        c.close("total against float64", out.t[n], R.combine_ref(inp, F64)["total"], want["total"])
