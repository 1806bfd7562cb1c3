"""fd_photo_ms_fwd / fd_photo_ms_bwd (csrc/photometric_ms.hip) with NF = 1 and 3: the all-scales fused loss for ONE and THREE source frames, the
stereo configurations of --use_stereo (frame_ids [0, "s"] and [0, -1, 1, "s"]).  Same yardsticks and tolerances as the two-frame
kernel's tests in test_gpu_losspath.py, whose helpers are reused: the CPU oracle, its float64 run, and the per-scale HIP kernels.
The stereo partner "s" is the scene of frame 0 shifted by 3 pixels; its pose ``stereo_T`` carries no gradient."""
import numpy as np
import pytest
import torch

import inputs as gin
from conftest import assert_close, assert_mostly_close
from oracle import layers as OL
from oracle import trainer as OT
from test_gpu_losspath import FD, _grad_error_stats, _hip_photo_terms, _hip_photo_terms_ms, _oracle_photo_terms, cpu, dev, grads  # noqa: F401

pytestmark = pytest.mark.gpu

FRAMES = {1: ["s"], 3: [-1, 1, "s"]}


def _case(seed, B, H, W, nf, sign=-1.0, **over):
    """Seeded inputs with the stereo partner, the disparity pyramid, the poses (``stereo_T`` for "s": mono_dataset.py:216-222) and
    the tie-break noise [B,NF,H,W] per scale."""
    fids = FRAMES[nf]
    opt = OT.default_opt(height=H, width=W, frame_ids=[0] + fids, use_stereo=True, **over)
    assert OT.frame_setup(opt)[2] == [0] + fids
    inp, rng = gin.batch_inputs(seed, B, H, W)
    base = gin.smooth_image(np.random.RandomState(seed), B, 3, H, W + 8)          # batch_inputs' scene; frame 0 is columns 4 .. 4 + W
    img = base[..., 7:7 + W] + 0.01 * np.random.RandomState(seed + 7).randn(B, 3, H, W).astype(np.float32)
    img = torch.from_numpy(np.clip(img, 0, 1).astype(np.float32))
    for s in range(4):
        inp[("color", "s", s)] = img if s == 0 else torch.nn.functional.avg_pool2d(img, 2 ** s)
    disp0 = gin.disp_pyramid(rng, B, H, W)
    T0 = {}
    for f in fids:
        if f == "s":
            T0[f] = torch.eye(4).repeat(B, 1, 1)
            T0[f][:, 0, 3] = sign * 0.1
        else:
            T0[f] = OL.transformation_from_parameters(*gin.small_poses(rng, B), invert=(f < 0))
    inp["stereo_T"] = T0["s"]
    noise = [torch.from_numpy(np.random.RandomState(1000 + seed + s).randn(B, nf, H, W).astype(np.float32)) for s in range(4)]
    return opt, inp, disp0, T0, noise


def _leaves(disp0, T0, to=None):
    """Disparities and temporal poses as leaves that require a gradient; ``stereo_T`` as a plain tensor."""
    put = (lambda t: t.clone()) if to is None else to
    d = {s: put(disp0[("disp", s)]).requires_grad_(True) for s in range(4)}
    T = {f: (put(t) if f == "s" else put(t).requires_grad_(True)) for f, t in T0.items()}
    return d, T


def _oracle(opt, inp, d, T, noise):
    i2 = dict(inp)
    i2["stereo_T"] = T["s"]
    return _oracle_photo_terms(opt, i2, d, {f: t for f, t in T.items() if f != "s"}, noise)


@pytest.mark.parametrize("nf", [1, 3])
@pytest.mark.parametrize("seed,B,H,W,rows,sign,over", [
    (404, 2, 64, 96, 0, -1.0, {}),
    (404, 2, 64, 96, 0, 1.0, {}),                       # the other sign of stereo_T[0, 3] (an "r" line, or a flipped "l" line)
    (404, 2, 64, 96, 7, -1.0, {}),                      # ragged strips: 64 = 9 x 7 + 1
    (31, 2, 48, 200, 16, 1.0, {}),                      # several strips in x (200 = 3 x 60 + 20) and y
    (909, 2, 32, 184, 0, -1.0, {}),                     # four owned columns in the last strip
    (505, 1, 192, 640, 0, -1.0, {}),                    # full size
    (606, 2, 64, 96, 0, -1.0, dict(disable_automasking=True)),
])
def test_multiscale_photo_loss_nf_vs_oracle(FD, monkeypatch, nf, seed, B, H, W, rows, sign, over):
    """Against the oracle's generate_images_pred + compute_losses (trainer.py:425-589), conditions of
    test_multiscale_photo_loss_vs_oracle; ``stereo_T`` gets no gradient and no fd_proj_matrix_bwd call."""
    from fusiondepth_amd import loss_ops
    opt, inp, disp0, T0, noise = _case(seed, B, H, W, nf, sign, **over)
    d_o, T_o = _leaves(disp0, T0)
    terms, _ = _oracle(opt, inp, d_o, T_o, noise)
    d_g, T_g = _leaves(disp0, T0, dev)
    photo, si, sel = _hip_photo_terms_ms(FD, opt, inp, d_g, T_g, noise, rows)
    temporal = [f for f in FRAMES[nf] if f != "s"]
    tot_o, tot_g, flips = 0, 0, 0
    for s in range(4):
        diff = cpu(sel[s]).astype(np.int64) != cpu(terms[s][2])
        flips += int(diff.sum())
        assert diff.mean() <= 3e-4, "argmin differs on %.4f%% of pixels at scale %d" % (100 * diff.mean(), s)
        assert_close(cpu(photo[s]), cpu(terms[s][0]), rtol=1e-4, atol=1e-7, what="to_optimise.mean() s%d" % s)
        assert_close(cpu(si[s]), cpu(terms[s][1]), rtol=1e-4, atol=1e-7, what="si_loss s%d" % s)
        w = 1.0 + 0.25 * s
        tot_o = tot_o + w * terms[s][0] + (2.0 - 0.3 * s) * terms[s][1]
        tot_g = tot_g + w * photo[s] + (2.0 - 0.3 * s) * si[s]
    want = grads(tot_o, [d_o[s] for s in range(4)] + [T_o[f] for f in temporal])
    called = []
    real_call = loss_ops.call
    monkeypatch.setattr(loss_ops, "call", lambda name, *a: (called.append(name), real_call(name, *a))[1])
    tot_g.backward()
    assert called.count("fd_photo_ms_bwd") == 1 and called.count("fd_proj_matrix_bwd") == len(temporal), called
    assert called.count("fd_photo_ms_fwd") == 0, called          # the forward ran before the hook: backward launches no second one
    assert T_g["s"].grad is None and not T_g["s"].requires_grad
    got = [cpu(d_g[s].grad) for s in range(4)] + [cpu(T_g[f].grad) for f in temporal]
    for s in range(4):
        sc = np.abs(want[s]).max()
        assert_mostly_close(got[s], want[s], rtol=2e-3, atol=2e-4 * sc, what="d loss / d disp s%d" % s)
        # see test_multiscale_photo_loss_vs_oracle: an isolated O(1) error in the disparity gradient is a branch within rounding of a tie
        flips += int((np.abs(got[s] - want[s]) > 1e-3 * sc).sum())
    for i, f in enumerate(temporal):
        sc = np.abs(want[4 + i]).max()
        assert_close(got[4 + i], want[4 + i], rtol=1e-3, atol=(3e-2 if flips else 1e-4) * sc, what="d loss / d T f%d" % f)


@pytest.mark.parametrize("nf", [1, 3])
def test_loss_path_nf_error_against_float64(FD, nf):
    """The rule of test_loss_path_error_against_float64: each loss within 1e-6 relative of the float64 oracle; the gradient maps no
    further from float64 than 1.5 x the float32 oracle, plus its floors of 3e-4 relative L1 and 0.2 % of the entries."""
    opt, inp, disp0, T0, noise = _case(404, 2, 64, 96, nf)

    def oracle(dt):
        to = lambda t: t.to(dt).clone()
        i2 = {k: (v.to(dt) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inp.items()}
        d, Tq = _leaves(disp0, T0, to)
        terms, _ = _oracle(opt, i2, d, Tq, [n.to(dt) for n in noise])
        g = torch.autograd.grad(sum(terms[s][0] for s in range(4)), [d[s] for s in range(4)])
        return [float(terms[s][0]) for s in range(4)], [x.double().numpy() for x in g]

    v64, g64 = oracle(torch.float64)
    v32, g32 = oracle(torch.float32)
    d, Tq = _leaves(disp0, T0, dev)
    photo = _hip_photo_terms_ms(FD, opt, inp, d, Tq, noise)[0]
    g = [cpu(x) for x in torch.autograd.grad(sum(photo), [d[s] for s in range(4)])]
    v = [float(p) for p in photo]
    for s in range(4):
        bad_ref, l1_ref = _grad_error_stats(g32[s], g64[s])
        bad, l1 = _grad_error_stats(g[s], g64[s])
        print("[vs float64] NF=%d s%d: loss %.9g (float64 %.9g, rel %.2e); %.3f%% of gradient entries out of tolerance (float32 "
              "reference %.3f%%), rel-L1 %.2e (float32 reference %.2e)"
              % (nf, s, v[s], v64[s], abs(v[s] - v64[s]) / abs(v64[s]), 100 * bad, 100 * bad_ref, l1, l1_ref))
        assert abs(v[s] - v64[s]) <= 1e-6 * abs(v64[s]), "NF=%d loss s%d: %.9g vs float64 %.9g" % (nf, s, v[s], v64[s])
        assert bad <= 1.5 * bad_ref + 2e-3, "NF=%d s%d: %.3f%% vs %.3f%% for the float32 reference" % (nf, s, 100 * bad, 100 * bad_ref)
        assert l1 <= 1.5 * l1_ref + 3e-4, "NF=%d s%d: rel-L1 %.3g vs %.3g for the float32 reference" % (nf, s, l1, l1_ref)


@pytest.mark.parametrize("nf", [1, 3])
def test_multiscale_photo_loss_nf_matches_per_scale_kernels(FD, nf):
    """Counterpart of test_multiscale_photo_loss_matches_per_scale_kernels: value, selection and gradients of fd_photo_ms_* (NF = 1, 3) against
    fd_photo_fwd_ex / fd_photo_bwd_ex, with the LiDAR term on scale 0 only."""
    opt, inp, disp0, T0, noise = _case(404, 2, 64, 96, nf)
    temporal = [f for f in FRAMES[nf] if f != "s"]
    da, Ta = _leaves(disp0, T0, dev)
    db, Tb = _leaves(disp0, T0, dev)
    res = _hip_photo_terms(FD, opt, inp, da, Ta, noise, materialize=False)
    photo, si, sel = _hip_photo_terms_ms(FD, opt, inp, db, Tb, noise, beam_scales=(0,))
    assert si[1] is None and si[2] is None and si[3] is None
    tot_a = sum((1 + s) * res[s][0] for s in range(4)) + 0.7 * res[0][1]
    tot_b = sum((1 + s) * photo[s] for s in range(4)) + 0.7 * si[0]
    for s in range(4):
        assert (cpu(res[s][2]) != cpu(sel[s])).mean() <= 3e-4
        assert_close(cpu(photo[s]), cpu(res[s][0]), rtol=2e-5, atol=1e-7, what="photo s%d" % s)
    assert_close(cpu(si[0]), cpu(res[0][1]), rtol=2e-5, atol=1e-7, what="si s0")
    ga = grads(tot_a, [da[s] for s in range(4)] + [Ta[f] for f in temporal])
    gb = grads(tot_b, [db[s] for s in range(4)] + [Tb[f] for f in temporal])
    for s in range(4):
        assert_mostly_close(gb[s], ga[s], rtol=2e-3, atol=2e-4 * np.abs(ga[s]).max(), what="d disp s%d" % s, max_bad_frac=3e-2)
    for i in range(4, 4 + len(temporal)):
        assert_close(gb[i], ga[i], rtol=1e-3, atol=3e-2 * np.abs(ga[i]).max(), what="d T")


def test_empty_lidar_mask_in_one_stacked_micro_batch_three_frames(FD):
    """Counterpart of test_empty_lidar_mask_in_one_stacked_micro_batch for NF = 3: ``groups = 2`` with micro-batch 0 free of LiDAR
    returns - the stacked si_loss is NaN at every scale, all gradients stay finite, and micro-batch 1's disparities receive their
    stand-alone gradient.  Oracle: the two micro-batches evaluated separately."""
    B = 2
    opt, inp, disp0, T0, noise = _case(404, B, 64, 96, 3)
    gin.make_si_mask_empty(inp, disp0, "sample0")
    want_g, want_si = [], []
    for b in range(B):
        sl = slice(b, b + 1)
        i_b = {k: (v[sl] if torch.is_tensor(v) else v) for k, v in inp.items()}
        d_b, T_b = _leaves({k: v[sl] for k, v in disp0.items()}, {f: t[sl] for f, t in T0.items()})
        terms, _ = _oracle(opt, i_b, d_b, T_b, [n[sl] for n in noise])
        tot = sum(terms[s][0] + terms[s][1] for s in range(4)) / B
        want_g.append(grads(tot, [d_b[s] for s in range(4)]))
        want_si.append([float(terms[s][1]) for s in range(4)])
    assert all(np.isnan(v) for v in want_si[0]) and all(np.isfinite(v) for v in want_si[1])
    d_g, T_g = _leaves(disp0, T0, dev)
    photo, si, _ = _hip_photo_terms_ms(FD, opt, inp, d_g, T_g, noise, groups=2)
    assert all(bool(torch.isnan(v)) for v in si), [float(v) for v in si]
    got = grads(sum(photo[s] + si[s] for s in range(4)), [d_g[s] for s in range(4)])
    for s in range(4):
        assert np.isfinite(got[s]).all()
        want = np.concatenate([want_g[0][s], want_g[1][s]], 0)
        assert_mostly_close(got[s], want, rtol=2e-3, atol=2e-4 * np.abs(want).max(), what="d loss / d disp s%d" % s,
                            max_bad_frac=max(1e-2, 4.0 / got[s].size))


@pytest.mark.parametrize("nf", [1, 3])
def test_multiscale_photo_loss_nf_is_reproducible(FD, nf):
    """Fixed-order reductions, no atomics: two calls on the same inputs give the same bits - losses, ``sel`` and every gradient."""
    opt, inp, disp0, T0, noise = _case(31, 2, 48, 200, nf)
    temporal = [f for f in FRAMES[nf] if f != "s"]
    runs = []
    for _ in range(2):
        d, Tq = _leaves(disp0, T0, dev)
        photo, si, sel = _hip_photo_terms_ms(FD, opt, inp, d, Tq, noise, rows=16)
        tot = sum((1 + s) * photo[s] + (2.0 - 0.3 * s) * si[s] for s in range(4))
        g = torch.autograd.grad(tot, [d[s] for s in range(4)] + [Tq[f] for f in temporal])
        runs.append([torch.stack(photo), torch.stack(si), sel] + list(g))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "%d entries differ between two runs" % int((a != b).sum())
