"""tests/bn_ref.py (the float64 restatement that tests/test_gpu_bn_edges.py holds the BatchNorm kernels to) against torch's own
BatchNorm2d (+ residual + relu + max_pool2d) in float64 with autograd, and the two guarantees of its input generator.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_ref as R

T64 = torch.float64
CPU_SHAPES = [(1, 3, 2, 2, 1), (4, 5, 4, 8, 2), (16, 3, 2, 2, 16), (2, 3, 5, 7, 1), (2, 3, 4, 8, 1), (2, 3, 12, 20, 1)]
CPU_STEM = [s for s in R.STEM]


def t64(a):
    return torch.from_numpy(np.asarray(a).astype(np.float64))


def close(got, want, what, tol=1e-11):
    got, want = np.asarray(got, np.float64), want.detach().numpy() if torch.is_tensor(want) else np.asarray(want)
    assert got.shape == want.shape, what
    err = np.abs(got - want).max() if got.size else 0.0
    assert err <= tol * max(1.0, np.abs(want).max()), "%s: %.3g" % (what, err)


def torch_bn(case, groups, relu, use_res, stem=False, g_feat=True):
    """G consecutive passes of one torch BatchNorm2d over the sub-batches, float64, autograd."""
    N, C, H, W, _ = case["shape"]
    bn = torch.nn.BatchNorm2d(C, eps=R.EPS, momentum=R.MOMENTUM).to(T64).train()
    with torch.no_grad():
        bn.weight.copy_(t64(case["w"])); bn.bias.copy_(t64(case["b"]))
        bn.running_mean.copy_(t64(case["rm"])); bn.running_var.copy_(t64(case["rv"]))
    x = t64(case["x"]).requires_grad_(True)
    res = t64(case["residual"]).requires_grad_(True) if use_res else None
    Ng = N // groups
    ys = []
    for g in range(groups):
        y = bn(x[g * Ng:(g + 1) * Ng])
        if use_res:
            y = y + res[g * Ng:(g + 1) * Ng]
        ys.append(F.relu(y) if relu else y)
    y = torch.cat(ys)
    out = {"y": y, "rm": bn.running_mean.clone(), "rv": bn.running_var.clone()}
    if stem:
        p, flat = F.max_pool2d(y, 3, 2, 1, return_indices=True)
        loss = (p * t64(case["g_pooled"])).sum() + ((y * t64(case["g_feat"])).sum() if g_feat else 0)
        out["pooled"], out["flat"] = p, flat
    else:
        loss = (y * t64(case["gy"])).sum()
    grads = torch.autograd.grad(loss, [x, bn.weight, bn.bias] + ([res] if use_res else []))
    out["gx"], out["gw"], out["gb"] = grads[:3]
    out["gres"] = grads[3] if use_res else None
    return out


@pytest.mark.parametrize("shape", CPU_SHAPES, ids=str)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("use_res", [False, True])
def test_train_matches_torch_float64(shape, relu, use_res):
    case = R.make_case(shape, seed=3)
    G = shape[4]
    res = case["residual"] if use_res else None
    want = torch_bn(case, G, relu, use_res)
    f = R.train_fwd(case["x"], case["w"], case["b"], res, G, R.EPS, R.MOMENTUM, relu, (case["rm"], case["rv"]))
    close(f["y"], want["y"], "y")
    close(f["running_mean"], want["rm"], "running_mean")
    close(f["running_var"], want["rv"], "running_var")
    b = R.train_bwd(case["x"], case["gy"], case["w"], case["b"], f["save_mean"], f["save_invstd"], res, relu, G)
    close(b["gx"], want["gx"], "gx")
    close(b["gweight"], want["gw"], "gweight")
    close(b["gbias"], want["gb"], "gbias")
    if use_res:
        close(b["g_residual"], want["gres"], "g_residual")
    else:
        assert b["g_residual"] is None
    # saved statistics: what torch's own batch_norm kernel reports for each sub-batch
    N, C = shape[:2]
    for g in range(G):
        xs = t64(case["x"])[g * (N // G):(g + 1) * (N // G)]
        _, m, i = torch.native_batch_norm(xs, None, None, None, None, True, R.MOMENTUM, R.EPS)
        close(f["save_mean"][g * C:(g + 1) * C], m, "save_mean")
        close(f["save_invstd"][g * C:(g + 1) * C], i, "save_invstd")
    # the float32 restatement is the same formula: it lands within float32 rounding of the float64 one
    f32 = R.train_fwd_f32(case["x"], case["w"], case["b"], res, G, R.EPS, R.MOMENTUM, relu, (case["rm"], case["rv"]))
    assert f32["y"].dtype == np.float32 and f32["save_invstd"].dtype == np.float32
    close(f32["y"], f["y"], "y (float32 restatement)", tol=1e-5)
    b32 = R.train_bwd_f32(case["x"], case["gy"], case["w"], case["b"], f32["save_mean"], f32["save_invstd"], res, relu, G)
    assert b32["gx"].dtype == np.float32
    close(b32["gx"], b["gx"], "gx (float32 restatement)", tol=1e-4)


def test_grouped_equals_consecutive_passes():
    case = R.make_case((4, 5, 4, 8, 2), seed=3)
    x, w, b = case["x"], case["w"], case["b"]
    both = R.train_fwd(x, w, b, None, 2, R.EPS, R.MOMENTUM, 1, (case["rm"], case["rv"]))
    first = R.train_fwd(x[:2], w, b, None, 1, R.EPS, R.MOMENTUM, 1, (case["rm"], case["rv"]))
    second = R.train_fwd(x[2:], w, b, None, 1, R.EPS, R.MOMENTUM, 1, (first["running_mean"], first["running_var"]))
    assert np.array_equal(both["y"], np.concatenate([first["y"], second["y"]]))
    assert np.array_equal(both["save_mean"], np.concatenate([first["save_mean"], second["save_mean"]]))
    assert np.array_equal(both["running_mean"], second["running_mean"]) and np.array_equal(both["running_var"], second["running_var"])


def test_eval_matches_torch_float64():
    case = R.make_case((2, 3, 5, 7, 1), seed=4)
    for relu in (0, 1):
        for res in (None, case["residual"]):
            want = F.batch_norm(t64(case["x"]), t64(case["rm"]), t64(case["rv"]), t64(case["w"]), t64(case["b"]), False, 0.0, R.EPS)
            want = want + t64(res) if res is not None else want
            want = F.relu(want) if relu else want
            close(R.eval_fwd(case["x"], case["w"], case["b"], res, case["rm"], case["rv"], R.EPS, relu), want, "eval")


@pytest.mark.parametrize("shape", CPU_STEM, ids=str)
@pytest.mark.parametrize("g_feat", [False, True])
def test_stem_tail_matches_torch_float64(shape, g_feat):
    case = R.make_case(shape, seed=5, stem=True)
    N, C, H, W, G = shape
    want = torch_bn(case, G, 1, False, stem=True, g_feat=g_feat)
    f = R.relu_maxpool_fwd(case["x"], case["w"], case["b"], G, R.EPS, R.MOMENTUM, (case["rm"], case["rv"]))
    close(f["feat"], want["y"], "features[0]")
    close(f["pooled"], want["pooled"], "pooled")
    close(f["running_var"], want["rv"], "running_var")
    # argmax byte kh * 3 + kw -> torch's flat index into the plane
    idx = f["idx"].astype(np.int64)
    ho, wo = np.meshgrid(np.arange(R.pool_out(H)), np.arange(R.pool_out(W)), indexing="ij")
    flat = (2 * ho - 1 + idx // 3) * W + (2 * wo - 1 + idx % 3)
    feat = f["feat"].reshape(N, C, -1)
    assert np.array_equal(np.take_along_axis(feat, flat.reshape(N, C, -1), 2), f["pooled"].reshape(N, C, -1))
    nz = f["pooled"] > 0                                   # where the maximum is a tie of zeros torch may name another tap
    assert np.array_equal(flat[nz], want["flat"].numpy()[nz])
    b = R.relu_maxpool_bwd(case["x"], case["g_pooled"], f["idx"], case["g_feat"] if g_feat else None, case["w"], case["b"],
                           f["save_mean"], f["save_invstd"], G)
    close(b["gx"], want["gx"], "gx")
    close(b["gweight"], want["gw"], "gweight")
    close(b["gbias"], want["gb"], "gbias")


def test_first_maximum_in_raster_order_wins():
    f = np.zeros((1, 1, 4, 4))
    f[0, 0, 1, 1] = f[0, 0, 1, 2] = f[0, 0, 2, 1] = 3.0
    p, idx = R.maxpool_fwd(f)
    assert idx[0, 0, 0, 0] == 8 and idx[0, 0, 0, 1] == 6 and idx[0, 0, 1, 0] == 2 and idx[0, 0, 1, 1] == 0
    g = R.maxpool_bwd(np.ones((1, 1, 2, 2)), idx, 4, 4)
    assert g[0, 0, 1, 1] == 4 and g.sum() == 4             # all four windows name pixel (1, 1)


def test_parts_merge_to_the_statistics():
    x = R.make_case((2, 3, 12, 20, 1), seed=6)["x"]
    ref = R.train_fwd(x, None, None, None, 1, R.EPS, R.MOMENTUM, 0, None)
    for S in (1, 2, 15, 60):
        p = R.parts_from(x, S).astype(np.float64)
        assert p.shape == (2, 3, S, 2) and R.parts_from(x, S).dtype == np.float32
        cnt, M = 240 // S, 480
        mean = p[..., 0].sum(axis=(0, 2)) / M
        m2 = (p[..., 1] + cnt * (p[..., 0] / cnt - mean[None, :, None]) ** 2).sum(axis=(0, 2))
        close(mean, ref["save_mean"], "mean", 1e-6)
        close(m2 / M, ref["var"], "var", 1e-6)


@pytest.mark.parametrize("shape", R.TRAIN_SHAPES + [s for s, _ in R.PARTS], ids=str)
def test_generator_keeps_preactivations_off_zero(shape):
    case = R.make_case(shape, seed=11)
    assert case["x"].dtype == np.float32 and case["moved"] <= max(1, 0.01 * case["x"].size)
    for res in (None, case["residual"]):
        assert R.min_margin(case["x"], case["w"], case["b"], res, shape[4]) >= R.MARGIN


@pytest.mark.parametrize("shape", R.STEM + [R.STEM_BIG], ids=str)
def test_generator_keeps_pooling_taps_apart(shape):
    case = R.make_case(shape, seed=11, stem=True)
    assert case["moved"] <= max(1, 0.01 * case["x"].size)
    assert R.min_margin(case["x"], case["w"], case["b"], None, shape[4]) >= R.MARGIN
    assert R.min_tap_gap(case["x"], case["w"], case["b"], shape[4]) >= R.MARGIN


def test_relu_of_the_restatement_keeps_nan():
    v = np.array([-1.0, -0.0, 0.0, 2.0, np.nan, np.inf, -np.inf])
    got, want = R.relu(v), torch.relu(torch.from_numpy(v)).numpy()
    assert np.array_equal(got, want, equal_nan=True) and not np.signbit(got[1])
