"""The guarded optimiser step without a GPU: the numpy restatement of its rules (tests/grad_guard_ref.py) against
``torch.nn.utils.clip_grad_norm_`` in float64, the command-line flags of train / refine / complete, and ``FlatAdam``'s host side."""
import numpy as np
import pytest
import torch

import grad_guard_ref as GR
from fusiondepth_amd import dp
from fusiondepth_amd.optim import FlatAdam, check_guard

SHAPES = [(4, 3, 3, 3), (4,), (2, 5), (7, 11)]
LR = 1.5e-4


def _split(flat, shapes):
    out, at = [], 0
    for s in shapes:
        n = int(np.prod(s))
        out.append(flat[at:at + n].reshape(s))
        at += n
    assert at == flat.size
    return out


@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
@pytest.mark.parametrize("factor", [0.5, 2.0, 100.0], ids=["half", "twice", "hundredfold"])
def test_restatement_against_torch_clip_grad_norm(factor, grad_scale):
    """The gradient norm is ``factor`` x max_norm.  torch clips float64 parameters whose gradients are the float32 products ``x``
    (what Adam sees); the restatement's norm agrees within n * 2^-53 relative (two orders of one sum of non-negative terms), and its
    clipped gradient equals torch's once torch's float64 factor has gone through the same float32 rounding."""
    rng = np.random.default_rng(17)
    n = sum(int(np.prod(s)) for s in SHAPES)
    g = rng.standard_normal(n).astype(np.float32)
    max_norm = 1.75
    g *= np.float32(factor * max_norm / grad_scale / np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    x = GR.scaled(g, grad_scale)
    params = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in SHAPES]
    for p, part in zip(params, _split(x.astype(np.float64), SHAPES)):
        p.grad = torch.from_numpy(part.copy())
    total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    sizes = [int(np.prod(s)) for s in SHAPES]
    stats, counters = GR.grad_stats(g, GR.offsets_of(sizes), grad_scale, max_norm)
    assert abs(stats[0] - total) <= GR.norm_bound(n) * total, (stats[0], total)
    assert stats[1] == 0 and stats[3] == 0 and counters == [0, -1, -1]
    for k, p in enumerate(params):                               # the per-segment norms: one parameter per segment here
        assert abs(stats[4 + k] - float(torch.from_numpy(_split(x.astype(np.float64), SHAPES)[k]).norm())) <= GR.norm_bound(sizes[k]) * stats[4 + k]
    coef64 = min(1.0, max_norm / (total + 1e-6))                 # torch's clamp(max_norm / (norm + 1e-6), max=1)
    assert stats[2] <= 1.0 and (stats[2] == 1.0) == (factor < 1.0)
    assert abs(stats[2] - coef64) <= 2.0 ** -23 * coef64
    if factor < 1.0:
        assert all(torch.equal(p.grad, torch.from_numpy(part)) for p, part in zip(params, _split(x.astype(np.float64), SHAPES)))
    else:
        torch_coef = np.concatenate([p.grad.numpy().reshape(-1) for p in params]) / x.astype(np.float64)
        assert np.allclose(torch_coef, coef64, rtol=1e-15, atol=0)
    want = (x * np.float32(coef64)).astype(np.float32)           # torch's factor after the same float32 rounding
    assert np.array_equal(GR.clipped(g, grad_scale, stats[2]).view(np.uint32), want.view(np.uint32))


def test_restatement_skip_rules_and_counters():
    g = np.array([1.0, -2.0, 3.0, 1e30, 0.5], np.float32)
    off = GR.offsets_of([3, 0, 2])
    stats, c = GR.grad_stats(g, off, 1.0, 0.0)
    big = float(np.float32(1e30))                                # its square overflows float32, not float64
    assert stats[0] == np.sqrt(14.0 + (big * big + 0.25)) and np.isfinite(stats[0]) and stats[0] > 9e29
    assert list(stats[4:]) == [np.sqrt(14.0), 0.0, np.sqrt(big * big + 0.25)] and c == [0, -1, -1]
    for bad in (np.nan, np.inf, -np.inf):
        h = g.copy(); h[2] = bad
        stats, c = GR.grad_stats(h, off, 1.0, 5.0, counters=(0, -1, -1), adam_step=6)
        assert stats[1] == 1 and stats[3] == 1 and stats[2] == 1.0 and c == [1, 7, 7]
        stats, c = GR.grad_stats(h, off, 1.0, 5.0, counters=c, adam_step=6)          # the step count did not advance: step 7 again
        assert c == [2, 7, 7]
        stats, c = GR.grad_stats(h, off, 1.0, 5.0, counters=c, adam_step=9)
        assert c == [3, 7, 10]
        stats, c = GR.grad_stats(h, off, 1.0, 0.0, skip_nonfinite=False)
        assert stats[1] == 1 and stats[3] == 0 and c == [0, -1, -1]
    big = np.full(4, 3e38, np.float32)                           # the product overflows in float32: Adam would see inf
    assert GR.grad_stats(big, [0, 4], 2.0)[0][1] == 4 and GR.grad_stats(big, [0, 4], 1.0)[0][1] == 0
    stats, c = GR.grad_stats(np.zeros(0, np.float32), [0, 0], 1.0, 1.0)
    assert list(stats) == [0.0, 0.0, 1.0, 0.0, 0.0] and c == [0, -1, -1]


def test_check_guard():
    assert check_guard("off", 0) == ("off", 0.0) and check_guard("skip", 0.0) == ("skip", 0.0) and check_guard("skip", "2.5") == ("skip", 2.5)
    for mode, norm in (("off", 1.0), ("clip", 0.0), ("skip", -1.0), ("skip", float("nan")), ("skip", float("inf")), (None, 0.0)):
        with pytest.raises(ValueError):
            check_guard(mode, norm)


def test_flags_of_the_three_commands():
    from fusiondepth_amd import complete as C, refine as R, train as T
    assert R.split_off_extra is T.split_off_extra
    for mod in (T, C):
        plain = mod.split_off_extra([])[0]
        assert not {"grad_guard", "clip_grad_norm", "max_skipped_steps"} & set(plain)          # joined only where given
        extra, rest = mod.split_off_extra(["--png", "--grad_guard", "skip", "--seed", "3"])
        assert extra == dict(plain, seed=3, grad_guard="skip") and rest == ["--png"]
        assert mod.split_off_extra(["--grad_guard=off"])[0] == dict(plain, grad_guard="off")
        extra, rest = mod.split_off_extra(["--clip_grad_norm", "1.0", "--png"])               # the norm implies the guard
        assert extra == dict(plain, grad_guard="skip", clip_grad_norm=1.0) and rest == ["--png"]
        assert mod.split_off_extra(["--clip_grad_norm=2.5", "--grad_guard", "skip"])[0] == dict(plain, grad_guard="skip", clip_grad_norm=2.5)
        assert mod.split_off_extra(["--clip_grad_norm", "0"])[0] == dict(plain, clip_grad_norm=0.0)          # no norm: no guard either
        assert mod.split_off_extra(["--grad_guard", "off", "--clip_grad_norm", "0"])[0] == dict(plain, grad_guard="off", clip_grad_norm=0.0)
        assert mod.split_off_extra(["--max_skipped_steps", "0"])[0] == dict(plain, max_skipped_steps=0)
        for bad, word in ((["--grad_guard", "off", "--clip_grad_norm", "1.0"], "needs grad_guard 'skip'"),
                          (["--clip_grad_norm", "-1"], "finite number >= 0"), (["--clip_grad_norm", "nan"], "finite number >= 0"),
                          (["--clip_grad_norm", "inf"], "finite number >= 0"), (["--clip_grad_norm", "big"], "must be a number"),
                          (["--grad_guard", "clip"], "off | skip"), (["--grad_guard"], "needs a value"),
                          (["--max_skipped_steps", "-1"], "max_skipped_steps")):
            with pytest.raises(ValueError, match=word):
                mod.split_off_extra(bad)
        with pytest.raises(ValueError):
            mod.split_off_extra(["--max_skipped_steps", "many"])

    class _Tr:
        grad_guard, clip_grad_norm, max_skipped_steps = "off", 0.0, 10
    tr = _Tr()
    T.apply_guard_flags(tr, T.split_off_extra(["--clip_grad_norm", "1.5", "--max_skipped_steps", "2"])[0])
    assert (tr.grad_guard, tr.clip_grad_norm, tr.max_skipped_steps) == ("skip", 1.5, 2)
    tr = _Tr()
    T.apply_guard_flags(tr, T.split_off_extra([])[0])
    assert (tr.grad_guard, tr.clip_grad_norm, tr.max_skipped_steps) == ("off", 0.0, 10)


def test_trainer_defaults_are_off():
    from fusiondepth_amd.trainer import Trainer
    assert (Trainer.grad_guard, Trainer.clip_grad_norm, Trainer.max_skipped_steps) == ("off", 0.0, 10)


def _adam(segments=None):
    g = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]
    return FlatAdam(dp.FlatParameters(params), LR, 6, segments=segments)


def _fill(ad, steps):
    g = torch.Generator().manual_seed(7)
    ad.exp_avg.copy_(torch.randn(ad.exp_avg.shape, generator=g))
    ad.exp_avg_sq.copy_(torch.rand(ad.exp_avg_sq.shape, generator=g))
    ad.step_count = steps
    ad.state[0] = float(steps)


def _todays_state_dict(ad):
    """``FlatAdam.state_dict()`` as it was before the guard, written out: the host step count, the moments per parameter."""
    state = {}
    if ad.step_count > 0:
        for i, p in enumerate(ad.flat.params):
            o, n = ad.flat.offsets[i], p.numel()
            state[i] = {"step": torch.tensor(float(ad.step_count)), "exp_avg": ad.exp_avg[o:o + n].view(p.shape).clone(),
                        "exp_avg_sq": ad.exp_avg_sq[o:o + n].view(p.shape).clone()}
    group = {"lr": ad.lr, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False, "maximize": False, "foreach": None,
             "capturable": False, "differentiable": False, "fused": None, "initial_lr": ad.initial_lr, "params": list(range(len(ad.flat.params)))}
    return {"state": state, "param_groups": [group]}


def _same_dict(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same_dict(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same_dict(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def test_state_dict_with_the_guard_off_is_todays():
    for steps in (0, 3):
        for segments in (None, [2, 2], [("encoder", 3), ("depth", 1)]):
            ad = _adam(segments)
            _fill(ad, steps)
            ad.state[0] = 99.0                                   # guard off: the device count is not what is written
            assert ad.guard_mode == "off" and ad.guard_stats is None and ad.guard_report() == {}
            assert _same_dict(ad.state_dict(), _todays_state_dict(ad))
            ad.configure_guard("off", 0.0)                       # spelled out: still nothing allocated, nothing different
            assert ad.guard_stats is None and _same_dict(ad.state_dict(), _todays_state_dict(ad))


def test_segment_table_and_guard_tables():
    ad = _adam([("encoder", 1), ("depth", 2), ("pose", 1)])
    assert ad.segment_names == ["encoder", "depth", "pose"] and ad._segment_offsets == [0, 108, 108 + 4 + 10, 199]
    assert _adam()._segment_offsets == [0, 199] and _adam([4]).segment_names == ["segment0"]
    with pytest.raises(ValueError, match="cover 3 parameters"):
        _adam([1, 2])
    with pytest.raises(ValueError, match="segments"):
        FlatAdam(dp.FlatParameters([torch.nn.Parameter(torch.zeros(1)) for _ in range(17)]), LR, 6, segments=[1] * 17)
    for bad in (("off", 1.0), ("clip", 0.0), ("skip", -1.0)):
        with pytest.raises(ValueError):
            ad.configure_guard(*bad)
    assert ad.guard_stats is None and ad.guard_counters_host() == [0, -1, -1]
    ad.configure_guard("skip", 2.0)                              # the tables, once (host tensors here: nothing is launched)
    assert ad.guard_stats.dtype == torch.float64 and ad.guard_stats.tolist() == [0, 0, 1, 0, 0, 0, 0]
    assert ad.guard_counters.dtype == torch.int64 and ad.guard_counters.tolist() == [0, -1, -1] and ad._guard_seg.tolist() == [0, 108, 122, 199]
    assert ad._guard_ws.numel() * 8 == (3 + 1) * 8               # one block for 199 elements: n_seg + 1 rows of one double
    stats = ad.guard_stats
    ad.load_guard_counters([2, 5, 9])
    ad.configure_guard("skip", 0.0)                              # reconfigured: same tables, the counters stay
    assert ad.guard_stats is stats and ad.max_norm == 0.0 and ad.guard_counters_host() == [2, 5, 9]
    assert ad.guard_report() == {"grad_norm": 0.0, "grad_norm/encoder": 0.0, "grad_norm/depth": 0.0, "grad_norm/pose": 0.0, "clip_coef": 1.0,
                                 "nonfinite": 0, "skipped_steps": 2, "first_skipped_step": 5, "last_skipped_step": 9}
    # with the guard on a skipped step is not an Adam step: adam.pth holds the count the kernel kept
    _fill(ad, 4)
    ad.state[0] = 3.0
    assert ad.applied_steps() == 3 and float(ad.state_dict()["state"][0]["step"]) == 3.0
    ad.configure_guard("off", 0.0)
    assert ad.applied_steps() == 4 and float(ad.state_dict()["state"][0]["step"]) == 4.0 and ad.guard_report() == {}


def test_ws_size_query():
    from fusiondepth_amd import functional as FD
    assert FD.grad_stats_ws_bytes(0, 1) == 16 and FD.grad_stats_ws_bytes(4096, 1) == 16 and FD.grad_stats_ws_bytes(4097, 3) == 2 * 4 * 8
    assert FD.grad_stats_ws_bytes(1 << 40, FD.GUARD_MAX_SEGMENTS) == 1024 * 17 * 8            # the grid stops growing: n alone decides it
    for bad in ((10, 0), (10, FD.GUARD_MAX_SEGMENTS + 1), (-1, 1)):
        with pytest.raises(ValueError):
            FD.grad_stats_ws_bytes(*bad)
