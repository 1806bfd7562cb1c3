"""The guarded optimiser step on the GPU: fd_grad_stats against the float64 restatement of
tests/grad_guard_ref.py, fd_adam_step_guarded bit for bit against the unguarded Adam entry points, the skip, a captured replay, the
Trainer with the guard on, two data-parallel ranks of which one meets an inf, and the train command with ``--clip_grad_norm``."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import grad_guard_ref as GR
import test_gpu_trainer as TT
from fusiondepth_amd import functional as FD
from fusiondepth_amd._lib import call, query, stream

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

BETAS, EPS, LR = (0.9, 0.999), 1e-8, 1.5e-4
GUARD = 8                                     # floats on either side of a buffer that no kernel may touch
SIZES = [0, 1, 3, 255, 256, 257, 65536 + 13, (1 << 20) + 5]
MID = 65536 + 13


class _Buf:
    """n floats at `off` floats past a 16-byte boundary, between two guard bands (n = 0 included: ``ptr`` is computed, not asked for)"""

    def __init__(self, values, off):
        n = values.numel()
        self.raw = torch.full((GUARD + off + n + GUARD,), 12345.0, device="cuda")
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.t = self.raw[self.lo:self.hi]
        self.t.copy_(values)
        self.ptr = self.raw.data_ptr() + 4 * self.lo
        assert self.ptr % 16 == 4 * off

    def guards_intact(self):
        return bool((self.raw[:self.lo] == 12345.0).all()) and bool((self.raw[self.hi:] == 12345.0).all())


class _Tables:
    """The small device tables of one guard: segment offsets, ws (with a guard band behind it), stats, counters, [step, lr]."""

    def __init__(self, n, sizes, step=0):
        self.n, self.n_seg = n, len(sizes)
        self.offsets = GR.offsets_of(sizes)
        assert self.offsets[-1] == n
        self.seg = torch.tensor(self.offsets, dtype=torch.int64, device="cuda")
        self.ws_doubles = query("fd_grad_stats_ws_bytes", n, self.n_seg) // 8
        assert self.ws_doubles >= self.n_seg + 1
        self.ws = torch.full((self.ws_doubles + 4,), -7.0, dtype=torch.float64, device="cuda")
        self.stats = torch.full((4 + self.n_seg + 2,), -7.0, dtype=torch.float64, device="cuda")
        self.counters = torch.tensor([0, -1, -1, 777], dtype=torch.int64, device="cuda")
        self.state = torch.tensor([float(step), LR], device="cuda")

    def run(self, grad_ptr, grad_scale=1.0, max_norm=0.0, skip_nonfinite=1):
        call("fd_grad_stats", grad_ptr, self.n, self.seg.data_ptr(), self.n_seg, grad_scale, max_norm, skip_nonfinite, self.ws.data_ptr(),
             self.stats.data_ptr(), self.counters.data_ptr(), self.state.data_ptr(), stream())

    def read(self):
        """(stats as float64 numpy, counters as a list) after checking that nothing was written past either table or ws"""
        stats, counters, ws = self.stats.cpu().numpy(), self.counters.tolist(), self.ws.cpu().numpy()
        assert (stats[4 + self.n_seg:] == -7.0).all() and counters[3] == 777 and (ws[self.ws_doubles:] == -7.0).all()
        return stats[:4 + self.n_seg], counters[:3]


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _seg_tables(n):
    return [s for s in ([n], [1, n - 1], [3, 0, 1, n - 4]) if min(s) >= 0]


_VALUES = {}


def _values(n):
    """n gradient values, made once per size: N(0, 0.1), every 97th one 1e30 (its square overflows float32, not the float64 sum)"""
    if n not in _VALUES:
        v = torch.randn(n, generator=torch.Generator().manual_seed(31 * n + 1)) * 0.1
        v[5::97] = 1e30
        _VALUES[n] = v
    return _VALUES[n]


def _check_stats(stats, want, n, sizes):
    bound = GR.norm_bound(n)
    assert abs(stats[0] - want[0]) <= bound * want[0], ("norm", stats[0], want[0])
    for k, size in enumerate(sizes):
        assert abs(stats[4 + k] - want[4 + k]) <= GR.norm_bound(size) * want[4 + k], ("segment %d" % k, stats[4 + k], want[4 + k])
    assert stats[1] == want[1], ("count", stats[1], want[1])
    assert stats[3] == want[3], ("skip", stats[3], want[3])


# ---- 1. fd_grad_stats against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_grad_stats_matches_the_float64_restatement(n):
    values = _values(n)
    host = values.numpy()
    for off in (0, 1):
        g = _Buf(values, off)
        for grad_scale in (1.0, 0.25):
            for sizes in _seg_tables(n):
                tb = _Tables(n, sizes)
                tb.run(g.ptr, grad_scale)
                first, counters = tb.read()
                want, want_counters = GR.grad_stats(host, tb.offsets, grad_scale)
                assert np.isfinite(want[0]) and want[1] == 0
                _check_stats(first, want, n, sizes)
                assert first[2] == 1.0 and counters == want_counters == [0, -1, -1]
                ws_first = tb.ws.clone()
                tb.run(g.ptr, grad_scale)                        # two calls on one buffer: the same bits
                second, _ = tb.read()
                assert np.array_equal(first.view(np.uint64), second.view(np.uint64)) and torch.equal(ws_first.view(torch.int64), tb.ws.view(torch.int64))
                assert _same(g.t, values.cuda()) and g.guards_intact(), "fd_grad_stats wrote to the gradient or beside it"


def test_grad_stats_refuses_what_it_does_not_cover():
    g = _Buf(torch.zeros(8), 0)
    tb = _Tables(8, [8])
    too_many = torch.zeros(FD.GUARD_MAX_SEGMENTS + 2, dtype=torch.int64, device="cuda")
    for args in ((g.ptr, 8, too_many.data_ptr(), FD.GUARD_MAX_SEGMENTS + 1), (g.ptr, 8, tb.seg.data_ptr(), 0), (g.ptr, -1, tb.seg.data_ptr(), 1),
                 (g.ptr + 2, 8, tb.seg.data_ptr(), 1), (None, 8, tb.seg.data_ptr(), 1)):
        with pytest.raises(RuntimeError, match="fd_grad_stats"):
            call("fd_grad_stats", *args, 1.0, 0.0, 1, tb.ws.data_ptr(), tb.stats.data_ptr(), tb.counters.data_ptr(), tb.state.data_ptr(), stream())
    assert query("fd_grad_stats_ws_bytes", 8, FD.GUARD_MAX_SEGMENTS + 1) == -1
    with pytest.raises(RuntimeError, match="float64"):
        FD.grad_stats(g.t, tb.seg, tb.ws, tb.stats.float(), tb.counters, tb.state)
    with pytest.raises(RuntimeError, match="ws"):
        FD.grad_stats(g.t, tb.seg, tb.ws[:1], tb.stats, tb.counters, tb.state)


# ---- 2. where the value that is not finite sits --------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_one_nonfinite_value_anywhere_is_counted_and_skips(bad):
    """Element 0, the last one, both sides of the first boundary between two blocks' 16-byte loads (256 threads x 4 floats behind the
    start of the long segment at 4: elements 1027 | 1028 at offset 0; 1023 | 1024 for a table with one segment) and both sides of
    the segment boundaries at 3 and 4 - which are no multiples of four."""
    n, sizes = MID, [3, 0, 1, MID - 4]
    values = _values(n)
    for off in (0, 1):
        for pos in (0, n - 1, 1023, 1024, 1027, 1028, 2, 3, 4):
            v = values.clone()
            v[pos] = bad
            g = _Buf(v, off)
            tb = _Tables(n, sizes, step=5)
            want_counters = (0, -1, -1)
            for call_no, step in enumerate((5, 5, 8)):           # a skipped step does not advance the count; later steps do
                tb.state[0] = float(step)
                tb.run(g.ptr, 1.0, max_norm=1.0)
                stats, counters = tb.read()
                want, want_counters = GR.grad_stats(v.numpy(), tb.offsets, 1.0, 1.0, counters=want_counters, adam_step=step)
                assert stats[1] == 1 and stats[3] == 1 and stats[2] == 1.0, (pos, off, stats[:4])
                assert counters == want_counters == [call_no + 1, 6, step + 1], (pos, off, counters)
                seg_of_pos = 0 if pos < 3 else (2 if pos == 3 else 3)
                for k in range(4):                               # the segment that holds it has no finite norm, the others do
                    assert np.isfinite(stats[4 + k]) == (k != seg_of_pos), (pos, k, stats)
            tb.run(g.ptr, 1.0, max_norm=1.0, skip_nonfinite=0)   # counted, not skipped, counters untouched
            stats, counters = tb.read()
            assert stats[1] == 1 and stats[3] == 0 and counters == want_counters


def test_a_product_that_overflows_float32_counts_as_not_finite():
    v = torch.full((300,), 3e38)
    g, tb = _Buf(v, 1), _Tables(300, [300])
    tb.run(g.ptr, 2.0)                                           # Adam would see inf
    assert tb.read()[0][1] == 300 and tb.read()[0][3] == 1
    tb.run(g.ptr, 1.0)
    stats, _ = tb.read()
    assert stats[1] == 0 and stats[3] == 0 and abs(stats[0] - GR.grad_stats(v.numpy(), [0, 300])[0][0]) <= GR.norm_bound(300) * stats[0]


# ---- 3. coef == 1, no skip: the unguarded update, bit for bit ---------------------------------------------------------------------
def _adam_run(name, p0, grads, off, grad_scale, guarded_sizes=None, zero=True, max_norm=0.0):
    """Two consecutive steps of entry point ``name`` (or, with ``guarded_sizes``, of fd_grad_stats + fd_adam_step_guarded) ->
    [(p, m, v, g, state) after each step], the stats after each step; guard bands checked."""
    n = p0.numel()
    p, m, v, gr = _Buf(p0, off), _Buf(torch.zeros(n), off), _Buf(torch.zeros(n), off), _Buf(torch.zeros(n), off)
    state = torch.tensor([0.0, LR], device="cuda")
    tb = _Tables(n, guarded_sizes) if guarded_sizes is not None else None
    trace, stats = [], []
    for gk in grads:
        gr.t.copy_(gk)
        if tb is not None:
            tb.state = state
            tb.run(gr.ptr, grad_scale, max_norm)
            call("fd_adam_step_guarded", p.ptr, gr.ptr, m.ptr, v.ptr, n, state.data_ptr(), BETAS[0], BETAS[1], EPS, grad_scale,
                 tb.stats.data_ptr(), int(zero), stream())
            stats.append(tb.read())
        else:
            call(name, p.ptr, gr.ptr, m.ptr, v.ptr, n, state.data_ptr(), BETAS[0], BETAS[1], EPS, grad_scale, stream())
        trace.append([b.t.clone() for b in (p, m, v, gr)] + [state.clone()])
    for b, what in ((p, "param"), (m, "exp_avg"), (v, "exp_avg_sq"), (gr, "grad")):
        assert b.guards_intact(), "%s wrote outside %s[0 .. %d)" % (name, what, n)
    return trace, stats


def _assert_traces_equal(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        for x, y, name in zip(a, b, ("param", "exp_avg", "exp_avg_sq", "grad", "state")):
            assert _same(x, y), "%s, step %d: %s differs in %d of %d elements" % (what, k + 1, name, int((x != y).sum()), x.numel())


@pytest.mark.parametrize("n", SIZES)
def test_guarded_adam_with_coef_one_is_the_unguarded_update(n):
    gen = torch.Generator().manual_seed(17 * n + 3)
    p0, grads = torch.randn(n, generator=gen), [torch.randn(n, generator=gen) * 0.1 for _ in range(2)]
    for off in (0, 1):
        for grad_scale in (1.0, 0.25):
            for zero, name in ((True, "fd_adam_step_dev_zero"), (False, "fd_adam_step_dev")):
                want, _ = _adam_run(name, p0, grads, off, grad_scale)
                got, stats = _adam_run("guarded", p0, grads, off, grad_scale, guarded_sizes=_seg_tables(n)[-1], zero=zero)
                assert all(s[0][2] == 1.0 and s[0][3] == 0.0 and s[1] == [0, -1, -1] for s in stats)
                _assert_traces_equal(got, want, "%s off %d scale %g" % (name, off, grad_scale))
                assert float(got[1][4][0]) == 2.0
                if n and zero:
                    assert float(got[1][3].abs().max()) == 0.0 and not bool(torch.signbit(got[1][3]).any())
                elif n:
                    assert _same(got[1][3], grads[1].cuda())
    if n:
        assert not _same(got[0][0], p0.cuda()) and torch.isfinite(got[1][0]).all()


# ---- 4. clipping -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [0.5, 2.0, 100.0], ids=["half", "twice", "hundredfold"])
def test_clipping_is_the_unguarded_update_of_the_scaled_gradient(factor):
    n, max_norm = MID, 1.75
    gen = torch.Generator().manual_seed(99)
    p0 = torch.randn(n, generator=gen)
    for off, grad_scale in ((0, 1.0), (1, 0.25)):
        grads = []
        for _ in range(2):                                       # norm of g * grad_scale = factor * max_norm: well away from the clamp's edge
            g = torch.randn(n, generator=gen)
            grads.append(g * float(factor * max_norm / grad_scale / float(g.double().norm())))
        got, stats = _adam_run("guarded", p0, grads, off, grad_scale, guarded_sizes=[3, 0, 1, n - 4], zero=False, max_norm=max_norm)
        pre = []
        for gk, (st, counters) in zip(grads, stats):
            want, _ = GR.grad_stats(gk.numpy(), [0, 3, 3, 4, n], grad_scale, max_norm)
            _check_stats(st, want, n, [3, 0, 1, n - 4])
            coef64 = min(1.0, max_norm / (want[0] + 1e-6))
            assert st[2] <= 1.0 and (st[2] == 1.0) == (factor < 1.0) and abs(st[2] - coef64) <= 2.0 ** -23 * coef64, (st[2], coef64)
            assert st[2] == float(np.float32(st[2])) and counters == [0, -1, -1]
            pre.append(torch.from_numpy(GR.clipped(gk.numpy(), grad_scale, st[2])))
        want_trace, _ = _adam_run("fd_adam_step_dev", p0, pre, off, 1.0)
        for k in range(2):                                       # the gradient itself is left as it was; compare p, m, v and the state
            got[k][3] = want_trace[k][3]
        _assert_traces_equal(got, want_trace, "factor %g off %d scale %g" % (factor, off, grad_scale))


# ---- 5. the skip -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero", [True, False], ids=["zero_grad", "keep_grad"])
def test_a_skipped_step_changes_nothing_and_the_next_one_is_the_unskipped_step(zero):
    n, sizes = MID, [3, 0, 1, MID - 4]
    gen = torch.Generator().manual_seed(5)
    p0, grads = torch.randn(n, generator=gen), [torch.randn(n, generator=gen) * 0.1 for _ in range(3)]
    poisoned = grads[1].clone()
    poisoned[n // 2] = float("inf")
    name = "fd_adam_step_dev_zero" if zero else "fd_adam_step_dev"
    for off in (0, 1):
        want, _ = _adam_run(name, p0, [grads[0], grads[2]], off, 0.25)          # the optimiser that never saw the poisoned gradient
        got, stats = _adam_run("guarded", p0, [grads[0], poisoned, grads[2]], off, 0.25, guarded_sizes=sizes, zero=zero, max_norm=1000.0)   # far above the norm: coef 1
        assert [s[0][3] for s in stats] == [0.0, 1.0, 0.0] and [s[1] for s in stats] == [[0, -1, -1], [1, 2, 2], [1, 2, 2]]
        assert stats[1][0][1] == 1 and stats[1][0][2] == 1.0
        for x, y, what in zip(got[1][:3] + got[1][4:], got[0][:3] + got[0][4:], ("param", "exp_avg", "exp_avg_sq", "state")):
            assert _same(x, y), "the skipped step changed %s" % what
        assert float(got[1][4][0]) == 1.0
        if zero:
            assert float(got[1][3].abs().max()) == 0.0 and not bool(torch.signbit(got[1][3]).any()), "the poisoned gradient survived"
        else:
            assert _same(got[1][3], poisoned.cuda())
        _assert_traces_equal([got[0], got[2]], want, "off %d" % off)


# ---- 6. capture --------------------------------------------------------------------------------------------------------------------
def test_the_two_calls_replay_from_a_captured_graph():
    n, sizes = 1000, [3, 0, 1, 996]
    gen = torch.Generator().manual_seed(11)
    p0, grads = torch.randn(n, generator=gen), [torch.randn(n, generator=gen) * 0.1 for _ in range(3)]
    grads[1][123] = float("nan")

    def fresh():
        bufs = [_Buf(p0, 1), _Buf(torch.zeros(n), 1), _Buf(torch.zeros(n), 1), _Buf(torch.zeros(n), 1)]
        return bufs, _Tables(n, sizes)

    def issue(bufs, tb):
        p, m, v, gr = bufs
        tb.run(gr.ptr, 0.5, 1.0)
        call("fd_adam_step_guarded", p.ptr, gr.ptr, m.ptr, v.ptr, n, tb.state.data_ptr(), BETAS[0], BETAS[1], EPS, 0.5, tb.stats.data_ptr(), 1,
             stream())

    def snapshot(bufs, tb):
        return [b.t.clone() for b in bufs] + [tb.state.clone(), tb.counters.clone(), tb.stats.clone()]

    eager = []
    bufs, tb = fresh()
    for gk in grads:
        bufs[3].t.copy_(gk)
        issue(bufs, tb)
        eager.append(snapshot(bufs, tb))
    assert tb.read()[1] == [1, 2, 2] and float(tb.state[0]) == 2.0

    bufs, tb = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                # a linear graph: no parallel branches
        issue(bufs, tb)
    torch.cuda.synchronize()
    assert float(tb.state[0]) == 0.0 and _same(bufs[0].t, p0.cuda()), "capturing ran the kernels"
    for k, gk in enumerate(grads):
        bufs[3].t.copy_(gk)
        graph.replay()
        torch.cuda.synchronize()
        for x, y, what in zip(snapshot(bufs, tb), eager[k], ("param", "exp_avg", "exp_avg_sq", "grad", "state", "counters", "stats")):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), "replay %d: %s differs from the eager step" % (k + 1, what)
    assert tb.read()[1] == [1, 2, 2] and all(b.guards_intact() for b in bufs)


# ---- 7. the Trainer ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batches():
    out = []
    for i in range(3):
        inp, noise = TT._batch(2, 64, 96, 1500 + i)
        g = {k: v.cuda() for k, v in inp.items()}
        g["_noise"] = [t.cuda() for t in noise]
        out.append(g)
    return out


def _trainer(tmp_path=None, **attrs):
    from fusiondepth_amd.trainer import Trainer
    torch.manual_seed(4321)                                      # the same initial weights for every trainer of this file
    tr = Trainer(TT._opts(batch_size=2, **({} if tmp_path is None else {"log_dir": str(tmp_path)})), verbose=False)
    for k, v in attrs.items():
        setattr(tr, k, v)
    assert tr.accumulate_step == 1
    return tr


def _manual_step(tr, batch, before_optimizer="step"):
    """``Trainer.train_step`` of one batch, written out so that something can happen between the backward pass and the optimiser:
    "nan" writes one into the gradient first, "zero" clears the gradient instead of stepping."""
    inputs, outputs, losses = tr._forward_backward(batch, eager=True)
    if before_optimizer == "nan":
        tr.flat.flat_grad[tr.flat.numel() // 3] = float("nan")
    if before_optimizer == "zero":
        tr.flat.zero_grad()
    else:
        tr.optimizer_step(1.0)
    tr._ensure_weight_plan()
    tr.step += tr.accumulate_step
    tr.last_losses = losses
    return losses


def _state_of(tr):
    torch.cuda.synchronize()
    return [tr.flat.flat_param.clone(), tr.optim.exp_avg.clone(), tr.optim.exp_avg_sq.clone()]


def _drop(tr):
    FD.sync_late_layouts()
    del tr


def test_trainer_with_the_guard_on_and_finite_gradients_is_the_trainer_without(batches, monkeypatch):
    used = []
    real = FD.call
    monkeypatch.setattr(FD, "call", lambda name, *a: (used.append(name) if ("adam" in name or "grad_stats" in name) else None, real(name, *a))[1])
    result, calls = {}, {}
    for mode in ("off", "skip"):
        del used[:]
        tr = _trainer(grad_guard=mode)
        for g in batches:
            tr.train_step([g])
        result[mode], calls[mode] = _state_of(tr), list(used)
        assert float(tr.flat.flat_grad.abs().max()) == 0.0 and float(tr.optim.state[0]) == 3.0
        if mode == "skip":
            rep = tr.guard_report()
            assert rep["skipped_steps"] == 0 and rep["first_skipped_step"] == rep["last_skipped_step"] == -1 and rep["nonfinite"] == 0
            assert rep["clip_coef"] == 1.0 and rep["grad_norm"] > 0 and set(rep) >= {"grad_norm/%s" % k for k in tr.trained}
            norms = [rep["grad_norm/%s" % k] for k in tr.trained]
            assert abs(rep["grad_norm"] - float(np.sqrt(np.sum(np.square(norms))))) <= 1e-12 * rep["grad_norm"]
        else:
            assert tr.guard_report() == {} and tr.guard_summary() is None and tr.optim.guard_stats is None
        _drop(tr)
    assert calls["off"] == ["fd_adam_step_dev_zero"] * 3, calls["off"]           # exactly today's launches
    assert calls["skip"] == ["fd_grad_stats", "fd_adam_step_guarded"] * 3, calls["skip"]
    for a, b, what in zip(result["off"], result["skip"], ("param", "exp_avg", "exp_avg_sq")):
        assert _same(a, b), "%s: %d elements differ with the guard on" % (what, int((a != b).sum()))


def test_trainer_skips_the_step_whose_gradient_holds_a_nan(batches, tmp_path):
    # what the guard is for: without it the same NaN reaches the parameters and both moments
    bare = _trainer()
    _manual_step(bare, batches[0])
    _manual_step(bare, batches[1], "nan")
    torch.cuda.synchronize()
    assert bool(torch.isnan(bare.flat.flat_param).any()) and bool(torch.isnan(bare.optim.exp_avg).any())
    _drop(bare)

    # the run that zeroed the gradient instead of stepping at step 2
    ref = _trainer()
    for g, what in zip(batches, ("step", "zero", "step")):
        _manual_step(ref, g, what)
    want = _state_of(ref)
    assert float(ref.optim.state[0]) == 2.0
    _drop(ref)

    tr = _trainer(tmp_path, grad_guard="skip")
    for g, what in zip(batches, ("step", "nan", "step")):
        losses = _manual_step(tr, g, what)
    for a, b, what in zip(_state_of(tr), want, ("param", "exp_avg", "exp_avg_sq")):
        assert _same(a, b), "%s: %d elements differ from the run that zeroed the gradient" % (what, int((a != b).sum()))
    assert bool(torch.isfinite(tr.flat.flat_param).all()) and float(tr.flat.flat_grad.abs().max()) == 0.0
    rep = tr.guard_report()
    assert (rep["skipped_steps"], rep["first_skipped_step"], rep["last_skipped_step"]) == (1, 2, 2) and rep["nonfinite"] == 0
    assert tr.step == 3 and float(tr.optim.state[0]) == 2.0                      # three batches consumed, two Adam steps taken
    assert all(float(e["step"]) == 2.0 for e in tr.optimizer_state_dict()["state"].values())
    assert tr.guard_summary() == {"mode": "skip", "max_norm": 0.0, "skipped_steps": 1, "first_skipped_step": 2, "last_skipped_step": 2}

    # (c) the log carries the report; more skipped steps than max_skipped_steps stop the run at the log event
    tr.log("train", {"loss": losses["loss"].detach()})
    rec = json.loads(open(os.path.join(tr.log_path, "train", "scalars.jsonl")).read().splitlines()[-1])
    assert rec["skipped_steps"] == 1 and rec["grad_norm"] > 0 and rec["clip_coef"] == 1.0 and "grad_norm/encoder" in rec
    tr.max_skipped_steps = 0
    with pytest.raises(RuntimeError, match=r"1 optimiser steps were skipped.*first was optimiser step 2, the last 2"):
        tr.log("train", {"loss": losses["loss"].detach()})
    with pytest.raises(RuntimeError, match="max_skipped_steps = 0"):
        tr.check_skipped_steps()
    tr.max_skipped_steps = 10

    # (d) the counters travel in the run state; a run state without them reads as "nothing skipped"
    folder = tr.save_model()
    path = tr.save_run_state(folder)
    assert float(torch.load(os.path.join(folder, "adam.pth"))["state"][0]["step"]) == 2.0
    params = tr.flat.flat_param.clone()
    _drop(tr)
    again = _trainer(tmp_path, grad_guard="skip")
    again.resume(folder, None)
    rep = again.guard_report()
    assert (rep["skipped_steps"], rep["first_skipped_step"], rep["last_skipped_step"]) == (1, 2, 2)
    assert float(again.optim.state[0]) == 2.0 and again.step == 3 and _same(again.flat.flat_param, params)
    state = torch.load(path)
    for k in ("skipped_steps", "first_skipped_step", "last_skipped_step"):
        del state[k]
    torch.save(state, path)
    again.resume(folder, None)
    assert again.optim.guard_counters_host() == [0, -1, -1]
    _drop(again)


# ---- 8. two ranks, one of which meets an inf ---------------------------------------------------------------------------------------
def test_two_ranks_take_the_same_decision_without_another_collective(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "guard_dp")
    env = dict(os.environ, FD_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(HERE, "guard_dp_worker.py"), out]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:]
    r0, r1 = [json.load(open(out + ".%d" % k)) for k in range(2)]
    assert r0["injected"] is False and r1["injected"] is True                    # rank 1 alone met the inf, before the exchange
    for r in (r0, r1):
        assert r["report"]["skipped_steps"] == 1 and r["report"]["first_skipped_step"] == r["report"]["last_skipped_step"] == 1
        assert r["report"]["nonfinite"] >= 1 and r["unchanged"] and r["grad_zero"] and r["device_step"] == 0.0
        assert r["after"] == r["before"] and r["finite"]
        assert r["device_step_next"] == 1.0 and r["moved_next"] and r["finite_next"]
    assert r0["before"] == r1["before"] and r0["after"] == r1["after"] and r0["after_next"] == r1["after_next"]
    assert r0["stats_bits"] == r1["stats_bits"]                  # the same float64 bits on both ranks: the same decision


# ---- 9. the command ----------------------------------------------------------------------------------------------------------------
def test_train_command_with_clip_grad_norm(tmp_path):
    import kitti_tree
    from fusiondepth_amd import train as T
    root, splits = str(tmp_path / "kitti"), str(tmp_path / "splits")
    os.makedirs(root)
    lines = kitti_tree.make_tree(root, [("2011_09_26", "2011_09_26_drive_0001_sync", (375, 1242), (1.0, 1.0))], frames=6, down=0.35)
    os.makedirs(os.path.join(splits, "eigen_zhou"))
    with open(os.path.join(splits, "eigen_zhou", "train_files.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    tr = T.main(["--num_layers", "18", "--weights_init", "scratch", "--height", "192", "--width", "640", "--batch_size", "2", "--data_path", root,
                 "--png", "--log_dir", str(tmp_path), "--num_workers", "4", "--model_name", "clip", "--num_epochs", "1", "--log_frequency", "1",
                 "--splits_dir", splits, "--seed", "5", "--no_val", "--clip_grad_norm", "1.0"])
    assert (tr.grad_guard, tr.clip_grad_norm, tr.max_skipped_steps) == ("skip", 1.0, 10)
    log = os.path.join(str(tmp_path), "clip")
    summary = json.load(open(os.path.join(log, "train_summary.rank0.json")))
    assert summary["steps"] == 2 and np.isfinite(summary["param_checksum"]).all()
    assert summary["grad_guard"] == {"mode": "skip", "max_norm": 1.0, "skipped_steps": 0, "first_skipped_step": -1, "last_skipped_step": -1}
    scalars = [json.loads(l) for l in open(os.path.join(log, "train", "scalars.jsonl"))]
    assert len(scalars) == 2
    for rec in scalars:
        assert rec["grad_norm"] > 0 and np.isfinite(rec["grad_norm"]) and rec["nonfinite"] == 0 and rec["skipped_steps"] == 0
        want = float(np.float32(min(1.0, 1.0 / (rec["grad_norm"] + 1e-6))))
        assert rec["clip_coef"] == want and all(("grad_norm/%s" % k) in rec for k in tr.trained)
