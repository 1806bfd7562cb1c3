"""fd_adam_step_dev_zero - the Adam update that clears the gradient it has read - against fd_adam_step_dev followed by a fill, bit for
bit, and the trainer's optimiser step with ``tuning.host.adam_zero`` on and off."""
import pytest
import torch

import test_gpu_trainer as TT
from fusiondepth_amd import functional as FD
from fusiondepth_amd._lib import call, ptr, stream

pytestmark = pytest.mark.gpu

BETAS, EPS, LR = (0.9, 0.999), 1e-8, 1.5e-4
GUARD = 8                                     # floats on either side of a buffer that no kernel may touch


class _Buf:
    """n floats at `off` floats past a 16-byte boundary, between two guard bands"""

    def __init__(self, values, off):
        n = values.numel()
        self.raw = torch.full((GUARD + off + n + GUARD,), 12345.0, device="cuda")
        self.t = self.raw[GUARD + off:GUARD + off + n]
        self.t.copy_(values)
        assert self.t.data_ptr() % 16 == 4 * off
        self.lo, self.hi = GUARD + off, GUARD + off + n

    def guards_intact(self):
        return bool((self.raw[:self.lo] == 12345.0).all()) and bool((self.raw[self.hi:] == 12345.0).all())


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "one-float-past"])
@pytest.mark.parametrize("n", [1, 3, 4, 1023, (1 << 20) + 5])
def test_adam_step_dev_zero_is_adam_step_dev_then_fill(n, off, grad_scale):
    g = torch.Generator(device="cuda").manual_seed(31 * n + off)
    rnd = lambda scale: torch.randn(n, generator=g, device="cuda") * scale
    p0, grads = rnd(1.0), [rnd(0.1), rnd(0.1)]
    runs = {}
    for name in ("fd_adam_step_dev", "fd_adam_step_dev_zero"):
        p, m, v = _Buf(p0, off), _Buf(torch.zeros(n), off), _Buf(torch.zeros(n), off)
        gr = _Buf(torch.zeros(n), off)
        state = torch.tensor([0.0, LR], device="cuda")
        trace = []
        for k, gk in enumerate(grads):                          # two consecutive steps
            gr.t.copy_(gk)
            call(name, ptr(p.t), ptr(gr.t), ptr(m.t), ptr(v.t), n, ptr(state), BETAS[0], BETAS[1], EPS, grad_scale, stream())
            if name == "fd_adam_step_dev":
                assert _same(gr.t, gk), "fd_adam_step_dev changed the gradient"
                gr.t.zero_()
            torch.cuda.synchronize()
            assert float(gr.t.abs().max()) == 0.0 and not bool(torch.signbit(gr.t).any()), "%s: gradient not all +0 after step %d" % (name, k + 1)
            assert state.tolist() == [float(k + 1), float(torch.tensor(LR, dtype=torch.float32))], "%s: step counter / lr after step %d" % (name, k + 1)
            trace.append([b.t.clone() for b in (p, m, v)])
        for b, what in ((p, "param"), (m, "exp_avg"), (v, "exp_avg_sq"), (gr, "grad")):
            assert b.guards_intact(), "%s wrote outside %s[0 .. %d)" % (name, what, n)
        runs[name] = trace
    for k in range(2):
        for a, b, what in zip(runs["fd_adam_step_dev"][k], runs["fd_adam_step_dev_zero"][k], ("param", "exp_avg", "exp_avg_sq")):
            assert _same(a, b), "step %d: %s differs in %d of %d elements" % (k + 1, what, int((a != b).sum()), n)
    assert not _same(runs["fd_adam_step_dev"][0][0], p0) and torch.isfinite(runs["fd_adam_step_dev_zero"][1][0]).all()


def test_adam_step_dev_zero_of_no_elements_still_counts_the_step():
    p, gr, m, v = (torch.zeros(4, device="cuda") for _ in range(4))
    state = torch.tensor([7.0, LR], device="cuda")
    call("fd_adam_step_dev_zero", ptr(p), ptr(gr), ptr(m), ptr(v), 0, ptr(state), BETAS[0], BETAS[1], EPS, 1.0, stream())
    assert float(state[0]) == 8.0


def test_trainer_optimizer_step_with_and_without_adam_zero(fdtune, monkeypatch):
    """Three optimiser steps of the small Trainer configuration: the same parameters bit for bit whether Adam clears the gradient
    or a fill of its own does, and an all-zero gradient buffer after every step in both modes."""
    from fusiondepth_amd.trainer import Trainer
    B, H, W = 2, 64, 96
    batches = []
    for i in range(3):
        inp, noise = TT._batch(B, H, W, 1500 + i)
        g = {k: v.cuda() for k, v in inp.items()}
        g["_noise"] = [n.cuda() for n in noise]
        batches.append(g)
    used = []
    real = FD.call
    monkeypatch.setattr(FD, "call", lambda name, *a: (used.append(name) if "adam" in name else None, real(name, *a))[1])
    params, calls = {}, {}
    for mode in (True, False):
        fdtune.host(adam_zero=mode)
        del used[:]
        torch.manual_seed(4321)                                  # the same initial weights for both trainers
        tr = Trainer(TT._opts(batch_size=B), verbose=False)
        for g in batches:
            tr.train_step([g])
            torch.cuda.synchronize()
            assert float(tr.flat.flat_grad.abs().max()) == 0.0, "adam_zero=%s: gradient buffer not zero after the step" % mode
            for p, o in zip(tr.flat.params, tr.flat.offsets):
                assert p.grad.data_ptr() == tr.flat.flat_grad.data_ptr() + 4 * o
        params[mode], calls[mode] = tr.flat.flat_param.clone(), list(used)
        FD.sync_late_layouts()
        del tr
    assert calls[True] == ["fd_adam_step_dev_zero"] * 3 and calls[False] == ["fd_adam_step_dev"] * 3, calls
    assert torch.isfinite(params[True]).all()
    assert torch.equal(params[True], params[False]), "%d parameters differ" % int((params[True] != params[False]).sum())
