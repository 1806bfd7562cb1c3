"""The data-parallel exchange under ProcessGroupNCCL's STREAM semantics, on one GPU.

RCCL (torch backend "nccl") has never executed this code on the builder's side - only 1-GPU boxes - and gloo (host-staged, in
effect synchronous) exercises none of what dp.GradientSynchronizer relies on:
  * a collective is enqueued on the communicator's OWN stream, which first waits on an event recorded on the caller's CURRENT
    stream at call time (so the reduce is ordered behind the kernel that finished the bucket - on whichever module stream the
    backward node ran);
  * an asynchronous call returns a Work immediately; ``Work.wait()`` makes the then-current stream wait for the communicator
    stream (no host block); a synchronous call does the same before returning;
  * nothing else orders the communicator stream against the streams of the step.
``_FakeNccl`` reproduces exactly that with a private HIP stream and, for two identical replicas, the exact arithmetic of the sum
(x + x = 2x), and it holds its stream back by ~50 ms of queued matrix products in front of every step, so that any consumer that
does not go through ``wait()`` (the optimiser reading a bucket that is still being reduced, a bucket leaving before the kernel that
completes it) reads wrong data.  With 2x summed and 1/world folded into Adam the result must equal the single-process run BIT FOR
BIT; the overlapped buckets and the one whole-buffer exchange must agree bit for bit as well - for ``Trainer`` (eager and graphed
step) and ``Refiner``.

What stays untested without a multi-GPU node: link bandwidth, the 8-rank overlap fraction, RCCL's own kernels."""
import os
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu


class _Work:
    def __init__(self, event):
        self.event = event

    def wait(self):
        torch.cuda.current_stream().wait_event(self.event)
        return True

    def is_completed(self):
        return self.event.query()


class _FakeNccl:
    """``all_reduce(sum)`` of two identical replicas with ProcessGroupNCCL's stream behaviour."""

    def __init__(self):
        self.comm = torch.cuda.Stream()
        self.junk = torch.randn(4096, 4096, device="cuda")
        self.calls = []                      # (numel, async?, raw stream the call was made on)

    def hold_back(self, n=40):
        with torch.cuda.stream(self.comm):
            for _ in range(n):
                self.junk @ self.junk

    def all_reduce(self, tensor, op=None, group=None, async_op=False):
        cur = torch.cuda.current_stream()
        ready = torch.cuda.Event()
        ready.record(cur)                                        # ncclStream waits for the caller's stream AS OF NOW
        self.comm.wait_event(ready)
        with torch.cuda.stream(self.comm):
            tensor.mul_(2.0)                                     # x + x
            tensor.record_stream(self.comm)
        done = torch.cuda.Event()
        done.record(self.comm)
        self.calls.append((tensor.numel(), bool(async_op), cur.cuda_stream))
        work = _Work(done)
        if async_op:
            return work
        work.wait()
        return None


def _patch(monkeypatch, fake):
    import torch.distributed as dist
    from fusiondepth_amd import dp
    monkeypatch.setattr(dp.dist, "all_reduce", fake.all_reduce)
    assert dist.all_reduce == fake.all_reduce                   # graph_step._sync_and_step imports torch.distributed itself


def _opts(B=2, H=64, W=96, extra=()):
    from fusiondepth_amd.options import MonodepthOptions
    return MonodepthOptions().parse(["--num_layers", "18", "--weights_init", "scratch", "--batch_size", str(B), "--height", str(H),
                                     "--width", str(W)] + list(extra))


def _batches(n, B, H, W):
    from fusiondepth_amd import synthetic
    out = []
    for i in range(n):
        b = synthetic.make_batch(B, H, W, seed=2100 + i)
        g = torch.Generator(device="cuda"); g.manual_seed(50 + i)
        b["_noise"] = [torch.randn(B, 2, H, W, device="cuda", generator=g) for _ in range(4)]
        out.append(b)
    return out


def _run_trainer(world, overlap, fake, fdtune, graphed=False, steps=3):
    from fusiondepth_amd.trainer import Trainer
    fdtune.host(dp_overlap=overlap)
    torch.manual_seed(777)
    tr = Trainer(_opts(), rank=0, world_size=world, verbose=False)
    assert tr.accumulate_step == 1
    n_over = []
    for b in _batches(steps, 2, 64, 96):
        if fake is not None:
            fake.hold_back()
        if graphed:
            tr.train_step_graphed([b])
        else:
            tr.train_step([b])
        n_over.append(tr.grad_sync.n_overlapped)
    torch.cuda.synchronize()
    p = tr.flat.flat_param.clone()
    nb = len(tr.grad_sync.buckets)
    del tr
    return p, n_over, nb


def test_trainer_under_nccl_stream_semantics_matches_the_single_process_run(monkeypatch, fdtune):
    fake = _FakeNccl()
    _patch(monkeypatch, fake)
    solo, _, _ = _run_trainer(1, True, None, fdtune)
    assert not fake.calls
    over, n_over, nb = _run_trainer(2, True, fake, fdtune)
    calls_over = list(fake.calls)
    assert all(n == nb for n in n_over) and nb >= 6, (n_over, nb)           # every bucket left from inside the backward pass ...
    assert all(a for _, a, _ in calls_over) and len(calls_over) == 3 * nb     # ... asynchronously
    assert len({s for _, _, s in calls_over}) >= 3, "the buckets were expected to leave from several module streams"
    fake.calls.clear()
    whole, n_whole, _ = _run_trainer(2, False, fake, fdtune)
    assert n_whole == [0, 0, 0] and len(fake.calls) == 3 and not any(a for _, a, _ in fake.calls)
    assert torch.isfinite(solo).all() and float((solo - over).abs().max()) == 0.0, "overlapped buckets: %d entries differ from the " \
        "single-process parameters" % int((solo != over).sum())
    assert torch.equal(over, whole)


def test_graphed_step_with_an_eager_exchange_behind_it(monkeypatch, fdtune):
    """train_step_graphed with world_size > 1: forward / backward replayed from the hipGraph, all-reduce + Adam + the (late,
    side-stream) re-layout eager behind it - the path ADVICE round 3 found unordered against the next replay."""
    from fusiondepth_amd import functional as FD, weight_layouts as WL
    fake = _FakeNccl()
    _patch(monkeypatch, fake)
    solo, _, _ = _run_trainer(1, True, None, fdtune, graphed=True, steps=5)
    late = []
    orig = FD.refresh_weight_layouts

    def held_back():
        # queue ~50 ms in front of the side-stream re-layout this refresh is about to issue
        if WL.late_stream() is not None and not torch.cuda.is_current_stream_capturing():
            with torch.cuda.stream(WL.late_stream()):
                for _ in range(40):
                    fake.junk @ fake.junk
        r = orig()
        late.append(WL.late_event() is not None)
        return r
    monkeypatch.setattr(FD, "refresh_weight_layouts", held_back)          # the refresh behind every Adam launch ...
    monkeypatch.setattr(WL, "refresh_weight_layouts", held_back)          # ... and the one that follows the first plan
    dp2, _, _ = _run_trainer(2, True, fake, fdtune, graphed=True, steps=5)
    assert sum(late) >= 2, "the side-stream re-layout never ran behind a graph replay"
    assert torch.equal(solo, dp2), "%d entries differ" % int((solo != dp2).sum())


def test_refiner_under_nccl_stream_semantics(monkeypatch, fdtune):
    """The Refiner's optimiser step (frozen stage-1 networks, refine decoder trained, refiner.py:264-297) under the same stub; set up
    like tests/test_gpu_refiner.py (seeded networks whose disparity heads stay away from saturation, 192x640)."""
    import inputs as gin
    from oracle import refiner as OR
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.refiner import Refiner
    B, H, W = 1, 192, 640
    oopt = OR.default_opt(batch_size=B, height=H, width=W)
    omodels = gin.refiner_models(OR.build_models(oopt, 0))
    folder = tempfile.mkdtemp(prefix="fd_stage1_")
    for k, m in omodels.items():
        sd = {n: v.detach().clone() for n, v in m.state_dict().items()}
        if k == "encoder":
            sd.update(height=H, width=W, use_stereo=False)
        torch.save(sd, "%s/%s.pth" % (folder, k))
    fake = _FakeNccl()
    _patch(monkeypatch, fake)
    res = {}
    for tag, world, overlap in (("solo", 1, True), ("overlap", 2, True), ("whole", 2, False)):
        fdtune.host(dp_overlap=overlap)
        o = MonodepthOptions().parse(["--num_layers", "18", "--weights_init", "scratch", "--batch_size", str(B), "--height", str(H), "--width", str(W),
                                      "--refine_load_weights_folder", folder])
        rf = Refiner(o, rank=0, world_size=world, verbose=False)
        for i in range(3):
            inp, noise = gin.refiner_inputs(820 + i, B, H, W)
            ginp = {k: v.cuda() for k, v in inp.items()}
            ginp["_noise"] = [n.cuda() for n in noise]
            if world > 1:
                fake.hold_back()
            rf.train_step(ginp)
        torch.cuda.synchronize()
        res[tag] = rf.flat.flat_param.clone()
        del rf
    assert len(fake.calls) >= 6
    assert torch.isfinite(res["solo"]).all()
    assert torch.equal(res["solo"], res["overlap"]), "%d entries differ" % int((res["solo"] != res["overlap"]).sum())
    assert torch.equal(res["overlap"], res["whole"])
