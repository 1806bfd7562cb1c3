"""Which loss kernels a ``--use_stereo`` step runs: the all-scales kernel (fd_photo_ms_*, one / three source frames) by default,
the per-scale kernels (fd_photo_fwd_ex / fd_photo_bwd_ex) with ``tuning.host.photo_ms`` off - the route of these configurations
before the all-scales kernel took one and three frames - and that both routes give the same loss.  The default three-frame mono
configuration runs fd_photo_ms_* as well; the separate fd_photo_msn_* entry points of the first stereo kernel are gone."""
import pytest
import torch

from fusiondepth_amd import _lib
from test_gpu_ablations import B, H, W, _batch, _opts

pytestmark = pytest.mark.gpu


def _step(monkeypatch, over, seed):
    """process_batch + backward of a fresh Trainer (same seed: same weights) on the ablation test's batch -> (names passed to
    loss_ops.call, total loss)."""
    from fusiondepth_amd import loss_ops
    from fusiondepth_amd.trainer import Trainer
    torch.manual_seed(seed)
    tr = Trainer(_opts(**over), verbose=False)
    inp, noise = _batch(4242, list(tr.opt.frame_ids))
    ginp = {k: v.cuda() for k, v in inp.items()}
    ginp["_noise"] = [n.cuda() for n in noise]
    called = []
    real_call = loss_ops.call
    with monkeypatch.context() as m:
        m.setattr(loss_ops, "call", lambda name, *a: (called.append(name), real_call(name, *a))[1])
        tr.flat.zero_grad()
        _, losses = tr.process_batch(ginp)
        losses["loss"].backward()
        tr._join_side_streams()
        torch.cuda.synchronize()
    return called, float(losses["loss"])


@pytest.mark.parametrize("over", [dict(use_stereo=True), dict(use_stereo=True, frame_ids=[0])], ids=["stereo+mono", "stereo-only"])
def test_stereo_step_runs_the_fused_kernel_and_matches_the_per_scale_route(monkeypatch, fdtune, over):
    fused, loss_fused = _step(monkeypatch, over, 11)
    assert fused.count("fd_photo_ms_fwd") == 1 and fused.count("fd_photo_ms_bwd") == 1, fused
    assert "fd_photo_fwd_ex" not in fused and "fd_photo_bwd_ex" not in fused
    assert not [k for k in _lib.SIGNATURES if k.startswith("fd_photo_msn")]      # the old entry points cannot quietly come back
    fdtune.host(photo_ms=False)
    per_scale, loss_per_scale = _step(monkeypatch, over, 11)
    assert per_scale.count("fd_photo_fwd_ex") == 4 and per_scale.count("fd_photo_bwd_ex") == 4, per_scale
    assert "fd_photo_ms_fwd" not in per_scale and "fd_photo_ms_bwd" not in per_scale
    print("total loss: fused %.9g, per-scale %.9g" % (loss_fused, loss_per_scale))
    assert abs(loss_fused - loss_per_scale) <= 2e-4 * abs(loss_per_scale), (loss_fused, loss_per_scale)


def test_default_mono_step_stays_on_the_two_frame_kernel(monkeypatch):
    called, _ = _step(monkeypatch, {}, 11)
    assert called.count("fd_photo_ms_fwd") == 1 and called.count("fd_photo_ms_bwd") == 1, called
    assert "fd_photo_fwd_ex" not in called
    assert not [k for k in _lib.SIGNATURES if k.startswith("fd_photo_msn")]      # the old entry points cannot quietly come back
