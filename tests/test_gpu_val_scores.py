"""The training-time scorer on the device (``fd_val_scores`` through ``validation.ValGroundTruth`` / ``validation.val_scores``) against its
numpy restatement (tests/val_ref.py, pinned to torch on the CPU by tests/test_train_cli_cpu.py): six images of every kind in one call,
more than one chunk, descriptors that leave the buffers.

The distance of the kernel's metrics to torch's own float32 ``.mean()`` values is printed in the terminal summary, not asserted: torch
sums float32 terms in float32 and takes float32 logarithms, the kernel sums the same terms in float64."""
import numpy as np
import pytest
import torch

import conftest
import val_ref
from conftest import assert_close

pytestmark = pytest.mark.gpu

# 1e-9: n <= 2.6e5 float64 additions of positive terms differ between two summation orders by at most about n * 2^-53 = 3e-11
# relative; the bound fd_eigen_scores is held to for the same construction
SUM_RTOL = 1e-9


def _bits(x):
    """The bit patterns of float32 values; every NaN counts as the same one."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    return np.where(np.isnan(x), np.float32(np.nan), x).view(np.uint32)


def _medians(vg, n):
    """The (median(gt), median(pred)) table of the latest single-chunk call, read from the workspace (score_lists.h: n x 32 x 7 float64
    partials, n x 16 bytes of list positions, then n x 2 float32 medians)."""
    at = n * (32 * 7 * 8 + 16)
    return vg.ws[at:at + n * 8].cpu().numpy().view(np.float32).reshape(n, 2)


def _check(per, ratios, counts, want, rows, what):
    assert np.array_equal(counts[rows], want["counts"]), (what, counts[rows], want["counts"])
    assert np.array_equal(_bits(ratios[rows]), _bits(want["ratios"])), (what, ratios[rows], want["ratios"])
    got, some = per[rows], want["counts"] > 0
    tc = np.rint(got[some, 4:] * want["counts"][some, None]).astype(np.int64)
    assert np.array_equal(tc, want["thresh_counts"][some]), (what, tc, want["thresh_counts"][some])
    assert np.abs(got[some, 4:] * want["counts"][some, None] - tc).max(initial=0) < 1e-6
    assert_close(got[:, :4], want["metrics"][:, :4], rtol=SUM_RTOL, atol=0, what=what + ": abs_rel / sq_rel / rmse / rmse_log")
    assert np.array_equal(np.isnan(got), np.isnan(want["metrics"]))


def test_six_images_in_one_call():
    from fusiondepth_amd import validation as V
    depths, gts, want = val_ref.six_case()
    vg = V.ValGroundTruth(gts, gap=[1, 2, 2, 2, 2, 2])           # the planes are even in size: every one at an odd element offset
    assert all(int(d["offset"]) % 2 == 1 for d in vg.desc) and len(vg.chunks) == 1
    dev = torch.from_numpy(depths.copy()).cuda()                # the shared case is read-only
    per, ratios, counts = V.val_scores(dev, vg)
    first = vg.out.cpu().numpy().copy()
    assert per.shape == (6, 7) and per.dtype == np.float64 and ratios.dtype == np.float32 and counts.dtype == np.int64
    assert counts.tolist() == want["counts"].tolist() and counts[2] == counts[3] == 0 and counts[5] == 251354
    assert counts[0] % 2 == 0 and counts[1] % 2 == 1
    _check(per, ratios, counts, want, slice(None), "six images")
    med = _medians(vg, 6)
    assert np.array_equal(_bits(med[:, 0]), _bits(want["med_gt"])) and np.array_equal(_bits(med[:, 1]), _bits(want["med_pred"]))
    # nothing selected: NaN metrics, NaN ratio, count 0; a NaN prediction: what torch gives
    assert np.isnan(per[2:4]).all() and np.isnan(ratios[2:4]).all()
    assert np.isnan(per[4, :4]).all() and (per[4, 4:] == 0).all() and np.isnan(ratios[4]) and counts[4] > 0
    # two calls give identical bits
    V.val_scores(dev, vg)
    assert np.array_equal(vg.out.cpu().numpy().view(np.uint64), first.view(np.uint64))
    # a list of maps instead of the resident object: packed back to back, the same rows
    per2, ratios2, counts2 = V.val_scores(dev, gts)
    assert np.array_equal(per2.view(np.uint64), per.view(np.uint64)) and np.array_equal(counts2, counts)
    # against the reference's float32 means (reported, not asserted)
    for i in (0, 1, 5):
        ref = val_ref.torch_reference(depths[i], gts[i])
        assert ref["count"] == counts[i]
        rel = np.abs(per[i] - ref["metrics"]) / np.abs(ref["metrics"])
        conftest.report("fd_val_scores vs torch float32 .mean(), image %d (n = %d), worst of 7 (rel)" % (i, counts[i]), rel.max(), np.inf,
                        "(reported only)")


def test_more_than_one_chunk():
    """130 maps of 40 x 100 with an explicit window: three calls (64 + 64 + 2); the rows at the chunk boundaries."""
    from fusiondepth_amd import validation as V
    rng = np.random.default_rng(130)
    window, rows = (5, 37, 4, 90), [63, 64, 65, 129]
    depths = val_ref.depth_pred(rng, 130)
    gts = [val_ref.sparse_gt(rng, 40, 100, valid=0.3) for _ in range(130)]
    vg = V.ValGroundTruth(gts, window=window)
    assert [(a, b) for a, b, _, _ in vg.chunks] == [(0, 64), (64, 128), (128, 130)]
    per, ratios, counts = V.val_scores(torch.from_numpy(depths).cuda(), vg)
    want = val_ref.val_scores(depths[rows], [gts[i] for i in rows], window)
    assert (want["counts"] > 500).all()
    _check(per, ratios, counts, want, rows, "chunk boundaries")
    assert (counts > 0).all() and np.isfinite(per).all()


def test_bad_descriptors_give_count_minus_one():
    from fusiondepth_amd import validation as V
    rng = np.random.default_rng(4)
    window = (5, 37, 4, 90)
    depths = torch.from_numpy(val_ref.depth_pred(rng, 4)).cuda()
    gts = [val_ref.sparse_gt(rng, 40, 100, valid=0.3) for _ in range(4)]
    vg = V.ValGroundTruth(gts, window=window)
    clean = V.val_scores(depths, vg)
    bad = vg.desc.copy()
    bad["offset"][1] = vg.packed.numel() - 10                    # the plane leaves the packed buffer
    bad["pred"][2] = 4                                           # no such prediction
    vg.desc_dev = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
    per, ratios, counts = V.val_scores(depths, vg)
    assert counts[1] == counts[2] == -1 and np.isnan(per[1:3]).all() and np.isnan(ratios[1:3]).all()
    for i in (0, 3):                                             # the neighbours are intact
        assert counts[i] == clean[2][i] > 0 and np.array_equal(per[i].view(np.uint64), clean[0][i].view(np.uint64))
        assert np.array_equal(_bits(ratios[i]), _bits(clean[1][i]))
    with pytest.raises(ValueError, match="predictions"):
        vg.score(depths[:3].contiguous())
