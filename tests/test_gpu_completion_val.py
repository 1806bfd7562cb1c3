"""The Completor's training-time scorer on the device (``fd_completion_val_scores`` through ``validation.CompletionGroundTruth`` /
``validation.completion_val_scores`` / ``validation.CompletionValScorer``) against its numpy restatement (tests/completion_val_ref.py,
pinned to torch on the CPU by tests/test_stage_cli_cpu.py): nine images of every kind in one call, the resident scorer across a chunk
boundary, descriptors whose window leaves the map."""
import numpy as np
import pytest
import torch

import completion_val_ref as CV
from conftest import assert_close

pytestmark = pytest.mark.gpu

# 1e-9: the tolerance tests/test_gpu_val_scores.py holds fd_val_scores to against tests/val_ref.py - n <= 2.6e5 float64 additions of
# positive terms differ between two summation orders by at most about n * 2^-53 = 3e-11 relative
SUM_RTOL = 1e-9


def _bits(x):
    """The bit patterns of float32 values; every NaN counts as the same one."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    return np.where(np.isnan(x), np.float32(np.nan), x).view(np.uint32)


def _medians(ws, n):
    """The (median(gt), median(pred)) table of the latest call of ``n`` images, read from the workspace (score_lists.h: n x 32 x 7
    float64 partials, n x 16 bytes of list positions, then n x 2 float32 medians)."""
    at = n * (32 * 7 * 8 + 16)
    return ws[at:at + n * 8].cpu().numpy().view(np.float32).reshape(n, 2)


def _check(per, ratios, counts, want, rows, what):
    assert np.array_equal(counts[rows], want["counts"]), (what, counts[rows], want["counts"])
    assert np.array_equal(_bits(ratios[rows]), _bits(want["ratios"])), (what, ratios[rows], want["ratios"])
    got, some = per[rows], want["counts"] > 0
    tc = np.rint(got[some, 4:] * want["counts"][some, None]).astype(np.int64)
    assert np.array_equal(tc, want["thresh_counts"][some]), (what, tc, want["thresh_counts"][some])
    assert np.abs(got[some, 4:] * want["counts"][some, None] - tc).max(initial=0) < 1e-6
    assert_close(got[:, :4], want["metrics"][:, :4], rtol=SUM_RTOL, atol=0, what=what + ": abs_rel / sq_rel / rmse / rmse_log")
    assert np.array_equal(np.isnan(got), np.isnan(want["metrics"]))


def _windows(crops):
    from fusiondepth_amd import validation as V
    return [V.VAL_CROP if c else V.WHOLE_MAP for c in crops]


def test_nine_images_in_one_call():
    from fusiondepth_amd import validation as V
    depths, gts, crops, want = CV.mixed_case()
    gap = [1] + [2 if g.size % 2 == 0 else 1 for g in gts[:-1]]  # every plane at an odd element offset
    vg = V.CompletionGroundTruth(gts, window=_windows(crops), gap=gap)
    assert all(int(d["offset"]) % 2 == 1 for d in vg.desc) and len(vg.chunks) == 1
    assert tuple(vg.desc[4][["y0", "y1", "x0", "x1"]]) == (153, 352, 44, 1197)                 # clipped by the 352-row map
    assert tuple(vg.desc[5][["y0", "y1"]]) == (128, 128)                                       # clipped away entirely
    assert (37 - 0) % 4 != 0 and 101 % 64 != 0
    dev = torch.from_numpy(depths.copy()).cuda()                 # the shared case is read-only
    per, ratios, counts = V.completion_val_scores(dev, vg)
    first = vg.out.cpu().numpy().copy()
    assert per.shape == (9, 7) and per.dtype == np.float64 and ratios.dtype == np.float32 and counts.dtype == np.int64
    assert counts.tolist() == want["counts"].tolist()
    some = [0, 1, 2, 4, 6, 7, 8]
    assert (counts[some] > 100).all() and counts[3] == counts[5] == 0                          # every non-empty case: > 100 pairs
    assert counts[0] % 2 == 0 and counts[1] % 2 == 1 and counts[4] > 1024 and counts[2] == 96 * 128 > 8192
    _check(per, ratios, counts, want, slice(None), "nine images")
    med = _medians(vg.ws, 9)
    assert np.array_equal(_bits(med[:, 0]), _bits(want["med_gt"])) and np.array_equal(_bits(med[:, 1]), _bits(want["med_pred"]))
    # the three values around 0.1: float32(0.1) and its lower neighbour are not selected, the upper neighbour is
    for i in (0, 1, 4, 7, 8):
        y0, y1, x0, x1 = (int(v) for v in vg.desc[i][["y0", "y1", "x0", "x1"]])
        win = gts[i][y0:y1, x0:x1]
        assert all((win == v).any() for v in CV.EDGE) and counts[i] == int((win > np.float32(0.2)).sum()) + 1
    # nothing selected: NaN metrics, NaN ratio, count 0; a NaN prediction: what torch gives
    assert np.isnan(per[[3, 5]]).all() and np.isnan(ratios[[3, 5]]).all()
    assert np.isnan(per[6, :4]).all() and (per[6, 4:] == 0).all() and np.isnan(ratios[6]) and counts[6] == 4000
    # millimetres: the RMSE of metre-scale maps is of the order of 10^4
    assert (per[[0, 1, 2, 4, 7, 8], 2] > 1000.0).all()
    # two calls give identical bits
    V.completion_val_scores(dev, vg)
    assert np.array_equal(vg.out.cpu().numpy().view(np.uint64), first.view(np.uint64))
    # against the reference's float32 means (the restatement's distance is what tests/test_stage_cli_cpu.py bounds)
    for i in (0, 2, 8):
        ref = CV.torch_reference(depths[i], gts[i])
        assert ref["count"] == counts[i]
        np.testing.assert_allclose(per[i], ref["metrics"], rtol=2e-5)


def test_resident_scorer_crosses_a_chunk_boundary():
    """11 images of 37 x 101 against predictions of 48 x 160 through ``CompletionValScorer(chunk=4)`` in batches of 3: three library
    calls (4 + 4 + 3), a batch that straddles two chunks; the rows are those of a single call and of the restatement."""
    from fusiondepth_amd import validation as V
    rng = np.random.default_rng(11)
    depths = CV.depth_pred(rng, (11,) + CV.PRED_SIZE)
    gts = np.stack([CV.sparse_gt(rng, 37, 101, valid=0.3) for _ in range(11)])
    dev, dgt = torch.from_numpy(depths).cuda(), torch.from_numpy(gts).cuda()
    sc = V.CompletionValScorer(11, (37, 101), CV.PRED_SIZE, chunk=4)
    assert sc.chunk == 4 and tuple(sc.gt.shape) == (4, 37, 101) and tuple(sc.pred.shape) == (4,) + CV.PRED_SIZE and tuple(sc.out.shape) == (11, 9)
    for round_ in range(2):                                      # the second round reuses every buffer
        sc.begin()
        for a in range(0, 11, 3):
            sc.add(dev[a:a + 3, None], dgt[a:a + 3, None])
        rows = sc.finish().cpu().numpy()
        assert sc.calls == 3
        if round_ == 0:
            first = rows.copy()
    assert np.array_equal(rows.view(np.uint64), first.view(np.uint64))
    one = V.CompletionGroundTruth(list(gts)).score(dev).cpu().numpy()
    assert np.array_equal(rows.view(np.uint64), one.view(np.uint64))                           # the rows of a single call
    want = CV.completion_val_scores(depths, gts)
    assert (want["counts"] > 100).all()
    _check(rows[:, :7], rows[:, 7].astype(np.float32), rows[:, 8].astype(np.int64), want, slice(None), "chunk 4 of 11")
    # with the crop, at the size the command runs at: the window clipped by the 352-row map
    crop = V.CompletionValScorer(2, (352, 1216), (352, 1216), eigen_crop=True, chunk=64)
    assert crop.chunk == 2 and crop.max_rows == 199 and crop.area == 199 * 1153
    with pytest.raises(ValueError, match="for a scorer of"):
        sc.add(dev[:1, None], dgt[:1, None, :30])
    sc.begin()
    sc.add(dev[:5], dgt[:5])
    with pytest.raises(ValueError, match="5 images were added for the 11"):
        sc.finish()
    sc.begin()
    sc.add(dev[:9], dgt[:9])
    with pytest.raises(ValueError, match="more images than the scorer was built for"):
        sc.add(dev[:3], dgt[:3])


def test_bad_descriptors_give_count_minus_one():
    from fusiondepth_amd import validation as V
    rng = np.random.default_rng(4)
    depths = torch.from_numpy(CV.depth_pred(rng, (4,) + CV.PRED_SIZE)).cuda()
    gts = [CV.sparse_gt(rng, 40, 100, valid=0.3) for _ in range(4)]
    vg = V.CompletionGroundTruth(gts)
    clean = V.completion_val_scores(depths, vg)
    guard = vg.out.clone()
    bad = vg.desc.copy()
    bad["y1"][1] = 41                                            # the window leaves the map below
    bad["x0"][2] = -1                                            # ... and on the left
    vg.desc_dev = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
    per, ratios, counts = V.completion_val_scores(depths, vg)
    assert counts[1] == counts[2] == -1 and np.isnan(per[1:3]).all() and np.isnan(ratios[1:3]).all()
    for i in (0, 3):                                             # the neighbours are intact
        assert counts[i] == clean[2][i] > 100 and np.array_equal(per[i].view(np.uint64), clean[0][i].view(np.uint64))
        assert np.array_equal(_bits(ratios[i]), _bits(clean[1][i]))
    assert torch.equal(vg.out[[0, 3]].view(torch.int64), guard[[0, 3]].view(torch.int64))
