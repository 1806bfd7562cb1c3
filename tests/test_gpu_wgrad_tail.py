"""The tail of the weight gradients at its edges, through the raw C ABI on exact integer data (the _Data recipe of
test_gpu_conv_exact.py: values in -2..2, sparse gy, every partial sum below 2^22), compared element by element with float64:

* k_wgrad_stem (7x7 stride-2 stems): every channel count it is built for, a full and a masked (40 of 64) row tile, one whole output
  tile, ragged tiles in both directions, a last tile one column wide, and more tiles than the 512 persistent workgroups.
* k_wgrad_finish9 behind the Winograd weight gradient: every (channels per workgroup, slices in flight) variant its launcher picks,
  one slice and several, slice counts that are no multiple of the unroll, the 16-channel tail block, zero and reflect padding.

fd_tuning.log names the kernel family of every call, so a case that stops reaching the kernel it is here for fails."""
import ctypes
import re

import pytest
import torch

import test_gpu_conv_exact as X
from fusiondepth_amd import tuning
from fusiondepth_amd._lib import ConvDesc, call, ptr, query, stream

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _wgrad_case(t, seed, capfd, family, **tune):
    """fd_conv2d_bwd_weight of descriptor t with accumulate 0 and 1 against float64, element by element -> the family it ran on"""
    D = X._Data(seed, t)
    bud = D.budget(t)
    assert bud["wgrad"] < X.LIMIT, "exactness budget exceeded: %s" % bud
    want = X._ref_wgrad(D.gyc, D.xc, t)
    N, Cin, H, W, Cout, K = t[:6]
    d = ConvDesc(*t)
    dp = ctypes.addressof(d)
    capfd.readouterr()
    with tuning.override(log=1, **tune):
        ws = X._nan(query("fd_conv2d_bwd_weight_ws_floats", dp))
        got = {}
        for acc in (0, 1):
            gw = D.gw0.clone() if acc else X._nan((Cout, Cin, K, K))
            gb = D.gb0.clone() if acc else X._nan((Cout,))
            ws.fill_(float("nan"))
            call("fd_conv2d_bwd_weight", dp, ptr(D.x), ptr(D.gy), ptr(gw), ptr(gb), ptr(ws), acc, stream())
            got[acc] = gw
        torch.cuda.synchronize()
    fams = set(re.findall(r"^FDCONV wgrad (.+?) N=", capfd.readouterr().err, re.M))
    assert fams == {family}, "%s: routed to %s, this case is about %r" % (t, sorted(fams), family)
    for acc in (0, 1):
        ref = want + D.gw0.cpu().to(F64) if acc else want
        g = got[acc].cpu().to(F64)
        bad = g != ref                                          # (a NaN left in place compares unequal as well)
        assert not bad.any(), "accumulate %d: %d of %d elements differ from float64; first at %s: %r vs %r" % (
            acc, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()), float(g[bad][0]), float(ref[bad][0]))


# --------------------------------------------------------------------------------------------------------------------- k_wgrad_stem
STEM_SIZES = {"one-tile": (8, 64),        # Ho x Wo = 4 x 32: exactly one output tile
              "ragged": (18, 70),         # 9 x 35: ragged tiles in both directions
              "thin-last": (10, 130)}     # 5 x 65: a last tile one column wide


def _stem(N, Cin, H, W, Cout):
    return (N, Cin, H, W, Cout, 7, 7, 2, 3, 0, 0, 0)


@pytest.mark.parametrize("size", list(STEM_SIZES))
@pytest.mark.parametrize("Cout", [64, 40])
@pytest.mark.parametrize("Cin", [2, 3, 4, 6])
def test_stem_wgrad(Cin, Cout, size, capfd):
    H, W = STEM_SIZES[size]
    _wgrad_case(_stem(2, Cin, H, W, Cout), 1000 + 16 * Cin + (Cout == 40) + 2 * list(STEM_SIZES).index(size), capfd, "stem")


def test_stem_wgrad_more_tiles_than_workgroups(capfd):
    """32 images of 48x160: 6 x 3 tiles each, 576 in all for 512 persistent workgroups - 64 of them take a second tile"""
    t = _stem(32, 6, 48, 160, 64)
    assert query("fd_conv2d_bwd_weight_ws_floats", ctypes.addressof(ConvDesc(*t))) == 512 * 64 * 6 * 49
    _wgrad_case(t, 1999, capfd, "stem")


# ------------------------------------------------------------------------------------------------------------------ k_wgrad_finish9
# (N, Cin, H, W, Cout, tuning): what the launcher makes of it is in the comment - mb output channels per workgroup (Cout * ceil(Cin /
# 32) / 1024, 1 .. 8), the slices of wino_wgrad_splits at wino_wgrad_target = 256, and the <channels, slices> in flight it picks
FINISH = {
    "512-512_4x8_n1": (1, 512, 4, 8, 512, {}),             # mb 8, 1 slice: <8, 1>
    "256-256_4x8_n2": (2, 256, 4, 8, 256, {}),             # mb 2, 1 slice: <2, 8>
    "64-64_16x32_n4": (4, 64, 16, 32, 64, {}),             # mb 1, 8 slices: <1, 16>, half a batch
    "64-64_16x32_n3": (3, 64, 16, 32, 64, {}),             # mb 1, 6 slices: no multiple of 8 (from 8 up the count is rounded to one)
    "64-64_16x32_n12": (12, 64, 16, 32, 64, {}),           # mb 1, 24 slices: a full batch of 16 and half a one
    # 48 -> 64 does not reach the Winograd weight gradient (it takes Cin >= 64); the nearest channel count with a 16-wide last block
    # that does is 80 = 2 x 32 + 16
    "80-64_8x16_n2": (2, 80, 8, 16, 64, {}),               # mb 1, cw = 16 tail block
    "512-256_4x8_n1": (1, 512, 4, 8, 256, {}),             # mb 4, 1 slice: <4, 4>
    "512-512_8x16_n3_2slices": (3, 512, 8, 16, 512, {"wino_wgrad_target": 512}),      # mb 8, 2 slices: <8, 2> (not reached at the default target)
}


@pytest.mark.parametrize("pad_mode", [0, 1], ids=["zero", "reflect"])
@pytest.mark.parametrize("case", list(FINISH))
def test_wino_wgrad_finish(case, pad_mode, capfd):
    N, Cin, H, W, Cout, tune = FINISH[case]
    t = (N, Cin, H, W, Cout, 3, 3, 1, 1, pad_mode, 0, 0)
    _wgrad_case(t, 2000 + 2 * list(FINISH).index(case) + pad_mode, capfd, "wino", **tune)
