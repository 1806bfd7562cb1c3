"""Host side of ``train --log_images``: the numpy restatement (tests/log_images_ref.py) against the reference's torch expression, the
quantisation rule at its edges, ``log_images.layout``, the binding of ``fd_log_sheets``, the default PNG sink and the command's switch.
No GPU is touched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import log_images_ref as LR

F32 = np.float32


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, F32)).reshape(-1).view(np.uint32)


# --------------------------------------------------------------------------------------------- the restatement against torch
def _torch_normalize_image(x):
    """utils.normalize_image, word for word."""
    ma = float(x.max().cpu().data)
    mi = float(x.min().cpu().data)
    d = ma - mi if ma != mi else 1e5
    return (x - mi) / d


def _maps():
    rng = np.random.RandomState(7)
    maps = [rng.uniform(0.01, 0.9, (5, 9)).astype(F32), rng.randn(7, 13).astype(F32), (rng.randn(3, 4) * 1e-3 + 7).astype(F32),
            rng.uniform(-3, 5, (1, 1)).astype(F32)]
    maps.append(np.full((4, 6), 0.37, F32))                       # constant: the 1e5 branch
    maps.append(np.zeros((2, 3), F32))
    one = np.full((6, 5), 0.25, F32)                              # a range of one float32 spacing
    one[2, 3] = np.nextafter(F32(0.25), F32(1.0))
    maps.append(one)
    wide = np.full((3, 3), 1.0, F32)
    wide[0, 0] = np.nextafter(F32(1.0), F32(0.0))
    maps.append(wide)
    return maps


def test_normalize_image_equals_the_torch_expression_bit_for_bit():
    for m in _maps():
        want = _torch_normalize_image(torch.from_numpy(m[None])).numpy()[0]
        got, mi, ma = LR.normalize_image(m)
        assert got.dtype == F32 and np.array_equal(_bits(got), _bits(want)), (m.shape, got, want)
        assert mi == m.min() and ma == m.max()
    const, mi, ma = LR.normalize_image(np.full((4, 6), 0.37, F32))
    assert mi == ma and np.array_equal(const, np.zeros((4, 6), F32))
    holed = np.array([[0.1, np.nan], [0.5, 0.2]], F32)            # torch's max() of a map with a NaN is NaN: so is every pixel
    assert np.isnan(_torch_normalize_image(torch.from_numpy(holed)).numpy()).all() and np.isnan(LR.normalize_image(holed)[0]).all()


def test_quantisation_at_its_edges():
    levels = np.arange(256, dtype=np.float64)
    exact = (levels / 255.0).astype(F32)                          # the float32 nearest k / 255 and its neighbours either side
    for x in (exact, np.nextafter(exact, F32(-1)), np.nextafter(exact, F32(2))):
        got = LR.quantise(x)
        with np.errstate(all="ignore"):
            want = np.clip(np.trunc(np.clip(x * F32(255.0), 0, 255)), 0, 255).astype(np.uint8)   # the rule, in float32 products
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    # values whose float32 product with 255 IS an integer (asserted), and one float32 spacing either side of them
    xs =np.array([0.0, 1.0, 0.2, 0.4, 0.6, 0.8], F32)
    prod = xs * F32(255.0)
    assert np.array_equal(prod, np.trunc(prod)) and np.array_equal(LR.quantise(xs), prod.astype(np.uint8))
    below, above = np.nextafter(xs[1:], F32(-1)), np.nextafter(xs, F32(2))
    assert np.array_equal(LR.quantise(below), (prod[1:] - 1).astype(np.uint8))       # one spacing below an integer product: a level less
    assert np.array_equal(LR.quantise(above), np.minimum(prod, 255).astype(np.uint8))
    odd = np.array([-0.5, -0.0, -1e-30, 1.0000001, 1.5, 300.0, np.inf, -np.inf, np.nan], F32)
    assert LR.quantise(odd).tolist() == [0, 0, 0, 255, 255, 255, 255, 0, 0]
    assert LR.automask(np.array([[0, 1, 2, 3]], np.uint8), 2).tolist() == [[0, 0, 255, 255]]
    assert LR.automask(np.array([[0, 1]], np.uint8), 1).tolist() == [[0, 255]]


# --------------------------------------------------------------------------------------------- layout
def _reference_tags(frame_ids, scales, j, automask, predictive_mask, val):
    """The tags trainer.py:656-681 writes for item j, grouped per scale as the sheet packs them."""
    tags = []
    for s in scales:
        tags += ["color_{}_{}/{}".format(f, s, j) for f in frame_ids]
        if s == 0:
            tags += ["color_pred_{}_{}/{}".format(f, s, j) for f in frame_ids if f != 0]
        tags.append("disp_{}/{}".format(s, j))
        if predictive_mask:
            tags += ["predictive_mask_{}_{}/{}".format(f, s, j) for f in frame_ids[1:]]
        elif automask and not val:
            tags.append("automask_{}/{}".format(s, j))
    return tags


@pytest.mark.parametrize("frame_ids", [[0], [0, -1, 1], [0, -1, 1, "s"]], ids=["F1", "F3", "F4"])
@pytest.mark.parametrize("scales", [[0, 1, 2, 3], [0]], ids=["S4", "S1"])
@pytest.mark.parametrize("mode", ["automask", "automask_v1", "plain", "predictive", "val"])
def test_layout(frame_ids, scales, mode):
    from fusiondepth_amd import log_images as L
    H, W, J = 32, 64, 3
    val = mode == "val"
    fids = [0] if val else frame_ids
    kw = dict(automask=mode in ("automask", "automask_v1", "val"), predictive_mask=mode == "predictive", val=val,
              mask_size="scale" if mode == "automask_v1" else None)
    lay = L.layout(fids, scales, H, W, J=J, **kw)
    per = len(lay.tiles) // J
    assert len(lay.tiles) == per * J and len(lay.rows) == len(scales)
    for j in range(J):
        mine = lay.tiles[j * per:(j + 1) * per]
        assert [t.tag for t in mine] == _reference_tags(fids, scales, j, kw["automask"], kw["predictive_mask"], val)
        assert all(t.item == j for t in mine)
        assert [tuple(t[2:7]) for t in mine] == [tuple(t[2:7]) for t in lay.tiles[:per]]       # the same geometry for every item
    assert not any("mask" in t.tag for t in lay.tiles) or mode in ("automask", "automask_v1", "predictive")
    if val:
        assert not any("pred" in t.tag or "mask" in t.tag for t in lay.tiles)
    # sizes: a tile has the size of the tensor the reference hands over; the automask planes are scale 0's unless v1_multiscale
    for t in lay.tiles[:per]:
        hs, ws = H // 2 ** t.scale, W // 2 ** t.scale
        want = (H, W) if (t.kind == L.KIND_AUTOMASK and mode == "automask") else (hs, ws)
        assert (t.h, t.w) == want and t.channels == (3 if t.kind in (L.KIND_COLOR, L.KIND_PRED) else 1), t
    # Hs, Ws: the sum of the block heights - the scales' own heights wherever no tile is taller -, the widest block
    heights = [max(t.h for t in lay.tiles[:per] if t.scale == s) for s in scales]
    if mode != "automask":
        assert heights == [H // 2 ** s for s in scales]
    assert lay.Hs == sum(heights) and [r[1] for r in lay.rows] == heights
    assert lay.Ws == max(sum(t.w for t in lay.tiles[:per] if t.scale == s) for s in scales)
    # packed left to right from 0 with no gaps, top edges on the block's; disjoint and inside the sheet
    cover = np.zeros((lay.Hs, lay.Ws), np.int32)
    for s, (y, h, first, count) in zip(scales, lay.rows):
        x = 0
        for t in lay.tiles[first:first + count]:
            assert t.scale == s and (t.y, t.x) == (y, x) and t.h <= h
            x += t.w
            assert t.y + t.h <= lay.Hs and t.x + t.w <= lay.Ws
            cover[t.y:t.y + t.h, t.x:t.x + t.w] += 1
    assert cover.max() == 1
    # ... and the restatement's layout agrees
    Hs, Ws, ref = LR.layout(fids, scales, H, W, kw["automask"], kw["predictive_mask"], val, kw["mask_size"])
    assert (Hs, Ws) == (lay.Hs, lay.Ws)
    assert [(t.tag.rsplit("/", 1)[0], t.y, t.x, t.h, t.w, t.channels) for t in lay.tiles[:per]] == ref


def test_layout_of_the_default_run_and_refusals():
    from fusiondepth_amd import log_images as L
    lay = L.layout([0, -1, 1], [0, 1, 2, 3], 192, 640, J=2, automask=False)
    assert (lay.Hs, lay.Ws) == (192 + 96 + 48 + 24, 6 * 640)
    assert [t.tag for t in lay.tiles[:6]] == ["color_0_0/0", "color_-1_0/0", "color_1_0/0", "color_pred_-1_0/0", "color_pred_1_0/0", "disp_0/0"]
    assert lay.tiles[-1].tag == "disp_3/1" and tuple(lay.tiles[-1][2:7]) == (192 + 96 + 48, 3 * 80, 24, 80, 1)
    stereo = L.layout([0, -1, 1, "s"], [0], 32, 64)
    assert "color_pred_s_0/0" in [t.tag for t in stereo.tiles] and "color_s_0/0" in [t.tag for t in stereo.tiles]
    full = L.layout([0, -1, 1], [0, 1, 2, 3], 192, 640)           # the automask of every scale is a full-resolution plane
    assert (full.Hs, full.Ws) == (4 * 192, 7 * 640) and full.tiles[-1].tag == "automask_3/0" and tuple(full.tiles[-1][2:6]) == (576, 320, 192, 640)
    for bad in (dict(J=0), dict(frame_ids=[]), dict(scales=[])):
        kw = dict(frame_ids=[0], scales=[0], height=8, width=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            L.layout(**kw)
    with pytest.raises(RuntimeError, match="needs an MI355X") if not torch.cuda.is_available() else pytest.raises(ValueError):
        L.render({}, {}, [0], [0], 1)


# --------------------------------------------------------------------------------------------- the binding
def test_binding_of_the_renderer():
    from fusiondepth_amd import _lib
    root = __import__("conftest").ROOT
    assert _lib.ABI_VERSION == 8
    assert _lib.SIGNATURES["fd_log_sheets_ws_bytes"] == ("ii", "l")
    args, res = _lib.SIGNATURES["fd_log_sheets"]
    assert res == "i" and args == "ppiipppp"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "fd_log_sheets") and hasattr(lib, "fd_log_sheets_ws_bytes")
    header = open(os.path.join(root, "include", "fdhip.h")).read()
    assert "#define FD_ABI_VERSION 8" in header and "long fd_log_sheets_ws_bytes(int J, int n_disp);" in header
    proto = header[header.index("int fd_log_sheets("):]
    proto = proto[:proto.index(";")]
    assert proto.count(",") + 1 == len(args)
    table = open(os.path.join(root, "fusiondepth_amd", "csrc", "replay_table.inc")).read()
    assert '{"fd_log_sheets", "ppiipppp"},' in table and "(&fd_log_sheets)(" in table
    # the mirrors have the header's sizes: five pointers and eight ints; 4 + 5 * 8 ints, three floats and one int
    assert ctypes.sizeof(_lib.LogTile) == 5 * 8 + 8 * 4 and ctypes.sizeof(_lib.LogCfg) == 4 * (4 + 40 + 3 + 1)
    fn = lib.fd_log_sheets_ws_bytes
    fn.restype, fn.argtypes = ctypes.c_long, [ctypes.c_int, ctypes.c_int]
    assert fn(1, 0) == 16 and fn(4, 4) == 256 and fn(0, 1) == 0 and fn(65, 1) == 0 and fn(1, 9) == 0


# --------------------------------------------------------------------------------------------- the default sink
def test_default_sink_writes_the_sheets_as_png(tmp_path):
    from PIL import Image
    from fusiondepth_amd import log_images as L
    rng = np.random.RandomState(3)
    planes = {"color_0_0": rng.uniform(-0.2, 1.2, (3, 7, 13)).astype(F32), "disp_0": rng.uniform(0, 1, (7, 13)).astype(F32)}
    _, _, tiles = LR.layout([0], [0], 7, 13, automask=False)
    sheets = np.stack([LR.assemble(tiles, planes), LR.assemble(tiles, {k: 1 - v for k, v in planes.items()})])
    assert sheets.shape == (2, 7, 26, 3) and sheets.dtype == np.uint8
    sink = L.PngSink(str(tmp_path))
    sink("train", 12, sheets, {})
    sink("val", 12, sheets[:1], {})
    sink("train", 250, sheets[::-1], {})
    sink.join()
    assert sink._thread is None                                   # nothing is left running
    for mode, step, want in (("train", 12, sheets), ("val", 12, sheets[:1]), ("train", 250, sheets[::-1])):
        for j in range(len(want)):
            path = os.path.join(str(tmp_path), mode, "images", "%07d_%d.png" % (step, j))
            assert path == L.PngSink.path(str(tmp_path), mode, step, j) and os.path.isfile(path), path
            got = np.asarray(Image.open(path))
            assert got.dtype == np.uint8 and np.array_equal(got, want[j])
    assert sorted(os.listdir(os.path.join(str(tmp_path), "train", "images"))) == ["0000012_0.png", "0000012_1.png", "0000250_0.png", "0000250_1.png"]
    sink("train", 3, sheets, {})                                  # a sink that was joined starts its thread again
    sink.close()
    assert os.path.isfile(L.PngSink.path(str(tmp_path), "train", 3, 1))
    bad = L.PngSink(os.path.join(str(tmp_path), "train", "images", "0000012_0.png"))      # a file where a folder must go
    bad("train", 1, sheets, {})
    with pytest.raises(OSError):
        bad.join()


# --------------------------------------------------------------------------------------------- the command's switch
def test_the_command_knows_log_images():
    from fusiondepth_amd import train as T
    before = {"splits_dir": "splits", "seed": 0, "lidar_source": "files", "val_limit": None, "no_val": False}
    assert T.split_off_extra([]) == (before, [])
    assert T.split_off_extra(["--png", "--seed", "4"]) == (dict(before, seed=4), ["--png"])
    extra, rest = T.split_off_extra(["--png", "--log_images", "--seed=4", "--no_val"])
    assert extra == dict(before, seed=4, no_val=True, log_images=True) and rest == ["--png"]
    assert "log_images" in T.EXTRA_SWITCHES
    from fusiondepth_amd.trainer import Trainer
    assert Trainer.log_images is False and Trainer.image_sink is None
