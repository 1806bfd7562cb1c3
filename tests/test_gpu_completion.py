"""KITTI depth completion on the GPU: ``fd_depth_png_keys`` against the numpy restatement (tests/completion_ref.py) and the reference's
own outputs (tests/golden/completion_*.npz), ``KITTICompletionBatches`` on the synthetic tree key by key, the scorer
(``fd_completion_medians`` / ``fd_completion_errors``) against numpy, and the chain ``Completor.train(loader)`` ->
``python -m fusiondepth_amd.evaluate_completion`` end to end."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import completion_ref as CR
import completion_tree as CT
import conftest
from conftest import assert_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITEMS = {"train": (True, 1), "train_flip": (True, 4), "val": (False, 2), "test": (False, 1)}
JITTER = ((1.13, 0.85, 1.2, -0.07), (2, 0, 3, 1))                # make_completion.JITTER
FRAMES = [0, -1, 1]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return CT.make_tree(str(tmp_path_factory.mktemp("completion") / "completion"))


def host(t):
    return t.detach().cpu().numpy()


def same(a, b):
    """Bit-equal float32 arrays (NaN patterns included)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------- fd_depth_png_keys
def window_ref(plane, desc, canvas, pool, channels, div0, div1):
    """The descriptor's meaning in numpy, with get_depth's operations: / div0, fliplr, the window, the pool, / div1."""
    _, h, w, mirror, sy, sx, wy, wx, wh, ww = desc
    depth = plane.astype(np.float32) / np.float32(div0)
    if mirror:
        depth = np.fliplr(depth)
    out = np.zeros(canvas, np.float32)
    out[wy:wy + wh, wx:wx + ww] = depth[sy:sy + wh, sx:sx + ww]
    if pool == 2:
        out = CR.max_pool_ceil(out)
    out = out / np.float32(div1)
    return np.stack([out] * channels)


def pack(planes):
    """uint16 planes -> (packed int16 device tensor, offsets); every plane starts 8-byte aligned."""
    offs, at = [], 0
    for p in planes:
        offs.append(at)
        at += (p.size + 3) // 4 * 4
    buf = np.zeros(max(at, 4), np.uint16)
    for p, o in zip(planes, offs):
        buf[o:o + p.size] = p.reshape(-1)
    return torch.from_numpy(buf.view(np.int16)).cuda(), offs


def small_planes(seed=1):
    rng = np.random.default_rng(seed)
    planes = []
    for h, w in ((23, 37), (24, 36), (23, 37), (24, 36), (23, 37)):
        p = rng.integers(0, 65536, (h, w)).astype(np.uint16)
        p[rng.random((h, w)) < 0.5] = 0
        p[0, :5] = p[-1, -5:] = p[h // 2, 3:8] = (0, 1, 255, 256, 65535)
        p[:5, 0] = p[-5:, -1] = (65535, 256, 255, 1, 0)
        planes.append(p)
    return planes


def small_descs(planes, offs, kind, canvas, mirrors):
    descs = []
    for p, o, m in zip(planes, offs, mirrors):
        h, w = p.shape
        if kind == "crop":                                       # bottom_crop to the 16x32 canvas
            descs.append((o, h, w, m, h - 16, int(round((w - 32) / 2.)), 0, 0, 16, 32))
        elif kind == "pad":                                      # rows on top, half of the columns on the left
            descs.append((o, h, w, m, 0, 0, canvas[0] - h, (canvas[1] - w) // 2, h, w))
        else:                                                    # crop, then pad the 16x32 map
            descs.append((o, h, w, m, h - 16, int(round((w - 32) / 2.)), canvas[0] - 16, (canvas[1] - 32) // 2, 16, 32))
    return descs


@pytest.mark.parametrize("kind,canvas", [("crop", (16, 32)), ("pad", (24, 40)), ("pad", (25, 41)), ("croppad", (24, 40)), ("croppad", (25, 41))])
def test_depth_png_keys_small_shapes(kind, canvas):
    """S = 5 planes of two sizes (23x37, 24x36) in one call: crop, pad and crop-then-pad, an even and an odd canvas (clipped ceil-mode
    blocks; 23-row and 37-column planes put the filled window at odd offsets, so pool blocks straddle its border), mirrored and not,
    pool 1 and 2, one and two channels, / 1 and / 100 - bit-exact."""
    from fusiondepth_amd import data_ops
    planes = small_planes()
    packed, offs = pack(planes)
    for mirrors in ([False, True, True, False, True], [True, False, False, True, False]):
        descs = small_descs(planes, offs, kind, canvas, mirrors)
        for pool in (1, 2):
            for channels, div1 in ((1, 1.0), (2, 100.0), (1, 100.0)):
                got = host(data_ops.depth_png_keys(packed, descs, canvas, pool, channels, 256.0, div1))
                assert got.shape == (5, channels, (canvas[0] + pool - 1) // pool, (canvas[1] + pool - 1) // pool)
                for s, (p, d) in enumerate(zip(planes, descs)):
                    want = window_ref(p, d, canvas, pool, channels, 256.0, div1)
                    assert same(got[s], want), (kind, canvas, mirrors[s], pool, channels, div1, s, int((got[s] != want).sum()))
    vals = host(data_ops.depth_png_keys(packed, small_descs(planes, offs, "pad", (24, 40), [False] * 5), (24, 40), 1, 1, 256.0, 100.0))
    for v in (1, 255, 256, 65535):                               # two true divisions: (v / 256) / 100 as numpy rounds it
        assert (vals == np.float32(np.float32(v) / np.float32(256.)) / np.float32(100.0)).any(), v


def test_depth_png_keys_descriptor_leaving_the_buffer_gives_a_nan_plane():
    from fusiondepth_amd import _lib, data_ops
    planes = small_planes(2)
    packed, offs = pack(planes)
    descs = small_descs(planes, offs, "pad", (24, 40), [False, True, False, True, False])
    good = host(data_ops.depth_png_keys(packed, descs, (24, 40), 2, 2, 256.0, 100.0))
    for field, value in (("offset", packed.numel() - 10), ("src_y", 1), ("win_x", 30), ("h", -1)):
        table = data_ops.depth_png_desc_table(descs)
        setattr(table[2], field, value)                          # only the device table is wrong: the host check sees `descs`
        dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
        got = host(data_ops.depth_png_keys(packed, descs, (24, 40), 2, 2, 256.0, 100.0, desc_table=dev))
        assert np.isnan(got[2]).all(), field
        assert same(got[[0, 1, 3, 4]], good[[0, 1, 3, 4]]), field
    with pytest.raises(ValueError, match="leaves the packed buffer"):
        data_ops.depth_png_keys(packed, [(packed.numel() - 10, 23, 37, False, 0, 0, 1, 1, 23, 37)], (24, 40))
    with pytest.raises(ValueError, match="does not fit"):
        data_ops.depth_png_keys(packed, [(0, 23, 37, False, 0, 0, 2, 1, 23, 37)], (24, 40))
    with pytest.raises(ValueError):
        data_ops.depth_png_keys(packed.float(), descs, (24, 40))
    with pytest.raises(RuntimeError, match="fd_depth_png_keys"):
        _lib.call("fd_depth_png_keys", packed.data_ptr(), packed.numel(), None, 1, 24, 40, 3, 1, 256.0, 1.0, None, None)


def item_pngs(tree, name, mode):
    is_train, index = ITEMS[name]
    split = "test_completion" if name == "test" else ("train" if is_train else "val")
    paths = CR.completion_paths(tree, split, "select")
    d = paths["d"][index]
    head, tail = os.path.split(d)
    n = int(tail[:tail.find(".")]) if is_train else 0
    frames = {f: CR.load_png(os.path.join(head, "%010d.png" % (n + f))) for f in FRAMES} if is_train else {0: CR.load_png(d)}
    gt = CR.load_png(paths["gt"][index]) if paths["gt"][index] else None
    return frames, gt


@pytest.mark.parametrize("mode", ["full", "pad"])
@pytest.mark.parametrize("name", list(ITEMS))
def test_depth_png_keys_full_size_against_the_reference(tree, golden, name, mode):
    """The keys of the four golden items in both modes, full_res_4beam included, from one packed buffer per item."""
    from fusiondepth_amd import completion_data as CD, data_ops
    g = golden("completion_%s_%s" % (name, mode))
    flip, full_res = bool(g["do_flip"]), mode == "full"
    frames, gt = item_pngs(tree, name, mode)
    order = list(frames)
    planes = [frames[f] for f in order] + ([gt] if gt is not None else [])
    packed, offs = pack(planes)
    pool = 1 if full_res else 2
    beam = [CD.depth_desc(offs[k], *planes[k].shape, flip, full_res, not full_res) for k in range(len(order))]
    two = host(data_ops.depth_png_keys(packed, [d for d, _ in beam], beam[0][1], pool, 2, 256.0, 100.0))
    for k, f in enumerate(order):
        want = g["2channel_%d" % f] if "2channel_%d" % f in g else g["4beam"][0]
        assert same(two[k, 0], want) and same(two[k, 1], want), (f, int((two[k, 0] != want).sum()))
    assert same(two[order.index(0), :1], g["4beam"])
    d, canvas = CD.depth_desc(offs[order.index(0)], *planes[order.index(0)].shape, flip, full_res, True)
    assert canvas == (384, 1280)
    assert same(host(data_ops.depth_png_keys(packed, [d], canvas, 1, 1, 256.0, 1.0))[0], g["full_res_4beam"])
    if gt is not None:
        d, canvas = CD.depth_desc(offs[-1], *gt.shape, flip, full_res, not full_res)
        assert same(host(data_ops.depth_png_keys(packed, [d], canvas, 1, 1, 256.0, 1.0))[0], g["depth_gt"])


# ---------------------------------------------------------------------------------------------- the loader
def golden_draws(epoch, index):
    """Item 4 is the golden's flipped and augmented item; every other item is plain."""
    on = index == 4
    return {"do_color_aug": on, "do_flip": on, "jitter": JITTER if on else None}


def check_colour(batch, b, frames, g):
    planes = lambda k: g[k].astype(np.float32) / np.float32(255)
    n = 0
    for k in g:
        if not k.startswith("color"):
            continue
        kind = "color_aug" if k.startswith("color_aug") else "color"
        rest = k[len(kind) + 1:].split("_")
        f, s = int(rest[0]), int(rest[1])
        if f not in frames:
            continue
        got = host(batch[(kind, f, s)][b])
        if len(rest) == 3:
            r = int(rest[2][4:])
            got = got[:, r:r + 4]
        assert same(got, planes(k)), k
        n += 1
    return n


@pytest.mark.parametrize("mode", ["full", "pad"])
def test_loader_training_batch_equals_the_reference(tree, golden, mode):
    """One training batch of mixed source sizes (375x1242 and 376x1241), the second item flipped and augmented: every key against
    what the reference returned for the same two items."""
    from fusiondepth_amd.completion_data import KITTICompletionBatches
    nfr = mode == "pad"
    h, w = (192, 640) if nfr else (352, 1216)
    opt = CT.options(completion_not_full_res=nfr, eval_gdc=True, need_path=True)
    loader = KITTICompletionBatches(tree, h, w, FRAMES, 4, is_train=True, opt=opt, batch_size=2, draws=golden_draws)
    batch = loader.build_batch(0, [1, 4])
    torch.cuda.synchronize()
    loader.close()
    gs = [golden("completion_train_%s" % mode), golden("completion_train_flip_%s" % mode)]
    assert batch["date"] == [str(g["date"]) for g in gs] == ["2011_09_26", "2011_09_28"]
    assert [os.path.relpath(p, tree) for p in batch["path"]] == [str(g["path"]) for g in gs]
    dh, dw = (192, 640) if nfr else (352, 1216)
    gh, gw = (384, 1280) if nfr else (352, 1216)
    assert batch["4beam"].shape == (2, 1, dh, dw) and batch["2channel"].shape == (2, 2, dh, dw) and batch["4beam"].is_contiguous()
    assert batch["depth_gt"].shape == (2, 1, gh, gw) and batch["full_res_4beam"].shape == (2, 1, 384, 1280)
    for b, g in enumerate(gs):
        for k in ("4beam", "depth_gt", "full_res_4beam"):
            assert same(host(batch[k][b]), g[k]), (b, k)
        assert same(host(batch["2channel"][b]), np.stack([g["4beam"][0]] * 2))
        for f in FRAMES:
            assert same(host(batch[("2channel", f, 0)][b]), np.stack([g["2channel_%d" % f]] * 2)), (b, f)
        assert check_colour(batch, b, FRAMES, g) >= 3 * (2 + 6) * (2 if b else 1)
        if not b:
            for f in FRAMES:
                for s in range(4):
                    assert batch[("color_aug", f, s)].data_ptr() == batch[("color", f, s)].data_ptr() or \
                        torch.equal(batch[("color_aug", f, s)][0], batch[("color", f, s)][0])
    for s in range(4):
        K = host(batch[("K", s)])
        assert K.shape == (2, 4, 4) and K[0, 0, 0] == np.float32(0.58) * (w // 2 ** s) and K[1, 1, 1] == np.float32(1.92) * (h // 2 ** s)
        assert_close(host(batch[("inv_K", s)][0]) @ K[0], np.eye(4), rtol=0, atol=1e-5)
    if not nfr:                                                  # scale 0 is a same-size resample: the cropped frame itself
        rgb = CR.load_png(os.path.join(tree, str(gs[0]["path"])))
        assert same(host(batch[("color", 0, 0)][0]), CR.get_color(rgb, False, False).astype(np.float32).transpose(2, 0, 1) / np.float32(255))


@pytest.mark.parametrize("name,mode", [("val", "full"), ("val", "pad"), ("test", "full"), ("test", "pad")])
def test_loader_eval_batches_equal_the_reference(tree, golden, name, mode):
    """The validation (select) and test_completion splits: every batch against completion_ref, the golden item against the reference;
    batch size 2 over 3 (or 2) items leaves a trailing partial batch."""
    from fusiondepth_amd.completion_data import KITTICompletionBatches
    nfr = mode == "pad"
    h, w = (192, 640) if nfr else (352, 1216)
    opt = CT.options(completion_not_full_res=nfr, completion_test=name == "test", eval_gdc=True, need_path=True)
    loader = KITTICompletionBatches(tree, h, w, [0], 4, is_train=False, opt=opt, batch_size=2, drop_last=False)
    assert loader.split == ("test_completion" if name == "test" else "val")
    paths = CR.completion_paths(tree, loader.split, "select")
    g = golden("completion_%s_%s" % (name, mode))
    seen = 0
    for batch in loader:
        B = batch[("color", 0, 0)].shape[0]
        assert ("depth_gt" in batch) == (name != "test") and ("2channel", 0, 0) not in batch and ("color", -1, 0) not in batch
        for b in range(B):
            index = seen + b
            want = CR.depth_keys(paths, index, opt, False, [0], False)
            assert set(k for k in want) <= set(batch)
            for k, v in want.items():
                assert same(host(batch[k][b]), v), (index, k)
            assert batch["date"][b] == os.path.basename(paths["rgb"][index])[:10] and batch["path"][b] == paths["rgb"][index]
            if index == ITEMS[name][1]:
                for k in ("4beam", "depth_gt", "full_res_4beam"):
                    if k in g:
                        assert same(host(batch[k][b]), g[k]), k
                assert check_colour(batch, b, [0], g) == 2 + 6
        seen += B
    loader.close()
    assert seen == len(paths["rgb"]) and len(loader) == (seen + 1) // 2


def test_loader_prefetch_order_and_partial_batch(tree):
    """The builder stream (prefetch) yields the batches ``build_batch`` makes on the current stream, in epoch order, the trailing
    partial batch included; with drop_last it is dropped."""
    from fusiondepth_amd.completion_data import KITTICompletionBatches
    opt = CT.options()
    mk = lambda **kw: KITTICompletionBatches(tree, 352, 1216, FRAMES, 4, is_train=True, opt=opt, batch_size=3, shuffle=True, seed=4, **kw)
    ref = mk(prefetch=False, drop_last=False)
    order = ref.epoch_order(0)
    assert sorted(order) == list(range(8)) and order != list(range(8)) and len(ref) == 3 and len(mk()) == 2
    want = [ref.build_batch(0, order[i:i + 3]) for i in range(0, 8, 3)]
    assert [b["4beam"].shape[0] for b in want] == [3, 3, 2]
    for prefetch in (True, False):
        loader = mk(prefetch=prefetch, drop_last=False)
        got = list(loader)
        torch.cuda.synchronize()
        loader.close()
        assert len(got) == 3
        for a, b in zip(got, want):
            assert set(a) == set(b)
            for k in a:
                assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k
    ref.close()
    assert len(list(mk())) == 2


def test_loader_online_2channel_map(tree, golden):
    """completion_need2channel = true in full-res mode: the scatter of the cropped map / 100 with gen2cha_completion.py's window - the
    reference's own maps for unflipped items, the scatter oracle of the mirrored map for a flipped one (the reference flips its
    stored map vertically there: module docstring of completion_data)."""
    from fusiondepth_amd.completion_data import KITTICompletionBatches
    from oracle import scatter as OS
    g = golden("completion_scatter")
    opt = CT.options(completion_need2channel="true")
    flips = {}
    loader = KITTICompletionBatches(tree, 352, 1216, FRAMES, 4, is_train=True, opt=opt, batch_size=2,
                                    draws=lambda e, i: {"do_color_aug": False, "do_flip": flips.get(i, False), "jitter": None})
    assert [int(g["index0"]), int(g["index1"])] == [1, 4]
    plain = loader.build_batch(0, [1, 4])
    for b in range(2):
        assert same(host(plain["2channel"][b]), np.stack([g["depth%d" % b], g["conf%d" % b]])), b
        assert same(host(plain[("2channel", 0, 0)][b]), host(plain["2channel"][b]))
    flips[4] = True
    flipped = loader.build_batch(0, [1, 4])
    loader.close()
    beam = host(flipped["4beam"][1, 0])
    paths = CR.completion_paths(tree, "train", "select")
    # mirror, then crop: at width 1241 (12 columns cut on the left, 13 on the right) that is not the mirror of the unflipped crop
    assert same(beam, CR.get_depth(CR.load_png(paths["d"][4]), True, False, False, False)[0] / np.float32(100.0))
    assert not same(beam, host(plain["4beam"][1, 0])[:, ::-1]) and same(host(flipped["2channel"][0]), host(plain["2channel"][0]))
    depth, conf = OS.scatter_2channel_c(np.ascontiguousarray(beam), roi=CT.ROI, expand=2)
    assert same(host(flipped["2channel"][1]), np.stack([depth, conf]))
    side = host(flipped[("2channel", -1, 0)][1])                 # a neighbour frame's map is the scatter of ITS mirrored beam map
    head, tail = os.path.split(paths["d"][4])
    png = CR.load_png(os.path.join(head, "%010d.png" % (int(tail[:10]) - 1)))
    four = CR.get_depth(png, True, False, False, False)[0] / np.float32(100.0)
    depth, conf = OS.scatter_2channel_c(np.ascontiguousarray(four), roi=CT.ROI, expand=2)
    assert same(side, np.stack([depth, conf]))
    with pytest.raises(NotImplementedError, match="completion_need2channel"):
        KITTICompletionBatches(tree, 192, 640, FRAMES, 4, is_train=True,
                               opt=CT.options(completion_need2channel="true", completion_not_full_res=True))


def test_loader_refuses_an_8_bit_depth_map(tree):
    """The reference's ``max > 255`` assertion, raised from the worker with the file's path."""
    from fusiondepth_amd.completion_data import KITTICompletionBatches
    loader = KITTICompletionBatches(tree, 352, 1216, [0], 4, is_train=False, val_split="full", opt=CT.options(), batch_size=1, drop_last=False)
    bad = [i for i, p in enumerate(loader.paths["d"]) if p.endswith("%010d.png" % CT.EIGHT_BIT_FRAME)]
    assert len(bad) == 1 and len(loader) == len(CT.VAL_FRAMES)
    with pytest.raises(AssertionError, match=r"np.max\(depth_png\)=255, path=.*%010d.png" % CT.EIGHT_BIT_FRAME):
        loader.build_batch(0, bad)
    good = loader.build_batch(0, [0])                            # 370x1224, the fifth source size
    loader.close()
    want = CR.depth_keys(loader.paths, 0, CT.options(), False, [0], False)
    assert all(same(host(good[k][0]), v) for k, v in want.items())


# ---------------------------------------------------------------------------------------------- the scorer
def test_medians_and_errors_against_numpy_and_the_reference(golden):
    """Images of 37x53 with 0, 1, 2, 301 and 400 selected pixels, duplicated values across the middle: medians and ratio bit-equal to
    numpy's, the four errors against the reference's compute_errors within the project's 1e-4 relative, against float64 sums of the
    same float32 terms (gap reported), and run to run bitwise identical."""
    import make_completion as MC
    from fusiondepth_amd import evaluate_completion as EC
    g = golden("completion_metrics")
    gt, pred = MC.metric_pairs(int(g["seed"]))
    dg, dp = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()
    worst = 0.0
    for tag, scale in (("", 1.0), ("_s", 1.3)):
        med = host(EC.completion_medians(dp, dg, 0.1, scale))
        ratio = torch.from_numpy(med[:, 0].copy()).cuda()
        err = host(EC.completion_errors(dp, dg, ratio, 0.1, scale))
        assert np.array_equal(host(EC.completion_medians(dp, dg, 0.1, scale)).view(np.uint32), med.view(np.uint32))
        assert np.array_equal(host(EC.completion_errors(dp, dg, ratio, 0.1, scale)).view(np.uint64), err.view(np.uint64))
        for n, count in enumerate(MC.METRIC_COUNTS):
            assert med[n, 3] == count == err[n, 4]
            if count == 0:
                assert np.isnan(med[n, :3]).all() and np.isnan(err[n, :4]).all()
                continue
            mask = gt[n] > 0.1
            p = pred[n] * np.float32(scale)
            want = np.array([np.median(gt[n][mask]) / np.median(p[mask]), np.median(gt[n][mask]), np.median(p[mask])], np.float32)
            assert same(med[n, :3], want), (n, med[n], want)
            assert same(want, np.array([g["ratio%d%s" % (n, tag)], g["median_gt%d%s" % (n, tag)], g["median_pred%d%s" % (n, tag)]], np.float32))
            assert_close(err[n, :4], g["errors%d%s" % (n, tag)], rtol=1e-4, atol=0, what="errors of image %d%s" % (n, tag))
            _, gs, ps = CR.scored(pred[n].copy(), gt[n], scale)
            f64 = np.array(CR.compute_errors_f64_sums(gs, ps))
            worst = max(worst, float(np.max(np.abs(err[n, :4] - f64) / np.maximum(np.abs(f64), 1e-300))))
    conftest.report("completion errors |HIP - float64 sums of the same float32 terms| / |.| (recorded, no bound)", worst, float("nan"))
    # compute_errors on already selected values; a NaN prediction inside the selection poisons the medians
    sel = gt[4] > 0.1
    assert_close(EC.compute_errors(dg[4][torch.from_numpy(sel).cuda()], dp[4][torch.from_numpy(sel).cuda()]),
                 CR.compute_errors(gt[4][sel], pred[4][sel]), rtol=1e-4, atol=0, what="compute_errors")
    bad = dp.clone()
    bad[3][torch.from_numpy(gt[3] > 0.1).cuda()] = float("nan")
    m = host(EC.completion_medians(bad, dg))
    assert np.isnan(m[3, 0]) and np.isnan(m[3, 2]) and not np.isnan(m[3, 1]) and not np.isnan(m[4]).any()


def eval_scene(seed, N=2, H=352, W=1216):
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    truth = np.stack([(6.0 + 0.05 * n + 30.0 * (1.0 - v / H) + 2.0 * np.sin(u / 90.0)) for n in range(N)]).astype(np.float32)
    gt = np.where(rng.random((N, H, W)) < 0.1, truth, 0.0).astype(np.float32)
    gt[:, :120] = 0.0
    pred = (truth * rng.uniform(0.4, 0.6, (N, 1, 1)) * (1.0 + 0.05 * np.sin(u / 200.0)) + rng.normal(0, 0.05, (N, H, W))).astype(np.float32)
    pred[:, :4] = 1e-5                                           # below MIN_DEPTH, outside the mask
    beam = np.zeros((N, H, W), np.float32)
    for row in (200, 230, 260, 300):
        beam[:, row, ::3] = truth[:, row, ::3]
    return gt, pred, beam


def test_evaluate_completion_predictions_at_full_size():
    """N = 2 at 352x1216 against the per-image numpy recipe of evaluate_completion.py:297-355; with eval_gdc the scores are those of a
    direct gdc.GDC call on the scaled prediction (wiring only: GDC has its own tests)."""
    from fusiondepth_amd import evaluate_completion as EC, gdc as G
    gt, pred, beam = eval_scene(8)
    dg, dp = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()
    med = host(EC.completion_medians(dp, dg, 0.1, 1.3))          # 352 * 1216 is a multiple of 4: the float4 passes of the select
    for n in range(2):
        m = gt[n] > 0.1
        p = pred[n] * np.float32(1.3)
        assert same(med[n], np.array([np.median(gt[n][m]) / np.median(p[m]), np.median(gt[n][m]), np.median(p[m]), m.sum()], np.float32))
    odd = host(EC.completion_medians(dp[:, 1:, 1:], dg[:, 1:, 1:]))      # 351 * 1215 is odd: the element-wise passes at full size
    for n in range(2):
        m = gt[n, 1:, 1:] > 0.1
        assert same(odd[n, 1:3], np.array([np.median(gt[n, 1:, 1:][m]), np.median(pred[n, 1:, 1:][m])], np.float32))
    for scale, median in ((1.0, True), (5.4, False)):
        mean, ratios, per = EC.evaluate_completion_predictions(dp[:, None], dg[:, None], scale, not median)
        want = []
        for n in range(2):
            ratio, g_, p_ = CR.scored(pred[n].copy(), gt[n], scale, median)
            if median:
                assert ratios[n] == ratio
            want.append(CR.compute_errors(g_, p_))
        assert ratios.shape == ((2,) if median else (0,)) and per.shape == (2, 4)
        assert_close(per, np.array(want, np.float64), rtol=1e-4, atol=0, what="per-image errors")
        assert_close(mean, np.array(want, np.float64).mean(0), rtol=1e-4, atol=0, what="mean errors")
    K = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791]])
    cam = types.SimpleNamespace(c_u=K[0, 2], c_v=K[1, 2], f_u=K[0, 0], f_v=K[1, 1], b_x=K[0, 3] / -K[0, 0], b_y=K[1, 3] / -K[1, 1])
    far = pred.copy()
    far[:, :190] = 200.0                                         # beyond GDC's 80 m: keeps its point set small
    far[:, 310:] = 200.0
    dfar = torch.from_numpy(far).cuda()
    band = gt.copy()                                             # ground truth inside the same rows, so that the median ratio is the scene's
    band[:, :190] = 0.0
    band[:, 310:] = 0.0
    dg = torch.from_numpy(band).cuda()
    mean, ratios, per, maps = EC.evaluate_completion_predictions(dfar, dg, 1.0, False, True, torch.from_numpy(beam).cuda(), [cam, cam],
                                                                 return_maps=True)
    corrected = []
    for n in range(2):
        scaled = (dfar[n] * np.float32(1.0)) * torch.from_numpy(ratios).cuda()[n]
        gtd = torch.from_numpy(beam[n].astype(np.float64)).cuda()
        gtd[gtd == 0] = -1
        out, info = G.GDC(scaled, gtd, cam, W_tol=3e-5, recon_tol=5e-4, consider_range=(-3, 9), k=10, method="cg", return_info=True)
        assert info.status == "converged" and info.N_L > 100 and not torch.equal(out, scaled)
        corrected.append(out)
    assert torch.equal(maps.view(torch.int32), torch.stack(corrected).view(torch.int32))      # the corrected maps, bit for bit
    want = host(EC.completion_errors(torch.stack(corrected), dg, None, 0.1, 1.0))[:, :4]
    assert np.array_equal(per.view(np.uint64), want.view(np.uint64))
    plain = EC.evaluate_completion_predictions(dfar, dg, return_maps=True)
    assert not np.array_equal(per, plain[2])
    assert torch.equal(plain[3], (dfar * np.float32(1.0)) * torch.from_numpy(plain[1]).cuda()[:, None, None])
    # a correction that raises is reported and the image is scored uncorrected, as the reference's try / except does
    failed = EC.evaluate_completion_predictions(dfar, dg, 1.0, False, True, torch.from_numpy(beam).cuda(), [cam, None], return_maps=True)
    assert torch.equal(failed[3][0], maps[0]) and torch.equal(failed[3][1], plain[3][1]) and np.array_equal(failed[2][1], plain[2][1])
    with pytest.raises(ValueError, match="eval_gdc needs"):
        EC.evaluate_completion_predictions(dfar, dg, eval_gdc=True)


# ---------------------------------------------------------------------------------------------- end to end
def test_completor_trains_from_the_tree_and_the_script_scores_it(tree, tmp_path):
    """``Completor(opts).train(KITTICompletionBatches(...))`` for one epoch of 2 batches (ResNet-18), its checkpoint scored in this
    process (validation split) and by ``python -m fusiondepth_amd.evaluate_completion --completion_test`` in a child process: four
    finite metrics, and PNGs that decode to ``(pred * 256)`` as uint16."""
    from PIL import Image
    from fusiondepth_amd import evaluate_completion as EC
    from fusiondepth_amd.completion_data import KITTICompletionBatches
    from fusiondepth_amd.completor import Completor
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.predict import Predictor
    data = os.path.dirname(tree)                                 # --data_path: the tree is <data_path>/completion
    common = ["--num_layers", "18", "--completion_num_layers", "18", "--weights_init", "scratch", "--data_path", data, "--png",
              "--completion_not_full_res", "--log_dir", str(tmp_path / "log")]
    opt = MonodepthOptions().parse(common + ["--batch_size", "2", "--completion_num_epochs", "1", "--log_frequency", "1"])
    torch.manual_seed(3)
    cp = Completor(opt, verbose=False)
    before = cp.flat.flat_param.clone()
    loader = KITTICompletionBatches(tree, opt.height, opt.width, opt.frame_ids, 4, is_train=True, opt=opt, batch_size=2, shuffle=True, seed=2)
    loader.filenames = loader.filenames[:4]                      # one epoch of 2 batches
    cp.train(loader)
    torch.cuda.synchronize()
    loader.close()
    assert cp.step == 2 and np.isfinite(cp.last_log_time["loss"])
    after = cp.flat.flat_param
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    folder = cp.save_model("e2e")
    del cp

    eval_flags = common + ["--load_weights_folder", folder, "--eval_mono", "--eval_batch_size", "2"]
    mean, ratios, per = EC.evaluate(MonodepthOptions().parse(eval_flags))
    assert per.shape == (len(CT.SELECT), 4) and ratios.shape == (len(CT.SELECT),) and np.isfinite(per).all() and np.isfinite(mean).all()

    out_dir = str(tmp_path / "test_result")
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "fusiondepth_amd.evaluate_completion"] + eval_flags +
                         ["--completion_test", "--eval_out_dir", out_dir], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-3000:]
    line = [ln for ln in run.stdout.splitlines() if ln.startswith("&")][-1]
    metrics = [float(v) for v in line.strip("\\").replace("&", " ").split()]
    assert len(metrics) == 4 and np.isfinite(metrics).all()
    # the same predictions in this process: the PNGs hold (pred * ratio * 256) as uint16
    topt = MonodepthOptions().parse(eval_flags + ["--completion_test"])
    topt.need_4beam = True
    topt.eval_gdc = True                                         # for "full_res_4beam": what the script scores against in this mode
    predictor = Predictor(folder, num_layers=18)
    tl = KITTICompletionBatches(tree, topt.height, topt.width, [0], 4, opt=topt, batch_size=2, drop_last=False)
    preds, gts = [], []
    for batch in tl:
        preds.append(EC.predict_depths(predictor, batch, topt))
        gts.append(batch["full_res_4beam"][:, 0])
    tl.close()
    pred, gt = torch.cat(preds), torch.cat(gts)
    assert pred.shape == (len(CT.TEST), 384, 1280) and float(pred.min()) >= 1e-3 and float(pred.max()) <= 80
    ratio = EC.completion_medians(pred, gt)[:, :1, None]
    want = host(pred * ratio * 256.0).astype(np.uint16)
    for i in range(len(CT.TEST)):
        got = np.array(Image.open(os.path.join(out_dir, "%010d.png" % i)))
        assert got.dtype == np.uint16 and np.array_equal(got, want[i]), (i, int((got != want[i]).sum()))
    here = EC.evaluate_completion_predictions(pred, gt)[0]
    assert_close(metrics, here, rtol=0, atol=6e-4, what="the child's printed metrics (3 decimals)")
