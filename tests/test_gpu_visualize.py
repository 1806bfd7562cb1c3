"""``evaluate_depth --visualize`` on the device: ``fd_vis_render`` (through ``fusiondepth_amd.visualize``) against its numpy restatement
(tests/visualize_ref.py, which tests/test_visualize_cpu.py holds against numpy and matplotlib) - every byte of the two pictures and
every bit of (vmin, vmax), no tolerance -, the depth chain against ``depth_export``, chunking, both sources, ``colorize_disparity``,
the wrapper's refusals and the script end to end."""
import os

import numpy as np
import pytest
import torch

import kitti_tree
import visualize_ref as VR

pytestmark = pytest.mark.gpu
F32 = np.float32
LUT_DISP, LUT_ERR = VR.random_luts()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _render(*args, **kw):
    from fusiondepth_amd.visualize import render
    kw.setdefault("lut_disp", LUT_DISP)
    kw.setdefault("lut_err", LUT_ERR)
    return render(*args, **kw)


def _check(got_c, got_e, got_s, depth, gt, split, what):
    want_c, want_e, (vmin, vmax) = VR.restate(depth, gt, split, LUT_DISP, LUT_ERR)
    assert got_s.dtype == F32 and np.array_equal(_bits(got_s), _bits(np.array([vmin, vmax], F32))), (what, got_s, vmin, vmax)
    assert got_c.dtype == np.uint8 and got_c.shape == want_c.shape and np.array_equal(got_c, want_c), (what, np.argwhere(got_c != want_c)[:5])
    assert got_e.dtype == np.uint8 and got_e.shape == want_e.shape and np.array_equal(got_e, want_e), (what, np.argwhere(got_e != want_e)[:5])
    return want_e


@pytest.fixture(scope="module")
def small():
    """Seven maps of the sizes of tests/visualize_ref.py from 6x20 disparities, ground truth for both splits, ratios; computed once."""
    rng = np.random.RandomState(41)
    disps = rng.uniform(0.02, 0.5, (len(VR.SIZES),) + VR.SRC).astype(F32)
    ratios = rng.uniform(0.7, 1.4, len(VR.SIZES)).astype(F32)
    depths = [VR.depth_of(d, s, 1.0, r) for d, s, r in zip(disps, VR.SIZES, ratios)]
    gts = {split: [VR.ground_truth(rng, p, split) for p in depths] for split in ("eigen", "eigen_benchmark")}
    return disps, ratios, depths, gts


@pytest.mark.parametrize("split", ["eigen", "eigen_benchmark"])
def test_pictures_equal_the_restatement(small, split):
    from fusiondepth_amd.detection import depth_export
    disps, ratios, depths, gts = small
    dev = torch.from_numpy(disps).cuda()
    colors, errors, stats, maps = _render(dev, gts[split], ratios, split, want_stats=True, want_depth=True)
    assert len(colors) == len(errors) == len(maps) == len(VR.SIZES) and stats.shape == (len(VR.SIZES), 2)
    _, exported = depth_export(dev, VR.SIZES, ratios=ratios, want_depth=True)
    scored = 0
    for i, size in enumerate(VR.SIZES):
        got = maps[i].cpu().numpy()
        assert np.array_equal(_bits(got), _bits(depths[i])) and np.array_equal(_bits(got), _bits(exported[i].cpu().numpy())), size
        want_e = _check(colors[i], errors[i], stats[i], depths[i], gts[split][i], split, (split, size))
        scored += int((want_e != 220).any())
    assert scored >= (1 if split == "eigen" else 5)              # the pictures are not all grey
    if split == "eigen":                                          # 1x1: the Garg crop selects nothing -> an all-220 picture
        assert errors[0].shape == (1, 1, 3) and (errors[0] == 220).all()
    # without the optional outputs, and every image alone (N = 1)
    plain = _render(dev, gts[split], ratios, split)
    assert len(plain) == 2
    for i, size in enumerate(VR.SIZES):
        assert np.array_equal(plain[0][i], colors[i]) and np.array_equal(plain[1][i], errors[i]), size
        c, e = _render(dev[i:i + 1], gts[split][i:i + 1], ratios[i:i + 1], split)
        assert np.array_equal(c[0], colors[i]) and np.array_equal(e[0], errors[i]), size


def test_no_selected_pixel_gives_a_grey_picture(small):
    disps, ratios, depths, gts = small
    i = VR.SIZES.index((37, 41))
    empty = np.zeros((37, 41), F32)
    (c,), (e,) = _render(disps[i:i + 1], [empty], ratios[i:i + 1], "eigen_benchmark")
    assert e.shape == (19, 21, 3) and (e == 220).all()
    assert np.array_equal(c, VR.colorize(depths[i], LUT_DISP)[0])


def _special_maps():
    rng = np.random.RandomState(8)
    const = np.full((9, 14), 0.137, F32)
    levels = (F32(0.02) + rng.randint(0, 16, (24, 40)).astype(F32) * F32(0.03)).astype(F32)
    top = rng.uniform(0.02, 0.4, (24, 40)).astype(F32)
    top.reshape(-1)[rng.choice(top.size, 100, replace=False)] = F32(0.5)      # more than 5 % share the largest disparity
    return [("constant", const), ("16 levels", levels), ("top == vmax", top)]


@pytest.mark.parametrize("name,disp", _special_maps(), ids=[n for n, _ in _special_maps()])
def test_special_maps(name, disp):
    """vmin == vmax; ties across the selected rank; a top value equal to vmax (xa == 256 -> the last entry).  Identity resize."""
    rng = np.random.RandomState(5)
    depth = VR.depth_of(disp, disp.shape)
    gt = VR.ground_truth(rng, depth, "eigen_benchmark")
    (c,), (e,), stats = _render(disp[None], [gt], None, "eigen_benchmark", want_stats=True)
    _check(c, e, stats[0], depth, gt, "eigen_benchmark", name)
    if name == "constant":
        assert stats[0, 0] == stats[0, 1] and (c == LUT_DISP[0]).all()
    if name == "16 levels":
        assert len(np.unique(F32(1) / depth)) <= 16
    if name == "top == vmax":
        d = F32(1) / depth
        assert stats[0, 1] == d.max() and (c == LUT_DISP[255]).all(axis=2).sum() >= 100


def test_full_size_map():
    """One 375x1242 map from 192x640: n = 465 750, where the float32 virtual index is 442 461.53125."""
    rng = np.random.RandomState(17)
    assert VR.virtual_index(VR.BIG[0] * VR.BIG[1]) == (442461, 0.53125)
    disp = rng.uniform(0.02, 0.5, VR.BIG_SRC).astype(F32)
    ratio = np.array([1.21], F32)
    depth = VR.depth_of(disp, VR.BIG, 1.0, ratio[0])
    gt = VR.ground_truth(rng, depth, "eigen")
    (c,), (e,), stats = _render(disp[None], [gt], ratio, "eigen", want_stats=True)
    want_e = _check(c, e, stats[0], depth, gt, "eigen", "375x1242")
    assert e.shape == (188, 621, 3) and (want_e != 220).any() and (want_e[:70] == 220).all()      # above the Garg crop: grey


def test_chunks_sources_and_repeats(small):
    """Five images with per-image ratios: chunk=2 (borders inside the list) equals chunk=64; the depth_in route equals the disp route
    on the same maps; two calls give the same bytes."""
    disps, ratios, depths, gts = small
    pick = [6, 2, 5, 0, 4]                                        # 37x41, 2x3, 7x5, 1x1, 1x41
    d = torch.from_numpy(disps[pick]).cuda()
    g, r = [gts["eigen_benchmark"][i] for i in pick], ratios[pick]
    whole = _render(d, g, r, "eigen_benchmark", want_stats=True, want_depth=True, chunk=64)
    for other in (_render(d, g, r, "eigen_benchmark", want_stats=True, want_depth=True, chunk=2),
                  _render(d, g, r, "eigen_benchmark", want_stats=True, want_depth=True, chunk=64),
                  _render(None, g, None, "eigen_benchmark", depths=whole[3], want_stats=True, want_depth=True, chunk=3),
                  _render(None, g, None, "eigen_benchmark", depths=[depths[i] for i in pick], want_stats=True, want_depth=True)):
        assert np.array_equal(_bits(other[2]), _bits(whole[2]))
        for k in range(len(pick)):
            assert np.array_equal(other[0][k], whole[0][k]) and np.array_equal(other[1][k], whole[1][k]), k
            assert np.array_equal(_bits(other[3][k].cpu().numpy()), _bits(whole[3][k].cpu().numpy())), k
    for k, i in enumerate(pick):
        _check(whole[0][k], whole[1][k], whole[2][k], depths[i], g[k], "eigen_benchmark", VR.SIZES[i])


def test_colorize_disparity_equals_render():
    from fusiondepth_amd import functional as FD
    from fusiondepth_amd.visualize import colorize_disparity, magma_lut
    assert FD.colorize_disparity is colorize_disparity
    rng = np.random.RandomState(23)
    disp = rng.uniform(0.01, 0.9, (3, 13, 37)).astype(F32)
    dev = torch.from_numpy(disp).cuda()
    gts = [np.zeros((13, 37), F32)] * 3
    colors, _ = _render(dev, gts, None, "eigen_benchmark", lut_disp=magma_lut())
    got = colorize_disparity(dev)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, 13, 37, 3)
    assert np.array_equal(got.cpu().numpy(), np.stack(colors))
    assert torch.equal(colorize_disparity(dev[:, None]), got)
    assert np.array_equal(colorize_disparity(dev, LUT_DISP).cpu().numpy()[1], VR.colorize(VR.depth_of(disp[1], (13, 37)), LUT_DISP)[0])


def test_unaligned_buffers_and_bad_descriptors(small):
    """The library call itself with pictures that start 1, 5 and 16 bytes past a 16-byte boundary: the head length comes from the
    address, nothing outside the pictures is written; a descriptor that leaves the buffers, or names no prediction, writes nothing."""
    from fusiondepth_amd import _lib
    from fusiondepth_amd.evaluate_depth import pack_gt_depths
    from fusiondepth_amd.visualize import err_size
    disps, ratios, depths, gts = small
    g = gts["eigen_benchmark"]
    N = len(g)
    dev = torch.from_numpy(disps).cuda()
    packed, desc = pack_gt_depths(g, "eigen_benchmark")
    total = packed.numel()
    packed_d, ratio_d = packed.cuda(), torch.from_numpy(ratios).cuda()
    luts = torch.from_numpy(np.concatenate([LUT_DISP, LUT_ERR])).cuda()
    sizes = [err_size(*m.shape) for m in g]
    err_pixels = sum(h * w for h, w in sizes)
    want = [VR.restate(p, m, "eigen_benchmark", LUT_DISP, LUT_ERR) for p, m in zip(depths, g)]
    want_c = np.concatenate([c.reshape(-1) for c, _, _ in want])
    want_e = np.concatenate([e.reshape(-1) for _, e, _ in want])
    ws = torch.empty((_lib.query("fd_vis_render_ws_bytes", N, total),), device="cuda", dtype=torch.uint8)
    assert ws.numel() > 0 and _lib.query("fd_vis_render_ws_bytes", 65, total) == 0
    pad = 40

    def run(desc_np, shift, use_c=True, use_e=True):
        c = torch.full((3 * total + 2 * pad,), 0xAA, device="cuda", dtype=torch.uint8)
        e = torch.full((3 * err_pixels + 2 * pad,), 0xAA, device="cuda", dtype=torch.uint8)
        desc_d = torch.from_numpy(desc_np.view(np.uint8).copy()).cuda()
        _lib.call("fd_vis_render", dev.data_ptr(), N, VR.SRC[0], VR.SRC[1], 1.0, ratio_d.data_ptr(), None, packed_d.data_ptr(), total,
                  desc_d.data_ptr(), N, 37 * 41, 0.0, float("inf"), luts.data_ptr(), luts.data_ptr() + 768,
                  c.data_ptr() + shift if use_c else None, e.data_ptr() + shift if use_e else None, err_pixels, None, None, ws.data_ptr(),
                  _lib.stream())
        return c.cpu().numpy(), e.cpu().numpy()

    for shift, use_c, use_e in ((1, True, True), (5, True, False), (16, False, True), (0, True, True), (15, True, True)):
        ch, eh = run(desc, shift, use_c, use_e)
        if use_c:
            assert np.array_equal(ch[shift:shift + 3 * total], want_c), shift
            ch[shift:shift + 3 * total] = 0xAA
        if use_e:
            assert np.array_equal(eh[shift:shift + 3 * err_pixels], want_e), shift
            eh[shift:shift + 3 * err_pixels] = 0xAA
        assert (ch == 0xAA).all() and (eh == 0xAA).all(), shift
    bad = desc.copy()
    bad["offset"][4] = total - 5                                  # 1x41 leaves the packed planes
    bad["pred"][5] = N                                            # 7x5 names no prediction
    bad["x1"][2] = 4                                              # 2x3: the window leaves the plane
    ch, eh = run(bad, 0)
    at = 0
    for i, (d, (h2, w2)) in enumerate(zip(desc, sizes)):
        o, n = 3 * int(d["offset"]), 3 * int(d["H"]) * int(d["W"])
        if i in (2, 4, 5):
            assert (ch[o:o + n] == 0xAA).all(), i                # nothing written, and the error pictures behind it move up
        else:
            assert np.array_equal(ch[o:o + n], want_c[o:o + n]), i
            assert np.array_equal(eh[at:at + 3 * h2 * w2], want[i][1].reshape(-1)), i
            at += 3 * h2 * w2
    assert (eh[at:] == 0xAA).all() and (ch[3 * total:] == 0xAA).all()
    for args in ((dev.data_ptr(), packed_d.data_ptr()), (None, None)):      # both sources, or neither
        with pytest.raises(RuntimeError, match="fd_vis_render"):
            _lib.call("fd_vis_render", args[0], N, VR.SRC[0], VR.SRC[1], 1.0, None, args[1], packed_d.data_ptr(), total,
                      torch.from_numpy(desc.view(np.uint8).copy()).cuda().data_ptr(), N, 37 * 41, 0.0, float("inf"), luts.data_ptr(),
                      luts.data_ptr() + 768, None, None, err_pixels, ws.data_ptr(), None, ws.data_ptr(), _lib.stream())


def test_wrapper_refusals(small):
    from fusiondepth_amd.visualize import colorize_disparity
    disps, ratios, depths, gts = small
    g = gts["eigen"]
    with pytest.raises(ValueError, match="6 maps for 7"):
        _render(disps[:6], g, None)
    with pytest.raises(ValueError, match="3 ratios for 7"):
        _render(disps, g, ratios[:3])
    with pytest.raises(ValueError, match="non-empty"):
        _render(disps[:1], [np.zeros((0, 5), F32)], None)
    with pytest.raises(ValueError, match="lut_disp"):
        _render(disps, g, None, lut_disp=np.zeros((255, 3), np.uint8))
    with pytest.raises(ValueError, match="lut_err"):
        _render(disps, g, None, lut_err=np.zeros((256, 3), np.float32))
    with pytest.raises(ValueError, match="chunk"):
        _render(disps, g, None, chunk=65)
    with pytest.raises(ValueError, match="not both"):
        _render(disps, g, None, depths=depths)
    with pytest.raises(ValueError, match="depth map 1 has shape"):
        _render(None, g[:2], None, depths=[depths[0], depths[0]])
    with pytest.raises(ValueError, match="colorize_disparity"):
        colorize_disparity(torch.zeros((2, 3, 4, 5), device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- the script
H, W = 192, 640
SIZES = {"2011_09_26": (375, 1242), "2011_09_30": (370, 1226)}


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """A ``Trainer.save_model`` folder from a seeded random ResNet-18 (the recipe of tests/test_gpu_eigen_eval.py)."""
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.trainer import Trainer
    tmp = tmp_path_factory.mktemp("visualize_models")
    torch.manual_seed(5)
    net = Trainer(MonodepthOptions().parse(["--num_layers", "18", "--weights_init", "scratch", "--batch_size", "2", "--height", str(H),
                                            "--width", str(W), "--log_dir", str(tmp / "stage1")]), verbose=False)
    saved = net.save_model("init")
    del net
    return saved


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    """A three-image split over a two-drive tree with different image sizes, and its ``gt_depths.npz``."""
    from fusiondepth_amd import kitti_utils as KU
    root = str(tmp_path_factory.mktemp("kitti"))
    lines = kitti_tree.make_tree(root, [("2011_09_26", "2011_09_26_drive_0001_sync", SIZES["2011_09_26"], (1.0, 1.0)),
                                        ("2011_09_30", "2011_09_30_drive_0016_sync", SIZES["2011_09_30"], (1.0, 1.0))], frames=4, down=0.35)
    lines = [lines[3], lines[0], lines[1]]
    splits = str(tmp_path_factory.mktemp("splits"))
    os.makedirs(os.path.join(splits, "eigen"))
    with open(os.path.join(splits, "eigen", "test_files.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    gts = KU.export_gt_depths(root, lines, "eigen", os.path.join(splits, "eigen", "gt_depths.npz"))
    assert [g.shape for g in gts] == [SIZES[l.split("/")[0]] for l in lines]
    KU.export_gt_depths(root, lines, "4beam", os.path.join(splits, "eigen", "4beam.npz"))      # read by --eval_gdc alone
    return root, splits, gts


def test_script_end_to_end(folder, split, tmp_path):
    from PIL import Image
    from fusiondepth_amd import evaluate_depth as ED
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.visualize import render
    root, splits, gts = split
    common = ["--num_layers", "18", "--data_path", root, "--png", "--load_weights_folder", folder, "--eval_mono", "--eval_batch_size", "2",
              "--save_pred_disps"]
    vis = str(tmp_path / "vis")
    got = ED.main(["--splits_dir", splits, "--vis_dir", vis, "--visualize", "--vis_name", "t"] + common)
    # the same disparities without the flag (loaded, so that the network runs once)
    plain = ED.evaluate(MonodepthOptions().parse(["--eval_mono", "--ext_disp_to_eval", os.path.join(folder, "disps_eigen_split.npy")]), splits)
    assert len(got) == len(plain) == 3
    for a, b in zip(got, plain):                                  # the flag changes nothing it does not add
        assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))
    disps = np.load(os.path.join(folder, "disps_eigen_split.npy"))
    colors, errors, maps = render(disps, gts, got[1], "eigen", want_depth=True)
    names = {"%drgb.png" % i for i in range(3)} | {"%dt.png" % i for i in range(3)} | {"%dtdepth.png" % i for i in range(3)}
    assert set(os.listdir(os.path.join(vis, "prediction"))) == names
    assert set(os.listdir(os.path.join(vis, "npy"))) == {"%dt%s.npy" % (i, k) for i in range(3) for k in ("pred_depth", "diff", "mask")}
    for i, gt in enumerate(gts):
        assert np.array_equal(np.array(Image.open(os.path.join(vis, "prediction", "%dt.png" % i))), errors[i])
        assert np.array_equal(np.array(Image.open(os.path.join(vis, "prediction", "%dtdepth.png" % i))), colors[i])
        assert (errors[i] != 220).any() and len(np.unique(colors[i].reshape(-1, 3), axis=0)) > 50
        rgb = np.array(Image.open(os.path.join(vis, "prediction", "%drgb.png" % i)))
        assert rgb.shape == (375, 1242, 3) and rgb.dtype == np.uint8 and rgb.std() > 1
        pred, diff, mask = (np.load(os.path.join(vis, "npy", "%dt%s.npy" % (i, k))) for k in ("pred_depth", "diff", "mask"))
        assert pred.shape == diff.shape == mask.shape == gt.shape and pred.dtype == diff.dtype == F32 and mask.dtype == bool
        assert np.array_equal(_bits(pred), _bits(maps[i].cpu().numpy())) and np.array_equal(_bits(diff), _bits(np.abs(pred - gt)))
        assert np.array_equal(mask, VR.split_mask(gt, "eigen")) and mask.any()


def test_script_with_gdc(folder, split, tmp_path):
    """--eval_gdc: the dense maps reach the renderer through ``on_depth``, rounded to float32 once; ``beam_depth.npy`` is written."""
    from PIL import Image
    from fusiondepth_amd import evaluate_depth as ED
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.visualize import render
    root, splits, gts = split
    one = str(tmp_path / "splits")
    os.makedirs(os.path.join(one, "eigen"))
    with open(os.path.join(splits, "eigen", "test_files.txt")) as f:
        first = f.read().splitlines()[0]
    with open(os.path.join(one, "eigen", "test_files.txt"), "w") as f:
        f.write(first + "\n")
    beams = np.load(os.path.join(splits, "eigen", "4beam.npz"), allow_pickle=True)["data"]
    np.savez_compressed(os.path.join(one, "eigen", "gt_depths.npz"), data=np.array(gts[:1]))
    np.savez_compressed(os.path.join(one, "eigen", "4beam.npz"), data=np.array([np.asarray(beams[0], F32)]))
    common = ["--num_layers", "18", "--data_path", root, "--png", "--load_weights_folder", folder, "--eval_mono", "--eval_gdc"]
    plain = ED.evaluate(MonodepthOptions().parse(common), one)
    vis = str(tmp_path / "vis")
    got = ED.evaluate(MonodepthOptions().parse(common + ["--visualize"]), one, vis_dir=vis)
    assert len(got) == 3 and got[2] is None and plain[2] is None
    assert np.array_equal(_bits(got[0]), _bits(plain[0])) and np.array_equal(_bits(got[1]), _bits(plain[1]))
    assert set(os.listdir(os.path.join(vis, "npy"))) == {"0diff%s.npy" % k for k in ("pred_depth", "diff", "mask", "beam_depth")}
    pred = np.load(os.path.join(vis, "npy", "0diffpred_depth.npy"))
    assert pred.dtype == F32 and pred.shape == gts[0].shape and np.isfinite(pred).all()
    assert np.array_equal(np.load(os.path.join(vis, "npy", "0diffbeam_depth.npy")), beams[0])
    (c,), (e,) = render(None, gts[:1], None, "eigen", depths=[pred])
    assert np.array_equal(np.array(Image.open(os.path.join(vis, "prediction", "0diff.png"))), e)
    assert np.array_equal(np.array(Image.open(os.path.join(vis, "prediction", "0diffdepth.png"))), c)
    want_c, want_e, _ = VR.restate(pred, gts[0], "eigen", *[np.asarray(t) for t in _default_luts()])
    assert np.array_equal(c, want_c) and np.array_equal(e, want_e)


def _default_luts():
    from fusiondepth_amd.visualize import hue_lut, magma_lut
    return magma_lut(), hue_lut()
