"""CPU checks of the depth-completion data path: the numpy restatement (tests/completion_ref.py) against what the reference itself
returned (tests/golden/completion_*.npz, written by tests/golden/make_completion.py), ``completion_paths`` on the synthetic tree, the
descriptor tables of ``fd_depth_png_keys`` against hand-computed offsets, and the loud failure without a GPU."""
import ctypes
import os

import numpy as np
import pytest

import completion_ref as CR
import completion_tree as CT

ITEMS = {"train": (True, 1), "train_flip": (True, 4), "val": (False, 2), "test": (False, 1)}
JITTER = ((1.13, 0.85, 1.2, -0.07), (2, 0, 3, 1))                # make_completion.JITTER
FRAMES = [0, -1, 1]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return CT.make_tree(str(tmp_path_factory.mktemp("completion") / "completion"))


def golden_item(golden, name, mode):
    g = golden("completion_%s_%s" % (name, mode))
    planes = lambda k: g[k].astype(np.float32) / np.float32(255)              # colour is stored as ToTensor's uint8 numerator
    return g, planes


def ref_item(tree, name, mode, colour=True):
    is_train, index = ITEMS[name]
    nfr = mode == "pad"
    opt = CT.options(completion_not_full_res=nfr, completion_test=name == "test", eval_gdc=True, need_path=True)
    split = "test_completion" if name == "test" else ("train" if is_train else "val")
    paths = CR.completion_paths(tree, split, "select")
    flip, aug = name == "train_flip", name == "train_flip"
    h, w = (192, 640) if nfr else (352, 1216)
    if colour:
        return CR.item(paths, index, opt, is_train, FRAMES, h, w, 4, flip, JITTER if aug else None), paths
    return CR.depth_keys(paths, index, opt, is_train, FRAMES, flip), paths


@pytest.mark.parametrize("mode", ["full", "pad"])
@pytest.mark.parametrize("name", list(ITEMS))
def test_restatement_equals_the_reference_bit_for_bit(tree, golden, name, mode):
    """Pins completion_ref, which the GPU tests then use at shapes the golden does not hold."""
    g, planes = golden_item(golden, name, mode)
    it, paths = ref_item(tree, name, mode)
    assert str(g["path"]) == os.path.relpath(paths["rgb"][ITEMS[name][1]], tree)
    checked = 0
    for k in g:
        if k in ("4beam", "depth_gt", "full_res_4beam"):
            assert it[k].dtype == np.float32 and np.array_equal(it[k], g[k]), k
        elif k.startswith("2channel_"):
            two = it[("2channel", int(k.split("_")[1]), 0)]
            assert np.array_equal(two[0], g[k]) and np.array_equal(two[1], g[k]), k
        elif k.startswith("color"):
            kind = "color_aug" if k.startswith("color_aug") else "color"
            rest = k[len(kind) + 1:].split("_")
            got = it[(kind, int(rest[0]), int(rest[1]))]
            if len(rest) == 3:
                r = int(rest[2][4:])
                got = got[:, r:r + 4]
            assert np.array_equal(got, planes(k)), k
        else:
            continue
        checked += 1
    assert checked >= (4 if name == "test" else 6)
    assert ("depth_gt" in it) == (name != "test") and "full_res_4beam" in it
    assert it["4beam"].shape == ((1, 192, 640) if mode == "pad" else (1, 352, 1216))
    assert it["full_res_4beam"].shape == (1, 384, 1280)


def test_scatter_oracle_equals_gen2cha_completion(tree, golden):
    """The project's scatter oracle with gen2cha_completion.py's window equals the reference's get_4beam_2channel on the cropped
    sparse map / 100: the online 2-channel map needs no 2cha/*.npy files."""
    from oracle import scatter as OS
    g = golden("completion_scatter")
    paths = CR.completion_paths(tree, "train", "select")
    for k in range(2):
        png = CR.load_png(paths["d"][int(g["index%d" % k])])
        four = CR.get_depth(png, False, False, False, False)[0] / np.float32(100.0)
        depth, conf = OS.scatter_2channel_np(four, roi=CT.ROI, expand=2)
        assert np.array_equal(depth, g["depth%d" % k]) and np.array_equal(conf, g["conf%d" % k])
        assert (g["depth%d" % k][:CT.ROI[0] - 2] == 0).all() and g["conf%d" % k].max() == 1.0


def test_scorer_restatement_equals_the_reference(golden):
    """completion_ref's recipe (selection, scaling, clamp, float32 means of the float32 terms) against what the reference's
    compute_errors and np.median returned for the seeded pairs."""
    import make_completion as MC
    g = golden("completion_metrics")
    gt, pred = MC.metric_pairs(int(g["seed"]))
    for n, count in enumerate(MC.METRIC_COUNTS):
        if count == 0:
            continue
        for tag, scale in (("", 1.0), ("_s", 1.3)):
            ratio, gs, ps = CR.scored(pred[n].copy(), gt[n], scale)
            assert ratio == g["ratio%d%s" % (n, tag)] and gs.size == count
            assert np.array_equal(np.array(CR.compute_errors(gs, ps), dtype=np.float64), g["errors%d%s" % (n, tag)]), (n, tag)


def test_completion_paths(tree, golden):
    from fusiondepth_amd.completion_data import completion_paths
    g = golden("completion_paths")
    rel = lambda ps: ["" if p is None else os.path.relpath(p, tree) for p in ps]
    for split, val_split in (("train", "select"), ("val", "select"), ("val", "full"), ("test_completion", "select")):
        got = completion_paths(tree, split, val_split)
        want = CR.completion_paths(tree, split, val_split)
        for k in ("rgb", "d", "gt"):
            assert rel(got[k]) == [str(p) for p in g["%s_%s_%s" % (split, val_split, k)]] == rel(want[k]), (split, val_split, k)
    train = completion_paths(tree, "train")
    assert len(train["d"]) == sum(len(v) for v in CT.TRAIN_KEPT.values()) == 8
    kept = {}
    for p in train["d"]:
        kept.setdefault(p.split("/")[-5], []).append(int(os.path.basename(p)[:10]))
    assert kept == CT.TRAIN_KEPT                                  # frame 7 and 9 of drive 0002 lack frame 8; the ends lack a neighbour
    assert len(completion_paths(tree, "train", verify=False)["d"]) == sum(len(v) for v in CT.TRAIN_FRAMES.values())
    for d, rgb, gt in zip(train["d"], train["rgb"], train["gt"]):
        drive, n = d.split("/")[-5], os.path.basename(d)
        assert rgb == "/".join([tree, "data_rgb", "train", drive, "image_02", "data", n]) and os.path.isfile(rgb)
        assert gt.split("/")[-5] == drive and os.path.basename(gt) == n
    full = completion_paths(tree, "val", "full")
    assert len(full["rgb"]) == len(CT.VAL_FRAMES) and all(os.path.isfile(p) and "/data_rgb/val/" in p for p in full["rgb"])
    sel = completion_paths(tree, "val", "select")
    assert len(sel["rgb"]) == len(CT.SELECT) and all(os.path.isfile(p) and "/image/" in p and "groundtruth" not in p for p in sel["rgb"])
    test = completion_paths(tree, "test_completion")
    assert test["gt"] == [None, None] and len(test["d"]) == 2 and all(os.path.isfile(p) for p in test["rgb"] + test["d"])
    with pytest.raises(ValueError, match="Unrecognized split"):
        completion_paths(tree, "testing")
    with pytest.raises(RuntimeError, match="Found 0 images"):
        completion_paths(os.path.join(tree, "nowhere"), "train")
    with pytest.raises(RuntimeError, match="Found 0 images"):
        completion_paths(tree, "test_prediction")                # the tree has no test_depth_prediction_anonymous
    with pytest.raises(RuntimeError, match="different sizes"):   # an image without its sparse map
        _unequal(tree)


def _unequal(tree):
    import shutil
    import tempfile
    from fusiondepth_amd.completion_data import completion_paths
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "depth_selection/test_depth_completion_anonymous")
        shutil.copytree(os.path.join(tree, "depth_selection/test_depth_completion_anonymous"), dst)
        os.remove(os.path.join(dst, "velodyne_raw/%010d.png" % 1))
        completion_paths(tmp, "test_completion")


SOURCES = [(375, 1242), (376, 1241), (374, 1238), (370, 1226), (370, 1224)]
#            crop origin (i, j)        pad origin (y, x)
EXPECTED = {(375, 1242): ((23, 13), (9, 19)), (376, 1241): ((24, 12), (8, 19)), (374, 1238): ((22, 11), (10, 21)),
            (370, 1226): ((18, 5), (14, 27)), (370, 1224): ((18, 4), (14, 28))}


@pytest.mark.parametrize("h,w", SOURCES)
def test_descriptor_tables_against_hand_computed_offsets(h, w):
    from fusiondepth_amd import _lib, completion_data as CD, data_ops
    (i, j), (y, x) = EXPECTED[(h, w)]
    assert CD.crop_origin(h, w) == (i, j) and CD.pad_origin(h, w) == (y, x)
    assert CD.crop_origin(376, 1241)[1] == 12                    # (1241 - 1216) / 2 = 12.5 rounds half to even, not to 13
    for flip in (False, True):
        assert CD.depth_desc(7, h, w, flip, True, False) == ((7, h, w, flip, i, j, 0, 0, 352, 1216), (352, 1216))
        assert CD.depth_desc(7, h, w, flip, True, True) == ((7, h, w, flip, i, j, 32, 32, 352, 1216), (384, 1280))
        assert CD.depth_desc(7, h, w, flip, False, True) == ((7, h, w, flip, 0, 0, y, x, h, w), (384, 1280))
        # the colour crop / pad runs on the host before the device mirrors: offsets are the mirrored ones for a flipped item
        assert CD.colour_placement(h, w, flip, True) == ((352, 1216), (i, w - 1216 - j if flip else j), (0, 0), (352, 1216))
        assert CD.colour_placement(h, w, flip, False) == ((384, 1280), (0, 0), (y, 1280 - w - x if flip else x), (h, w))
    with pytest.raises(ValueError):
        CD.depth_desc(0, h, w, False, False, False)
    table = data_ops.depth_png_desc_table([CD.depth_desc(8, h, w, True, True, True)[0], CD.depth_desc(8 + h * w, h, w, False, False, True)[0]])
    assert ctypes.sizeof(_lib.DepthPngDesc) == 48 and len(bytes(table)) == 96
    raw = np.frombuffer(bytes(table), dtype=np.int32).reshape(2, 12)
    assert raw[0].tolist() == [8, 0, h, w, 1, i, j, 32, 32, 352, 1216, 0]
    assert raw[1].tolist() == [8 + h * w, 0, h, w, 0, 0, 0, y, x, h, w, 0]


def test_colour_placement_equals_mirror_then_crop():
    """crop at the mirrored offset, mirror afterwards == the reference's mirror, then crop (and the same for the pad)."""
    from fusiondepth_amd import completion_data as CD
    rng = np.random.default_rng(3)
    for h, w in SOURCES:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for flip in (False, True):
            for full_res in (True, False):
                canvas, (sy, sx), (dy, dx), (rows, cols) = CD.colour_placement(h, w, flip, full_res)
                out = np.zeros(canvas + (3,), np.uint8)
                out[dy:dy + rows, dx:dx + cols] = img[sy:sy + rows, sx:sx + cols]
                if flip:
                    out = out[:, ::-1]
                assert np.array_equal(out, CR.get_color(img, flip, not full_res)), (h, w, flip, full_res)


def test_same_size_lanczos_table_is_the_identity():
    """Scale 0 of the full-res pyramid is a same-size resample; Pillow returns a copy there.  The fixed-point Lanczos table at ratio 1
    has one tap of weight 1 << 22 per output, so fd_resize_lanczos_u8 copies too and needs no special case."""
    from fusiondepth_amd import data_ops
    for n in (352, 1216):
        tab, k = data_ops.lanczos_table(n, n)
        for o in range(n):
            first, count = tab[o, 0], tab[o, 1]
            coef = tab[o, 2:2 + count]
            assert coef[o - first] == 1 << 22 and coef.sum() == 1 << 22 and np.count_nonzero(coef) == 1


def test_loader_plan_and_loud_failure_without_a_gpu(tree):
    import torch
    from fusiondepth_amd import completion_data as CD, evaluate_completion as EC
    opt = CT.options(eval_gdc=True)
    loader = CD.KITTICompletionBatches(tree, 352, 1216, FRAMES, 4, is_train=True, opt=opt, batch_size=2, device="cpu",
                                       draws=lambda e, i: {"do_color_aug": False, "do_flip": i % 2 == 0, "jitter": None})
    assert len(loader) == 4 and loader.split == "train"
    items = loader.plan_batch(0, [3, 4])                         # 375x1242 and 376x1241 in one batch
    plan = loader._plan_depth(items)
    assert [len(plan["tables"][k]) for k in ("beam", "gt", "full")] == [6, 2, 2]
    assert len(plan["planes"]) == 6 + 2 and all(off % 4 == 0 for off, _, _ in plan["planes"].values())
    assert plan["tables"]["beam"][0][:4] == (plan["planes"][items[0]["beams"][0]][0], 375, 1242, False)
    assert plan["tables"]["beam"][1][1:6] == (376, 1241, True, 24, 12) and plan["tables"]["full"][1][6:] == (32, 32, 352, 1216)
    assert items[0]["date"] == "2011_09_26" and items[1]["date"] == "2011_09_28"
    assert CD.KITTICompletionBatches(tree, 352, 1216, [0], 4, opt=CT.options(completion_test=True), device="cpu").split == "test_completion"
    with pytest.raises(NotImplementedError, match="completion_need2channel"):
        CD.KITTICompletionBatches(tree, 192, 640, [0], 4, opt=CT.options(completion_not_full_res=True, completion_need2channel="true"))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            next(iter(loader))
        with pytest.raises(RuntimeError, match="GPU"):
            next(iter(CD.KITTICompletionBatches(tree, 352, 1216, [0], 4, opt=CT.options())))
        with pytest.raises(RuntimeError, match="GPU"):
            EC.compute_errors(torch.ones(5), torch.ones(5))
        with pytest.raises(RuntimeError, match="GPU"):
            EC.evaluate_completion_predictions(torch.ones(1, 4, 4), torch.ones(1, 4, 4))
    loader.close()
