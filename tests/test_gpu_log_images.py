"""``train --log_images`` on the device: ``fd_log_sheets`` (through ``fusiondepth_amd.log_images``) against its numpy restatement
(tests/log_images_ref.py, which tests/test_log_images_cpu.py holds against torch) - every byte of every sheet outside the colour
predictions, the background included, and every bit of the minima and maxima, no tolerance -, the colour predictions against the
project's own materialised warp (``FD.photo_loss(..., materialize=True)``, which tests/test_gpu_losspath.py holds to the oracle),
repeatability, the wrapper's refusals and the command end to end."""
import json
import os

import numpy as np
import pytest
import torch

import kitti_tree
import log_images_ref as LR

pytestmark = pytest.mark.gpu
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).reshape(-1).view(np.uint32)


def _case(H, W, scales, frame_ids, B, mode, seed):
    """Random dicts in numpy: colours beyond [0, 1], and per disparity tile - in turn over item + scale - values outside [0, 1], a
    constant plane, a plane with NaNs (and an infinity).  ``sel`` holds indices on both sides of ``n_id - 1``."""
    rng = np.random.RandomState(seed)
    nf = len(frame_ids) - 1
    inputs, outputs = {}, {}
    for si, s in enumerate(scales):
        h, w = H // 2 ** s, W // 2 ** s
        for f in frame_ids:
            inputs[("color", f, s)] = rng.uniform(-0.1, 1.1, (B, 3, h, w)).astype(F32)
        disp = (rng.randn(B, 1, h, w) * 0.8 + 0.4).astype(F32)
        for b in range(B):
            kind = (b + si + seed) % 3
            if kind == 1:
                disp[b] = F32(0.3125)
            elif kind == 2:
                disp[b, 0, rng.randint(h), rng.randint(w)] = np.nan
                disp[b, 0, 0, 0] = np.inf
        outputs[("disp", s)] = disp
        mh, mw = (h, w) if mode == "automask_v1" else (H, W)
        n_id = max(nf, 1)
        outputs[("sel", s)] = (rng.randint(0, n_id + max(nf, 1), (B, mh, mw)).astype(np.uint8), n_id)
    outputs["predictive_mask"] = {("disp", s): rng.uniform(-0.2, 1.2, (B, max(nf, 1), H // 2 ** s, W // 2 ** s)).astype(F32) for s in scales}
    K = np.tile(np.array([[0.58 * W, 0, 0.5 * W, 0], [0, 1.92 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1]], F32), (B, 1, 1))
    inputs[("K", 0)], inputs[("inv_K", 0)] = K, np.linalg.inv(K).astype(F32)
    Ts = {}
    for f in frame_ids[1:]:
        T = np.tile(np.eye(4, dtype=F32), (B, 1, 1))
        T[:, :3, 3] = rng.uniform(-0.05, 0.05, (B, 3))
        Ts[f] = T
    return inputs, outputs, Ts


def _upload(d):
    up = lambda v: torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v
    out = {}
    for k, v in d.items():
        out[k] = {kk: up(vv) for kk, vv in v.items()} if isinstance(v, dict) else ((up(v[0]), v[1]) if isinstance(v, tuple) else up(v))
    return out


def _flags(mode):
    return dict(automask=mode in ("automask", "automask_v1"), predictive_mask=mode == "predictive", val=mode == "val",
                v1_multiscale=mode == "automask_v1")


CASES = [
    # H, W, scales, frame ids, J, first, mode
    (32, 64, [0, 1, 2, 3], [0, -1, 1], 4, 0, "automask"),
    (32, 64, [0, 1, 2, 3], [0, -1, 1, "s"], 1, 1, "automask"),
    (32, 64, [0, 1, 2, 3], [0, -1, 1], 4, 0, "automask_v1"),
    (32, 64, [0, 1, 2, 3], [0], 4, 0, "val"),
    (32, 64, [0, 1, 2, 3], [0, -1, 1, "s"], 4, 0, "predictive"),
    (7, 13, [0], [0], 1, 0, "val"),
    (7, 13, [0], [0, -1, 1], 4, 0, "automask"),
    (7, 13, [0, 1], [0, -1, 1, "s"], 1, 2, "plain"),
    (7, 13, [0, 1], [0, -1, 1], 4, 0, "predictive"),
    (5, 9, [0], [0, -1, 1, "s"], 4, 0, "automask"),
    (5, 9, [0, 1], [0], 1, 0, "val"),
    (5, 9, [0, 1], [0, -1, 1], 1, 3, "automask_v1"),
    (5, 9, [0], [0, -1, 1], 1, 0, "plain"),
]


@pytest.mark.parametrize("H,W,scales,frame_ids,J,first,mode", CASES,
                         ids=["%dx%d-S%d-F%d-J%d-%s" % (c[0], c[1], len(c[2]), len(c[3]), c[4], c[6]) for c in CASES])
def test_sheets_equal_the_restatement(H, W, scales, frame_ids, J, first, mode):
    from fusiondepth_amd import log_images as L
    B = 4
    for seed in (0, 1, 2):                                        # every disparity tile takes each of the three kinds of content once
        inputs, outputs, Ts = _case(H, W, scales, frame_ids, B, mode, seed)
        kw = _flags(mode)
        sheets, tiles, stats = L.render(_upload(inputs), _upload(outputs), frame_ids, scales, J, Ts=_upload(Ts), first=first,
                                        want_stats=True, **kw)
        lay = L.layout(frame_ids, scales, H, W, J=J, automask=kw["automask"], predictive_mask=kw["predictive_mask"], val=kw["val"],
                       mask_size="scale" if kw["v1_multiscale"] else None)
        assert sheets.dtype == np.uint8 and sheets.shape == (J, lay.Hs, lay.Ws, 3) and sorted(tiles) == sorted(t.tag for t in lay.tiles)
        for j in range(J):
            got = sheets[j].copy()
            preds = {}
            for f in frame_ids[1:]:                               # the warp is not restated: its tiles are taken over, then compared as equal
                preds[f] = tiles["color_pred_%s_0/%d" % (f, j)].copy()
            want, want_stats = LR.restate(inputs, outputs, frame_ids, scales, first + j, preds, kw["automask"], kw["predictive_mask"],
                                          kw["val"], "scale" if kw["v1_multiscale"] else None)
            assert got.shape == want.shape and np.array_equal(got, want), (seed, j, np.argwhere(got != want)[:5])
            for t in lay.tiles:
                if t.item == j:
                    assert np.array_equal(tiles[t.tag], want[t.y:t.y + t.h, t.x:t.x + t.w]) and tiles[t.tag].shape == (t.h, t.w, 3), t.tag
            for tag, (mi, ma) in want_stats.items():
                g_mi, g_ma = stats["%s/%d" % (tag, j)]
                if np.isnan(ma):
                    assert np.isnan(g_mi) and np.isnan(g_ma) and (tiles["%s/%d" % (tag, j)] == 0).all(), tag
                else:
                    assert np.array_equal(_bits([g_mi, g_ma]), _bits([mi, ma])), (tag, j, g_mi, g_ma, mi, ma)
        if seed == 2:
            continue
        # the test's own inputs: the background is there and is black, a mask tile holds both values
        cover = np.zeros((lay.Hs, lay.Ws), bool)
        for t in lay.tiles[:len(lay.tiles) // J]:
            cover[t.y:t.y + t.h, t.x:t.x + t.w] = True
        assert (sheets[:, ~cover] == 0).all()
        if kw["automask"]:
            assert set(np.unique(tiles["automask_%d/0" % scales[-1]])) == {0, 255}


def test_every_kind_of_disparity_tile_was_drawn():
    """The three contents of ``_case`` all occur in the cases above (a constant plane: the 1e5 branch; NaNs; a range beyond [0, 1])."""
    seen = set()
    for H, W, scales, frame_ids, J, first, mode in CASES:
        for seed in (0, 1, 2):
            seen |= {(b + si + seed) % 3 for b in range(first, first + J) for si in range(len(scales))}
    assert seen == {0, 1, 2}


# --------------------------------------------------------------------------------------------- the colour predictions
@pytest.fixture(scope="module")
def scene():
    """``synthetic.make_scene_batch`` at 32 x 64, batch 4, frames -1, 1 and the stereo partner; a smooth disparity; the warps the
    project's loss kernel materialises for them, downloaded once."""
    from fusiondepth_amd import functional as FD, synthetic
    H, W, B = 32, 64, 4
    frame_ids = [0, -1, 1, "s"]
    inputs = synthetic.make_scene_batch(B, H, W, num_scales=1, frame_ids=frame_ids, seed=77, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(78)
    coarse = torch.rand(B, 1, 4, 8, device="cuda", generator=gen)
    disp = (0.05 + 0.5 * torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)).contiguous()
    Ts = {f: (inputs["stereo_T"] if f == "s" else inputs[("T_gt", f)]).contiguous() for f in frame_ids[1:]}
    po = FD.PhotoOptions(0.1, 100.0)
    with torch.no_grad():
        res = FD.photo_loss(disp, [Ts[f] for f in frame_ids[1:]], inputs[("K", 0)], inputs[("inv_K", 0)],
                            [inputs[("color", f, 0)] for f in frame_ids[1:]], inputs[("color", 0, 0)], None, None, None, po, True)
    color = res[5].cpu().numpy()                                  # [NF, B, 3, H, W]
    return inputs, {("disp", 0): disp}, Ts, frame_ids, color


def test_colour_predictions_against_the_materialised_warp(scene):
    """Every byte within one level of the quantised materialised warp, at most 0.5 % of a tile's bytes different at all: two correct
    float32 evaluations of the warp can land on either side of an integer of x * 255 (expected share about 1e-4); a wrong sampling
    convention changes most bytes.  A condition, not a measurement."""
    from conftest import report
    from fusiondepth_amd import log_images as L
    inputs, outputs, Ts, frame_ids, color = scene
    sheets, tiles = L.render(inputs, outputs, frame_ids, [0], 4, Ts=Ts, automask=False)
    worst_share = 0.0
    for i, f in enumerate(frame_ids[1:]):
        for j in range(4):
            got = tiles["color_pred_%s_0/%d" % (f, j)].astype(np.int32)
            want = LR.quantise(color[i, j]).transpose(1, 2, 0).astype(np.int32)
            assert got.shape == want.shape == (32, 64, 3)
            assert got.min() != got.max() and np.unique(got).size > 16, "a blank picture"
            diff = np.abs(got - want)
            share = float((diff != 0).mean())
            worst_share = max(worst_share, share)
            print("color_pred_%s_0/%d: max |d| %d, share of bytes that differ %.5f" % (f, j, diff.max(), share))
            assert diff.max() <= 1, (f, j, diff.max())
            assert share <= 0.005, (f, j, share)
            # and it is the warp, not the source frame copied over
            src = LR.quantise(inputs[("color", f, 0)][j].cpu().numpy()).transpose(1, 2, 0).astype(np.int32)
            assert (np.abs(got - src) > 1).mean() > 0.05
    report("log_images: worst share of colour-prediction bytes that differ from the materialised warp", worst_share, 0.005)


def test_two_calls_give_the_same_bytes(scene):
    from fusiondepth_amd import log_images as L
    inputs, outputs, Ts, frame_ids, _ = scene
    outputs = dict(outputs)
    outputs[("sel", 0)] = (torch.randint(0, 6, (4, 32, 64), device="cuda", dtype=torch.uint8), 3)
    a, tiles_a = L.render(inputs, outputs, frame_ids, [0], 4, Ts=Ts)
    b, _ = L.render(inputs, outputs, frame_ids, [0], 4, Ts=Ts)
    assert np.array_equal(a, b)
    one, tiles_one = L.render(inputs, outputs, frame_ids, [0], 1, Ts=Ts)
    assert one.shape == (1,) + a.shape[1:] and np.array_equal(one[0], a[0])
    assert np.array_equal(tiles_one["automask_0/0"], tiles_a["automask_0/0"])
    third, _ = L.render(inputs, outputs, frame_ids, [0], 1, Ts=Ts, first=2)
    assert np.array_equal(third[0], a[2])
    shared = dict(Ts, s=Ts["s"][:1].contiguous())                 # one matrix shared by the items: the stereo baseline is the same for all
    c, _ = L.render(inputs, outputs, frame_ids, [0], 4, Ts=shared)
    assert np.array_equal(a, c)


def test_render_refuses_before_any_launch(scene, monkeypatch):
    from fusiondepth_amd import _lib, log_images as L
    inputs, outputs, Ts, frame_ids, _ = scene

    def no_launch(name, *a):
        raise AssertionError("launched %s" % name)
    monkeypatch.setattr(_lib, "call", no_launch)
    kw = dict(Ts=Ts, automask=False)
    with pytest.raises(ValueError, match="J must be"):
        L.render(inputs, outputs, frame_ids, [0], 0, **kw)
    with pytest.raises(ValueError, match="items"):
        L.render(inputs, outputs, frame_ids, [0], 5, **kw)
    missing = {k: v for k, v in inputs.items() if k != ("color", 1, 0)}
    with pytest.raises(ValueError, match=r"\('color', 1, 0\).* missing"):
        L.render(missing, outputs, frame_ids, [0], 2, **kw)
    with pytest.raises(ValueError, match="missing"):
        L.render(inputs, {}, frame_ids, [0], 2, **kw)
    with pytest.raises(ValueError, match="missing"):                     # the automask needs the loss's selection
        L.render(inputs, outputs, frame_ids, [0], 2, Ts=Ts)
    with pytest.raises(ValueError, match="missing"):
        L.render(inputs, outputs, frame_ids, [0], 2, Ts={-1: Ts[-1]}, automask=False)
    wrong = dict(inputs)
    wrong[("color", -1, 0)] = inputs[("color", -1, 0)][:, :, :, :63].contiguous()
    with pytest.raises(ValueError, match="shape"):
        L.render(wrong, outputs, frame_ids, [0], 2, **kw)
    with pytest.raises(ValueError, match="shape"):
        L.render(inputs, {("disp", 0): outputs[("disp", 0)][:, :, :16].contiguous()}, frame_ids, [0], 2, **kw)
    short = dict(inputs)
    short[("color", 1, 0)] = inputs[("color", 1, 0)][:3].contiguous()
    with pytest.raises(ValueError, match="holds 3 items"):
        L.render(short, outputs, frame_ids, [0], 2, **kw)
    host = dict(inputs)
    host[("color", -1, 0)] = inputs[("color", -1, 0)].cpu()
    with pytest.raises(ValueError, match="GPU only"):
        L.render(host, outputs, frame_ids, [0], 2, **kw)


# --------------------------------------------------------------------------------------------- the command
H, W = 192, 640


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The tiny KITTI tree of tests/test_gpu_train_cli.py and the same short command twice: with ``--log_images`` and without."""
    from fusiondepth_amd import kitti_utils as KU, train as T
    root = str(tmp_path_factory.mktemp("kitti"))
    lines = kitti_tree.make_tree(root, [("2011_09_26", "2011_09_26_drive_0001_sync", (375, 1242), (1.0, 1.0))], frames=6, down=0.35)
    splits = str(tmp_path_factory.mktemp("splits"))
    for name, file in (("eigen_zhou", "train_files.txt"), ("eigen", "test_files.txt")):
        os.makedirs(os.path.join(splits, name))
        with open(os.path.join(splits, name, file), "w") as f:
            f.write("\n".join(lines) + "\n")
    KU.export_gt_depths(root, lines, "eigen", os.path.join(splits, "eigen", "gt_depths.npz"))
    logs = str(tmp_path_factory.mktemp("logs"))
    flags = ["--num_layers", "18", "--weights_init", "scratch", "--height", str(H), "--width", str(W), "--batch_size", "2",
             "--data_path", root, "--png", "--log_dir", logs, "--num_workers", "4", "--num_epochs", "1", "--log_frequency", "1",
             "--splits_dir", splits, "--seed", "5", "--val_limit", "2"]
    plain = T.main(flags + ["--model_name", "plain"])
    assert plain.log_images is False and plain.image_sink is None and plain._last_val_io is None
    del plain
    pictures = T.main(flags + ["--model_name", "pictures", "--log_images"])
    return logs, pictures


def test_command_writes_the_pictures_and_leaves_training_alone(runs):
    from PIL import Image
    from fusiondepth_amd import log_images as L
    logs, tr = runs
    a, b = os.path.join(logs, "plain"), os.path.join(logs, "pictures")
    assert not os.path.exists(os.path.join(a, "train", "images")) and not os.path.exists(os.path.join(a, "val", "images"))
    sa, sb = [json.load(open(os.path.join(p, "train_summary.rank0.json"))) for p in (a, b)]
    assert sa["steps"] == sb["steps"] == 2
    assert sa["param_checksum"] == sb["param_checksum"] and sa["last_loss"] == sb["last_loss"] and sa["items"] == sb["items"]
    for mode in ("train", "val"):                                 # the scalars are what they are without the switch
        ra, rb = [[json.loads(l) for l in open(os.path.join(p, mode, "scalars.jsonl"))] for p in (a, b)]
        assert len(ra) == 2 and ra == rb, mode
        assert sorted(os.listdir(os.path.join(b, mode, "images"))) == ["0000001_0.png", "0000002_0.png"], mode    # J = min(4, eval_batch_size = 1)
    assert tr.log_images and isinstance(tr.image_sink, L.PngSink) and tr.image_sink._thread is None               # joined
    # the sheets have the layout's size, and the last training event's PNG holds the bytes the renderer gives on _last_io
    lay = L.layout([0, -1, 1], [0, 1, 2, 3], H, W)
    train_png = np.asarray(Image.open(L.PngSink.path(b, "train", 2, 0)))
    assert train_png.shape == (lay.Hs, lay.Ws, 3) == (4 * H, 7 * W, 3)
    val_png = np.asarray(Image.open(L.PngSink.path(b, "val", 2, 0)))
    assert val_png.shape == (H + H // 2 + H // 4 + H // 8, 2 * W, 3)
    caught = []
    tr.image_sink = lambda mode, step, sheets, tiles: caught.append((mode, step, sheets, tiles))
    tr.log_pictures("train", *tr._last_io)
    (mode, step, sheets, tiles), = caught
    assert (mode, step) == ("train", 2) and sheets.shape == (1,) + train_png.shape and np.array_equal(sheets[0], train_png)
    # items: the window's last micro-batch is the whole batch of 2 here, drawn from its first item
    inputs, outputs = tr._last_io
    direct, _ = L.render(inputs, outputs, [0, -1, 1], [0, 1, 2, 3], 1, Ts={f: outputs[("cam_T_cam", 0, f)] for f in (-1, 1)},
                         min_depth=tr.opt.min_depth, max_depth=tr.opt.max_depth)
    assert np.array_equal(direct[0], train_png)
    # the picture shows something: the colours are the batch's, the prediction and the disparity are not blank
    assert np.array_equal(tiles["color_0_0/0"], LR.quantise(inputs[("color", 0, 0)][0].cpu().numpy()).transpose(1, 2, 0))
    for tag in ("color_pred_-1_0/0", "color_pred_1_0/0", "disp_0/0", "disp_3/0"):
        assert tiles[tag].min() != tiles[tag].max(), tag
    assert tiles["disp_0/0"].max() == 255 and tiles["disp_0/0"].min() == 0
    assert set(np.unique(tiles["automask_0/0"])) <= {0, 255}
    assert val_png[:H, :W].min() != val_png[:H, :W].max() and (val_png[H:, W + W // 2:] == 0).all()                 # background
