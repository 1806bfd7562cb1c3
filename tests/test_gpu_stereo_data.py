"""``fusiondepth_amd.datasets.KITTIStereoBatches`` end to end on a synthetic KITTI tree with both cameras: the keys of the stereo
partner "s" against the existing loader - itself pinned bit-exact to PIL (tests/test_gpu_datasets.py) - reading the same lines with
the other side; every other key against the plain loader; ``stereo_T``; and one optimiser step of a ``--use_stereo`` Trainer on a
builder batch, for both frame sets."""
import os
import types

import numpy as np
import pytest
import torch

import kitti_tree as KT

pytestmark = pytest.mark.gpu

H, W, SCALES = 64, 96, 4
JITTERS = [((1.2, 0.8, 1.1, 0.1), [0, 1, 2, 3]), ((0.8, 1.2, 0.85, -0.1), [3, 2, 1, 0]), ((1.05, 0.95, 1.2, -0.04), [2, 0, 3, 1])]


def injected(epoch, index):
    """Flags and jitter parameters by item index: all four flag combinations occur."""
    aug, flip = bool(index % 2), bool((index // 2) % 2)
    return {"do_color_aug": aug, "do_flip": flip, "jitter": JITTERS[index % 3] if aug else None}


def _opt(**over):
    o = types.SimpleNamespace(need_4beam=True, need_2_channel=True, need_full_res_4beam=False, need_inf_gdc=False, clone_gdc=False,
                              need_path=True, nbeams=4, random_sample=-1)
    for k, v in over.items():
        setattr(o, k, v)
    return o


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """Two drives of different image size; ``kitti_tree.make_tree`` writes camera 2, the scans and the calibration (the same
    projection for both cameras), camera 3's images are added here."""
    from PIL import Image
    root = str(tmp_path_factory.mktemp("kitti_stereo"))
    drives = [("2011_09_26", "2011_09_26_drive_0001_sync", (128, 192), (192 / 1242.0, 128 / 375.0)),
              ("2011_09_30", "2011_09_30_drive_0016_sync", (120, 180), (180 / 1242.0, 120 / 375.0))]
    lines = KT.make_tree(root, drives, frames=5)
    rng = np.random.default_rng(78)
    for date, drive, (im_h, im_w), _ in drives:
        d = os.path.join(root, date, drive, "image_03/data")
        os.makedirs(d)
        for i in range(5):
            blocks = rng.integers(0, 256, (im_h // 16 + 1, im_w // 16 + 1, 3))
            img = np.repeat(np.repeat(blocks, 16, axis=0), 16, axis=1)[:im_h, :im_w] + rng.integers(-30, 31, (im_h, im_w, 3))
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(d, "%010d.png" % i))
    return root, lines                                          # 3 "l" lines per drive: 6 items, indices 0 .. 5


def _batches(cls, root, lines, frames, source, **kw):
    b = cls(root, lines, H, W, frames, SCALES, is_train=True, img_ext=".png", opt=_opt(), batch_size=len(lines), draws=injected,
            prefetch=False, lidar_source=source, **kw)
    batch = b.build_batch(0, list(range(len(lines))))
    torch.cuda.synchronize()
    b.close()
    return batch


@pytest.mark.parametrize("source", ["files", "raw"])
@pytest.mark.parametrize("frames", [[0, "s"], [0, -1, 1, "s"]])
def test_stereo_batch_against_the_plain_loader(tree, frames, source):
    from fusiondepth_amd.datasets import KITTIRAWBatches, KITTIStereoBatches
    root, lines = tree
    assert len(lines) == 6 and all(line.endswith(" l") for line in lines)
    temporal = [f for f in frames if f != "s"]
    got = _batches(KITTIStereoBatches, root, lines, frames, source)
    plain = _batches(KITTIRAWBatches, root, lines, temporal, source)
    other = _batches(KITTIRAWBatches, root, [line[:-1] + "r" for line in lines], [0], source)
    for s in range(SCALES):
        for name in ("color", "color_aug"):
            assert got[(name, "s", s)].shape == (6, 3, H >> s, W >> s)
            assert torch.equal(got[(name, "s", s)], other[(name, 0, s)]), (name, s)
            assert not torch.equal(got[(name, "s", s)], got[(name, 0, s)])
    # every other key is the plain loader's, bit for bit
    extra = {(name, "s", s) for name in ("color", "color_aug") for s in range(SCALES)} | {"stereo_T"}
    assert set(got) == set(plain) | extra
    assert ("2channel", "s", 0) not in got and ("2channel", 0, 0) in got
    for k, v in plain.items():
        if torch.is_tensor(v):
            assert got[k].shape == v.shape and torch.equal(got[k], v), k
        else:
            assert got[k] == v, k
    # mono_dataset.py:216-222 for "l" lines: -0.1, +0.1 where the item is flipped (indices 2, 3)
    T = got["stereo_T"]
    assert T.shape == (6, 4, 4) and T.dtype == torch.float32 and T.is_cuda
    want = torch.eye(4).repeat(6, 1, 1)
    want[:, 0, 3] = torch.tensor([0.1 if injected(0, i)["do_flip"] else -0.1 for i in range(6)])
    assert torch.equal(T.cpu(), want)


@pytest.mark.parametrize("per_image", [False, True])
def test_right_hand_lines_read_camera_2_as_their_partner(tree, per_image):
    """``r`` lines: "s" is ``image_02`` at the same frame index - what the plain loader reads for the same lines with side ``l``.
    With ``jitter_per_image`` the slot of "s" takes its own [scale] list of draws through the pyramid: the plain loader is given that
    list for its only frame."""
    from fusiondepth_amd.datasets import KITTIRAWBatches, KITTIStereoBatches
    root, lines = tree
    r_lines = [line[:-1] + "r" for line in lines]

    def per_slot(slots):
        def draws(epoch, index):
            d = dict(injected(epoch, index))
            if per_image and d["do_color_aug"]:
                d["jitter"] = [[JITTERS[(index + 2 * slot + s) % 3] for s in range(SCALES)] for slot in slots]
            return d
        return draws

    def build(cls, lns, frames, slots):
        b = cls(root, lns, H, W, frames, SCALES, is_train=True, img_ext=".png", opt=_opt(), batch_size=len(lns), draws=per_slot(slots),
                prefetch=False, jitter_per_image=per_image)
        batch = b.build_batch(0, list(range(len(lns))))
        torch.cuda.synchronize()
        b.close()
        return batch

    got = build(KITTIStereoBatches, r_lines, [0, "s"], [0, 1])
    own = build(KITTIRAWBatches, r_lines, [0], [0])              # frame 0 of the r lines, slot 0's draws
    other = build(KITTIRAWBatches, lines, [0], [1])              # camera 2 with the draws of slot 1, the slot of "s"
    for s in range(SCALES):
        for name in ("color", "color_aug"):
            assert torch.equal(got[(name, "s", s)], other[(name, 0, s)]), (name, s)
            assert torch.equal(got[(name, 0, s)], own[(name, 0, s)]), (name, s)
    if per_image:                                                # the two slots really were jittered differently
        plain = build(KITTIRAWBatches, lines, [0], [0])
        assert not torch.equal(plain[("color_aug", 0, 0)], other[("color_aug", 0, 0)])


def test_stereo_T_of_right_hand_lines(tree):
    from fusiondepth_amd.datasets import KITTIStereoBatches
    root, lines = tree
    got = _batches(KITTIStereoBatches, root, [line[:-1] + "r" for line in lines[:4]], [0, "s"], "files")
    assert torch.equal(got["stereo_T"][:, 0, 3].cpu(), torch.tensor([0.1, 0.1, -0.1, -0.1]))      # flipped: indices 2, 3
    assert torch.equal(got["stereo_T"][:, :3, :3].cpu(), torch.eye(3).repeat(4, 1, 1))


@pytest.mark.parametrize("source", ["files", "raw"])
@pytest.mark.parametrize("frame_ids", [["0"], ["0", "-1", "1"]])
def test_one_stereo_train_step_on_a_builder_batch(tree, tmp_path, frame_ids, source):
    from fusiondepth_amd.datasets import KITTIStereoBatches
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.trainer import Trainer
    root, lines = tree
    opt = MonodepthOptions().parse(["--num_layers", "18", "--weights_init", "scratch", "--batch_size", "2", "--height", str(H), "--width",
                                    str(W), "--png", "--data_path", root, "--log_dir", str(tmp_path), "--use_stereo", "--frame_ids"]
                                   + frame_ids)
    torch.manual_seed(5)
    tr = Trainer(opt, verbose=False)
    assert tr.opt.frame_ids[-1] == "s"
    loader = KITTIStereoBatches(opt.data_path, lines, opt.height, opt.width, tr.opt.frame_ids, 4, is_train=True, img_ext=".png", opt=opt,
                                batch_size=opt.batch_size, draws=injected, lidar_source=source)
    batches = []
    for batch in loader:
        batches.append(batch)
        if len(batches) == tr.accumulate_step:
            break
    loader.close()
    out = tr.train_step(batches)
    torch.cuda.synchronize()
    assert torch.isfinite(out["loss"]).item() and torch.isfinite(tr.flat.flat_param).all().item()
