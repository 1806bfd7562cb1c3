"""The Refiner's data chain on the GPU: ``fd_resize_bilinear_batch`` against torch's CPU ``F.interpolate`` bit for bit,
``KITTIRefinerBatches`` against the reference's recipe on the CPU, the ``inf_depth_map`` producer against the Refiner's own frozen
forward and the oracle, and the whole chain ``inf_depth_map`` -> ``inf_gdc`` -> ``Refiner.train(KITTIRefinerBatches)`` on one tree."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kitti_tree

pytestmark = pytest.mark.gpu

FRAME_IDS = [0, -1, 1]


def _np(v):
    return v.cpu().numpy()


def _interp(x, size):
    """The expectation: torch on the CPU."""
    return F.interpolate(torch.from_numpy(x)[None, None], list(size), mode="bilinear", align_corners=False)[0, 0].numpy()


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel
def _pack(planes):
    descs, at = [], 0
    for p, mirror in planes:
        descs.append((at, p.shape[0], p.shape[1], mirror))
        at += p.size
    return torch.from_numpy(np.concatenate([p.reshape(-1) for p, _ in planes])).cuda(), descs


def _check_resize(planes, size):
    from fusiondepth_amd import functional as FD
    packed, descs = _pack(planes)
    got = FD.resize_bilinear_batch(packed, descs, size)                  # ONE call for all planes
    assert got.shape == (len(planes),) + tuple(size) and got.dtype == torch.float32
    got = _np(got)
    for k, (p, mirror) in enumerate(planes):
        plain = _interp(p, size)
        want = np.fliplr(plain) if mirror else plain
        assert np.array_equal(got[k].view(np.uint32), want.view(np.uint32)), \
            "plane %d (%s -> %s, mirror %s): %d of %d elements differ" % (k, p.shape, size, mirror, (got[k] != want).sum(), want.size)
        if mirror:          # resizing the mirrored SOURCE is another float32 result: an implementation that mirrors first fails above
            assert not np.array_equal(_interp(np.ascontiguousarray(np.fliplr(p)), size), want)
    return got


def test_resize_bilinear_batch_equals_torch_cpu_bitwise():
    rng = np.random.default_rng(31)
    planes = [(kitti_tree.depth_like(rng, h, w), m) for (h, w), m in zip(((94, 311), (93, 307), (96, 312), (40, 100)), (False, True, True, False))]
    assert all((p == 0).any() and p.max() < 80 for p, _ in planes)
    _check_resize(planes, (48, 160))
    _check_resize(planes, (64, 96))


def test_resize_bilinear_batch_full_size_and_device_table():
    from fusiondepth_amd import functional as FD
    rng = np.random.default_rng(32)
    planes = [(kitti_tree.depth_like(rng, 375, 1242), True), (kitti_tree.depth_like(rng, 370, 1226), False)]
    got = _check_resize(planes, (192, 640))
    # the descriptor table already on the device (how the loader calls it) gives the same result
    packed, descs = _pack(planes)
    table = torch.frombuffer(bytearray(bytes(FD.resize_desc_table(descs))), dtype=torch.uint8).cuda()
    assert np.array_equal(_np(FD.resize_bilinear_batch(packed, descs, (192, 640), desc_table=table)), got)
    with pytest.raises(ValueError, match="leaves the packed buffer"):
        FD.resize_bilinear_batch(packed, [(descs[1][0], 375, 1242, False)], (192, 640))
    with pytest.raises(RuntimeError, match="GPU"):
        FD.resize_bilinear_batch(packed.cpu(), descs, (192, 640))


# ------------------------------------------------------------------------------------------------------------------ 2. the loader
SIZES = {"2011_09_26": (375, 1242), "2011_09_30": (370, 1226)}
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
    root = str(tmp_path_factory.mktemp("kitti"))
    lines = kitti_tree.make_tree(root, [("2011_09_26", "2011_09_26_drive_0001_sync", SIZES["2011_09_26"], (1.0, 1.0)),
                                        ("2011_09_30", "2011_09_30_drive_0016_sync", SIZES["2011_09_30"], (1.0, 1.0))], full_scans=False)
    kitti_tree.write_gdc_maps(root, lines, SIZES)
    return root, lines


def _loader(cls, root, lines, opt, **kw):
    return cls(root, lines, 192, 640, FRAME_IDS, 4, is_train=True, img_ext=".png", opt=opt, batch_size=4, shuffle=True, seed=4,
               draws=injected, **kw)


def test_refiner_loader_inf_gdc_key(tree):
    from fusiondepth_amd.datasets import KITTIRAWBatches, KITTIRefinerBatches
    root, lines = tree
    assert len(lines) == 8
    a = _loader(KITTIRefinerBatches, root, lines, _opt(clone_gdc=True))
    b = _loader(KITTIRefinerBatches, root, lines, _opt(clone_gdc=True), prefetch=False)
    parent = _loader(KITTIRAWBatches, root, lines, _opt())
    order = a.epoch_order(0)
    ba, bb, bp = list(a), list(b), list(parent)
    torch.cuda.synchronize()
    assert len(ba) == len(bb) == len(bp) == 2
    mixed = 0
    for i, (x, y, p) in enumerate(zip(ba, bb, bp)):
        idx = order[4 * i:4 * i + 4]
        assert x["path"] == y["path"] == p["path"] == [lines[j] for j in idx]
        assert x["inf_gdc"].shape == (4, 192, 640) and x["inf_gdc"].dtype == torch.float32
        flips = [injected(0, j)["do_flip"] for j in idx]
        mixed += len(set(flips)) == 2 and len({lines[j].split("/")[0] for j in idx}) == 2
        got = _np(x["inf_gdc"])
        for k, j in enumerate(idx):
            want = kitti_tree.reference_gdc(kitti_tree.gdc_path(root, lines[j]), flips[k], (192, 640))
            assert np.array_equal(got[k].view(np.uint32), want.view(np.uint32)), (i, k, lines[j], int((got[k] != want).sum()))
        # every other key is the parent's, bit for bit; prefetched == unprefetched
        assert set(x) == set(y) == set(p) | {"inf_gdc"}
        for key in x:
            if torch.is_tensor(x[key]):
                assert np.array_equal(_np(x[key]), _np(y[key])), (i, key)
                if key != "inf_gdc":
                    assert np.array_equal(_np(x[key]), _np(p[key])), (i, key)
    assert mixed >= 1, "no batch mixes mirrored and unmirrored items of both dates: choose another seed"
    # evaluation with clone_gdc alone: no key; need_inf_gdc: the key, unmirrored
    ev = KITTIRefinerBatches(root, lines, 192, 640, [0], 4, is_train=False, img_ext=".png", opt=_opt(clone_gdc=True), batch_size=2)
    assert "inf_gdc" not in next(iter(ev))
    nv = KITTIRefinerBatches(root, lines, 192, 640, [0], 4, is_train=False, img_ext=".png", opt=_opt(need_inf_gdc=True), batch_size=3,
                             drop_last=False)
    last = list(nv)[-1]
    torch.cuda.synchronize()
    assert last["inf_gdc"].shape == (2, 192, 640) and last[("K", 0)].shape[0] == 2            # the trailing partial batch
    want = kitti_tree.reference_gdc(kitti_tree.gdc_path(root, lines[7]), False, (192, 640))
    assert np.array_equal(_np(last["inf_gdc"])[1], want)
    for l in (a, b, parent, ev, nv):
        l.close()


def test_refiner_loader_missing_or_wrong_map(tree, tmp_path):
    import shutil
    from fusiondepth_amd.datasets import KITTIRefinerBatches
    root, lines = tree
    two = KITTIRefinerBatches(root, lines, 192, 640, [0], 4, is_train=True, img_ext=".png", opt=_opt(clone_gdc=True, need_4beam=False,
                                                                                                     need_2_channel=False, random_sample=200),
                              batch_size=2, prefetch=False)
    missing = two.get_gdc_path(*lines[0].split()[:1], int(lines[0].split()[1]), "l")
    assert missing.endswith("inf_gdc_r200/1_l.npy")
    with pytest.raises(FileNotFoundError) as e:
        next(iter(two))
    assert missing in str(e.value) and "fusiondepth_amd.inf_gdc" in str(e.value)
    two.close()
    # a map whose size is not its date's: refused with the path, not resized from the wrong layout.  In a tree of its own (the
    # first date's calibration and frames copied), so that the shared one stays as the fixture made it
    own = str(tmp_path / "kitti")
    date, drive = lines[0].split()[0].split("/")
    os.makedirs(os.path.join(own, date, drive))
    shutil.copy(os.path.join(root, date, "calib_cam_to_cam.txt"), os.path.join(own, date))
    shutil.copy(os.path.join(root, date, "calib_velo_to_cam.txt"), os.path.join(own, date))
    shutil.copytree(os.path.join(root, date, drive, "image_02"), os.path.join(own, date, drive, "image_02"))
    kitti_tree.write_gdc_maps(own, lines[:2], {date: (370, 1226)})
    bad = KITTIRefinerBatches(own, lines[:2], 192, 640, [0], 4, is_train=True, img_ext=".png", opt=_opt(clone_gdc=True, need_4beam=False,
                                                                                                         need_2_channel=False),
                              batch_size=2, prefetch=False)
    with pytest.raises(RuntimeError, match="inf_gdc_4beam/1_l.npy"):
        next(iter(bad))
    bad.close()


# ------------------------------------------------------------------------------------------------------------------ 3. the producer
def _stage1_folder(tmp_path, height, width, seed=5):
    """A ``Trainer.save_model`` folder from a seeded random initialisation."""
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.trainer import Trainer
    o = MonodepthOptions().parse(["--num_layers", "18", "--weights_init", "scratch", "--batch_size", "2", "--height", str(height),
                                  "--width", str(width), "--log_dir", str(tmp_path / "stage1")])
    torch.manual_seed(seed)
    tr = Trainer(o, verbose=False)
    folder = tr.save_model("init")
    del tr
    return folder


def _refiner(tmp_path, folder, height, width, root, name, *extra):
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.refiner import Refiner
    o = MonodepthOptions().parse(["--num_layers", "18", "--weights_init", "scratch", "--batch_size", "2", "--height", str(height),
                                  "--width", str(width), "--png", "--data_path", root, "--log_dir", str(tmp_path / name),
                                  "--log_frequency", "1", "--num_epochs", "1", "--refine_load_weights_folder", folder] + list(extra))
    return Refiner(o, verbose=False)


def _rel_err(a, ref):
    """Worst element-wise relative error, the measure tests/test_gpu_trainer.py holds ("disp", s) to."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(a - ref) / np.maximum(np.abs(ref), 1e-30)).max())


def test_inf_depth_map_producer(tmp_path):
    import copy
    import conftest
    from fusiondepth_amd import inf_depth_map
    from fusiondepth_amd.datasets import KITTIRAWBatches
    from oracle import networks as ON
    H, W = 64, 96
    root = str(tmp_path / "kitti")
    # native 128x192 frames; the camera is scaled with the image so that the scans still cover it
    lines = kitti_tree.make_tree(root, [("2011_09_26", "2011_09_26_drive_0001_sync", (128, 192), (192 / 1242.0, 128 / 375.0))], frames=7,
                                 full_scans=False)
    assert len(lines) == 5
    split = tmp_path / "split.txt"
    split.write_text("\n".join(lines) + "\n")
    folder = _stage1_folder(tmp_path, H, W)
    argv = ["--load_weights_folder", folder, "--data_path", root, "--split_files", str(split), "--png", "--num_layers", "18",
            "--height", str(H), "--width", str(W), "--batch_size", "2"]
    assert inf_depth_map.main(argv) == 0
    args = inf_depth_map.parse_args(argv)
    got = {}
    for line in lines:
        path = inf_depth_map.out_path(args, line)
        assert path.startswith(root) and os.path.isfile(path), path
        got[line] = np.load(path)
        assert got[line].dtype == np.float32 and got[line].shape == (1, 1, H, W)
    assert len(os.listdir(os.path.dirname(path))) == 5
    # the Refiner's own frozen forward on the same batches (2 + 2 + 1 items).  inf_depth_map.py:166-170 hands the LiDAR encoder's
    # features to the depth decoder; the Refiner does with --refine_depthnet_with_beam true
    rf = _refiner(tmp_path, folder, H, W, root, "rf", "--refine_depthnet_with_beam", "true")
    loader = KITTIRAWBatches(root, lines, H, W, [0], 4, is_train=False, img_ext=".png", opt=inf_depth_map.loader_options(args), batch_size=2,
                             drop_last=False)
    sd = {k: torch.load(os.path.join(folder, k + ".pth"), map_location="cpu") for k in ("encoder", "beam_encoder", "depth")}
    o32 = {"encoder": ON.ResnetEncoder(18, False), "beam_encoder": ON.ResnetEncoder(18, False, beam_encoder=True)}
    o32["depth"] = ON.DepthDecoder(o32["encoder"].num_ch_enc, range(4))
    for k, net in o32.items():
        net.load_state_dict({n: v for n, v in sd[k].items() if n in net.state_dict()})
        net.eval()
    o64 = {k: copy.deepcopy(net).double().eval() for k, net in o32.items()}
    seen = 0
    for batch in loader:
        with torch.no_grad():
            _, _, depth, _ = rf._frozen_forward(batch, False, False)
            disp = _np(depth[("disp", 0)])
            color, two = batch["color_aug", 0, 0].cpu(), batch["2channel"].cpu()
            w32 = o32["depth"](o32["encoder"](color), beam_features=o32["beam_encoder"](two))[("disp", 0)].numpy()
            w64 = o64["depth"](o64["encoder"](color.double()), beam_features=o64["beam_encoder"](two.double()))[("disp", 0)].numpy()
        for k, line in enumerate(batch["path"]):
            assert np.array_equal(got[line].view(np.uint32), disp[k:k + 1].view(np.uint32)), (line, int((got[line] != disp[k:k + 1]).sum()))
            # worst element-wise relative error against float64 <= max(1e-4, 2 x the float32 oracle's own)
            e, e32 = _rel_err(got[line][0], w64[k]), _rel_err(w32[k], w64[k])
            conftest.report("inf_depth_map %s: disp vs the float64 oracle (worst element, relative)" % line.split()[1], e, max(1e-4, 2 * e32),
                            "(float32 oracle %.2e)" % e32)
            assert e <= max(1e-4, 2 * e32), (line, e, e32)
            seen += 1
    assert seen == 5
    loader.close()


# ------------------------------------------------------------------------------------------------------------------ 4. the chain
def test_chain_from_a_checkpoint_to_a_refiner_epoch(tmp_path):
    """``inf_depth_map.main`` -> ``inf_gdc.main`` -> ``Refiner(opts).train(KITTIRefinerBatches(...))`` on one tree, nothing fabricated
    in between; and the refine decoder after the epoch is bit-identical to a run fed the same batches from a pre-built list - the
    ``inf_gdc`` key takes part in the builder's stream hand-over race-free."""
    from fusiondepth_amd import inf_depth_map, inf_gdc
    from fusiondepth_amd.datasets import KITTIRefinerBatches
    H, W = 96, 320
    root = str(tmp_path / "kitti")
    # native 192x640 frames, camera scaled; scans that reach the bottom rows, where the Refiner's crop window [78:190, 23:617] lies
    lines = kitti_tree.make_tree(root, [("2011_09_26", "2011_09_26_drive_0001_sync", (192, 640), (640 / 1242.0, 192 / 375.0))], frames=6,
                                 full_scans=False, down=0.35)
    assert len(lines) == 4
    split = tmp_path / "split.txt"
    split.write_text("\n".join(lines) + "\n")
    folder = _stage1_folder(tmp_path, H, W)
    assert inf_depth_map.main(["--load_weights_folder", folder, "--data_path", root, "--split_files", str(split), "--png",
                               "--num_layers", "18", "--height", str(H), "--width", str(W), "--batch_size", "2"]) == 0
    inf_gdc.main(["--data_path", root, "--split_files", str(split)])
    for line in lines:
        m = np.load(kitti_tree.gdc_path(root, line))
        assert m.dtype == np.float32 and m.shape == (192, 640) and np.isfinite(m).all()

    def builder(opt, **kw):
        return KITTIRefinerBatches(opt.data_path, lines, opt.height, opt.width, opt.frame_ids, 4, is_train=True, img_ext=".png", opt=opt,
                                   batch_size=opt.batch_size, shuffle=True, seed=1, **kw)

    def run(name, feed):
        torch.manual_seed(5)
        rf = _refiner(tmp_path, folder, H, W, root, name)
        rf.opt.num_epochs = 1                                      # the constructor derives the epoch count from the batch size
        loader = feed(rf.opt)                                      # built from the Refiner's own options (clone_gdc is set there)
        torch.manual_seed(6)
        rf.train(loader)
        torch.cuda.synchronize()
        return rf

    a = run("a", lambda opt: builder(opt))
    assert a.step == 2 and np.isfinite(a.last_log_time["loss"])

    def prebuilt(opt):
        b = builder(opt, prefetch=False)
        batches = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()} for batch in b]
        torch.cuda.synchronize()
        b.close()
        assert len(batches) == 2
        for batch in batches:
            assert batch["inf_gdc"].shape == (2, H, W) and batch["4beam"].shape == (2, 1, H, W)
            inside = (batch["4beam"][:, 0, 78:190, 23:617] > 0).flatten(1).sum(1)
            assert (inside > 0).all(), "an item has no beam return inside the Refiner's crop window: %s" % inside.tolist()
        return batches

    b = run("b", prebuilt)
    assert b.step == 2
    pa, pb = a.flat.flat_param.cpu().numpy(), b.flat.flat_param.cpu().numpy()
    assert np.isfinite(pa).all() and np.array_equal(pa, pb), "%d parameters differ" % (pa != pb).sum()
    assert a.last_log_time["loss"] == b.last_log_time["loss"]
