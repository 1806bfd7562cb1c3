"""The pseudo-LiDAR export on the device: ``fd_points_export`` (through ``fusiondepth_amd.detection.points_export`` and directly) against
its numpy restatement (tests/pseudo_lidar_ref.py) - every byte of the points and every entry of ``starts``, no tolerance: each step of
the rule is one IEEE float64 operation on both sides -, the library's refusals, and ``export_detection --pl_name`` end to end."""
import os
import types

import numpy as np
import pytest
import torch

import detection_tree
import kitti_tree
import pseudo_lidar_ref as PR

pytestmark = pytest.mark.gpu
F32 = np.float32

# widths under 64, the lane tail (65), whole segments (64), several segments per row and a wave without one (130), more than one round
# of the four waves (513, 1030), a single row, a single pixel; an all-NaN map between ordinary ones must not shift the next start
EDGE_SIZES = [(1, 1), (1, 65), (3, 64), (4, 70), (5, 130), (2, 513), (9, 1030)]
ALL_NAN = 3
EDGE_MAX_HIGH = 0.5          # with depths in [2, 60] m and these cameras the rule keeps about half of each map (asserted below)


def edge_case(calib_dir, sizes=EDGE_SIZES, all_nan=ALL_NAN, seed=11):
    """-> (maps, calibs): depths uniform in [2, 60] m with NaN, +inf, 0 and negative values sprinkled in (2 % each); per-map cameras
    scaled to the map (c_u = W / 2, c_v = H / 2, f = 0.58 W) with the date folder's Velodyne transform."""
    from fusiondepth_amd import kitti_utils as KU
    A, t = KU.rect_to_velo(calib_dir)
    rng = np.random.RandomState(seed)
    maps, calibs = [], []
    for i, (H, W) in enumerate(sizes):
        m = rng.uniform(2.0, 60.0, (H, W)).astype(F32)
        kind = rng.randint(0, 50, (H, W))
        for k, value in enumerate((np.nan, np.inf, 0.0, -7.5)):
            m[kind == k] = value
        if i == all_nan:
            m[:] = np.nan
        maps.append(m)
        calibs.append((types.SimpleNamespace(c_u=W / 2.0, c_v=H / 2.0, f_u=0.58 * W, f_v=0.58 * W, b_x=0.06 + 0.001 * i, b_y=-0.003), A, t))
    return maps, calibs


@pytest.fixture(scope="module")
def edges(tmp_path_factory):
    """The edge maps, their restated clouds (computed once, never changed) and the device copies."""
    d = str(tmp_path_factory.mktemp("pl_calib") / "2011_09_26")
    kitti_tree.write_calib(d, 375, 1242)
    maps, calibs = edge_case(d)
    want, starts = PR.clouds(maps, calibs, EDGE_MAX_HIGH)
    for w in want:
        w.setflags(write=False)
    return maps, calibs, want, starts, [torch.from_numpy(m).cuda() for m in maps]


def _same_bytes(a, b):
    return a.dtype == b.dtype == F32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _raw_call(maps_d, calibs, max_high, desc=None, packed_elems=None, shift_floats=4, pad_floats=8):
    """``fd_points_export`` itself, the output ``shift_floats`` floats into a larger sentinel-filled buffer -> (buffer, starts)."""
    from fusiondepth_amd import _lib
    from fusiondepth_amd import detection as D
    if desc is None:
        desc, _ = D.pack_export_sizes([tuple(m.shape) for m in maps_d])
    depth = torch.cat([m.reshape(-1) for m in maps_d])
    total = int(depth.numel()) if packed_elems is None else packed_elems
    n = len(desc)
    table = torch.from_numpy(np.concatenate([desc.view(np.uint8).reshape(-1),
                                             np.stack([D.points_calib_row(*c) for c in calibs]).view(np.uint8).reshape(-1)])).cuda()
    max_H, max_W = int(desc["H"].max()), int(desc["W"].max())
    ws = torch.empty((_lib.query("fd_points_export_ws_bytes", n, max_H),), device="cuda", dtype=torch.uint8)
    buf = torch.full((4 * total + shift_floats + pad_floats,), -7.0, device="cuda", dtype=torch.float32)
    starts = torch.full((n + 1,), -1, device="cuda", dtype=torch.int64)
    _lib.call("fd_points_export", depth.data_ptr(), table.data_ptr(), table.data_ptr() + desc.nbytes, n, total, max_H, max_W, float(max_high),
              ws.data_ptr(), buf.data_ptr() + 4 * shift_floats, starts.data_ptr(), _lib.stream())
    return buf.cpu().numpy(), starts.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- 1: the edges
def test_edges_equal_the_restatement(edges):
    """Seven maps in ONE call, the output 16 bytes into a larger buffer: every byte of the points, every entry of ``starts``, nothing
    written outside; the same call twice gives the same bits.
    Both branches of the predicate run: the restatement keeps between 10 % and 90 % of every ordinary map - except the 1 x 1 map,
    whose share can only be 0 or 1 (here 0: at f = 0.58 px its only pixel looks 40 degrees up, far above 0.5 m).  No kept point holds
    a NaN (an infinite depth could give one, and the sign of a NaN that inf - inf produces is the platform's, not the rule's)."""
    maps, calibs, want, starts, maps_d = edges
    for i, (m, w) in enumerate(zip(maps, want)):
        share = len(w) / float(m.size)
        print("map %d %s: %d of %d pixels kept (%.2f)" % (i, m.shape, len(w), m.size, share))
        assert not np.isnan(w).any()
        if i == ALL_NAN:
            assert len(w) == 0 and starts[i + 1] == starts[i]
        elif m.size == 1:
            assert len(w) == 0
        else:
            assert 0.10 <= share <= 0.90, (i, m.shape, share)
    flat = np.concatenate(want).reshape(-1)
    for special in (np.inf, 0.0):                                # an infinite and a zero depth each survive somewhere or are filtered: both happen
        assert any((m == special).any() for m in maps)
    buf, got_starts = _raw_call(maps_d, calibs, EDGE_MAX_HIGH)
    assert got_starts.dtype == np.int64 and np.array_equal(got_starts, starts), (got_starts, starts)
    assert np.array_equal(buf[4:4 + flat.size].view(np.uint32), flat.view(np.uint32))
    assert (buf[:4] == -7.0).all() and (buf[4 + flat.size:] == -7.0).all()
    again, again_starts = _raw_call(maps_d, calibs, EDGE_MAX_HIGH)
    assert np.array_equal(again.view(np.uint32), buf.view(np.uint32)) and np.array_equal(again_starts, got_starts)


def test_points_export_chunks_and_the_default_height(edges):
    """The Python layer: all maps in one chunk, then ``chunk=2`` over 5 maps (2 + 2 + 1: the first chunk ends with the all-NaN map), a map
    alone, and ``max_high`` at its default of 1 m."""
    from fusiondepth_amd import detection as D
    maps, calibs, want, starts, maps_d = edges
    got = D.points_export(maps_d, calibs, EDGE_MAX_HIGH)
    assert len(got) == len(want) and all(_same_bytes(g, w) for g, w in zip(got, want))
    assert all(g.shape == (len(w), 4) and (g[:, 3] == 1.0).all() for g, w in zip(got, want))
    five = D.points_export(maps_d[2:7], calibs[2:7], EDGE_MAX_HIGH, chunk=2)
    assert len(five) == 5 and all(_same_bytes(g, w) for g, w in zip(five, want[2:7]))
    alone, = D.points_export(maps_d[6:], calibs[6:], EDGE_MAX_HIGH, chunk=1)
    assert _same_bytes(alone, want[6])
    default = D.points_export(maps_d, calibs)
    want1, _ = PR.clouds(maps, calibs, 1.0)
    assert all(_same_bytes(g, w) for g, w in zip(default, want1)) and sum(map(len, want1)) > sum(map(len, want))
    # the packed form depth_export hands over: one tensor, its descriptors
    desc, total = D.pack_export_sizes([m.shape for m in maps])
    packed = D.points_export(None, calibs, EDGE_MAX_HIGH, packed=(torch.cat([m.reshape(-1) for m in maps_d]), desc))
    assert all(_same_bytes(g, w) for g, w in zip(packed, want))


def test_hand_made_map_on_the_device():
    """Selection, order and the fourth column on the 2 x 3 map of tests/pseudo_lidar_ref.py, against the values worked out by hand."""
    from fusiondepth_amd import detection as D
    depth, calib, by_hand = PR.hand_made_case()
    dev = torch.from_numpy(depth).cuda()
    cloud, = D.points_export([dev], [calib])
    assert cloud.dtype == F32 and np.array_equal(cloud, by_hand)
    lower, = D.points_export([dev], [calib], max_high=0.5)
    assert np.array_equal(lower, by_hand[1:])
    buf, starts = _raw_call([dev, torch.full((1, 2), float("nan"), device="cuda"), dev], [calib] * 3, 1.0)
    assert starts.tolist() == [0, 3, 3, 6] and np.array_equal(buf[4:28].reshape(6, 4), np.concatenate([by_hand, by_hand]))


def test_many_maps_in_one_call(tmp_path):
    """2100 small maps in ONE call - more scan workgroups (one per map and one for the total) than a device holds at once, so the
    later ones start after the earlier ones have finished: every start is the sum of the COUNTS of the maps before it, whichever
    order the workgroups ran in.  Mostly 1 x 70, every seventh 3 x 70 (row starts that are not 0), every eleventh all NaN."""
    from fusiondepth_amd import detection as D
    d = str(tmp_path / "2011_09_26")
    kitti_tree.write_calib(d, 375, 1242)
    n = 2100
    sizes = [(3, 70) if i % 7 == 3 else (1, 70) for i in range(n)]
    maps, calibs = edge_case(d, sizes=sizes, all_nan=-1, seed=23)
    for i in range(0, n, 11):
        maps[i][:] = np.nan
    want, starts = PR.clouds(maps, calibs, EDGE_MAX_HIGH)
    assert 0.2 * sum(m.size for m in maps) < starts[-1] < 0.8 * sum(m.size for m in maps)
    maps_d = [torch.from_numpy(m).cuda() for m in maps]
    flat = np.concatenate(want).reshape(-1)
    for _ in range(2):
        buf, got_starts = _raw_call(maps_d, calibs, EDGE_MAX_HIGH)
        assert np.array_equal(got_starts, starts), np.flatnonzero(got_starts != starts)[:5]
        assert np.array_equal(buf[4:4 + flat.size].view(np.uint32), flat.view(np.uint32)) and (buf[4 + flat.size:] == -7.0).all()
    got = D.points_export(maps_d, calibs, EDGE_MAX_HIGH, chunk=4096)
    assert len(got) == n and all(_same_bytes(g, w) for g, w in zip(got, want))


# ---------------------------------------------------------------------------------------------------------------- 2: bad arguments
def test_bad_arguments_return_the_library_error(edges):
    from fusiondepth_amd import _lib
    from fusiondepth_amd import detection as D
    maps, calibs, want, starts, maps_d = edges
    desc, total = D.pack_export_sizes([m.shape for m in maps])
    depth = torch.cat([m.reshape(-1) for m in maps_d])
    table = torch.from_numpy(np.concatenate([desc.view(np.uint8).reshape(-1),
                                             np.stack([D.points_calib_row(*c) for c in calibs]).view(np.uint8).reshape(-1)])).cuda()
    n, max_H, max_W = len(desc), int(desc["H"].max()), int(desc["W"].max())
    ws = torch.empty((_lib.query("fd_points_export_ws_bytes", n, max_H),), device="cuda", dtype=torch.uint8)
    out = torch.full((4 * total + 4,), -7.0, device="cuda", dtype=torch.float32)
    st = torch.full((n + 1,), -1, device="cuda", dtype=torch.int64)

    def call(points, count=n, starts_ptr=st.data_ptr()):
        _lib.call("fd_points_export", depth.data_ptr(), table.data_ptr(), table.data_ptr() + desc.nbytes, count, total, max_H, max_W,
                  EDGE_MAX_HIGH, ws.data_ptr(), points, starts_ptr, _lib.stream())
    with pytest.raises(RuntimeError, match="fd_points_export"):
        call(None)                                               # a null output
    with pytest.raises(RuntimeError, match="fd_points_export"):
        call(out.data_ptr(), starts_ptr=None)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        call(out.data_ptr() + 4)                                 # misaligned points
    with pytest.raises(RuntimeError, match="1 .. 65535"):
        call(out.data_ptr(), count=0)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (st.cpu().numpy() == -1).all()       # nothing ran
    # a descriptor that runs past packed_elems: that map is skipped, the others are what they were
    bad = desc.copy()
    bad["offset"][4] = total - 7
    buf, got_starts = _raw_call(maps_d, calibs, EDGE_MAX_HIGH, desc=bad)
    kept = [w for i, w in enumerate(want) if i != 4]
    flat = np.concatenate(kept).reshape(-1)
    lens = [0 if i == 4 else len(w) for i, w in enumerate(want)]
    assert np.array_equal(got_starts, np.concatenate([[0], np.cumsum(lens)]))
    assert np.array_equal(buf[4:4 + flat.size].view(np.uint32), flat.view(np.uint32)) and (buf[4 + flat.size:] == -7.0).all()


# ---------------------------------------------------------------------------------------------------------------- 3: the script
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    raw_root, obj_root = str(tmp_path_factory.mktemp("pl_raw")), str(tmp_path_factory.mktemp("pl_object"))
    raw_lines, obj_lines, dates = detection_tree.make_trees(raw_root, obj_root)
    return obj_root, obj_lines, dates


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """A ``Trainer.save_model`` folder from a seeded random ResNet-18, as tests/test_gpu_detection.py saves its own."""
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.trainer import Trainer
    tmp = tmp_path_factory.mktemp("pl_models")
    torch.manual_seed(5)
    net = Trainer(MonodepthOptions().parse(["--num_layers", "18", "--weights_init", "scratch", "--batch_size", "2", "--height", "192",
                                            "--width", "640", "--log_dir", str(tmp / "stage1")]), verbose=False)
    folder = net.save_model("init")
    del net
    return folder


def _script_opt(root, folder, *extra):
    from fusiondepth_amd.options import MonodepthOptions
    return MonodepthOptions().parse(["--num_layers", "18", "--data_path", root, "--png", "--load_weights_folder", folder, "--eval_mono",
                                     "--eval_batch_size", "3", "--save_pred_disps"] + list(extra))


def _splits(tmp_path_factory, obj_root, lines, beams=False):
    from fusiondepth_amd import detection as D
    splits = str(tmp_path_factory.mktemp("pl_splits"))
    os.makedirs(os.path.join(splits, "detection"))
    with open(os.path.join(splits, "detection", "test.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    gts = D.export_gt_depths_detec(obj_root, lines, "detec", os.path.join(splits, "detection", D.detec_output_name("detec")))
    if beams:
        D.export_gt_depths_detec(obj_root, lines, "detec4beam", os.path.join(splits, "detection", D.detec_output_name("detec4beam")))
    return splits, gts


def _date_calib(obj_root, date):
    from fusiondepth_amd import kitti_utils as KU
    return (KU.Calibration(os.path.join(obj_root, date, "calib_cam_to_cam.txt")),) + KU.rect_to_velo(os.path.join(obj_root, date))


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _cloud(path):
    raw = np.fromfile(path, dtype=F32)
    assert raw.size % 4 == 0
    return raw.reshape(-1, 4)


def test_script_writes_the_clouds_of_the_exported_maps(model, trees, tmp_path_factory, capsys):
    """``--pl_name``: each .bin is the restatement on the downloaded ``want_depth`` map with the line's date calibration, byte for byte;
    the PNGs and the metrics are those of a run without the flag, bit for bit; the command line and ``--ext_disp_to_eval`` (dates
    from the image sizes) give the same clouds."""
    from fusiondepth_amd import detection as D
    from fusiondepth_amd import export_detection as X
    obj_root, obj_lines, dates = trees
    order = [3, 0, 2]                                            # two dates, not in frame order
    lines = [obj_lines[k] for k in order]
    splits, gts = _splits(tmp_path_factory, obj_root, lines)
    sizes = [g.shape for g in gts]
    plain = X.evaluate(_script_opt(obj_root, model, "--det_name", "plain"), splits)
    printed_plain = capsys.readouterr().out
    assert len(plain) == 4 and "pseudo-LiDAR" not in printed_plain
    with_pl = X.evaluate(_script_opt(obj_root, model, "--det_name", "with_pl"), splits, pl_name="pl")
    printed = capsys.readouterr().out
    assert len(with_pl) == 5 and "-> Saved 3 pseudo-LiDAR clouds to <data_path>/<folder>/pl" in printed
    assert printed.replace("-> Saved 3 pseudo-LiDAR clouds to <data_path>/<folder>/pl\n", "").replace("with_pl", "plain") == printed_plain
    mean, ratios, per, paths, pl_paths = with_pl
    assert np.array_equal(mean.view(np.uint64), plain[0].view(np.uint64)) and np.array_equal(ratios.view(np.uint32), plain[1].view(np.uint32))
    assert np.array_equal(per.view(np.uint64), plain[2].view(np.uint64))
    assert pl_paths == [os.path.join(obj_root, "training", "pl", "%06d.bin" % k) for k in order]
    assert sorted(os.listdir(os.path.join(obj_root, "training", "pl"))) == ["%06d.bin" % k for k in sorted(order)]
    for a, b in zip(plain[3], paths):
        assert a != b and _read(a) == _read(b), (a, b)
    disps = np.load(os.path.join(model, "disps_eigen_split.npy"))
    _, depths = D.depth_export(disps, sizes, ratios=ratios, want_depth=True)
    want = []
    for k, depth, path in zip(order, depths, pl_paths):
        w, keep = PR.points(depth.cpu().numpy(), _date_calib(obj_root, dates[k]))
        assert 1000 < len(w) < keep.size, (k, keep.mean())      # a real cloud; both sides of the predicate occur
        assert _same_bytes(_cloud(path), w), path
        want.append(w)
    lower = X.evaluate(_script_opt(obj_root, model, "--det_name", "with_pl"), splits, pl_name="pl_low", pl_max_high=-0.5)
    capsys.readouterr()
    for k, depth, path, w in zip(order, depths, lower[4], want):
        wl, _ = PR.points(depth.cpu().numpy(), _date_calib(obj_root, dates[k]), -0.5)
        assert _same_bytes(_cloud(path), wl) and 0 < len(wl) < len(w), path
    # the command line; the loader does not run, so the dates come from the sizes of the images
    saved = os.path.join(model, "disps_eigen_split.npy")
    st = X.main(["--splits_dir", splits, "--pl_name", "pl_stereo", "--eval_stereo", "--ext_disp_to_eval", saved, "--data_path", obj_root,
                 "--det_name", "stereo"])
    assert len(st) == 5 and st[1].size == 0
    _, depths = D.depth_export(disps, sizes, pred_depth_scale_factor=5.4, want_depth=True)
    for k, depth, path in zip(order, depths, st[4]):
        assert _same_bytes(_cloud(path), PR.points(depth.cpu().numpy(), _date_calib(obj_root, dates[k]))[0]), path


def test_script_with_gdc_writes_the_cloud_of_the_corrected_map(model, trees, tmp_path_factory):
    """Batch-1 ``--eval_gdc`` with ``--pl_name``: the cloud of the corrected map, rounded to float32 once; the PNG is what it was."""
    from fusiondepth_amd import detection as D
    from fusiondepth_amd import evaluate_depth as ED
    from fusiondepth_amd import export_detection as X
    from fusiondepth_amd import functional as FD
    from fusiondepth_amd import kitti_utils as KU
    from fusiondepth_amd.gdc import GDC
    obj_root, obj_lines, dates = trees
    lines = [obj_lines[2]]
    splits, gts = _splits(tmp_path_factory, obj_root, lines, beams=True)
    plain = X.evaluate(_script_opt(obj_root, model, "--det_name", "gdc_plain", "--eval_gdc"), splits)
    mean, ratios, per, paths, pl_paths = X.evaluate(_script_opt(obj_root, model, "--det_name", "gdc_pl", "--eval_gdc"), splits, pl_name="pl_gdc")
    assert per is None and pl_paths == [os.path.join(obj_root, "training", "pl_gdc", "000002.bin")]
    assert np.array_equal(mean.view(np.uint64), plain[0].view(np.uint64)) and np.array_equal(ratios, plain[1])
    assert _read(paths[0]) == _read(plain[3][0])
    disp = torch.from_numpy(np.load(os.path.join(model, "disps_eigen_split.npy"))).cuda()
    gh, gw = gts[0].shape
    pred = 1.0 / FD.resize_linear_cv(disp[:1, None], (gh, gw))[0, 0]
    pred = pred * 1.0 * torch.tensor(ratios[0], dtype=torch.float32, device="cuda")
    beam = np.load(os.path.join(splits, "detection", "4beam.npz"), allow_pickle=True)["data"][0]
    gtd = torch.as_tensor(beam, dtype=torch.float64).cuda().clone()
    gtd[gtd == 0] = -1
    calib = KU.Calibration(os.path.join(obj_root, dates[2], "calib_cam_to_cam.txt"))
    corrected = GDC(pred, gtd, calib, W_tol=3e-5, recon_tol=5e-4, k=10, method="cg", consider_range=ED.gdc_range(-1, 4), idx=0)
    assert not torch.equal(corrected, pred)
    want, keep = PR.points(corrected.to(torch.float32).cpu().numpy(), _date_calib(obj_root, dates[2]))
    assert len(want) > 1000 and _same_bytes(_cloud(pl_paths[0]), want)
    assert not _same_bytes(want, PR.points(pred.cpu().numpy(), _date_calib(obj_root, dates[2]))[0])          # GDC moved the points
