"""The LiDAR sparsifier without a GPU: the numpy restatement (tests/sparsify_ref.py) against what the reference itself returned
(tests/golden/sparsify_*.npz, written by tests/golden/make_sparsify.py), the near-edge share of every fixture, the command line's
flag surface and folder names, and the default row lists against the reference's prepare scripts."""
import json
import os

import numpy as np
import pytest

import sparsify_ref as SR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", params=["clean", "full"])
def fixture(request):
    g = np.load(os.path.join(GOLD, "sparsify_%s.npz" % request.param))
    scan = SR.fixture_scan(request.param, g["removed"])
    assert len(scan) == int(g["n_points"])
    return request.param, g, scan


def test_restatement_cells_equal_the_reference(fixture):
    kind, g, scan = fixture
    kept = np.flatnonzero(SR.filter_mask(scan))
    assert np.array_equal(kept, g["kept"])
    assert 55000 < len(kept) < 70000
    for W in (1024, 512):
        row, col = SR.cells(scan[kept], 64, W)
        assert np.array_equal(row, g["row"]) and np.array_equal(col, g["col_w%d" % W]), (kind, W)


@pytest.mark.parametrize("config", sorted(SR.CONFIGS))
def test_restatement_output_equals_the_reference(fixture, config):
    """Winners, output order and, for the random configurations, the selection under ``np.random.seed``-ed uniforms."""
    kind, g, scan = fixture
    idx = SR.sparsify_indices(scan, **SR.CONFIGS[config])
    want = g["out_" + config]
    assert len(idx) == len(want) and np.array_equal(idx, want), (kind, config, len(idx), len(want))


def test_near_edge_share_stays_within_the_cap(fixture):
    kind, g, scan = fixture
    kept = np.flatnonzero(SR.filter_mask(scan))
    for W in (1024, 512):
        near = SR.near_edge(scan[kept], 64, W)
        share = near.sum() / len(kept)
        print("%s W=%d: %d of %d points near an edge (%.2e)" % (kind, W, near.sum(), len(kept), share))
        assert share <= SR.NEAR_EDGE_CAP, (kind, W, share)
        if W == 1024:
            assert np.array_equal(np.flatnonzero(near), g["near"])
        if kind == "clean":
            assert near.sum() == 0
    if kind == "full":
        assert len(g["near"]) > 0                                # the full fixture does exercise the rule


def test_restatement_equals_the_reference_on_the_hand_made_scans():
    g = np.load(os.path.join(GOLD, "sparsify_edge.npz"))
    for sname, scan in SR.edge_scans().items():
        kept = np.flatnonzero(SR.filter_mask(scan))
        if len(kept):
            row, col = SR.cells(scan[kept], 64, 1024)
            assert np.array_equal(row, g[sname + "__row"]) and np.array_equal(col, g[sname + "__col"]), sname
        for cname, cfg in SR.EDGE_CONFIGS.items():
            got = scan[SR.sparsify_indices(scan, **cfg)]
            want = g["%s__%s" % (sname, cname)]
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), (sname, cname)
    assert len(g["empty__all"]) == 0 and len(g["outside__all"]) == 0 and len(g["one__all"]) == 1
    # the all-zero point wins its cell (the last of three) and random sampling drops it: its float64 norm is 0
    zero = SR.edge_scans()["zero"]
    assert g["zero__all"].tobytes() == zero[[4, 1, 3]].tobytes() and g["zero__random1"].tobytes() == zero[[1, 3]].tobytes()
    # clamped angles land in the first / last row and column
    assert g["clamped__row"].min() == 0 and g["clamped__row"].max() == 63 and g["clamped__col"].min() == 0 and g["clamped__col"].max() == 1023


def test_default_row_lists_match_the_prepare_scripts():
    from fusiondepth_amd import functional as FD
    from fusiondepth_amd import sparsify as SP
    settings = json.load(open(os.path.join(GOLD, "sparsify_line_specs.json")))
    seen = set()
    for script, st in settings.items():
        if "line_spec" not in st:
            assert st["random_sample"] in (100, 200) and st["W"] == 1024 and st["H"] == 64
            continue
        nbeams = st.get("nbeams", SP.build_parser().get_default("nbeams"))
        assert list(FD.SPARSIFY_LINE_SPEC[nbeams]) == st["line_spec"], script
        assert st["W"] == 1024 and st["H"] == 64
        assert "prepare_%dbeam" % nbeams in script
        seen.add(nbeams)
    assert seen == {1, 2, 3, 4} == set(FD.SPARSIFY_LINE_SPEC)
    assert FD.sparsify_rows(64, None, 2) == list(range(0, 64, 2)) and FD.sparsify_rows(64, [2, 7], 1) == [2, 7]
    assert FD.SPARSIFY_BOX == SR.BOX


def test_cli_takes_the_reference_flags_and_names_its_folders():
    from fusiondepth_amd import sparsify as SP
    a = SP.parse_args("--W 1024 --H 64 --line_spec 9 11 --nbeams 2 --split_file ../splits/eigen_zhou/train_files.txt".split())
    assert (a.W, a.H, a.line_spec, a.nbeams, a.slice, a.random_sample) == (1024, 64, [9, 11], 2, 1, 0)
    assert a.ptc_path == a.output_path == "../kitti_data/" and a.threads == 16            # the reference's 20, capped
    assert SP.output_folder(a, "2011_09_26/2011_09_26_drive_0001_sync") == "../kitti_data/2011_09_26/2011_09_26_drive_0001_sync/2beam/"
    assert SP.input_path(a, "2011_09_26/d", 7) == "../kitti_data/2011_09_26/d/velodyne_points/data/0000000007.bin"
    r = SP.parse_args("--W 1024 --H 64 --random_sample 100 --split_file s.txt --ptc_path /in/ --output_path /out/ --threads 4".split())
    assert r.random_sample == 100 and r.threads == 4 and r.line_spec is None
    assert SP.output_folder(r, "d/e") == "/out/d/e/random100/"
    d = SP.parse_args(["--split_file", "s.txt"])
    assert (d.W, d.H, d.nbeams, d.seed) == (512, 64, 4, 0)                               # the reference's defaults
    SP.parse_args("--split_file s.txt --calib_path a --image_path b --D 700".split())    # accepted and ignored, as there
    for flags in ("--fill_in_map_dir m", "--fill_in_spec 1 2", "--fill_in_slice 2", "--store_line_map_dir d", "--visualize"):
        with pytest.raises(NotImplementedError, match=flags.split()[0]):
            SP.parse_args(["--split_file", "s.txt"] + flags.split())
    with pytest.raises(ValueError):
        SP.parse_args([])


def test_scan_keys_depend_on_folder_and_frame_alone(tmp_path):
    from fusiondepth_amd import sparsify as SP
    k = SP.scan_key("2011_09_26/2011_09_26_drive_0001_sync", 5)
    assert k == SP.scan_key("2011_09_26/2011_09_26_drive_0001_sync", 5) and 0 <= k < 2 ** 64
    assert len({SP.scan_key("a/b", i) for i in range(100)} | {SP.scan_key("a/c", i) for i in range(100)}) == 200
    split = tmp_path / "s.txt"
    split.write_text("a/b 3 l\n\n  \na/c 10 r\n")
    assert SP.split_entries(str(split)) == [("a/b", 3), ("a/c", 10)]
