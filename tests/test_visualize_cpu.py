"""``evaluate_depth --visualize`` without a GPU: the numpy restatement (tests/visualize_ref.py) against numpy's ``np.percentile`` and
matplotlib's ``Normalize`` / ``magma`` themselves, the committed tables, and the command line (``--vis_dir`` is taken off before the
options are parsed; ``--visualize`` is refused without it and covered with it, before anything touches the GPU)."""
import numpy as np
import pytest

import visualize_ref as VR

F32 = np.float32


def _maps():
    """Uniform random positive depth maps at the sizes of the GPU test, and its three special maps."""
    rng = np.random.RandomState(3)
    out = [("%dx%d" % s, rng.uniform(1.0, 80.0, s).astype(F32)) for s in VR.SIZES + [VR.BIG]]
    out.append(("constant", np.full((9, 14), 7.25, F32)))
    out.append(("16 levels", (F32(2.0) + rng.randint(0, 16, (24, 40)).astype(F32) * F32(1.5)).astype(F32)))
    top = rng.uniform(2.0, 80.0, (24, 40)).astype(F32)
    top.reshape(-1)[rng.choice(top.size, 100, replace=False)] = F32(1.5)       # more than 5 % share the largest d'
    out.append(("top == vmax", top))
    return out


def test_virtual_index_is_float32():
    """(n - 1) * 0.95 in float32: 465 749 * 0.95 = 442 461.55 has no float32 neighbour closer than 442 461.53125."""
    assert VR.virtual_index(375 * 1242) == (442461, 0.53125)
    assert VR.virtual_index(1) == (0, 0.0)
    k, g = VR.virtual_index(2)
    assert k == 0 and g == float(F32(0.95)) and g >= 0.5
    assert VR.virtual_index(6) == (4, 0.75)
    assert VR.virtual_index(21) == (19, 0.0) and VR.virtual_index(41) == (38, 0.0)


@pytest.mark.parametrize("name,depth", _maps(), ids=[n for n, _ in _maps()])
def test_percentile_equals_numpy(name, depth):
    d = F32(1.0) / depth
    want = np.percentile(d, 95)
    got = VR.percentile95(d)
    assert want.dtype == F32 and got.dtype == F32 and got.tobytes() == want.tobytes(), (name, got, want)


@pytest.mark.parametrize("name,depth", _maps(), ids=[n for n, _ in _maps()])
def test_colour_equals_matplotlib(name, depth):
    mpl = pytest.importorskip("matplotlib")
    from matplotlib import cm
    from fusiondepth_amd.visualize import magma_lut
    disp = 1 / depth                                              # evaluate_depth.py:437-441
    vmax = np.percentile(disp, 95)
    normalizer = mpl.colors.Normalize(vmin=disp.min(), vmax=vmax)
    mapper = cm.ScalarMappable(norm=normalizer, cmap="magma")
    want = (mapper.to_rgba(disp)[:, :, :3] * 255).astype(np.uint8)
    got, (vmin, vmax_r) = VR.colorize(depth, magma_lut())
    assert vmin == disp.min() and vmax_r.tobytes() == vmax.tobytes()
    xn = np.asarray(normalizer(disp))                             # the normalised values themselves, bit for bit
    assert xn.dtype == F32 and xn.tobytes() == VR.normalize(disp, vmin, vmax_r).tobytes(), name
    assert got.shape == want.shape and np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
    if name == "top == vmax":
        assert (got == magma_lut()[255]).all(axis=2).sum() >= 100  # xa == 256 -> the last entry
    if name == "constant":
        assert (got == magma_lut()[0]).all()


def test_block_reduce_pads_with_zeros():
    img = np.arange(1, 3 * 5 * 3 + 1, dtype=np.uint8).reshape(3, 5, 3)
    got = VR.block_reduce_max(img)
    assert got.shape == (2, 3, 3)
    assert np.array_equal(got[0, 0], img[:2, :2].max(axis=(0, 1))) and np.array_equal(got[1, 2], img[2, 4])


def test_magma_table_is_matplotlibs():
    mpl = pytest.importorskip("matplotlib")
    from fusiondepth_amd.visualize import magma_lut
    want = (mpl.colormaps["magma"](np.arange(256))[:, :3] * 255).astype(np.uint8)
    got = magma_lut()
    assert got.dtype == np.uint8 and got.shape == (256, 3) and np.array_equal(got, want)


def test_hue_table_is_the_analytic_ramp():
    import colorsys
    from fusiondepth_amd.visualize import hue_lut
    got = hue_lut()
    assert got.dtype == np.uint8 and got.shape == (256, 3)
    assert got[0].tolist() == [255, 0, 0] and got[64].tolist() == [128, 255, 0] and got[128].tolist() == [0, 255, 255]
    for k in (1, 17, 80, 200, 255):
        assert got[k].tolist() == [int(round(255 * c)) for c in colorsys.hsv_to_rgb(k / 256.0, 1.0, 1.0)]


def test_vis_dir_is_taken_off_the_command_line():
    from fusiondepth_amd import evaluate_depth as ED
    found, rest = ED.split_off_flags(["--eval_mono", "--vis_dir", "out/vis", "--visualize", "--splits_dir=s"], ED.SCRIPT_FLAGS)
    assert found["vis_dir"] == "out/vis" and found["splits_dir"] == "s" and found["semantic_dir"] is None
    assert rest == ["--eval_mono", "--visualize"]
    found, _ = ED.split_off_flags(["--eval_mono"], ED.SCRIPT_FLAGS)
    assert found["vis_dir"] is None


def test_visualize_is_refused_without_a_folder_and_covered_with_one(tmp_path):
    from fusiondepth_amd import evaluate_depth as ED
    from fusiondepth_amd.options import MonodepthOptions
    opt = MonodepthOptions().parse(["--eval_mono", "--visualize", "--ext_disp_to_eval", "none.npy"])
    with pytest.raises(NotImplementedError, match="visualize"):
        ED._refuse_uncovered(opt)
    with pytest.raises(NotImplementedError, match="visualize"):
        ED.evaluate(opt, str(tmp_path))
    with pytest.raises(NotImplementedError, match="visualize"):
        ED.main(["--splits_dir", str(tmp_path), "--eval_mono", "--visualize", "--ext_disp_to_eval", "none.npy"])
    ED._refuse_uncovered(opt, vis_dir=str(tmp_path / "vis"))      # covered: no refusal
    # with the folder the script gets as far as the file it was told to load
    with pytest.raises(FileNotFoundError, match="none.npy"):
        ED.main(["--splits_dir", str(tmp_path), "--vis_dir", str(tmp_path / "vis"), "--eval_mono", "--visualize", "--ext_disp_to_eval", "none.npy"])
    # --demo stays refused, with or without the folder
    demo = MonodepthOptions().parse(["--eval_mono", "--visualize", "--demo", "--ext_disp_to_eval", "none.npy"])
    with pytest.raises(NotImplementedError, match="demo"):
        ED._refuse_uncovered(demo, vis_dir=str(tmp_path / "vis"))
