"""CPU checks of the GPU batch builder's arithmetic and host logic (no device needed):

  * tests/augment_ref.py - the numpy restatement the kernels of csrc/augment.hip are compared with on the GPU - equals PIL itself,
    bit for bit (PIL is what torchvision's ``Resize`` / ``ColorJitter`` / ``ToTensor`` call on PIL images);
  * tests/golden/augment_*.npz is what its committed generator produces;
  * the host side of ``fusiondepth_amd.datasets.KITTIRAWBatches``: paths, order, draws, the options it refuses.
"""
import itertools
import os
import types

import numpy as np
import pytest

import augment_ref as R
import make_augment as G

from PIL import Image                      # required: these tests run, they do not skip

FACTORS = (0.8, 0.93, 1.0, 1.07, 1.2)


def _all_colours():
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def test_hue_conversions_equal_pil_on_all_colours():
    allc = _all_colours()
    hsv = np.asarray(Image.fromarray(allc).convert("HSV"))
    rgb = np.asarray(Image.fromarray(allc, "HSV").convert("RGB"))          # every (H, S, V) triple back to RGB
    for i in range(0, 4096, 512):
        assert np.array_equal(R.rgb_to_hsv(allc[i:i + 512]), hsv[i:i + 512])
        assert np.array_equal(R.hsv_to_rgb(allc[i:i + 512]), rgb[i:i + 512])


@pytest.mark.parametrize("h", [-0.1, -0.05, 0.03, 0.1])
def test_hue_shift_equals_pil(h):
    img = G.pil_pyramid(G.frame())[1]
    assert np.array_equal(R.hue(img, h), G.pil_jitter(img, (1, 1, 1, h), [3]))
    assert R.hue_shift(-0.05) == 244


@pytest.mark.parametrize("op", [0, 1, 2])
def test_blends_equal_pil(op):
    img = G.pil_pyramid(G.frame())[1]
    dark = (img // 3).astype(np.uint8)
    for f in FACTORS:
        fac = [1.0, 1.0, 1.0, 0.0]
        fac[op] = f
        for im in (img, dark):
            assert np.array_equal(R.color_jitter(im, fac, [op]), G.pil_jitter(im, fac, [op])), (op, f)


def test_full_jitter_orders_equal_pil():
    img = G.pil_pyramid(G.frame())[2]
    fac = (1.2, 0.8, 1.2, -0.1)
    for order in itertools.permutations(range(4)):
        assert np.array_equal(R.color_jitter(img, fac, order), G.pil_jitter(img, fac, order)), order


@pytest.mark.parametrize("mirror", [False, True])
def test_pyramid_equals_pil(mirror):
    src = G.frame()
    got = R.pyramid(src, 192, 640, 4, mirror)
    want = G.pil_pyramid(src, mirror=mirror)
    assert [g.shape for g in got] == [(192, 640, 3), (96, 320, 3), (48, 160, 3), (24, 80, 3)]
    for s in range(4):
        assert np.array_equal(got[s], want[s]), s


@pytest.mark.parametrize("shape,size", [((370, 1226), (320, 1024)), ((375, 1242), (352, 1216))])
@pytest.mark.parametrize("mirror", [False, True])
def test_resize_equals_pil(shape, size, mirror):
    rng = np.random.default_rng(shape[1])
    img = rng.integers(0, 256, shape + (3,)).astype(np.uint8)
    pil = Image.fromarray(img)
    if mirror:
        pil = pil.transpose(Image.FLIP_LEFT_RIGHT)
    want = np.asarray(pil.resize((size[1], size[0]), Image.LANCZOS))
    assert np.array_equal(R.resize_lanczos(img, size[0], size[1], mirror), want)


def test_library_tables_equal_the_restatement():
    from fusiondepth_amd import functional as FD
    for n_in, n_out in ((1242, 640), (375, 192), (640, 320), (48, 24), (1226, 1024), (370, 320), (1242, 1216), (375, 352), (10, 3), (7, 7)):
        tab, k = FD.lanczos_table(n_in, n_out)
        xmin, count, coef, ksize = R.lanczos_coeffs(n_in, n_out)
        assert count.max() <= k and tab.shape == (n_out, 2 + k)
        assert np.array_equal(tab[:, 0], xmin) and np.array_equal(tab[:, 1], count)
        kk = min(k, ksize)
        assert np.array_equal(tab[:, 2:2 + kk], coef[:, :kk]) and not tab[:, 2 + kk:].any() and not coef[:, kk:].any()


def test_to_planes_is_correctly_rounded():
    v = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)
    want = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    assert np.array_equal(R.to_planes(v)[0, 0], want)


def test_golden_files_are_what_the_generator_makes(golden):
    sets = G.build()
    assert sorted(sets) == ["augment_jitter0", "augment_jitter1", "augment_jitter2", "augment_pyramid"]
    for stem, arrays in sets.items():
        path = os.path.join(os.path.dirname(G.__file__), stem + ".npz")
        assert os.path.getsize(path) <= 1 << 20
        stored = golden(stem)
        assert sorted(stored) == sorted(arrays), stem
        for k, v in arrays.items():
            assert stored[k].dtype == np.asarray(v).dtype and np.array_equal(stored[k], v), (stem, k)
    orders = {tuple(o) for _, o in G.JITTER_SETS}
    hues = [f[3] for f, _ in G.JITTER_SETS]
    assert len(orders) >= 2 and min(hues) < 0 < max(hues)
    # and the restatement reproduces the stored expectations from the seeded frame alone
    src = G.frame(int(golden("augment_pyramid")["seed"]))
    pyr = R.pyramid(src, G.HEIGHT, G.WIDTH, G.NUM_SCALES)
    for s in range(G.NUM_SCALES):
        assert np.array_equal(pyr[s], golden("augment_pyramid")["color_%d" % s])
    assert np.array_equal(R.pyramid(src, G.HEIGHT, G.WIDTH, G.NUM_SCALES, True)[3], golden("augment_pyramid")["mirror_3"])
    for j in range(3):
        g = golden("augment_jitter%d" % j)
        for s in (1, 3):
            assert np.array_equal(R.color_jitter(pyr[s], g["factors"], g["order"]), g["aug_%d" % s])
        assert np.array_equal(R.to_planes(g["aug_3"]), g["aug_planes_3"])


# ---------------------------------------------------------------------------------------------------- KITTIRAWBatches, host side
def _opt(**over):
    o = types.SimpleNamespace(need_4beam=True, need_2_channel=True, need_full_res_4beam=False, need_inf_gdc=False, clone_gdc=False,
                              need_path=False, nbeams=4, random_sample=-1)
    for k, v in over.items():
        setattr(o, k, v)
    return o


def _lines(n=7):
    return ["2011_09_26/2011_09_26_drive_0001_sync %d %s" % (i + 1, "lr"[i % 2]) for i in range(n)]


def _builder(**kw):
    from fusiondepth_amd.datasets import KITTIRAWBatches
    args = dict(is_train=True, img_ext=".png", opt=_opt(), batch_size=2, device="cpu")
    args.update(kw)
    return KITTIRAWBatches("/data/kitti", _lines(), 192, 640, [0, -1, 1], 4, **args)


def test_builder_paths_follow_the_reference_scheme():
    b = _builder()
    folder = "2011_09_26/2011_09_26_drive_0001_sync"
    assert b.get_image_path(folder, 7, "l") == "/data/kitti/%s/image_02/data/0000000007.png" % folder
    assert b.get_image_path(folder, 7, "r") == "/data/kitti/%s/image_03/data/0000000007.png" % folder
    assert b.get_velo_path(folder, 7) == "/data/kitti/%s/velodyne_points/data/0000000007.bin" % folder
    assert b.get_beam_path(folder, 12) == "/data/kitti/%s/4beam/0000000012.bin" % folder
    assert _builder(opt=_opt(nbeams=16)).get_beam_path(folder, 12).endswith("/16beam/0000000012.bin")
    assert _builder(opt=_opt(random_sample=100)).get_beam_path(folder, 12).endswith("/random100/0000000012.bin")
    assert _builder(img_ext=".jpg").get_image_path(folder, 0, "2").endswith("image_02/data/0000000000.jpg")
    assert not b.load_depth                                     # no velodyne file for the first line: no depth_gt
    plan = b.plan_batch(0, [2, 3])
    assert [p["frame_index"] for p in plan] == [3, 4] and [p["side"] for p in plan] == ["l", "r"]
    assert plan[0]["images"] == [b.get_image_path(folder, 3 + f, "l") for f in (0, -1, 1)]
    assert plan[0]["beams"] == [b.get_beam_path(folder, 3 + f) for f in (0, -1, 1)]
    assert plan[1]["date"] == "2011_09_26" and plan[1]["velo"] is None
    only_beam = _builder(opt=_opt(need_2_channel=False)).plan_batch(0, [2])[0]
    assert only_beam["beams"] == [b.get_beam_path(folder, 3)]


def test_builder_length_order_and_determinism():
    b = _builder()
    assert len(b) == 3 and b.epoch_order(0) == [0, 1, 2, 3, 4, 5]            # 7 items, batch 2, drop_last
    assert len(_builder(batch_size=7)) == 1 and len(_builder(batch_size=8)) == 0
    s1, s2, s3 = _builder(shuffle=True, seed=5), _builder(shuffle=True, seed=5), _builder(shuffle=True, seed=6)
    assert s1.epoch_order(0) == s2.epoch_order(0) and s1.epoch_order(1) == s2.epoch_order(1)
    assert s1.epoch_order(0) != s1.epoch_order(1) and s1.epoch_order(0) != s3.epoch_order(0)
    assert len(s1.epoch_order(0)) == 6 and len(set(s1.epoch_order(0))) == 6
    draws = [s1.item_draws(0, i) for i in range(7)]
    assert draws == [s2.item_draws(0, i) for i in range(7)]
    assert draws != [s3.item_draws(0, i) for i in range(7)] and draws != [s1.item_draws(1, i) for i in range(7)]
    many = [s1.item_draws(e, i) for e in range(40) for i in range(7)]
    assert {d["do_flip"] for d in many} == {True, False} and {d["do_color_aug"] for d in many} == {True, False}
    for d in many:
        assert (d["jitter"] is not None) == d["do_color_aug"]
        if d["jitter"] is not None:
            (bb, c, s, h), order = d["jitter"]
            assert 0.8 <= bb <= 1.2 and 0.8 <= c <= 1.2 and 0.8 <= s <= 1.2 and -0.1 <= h <= 0.1 and sorted(order) == [0, 1, 2, 3]
    assert len({tuple(d["jitter"][1]) for d in many if d["jitter"]}) > 4
    # evaluation: no augmentation at all
    ev = _builder(is_train=False)
    assert all(ev.item_draws(0, i) == {"do_color_aug": False, "do_flip": False, "jitter": None} for i in range(7))
    per = _builder(jitter_per_image=True, seed=2)
    d = next(x for x in (per.item_draws(0, i) for i in range(7)) if x["do_color_aug"])
    assert len(d["jitter"]) == 3 and all(len(f) == 4 for f in d["jitter"]) and d["jitter"][0][0] != d["jitter"][0][1]


def test_builder_draw_injection():
    fixed = {"do_color_aug": True, "do_flip": True, "jitter": ((1.1, 0.9, 1.0, 0.05), [3, 0, 1, 2])}
    seen = []

    def draws(epoch, index):
        seen.append((epoch, index))
        return fixed if index % 2 else {"do_color_aug": False, "do_flip": False, "jitter": None}

    b = _builder(draws=draws)
    plan = b.plan_batch(4, [0, 1])
    assert seen == [(4, 0), (4, 1)]
    assert plan[0]["jitter"] is None and not plan[0]["do_flip"]
    assert plan[1]["jitter"] == fixed["jitter"] and plan[1]["do_flip"]


def test_builder_refuses_what_it_does_not_cover():
    from fusiondepth_amd.datasets import KITTIRAWBatches
    with pytest.raises(NotImplementedError, match="stereo"):
        KITTIRAWBatches("/d", _lines(), 192, 640, [0, "s"], 4, opt=_opt())
    with pytest.raises(NotImplementedError, match="need_full_res_4beam"):
        _builder(opt=_opt(need_full_res_4beam=True))
    with pytest.raises(NotImplementedError, match="need_inf_gdc"):
        _builder(opt=_opt(need_inf_gdc=True))
    with pytest.raises(NotImplementedError, match="clone_gdc"):
        _builder(opt=_opt(clone_gdc=True))
    with pytest.raises(ValueError):
        _builder(batch_size=0)


def test_two_channel_keys_do_not_need_need_4beam():
    folder = "2011_09_26/2011_09_26_drive_0001_sync"
    b = _builder(opt=_opt(need_4beam=False))
    assert b.plan_batch(0, [2])[0]["beams"] == [b.get_beam_path(folder, 3 + f) for f in (0, -1, 1)]
    assert _builder(opt=_opt(need_4beam=False, need_2_channel=False)).plan_batch(0, [2])[0]["beams"] == []
    from fusiondepth_amd.datasets import KITTIRAWBatches
    with pytest.raises(ValueError, match="contain 0"):
        KITTIRAWBatches("/d", _lines(), 192, 640, [-1, 1], 4, opt=_opt())


def test_resample_clip_is_not_fused_into_the_packed_shift():
    """csrc/augment.hip clip8: hipcc's fusion of shift + clamp into v_ashr_pk_u8_i32 gave wrong bytes on the MI355X; an empty asm
    keeps the two apart.  If a later compiler fuses them again, this notices on the build machine."""
    import subprocess
    from fusiondepth_amd import build
    src = os.path.join(build.CSRC, "augment.hip")
    cmd = [build.HIPCC] + build.FLAGS + build._file_flags(src) + ["--cuda-device-only", "-S", "-o", "-", src]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "k_lanczos_v" in r.stdout and "v_med3_i32" in r.stdout
    assert "v_ashr_pk_u8_i32" not in r.stdout


def test_package_loads_without_pil():
    import subprocess
    import sys
    code = ("import sys; import fusiondepth_amd, fusiondepth_amd.datasets, fusiondepth_amd.functional; "
            "assert not any(m == 'PIL' or m.startswith('PIL.') for m in sys.modules), 'PIL imported eagerly'")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)
