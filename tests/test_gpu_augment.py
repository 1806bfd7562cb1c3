"""csrc/augment.hip against tests/augment_ref.py (which tests/test_augment_cpu.py pins to PIL): Lanczos resample, colour jitter
and ToTensor on uint8 images, bit for bit - no tolerance, no excluded pixels."""
import itertools

import numpy as np
import pytest
import torch

import augment_ref as R
import make_augment as G

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def ref_resize_batch(imgs, out_h, out_w, mirrors):
    """R.resize_lanczos for a batch [N,H,W,3], vectorised over the batch (same arithmetic: one pass per axis)."""
    imgs = np.stack([im[:, ::-1] if m else im for im, m in zip(imgs, mirrors)])
    N, H, W, _ = imgs.shape
    tmp = R._resample_axis1(imgs.reshape(N * H, W, 3), out_w).reshape(N, H, out_w, 3)
    cols = tmp.transpose(1, 0, 2, 3).reshape(H, N * out_w, 3).transpose(1, 0, 2)            # [N*out_w, H, 3]
    out = R._resample_axis1(np.ascontiguousarray(cols), out_h)                              # [N*out_w, out_h, 3]
    return np.ascontiguousarray(out.reshape(N, out_w, out_h, 3).transpose(0, 2, 1, 3))


def test_pyramid_of_the_golden_frame(golden):
    from fusiondepth_amd import functional as FD
    g = golden("augment_pyramid")
    src = G.frame(int(g["seed"]))
    cur = dev(src[None])
    for s in range(G.NUM_SCALES):
        cur = FD.resize_lanczos_u8(cur, (G.HEIGHT >> s, G.WIDTH >> s))
        assert np.array_equal(host(cur)[0], g["color_%d" % s]), "scale %d" % s
    cur = dev(src[None])
    for s in range(G.NUM_SCALES):
        cur = FD.resize_lanczos_u8(cur, (G.HEIGHT >> s, G.WIDTH >> s), mirror=(s == 0))
    assert np.array_equal(host(cur)[0], g["mirror_3"])


@pytest.mark.parametrize("shape,size", [((375, 1242), (192, 640)), ((370, 1226), (320, 1024)), ((375, 1242), (352, 1216))])
@pytest.mark.parametrize("N", [1, 36])
def test_resize_random_images(shape, size, N):
    """The three shapes of the issue at batch 1 and 36 (12 items x 3 frames), every other frame mirrored; the second level of
    the pyramid is chained from the first."""
    from fusiondepth_amd import functional as FD
    rng = np.random.default_rng(1000 + N + size[1])
    imgs = rng.integers(0, 256, (N,) + shape + (3,)).astype(np.uint8)
    if N > 1:
        imgs[1] = 0
        imgs[2] = 255
        imgs[3, :, ::2] = 0
        imgs[3, :, 1::2] = 255                                    # overshoot on both sides: exercises the clip
    mirrors = [bool(i % 2) for i in range(N)] if N > 1 else [True]
    got = FD.resize_lanczos_u8(dev(imgs), size, mirror=mirrors)
    want = ref_resize_batch(imgs, size[0], size[1], mirrors)
    g = host(got)
    assert g.shape == want.shape and np.array_equal(g, want), "%d bytes differ" % (g != want).sum()
    half = (size[0] // 2, size[1] // 2)
    got2 = host(FD.resize_lanczos_u8(got, half))
    assert np.array_equal(got2, ref_resize_batch(want, half[0], half[1], [False] * N))
    again = host(FD.resize_lanczos_u8(dev(imgs), size, mirror=mirrors))
    assert np.array_equal(again, g)                               # deterministic


def test_resize_odd_widths_take_the_unaligned_path():
    """A row pitch that is not a multiple of 16 bytes (output and input), upscaling included."""
    from fusiondepth_amd import functional as FD
    rng = np.random.default_rng(5)
    for shape, size in (((37, 53), (19, 27)), ((19, 27), (40, 61)), ((64, 96), (64, 50)), ((30, 40), (13, 40))):
        imgs = rng.integers(0, 256, (3,) + shape + (3,)).astype(np.uint8)
        mirrors = [False, True, False]
        got = host(FD.resize_lanczos_u8(dev(imgs), size, mirror=mirrors))
        assert np.array_equal(got, ref_resize_batch(imgs, size[0], size[1], mirrors)), (shape, size)


def test_jitter_of_the_golden_pyramid(golden):
    from fusiondepth_amd import functional as FD
    pyr = golden("augment_pyramid")
    for j in range(3):
        g = golden("augment_jitter%d" % j)
        params = (tuple(g["factors"]), list(g["order"]))
        for s in range(G.NUM_SCALES):
            got = host(FD.color_jitter_u8(dev(pyr["color_%d" % s][None]), [params]))[0]
            assert np.array_equal(got, g["aug_%d" % s]), (j, s, int((got != g["aug_%d" % s]).sum()))
        for s in G.PLANE_SCALES:
            got = host(FD.color_jitter_u8(dev(pyr["color_%d" % s][None]), [params], planes=True))[0]
            assert np.array_equal(got, g["aug_planes_%d" % s]), (j, s)


def test_every_order_and_the_range_ends():
    """All 24 orders of the four operations, each with factors at the ends of the reference's ranges, in one launch sequence."""
    from fusiondepth_amd import functional as FD
    rng = np.random.default_rng(24)
    orders = list(itertools.permutations(range(4)))
    ends = list(itertools.product((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1)))
    imgs = rng.integers(0, 256, (len(orders), 40, 56, 3)).astype(np.uint8)
    imgs[5] //= 4                                                  # a dark image
    imgs[6] = 255 - imgs[6] // 4                                   # a bright one
    params = [(ends[i % len(ends)], list(o)) for i, o in enumerate(orders)]
    got = host(FD.color_jitter_u8(dev(imgs), params))
    for i, (fac, order) in enumerate(params):
        assert np.array_equal(got[i], R.color_jitter(imgs[i], fac, order)), (i, fac, order)
    planes = host(FD.color_jitter_u8(dev(imgs), params, planes=True))
    for i, (fac, order) in enumerate(params):
        assert np.array_equal(planes[i], R.to_planes(R.color_jitter(imgs[i], fac, order))), i


def test_jitter_batch_of_36_with_partial_orders_and_copies(golden):
    from fusiondepth_amd import functional as FD
    rng = np.random.default_rng(36)
    base = golden("augment_pyramid")["color_1"]
    imgs = np.stack([np.roll(base, 7 * i, axis=1) for i in range(36)])
    params = []
    for i in range(36):
        if i % 9 == 0:
            params.append(None)
            continue
        order = [int(o) for o in rng.permutation(4)][:1 + i % 4]
        fac = (float(rng.uniform(0.8, 1.2)), float(rng.uniform(0.8, 1.2)), float(rng.uniform(0.8, 1.2)), float(rng.uniform(-0.1, 0.1)))
        params.append((fac, order))
    got = host(FD.color_jitter_u8(dev(imgs), params))
    for i, p in enumerate(params):
        want = imgs[i] if p is None else R.color_jitter(imgs[i], p[0], p[1])
        assert np.array_equal(got[i], want), (i, p)
    assert np.array_equal(host(FD.color_jitter_u8(dev(imgs), params)), got)      # deterministic


def test_jitter_image_size_that_is_no_multiple_of_16():
    from fusiondepth_amd import functional as FD
    rng = np.random.default_rng(7)
    imgs = rng.integers(0, 256, (3, 13, 11, 3)).astype(np.uint8)
    params = [((1.1, 0.9, 1.15, 0.07), [1, 3, 2, 0]), None, ((0.85, 1.2, 0.8, -0.03), [3, 1, 0, 2])]
    got = host(FD.color_jitter_u8(dev(imgs), params))
    planes = host(FD.color_jitter_u8(dev(imgs), params, planes=True))
    for i, p in enumerate(params):
        want = imgs[i] if p is None else R.color_jitter(imgs[i], p[0], p[1])
        assert np.array_equal(got[i], want) and np.array_equal(planes[i], R.to_planes(want)), i


@pytest.mark.parametrize("h", [0.1, -0.1, -0.05])
def test_hue_on_all_colours(h):
    from fusiondepth_amd import functional as FD
    v = np.arange(1 << 24, dtype=np.uint32)
    allc = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(1, 4096, 4096, 3)
    got = host(FD.color_jitter_u8(dev(allc), [((1.0, 1.0, 1.0, h), [3])]))[0]
    for i in range(0, 4096, 512):
        want = R.hue(allc[0, i:i + 512], h)
        assert np.array_equal(got[i:i + 512], want), "rows %d..: %d bytes differ" % (i, (got[i:i + 512] != want).sum())


def test_hue_offset_comes_from_the_double_factor():
    """h * 255 a hair below an integer in double, on it after rounding h to float32: the offset is the double's truncation."""
    from fusiondepth_amd import functional as FD
    h = float(np.nextafter(10.0 / 255.0, 0.0))
    assert int(h * 255.0) == 9 and int(float(np.float32(h)) * 255.0) == 10 and R.hue_shift(h) == 9
    rng = np.random.default_rng(12)
    img = rng.integers(0, 256, (1, 32, 48, 3)).astype(np.uint8)
    got = host(FD.color_jitter_u8(dev(img), [((1.0, 1.0, 1.0, h), [3])]))[0]
    assert np.array_equal(got, R.hue(img[0], h)) and not np.array_equal(got, R.hue(img[0], 10.0 / 255.0 + 1e-9))


def test_contrast_mean_is_the_exact_integer_mean():
    from fusiondepth_amd import functional as FD
    rng = np.random.default_rng(3)
    imgs = np.stack([np.zeros((192, 640, 3), np.uint8), np.full((192, 640, 3), 255, np.uint8),
                     rng.integers(0, 256, (192, 640, 3)).astype(np.uint8), rng.integers(0, 256, (192, 640, 3)).astype(np.uint8)])
    params = [((1.0, 1.2, 1.0, 0.0), [1])] * 3 + [((0.8, 0.8, 1.0, 0.0), [0, 1])]      # the last: contrast after brightness
    out, means = FD.color_jitter_u8(dev(imgs), params, return_means=True)
    m = host(means)
    want = [R.contrast_mean(imgs[0]), R.contrast_mean(imgs[1]), R.contrast_mean(imgs[2]), R.contrast_mean(R.brightness(imgs[3], 0.8))]
    assert m.tolist() == want and want[0] == 0 and want[1] == 255
    out2, means2 = FD.color_jitter_u8(dev(imgs), params, return_means=True)
    assert np.array_equal(host(means2), m) and np.array_equal(host(out2), host(out))
    _, none = FD.color_jitter_u8(dev(imgs[:1]), [((1.1, 1.0, 1.0, 0.0), [0])], return_means=True)
    assert host(none).tolist() == [-1]


def test_u8_to_planes_on_all_values_and_into_a_batch_slot():
    from fusiondepth_amd import functional as FD
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, axis=3).copy()
    u8[..., 1] = u8[..., 1][:, ::-1]
    want = torch.from_numpy(u8).float().div(255).permute(0, 3, 1, 2).contiguous().numpy()
    assert np.array_equal(host(FD.u8_to_planes(dev(u8))), want)
    rng = np.random.default_rng(9)
    imgs = rng.integers(0, 256, (2, 24, 80, 3)).astype(np.uint8)
    batch = torch.full((5, 3, 24, 80), -1.0, device="cuda")
    FD.u8_to_planes(dev(imgs), out=batch[2:4])
    b = host(batch)
    assert np.array_equal(b[2:4], torch.from_numpy(imgs).float().div(255).permute(0, 3, 1, 2).numpy())
    assert (b[:2] == -1).all() and (b[4:] == -1).all()
    odd = rng.integers(0, 256, (2, 7, 9, 3)).astype(np.uint8)
    assert np.array_equal(host(FD.u8_to_planes(dev(odd))), torch.from_numpy(odd).float().div(255).permute(0, 3, 1, 2).numpy())


def test_image_pyramid_equals_the_restatement():
    from fusiondepth_amd import functional as FD
    rng = np.random.default_rng(11)
    frames = np.stack([G.frame(50 + i) for i in range(4)])
    flip = [False, True, True, False]
    one = ((1.15, 0.85, 1.1, 0.08), [2, 0, 3, 1])
    per_scale = [((0.9, 1.1, 0.95, -0.06), [int(o) for o in rng.permutation(4)]) for _ in range(4)]
    jitter = [one, None, per_scale, one]
    out = FD.image_pyramid(dev(frames), 192, 640, 4, flip, jitter)
    plain = FD.image_pyramid(dev(frames), 192, 640, 4, flip, None)
    for n in range(4):
        pyr = R.pyramid(frames[n], 192, 640, 4, flip[n])
        for s in range(4):
            assert np.array_equal(host(out[("color", s)])[n], R.to_planes(pyr[s])), (n, s)
            j = jitter[n][s] if isinstance(jitter[n], list) else jitter[n]
            want = pyr[s] if j is None else R.color_jitter(pyr[s], j[0], j[1])
            assert np.array_equal(host(out[("color_aug", s)])[n], R.to_planes(want)), (n, s)
            assert np.array_equal(host(plain[("color", s)])[n], R.to_planes(pyr[s]))
    assert all(plain[("color_aug", s)] is plain[("color", s)] for s in range(4))
    assert out[("color", 0)].shape == (4, 3, 192, 640) and out[("color_aug", 3)].shape == (4, 3, 24, 80)
    assert all(t.is_contiguous() for t in out.values())


def test_bad_arguments_return_an_error_not_a_crash():
    from fusiondepth_amd import _lib
    from fusiondepth_amd import data_ops
    from fusiondepth_amd import functional as FD
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    y = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device="cuda")
    ws = torch.zeros((4096,), dtype=torch.uint8, device="cuda")
    tab = torch.zeros((4096,), dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="fd_resize_lanczos_u8"):
        _lib.call("fd_resize_lanczos_u8", None, None, 1, 8, 8, 4, 4, None, 13, None, 13, None, None, None)
    assert "bad args" in _lib.last_error()
    with pytest.raises(RuntimeError, match="bad args"):
        _lib.call("fd_resize_lanczos_u8", x.data_ptr(), y.data_ptr(), 0, 8, 8, 4, 4, tab.data_ptr(), 13, tab.data_ptr(), 13, None, ws.data_ptr(), None)
    with pytest.raises(RuntimeError, match="tap counts"):
        _lib.call("fd_resize_lanczos_u8", x.data_ptr(), y.data_ptr(), 1, 8, 8, 4, 4, tab.data_ptr(), 5, tab.data_ptr(), 13, None, ws.data_ptr(), None)
    with pytest.raises(RuntimeError, match="aligned"):
        _lib.call("fd_resize_lanczos_u8", x.data_ptr() + 1, y.data_ptr(), 1, 8, 8, 4, 4, tab.data_ptr(), 13, tab.data_ptr(), 13, None, ws.data_ptr(), None)
    with pytest.raises(RuntimeError, match="shrinks too far"):
        _lib.call("fd_resize_lanczos_u8", x.data_ptr(), y.data_ptr(), 1, 8, 100000, 4, 4, tab.data_ptr(), 150001, tab.data_ptr(), 13, None,
                  ws.data_ptr(), None)
    assert _lib.query("fd_resize_lanczos_u8_ws_bytes", 0, 8, 8, 4, 4) == 0
    with pytest.raises(RuntimeError, match="fd_u8_to_planes"):
        _lib.call("fd_u8_to_planes", None, None, 1, 8, 8, 192, None)
    with pytest.raises(RuntimeError, match="image stride"):
        _lib.call("fd_u8_to_planes", x.data_ptr(), ws.data_ptr(), 1, 8, 8, 10, None)
    with pytest.raises(RuntimeError, match="fd_color_jitter_u8"):
        _lib.call("fd_color_jitter_u8", None, 0, None, 0, None, 0, None, 1, 64, None, None)
    with pytest.raises(RuntimeError, match="bad args"):
        _lib.call("fd_color_jitter_u8", x.data_ptr(), 192, y.data_ptr(), 48, None, 0, tab.data_ptr(), 0, 64, ws.data_ptr(), None)
    assert _lib.query("fd_color_jitter_u8_ws_bytes", 0) == 0
    # a table entry whose extent leaves the buffers is skipped on the device: the output keeps its contents
    out = torch.full((1, 8, 8, 3), 7, dtype=torch.uint8, device="cuda")
    means = data_ops._run_jitter(x.view(-1), [(64, 0, -1, -1, 8, 8, (1.0, 1.0, 1.0, 0.0), [])], out.view(-1), None, 64)
    assert (host(out) == 7).all() and means.numel() == 1
    # an operation listed twice: refused by the wrapper, skipped by the kernel
    with pytest.raises(ValueError, match="distinct"):
        FD.color_jitter_u8(x, [((1.1, 0.9, 1.0, 0.0), [1, 0, 1])])
    data_ops._run_jitter(x.view(-1), [(0, 0, -1, -1, 8, 8, (1.1, 0.9, 1.0, 0.0), [1, 1])], out.view(-1), None, 64)
    assert (host(out) == 7).all()
    with pytest.raises(RuntimeError, match="uint8"):
        FD.resize_lanczos_u8(torch.zeros((1, 8, 8, 3), device="cuda"), (4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        FD.image_pyramid(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 4, 4, 1)
