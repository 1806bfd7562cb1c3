"""Baseline JPEG frames on the device: ``image_codecs.decode_jpeg_batch`` against Pillow on every byte (the fixtures of
tests/test_jpeg_cpu.py, all inside the covered set, so a fallback cannot hide a kernel failure), the fallback for an uncovered
stream, the descriptor rules of ``fd_jpeg_reconstruct``, and ``KITTIRAWBatches(decoder="device")`` - and one derived builder -
against the ``decoder="pil"`` batch, key by key."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

pytest.importorskip("PIL")

import jpeg_fixtures as JF
import kitti_tree as KT

pytestmark = pytest.mark.gpu

H, W, SCALES = 64, 96, 4
JITTERS = [((1.2, 0.8, 1.1, 0.1), [0, 1, 2, 3]), ((0.8, 1.2, 0.85, -0.1), [3, 2, 1, 0]), ((1.05, 0.95, 1.2, -0.04), [2, 0, 3, 1])]


def injected(epoch, index):
    aug, flip = bool(index % 2), bool((index // 2) % 2)
    return {"do_color_aug": aug, "do_flip": flip, "jitter": JITTERS[index % 3] if aug else None}


def _opt():
    return types.SimpleNamespace(need_4beam=True, need_2_channel=True, need_full_res_4beam=False, need_inf_gdc=False, clone_gdc=False,
                                 need_path=True, nbeams=4, random_sample=-1)


def _check(frames, datas, names):
    assert len(frames) == len(datas)
    for f, data, name in zip(frames, datas, names):
        want = JF.pillow_rgb(data)
        assert f.dtype == torch.uint8 and tuple(f.shape) == want.shape and f.is_cuda, name
        got = f.cpu().numpy()
        assert np.array_equal(got, want), (name, int((got != want).sum()))


def test_mixed_batch_equals_pillow_on_every_byte():
    from fusiondepth_amd import image_codecs
    names, datas = zip(*JF.fixtures())
    frames, stats = image_codecs.decode_jpeg_batch(list(datas))
    torch.cuda.synchronize()
    assert stats == {"device": len(datas), "fallback": 0}
    _check(frames, datas, names)
    # views of one buffer, same-size frames contiguous
    base = frames[0].untyped_storage().data_ptr()
    assert all(f.untyped_storage().data_ptr() == base for f in frames)
    by_size = {}
    for f in frames:
        by_size.setdefault(tuple(f.shape), []).append(f)
    for shape, group in by_size.items():
        for a, b in zip(group, group[1:]):
            assert b.data_ptr() == a.data_ptr() + a.numel(), shape


def test_one_file_alone(tmp_path):
    from fusiondepth_amd import image_codecs
    name, data = next((n, d) for n, d in JF.fixtures() if n == "33x31-420-noise-q92")
    path = os.path.join(str(tmp_path), "one.jpg")
    with open(path, "wb") as fh:
        fh.write(data)
    for src in (data, path):
        frames, stats = image_codecs.decode_jpeg_batch([src])
        assert stats == {"device": 1, "fallback": 0}
        _check(frames, [data], [name])


def test_uncovered_stream_falls_back_to_pillow():
    from fusiondepth_amd import image_codecs
    picks = [d for n, d in JF.fixtures() if n.startswith("50x40-") or n.startswith("33x31-422")]
    prog = dict(JF.uncovered())["progressive"]
    datas = picks[:3] + [prog] + picks[3:]
    frames, stats = image_codecs.decode_jpeg_batch(datas)
    assert stats == {"device": len(datas) - 1, "fallback": 1}
    _check(frames, datas, ["mixed %d" % i for i in range(len(datas))])


def _staging_for(datas):
    """The host job of a batch -> (its layout, descriptor table, total bytes, out bytes), to be uploaded by hand."""
    from fusiondepth_amd import image_codecs
    job = image_codecs.JpegBatchJob(datas)
    lay = job.wait_host()
    job.finish("cuda")                                           # writes the descriptor table
    torch.cuda.synchronize()
    table = job.descriptors()
    out_bytes = max(d.out_off + 3 * d.width * d.height for d in table)
    return lay, table, lay["total_bytes"], out_bytes


def _reconstruct(lay, table, total, out_bytes, fill=0x77):
    from fusiondepth_amd import _lib
    from fusiondepth_amd._lib import call, stream
    n = len(table)
    nbytes = n * ctypes.sizeof(_lib.JpegDesc)
    host = lay["staging"].clone()
    host.numpy()[:nbytes] = np.frombuffer(table, dtype=np.uint8)
    dev = torch.zeros((total,), dtype=torch.uint8, device="cuda")
    dev[:lay["upload_bytes"]].copy_(host)
    out = torch.full((out_bytes + 64,), fill, dtype=torch.uint8, device="cuda")
    call("fd_jpeg_reconstruct", dev.data_ptr(), total, dev.data_ptr(), n, out.data_ptr(), out_bytes, stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_two_calls_give_the_same_bytes_and_bad_descriptors_write_zeros_or_nothing():
    by_name = dict(JF.fixtures())
    datas = [by_name[n] for n in ("50x40-420-noise-q92", "17x9-422-optimize", "33x31-grey-noise-q92", "64x24-444-checker-q100")]
    lay, table, total, out_bytes = _staging_for(datas)
    a = _reconstruct(lay, table, total, out_bytes)
    b = _reconstruct(lay, table, total, out_bytes)
    assert np.array_equal(a, b)
    assert (a[out_bytes:] == 0x77).all()                          # nothing behind out_bytes
    for d, data in zip(table, datas):
        want = JF.pillow_rgb(data)
        assert np.array_equal(a[d.out_off:d.out_off + want.size].reshape(want.shape), want)
    # frame 0's coefficients leave staging -> a zero frame; frame 1's sampling is unknown -> zeros; frame 2 leaves `out` -> untouched
    bad = (type(table[0]) * 4).from_buffer_copy(bytes(table))
    bad[0].coef_off = total - 64
    bad[1].h_samp = 3
    bad[2].out_off = out_bytes - 5
    c = _reconstruct(lay, bad, total, out_bytes)
    for k, (d, data) in enumerate(zip(table, datas)):
        want = JF.pillow_rgb(data)
        got = c[d.out_off:d.out_off + want.size]
        if k in (0, 1):
            assert (got == 0).all(), k
        elif k == 2:
            assert (got == 0x77).all(), k
        else:
            assert np.array_equal(got.reshape(want.shape), want)
    assert (c[out_bytes:] == 0x77).all()
    # sampling factors that a packed compare (16 * h + v) would take for 1x1 / 2x1, and that shrink the plane sizes a shift computes:
    # every frame must come out zero.  The planes lie at the very end of staging, so a plane read past its region leaves the buffer.
    assert table[3].plane_off + 64 * (8 * 3 * 3) == total          # the 64x24 4:4:4 frame's 72 blocks end the buffer
    for hv3, hv1 in (((1, 17), (0, 17)), ((0, 33), (2, -15)), ((2, -15), (1, 17)), ((3, -14), (-1, 33)), ((2, 3), (1, 2))):
        bad = (type(table[0]) * 4).from_buffer_copy(bytes(table))
        for d in bad:
            d.h_samp, d.v_samp = hv3 if d.components == 3 else hv1
        bad[2].plane_off = total                                  # greyscale: a zero-length plane region right behind the buffer
        c = _reconstruct(lay, bad, total, out_bytes)
        for d, data in zip(table, datas):
            n = 3 * d.width * d.height
            assert (c[d.out_off:d.out_off + n] == 0).all(), (hv3, hv1, d.width, d.height)
        assert (c[out_bytes:] == 0x77).all()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """Two drives of different native size, JPEG frames (Pillow's defaults: quality 75, 4:2:0)."""
    root = str(tmp_path_factory.mktemp("kitti_jpeg"))
    drives = [("2011_09_26", "2011_09_26_drive_0001_sync", (128, 192), (192 / 1242.0, 128 / 375.0)),
              ("2011_09_30", "2011_09_30_drive_0016_sync", (121, 181), (181 / 1242.0, 121 / 375.0))]
    lines = KT.make_tree(root, drives, frames=4, ext=".jpg")
    from PIL import Image
    for date, drive, (im_h, im_w), _ in drives:                   # the stereo partner's frames
        d = os.path.join(root, date, drive, "image_03/data")
        os.makedirs(d)
        rng = np.random.default_rng(im_h)
        for i in range(4):
            Image.fromarray(rng.integers(0, 256, (im_h, im_w, 3), dtype=np.uint8)).save(os.path.join(d, "%010d.jpg" % i), quality=92, subsampling=1)
    return root, lines                                           # 2 lines per drive: items 0 .. 3


def _all_batches(cls, root, lines, frames, decoder):
    b = cls(root, lines, H, W, frames, SCALES, is_train=True, img_ext=".jpg", opt=_opt(), batch_size=2, draws=injected,
            prefetch=False, decoder=decoder)
    order = [0, 2, 1, 3]                                          # both batches mix the two native sizes
    batches = [b.build_batch(0, order[i:i + 2]) for i in (0, 2)]
    torch.cuda.synchronize()
    stats = dict(b.decode_stats)
    b.close()
    return batches, stats


@pytest.mark.parametrize("builder, frames", [("KITTIRAWBatches", [0, -1, 1]), ("KITTIStereoBatches", [0, -1, 1, "s"])])
def test_loader_batches_equal_the_pil_route(tree, builder, frames):
    from fusiondepth_amd import datasets
    root, lines = tree
    assert len(lines) == 4
    cls = getattr(datasets, builder)
    want, pil_stats = _all_batches(cls, root, lines, frames, "pil")
    got, stats = _all_batches(cls, root, lines, frames, "device")
    assert pil_stats == {"device": 0, "fallback": 0}
    assert stats == {"device": 2 * 2 * len(frames), "fallback": 0}
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for key in w:
            if torch.is_tensor(w[key]):
                assert g[key].shape == w[key].shape and torch.equal(g[key], w[key]), key
            else:
                assert g[key] == w[key], key
    assert not torch.equal(got[0][("color", 0, 0)], got[1][("color", 0, 0)])


def test_prefetched_iteration_equals_the_pil_route(tree):
    """``for batch in loader`` - the route a training run takes: host jobs two batches ahead, the device work on the builder's own
    stream, staging and device buffers released while their copy and kernels are queued - over two epochs, against the pil route."""
    from fusiondepth_amd.datasets import KITTIRAWBatches
    root, lines = tree

    def epochs(decoder):
        b = KITTIRAWBatches(root, lines, H, W, [0, -1, 1], SCALES, is_train=True, img_ext=".jpg", opt=_opt(), batch_size=1, draws=injected,
                            shuffle=True, seed=3, prefetch=True, decoder=decoder)
        got = []
        for _ in range(2):
            for batch in b:
                got.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()})
        torch.cuda.synchronize()
        stats = dict(b.decode_stats)
        b.close()
        return got, stats

    want, _ = epochs("pil")
    got, stats = epochs("device")
    assert len(got) == len(want) == 8 and stats == {"device": 8 * 3, "fallback": 0}
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for key in w:
            assert torch.equal(g[key], w[key]) if torch.is_tensor(w[key]) else g[key] == w[key], key


def test_loader_arguments(tree):
    from fusiondepth_amd.datasets import KITTIRAWBatches, pil_loader
    root, lines = tree
    with pytest.raises(ValueError, match="loader="):
        KITTIRAWBatches(root, lines, H, W, [0], SCALES, opt=_opt(), decoder="device", loader=pil_loader)
    with pytest.raises(ValueError, match="decoder"):
        KITTIRAWBatches(root, lines, H, W, [0], SCALES, opt=_opt(), decoder="gpu")
    assert KITTIRAWBatches(root, lines, H, W, [0], SCALES, opt=_opt(), img_ext=".png", decoder="device").decoder == "pil"
    assert KITTIRAWBatches(root, lines, H, W, [0], SCALES, opt=_opt()).decoder == "pil"
