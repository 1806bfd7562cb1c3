"""PNG frames on the device: ``image_codecs.decode_png_batch`` against Pillow on every byte (the fixtures of tests/test_png_cpu.py, all
inside the covered set, so a fallback cannot hide a kernel failure), the fallback for uncovered and damaged files, the descriptor
rules of ``fd_png_unfilter``, ``KITTIRAWBatches(png_decoder="device")`` - and one derived builder - against the ``png_decoder="pil"``
batch key by key, and the depth keys of ``KITTICompletionBatches``.  Every comparison is ``array_equal``."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

pytest.importorskip("PIL")

import completion_tree as CT
import kitti_tree as KT
import png_fixtures as PF

pytestmark = pytest.mark.gpu

H, W, SCALES = 64, 96, 4
JITTERS = [((1.2, 0.8, 1.1, 0.1), [0, 1, 2, 3]), ((0.8, 1.2, 0.85, -0.1), [3, 2, 1, 0]), ((1.05, 0.95, 1.2, -0.04), [2, 0, 3, 1])]


def injected(epoch, index):
    aug, flip = bool(index % 2), bool((index // 2) % 2)
    return {"do_color_aug": aug, "do_flip": flip, "jitter": JITTERS[index % 3] if aug else None}


def _opt():
    return types.SimpleNamespace(need_4beam=True, need_2_channel=True, need_full_res_4beam=False, need_inf_gdc=False, clone_gdc=False,
                                 need_path=True, nbeams=4, random_sample=-1)


def _split():
    """The covered fixtures by the mode that takes them on the device: ([(name, data)] 8-bit, [(name, data)] 16-bit)."""
    eight = [(n, d) for n, d in PF.fixtures() if not n.startswith("g16")]
    sixteen = [(n, d) for n, d in PF.fixtures() if n.startswith("g16")]
    assert len(eight) > 80 and len(sixteen) > 20
    return eight, sixteen


def _check(frames, datas, names, dtype=torch.uint8):
    assert len(frames) == len(datas)
    for f, data, name in zip(frames, datas, names):
        want = PF.pillow(data) if dtype == torch.uint16 else PF.pillow_rgb(data)
        assert f.dtype == dtype and tuple(f.shape) == want.shape and f.is_cuda, (name, f.dtype, tuple(f.shape), want.shape)
        got = f.cpu().numpy()
        assert got.dtype == want.dtype and np.array_equal(got, want), (name, int((got != want).sum()))


def _contiguous_views(frames):
    base = frames[0].untyped_storage().data_ptr()
    assert all(f.untyped_storage().data_ptr() == base for f in frames)
    by_size = {}
    for f in frames:
        by_size.setdefault(tuple(f.shape), []).append(f)
    assert any(len(g) > 1 for g in by_size.values())
    for shape, group in by_size.items():
        for a, b in zip(group, group[1:]):
            assert b.data_ptr() == a.data_ptr() + a.numel() * a.element_size(), shape


def _count_calls(monkeypatch):
    from fusiondepth_amd import image_codecs
    seen = []
    real = image_codecs.call
    monkeypatch.setattr(image_codecs, "call", lambda name, *a: (seen.append(name), real(name, *a))[1])
    return seen


def test_mixed_rgb_batch_equals_pillow_on_every_byte(monkeypatch):
    from fusiondepth_amd import image_codecs
    seen = _count_calls(monkeypatch)
    names, datas = zip(*_split()[0])
    frames, stats = image_codecs.decode_png_batch(list(datas))
    torch.cuda.synchronize()
    assert stats == {"device": len(datas), "fallback": 0}
    assert seen == ["fd_png_unfilter"]                           # one call per batch
    _check(frames, datas, names)
    _contiguous_views(frames)


def test_gray16_batch_equals_pillow_on_every_value(monkeypatch):
    from fusiondepth_amd import image_codecs
    seen = _count_calls(monkeypatch)
    names, datas = zip(*_split()[1])
    frames, stats = image_codecs.decode_png_batch(list(datas), mode="gray16")
    torch.cuda.synchronize()
    assert stats == {"device": len(datas), "fallback": 0} and seen == ["fd_png_unfilter"]
    _check(frames, datas, names, torch.uint16)
    _contiguous_views(frames)
    assert any(int(f.cpu().numpy().max()) > 255 for f in frames)


def test_one_file_alone(tmp_path):
    from fusiondepth_amd import image_codecs
    name, data = next((n, d) for n, d in PF.fixtures() if n == "rgb8-texture-300x200")
    path = os.path.join(str(tmp_path), "one.png")
    with open(path, "wb") as fh:
        fh.write(data)
    for src in (data, path):
        frames, stats = image_codecs.decode_png_batch([src])
        assert stats == {"device": 1, "fallback": 0}
        _check(frames, [data], [name])


def test_uncovered_and_damaged_files_fall_back_to_pillow():
    from fusiondepth_amd import image_codecs
    eight, sixteen = _split()
    picks = [d for n, d in eight if "-wbits" in n or "-strategy-" in n]
    uncovered = [d for _, d in PF.uncovered()]
    damaged = bytearray(picks[0])
    damaged[-5] ^= 0x40                                          # IEND's CRC: this decoder refuses the file, Pillow reads it
    datas = picks[:3] + uncovered[:3] + [bytes(damaged), sixteen[0][1]] + uncovered[3:] + picks[3:]
    frames, stats = image_codecs.decode_png_batch(datas)
    assert stats == {"device": len(picks), "fallback": len(uncovered) + 2}       # a 16-bit file in rgb mode is Pillow's too
    _check(frames, datas, ["mixed %d" % i for i in range(len(datas))])
    # gray16 mode: an 8-bit grey file is Pillow's (np.asarray gives uint8 values), an RGB file is refused as the loader refuses it
    g8 = next(d for n, d in eight if n.startswith("g8-pillow"))
    frames, stats = image_codecs.decode_png_batch([sixteen[1][1], g8], mode="gray16")
    assert stats == {"device": 1, "fallback": 1}
    assert np.array_equal(frames[1].cpu().numpy(), PF.pillow_rgb(g8)[:, :, 0].astype(np.uint16))
    with pytest.raises(RuntimeError, match="single-channel integer"):
        image_codecs.decode_png_batch([picks[0]], mode="gray16")
    with pytest.raises(ValueError, match="mode"):
        image_codecs.decode_png_batch([picks[0]], mode="rgba")


def _staging_for(datas, mode):
    """The host job of a batch -> (its layout, descriptor table, out bytes), to be uploaded by hand."""
    from fusiondepth_amd import image_codecs
    job = image_codecs.PngBatchJob(datas, None, mode)
    lay = job.wait_host()
    table, _, _, _, out_bytes = job.layout()
    return lay, table, out_bytes


def test_sizes_are_pillow_s_after_wait_host():
    from fusiondepth_amd import image_codecs
    by_name = dict(PF.fixtures())
    small = next(d for _, d in PF.uncovered() if max(PF.pillow_rgb(d).shape[:2]) <= 65)      # its size comes from Pillow's header read
    datas = [by_name["rgb8-random-65x65"], small, by_name["rgb8-first4-5x3"], by_name["rgb8-random-65x65"]]
    job = image_codecs.PngBatchJob(datas)
    job.wait_host()
    assert job.sizes() == [PF.pillow_rgb(d).shape[:2] for d in datas]


def _unfilter(lay, table, out_bytes, fill=0x77, staging_bytes=None, out_size=None, twice=False):
    """-> (status, out as numpy); the table goes to the head of the device copy as ``fd_png_unfilter`` expects."""
    from fusiondepth_amd import _lib
    n = len(table)
    host = lay["staging"].clone()
    host.numpy()[:n * ctypes.sizeof(_lib.PngDesc)] = np.frombuffer(table, dtype=np.uint8)
    dev = host.cuda()
    out = torch.full((out_bytes + 64,), fill, dtype=torch.uint8, device="cuda")
    fn = _lib.load().fd_png_unfilter
    for _ in range(2 if twice else 1):
        st = fn(dev.data_ptr(), lay["upload_bytes"] if staging_bytes is None else staging_bytes, ctypes.addressof(table), n, out.data_ptr(),
                out_bytes if out_size is None else out_size, _lib.stream())
    torch.cuda.synchronize()
    return st, out.cpu().numpy()


def test_descriptor_rules_and_two_calls_give_the_same_bytes():
    from fusiondepth_amd import _lib
    by_name = dict(PF.fixtures())
    grey = next(n for n in by_name if n.startswith("g8-pillow-65x64") and n.endswith("l6"))
    names = ["rgb8-random-65x65", grey, "rgb8-band-3x%d" % (_lib.load().fd_png_band_rows() + 1), "rgb8-first4-5x3"]
    datas = [by_name[n] for n in names]
    lay, table, out_bytes = _staging_for(datas, "rgb")
    st, a = _unfilter(lay, table, out_bytes)
    st2, b = _unfilter(lay, table, out_bytes, twice=True)        # the second call finds reconstructed rows of filter type 0
    assert st == 0 and st2 == 0 and np.array_equal(a, b)
    assert (a[out_bytes:] == 0x77).all()                          # nothing behind out_bytes
    for d, data in zip(table, datas):
        want = PF.pillow_rgb(data)
        assert np.array_equal(a[d.out_off:d.out_off + want.size].reshape(want.shape), want)

    def refused(change, match, **kw):
        bad = (type(table[0]) * len(table)).from_buffer_copy(bytes(table))
        change(bad)
        st, c = _unfilter(lay, bad, out_bytes, **kw)
        assert st != 0 and match in _lib.last_error(), (st, _lib.last_error())
        assert (c == 0x77).all()                                 # not launched: not a byte of out was written

    total = lay["upload_bytes"]
    refused(lambda t: setattr(t[0], "raw_off", total - 64), "descriptor 0: the frame's source leaves staging")
    refused(lambda t: setattr(t[1], "raw_off", 16), "descriptor 1: raw_off lies before the end of the descriptor table")
    refused(lambda t: setattr(t[2], "out_off", out_bytes - 5), "descriptor 2: the frame leaves out")
    refused(lambda t: setattr(t[2], "out_off", -16), "descriptor 2: the frame leaves out")
    refused(lambda t: setattr(t[3], "bpp", 2), "descriptor 3: bpp and mode")
    refused(lambda t: setattr(t[3], "kind", 2), "descriptor 3: kind")
    refused(lambda t: setattr(t[3], "mode", 7), "descriptor 3: mode")
    refused(lambda t: setattr(t[0], "width", 0), "descriptor 0: width or height")
    refused(lambda t: setattr(t[0], "height", 65536), "descriptor 0: width or height")
    refused(lambda t: setattr(t[0], "width", 40000) or setattr(t[0], "height", 40000), "descriptor 0: more than 2^31 - 1 bytes")
    refused(lambda t: None, "the frame's source leaves staging", staging_bytes=total - 16)     # the last frame's scanlines
    refused(lambda t: None, "the frame leaves out", out_size=out_bytes - 16)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """Two drives of different native size, PNG frames written by Pillow."""
    root = str(tmp_path_factory.mktemp("kitti_png"))
    drives = [("2011_09_26", "2011_09_26_drive_0001_sync", (128, 192), (192 / 1242.0, 128 / 375.0)),
              ("2011_09_30", "2011_09_30_drive_0016_sync", (121, 181), (181 / 1242.0, 121 / 375.0))]
    lines = KT.make_tree(root, drives, frames=4, ext=".png")
    from PIL import Image
    for date, drive, (im_h, im_w), _ in drives:                   # the stereo partner's frames
        d = os.path.join(root, date, drive, "image_03/data")
        os.makedirs(d)
        rng = np.random.default_rng(im_h)
        for i in range(4):
            Image.fromarray(rng.integers(0, 256, (im_h, im_w, 3), dtype=np.uint8) // 16 * 16).save(os.path.join(d, "%010d.png" % i))
    return root, lines                                           # 2 lines per drive: items 0 .. 3


def _all_batches(cls, root, lines, frames, png_decoder):
    b = cls(root, lines, H, W, frames, SCALES, is_train=True, img_ext=".png", opt=_opt(), batch_size=2, draws=injected,
            prefetch=False, png_decoder=png_decoder)
    order = [0, 2, 1, 3]                                          # both batches mix the two native sizes
    batches = [b.build_batch(0, order[i:i + 2]) for i in (0, 2)]
    torch.cuda.synchronize()
    stats = dict(b.decode_stats)
    b.close()
    return batches, stats


def _same_batches(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for key in w:
            if torch.is_tensor(w[key]):
                assert g[key].shape == w[key].shape and torch.equal(g[key], w[key]), key
            else:
                assert g[key] == w[key], key


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
    _same_batches(got, want)
    assert not torch.equal(got[0][("color", 0, 0)], got[1][("color", 0, 0)])


def test_prefetched_iteration_equals_the_pil_route(tree):
    """``for batch in loader`` - the route a training run takes - over one shuffled epoch, against the pil route."""
    from fusiondepth_amd.datasets import KITTIRAWBatches
    root, lines = tree

    def epoch(png_decoder):
        b = KITTIRAWBatches(root, lines, H, W, [0, -1, 1], SCALES, is_train=True, img_ext=".png", opt=_opt(), batch_size=1, draws=injected,
                            shuffle=True, seed=3, prefetch=True, png_decoder=png_decoder)
        got = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()} for batch in b]
        torch.cuda.synchronize()
        stats = dict(b.decode_stats)
        b.close()
        return got, stats

    want, _ = epoch("pil")
    got, stats = epoch("device")
    assert len(got) == 4 and stats == {"device": 4 * 3, "fallback": 0}
    _same_batches(got, want)


def test_completion_depth_keys_equal_the_pil_route(tmp_path_factory):
    from fusiondepth_amd.completion_data import KITTICompletionBatches
    root = CT.make_tree(str(tmp_path_factory.mktemp("completion_png") / "completion"))
    opt = CT.options(eval_gdc=True, need_path=True)

    def batch(png_decoder):
        b = KITTICompletionBatches(root, 352, 1216, [0, -1, 1], 4, is_train=True, opt=opt, batch_size=2, draws=injected, prefetch=False,
                                   png_decoder=png_decoder)
        out = b.build_batch(0, [0, 1])
        torch.cuda.synchronize()
        stats = dict(b.decode_stats)
        b.close()
        return out, stats

    want, _ = batch("pil")
    got, stats = batch("device")
    for key in ("4beam", "2channel", "depth_gt", "full_res_4beam", ("2channel", 0, 0), ("2channel", -1, 0), ("2channel", 1, 0)):
        assert key in want, key
    assert stats["fallback"] == 0 and stats["device"] >= 4
    _same_batches([got], [want])
    # the reference's 16-bit assertion, with the path
    full = KITTICompletionBatches(root, 352, 1216, [0], 4, is_train=False, val_split="full", opt=CT.options(), batch_size=1, drop_last=False,
                                  prefetch=False, png_decoder="device")
    bad = [i for i, p in enumerate(full.paths["d"]) if p.endswith("%010d.png" % CT.EIGHT_BIT_FRAME)]
    assert len(bad) == 1
    with pytest.raises(AssertionError, match=r"np.max\(depth_png\)=255, path=.*%010d.png" % CT.EIGHT_BIT_FRAME):
        full.build_batch(0, bad)
    full.close()
