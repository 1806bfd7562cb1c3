"""JPEG outputs on the device: ``image_codecs.encode_jpeg_batch`` against the restatement (tests/jpeg_enc_ref.py) and against Pillow, whole
files with no tolerance, on the sizes and contents of tests/jpeg_enc_fixtures.py in batches that mix sizes and samplings; against itself
on a second call; through this project's own decoder; and ``convert_frames`` on a tiny tree against its ``pil`` run."""
import io
import os

import numpy as np
import pytest
import torch

pytest.importorskip("PIL")
from PIL import Image

import jpeg_enc_fixtures as EF
import jpeg_enc_ref as ER

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (8, 8), (7, 9), (24, 40), (12, 9), (31, 16), (64, 65), (17, 33))
QUALITIES = (10, 92, 100)


@pytest.fixture(scope="module")
def ops():
    from fusiondepth_amd import image_codecs
    return image_codecs


@pytest.fixture(scope="module")
def small():
    """{quality: [(name, rgb, sampling)]} - every size at every sampling and quality, every content at each."""
    out = {}
    for name, rgb, q, s in EF.cases(qualities=QUALITIES, sizes=SIZES):
        out.setdefault(q, []).append((name, rgb, s))
    for q in QUALITIES:                                          # every size x sampling x quality, whatever the round-robin gave
        have = {(r.shape[:2], s) for _, r, s in out[q]}
        for h, w in SIZES:
            for s in EF.SAMPLINGS:
                if ((h, w), s) not in have:
                    out[q].append(("noise-%dx%d-q%d-%s" % (h, w, q, s), EF.content("noise", h, w, seed=q), s))
    return out


@pytest.fixture(scope="module")
def encoded(ops, small):
    """{quality: (cases, files as bytes, stats)} - one call per quality, sizes and samplings mixed, device tensors and host arrays mixed."""
    out = {}
    for q, cases in small.items():
        images = [torch.from_numpy(r).cuda() if k % 2 == 0 else r for k, (_, r, _) in enumerate(cases)]
        files, stats = ops.encode_jpeg_batch(images, quality=q, sampling=[s for _, _, s in cases])
        assert all(isinstance(f, memoryview) for f in files)
        out[q] = (cases, [bytes(f) for f in files], stats)
    return out


def test_cases_reach_every_size_sampling_quality_and_content(small):
    for q in QUALITIES:
        assert {(r.shape[:2], s) for _, r, s in small[q]} == {(hw, s) for hw in SIZES for s in EF.SAMPLINGS}
        assert {n.split("-")[0] for n, _, _ in small[q]} >= set(EF.CONTENTS)
    assert any(n.startswith("checker") for n, _, _ in small[100])
    assert any(n.startswith("sparks") for n, _, _ in small[10]) and any(n.startswith("fine") for n, _, _ in small[10])


def test_files_equal_pillow_and_the_restatement_byte_for_byte(encoded):
    for q, (cases, files, stats) in encoded.items():
        for (name, rgb, s), data in zip(cases, files):
            assert data == EF.pillow(rgb, q, s), (name, len(data))
            assert data == ER.encode(rgb, q, s), name
        assert stats == {"device": len(cases), "fallback": 0, "bytes": sum(len(f) for f in files)}


def test_one_kitti_frame(ops):
    """375 x 1242: odd H, W = 77 * 16 + 10, 11 232 blocks at 2x2 and 21 996 at 1x1 - the only image with more than one step of the
    per-image scan and with many tiles - at all three samplings and at qualities 10, 92 and 100, each quality as one batch of the three
    samplings; every file against Pillow, one of them against the restatement too."""
    cases = EF.frame_cases()
    assert {(q, s) for _, _, q, s in cases} == {(q, s) for q in QUALITIES for s in EF.SAMPLINGS}
    for q in QUALITIES:
        part = [c for c in cases if c[2] == q]
        files, stats = ops.encode_jpeg_batch([torch.from_numpy(rgb).cuda() for _, rgb, _, _ in part], quality=q, sampling=[s for _, _, _, s in part])
        assert stats["device"] == 3 and stats["fallback"] == 0
        for (name, rgb, _, s), data in zip(part, files):
            assert bytes(data) == EF.pillow(rgb, q, s), name
    name, rgb, q, s = [c for c in cases if c[2] == 92 and c[3] == "2x2"][0]
    assert EF.pillow(rgb, q, s) == ER.encode(rgb, q, s), name


def test_a_mixed_batch_equals_single_calls_in_as_many_library_calls(ops, monkeypatch):
    picks = [((64, 65), "2x2", "noise"), ((17, 33), "2x1", "gradient"), ((1, 1), "1x1", "white"), ((31, 16), "2x2", "sparks"),
             ((24, 40), "1x1", "checker")]
    images = [EF.content(c, h, w) for (h, w), _, c in picks]
    names = [s for _, s, _ in picks]
    seen = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (seen.append(name), real(name, *a))[1])
    batch, stats = ops.encode_jpeg_batch(images, quality=92, sampling=names)
    five = list(seen)
    del seen[:]
    single, _ = ops.encode_jpeg_batch(images[:1], quality=92, sampling=names[:1])
    assert five == list(seen) == ["fd_jpeg_enc_encode"]           # one call of seven launches for N = 5 and for N = 1
    assert bytes(single[0]) == bytes(batch[0])
    for a, s, f in zip(images, names, batch):
        (alone,), _ = ops.encode_jpeg_batch([a], quality=92, sampling=s)
        assert bytes(alone) == bytes(f) == EF.pillow(a, 92, s)
    assert stats["device"] == 5 and all(f.obj is batch[0].obj for f in batch) and batch[0].obj.size == stats["bytes"]


def test_two_calls_give_equal_bytes(ops, small, encoded):
    cases, files, _ = encoded[100]
    again, _ = ops.encode_jpeg_batch([torch.from_numpy(r).cuda() for _, r, _ in cases], quality=100, sampling=[s for _, _, s in cases])
    assert [bytes(f) for f in again] == files


def test_own_decoder_returns_pillow_s_pixels(ops, encoded):
    cases, files, _ = encoded[92]
    frames, stats = ops.decode_jpeg_batch(files)
    assert stats == {"device": len(files), "fallback": 0}
    for (name, _, _), data, f in zip(cases, files, frames):
        with Image.open(io.BytesIO(data)) as img:
            assert np.array_equal(f.cpu().numpy(), np.asarray(img.convert("RGB"))), name


def test_uncovered_inputs_are_refused(ops):
    ok = torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda")
    for bad in (torch.zeros((4, 4, 3), device="cuda"), torch.zeros((4, 4, 4), dtype=torch.uint8, device="cuda"),
                torch.zeros((4, 4), dtype=torch.uint16, device="cuda"), torch.zeros((0, 4, 3), dtype=torch.uint8, device="cuda"),
                np.zeros((1, 65536, 3), np.uint8), np.zeros((2, 2, 4, 3), np.uint8), [[1, 2, 3]]):
        with pytest.raises(ValueError):
            ops.encode_jpeg_batch([ok, bad])
    for kw in ({"quality": 0}, {"quality": 101}, {"quality": 92.0}, {"sampling": "4x4"}, {"sampling": 2}, {"sampling": ["2x2"]}):
        with pytest.raises(ValueError):
            ops.encode_jpeg_batch([ok, ok], **kw)
    with pytest.raises(ValueError):
        ops.encode_jpeg_batch([])


def test_a_grey_image_arrives_through_the_fallback(ops):
    grey = EF.content("noise", 13, 21)[:, :, 0].copy()
    rgb = EF.content("gradient", 13, 21)
    files, stats = ops.encode_jpeg_batch([torch.from_numpy(grey).cuda(), rgb], quality=75, sampling="2x1")
    assert stats == {"device": 1, "fallback": 1, "bytes": len(files[0]) + len(files[1])}
    assert bytes(files[0]) == EF.pillow(grey, 75, None) and bytes(files[1]) == EF.pillow(rgb, 75, "2x1")
    with Image.open(io.BytesIO(bytes(files[0]))) as img:
        assert img.mode == "L"


# --------------------------------------------------------------------------------------------- the command
def _tree(root):
    """Two RGB sizes, one grey PNG, one 16-bit PNG and one PNG whose .jpg exists -> {relative path: kind}."""
    kinds = {}
    os.makedirs(os.path.join(root, "a", "image_02"))
    os.makedirs(os.path.join(root, "b"))
    for rel, arr, kind in (("a/image_02/0000000000.png", EF.content("texture", 37, 124), "rgb"),
                           ("a/image_02/0000000001.png", EF.content("texture", 37, 124, seed=1), "rgb"),
                           ("a/image_02/0000000002.png", EF.content("noise", 24, 40), "rgb"),
                           ("b/grey.png", EF.content("gradient", 19, 30)[:, :, 0].copy(), "grey"),
                           ("b/depth.png", (np.arange(19 * 30, dtype=np.uint16).reshape(19, 30) * 97), "depth"),
                           ("b/done.png", EF.content("checker", 16, 16), "done")):
        Image.fromarray(arr).save(os.path.join(root, rel))
        kinds[rel] = kind
    with open(os.path.join(root, "b", "done.jpg"), "wb") as f:
        f.write(b"already here")
    return kinds


def _want(path):
    f = io.BytesIO()
    with Image.open(path) as img:
        if img.mode == "L":
            img.save(f, "JPEG", quality=92)
        else:
            img.convert("RGB").save(f, "JPEG", quality=92, subsampling=2)
    return f.getvalue()


def test_convert_frames_on_a_tiny_tree(tmp_path):
    from fusiondepth_amd import convert_frames as C
    src = str(tmp_path / "kitti")
    kinds = _tree(src)
    depth_before = open(os.path.join(src, "b", "depth.png"), "rb").read()
    outs = {}
    for enc in ("device", "pil"):
        dst = str(tmp_path / ("out_" + enc))
        res = C.main(["--data_path", src, "--out_path", dst, "--encoder", enc, "--png_decoder", enc, "--batch", "3", "--workers", "4"])
        assert res["converted"] == 5 and res["skipped"] == 1 and res["deleted"] == 0, res      # out_path holds no done.jpg: it is converted
        assert (res["device"], res["fallback"]) == ((4, 1) if enc == "device" else (0, 5)), res
        outs[enc] = {}
        for rel, kind in kinds.items():
            jpg = os.path.join(dst, rel[:-4] + ".jpg")
            assert os.path.exists(jpg) == (kind != "depth"), rel
            if kind != "depth":
                outs[enc][rel] = open(jpg, "rb").read()
                assert outs[enc][rel] == _want(os.path.join(src, rel)), (enc, rel)
        assert res["bytes_out"] == sum(len(v) for v in outs[enc].values())
        assert not [n for _, _, names in os.walk(dst) for n in names if not n.endswith(".jpg")]         # no temporary file is left
    assert outs["device"] == outs["pil"]
    # in place, with --delete_png: the existing .jpg is kept and its PNG stays; the 16-bit file is untouched; the converted PNGs go
    res = C.main(["--data_path", src, "--delete_png", "--batch", "4", "--workers", "4"])
    assert res["converted"] == 4 and res["skipped"] == 2 and res["deleted"] == 4 and res["device"] == 3 and res["fallback"] == 1, res
    left = sorted(os.path.relpath(os.path.join(d, n), src) for d, _, names in os.walk(src) for n in names)
    assert left == sorted(["a/image_02/0000000000.jpg", "a/image_02/0000000001.jpg", "a/image_02/0000000002.jpg", "b/grey.jpg", "b/depth.png",
                           "b/done.png", "b/done.jpg"])
    assert open(os.path.join(src, "b", "depth.png"), "rb").read() == depth_before
    assert open(os.path.join(src, "b", "done.jpg"), "rb").read() == b"already here"
    for rel in ("a/image_02/0000000000", "a/image_02/0000000002", "b/grey"):
        assert open(os.path.join(src, rel + ".jpg"), "rb").read() == outs["pil"][rel + ".png"]
    res = C.main(["--data_path", src, "--overwrite", "--delete_png"])                         # now done.png is converted too
    assert res["converted"] == 1 and res["deleted"] == 1 and res["skipped"] == 1, res
    assert open(os.path.join(src, "b", "done.jpg"), "rb").read() == outs["pil"]["b/done.png"]
    with pytest.raises(ValueError):
        C.main(["--data_path", src, "--encoder", "magick"])
