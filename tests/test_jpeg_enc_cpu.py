"""The JPEG encoder without a GPU: the restated rules (tests/jpeg_enc_ref.py) give the bytes Pillow writes, with no tolerance; the other
arbiter (tests/jpeg_ref.py) decodes them to Pillow's pixels; and the host half of the encoder (fd_jpeg_enc_quant_tables / _header /
_layout, csrc/jpeg_enc_host.h) equals the restatement - which pins the stream of include/fdhip.h ("JPEG outputs") on any machine."""
import io

import numpy as np
import pytest

pytest.importorskip("PIL")
from PIL import Image

import jpeg_enc_fixtures as EF
import jpeg_enc_ref as ER
import jpeg_ref as JR


@pytest.fixture(scope="module")
def ops():
    from fusiondepth_amd import build
    build.build(verbose=False)
    from fusiondepth_amd import image_codecs
    return image_codecs


@pytest.fixture(scope="module")
def cases():
    """[(name, rgb, quality, sampling, the restatement's file, Pillow's file)] - the small sizes, built from seeds, encoded once."""
    return [(n, a, q, s, ER.encode(a, q, s), EF.pillow(a, q, s)) for n, a, q, s in EF.cases()]


def test_fixtures_cover_what_they_claim():
    cs = EF.cases()
    assert len({n for n, _, _, _ in cs}) == len(cs) >= len(EF.SIZES) * 3 * len(EF.CONTENTS)
    assert all("%s-%dx%d-q%d-%s" % (c, h, w, q, s) in {n for n, _, _, _ in cs}
               for c, q in (("checker", 100), ("sparks", 10), ("fine", 10)) for h, w in EF.SIZES for s in EF.SAMPLINGS)
    assert {a.shape[:2] for _, a, _, _ in cs} >= {(1, 1), (8, 8), (4, 8), (12, 9), (17, 33), (31, 16), (20, 23), (24, 40), (64, 65)}
    assert {q for _, _, q, _ in cs} >= {30, 75, 92, 100} and {s for _, _, _, s in cs} == {"1x1", "2x1", "2x2"}
    for c in EF.CONTENTS:                                        # every content meets every sampling
        assert {s for n, _, _, s in cs if n.startswith(c)} == {"1x1", "2x1", "2x2"}, c
    # the contents reach the branches they are there for
    blocks, which = ER.scan_blocks(EF.content("checker", 64, 65), 100, "1x1")
    dc = [int(b[0]) for b, c in zip(blocks, which) if c == 0]
    assert max(abs(a - b) for a, b in zip(dc[1:], dc[:-1])) >= 1024                        # DC differences of category 11
    for kind, q in (("fine", 10), ("sparks", 30)):
        blocks, _ = ER.scan_blocks(EF.content(kind, 64, 65), q, "1x1")
        runs = [np.diff(np.flatnonzero(np.r_[1, b[1:]])).max(initial=0) for b in blocks]
        assert max(runs) > 16, kind                                                                  # a run of 16 zeros before a coefficient
    blocks, _ = ER.scan_blocks(EF.content("white", 17, 33), 92, "2x2")
    assert not blocks[:, 1:].any() and len({int(b[0]) for b in blocks[[0, 1, 2, 3]]}) == 1      # DC plus end-of-block, differences zero
    data = ER.encode(EF.content("noise", 64, 65), 100, "1x1")
    assert data.count(b"\xff\x00") > 20                                                    # many FF bytes to stuff


def test_the_restatement_writes_pillow_s_bytes(cases):
    for name, _, _, _, ours, pil in cases:
        assert ours == pil, (name, len(ours), len(pil))


def test_the_restatement_writes_pillow_s_bytes_for_a_kitti_frame():
    cases = {n: (a, q, s) for n, a, q, s in EF.frame_cases()}
    assert len(cases) == 9 and {(q, s) for _, q, s in cases.values()} == {(q, s) for q in (10, 92, 100) for s in EF.SAMPLINGS}
    for name in ("texture-375x1242-q10-2x1", "texture-375x1242-q92-2x2", "noise-375x1242-q100-2x2"):
        a, q, s = cases[name]
        assert ER.encode(a, q, s) == EF.pillow(a, q, s), name


def test_every_quality_and_the_dummy_block_heights():
    a = EF.content("texture", 20, 23)
    for q in range(1, 101):
        assert ER.encode(a, q, "2x2") == EF.pillow(a, q, "2x2"), q
    for h in (4, 8, 12, 20, 24, 40):                             # even H that is no multiple of 16: the order of rule 2 decides
        b = EF.content("noise", h, 19)
        for s in EF.SAMPLINGS:
            assert ER.encode(b, 75, s) == EF.pillow(b, 75, s), (h, s)


def test_the_two_arbiters_agree(cases):
    for name, _, _, _, ours, _ in cases:
        with Image.open(io.BytesIO(ours)) as img:
            want = np.asarray(img.convert("RGB"))
        assert np.array_equal(JR.decode_rgb(ours), want), name


def test_uncovered_inputs_are_refused_by_the_restatement():
    ok = np.zeros((4, 4, 3), np.uint8)
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.uint16), np.zeros((0, 4, 3), np.uint8), np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(ValueError):
            ER.encode(bad)
    for q, s in ((0, "2x2"), (101, "2x2"), (92, "4x4"), (92.5, "2x2")):
        with pytest.raises(ValueError):
            ER.encode(ok, q, s)


# ------------------------------------------------------------------------------------------------- the host half, through the library
def test_constants_are_the_library_s(ops):
    assert ops.JPEG_ENC_HEADER_BYTES == ER.HEADER_BYTES == len(ER.headers(5, 7, 92, "2x2"))
    assert ops._lib.ABI_VERSION == 8 and ops._lib.load().fd_abi_version() == 8


def test_quantisation_tables_equal_the_restatement(ops):
    for q in range(1, 101):
        got = ops.jpeg_enc_quant_tables(q)
        assert got.dtype == np.uint16 and np.array_equal(got, ER.quant_tables(q)), q
    for q in (0, 101, -5):
        with pytest.raises(ValueError):
            ops.jpeg_enc_quant_tables(q)


def test_header_bytes_equal_the_restatement_and_pillow(ops, cases):
    for w, h in ((1, 1), (1242, 375), (65535, 65535), (256, 255), (255, 256)):
        for s in EF.SAMPLINGS:
            for q in (1, 50, 92, 100):
                assert ops.jpeg_enc_header(w, h, s, q) == ER.headers(w, h, q, s), (w, h, s, q)
    for name, a, q, s, _, pil in cases[::7]:
        assert ops.jpeg_enc_header(a.shape[1], a.shape[0], s, q) == pil[:ER.HEADER_BYTES], name
    buf = np.full((ER.HEADER_BYTES + 3,), 7, np.uint8)
    ops.jpeg_enc_header(9, 5, "2x1", 75, buf)
    assert buf[:-3].tobytes() == ER.headers(9, 5, 75, "2x1") and buf[-3:].tolist() == [7, 7, 7]
    short = np.full((ER.HEADER_BYTES - 1,), 7, np.uint8)
    with pytest.raises(ValueError):
        ops.jpeg_enc_header(9, 5, "2x1", 75, short)
    assert (short == 7).all()                                    # a buffer that is too small is not touched
    for args in ((0, 5, "2x2", 75), (5, 65536, "2x2", 75), (5, 5, (1, 2), 75), (5, 5, (2, 4), 75), (5, 5, "2x2", 0)):
        with pytest.raises(ValueError):
            ops.jpeg_enc_header(*args)


def test_layout_equals_the_restatement(ops):
    shapes = [(1242, 375, "2x2"), (1, 1, "1x1"), (65, 64, "2x1"), (33, 17, "2x2"), (16, 31, "1x1"), (65535, 3, "2x2"), (9, 7, "2x1")]
    table, sizes = ops.jpeg_enc_layout([(w, h) + ER.SAMPLINGS[s] for w, h, s in shapes])
    want = ER.layout(shapes)
    assert want[0]["blocks"] == 11232                            # a 375x1242 frame at 2x2
    for d, row in zip(table, want):
        assert {k: getattr(d, k) for k in row} == row
    assert sizes.blocks == sum(r["blocks"] for r in want) and sizes.tiles * ER.TILE_BYTES == sum(r["raw_cap"] for r in want) == sizes.raw_bytes
    assert sizes.out_bytes >= sum(r["out_cap"] for r in want) and sizes.out_bytes % 16 == 0
    # the regions of work follow each other without overlap, 16-byte aligned; the streams are the last
    n, b, t = len(shapes), sizes.blocks, sizes.tiles
    offs = [("tab_off", 96 * n), ("coef_off", 1888), ("bits_off", 128 * b), ("pos_off", 4 * b), ("tile_off", 8 * b), ("tilepos_off", 4 * t),
            ("total_off", 8 * t), ("result_off", 16 * n), ("raw_off", 32 * n)]
    at = 0
    for name, need in offs:
        assert getattr(sizes, name) >= at + need and getattr(sizes, name) % 16 == 0, name
        at = getattr(sizes, name)
    assert sizes.work_bytes == sizes.raw_off + sizes.raw_bytes and sizes.result_bytes == 32 * n
    assert [d.raw_off for d in table] == [sizes.raw_off + r["first_tile"] * ER.TILE_BYTES for r in want]
    # the worst case holds for the densest stream there is: noise at quality 100
    blocks, which = ER.scan_blocks(EF.content("noise", 17, 33), 100, "1x1")
    data, nbits = ER.entropy(blocks, which)
    assert nbits <= 8 * ER.BLOCK_BYTES * len(blocks) and len(data) <= 2 * ER.BLOCK_BYTES * len(blocks)
    for bad in ([(0, 4, 2, 2)], [(4, 65536, 2, 2)], [(4, 4, 1, 2)], [(4, 4, 3, 1)], []):
        with pytest.raises(ValueError):
            ops.jpeg_enc_layout(bad)
    with pytest.raises(ValueError):                              # more than 2^31 - 1 blocks in one batch
        ops.jpeg_enc_layout([(65535, 65535, 1, 1)] * 11)
