"""The PNG rules without a GPU: the host inflate (fd_png_probe / fd_png_inflate) against ``zlib.decompress`` of the joined IDAT data,
and the numpy restatement of the chunk walk and the five filters (tests/png_ref.py) against Pillow on every byte - which pins the
rules of include/fdhip.h on any machine."""
import zlib

import numpy as np
import pytest

pytest.importorskip("PIL")

import png_fixtures as PF
import png_ref as PR

GUARD = 4096


@pytest.fixture(scope="module")
def ops():
    from fusiondepth_amd import build
    build.build(verbose=False)
    from fusiondepth_amd import image_codecs
    return image_codecs


def inflate_guarded(ops, data, cap):
    """fd_png_inflate with ``cap`` bytes of room and a guard region behind them -> (status, info, dst); asserts the guard."""
    buf = np.full(cap + GUARD, 0x5A, np.uint8)
    st, info = ops.png_inflate(data, buf[:cap])
    assert (buf[cap:] == 0x5A).all(), "write past dst_cap"
    return st, info, buf[:cap]


def test_band_constant_is_the_library_s(ops):
    assert ops.PNG_BAND_ROWS == ops._lib.load().fd_png_band_rows()


def test_restatement_equals_pillow_on_every_byte():
    assert len(PF.fixtures()) > 100
    for name, data in PF.fixtures():
        got, want = PR.decode(data), PF.pillow(data)
        assert got.shape == want.shape and got.dtype == want.dtype, (name, got.dtype, want.dtype)
        assert np.array_equal(got, want), name
        if name.startswith("g8"):
            assert want.ndim == 3 and (want[:, :, 0] == want[:, :, 2]).all(), name


def test_every_fixture_probes_as_covered(ops):
    for name, data in PF.fixtures():
        st, info = ops.png_probe(data)
        h = PR.header(data)
        colour, depth, bpp = PF.FORMATS[name.split("-")[0]]
        assert st == 0 and info.covered == 1, (name, ops._lib.last_error())
        assert (info.width, info.height, info.bit_depth, info.colour_type, info.interlace) == (h["width"], h["height"], depth, colour, 0), name
        assert (info.bpp, info.row_bytes, info.raw_bytes) == (bpp, h["width"] * bpp, h["height"] * (1 + h["width"] * bpp)), name


def test_uncovered_files_are_reported_not_guessed(ops):
    names = [n for n, _ in PF.uncovered()]
    assert names == ["palette", "rgba", "interlaced", "1bit", "rgb16", "grey-trns"]
    for name, data in PF.uncovered():
        st, info = ops.png_probe(data)
        h = PR.header(data)
        assert st == 0 and info.covered == 0, name
        assert (info.width, info.height) == (h["width"], h["height"]), name
        assert (info.bpp, info.row_bytes, info.raw_bytes) == (0, 0, 0), name
        assert "not covered" in ops._lib.last_error(), name
        st, info, dst = inflate_guarded(ops, data, 4096)
        assert st == 3 and info.covered == 0, name               # FD_PNG_UNCOVERED
        assert (dst == 0x5A).all(), name
        assert PF.pillow_rgb(data).shape == (h["height"], h["width"], 3), name      # a valid file all the same
    assert ops.png_probe(b"\xff\xd8\xff\xe0 not a png at all, thirty-three bytes")[0] == 2                    # FD_PNG_NOT_PNG


def test_inflate_equals_zlib_byte_for_byte(ops):
    for name, data in PF.fixtures():
        want = np.frombuffer(zlib.decompress(PR.idat(data)), np.uint8)
        st, info, dst = inflate_guarded(ops, data, want.size)
        assert st == 0, (name, ops._lib.last_error())
        assert info.raw_bytes == want.size and np.array_equal(dst, want), name
        st, _, dst = inflate_guarded(ops, data, want.size - 1)
        assert st == 6 and (dst == 0x5A).all(), name             # FD_PNG_CAPACITY, and nothing written
        st, _, dst = inflate_guarded(ops, data, want.size + 100)
        assert st == 0 and np.array_equal(dst[:want.size], want) and (dst[want.size:] == 0x5A).all(), name


def test_prefixes_and_corruptions_return_a_status(ops):
    by_name = dict(PF.fixtures())
    statuses = set()
    for name in ("rgb8-idat-empty", "g16-texture-filter4"):
        data = by_name[name]
        cap = int(ops.png_probe(data)[1].raw_bytes)
        stream_end = data.rindex(b"IDAT") + 4 + len(PR.chunks(data)[-2][1])        # the last byte of stream data
        for n in range(len(data)):
            part = data[:n]
            pst, pinfo = ops.png_probe(part)
            st, _, _ = inflate_guarded(ops, part, cap)
            assert 0 <= pst <= 6 and 1 <= st <= 6, (name, n)      # only the whole file returns 0
            assert ops._lib.last_error(), (name, n)
            if n < 33:
                assert pst != 0 and pinfo.covered == 0, (name, n)
            if n < stream_end:
                assert st == 4, (name, n, st)                    # FD_PNG_TRUNCATED: stream data is missing
        assert inflate_guarded(ops, data, cap)[0] == 0
        for bad in PF.corruptions(data):
            pst, _ = ops.png_probe(bad)
            st, info, _ = inflate_guarded(ops, bad, cap)
            assert 0 <= pst <= 6 and 0 <= st <= 6
            assert st != 0 or info.covered == 1
            statuses.add(st)
    assert 5 in statuses, "no corruption was detected at all"


def test_damaged_streams_have_the_documented_status(ops):
    """one hand-made case per rule of include/fdhip.h that a random corruption seldom meets"""
    data = dict(PF.fixtures())["rgb8-strategy-default"]
    h, rows = PR.scanlines(data)
    raw = rows.tobytes()

    def status(stream, w=50, hh=40):
        st, _, _ = inflate_guarded(ops, PF.wrap(w, hh, 2, 8, stream), len(raw))
        return st, ops._lib.last_error()

    good = PF.deflate(raw)
    assert status(good)[0] == 0
    assert status(bytes([0x79]) + good[1:]) == (5, "png: zlib header: not deflate with a window of at most 32 KiB")
    assert status(bytes([good[0], good[1] ^ 1]) + good[2:])[0] == 5                  # FCHECK
    assert status(bytes([0x78, 0xBB]) + good[2:])[1] == "png: zlib header: preset dictionary"
    assert status(good[:-1] + bytes([good[-1] ^ 1])) == (5, "png: the scanlines fail the stream's Adler-32")
    assert status(PF.deflate(raw + b"\x00"))[0] == 5              # more than raw_bytes
    assert status(PF.deflate(raw[:-1]))[0] == 4                   # less
    bad = bytearray(raw)
    bad[151 * 3] = 5
    assert status(PF.deflate(bytes(bad))) == (5, "png: a scanline's filter type is above 4")
    b = PF.Bits()                                                # a distance before the first byte: fixed block, literal 0, match (3, 2)
    b.put(0x78, 8)
    b.put(0x01, 8)
    b.put(1, 1)
    b.put(1, 2)
    b.code(0x30, 8)
    b.code(1, 7)
    b.code(1, 5)
    b.code(0, 7)
    b.align()
    assert status(bytes(b.out) + b"\0\0\0\0") == (5, "png: a distance reaches before the first byte written")
    # a one-code distance tree is a code; its unused pattern is an undefined symbol
    far = dict(PF.fixtures())["g8-far-match-one-code-tree"]
    stream = bytearray(PR.idat(far))
    want = zlib.decompress(bytes(stream))
    at = len(stream) - 4 - 13                                    # inside the dynamic block's symbols
    hits = set()
    for i in range(at, len(stream) - 4):
        for bit in range(8):
            s = bytearray(stream)
            s[i] ^= 1 << bit
            st, _, _ = inflate_guarded(ops, PF.wrap(1023, 33, 0, 8, bytes(s)), len(want))
            hits.add((st, ops._lib.last_error()))
    assert (5, "png: undefined distance code") in hits, hits


def test_the_fixtures_hold_what_they_are_there_for():
    """all five filter types, all three block types, multi-IDAT files, a zero-length IDAT, length 258, distances 1 and 32768"""
    filters, blocks, multi, empty = set(), set(), 0, 0
    for name, data in PF.fixtures():
        h, rows = PR.scanlines(data)
        filters |= set(int(v) for v in rows[:, 0])
        payloads = [p for t, p in PR.chunks(data) if t == b"IDAT"]
        multi += len(payloads) > 1
        empty += any(len(p) == 0 for p in payloads)
        blocks.add((PR.idat(data)[2] >> 1) & 3)                  # the first block's type
    assert filters == {0, 1, 2, 3, 4}
    assert blocks == {0, 1, 2}
    assert multi >= 4 and empty >= 1
    by_name = dict(PF.fixtures())
    first_rows = {(n.split("-")[0], int(PR.scanlines(d)[1][0, 0])) for n, d in PF.fixtures()}
    assert first_rows >= {(f, t) for f in PF.FORMATS for t in range(5)}
    sync = PR.idat(by_name["rgb8-syncflush"])
    assert sync.count(b"\x00\x00\xff\xff") >= 5                  # the empty stored blocks Z_SYNC_FLUSH leaves
    heights = {PR.header(d)["height"] for n, d in PF.fixtures() if "-band-" in n}
    from fusiondepth_amd import image_codecs
    assert heights == {image_codecs.PNG_BAND_ROWS - 1, image_codecs.PNG_BAND_ROWS, image_codecs.PNG_BAND_ROWS + 1}


def test_png_decoder_flag_and_loader_argument(tmp_path):
    """--png_decoder joins the parsed extras only where it is given (the default is 'pil'); png_decoder= is checked by the loader."""
    from fusiondepth_amd import complete as C
    from fusiondepth_amd import refine as R
    from fusiondepth_amd import train as T
    from fusiondepth_amd.datasets import KITTIRAWBatches, KITTIRefinerBatches, KITTIStereoBatches, pil_loader
    from fusiondepth_amd.detection import KITTIDetecBatches
    for mod in (T, R, C):
        assert "png_decoder" not in mod.split_off_extra([])[0]
        assert "png_decoder" not in mod.split_off_extra(["--image_decoder", "device"])[0]
        extra, rest = mod.split_off_extra(["--png_decoder", "device", "--png"])
        assert extra["png_decoder"] == "device" and rest == ["--png"] and "image_decoder" not in extra
        assert mod.split_off_extra(["--png_decoder=pil"])[0]["png_decoder"] == "pil"
        with pytest.raises(ValueError, match="png_decoder"):
            mod.split_off_extra(["--png_decoder", "gpu"])
    root = str(tmp_path)
    for cls in (KITTIRAWBatches, KITTIStereoBatches, KITTIRefinerBatches, KITTIDetecBatches):
        assert cls(root, [], 64, 96, [0], 4, img_ext=".png").png_decoder == "pil"
        b = cls(root, [], 64, 96, [0], 4, img_ext=".png", png_decoder="device")
        assert b.png_decoder == "device" and b.decoder == "pil" and b.decode_stats == {"device": 0, "fallback": 0}
        assert cls(root, [], 64, 96, [0], 4, img_ext=".jpg", png_decoder="device").png_decoder == "pil"       # it speaks for PNG trees
        with pytest.raises(ValueError, match="loader="):
            cls(root, [], 64, 96, [0], 4, img_ext=".png", png_decoder="device", loader=pil_loader)
        with pytest.raises(ValueError, match="png_decoder"):
            cls(root, [], 64, 96, [0], 4, img_ext=".png", png_decoder="gpu")
