"""The PNG encoder without a GPU: the restated stream (tests/png_enc_ref.py) decodes to its input in Pillow, zlib and this project's
own host decoder, and the host half of the encoder (fd_png_enc_layout / _plan / _finish, csrc/png_deflate.h) equals the restatement
field for field - which pins the stream of include/fdhip.h ("PNG outputs") on any machine."""
import ctypes
import io
import struct
import zlib

import numpy as np
import pytest

pytest.importorskip("PIL")
from PIL import Image

import png_enc_fixtures as EF
import png_enc_ref as ER
import png_ref as PR

MODES = {"rgb8": "RGB", "g8": "L", "g16": "I;16"}


@pytest.fixture(scope="module")
def ops():
    from fusiondepth_amd import build
    build.build(verbose=False)
    from fusiondepth_amd import image_codecs
    return image_codecs


def test_constants_are_the_library_s(ops):
    assert ops.PNG_ENC_BLOCK_ROWS == ER.BLOCK_ROWS == ops._lib.load().fd_png_enc_block_rows()
    assert ops._lib.ABI_VERSION == 8 and ops._lib.load().fd_abi_version() == 8


def test_fixtures_cover_what_they_claim():
    names = [n for n, _ in EF.images()]
    assert len(names) == len(set(names)) == 3 * (4 * 36 + 6)
    for kind in EF.KINDS:
        for ft, name in enumerate(EF.FILTER_NAMES):
            a = dict(EF.images())["%s-9x85-wins-%s" % (kind, name)]
            _, got = ER.filter_rows(a)
            # on a frame's first row Up is None and Paeth is Sub, byte for byte, and the tie goes to the lower type: no image can make
            # Up or Paeth win row 0
            first = {2: 0, 4: 1}.get(ft, ft)
            assert got.tolist() == [first] + [ft] * 8, (kind, name, got)
        cost = ER.filter_costs(dict(EF.images())["%s-5x7-tie" % kind])
        _, got = ER.filter_rows(dict(EF.images())["%s-5x7-tie" % kind])
        assert (cost[2, 1:] == cost[4, 1:]).all() and (cost[2, 1:] == cost[:, 1:].min(axis=0)).all() and got[1:].tolist() == [2] * 4, kind
    zero = ER.filter_costs(np.zeros((3, 5), np.uint8))
    assert (zero == 0).all() and ER.filter_rows(np.zeros((3, 5), np.uint8))[1].tolist() == [0, 0, 0]     # a five-way tie


def test_restated_files_decode_to_their_input(ops):
    enc = EF.encoded()
    for name, a in EF.images():
        data = enc[name]
        with Image.open(io.BytesIO(data)) as img:
            assert img.mode == MODES[name.split("-")[0]], (name, img.mode)
            got = np.asarray(img)
        assert got.shape == a.shape and np.array_equal(got, a), name
        cs = PR.chunks(data)
        assert [t for t, _ in cs] == [b"IHDR", b"IDAT", b"IEND"], name                 # ONE IDAT, no ancillary chunks
        h, w, bpp, _, _ = ER.kind_of(a)
        raw = zlib.decompress(cs[1][1])
        assert cs[1][1][:2] == b"\x78\x01" and len(raw) == h * (1 + w * bpp), name
        st, info = ops.png_probe(data)
        assert st == 0 and info.covered == 1 and (info.width, info.height, info.bpp) == (w, h, bpp), (name, ops._lib.last_error())
        dst = np.zeros(info.raw_bytes, np.uint8)
        st, _ = ops.png_inflate(data, dst)
        assert st == 0, (name, ops._lib.last_error())
        assert dst.tobytes() == raw, name
        head = PR.header(data)
        recon = PR.unfilter(dst.reshape(h, 1 + w * bpp), bpp)
        back = PR.gray16(head, recon) if bpp == 2 else recon.reshape(a.shape)
        assert np.array_equal(back, a), name


def test_tokens_follow_the_run_rule():
    """A run of L equal bytes: one literal, (L - 1) // 258 matches of 258, then (L - 1) % 258 as a match or as up to two literals."""
    for L, want in ((1, [7]), (2, [7, 7]), (3, [7, 7, 7]), (4, [7, 257]), (259, [7, 285]), (260, [7, 285, 7]), (261, [7, 285, 7, 7]),
                    (262, [7, 285, 257]), (517, [7, 285, 285]), (518, [7, 285, 285, 7]), (258, [7, 284])):
        sym, ebits, ev, match = ER.tokens(np.full((1, L), 7, np.uint8))
        assert sym.tolist() == want, (L, sym)
        assert match.tolist() == [s > 256 for s in want], L
    sym, ebits, ev, _ = ER.tokens(np.full((1, 258), 7, np.uint8))
    assert (sym[1], ebits[1], ev[1]) == (284, 5, 30)                                   # 257 = 227 + 30
    sym, _, _, _ = ER.tokens(np.full((2, 5), 7, np.uint8))
    assert sym.tolist() == [7, 258, 7, 258]                                            # runs never cross a scanline


def _c_plan(ops, frames, hist, adler):
    """fd_png_enc_layout + fd_png_enc_plan on the same inputs as ``ER.plan`` -> (blocks as dicts, files as dicts)."""
    table, sizes = ops.png_enc_layout(frames)
    stats = np.zeros(sizes.stat_bytes // 4, np.uint32)
    stats[:hist.size] = hist.reshape(-1)
    stats[sizes.blocks * ER.HIST:sizes.blocks * ER.HIST + adler.size] = adler.reshape(-1)
    for d in table:
        d.src = 1                                                                     # never read on the host
    blocks, total = ops.png_enc_plan(table, len(frames), stats)
    out = []
    for b in blocks:
        words = list(b.header)
        header = sum(w << (32 * k) for k, w in enumerate(words))
        out.append({"len": list(b.len)[:286], "code": list(b.code)[:286], "dist_len": b.dist_len, "header": header,
                    "header_bits": b.header_bits, "bits": b.bits, "bit_off": b.bit_off})
        assert list(b.len)[286:] == [0, 0] and list(b.code)[286:] == [0, 0]
    files = [{"adler": d.adler, "off": d.out_off, "size": d.out_bytes, "stream_bits": d.stream_bits} for d in list(table)[:len(frames)]]
    assert total == sum(f["size"] for f in files)
    return out, files


def _same_plan(ops, frames, hist, adler, what):
    want_b, want_f = ER.plan(frames, hist, adler)
    got_b, got_f = _c_plan(ops, frames, hist, adler)
    assert len(got_b) == len(want_b)
    for k, (g, w) in enumerate(zip(got_b, want_b)):
        for field in ("len", "code", "dist_len", "header_bits", "header", "bits", "bit_off"):
            assert g[field] == w[field], (what, "block %d" % k, field)
    assert got_f == want_f, what
    return want_b


def test_plan_equals_the_restatement_on_the_fixtures(ops):
    items = EF.images()
    for part in (items[k::7] for k in range(7)):                                       # batches of mixed sizes and kinds
        frames, hist, adler = [], [], []
        for name, a in part:
            h, w, bpp, _, _ = ER.kind_of(a)
            filtered, _ = ER.filter_rows(a)
            frames.append((w, h, bpp))
            hist.append(ER.histograms(filtered))
            adler.append(ER.adler_rows(filtered))
        _same_plan(ops, frames, np.concatenate(hist), np.concatenate(adler), part[0][0])


def _hand_made():
    """{name: one block's histogram} - the cases of the Huffman and header rules that images do not reach."""
    out = {}
    h = np.zeros(ER.HIST, np.uint32)
    h[65] = 9
    out["one symbol plus end-of-block"] = h
    h = np.zeros(ER.HIST, np.uint32)
    h[:286] = 5
    h[286] = 5 * 29
    out["all 286 symbols equal"] = h
    h = np.zeros(ER.HIST, np.uint32)
    fib = [1, 1]
    while len(fib) < 44:
        fib.append(fib[-1] + fib[-2])
    h[10:10 + len(fib)] = fib                                                          # the last is 701 408 733 < 2^32
    out["fibonacci"] = h
    h = np.zeros(ER.HIST, np.uint32)
    for s in range(200):
        h[s] = 1 << ((s * 7) % 10 * 2)
    out["deep code-length code"] = h
    h = np.zeros(ER.HIST, np.uint32)
    h[0], h[285], h[286] = 3, 40, 40
    out["matches of length 258 only"] = h
    h = np.zeros(ER.HIST, np.uint32)
    h[255] = 1
    out["no matches"] = h
    return out


def test_plan_equals_the_restatement_on_hand_made_histograms(ops):
    cases = _hand_made()
    counts, _ = ER.block_counts(cases["fibonacci"])
    assert max(ER.code_lengths(counts, 10 ** 9)) > 15                                  # the unrestricted tree is too deep
    counts, matches = ER.block_counts(cases["deep code-length code"])
    _, cl_counts, _ = ER.code_length_counts(ER.code_lengths(counts, 15), matches)
    assert max(ER.code_lengths(cl_counts, 10 ** 9)) > 7                                # and so is this code-length code's
    adler = np.array([[3, 5]], np.uint32)
    for name, hist in cases.items():
        blk = _same_plan(ops, [(17, 1, 1)], hist[None], adler, name)[0]
        lens = blk["len"]
        assert max(lens) <= 15 and sum(2.0 ** -l for l in lens if l) == 1.0, name      # a complete code
        assert blk["dist_len"] == (1 if hist[286] else 0), name
    # several of them as the blocks of ONE frame: offsets add up, BFINAL on the last only
    hist = np.stack(list(cases.values()))
    rows = 64 * (len(cases) - 1) + 1
    adler = np.stack([np.arange(rows) * 37 % 65521, np.arange(rows) * 991 % 65521], axis=1).astype(np.uint32)
    blocks = _same_plan(ops, [(5, rows, 3)], hist, adler, "one frame")
    assert [b["header"] & 1 for b in blocks] == [0] * (len(cases) - 1) + [1]
    assert all((b["header"] >> 1) & 3 == 2 for b in blocks)


def test_adler_pairs_combine_to_zlib_s(ops):
    a = dict(EF.images())["g16-65x87-random"]
    filtered, _ = ER.filter_rows(a)
    _, files = _c_plan(ops, [(87, 65, 2)], ER.histograms(filtered), ER.adler_rows(filtered))
    assert files[0]["adler"] == zlib.adler32(filtered.tobytes())


def test_layout_refuses_what_is_not_covered(ops):
    for shape in ((0, 4, 1), (4, 0, 1), (4, 4, 4), (4, 4, 0), (65536, 1, 1), (65535, 65535, 3)):
        with pytest.raises(ValueError):
            ops.png_enc_layout([(3, 3, 1), shape])
    with pytest.raises(ValueError):
        ops.png_enc_layout([])
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.uint16), np.zeros((4,), np.uint8),
                np.zeros((0, 4), np.uint8), "a.png"):
        with pytest.raises(ValueError):                                                # before the GPU is touched: this test has none
            ops.encode_png_batch([np.zeros((2, 2), np.uint8), bad])
    with pytest.raises(ValueError):
        ops.encode_png_batch([])


def test_finish_equals_zlib_crc32(ops):
    enc = EF.encoded()
    names = ["rgb8-1x1-zero", "g16-129x259-random", "g8-1x600-ramp", "rgb8-65x87-ramp"]
    table = (ops._lib.PngEncDesc * len(names))()
    at, buf = 5, bytearray(b"\xaa" * 5)                                                # files at odd offsets
    for d, name in zip(table, names):
        data = bytearray(enc[name])
        zlen = len(data) - 57
        for off in (29, 41 + zlen, len(data) - 4):                                     # what the device leaves: no CRC
            data[off:off + 4] = b"\0\0\0\0"
        d.out_off, d.out_bytes = at, len(data)
        buf += data
        at += len(data)
    buf += b"\xaa" * 3
    flat = np.frombuffer(buf, np.uint8).copy()
    for d in table:
        ops.png_enc_finish(flat, d)
    assert bytes(flat[:5]) == b"\xaa" * 5 and bytes(flat[-3:]) == b"\xaa" * 3
    for d, name in zip(table, names):
        assert bytes(flat[d.out_off:d.out_off + d.out_bytes]) == enc[name], name
    bad = ops._lib.PngEncDesc()
    bad.out_off, bad.out_bytes = flat.size - 10, 100
    with pytest.raises(RuntimeError):
        ops.png_enc_finish(flat, bad)


def test_file_size_is_known_from_the_plan():
    a = dict(EF.images())["rgb8-129x87-ramp"]
    h, w, bpp, _, _ = ER.kind_of(a)
    filtered, _ = ER.filter_rows(a)
    blocks, files = ER.plan([(w, h, bpp)], ER.histograms(filtered), ER.adler_rows(filtered))
    assert len(blocks) == 3 and files[0]["size"] == len(EF.encoded()["rgb8-129x87-ramp"])
    assert struct.unpack(">I", EF.encoded()["rgb8-129x87-ramp"][33:37])[0] == files[0]["size"] - 57
    assert ctypes.sizeof(ctypes.c_long) == 8
