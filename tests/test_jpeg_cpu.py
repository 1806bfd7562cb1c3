"""The JPEG rules without a GPU: the host entropy decoder (fd_jpeg_probe / fd_jpeg_entropy_decode) against the numpy restatement
(tests/jpeg_ref.py), and the restatement against Pillow on every byte - which pins the rules of include/fdhip.h on any machine."""
import numpy as np
import pytest

pytest.importorskip("PIL")

import jpeg_fixtures as JF
import jpeg_ref as JR

GUARD = 4096


@pytest.fixture(scope="module")
def ops():
    from fusiondepth_amd import build
    build.build(verbose=False)
    from fusiondepth_amd import image_codecs
    return image_codecs


@pytest.fixture(scope="module")
def restated():
    """name -> (header, coefficients, tables) of the restatement, computed once."""
    return {name: JR.entropy_decode(data) for name, data in JF.fixtures()}


def decode_guarded(ops, data, cap):
    """fd_jpeg_entropy_decode with ``cap`` coefficients and a guard region behind them -> (status, info, coef, qt); asserts the guard."""
    buf = np.full(cap + GUARD, 0x5A5A, np.int16)
    qt = np.full(192 + 64, 0xA5A5, np.uint16)
    st, info = ops.jpeg_entropy_decode(data, buf[:cap], qt[:192])
    assert (buf[cap:] == 0x5A5A).all(), "write past coef_cap"
    assert (qt[192:] == 0xA5A5).all(), "write past the tables"
    return st, info, buf[:cap], qt[:192]


def test_every_fixture_probes_as_covered(ops):
    assert len(JF.fixtures()) > 100
    for name, data in JF.fixtures():
        st, info = ops.jpeg_probe(data)
        want = JF.pillow_rgb(data).shape
        assert st == 0 and info.covered == 1, name
        assert (info.height, info.width) == want[:2], name
        assert info.components == (1 if "grey" in name else 3), name
        hs, vs = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "grey": (1, 1)}[name.split("-")[1]]
        assert (info.h_samp, info.v_samp) == (hs, vs), name
        mx, my = -(-info.width // (8 * hs)), -(-info.height // (8 * vs))
        assert list(info.blocks_w)[:info.components] == [mx * hs, mx, mx][:info.components], name
        assert list(info.blocks_h)[:info.components] == [my * vs, my, my][:info.components], name
        assert info.coef_count == 64 * sum(info.blocks_w[c] * info.blocks_h[c] for c in range(info.components)), name
        assert (info.restart_interval > 0) == ("restart" in name), name


def test_entropy_decoder_equals_the_restatement(ops, restated):
    for name, data in JF.fixtures():
        h, coefs, qt = restated[name]
        want = JR.flat_coefficients(coefs)
        st, info, coef, got_qt = decode_guarded(ops, data, want.size)
        assert st == 0, (name, ops._lib.last_error())
        assert info.coef_count == want.size, name
        assert np.array_equal(coef, want), name
        assert np.array_equal(got_qt.reshape(3, 64), qt), name
        st, _, _, _ = decode_guarded(ops, data, want.size - 1)
        assert st == 6, name                                     # FD_JPEG_CAPACITY


def test_restatement_equals_pillow_on_every_byte(restated):
    for name, data in JF.fixtures():
        got = JR.reconstruct(*restated[name])
        want = JF.pillow_rgb(data)
        assert got.shape == want.shape and got.dtype == want.dtype, name
        assert np.array_equal(got, want), (name, int(np.abs(got.astype(int) - want).max()))


def test_checkerboard_reaches_the_range_limit(restated):
    """the quality-100 checkerboards are there to saturate: some sample must leave 0 .. 255 before the limit"""
    below = above = 0
    for name, _ in JF.fixtures():
        if "checker" in name:
            h, coefs, qt = restated[name]
            v = JR.idct_values(coefs[0], qt[0]) + 128             # the sample before the limit
            below, above = below + int((v < 0).sum()), above + int((v > 255).sum())
    assert below > 0 and above > 0, (below, above)


def test_uncovered_streams_are_reported_not_guessed(ops):
    for name, data in JF.uncovered():
        st, info = ops.jpeg_probe(data)
        assert st == 0 and info.covered == 0, name
        assert (info.height, info.width) == (31, 33), name
        assert "not covered" in ops._lib.last_error(), name
        st, info, coef, _ = decode_guarded(ops, data, 64 * 1024)
        assert st == 3 and info.covered == 0, name               # FD_JPEG_UNCOVERED
        assert (coef == 0x5A5A).all(), name
        with pytest.raises(JR.Uncovered):
            JR.entropy_decode(data)


def test_prefixes_and_corruptions_return_a_status(ops):
    name, data = next((n, d) for n, d in JF.fixtures() if n == "33x31-420-noise-q92")
    st, info = ops.jpeg_probe(data)
    cap = int(info.coef_count)
    scan = JR.parse(data)["scan"]
    for n in range(len(data)):
        part = data[:n]
        pst, pinfo = ops.jpeg_probe(part)
        st, _, _, _ = decode_guarded(ops, part, cap)
        assert 0 <= pst <= 6 and 0 <= st <= 6, n
        if n < scan:
            assert pst != 0 and pinfo.covered == 0, n
        if n <= len(data) - 3:                                   # at least one byte of entropy-coded data is missing
            assert st != 0 and ops._lib.last_error(), n
    assert decode_guarded(ops, data, cap)[0] == 0
    restart = next(d for n, d in JF.fixtures() if n == "50x40-422-restart3")
    statuses = set()
    for src in (data, restart):
        c = int(ops.jpeg_probe(src)[1].coef_count)
        for bad in JF.corruptions(src):
            pst, _ = ops.jpeg_probe(bad)
            st, info, _, _ = decode_guarded(ops, bad, c)
            assert 0 <= pst <= 6 and 0 <= st <= 6
            assert st != 0 or info.covered == 1
            statuses.add(st)
    assert statuses - {0}, "no corruption was detected at all"


def test_image_decoder_flag_and_loader_argument(tmp_path):
    """--image_decoder joins the parsed extras only where it is given (the default is 'pil'); decoder= is checked by the loader."""
    from fusiondepth_amd import complete as C
    from fusiondepth_amd import refine as R
    from fusiondepth_amd import train as T
    from fusiondepth_amd.datasets import KITTIRAWBatches, KITTIStereoBatches, pil_loader
    assert "image_decoder" not in T.split_off_extra([])[0] and "image_decoder" not in C.split_off_extra([])[0]
    for mod in (T, R, C):
        extra, rest = mod.split_off_extra(["--image_decoder", "device", "--png"])
        assert extra["image_decoder"] == "device" and rest == ["--png"]
        assert mod.split_off_extra(["--image_decoder=pil"])[0]["image_decoder"] == "pil"
        with pytest.raises(ValueError, match="image_decoder"):
            mod.split_off_extra(["--image_decoder", "gpu"])
    root = str(tmp_path)
    for cls in (KITTIRAWBatches, KITTIStereoBatches):
        assert cls(root, [], 64, 96, [0], 4).decoder == "pil"
        b = cls(root, [], 64, 96, [0], 4, decoder="device")
        assert b.decoder == "device" and b.decode_stats == {"device": 0, "fallback": 0}
        assert cls(root, [], 64, 96, [0], 4, img_ext=".png", decoder="device").decoder == "pil"
        with pytest.raises(ValueError, match="loader="):
            cls(root, [], 64, 96, [0], 4, decoder="device", loader=pil_loader)
        with pytest.raises(ValueError, match="decoder"):
            cls(root, [], 64, 96, [0], 4, decoder="gpu")
