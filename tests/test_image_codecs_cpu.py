"""fusiondepth_amd.image_codecs on the host alone: the output grouping against a restatement, host errors that reach the caller, where
the codec names live, and the encoders' shared argument check.  No GPU and no pinned memory."""
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODEC_NAMES = ["decode_jpeg_batch", "decode_png_batch", "encode_png_batch", "encode_jpeg_batch", "JpegBatchJob", "PngBatchJob", "PngEncodeJob",
               "jpeg_probe", "jpeg_entropy_decode", "png_probe", "png_inflate", "png_enc_layout", "png_enc_plan", "png_enc_finish",
               "jpeg_enc_quant_tables", "jpeg_enc_header", "jpeg_enc_layout", "check_png_encoder", "check_jpeg_params", "PNG_BAND_ROWS",
               "PNG_MODES", "PNG_ENC_BLOCK_ROWS", "PNG_ENCODERS", "JPEG_ENC_HEADER_BYTES", "JPEG_SAMPLINGS", "JPEG_SUBSAMPLING", "JPEG_ENCODERS",
               "host_pool", "pil_jpeg", "group_layout"]


def _restated(sizes, elem, out_base=0):
    """The grouping as JpegBatchJob._finish_on and PngBatchJob.layout each wrote it out before they shared one."""
    members = {}
    for i, (h, w) in enumerate(sizes):
        members.setdefault((h, w), []).append(i)
    out_off, at, spans = [0] * len(sizes), out_base, {}
    for (h, w), idx in members.items():
        spans[(h, w)] = at
        for i in idx:
            out_off[i] = at
            at += elem * h * w
        at = (at + 15) // 16 * 16
    return out_off, spans, members, max(at, 16)


A, B, C = (5, 7), (16, 16), (3, 11)                              # 5 * 7 * elem is no multiple of 16 for elem 2 or 3; 16 * 16 * elem is


@pytest.mark.parametrize("elem", [2, 3])
@pytest.mark.parametrize("out_base", [0, 4096])
@pytest.mark.parametrize("sizes", [[A], [A, B, A, C, B], [(1, 1)], [B, B, A, A, C]], ids=["one", "ABACB", "1x1", "BBAAC"])
def test_group_layout_equals_the_restatement(sizes, elem, out_base):
    from fusiondepth_amd.image_codecs import group_layout
    got = group_layout(sizes, elem, out_base)
    assert got == _restated(sizes, elem, out_base)
    out_off, spans, members, out_bytes = got
    assert list(members) == list(dict.fromkeys(sizes)) == list(spans)           # groups in order of first appearance
    assert sorted(i for idx in members.values() for i in idx) == list(range(len(sizes)))
    end = out_base
    for (h, w), idx in members.items():
        assert spans[(h, w)] == end and end % 16 == 0             # every group starts aligned, right behind the one before it
        assert [out_off[i] for i in idx] == [end + k * elem * h * w for k in range(len(idx))]      # its members contiguous, in input order
        end = (end + len(idx) * elem * h * w + 15) // 16 * 16
    assert out_bytes == max(end, 16)


def test_group_layout_of_the_named_cases():
    from fusiondepth_amd.image_codecs import group_layout
    assert group_layout([(1, 1)], 3) == ([0], {(1, 1): 0}, {(1, 1): [0]}, 16)
    assert group_layout([(1, 1)], 2) == ([0], {(1, 1): 0}, {(1, 1): [0]}, 16)
    out_off, spans, members, out_bytes = group_layout([A, B, A, C, B], 3, 32)
    assert members == {A: [0, 2], B: [1, 4], C: [3]}
    assert out_off == [32, 256, 137, 1792, 1024]                  # A's two frames end at 242: B starts at 256, C behind B's 1536 bytes
    assert spans == {A: 32, B: 256, C: 1792} and out_bytes == 1904               # 1792 + 99, rounded up


def _tiny(fmt):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(np.arange(48, dtype=np.uint8).reshape(4, 4, 3)).save(f, fmt)
    return f.getvalue()


@pytest.mark.parametrize("job,fmt", [("JpegBatchJob", "JPEG"), ("PngBatchJob", "PNG")])
def test_a_host_error_is_raised_by_wait_host(tmp_path, job, fmt):
    from fusiondepth_amd import image_codecs
    j = getattr(image_codecs, job)([os.path.join(str(tmp_path), "missing"), _tiny(fmt)])
    with pytest.raises(FileNotFoundError):
        j.wait_host()                                            # the planner returned before it asked for pinned memory


def test_data_ops_loads_neither_the_codecs_nor_pillow():
    code = ("import sys; import fusiondepth_amd.data_ops; "
            "assert 'fusiondepth_amd.image_codecs' not in sys.modules and 'PIL' not in sys.modules, sorted(m for m in sys.modules if 'PIL' in m or 'codec' in m)")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_the_codecs_do_not_import_functional():
    code = "import sys; import fusiondepth_amd.image_codecs; assert 'fusiondepth_amd.functional' not in sys.modules, 'functional imported'"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_the_codec_names_live_in_image_codecs_only():
    from fusiondepth_amd import data_ops, image_codecs
    assert [n for n in CODEC_NAMES if not hasattr(image_codecs, n)] == []
    assert [n for n in CODEC_NAMES + ["jpeg_pool", "_pil_jpeg", "_round16"] if hasattr(data_ops, n)] == []
    assert not hasattr(image_codecs, "jpeg_pool")


def test_round16_is_defined_once():
    found = []
    pkg = os.path.join(ROOT, "fusiondepth_amd")
    for name in sorted(os.listdir(pkg)):
        if name.endswith(".py"):
            with open(os.path.join(pkg, name)) as f:
                found += [(name, m) for m in re.findall(r"^\s*def (_?round16)\b", f.read(), re.M)]
    assert found == [("_lib.py", "round16")]
    from fusiondepth_amd import _lib
    assert [_lib.round16(n) for n in (0, 1, 15, 16, 17, 4096)] == [0, 16, 16, 16, 32, 4096]


@pytest.mark.parametrize("who,tail", [("encode_png_batch", "none of uint8 [H,W,3], uint8 [H,W], uint16 [H,W]"),
                                      ("encode_jpeg_batch", "neither uint8 [H,W,3] nor uint8 [H,W]")])
def test_encoders_refuse_an_image_with_their_own_words(who, tail):
    from fusiondepth_amd import image_codecs
    encode = getattr(image_codecs, who)
    good = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(ValueError, match=re.escape("%s: image 1 is a list, not a tensor or an array" % who)):
        encode([good, [[0]]])
    with pytest.raises(ValueError, match=re.escape("%s: image 0 is float32 [4, 4, 3], %s" % (who, tail))):
        encode([np.zeros((4, 4, 3), np.float32)])
    with pytest.raises(ValueError, match=re.escape("%s: image 1 is torch.uint8 [4, 4, 4], %s" % (who, tail))):
        encode([good, torch.zeros((4, 4, 4), dtype=torch.uint8)])
    with pytest.raises(ValueError, match=re.escape("%s: no images" % who)):
        encode([])
