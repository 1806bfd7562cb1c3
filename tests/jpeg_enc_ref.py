"""The JPEG encoder's rules of include/fdhip.h ("JPEG outputs") restated in numpy: slow, written to be read.  It is the arbiter between
that text and Pillow - tests/test_jpeg_enc_cpu.py holds ``encode`` to the bytes of ``Image.fromarray(rgb).save(f, "JPEG", quality=q,
subsampling=s)`` with no tolerance, and the library's tables, headers, layout and files to this file."""
import numpy as np

from jpeg_ref import NATURAL                                     # zigzag position -> natural (row-major) index

SAMPLINGS = {0: (1, 1), 1: (2, 1), 2: (2, 2), "1x1": (1, 1), "2x1": (2, 1), "2x2": (2, 2)}     # Pillow's subsampling / name -> (h, v) of luma

# Annex K, in the order a DQT segment holds them (zigzag)
QUANT_ZZ = (
    (16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51, 56,
     55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103,
     99),
    (17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99) + (99,) * 49)
DC_BITS = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0))
DC_VALS = (tuple(range(12)), tuple(range(12)))
AC_BITS = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119))
AC_VALS = (
    (1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36,
     51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83,
     84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135,
     136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182,
     183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228,
     229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250),
    (0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98,
     114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74,
     83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133,
     134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180,
     181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227,
     228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250))


def check(rgb, quality, sampling):
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("jpeg_enc_ref: %s %s is not uint8 [H,W,3]" % (rgb.dtype, rgb.shape))
    if not (1 <= rgb.shape[0] <= 65535 and 1 <= rgb.shape[1] <= 65535):
        raise ValueError("jpeg_enc_ref: a side outside 1 .. 65535")
    if not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError("jpeg_enc_ref: quality outside 1 .. 100")
    if sampling not in SAMPLINGS:
        raise ValueError("jpeg_enc_ref: sampling %r" % (sampling,))
    return rgb, int(quality), SAMPLINGS[sampling]


# ------------------------------------------------------------------------------------------------------- rule 1: colour --------
def ycc(rgb):
    """uint8 [H,W,3] -> int32 Y, Cb, Cr planes [H,W]."""
    r, g, b = (rgb[:, :, c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y.astype(np.int32), cb.astype(np.int32), cr.astype(np.int32)


# ------------------------------------------------------------------------------------------------- rule 2: edges and chroma ----
def cdiv(a, b):
    return -(-a // b)


def pad_to(plane, rows, cols):
    """Replicate the last row and the last column out to [rows, cols]."""
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode="edge")


def luma_plane(y):
    h, w = y.shape
    return pad_to(y, 8 * cdiv(h, 8), 8 * cdiv(w, 8))


def chroma_plane(c, hs, vs):
    """One chroma plane at full resolution -> the samples of its own blocks, ceil(W / (8 hs)) x ceil(H / (8 vs)) of them."""
    h, w = c.shape
    if (hs, vs) == (1, 1):
        return luma_plane(c)
    c = pad_to(c, h, 16 * cdiv(w, 16))                           # 1. the last column, at full resolution
    if vs == 2 and h % 2:
        c = pad_to(c, h + 1, c.shape[1])                         # 2. the last row once when H is odd
    cols = c.shape[1] // 2
    if vs == 1:
        bias = np.arange(cols) % 2                               # 0, 1, 0, 1, ...
        d = (c[:, 0::2] + c[:, 1::2] + bias) >> 1
    else:
        bias = 1 + np.arange(cols) % 2                           # 1, 2, 1, 2, ...
        d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
    return pad_to(d, 8 * cdiv(h, 8 * vs), cols)                  # 4. the last DOWNSAMPLED row to whole blocks


# ----------------------------------------------------------------------------------------------------- rule 3: transform -------
def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def fdct_pass(d, first):
    """One pass of the accurate integer forward DCT along the last axis of int32 [..., 8]."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.empty_like(d)
    shift = 13 - 2 if first else 13 + 2
    if first:
        out[..., 0] = (t10 + t11) << 2
        out[..., 4] = (t10 - t11) << 2
    else:
        out[..., 0] = descale(t10 + t11, 2)
        out[..., 4] = descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[..., 2] = descale(z1 + t13 * 6270, shift)
    out[..., 6] = descale(z1 - t12 * 15137, shift)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[..., 7] = descale(t4 + z1 + z3, shift)
    out[..., 5] = descale(t5 + z2 + z4, shift)
    out[..., 3] = descale(t6 + z2 + z3, shift)
    out[..., 1] = descale(t7 + z1 + z4, shift)
    return out


def fdct(blocks):
    """int32 [..., 8, 8] samples minus 128 -> coefficients times 8: rows first, then columns."""
    rows = fdct_pass(blocks.astype(np.int32), True)
    return np.swapaxes(fdct_pass(np.swapaxes(rows, -1, -2), False), -1, -2)


# --------------------------------------------------------------------------------------------------- rule 4: quantisation ------
def quant_tables(quality):
    """-> uint16 [2, 64] in zigzag order (as the DQT segments hold them): luminance, chrominance."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.array(QUANT_ZZ, np.int64) * s + 50) // 100, 1, 255).astype(np.uint16)


def quantise(coef, table_zz):
    """int32 [..., 8, 8] -> int16 [..., 64] in zigzag order."""
    v = coef.reshape(coef.shape[:-2] + (64,))[..., NATURAL].astype(np.int64)
    t = table_zz.astype(np.int64)
    return (np.sign(v) * ((np.abs(v) + 4 * t) // (8 * t))).astype(np.int16)


def component_blocks(plane, table_zz):
    """A padded plane -> int16 [rows of blocks, blocks per row, 64], zigzag."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    blocks = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128
    return quantise(fdct(blocks), table_zz)


# ---------------------------------------------------------------------------------------- rules 5 and 6: the blocks in scan order ---
def scan_blocks(rgb, quality, sampling):
    """-> (int16 [blocks, 64] in scan order, dummy blocks included; the component of each block)."""
    rgb, quality, (hs, vs) = check(rgb, quality, sampling)
    h, w = rgb.shape[:2]
    qt = quant_tables(quality)
    y, cb, cr = ycc(rgb)
    comps = [component_blocks(luma_plane(y), qt[0]), component_blocks(chroma_plane(cb, hs, vs), qt[1]),
             component_blocks(chroma_plane(cr, hs, vs), qt[1])]
    mw, mh = cdiv(w, 8 * hs), cdiv(h, 8 * vs)
    out, which = [], []
    for my in range(mh):
        for mx in range(mw):
            mcu = []                                             # the luma blocks of this MCU, row by row
            for by in range(vs):
                for bx in range(hs):
                    yy, xx = my * vs + by, mx * hs + bx
                    if yy < comps[0].shape[0] and xx < comps[0].shape[1]:
                        blk = comps[0][yy, xx]
                    else:                                        # rule 5: a dummy block
                        blk = np.zeros(64, np.int16)
                        blk[0] = mcu[-1][0]                      # the block to the left, or the LAST block of the row above
                        if yy >= comps[0].shape[0]:
                            blk[0] = mcu[by * hs - 1][0]
                    mcu.append(blk)
            out += mcu + [comps[1][my, mx], comps[2][my, mx]]
            which += [0] * (hs * vs) + [1, 2]
    return np.array(out, np.int16), which


def huffman_codes(bits, vals):
    """BITS and HUFFVAL -> {symbol: (code, length)}."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return codes


def block_tokens(blk, pred, dc, ac):
    """One block's [(value, bits)] tokens."""
    toks = []

    def value(v):                                                # (category, the low bits that travel)
        n = int(abs(v)).bit_length()
        return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)
    n, low = value(int(blk[0]) - pred)
    toks += [dc[n], (low, n)]
    run = 0
    for k in range(1, 64):
        v = int(blk[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            toks.append(ac[0xF0])
            run -= 16
        n, low = value(v)
        toks += [ac[(run << 4) | n], (low, n)]
        run = 0
    if run:
        toks.append(ac[0x00])
    return toks


def entropy(blocks, which):
    """The scan's bytes, stuffed and filled, without EOI; and the stream's length in bits before the fill."""
    dc = [huffman_codes(DC_BITS[t], DC_VALS[t]) for t in (0, 1)]
    ac = [huffman_codes(AC_BITS[t], AC_VALS[t]) for t in (0, 1)]
    pred, raw, acc, held, nbits = [0, 0, 0], bytearray(), 0, 0, 0
    for blk, c in zip(blocks, which):
        t = 0 if c == 0 else 1
        for v, n in block_tokens(blk, pred[c], dc[t], ac[t]):    # most significant bit first
            acc, held, nbits = (acc << n) | v, held + n, nbits + n
        pred[c] = int(blk[0])
        raw += (acc >> (held % 8)).to_bytes(held // 8, "big")    # the whole bytes so far
        acc, held = acc & ((1 << (held % 8)) - 1), held % 8
    if held:
        raw.append((acc << (8 - held)) | ((1 << (8 - held)) - 1))          # the last byte is filled with one-bits
    return bytes(raw).replace(b"\xff", b"\xff\x00"), nbits


# ------------------------------------------------------------------------------------------------------- rule 7: headers -------
def segment(marker, body):
    return bytes([0xFF, marker, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + bytes(body)


def headers(width, height, quality, sampling):
    hs, vs = SAMPLINGS[sampling]
    qt = quant_tables(quality)
    out = b"\xff\xd8" + segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in (0, 1):
        out += segment(0xDB, bytes([t]) + bytes(int(v) for v in qt[t]))
    out += segment(0xC0, bytes([8, height >> 8, height & 255, width >> 8, width & 255, 3, 1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for t in (0, 1):
        out += segment(0xC4, bytes([t]) + bytes(DC_BITS[t]) + bytes(DC_VALS[t]))
        out += segment(0xC4, bytes([0x10 | t]) + bytes(AC_BITS[t]) + bytes(AC_VALS[t]))
    return out + segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


HEADER_BYTES = 623
BLOCK_BYTES = 208            # no block takes more before stuffing: 11 + 11 bits of DC, 63 times 16 + 10 bits of AC, up to 16 bytes
TILE_BYTES = 4096


def layout(shapes):
    """[(width, height, sampling)] -> one dict per image: the MCU grid, the blocks of the scan (dummy ones included), the batch-wide
    index of the first, and the worst-case sizes - the descriptor table of ``fd_jpeg_enc_layout``."""
    rows, block, tile = [], 0, 0
    for w, h, s in shapes:
        hs, vs = SAMPLINGS[s]
        mw, mh = cdiv(w, 8 * hs), cdiv(h, 8 * vs)
        blocks = mw * mh * (hs * vs + 2)
        raw_cap = cdiv(blocks * BLOCK_BYTES + 8, TILE_BYTES) * TILE_BYTES
        rows.append({"width": w, "height": h, "hs": hs, "vs": vs, "mcus_w": mw, "mcus_h": mh, "blocks": blocks, "first_block": block,
                     "first_tile": tile, "raw_cap": raw_cap, "out_cap": HEADER_BYTES + 2 * blocks * BLOCK_BYTES + 2})
        block, tile = block + blocks, tile + raw_cap // TILE_BYTES
    return rows


def encode(rgb, quality=92, sampling="2x2"):
    """The file Pillow writes for ``Image.fromarray(rgb).save(f, "JPEG", quality=quality, subsampling=sampling)``."""
    rgb, quality, _ = check(rgb, quality, sampling)
    blocks, which = scan_blocks(rgb, quality, sampling)
    data, _ = entropy(blocks, which)
    return headers(rgb.shape[1], rgb.shape[0], quality, sampling) + data + b"\xff\xd9"
