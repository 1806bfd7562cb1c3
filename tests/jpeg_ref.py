"""The JPEG rules of include/fdhip.h ("baseline JPEG frames") restated in numpy, entropy decoder included: slow, written to be
read.  It is the arbiter between that text and Pillow - tests/test_jpeg_cpu.py holds ``decode_rgb`` to Pillow's bytes with no
tolerance, and the library's coefficients and frames to this file."""
import numpy as np

NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                    54, 47, 55, 62, 63])


class Uncovered(Exception):
    """The stream is a JPEG outside the covered set."""


class Corrupt(Exception):
    """The stream is truncated or damaged."""


# ---------------------------------------------------------------------------------------- rule 1: markers and Huffman decoding -----
def parse(data):
    """Markers up to the first SOS -> a dict (frame, tables, where the entropy-coded data starts).  Raises ``Uncovered`` / ``Corrupt``."""
    if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise Corrupt("no SOI")
    pos, h = 2, {"qt": {}, "dc": {}, "ac": {}, "ri": 0, "jfif": False, "adobe": False, "sof": None}
    while True:
        if pos + 2 > len(data):
            raise Corrupt("ends in the headers")
        if data[pos] != 0xFF:
            raise Corrupt("marker expected")
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        pos += 2
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0xD9, 0x00) or pos + 2 > len(data):
            raise Corrupt("bad marker")
        n = (data[pos] << 8) | data[pos + 1]
        if n < 2 or pos + n > len(data):
            raise Corrupt("segment leaves the file")
        seg = data[pos + 2:pos + n]
        if m == 0xE0 and seg[:5] == b"JFIF\0":
            h["jfif"] = True
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            h["adobe"] = True
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                need = 1 + (128 if pq else 64)
                if pq > 1 or tq > 3 or q + need > len(seg):
                    raise Corrupt("DQT")
                vals = [(seg[q + 1 + 2 * i] << 8) | seg[q + 2 + 2 * i] if pq else seg[q + 1 + i] for i in range(64)]
                table = np.zeros(64, np.uint16)
                table[NATURAL] = vals                              # the file holds zigzag order
                h["qt"][tq] = table
                q += need
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    raise Corrupt("DHT")
                tc, th = seg[q] >> 4, seg[q] & 15
                counts = list(seg[q + 1:q + 17])
                total = sum(counts)
                if tc > 1 or th > 3 or total > 256 or q + 17 + total > len(seg):
                    raise Corrupt("DHT")
                h["ac" if tc else "dc"][th] = huffman_codes(counts, list(seg[q + 17:q + 17 + total]))
                q += 17 + total
        elif m == 0xDD:
            if len(seg) != 2:
                raise Corrupt("DRI")
            h["ri"] = (seg[0] << 8) | seg[1]
        elif 0xC0 <= m <= 0xCF and m not in (0xC8, 0xCC):
            if h["sof"] is not None or len(seg) < 6 or not 1 <= seg[5] <= 4 or len(seg) != 6 + 3 * seg[5]:
                raise Corrupt("SOF")
            h["sof"] = m
            h["bits"], h["height"], h["width"] = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            h["comps"] = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])]
            if h["width"] < 1:
                raise Corrupt("zero width")
        elif m == 0xDC:
            if h["sof"] is None:
                raise Corrupt("DNL before SOF")
            raise Uncovered("DNL")
        elif m == 0xDA:
            if h["sof"] is None:
                raise Corrupt("SOS before SOF")
            if h["sof"] not in (0xC0, 0xC1) or h["bits"] != 8 or h["height"] < 1 or len(h["comps"]) not in (1, 3):
                raise Uncovered("frame type")
            nc = len(h["comps"])
            if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
                raise Corrupt("SOS")
            if seg[0] != nc:
                raise Uncovered("more than one scan")
            h["td"], h["ta"] = [], []
            for c in range(nc):
                if seg[1 + 2 * c] != h["comps"][c][0]:
                    raise Uncovered("component order")
                td, ta = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
                if td not in h["dc"] or ta not in h["ac"] or h["comps"][c][3] not in h["qt"]:
                    raise Corrupt("undefined table")
                h["td"].append(td)
                h["ta"].append(ta)
            if tuple(seg[1 + 2 * nc:4 + 2 * nc]) != (0, 63, 0):
                raise Uncovered("spectral selection")
            if nc == 3:
                ids = [c[0] for c in h["comps"]]
                if not h["jfif"] and (h["adobe"] or ids == [ord("R"), ord("G"), ord("B")]):
                    raise Uncovered("colour space")
                if any(c[1:3] != (1, 1) for c in h["comps"][1:]) or h["comps"][0][1:3] not in ((1, 1), (2, 1), (2, 2)):
                    raise Uncovered("sampling")
                h["hs"], h["vs"] = h["comps"][0][1:3]
            else:
                h["hs"], h["vs"] = 1, 1
            h["scan"] = pos + n
            return h
        pos += n


def huffman_codes(counts, vals):
    """{(length, code): symbol} - the canonical codes of a DHT table."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            if code >= 1 << length:
                raise Corrupt("code lengths overflow")
            table[(length, code)] = vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return table


class _Bits:
    """The entropy-coded segment as bits: FF 00 is a data byte FF, any other marker ends the data."""

    def __init__(self, data, pos):
        self.data, self.pos, self.buf, self.cnt = data, pos, 0, 0

    def bit(self):
        if self.cnt == 0:
            d = self.data
            while self.pos + 1 < len(d) and d[self.pos] == 0xFF and d[self.pos + 1] == 0xFF:
                self.pos += 1
            if self.pos >= len(d) or (d[self.pos] == 0xFF and (self.pos + 1 >= len(d) or d[self.pos + 1] != 0)):
                raise Corrupt("data ends before the last block")
            self.buf = d[self.pos]
            self.pos += 2 if self.buf == 0xFF else 1
            self.cnt = 8
        self.cnt -= 1
        return (self.buf >> self.cnt) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (length, code) in table:
                return table[(length, code)]
        raise Corrupt("undefined Huffman code")

    def restart(self, k):
        self.cnt, d = 0, self.data
        while self.pos + 1 < len(d) and d[self.pos] == 0xFF and d[self.pos + 1] == 0xFF:
            self.pos += 1
        if self.pos + 1 >= len(d) or d[self.pos] != 0xFF or d[self.pos + 1] != 0xD0 + (k & 7):
            raise Corrupt("restart marker")
        self.pos += 2


def _extend(v, s):
    return v - ((1 << s) - 1) if v < (1 << (s - 1)) else v


def block_grids(h):
    """[(blocks_h, blocks_w)] per component: whole MCUs."""
    hs, vs = h["hs"], h["vs"]
    mx, my = -(-h["width"] // (8 * hs)), -(-h["height"] // (8 * vs))
    return [(my * (vs if c == 0 else 1), mx * (hs if c == 0 else 1)) for c in range(len(h["comps"]))]


def entropy_decode(data):
    """-> (header, [int16 [blocks_h, blocks_w, 64] per component, natural order], uint16 [3, 64] tables)."""
    data = bytes(data)
    h = parse(data)
    grids = block_grids(h)
    coefs = [np.zeros((bh, bw, 64), np.int16) for bh, bw in grids]
    br, pred, mcu, rst = _Bits(data, h["scan"]), [0] * len(grids), 0, 0
    my, mx = grids[-1]
    for y in range(my):
        for x in range(mx):
            if h["ri"] and mcu and mcu % h["ri"] == 0:
                br.restart(rst)
                rst, pred = rst + 1, [0] * len(grids)
            mcu += 1
            for c in range(len(grids)):
                ch, cv = (h["hs"], h["vs"]) if c == 0 else (1, 1)
                for vy in range(cv):
                    for hx in range(ch):
                        blk = coefs[c][y * cv + vy, x * ch + hx]
                        t = br.symbol(h["dc"][h["td"][c]])
                        if t > 15:
                            raise Corrupt("DC size")
                        if t:
                            pred[c] = (pred[c] + _extend(br.bits(t), t) + 32768) % 65536 - 32768     # the predictor wraps in int16
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = br.symbol(h["ac"][h["ta"][c]])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                raise Corrupt("coefficient index")
                            blk[NATURAL[k]] = _extend(br.bits(s), s)
                            k += 1
    qt = np.stack([h["qt"][h["comps"][c if c < len(grids) else 0][3]] for c in range(3)])
    return h, coefs, qt


def flat_coefficients(coefs):
    """The layout of fd_jpeg_entropy_decode: component after component, blocks row-major."""
    return np.concatenate([c.reshape(-1) for c in coefs])


# ---------------------------------------------------------------------------------------- rule 2: reconstruction -------------------
def _idct8(x):
    """jidctint.c's 1-D pass along axis 0 of an int32 array [8, ...] (wrapping int32), before the descale."""
    x = [x[i] for i in range(8)]
    I = np.int32
    z1 = (x[2] + x[6]) * I(4433)
    t2, t3 = z1 - x[6] * I(15137), z1 + x[2] * I(6270)
    t0, t1 = (x[0] + x[4]) * I(8192), (x[0] - x[4]) * I(8192)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * I(9633)
    o0, o1, o2, o3 = o0 * I(2446), o1 * I(16819), o2 * I(25172), o3 * I(12299)
    z1, z2 = z1 * I(-7373), z2 * I(-20995)
    z3, z4 = z3 * I(-16069) + z5, z4 * I(-3196) + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    return np.stack([t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3])


def idct_values(coef, table):
    """int16 [bh, bw, 64] and uint16 [64] -> int32 [bh, bw, 8, 8]: the row pass's descaled output, BEFORE the level shift and the limit."""
    bh, bw, _ = coef.shape
    with np.errstate(over="ignore"):
        d = (coef.astype(np.int32) * table.astype(np.int32)).reshape(bh, bw, 8, 8)      # [.., row, column]
        cols = (_idct8(np.moveaxis(d, 2, 0)) + np.int32(1 << 10)) >> 11             # down the columns: axis "row"
        d = np.moveaxis(cols, 0, 2)
        rows = (_idct8(np.moveaxis(d, 3, 0)) + np.int32(1 << 17)) >> 18             # along the rows: axis "column"
        return np.moveaxis(rows, 0, 3)


def idct_plane(coef, table):
    """int16 [bh, bw, 64] and uint16 [64] -> the uint8 plane [8 bh, 8 bw]."""
    bh, bw, _ = coef.shape
    y = idct_values(coef, table)
    i = y & 1023
    s = np.where(i < 128, 128 + i, np.where(i < 512, 255, np.where(i < 896, 0, i - 896)))
    return s.transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw).astype(np.uint8)


def upsample(plane, hs, vs, width, height):
    """A chroma plane (padded) -> int32 [height, width] by libjpeg's fancy upsampling."""
    if hs == 1:
        return plane[:height, :width].astype(np.int32)
    dw, dh = -(-width // 2), (-(-height // 2) if vs == 2 else height)
    C = plane[:dh, :dw].astype(np.int32)
    if dw <= 2:
        out = np.repeat(C, 2, axis=1)
        return (np.repeat(out, 2, axis=0) if vs == 2 else out)[:height, :width]
    if vs == 1:
        rows = [C]
    else:
        above = np.concatenate([C[:1], C[:-1]])                    # far row of the even output rows, clamped to the real rows
        below = np.concatenate([C[1:], C[-1:]])
        rows = [3 * C + above, 3 * C + below]
    outs = []
    for s in rows:
        prev = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        nxt = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        if vs == 1:
            even, odd = (3 * s + prev + 1) >> 2, (3 * s + nxt + 2) >> 2
            even[:, 0], odd[:, -1] = s[:, 0], s[:, -1]
        else:
            even, odd = (3 * s + prev + 8) >> 4, (3 * s + nxt + 7) >> 4
            even[:, 0], odd[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
        outs.append(np.stack([even, odd], axis=2).reshape(dh, 2 * dw))
    out = outs[0] if vs == 1 else np.stack(outs, axis=1).reshape(2 * dh, 2 * dw)
    return out[:height, :width]


def reconstruct(h, coefs, qt):
    """Rule 2 -> uint8 [H, W, 3]."""
    W, H = h["width"], h["height"]
    planes = [idct_plane(c, qt[i]) for i, c in enumerate(coefs)]
    Y = planes[0][:H, :W].astype(np.int32)
    if len(planes) == 1:
        return np.repeat(Y[:, :, None], 3, axis=2).astype(np.uint8)
    cb = upsample(planes[1], h["hs"], h["vs"], W, H) - 128
    cr = upsample(planes[2], h["hs"], h["vs"], W, H) - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], axis=2), 0, 255).astype(np.uint8)


def decode_rgb(data):
    return reconstruct(*entropy_decode(data))
