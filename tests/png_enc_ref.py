"""numpy / Python restatement of the PNG encoder's stream (include/fdhip.h, "PNG outputs") - what the host plan
(csrc/png_deflate.h) and the three launches of csrc/png_enc.hip are held to, byte for byte.

``encode(array) -> bytes`` of a uint8 [H, W, 3], uint8 [H, W] or uint16 [H, W] array, built from the pieces
``filter_rows`` (the per-row filter choice), ``tokens`` (literals and distance-1 runs of one block of scanlines), ``histograms``,
``plan`` (code lengths, codes, block headers, sizes, Adler-32) and ``emit`` (the file)."""
import heapq
import struct
import zlib

import numpy as np

BLOCK_ROWS = 64                  # FD_PNG_ENC_BLOCK_ROWS
HIST = 288                       # FD_PNG_ENC_HIST: 286 literal/length counts, [286] = the block's matches, [287] unused
HEADER_WORDS = 128               # FD_PNG_ENC_HEADER_WORDS
ADLER = 65521
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)

# match length m (3 .. 258) -> its symbol, the number of its extra bits, their value
LEN_SYM = np.zeros(259, np.int64)
LEN_EBITS = np.zeros(259, np.int64)
LEN_EVAL = np.zeros(259, np.int64)
for _m in range(3, 259):
    _k = max(k for k in range(29) if LEN_BASE[k] <= _m)
    LEN_SYM[_m], LEN_EBITS[_m], LEN_EVAL[_m] = 257 + _k, LEN_EXTRA[_k], _m - LEN_BASE[_k]
SYM_EXTRA = np.zeros(HIST, np.int64)     # extra bits of a literal/length symbol
SYM_EXTRA[257:286] = LEN_EXTRA


def kind_of(arr):
    """-> (H, W, bpp, colour type, bit depth); ValueError for anything but the three covered kinds."""
    a = np.asarray(arr)
    if a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3:
        k = (3, 2, 8)
    elif a.dtype == np.uint8 and a.ndim == 2:
        k = (1, 0, 8)
    elif a.dtype == np.uint16 and a.ndim == 2:
        k = (2, 0, 16)
    else:
        raise ValueError("png_enc_ref: %s %s is none of uint8 [H,W,3], uint8 [H,W], uint16 [H,W]" % (a.dtype, a.shape))
    if a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("png_enc_ref: empty image")
    return (a.shape[0], a.shape[1]) + k


def raw_rows(arr):
    """The unfiltered scanline bytes, uint8 [H, W * bpp]: 16-bit samples big-endian."""
    h, w, bpp, _, _ = kind_of(arr)
    a = np.ascontiguousarray(arr)
    if bpp == 2:
        a = a.astype(">u2")
    return a.view(np.uint8).reshape(h, w * bpp)


def filter_candidates(arr):
    """-> int64 [5, H, R]: the bytes of every row under each of the five filters, the decoder's arithmetic."""
    h, w, bpp, _, _ = kind_of(arr)
    x = raw_rows(arr).astype(np.int64)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255


def filter_costs(arr):
    """-> int64 [5, H]: the sum over the row of |int8(filtered byte)|."""
    f = filter_candidates(arr)
    return np.where(f < 128, f, 256 - f).sum(axis=2)


def filter_rows(arr):
    """-> (uint8 [H, 1 + R] filtered scanlines with their filter byte, int64 [H] the filter types): the smallest cost, a tie to
    the lowest type (np.argmin returns the first minimum)."""
    f = filter_candidates(arr)
    ft = np.argmin(filter_costs(arr), axis=0)
    rows = np.take_along_axis(f, ft[None, :, None], axis=0)[0]
    return np.concatenate([ft[:, None], rows], axis=1).astype(np.uint8), ft


def tokens(rows):
    """The tokens of a block of filtered scanlines (uint8 [n, P]), end-of-block NOT included -> (sym, ebits, eval, is_match) int64
    arrays.  Every scanline is cut into maximal runs of equal bytes; a run of length L is one literal, (L-1) // 258 matches of
    length 258 and the remainder m = (L-1) % 258 as one match if m >= 3, else as m literals; every match has distance 1."""
    n, p = rows.shape
    flat = rows.reshape(-1).astype(np.int64)
    start = np.ones(flat.size, bool)
    start[1:] = flat[1:] != flat[:-1]
    start[::p] = True                                            # runs never cross a scanline
    pos = np.flatnonzero(start)
    length = np.diff(np.append(pos, flat.size))
    v = flat[pos]
    n258, m = (length - 1) // 258, (length - 1) % 258
    cnt = 1 + n258 + np.where(m >= 3, 1, m)
    first = np.cumsum(cnt) - cnt
    k = np.arange(cnt.sum()) - np.repeat(first, cnt)             # the token's index inside its run
    v, n258, m = np.repeat(v, cnt), np.repeat(n258, cnt), np.repeat(m, cnt)
    full = (k >= 1) & (k <= n258)
    rest = (k > n258) & (m >= 3)
    sym = np.where(k == 0, v, np.where(full, 285, np.where(rest, LEN_SYM[m], v)))
    ebits = np.where(rest, LEN_EBITS[m], 0)
    ev = np.where(rest, LEN_EVAL[m], 0)
    return sym, ebits, ev, full | rest


def histograms(filtered):
    """uint32 [blocks, HIST] of one frame's filtered scanlines: per block of BLOCK_ROWS rows the 286 literal/length counts (the
    end-of-block symbol NOT counted: the plan adds it) and, at [286], the number of matches."""
    out = []
    for r0 in range(0, filtered.shape[0], BLOCK_ROWS):
        sym, _, _, match = tokens(filtered[r0:r0 + BLOCK_ROWS])
        hist = np.zeros(HIST, np.uint32)
        hist[:286] = np.bincount(sym, minlength=286)
        hist[286] = match.sum()
        out.append(hist)
    return np.stack(out)


def adler_rows(filtered):
    """uint32 [H, 2]: per scanline of P bytes d_0 .. d_(P-1) the pair (sum d_j, sum (P - j) d_j), both mod 65521."""
    p = filtered.shape[1]
    d = filtered.astype(np.int64)
    return np.stack([d.sum(axis=1) % ADLER, (d * (p - np.arange(p))).sum(axis=1) % ADLER], axis=1).astype(np.uint32)


def code_lengths(counts, limit):
    """Huffman code lengths of the symbols with a non-zero count, none above `limit`.  Two nodes of smallest (weight, id) are merged
    until one is left; a leaf's id is its symbol, the k-th merged node's is len(counts) + k.  While the deepest leaf is deeper than
    `limit`, every weight w becomes (w + 1) >> 1 and the tree is built again.  One used symbol gets length 1."""
    n = len(counts)
    lens = [0] * n
    w = {s: int(counts[s]) for s in range(n) if counts[s] > 0}
    if len(w) == 1:
        lens[next(iter(w))] = 1
    if len(w) < 2:
        return lens
    while True:
        heap = [(wt, s) for s, wt in w.items()]
        heapq.heapify(heap)
        parent, nid = {}, n
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            parent[a[1]] = parent[b[1]] = nid
            heapq.heappush(heap, (a[0] + b[0], nid))
            nid += 1
        depth = {}
        for node in range(nid - 2, n - 1, -1):                   # parents have larger ids than their children
            depth[node] = depth.get(parent[node], 0) + 1
        for s in w:
            lens[s] = depth.get(parent[s], 0) + 1
        if max(lens) <= limit:
            return lens
        w = {s: (wt + 1) >> 1 for s, wt in w.items()}


def canonical_codes(lens):
    """The canonical code of every length, bit-reversed for LSB-first emission (0 where the length is 0)."""
    codes, code = [0] * len(lens), 0
    for bits in range(1, max(max(lens), 1) + 1):
        for s, l in enumerate(lens):
            if l == bits:
                codes[s] = int(format(code, "0%db" % bits)[::-1], 2)
                code += 1
        code <<= 1
    return codes


def code_length_sequence(lens):
    """The greedy run-length form of a code-length sequence -> [(symbol, extra bits, extra value)].  At each position with value v
    and r = the number of equal values from there on: v == 0: r >= 11 -> symbol 18 for min(r, 138); r >= 3 -> symbol 17 for r;
    else one 0.  v != 0: v itself once, then while r >= 3 remain symbol 16 for min(r, 6), then the rest one by one."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, r = lens[i], 1
        while i + r < n and lens[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r > 0:
                if r >= 11:
                    k = min(r, 138)
                    out.append((18, 7, k - 11))
                elif r >= 3:
                    k = r
                    out.append((17, 3, k - 3))
                else:
                    k = 1
                    out.append((0, 0, 0))
                r -= k
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, 2, k - 3))
                r -= k
            out.extend([(v, 0, 0)] * r)
    return out


class _Bits:
    def __init__(self):
        self.value, self.n = 0, 0

    def put(self, v, bits):
        self.value |= int(v) << self.n
        self.n += int(bits)


def block_counts(hist):
    """-> (the 286 literal/length counts of a block with its end-of-block, its matches)."""
    counts = [int(c) for c in hist[:286]]
    counts[256] = 1
    return counts, int(hist[286])


def code_length_counts(lens, matches):
    """-> (the run-length form of the block's HLIT + 1 code lengths, the 19 counts of its symbols, HLIT)."""
    hlit = max(257, max(s for s in range(286) if lens[s]) + 1)
    seq = code_length_sequence(lens[:hlit] + [1 if matches else 0])
    cl_counts = [0] * 19
    for s, _, _ in seq:
        cl_counts[s] += 1
    return seq, cl_counts, hlit


def plan_block(hist, final):
    """One block: {"len": 286 lengths, "code": 286 reversed codes, "dist_len": 0 / 1, "header": int, "header_bits", "bits"}."""
    counts, matches = block_counts(hist)
    lens = code_lengths(counts, 15)
    codes = canonical_codes(lens)
    dist_len = 1 if matches else 0
    seq, cl_counts, hlit = code_length_counts(lens, matches)
    cl_lens = code_lengths(cl_counts, 7)
    if sum(1 for l in cl_lens if l) == 1:                        # a code-length code of one code is incomplete: give it a second
        cl_lens[0 if cl_lens[0] == 0 else 1] = 1
    cl_codes = canonical_codes(cl_lens)
    hclen = max(4, max(k for k in range(19) if cl_lens[CL_ORDER[k]]) + 1)
    w = _Bits()
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(0, 5)
    w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cl_lens[CL_ORDER[k]], 3)
    for s, eb, ev in seq:
        w.put(cl_codes[s], cl_lens[s])
        w.put(ev, eb)
    bits = w.n + sum(counts[s] * (lens[s] + int(SYM_EXTRA[s])) for s in range(286)) + matches * dist_len
    return {"len": lens, "code": codes, "dist_len": dist_len, "header": w.value, "header_bits": w.n, "bits": bits}


def plan(frames, hist, adler):
    """``frames`` = [(W, H, bpp)], ``hist`` uint32 [sum of blocks, HIST], ``adler`` uint32 [sum of H, 2], both frame after frame ->
    (blocks, files): per block ``plan_block`` plus "bit_off" (its first bit inside the frame's deflate stream); per frame
    {"adler", "off", "size", "stream_bits"} - the files lie one behind the other."""
    blocks, files, b0, r0, off = [], [], 0, 0, 0
    for w, h, bpp in frames:
        nb = (h + BLOCK_ROWS - 1) // BLOCK_ROWS
        at = 0
        for k in range(nb):
            blk = plan_block(hist[b0 + k], k == nb - 1)
            blk["bit_off"] = at
            at += blk["bits"]
            blocks.append(blk)
        p = 1 + w * bpp
        a, b = 1, 0
        for s, wsum in adler[r0:r0 + h]:
            b = (b + (p % ADLER) * a + int(wsum)) % ADLER
            a = (a + int(s)) % ADLER
        size = 57 + 2 + (at + 7) // 8 + 4
        files.append({"adler": (b << 16) | a, "off": off, "size": size, "stream_bits": at})
        off += size
        b0 += nb
        r0 += h
    return blocks, files


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))


def emit(arr, filtered, blocks, info):
    """The file of one frame from its filtered scanlines, its blocks' plans and its entry of ``plan``'s files."""
    h, w, bpp, colour, depth = kind_of(arr)
    nbytes = (info["stream_bits"] + 7) // 8
    out = np.zeros(nbytes + 4, np.uint8)
    for k, blk in enumerate(blocks):
        hb = blk["header_bits"]
        head = np.frombuffer((blk["header"] << (blk["bit_off"] & 7)).to_bytes((hb + 14) // 8 + 1, "little"), np.uint8)
        out[blk["bit_off"] >> 3:(blk["bit_off"] >> 3) + head.size] |= head[:out.size - (blk["bit_off"] >> 3)]
        sym, ebits, ev, match = tokens(filtered[k * BLOCK_ROWS:(k + 1) * BLOCK_ROWS])
        sym = np.append(sym, 256)
        ebits, ev, match = np.append(ebits, 0), np.append(ev, 0), np.append(match, False)
        lens, codes = np.asarray(blk["len"], np.int64), np.asarray(blk["code"], np.int64)
        n = lens[sym] + ebits + match                            # a match ends with the one distance code: one 0 bit
        val = codes[sym] | (ev << lens[sym])
        pos = blk["bit_off"] + hb + np.cumsum(n) - n
        assert int(pos[-1] + n[-1]) == blk["bit_off"] + blk["bits"], "the plan's block size is not what the tokens take"
        sh = val << (pos & 7)
        for j in range(4):
            np.bitwise_or.at(out, (pos >> 3) + j, ((sh >> (8 * j)) & 255).astype(np.uint8))
    stream = b"\x78\x01" + out[:nbytes].tobytes() + struct.pack(">I", info["adler"])
    data = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, 0)) + _chunk(b"IDAT", stream) +
            _chunk(b"IEND", b""))
    assert len(data) == info["size"]
    return data


def encode(arr):
    """The PNG file of one array."""
    arr = np.asarray(arr)
    h, w, bpp, _, _ = kind_of(arr)
    filtered, _ = filter_rows(arr)
    blocks, files = plan([(w, h, bpp)], histograms(filtered), adler_rows(filtered))
    return emit(arr, filtered, blocks, files[0])
