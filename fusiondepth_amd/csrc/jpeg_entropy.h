// Host half of the JPEG decoder (include/fdhip.h, "baseline JPEG frames"): marker parsing and Huffman decoding of one interleaved
// baseline scan into quantised coefficients.  Plain C++17, no HIP, no globals, no allocation: every function works on its arguments
// alone, so a host compiler (and its sanitizers) can build it by itself - tests/jpeg_host_main.cpp does.  csrc/jpeg.hip wraps the two
// entry points behind the C ABI.
//
// Safety contract: no read outside [file, file + n), no write outside [coef, coef + coef_cap) and qt[0 .. 191], whatever the bytes.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fdhip.h"

namespace fdjpeg {

enum Status { OK = 0, E_ARGS = 1, E_NOT_JPEG = 2, E_UNCOVERED = 3, E_TRUNCATED = 4, E_CORRUPT = 5, E_CAPACITY = 6 };

constexpr int ERR_LEN = 160;
constexpr int FAST_BITS = 10;

// zigzag position -> natural (row-major) position
static const uint8_t NATURAL[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    uint16_t fast[1 << FAST_BITS];   // (length << 8) | symbol for codes of at most FAST_BITS bits, 0 = longer or none
    int32_t maxcode[18];             // first 16-bit-aligned value that is NOT a code of this length
    int32_t delta[17];               // index of a code's symbol = code + delta[length]
    uint8_t vals[256];
    int defined;
};

struct Header {
    int width, height, ncomp, progressive_or_other, bits;
    int id[4], h[4], v[4], tq[4], td[4], ta[4];
    int jfif, adobe, restart_interval, sof_seen;
    uint16_t qt[4][64];              // natural order
    int qt_defined[4];
    Huff dc[4], ac[4];
    size_t scan_start;               // first byte of entropy-coded data
    int covered;
};

inline int fail(char* err, int status, const char* msg) {
    if (err) snprintf(err, ERR_LEN, "%s", msg);
    return status;
}

inline int build_huff(Huff& t, const uint8_t* counts /*[16]*/, const uint8_t* vals, int total) {
    memset(t.fast, 0, sizeof(t.fast));
    memcpy(t.vals, vals, (size_t)total);
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        t.delta[len] = k - code;
        for (int i = 0; i < counts[len - 1]; ++i, ++code, ++k) {
            if (code >= (1 << len)) return E_CORRUPT;
            if (len <= FAST_BITS) {
                const int first = code << (FAST_BITS - len), span = 1 << (FAST_BITS - len);
                for (int j = 0; j < span; ++j) t.fast[first + j] = (uint16_t)((len << 8) | vals[k]);
            }
        }
        t.maxcode[len] = code << (16 - len);
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    t.defined = 1;
    return OK;
}

// Parse the markers up to and including the first SOS.  Returns OK when the file is a JPEG whose frame header was read; h.covered then
// says whether the entropy decoder takes it (`err` holds the reason when it does not).
inline int parse(const uint8_t* p, size_t n, Header& h, char* err) {
    h.width = h.height = h.ncomp = h.progressive_or_other = h.bits = 0;
    h.jfif = h.adobe = h.restart_interval = h.sof_seen = h.covered = 0;
    h.scan_start = 0;
    for (int i = 0; i < 4; ++i) h.qt_defined[i] = h.dc[i].defined = h.ac[i].defined = 0;
    if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return fail(err, E_NOT_JPEG, "jpeg: no SOI marker");
    size_t pos = 2;
    for (;;) {
        if (pos + 2 > n) return fail(err, E_TRUNCATED, "jpeg: file ends inside the headers");
        if (p[pos] != 0xFF) return fail(err, E_CORRUPT, "jpeg: marker expected in the headers");
        const int m = p[pos + 1];
        if (m == 0xFF) { ++pos; continue; }                      // fill byte
        pos += 2;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // parameterless
        if (m == 0xD9) return fail(err, E_CORRUPT, "jpeg: EOI before any scan");
        if (m == 0x00) return fail(err, E_CORRUPT, "jpeg: stuffed byte in the headers");
        if (pos + 2 > n) return fail(err, E_TRUNCATED, "jpeg: file ends inside the headers");
        const size_t len = ((size_t)p[pos] << 8) | p[pos + 1];
        if (len < 2) return fail(err, E_CORRUPT, "jpeg: segment length below 2");
        if (pos + len > n) return fail(err, E_TRUNCATED, "jpeg: file ends inside a segment");
        const uint8_t* s = p + pos + 2;
        const size_t sl = len - 2;
        if (m == 0xE0) {
            if (sl >= 5 && memcmp(s, "JFIF\0", 5) == 0) h.jfif = 1;
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) h.adobe = 1;
        } else if (m == 0xDB) {
            size_t q = 0;
            while (q < sl) {
                const int pq = s[q] >> 4, tq = s[q] & 15;
                if (pq > 1 || tq > 3) return fail(err, E_CORRUPT, "jpeg: bad quantisation table header");
                const size_t need = 1 + (pq ? 128 : 64);
                if (q + need > sl) return fail(err, E_CORRUPT, "jpeg: quantisation table leaves its segment");
                for (int i = 0; i < 64; ++i)
                    h.qt[tq][NATURAL[i]] = pq ? (uint16_t)((s[q + 1 + 2 * i] << 8) | s[q + 2 + 2 * i]) : (uint16_t)s[q + 1 + i];
                h.qt_defined[tq] = 1;
                q += need;
            }
        } else if (m == 0xC4) {
            size_t q = 0;
            while (q < sl) {
                if (q + 17 > sl) return fail(err, E_CORRUPT, "jpeg: Huffman table leaves its segment");
                const int tc = s[q] >> 4, th = s[q] & 15;
                if (tc > 1 || th > 3) return fail(err, E_CORRUPT, "jpeg: bad Huffman table header");
                int total = 0;
                for (int i = 0; i < 16; ++i) total += s[q + 1 + i];
                if (total > 256 || q + 17 + (size_t)total > sl) return fail(err, E_CORRUPT, "jpeg: Huffman table leaves its segment");
                Huff& t = tc ? h.ac[th] : h.dc[th];
                t.defined = 0;
                if (build_huff(t, s + q + 1, s + q + 17, total) != OK) return fail(err, E_CORRUPT, "jpeg: Huffman code lengths overflow");
                q += 17 + (size_t)total;
            }
        } else if (m == 0xDD) {
            if (sl != 2) return fail(err, E_CORRUPT, "jpeg: bad DRI segment");
            h.restart_interval = (s[0] << 8) | s[1];
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8) {        // a frame header (0xC4 was taken above, 0xCC is DAC)
            if (m == 0xCC) {
                pos += len;
                continue;
            }
            if (h.sof_seen) return fail(err, E_CORRUPT, "jpeg: two frame headers");
            if (sl < 6) return fail(err, E_CORRUPT, "jpeg: short frame header");
            h.sof_seen = 1;
            h.progressive_or_other = (m != 0xC0 && m != 0xC1);
            h.bits = s[0];
            h.height = (s[1] << 8) | s[2];
            h.width = (s[3] << 8) | s[4];
            h.ncomp = s[5];
            if (h.ncomp < 1 || h.ncomp > 4 || sl != 6 + 3 * (size_t)h.ncomp) return fail(err, E_CORRUPT, "jpeg: bad component count");
            for (int c = 0; c < h.ncomp; ++c) {
                h.id[c] = s[6 + 3 * c];
                h.h[c] = s[7 + 3 * c] >> 4;
                h.v[c] = s[7 + 3 * c] & 15;
                h.tq[c] = s[8 + 3 * c];
            }
            if (h.width < 1) return fail(err, E_CORRUPT, "jpeg: zero width");
        } else if (m == 0xDA) {
            if (!h.sof_seen) return fail(err, E_CORRUPT, "jpeg: scan before the frame header");
            if (h.progressive_or_other) return fail(err, OK, "jpeg: not covered: progressive, lossless or arithmetic-coded frame");
            if (h.bits != 8) return fail(err, OK, "jpeg: not covered: sample precision is not 8 bits");
            if (h.height < 1) return fail(err, OK, "jpeg: not covered: height given by a DNL marker");
            if (h.ncomp != 1 && h.ncomp != 3) return fail(err, OK, "jpeg: not covered: 2 or 4 components");
            if (sl < 1 || sl != 4 + 2 * (size_t)s[0]) return fail(err, E_CORRUPT, "jpeg: bad scan header");
            if (s[0] != h.ncomp) return fail(err, OK, "jpeg: not covered: more than one scan");
            for (int c = 0; c < h.ncomp; ++c) {
                if (s[1 + 2 * c] != h.id[c]) return fail(err, OK, "jpeg: not covered: scan components out of frame order");
                h.td[c] = s[2 + 2 * c] >> 4;
                h.ta[c] = s[2 + 2 * c] & 15;
                if (h.td[c] > 3 || h.ta[c] > 3 || h.tq[c] > 3) return fail(err, E_CORRUPT, "jpeg: table index above 3");
                if (!h.dc[h.td[c]].defined || !h.ac[h.ta[c]].defined || !h.qt_defined[h.tq[c]])
                    return fail(err, E_CORRUPT, "jpeg: scan names a table that was not defined");
            }
            const uint8_t* e = s + 1 + 2 * h.ncomp;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0) return fail(err, OK, "jpeg: not covered: spectral selection in a baseline scan");
            if (h.ncomp == 3) {
                if (!h.jfif && h.adobe) return fail(err, OK, "jpeg: not covered: Adobe marker (RGB or CMYK colour)");
                if (!h.jfif && h.id[0] == 'R' && h.id[1] == 'G' && h.id[2] == 'B') return fail(err, OK, "jpeg: not covered: RGB components");
                if (h.h[1] != 1 || h.v[1] != 1 || h.h[2] != 1 || h.v[2] != 1) return fail(err, OK, "jpeg: not covered: chroma sampling is not 1x1");
                const int hv = h.h[0] * 16 + h.v[0];
                if (hv != 0x11 && hv != 0x21 && hv != 0x22) return fail(err, OK, "jpeg: not covered: luma sampling is not 1x1, 2x1 or 2x2");
            } else {
                h.h[0] = h.v[0] = 1;                             // a one-component scan is never interleaved: its MCU is one block
            }
            h.scan_start = pos + len;
            h.covered = 1;
            return OK;
        } else if (m == 0xDC) {
            return h.sof_seen ? fail(err, OK, "jpeg: not covered: DNL marker") : fail(err, E_CORRUPT, "jpeg: DNL before the frame header");
        }
        pos += len;                                              // APPn, COM and anything else with a length
    }
}

inline void fill_info(const Header& h, fd_jpeg_info* info) {
    memset(info, 0, sizeof(*info));
    info->width = h.width;
    info->height = h.height;
    info->components = h.ncomp;
    info->covered = h.covered;
    info->restart_interval = h.restart_interval;
    if (!h.covered) return;
    info->h_samp = h.h[0];
    info->v_samp = h.v[0];
    const int mcux = (h.width + 8 * h.h[0] - 1) / (8 * h.h[0]), mcuy = (h.height + 8 * h.v[0] - 1) / (8 * h.v[0]);
    long blocks = 0;
    for (int c = 0; c < h.ncomp; ++c) {
        info->blocks_w[c] = mcux * (c ? 1 : h.h[0]);
        info->blocks_h[c] = mcuy * (c ? 1 : h.v[0]);
        blocks += (long)info->blocks_w[c] * info->blocks_h[c];
    }
    info->coef_count = 64 * blocks;
}

inline int probe(const uint8_t* file, long n, fd_jpeg_info* info, char* err) {
    if (!file || n < 0 || !info) return fail(err, E_ARGS, "fd_jpeg_probe: bad args");
    if (err) err[0] = 0;
    memset(info, 0, sizeof(*info));
    Header h;
    const int st = parse(file, (size_t)n, h, err);
    if (st != OK) return st;
    fill_info(h, info);
    return OK;
}

struct Bits {
    const uint8_t* p;
    size_t pos, n;
    uint64_t buf;   // the low `cnt` bits are unread, oldest highest
    int cnt;
    int fake;       // how many of them are zero padding appended after the data ran into a marker or the end
    int marker;     // 0, the marker byte that stopped the reader, or -1 at the end of the file

    inline void fill() {
        while (cnt <= 56) {
            unsigned b = 0;
            if (!marker) {
                if (pos >= n) {
                    marker = -1;
                } else {
                    b = p[pos];
                    if (b != 0xFF) {
                        ++pos;
                    } else if (pos + 1 >= n) {
                        marker = -1;
                    } else if (p[pos + 1] == 0) {
                        pos += 2;
                    } else if (p[pos + 1] == 0xFF) {
                        ++pos;                                   // a fill byte before a marker
                        continue;
                    } else {
                        marker = p[pos + 1];
                    }
                }
            }
            if (marker) {
                b = 0;
                fake += 8;
            }
            buf = (buf << 8) | b;
            cnt += 8;
        }
    }
    inline unsigned peek16() const { return (unsigned)(buf >> (cnt - 16)) & 0xFFFFu; }
    inline unsigned take(int k) {
        cnt -= k;
        return (unsigned)(buf >> cnt) & ((1u << k) - 1u);
    }
};

// one Huffman symbol, or -1; the caller keeps at least 32 unread bits in the buffer
inline int symbol(Bits& br, const Huff& t) {
    const unsigned look = br.peek16();
    const unsigned f = t.fast[look >> (16 - FAST_BITS)];
    if (f) {
        br.cnt -= (int)(f >> 8);
        return (int)(f & 255u);
    }
    int len = FAST_BITS + 1;
    while ((int32_t)look >= t.maxcode[len]) ++len;
    if (len > 16) return -1;
    const int idx = (int)(look >> (16 - len)) + t.delta[len];
    if (idx < 0 || idx > 255) return -1;
    br.cnt -= len;
    return t.vals[idx];
}

inline int extend(unsigned v, int s) { return v < (1u << (s - 1)) ? (int)v - ((1 << s) - 1) : (int)v; }

inline int entropy_decode(const uint8_t* file, long n, int16_t* coef, long coef_cap, uint16_t* qt, fd_jpeg_info* info, char* err) {
    if (!file || n < 0 || !coef || coef_cap < 0 || !qt || !info) return fail(err, E_ARGS, "fd_jpeg_entropy_decode: bad args");
    if (err) err[0] = 0;
    memset(info, 0, sizeof(*info));
    Header h;
    int st = parse(file, (size_t)n, h, err);
    if (st != OK) return st;
    fill_info(h, info);
    if (!h.covered) return E_UNCOVERED;                          // err holds the reason
    if (info->coef_count > coef_cap) return fail(err, E_CAPACITY, "fd_jpeg_entropy_decode: coef_cap is below the frame's coefficient count");
    memset(coef, 0, (size_t)info->coef_count * sizeof(int16_t));
    for (int c = 0; c < 3; ++c) memcpy(qt + 64 * c, h.qt[h.tq[c < h.ncomp ? c : 0]], 64 * sizeof(uint16_t));

    int16_t* base[3];
    long at = 0;
    for (int c = 0; c < h.ncomp; ++c) {
        base[c] = coef + at;
        at += 64L * info->blocks_w[c] * info->blocks_h[c];
    }
    const int mcux = info->blocks_w[h.ncomp - 1], mcuy = info->blocks_h[h.ncomp - 1];
    Bits br{file, h.scan_start, (size_t)n, 0, 0, 0, 0};
    int pred[3] = {0, 0, 0};
    long mcu = 0;
    int next_rst = 0;
    for (int my = 0; my < mcuy; ++my) {
        for (int mx = 0; mx < mcux; ++mx, ++mcu) {
            if (h.restart_interval && mcu && mcu % h.restart_interval == 0) {
                br.buf = 0;
                br.cnt = br.fake = 0;
                if (br.marker == -1) return fail(err, E_TRUNCATED, "jpeg: file ends where a restart marker is due");
                while (!br.marker) {
                    if (br.pos + 1 >= br.n) return fail(err, E_TRUNCATED, "jpeg: file ends where a restart marker is due");
                    if (br.p[br.pos] != 0xFF || br.p[br.pos + 1] == 0) return fail(err, E_CORRUPT, "jpeg: data where a restart marker is due");
                    if (br.p[br.pos + 1] == 0xFF) ++br.pos;
                    else br.marker = br.p[br.pos + 1];
                }
                if (br.marker != 0xD0 + next_rst) return fail(err, E_CORRUPT, "jpeg: wrong marker where a restart marker is due");
                br.pos += 2;
                br.marker = 0;
                next_rst = (next_rst + 1) & 7;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < h.ncomp; ++c) {
                const Huff& dct = h.dc[h.td[c]];
                const Huff& act = h.ac[h.ta[c]];
                const int ch = c ? 1 : h.h[0], cv = c ? 1 : h.v[0];
                for (int vy = 0; vy < cv; ++vy) {
                    for (int hx = 0; hx < ch; ++hx) {
                        int16_t* blk = base[c] + 64 * ((long)(my * cv + vy) * info->blocks_w[c] + (mx * ch + hx));
                        br.fill();
                        const int t = symbol(br, dct);
                        if (t < 0 || t > 15) return fail(err, E_CORRUPT, "jpeg: bad DC Huffman code");
                        if (t) pred[c] = (int16_t)(pred[c] + extend(br.take(t), t));
                        blk[0] = (int16_t)pred[c];
                        for (int k = 1; k < 64; ++k) {
                            if (br.cnt < 32) br.fill();
                            const int rs = symbol(br, act);
                            if (rs < 0) return fail(err, E_CORRUPT, "jpeg: bad AC Huffman code");
                            const int r = rs >> 4, s = rs & 15;
                            if (!s) {
                                if (r != 15) break;
                                k += 15;
                                continue;
                            }
                            k += r;
                            if (k > 63) return fail(err, E_CORRUPT, "jpeg: coefficient index above 63");
                            blk[NATURAL[k]] = (int16_t)extend(br.take(s), s);
                        }
                        if (br.cnt < br.fake) return fail(err, E_TRUNCATED, "jpeg: entropy-coded data ends before the last block");
                    }
                }
            }
        }
    }
    return OK;
}

}  // namespace fdjpeg
