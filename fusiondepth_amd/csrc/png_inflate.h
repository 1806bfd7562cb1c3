// Host half of the PNG decoder (include/fdhip.h, "PNG frames"): the chunk walk and an inflate of the IDAT stream into the FILTERED
// scanlines.  Plain C++17, no HIP, no zlib, no globals, no allocation: every function works on its arguments alone, so a host compiler
// (and its sanitizers) can build it by itself - tests/png_host_main.cpp does.  csrc/png.hip wraps the two entry points behind the C ABI.
//
// The inflate: a 64-bit bit buffer refilled eight bytes at a time while the current IDAT payload has that many left (byte by byte
// across chunk boundaries), an 11-bit literal/length table and an 8-bit distance table with second-level tables behind them, and the
// output slice as its own window - the whole picture is one contiguous write, so a match copies from `dst` itself.
//
// Safety contract: no read outside [file, file + n), no write outside [dst, dst + dst_cap), whatever the bytes.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fdhip.h"

namespace fdpng {

enum Status { OK = 0, E_ARGS = 1, E_NOT_PNG = 2, E_UNCOVERED = 3, E_TRUNCATED = 4, E_CORRUPT = 5, E_CAPACITY = 6 };

constexpr int ERR_LEN = 160;
constexpr int LIT_BITS = 11, DIST_BITS = 8;
// a second-level table has at most 2^(15 - root) entries and at least two codes under it: 144 * 16 and 16 * 128 entries bound them
constexpr int LIT_CAP = (1 << LIT_BITS) + 144 * 16, DIST_CAP = (1 << DIST_BITS) + 16 * 128, CL_CAP = 1 << 7;

// table entry: bits 0-7 the code's length, 8-11 the extra bits (or a second-level table's index bits), 12-15 flags, 16-31 the value
constexpr uint32_t F_LIT = 0x1000u, F_EOB = 0x2000u, F_SUB = 0x4000u, F_BAD = 0x8000u;

static const uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint16_t DIST_BASE[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                       193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
static const uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
static const uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
static const uint8_t IEND[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};

inline int fail(char* err, int status, const char* msg) {
    if (err) snprintf(err, ERR_LEN, "%s", msg);
    return status;
}

inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

inline uint32_t crc32(const uint8_t* p, size_t n) {             // bit by bit: it runs over the 17 bytes of IHDR alone
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

struct Header {
    uint32_t width, height;
    int depth, colour, interlace, covered, bpp;
    long row_bytes, raw_bytes;
    size_t first_idat;               // offset of the first IDAT chunk's length field, 0 when the file ends before one
};

// Signature, IHDR and the chunks up to the first IDAT.  OK once IHDR was read; h.covered says whether inflate takes the file (`err`
// holds the reason when it does not).
inline int parse(const uint8_t* p, size_t n, Header& h, char* err) {
    static const uint8_t SIG[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    memset(&h, 0, sizeof(h));
    if (n < 8) return fail(err, n && memcmp(p, SIG, n) ? E_NOT_PNG : E_TRUNCATED, "png: file ends inside the signature");
    if (memcmp(p, SIG, 8) != 0) return fail(err, E_NOT_PNG, "png: no PNG signature");
    if (n < 33) return fail(err, E_TRUNCATED, "png: file ends inside IHDR");
    if (be32(p + 8) != 13 || memcmp(p + 12, "IHDR", 4) != 0) return fail(err, E_CORRUPT, "png: the first chunk is not a 13-byte IHDR");
    if (crc32(p + 12, 17) != be32(p + 29)) return fail(err, E_CORRUPT, "png: IHDR fails its CRC");
    h.width = be32(p + 16);
    h.height = be32(p + 20);
    h.depth = p[24];
    h.colour = p[25];
    h.interlace = p[28];
    if (!h.width || !h.height || h.width > 0x7fffffffu || h.height > 0x7fffffffu) return fail(err, E_CORRUPT, "png: width or height outside 1 .. 2^31 - 1");
    if (p[26] != 0 || p[27] != 0) return fail(err, E_CORRUPT, "png: unknown compression or filter method");
    const char* why = nullptr;
    if (h.interlace) why = "png: not covered: interlaced (Adam7)";
    else if (h.colour == 3) why = "png: not covered: palette";
    else if (h.colour == 4 || h.colour == 6) why = "png: not covered: alpha channel";
    else if (h.colour == 2 && h.depth == 8) h.bpp = 3;
    else if (h.colour == 0 && h.depth == 8) h.bpp = 1;
    else if (h.colour == 0 && h.depth == 16) h.bpp = 2;
    else if (h.colour == 2 && h.depth == 16) why = "png: not covered: 16-bit RGB";
    else if (h.colour == 0 && (h.depth == 1 || h.depth == 2 || h.depth == 4)) why = "png: not covered: bit depth 1, 2 or 4";
    else return fail(err, E_CORRUPT, "png: colour type and bit depth do not go together");
    if (!why && ((uint64_t)h.width * h.bpp + 1) * h.height > 0x7fffffffull) why = "png: not covered: more than 2^31 - 1 scanline bytes";
    // tRNS and acTL stand before the first IDAT
    size_t pos = 33;
    while (!why) {
        if (pos + 8 > n) break;                                  // inflate reports the truncation
        const size_t len = be32(p + pos);
        const uint8_t* type = p + pos + 4;
        if (memcmp(type, "IDAT", 4) == 0) {
            h.first_idat = pos;
            break;
        }
        if (memcmp(type, "tRNS", 4) == 0) why = "png: not covered: tRNS (transparency)";
        else if (memcmp(type, "acTL", 4) == 0) why = "png: not covered: animated PNG";
        else if (memcmp(type, "IEND", 4) == 0) return fail(err, E_CORRUPT, "png: IEND before any IDAT");
        if (len > n - pos - 8 || n - pos - 8 - len < 4) break;
        pos += 12 + len;
    }
    if (why) return fail(err, OK, why);
    h.covered = 1;
    h.row_bytes = (long)h.width * h.bpp;
    h.raw_bytes = (long)h.height * (1 + h.row_bytes);
    return OK;
}

inline void fill_info(const Header& h, fd_png_info* info) {
    memset(info, 0, sizeof(*info));
    info->width = (int)h.width;
    info->height = (int)h.height;
    info->bit_depth = h.depth;
    info->colour_type = h.colour;
    info->interlace = h.interlace;
    info->covered = h.covered;
    if (!h.covered) return;
    info->bpp = h.bpp;
    info->row_bytes = h.row_bytes;
    info->raw_bytes = h.raw_bytes;
}

inline int probe(const uint8_t* file, long n, fd_png_info* info, char* err) {
    if (!file || n < 0 || !info) return fail(err, E_ARGS, "fd_png_probe: bad args");
    if (err) err[0] = 0;
    memset(info, 0, sizeof(*info));
    Header h;
    const int st = parse(file, (size_t)n, h, err);
    if (st != OK) return st;
    fill_info(h, info);
    return OK;
}

// The IDAT payloads as one bit stream, least significant bit first.
struct In {
    const uint8_t* p;
    size_t n;
    size_t pos, end;    // the unread rest of the current IDAT payload
    size_t next;        // the chunk behind it
    uint64_t buf;       // the low `cnt` bits are unread; bits above them repeat the bytes at `pos` (the fast refill) or are zero
    int cnt;            // below zero: more bits were taken than the stream holds
    int eof;            // no IDAT payload is left
    int status;         // why: E_TRUNCATED when the file ended inside the chunks, OK when the IDAT run simply ended

    // step to the next non-empty IDAT payload; 0 when there is none
    inline int next_chunk() {
        for (;;) {
            if (next + 8 > n) {
                status = E_TRUNCATED;
                return 0;
            }
            const size_t len = be32(p + next);
            if (memcmp(p + next + 4, "IDAT", 4) != 0) return 0;
            if (len > n - next - 8 || n - next - 8 - len < 4) {  // the payload and its CRC must lie inside the file
                status = E_TRUNCATED;
                return 0;
            }
            pos = next + 8;
            end = pos + len;
            next = end + 4;
            if (len) return 1;
        }
    }
    inline void refill() {
        if (end - pos >= 8) {
            uint64_t w;
            memcpy(&w, p + pos, 8);
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_BIG_ENDIAN__
            w = __builtin_bswap64(w);
#endif
            buf |= w << cnt;                                     // cnt <= 63 here: the callers refill below 56 only
            pos += (size_t)((63 - cnt) >> 3);
            cnt |= 56;
            return;
        }
        while (cnt <= 56 && !eof) {
            if (pos == end && !next_chunk()) {
                eof = 1;
                break;
            }
            buf |= (uint64_t)p[pos++] << cnt;
            cnt += 8;
        }
    }
    inline void need(int k) {
        if (cnt < k) refill();
    }
    inline uint32_t take(int k) {                                // k <= 16; the caller looks at cnt afterwards
        const uint32_t v = (uint32_t)buf & ((1u << k) - 1u);
        buf >>= k;
        cnt -= k;
        return v;
    }
};

inline uint32_t reverse_bits(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i, code >>= 1) r = (r << 1) | (code & 1u);
    return r;
}

enum Kind { K_LITLEN = 0, K_DIST = 1, K_CODELEN = 2 };

inline uint32_t entry_of(int kind, int sym, int len) {
    if (kind == K_CODELEN) return ((uint32_t)sym << 16) | (uint32_t)len;
    if (kind == K_DIST) {
        if (sym >= 30) return F_BAD | (uint32_t)len;
        return ((uint32_t)DIST_BASE[sym] << 16) | ((uint32_t)DIST_EXTRA[sym] << 8) | (uint32_t)len;
    }
    if (sym < 256) return ((uint32_t)sym << 16) | F_LIT | (uint32_t)len;
    if (sym == 256) return F_EOB | (uint32_t)len;
    if (sym >= 286) return F_BAD | (uint32_t)len;
    return ((uint32_t)LEN_BASE[sym - 257] << 16) | ((uint32_t)LEN_EXTRA[sym - 257] << 8) | (uint32_t)len;
}

// Canonical Huffman code of `lens` -> a `root`-bit first-level table, second-level tables behind it.  zlib's rule for what is a code:
// over-subscribed never; incomplete only as at most one code of length 1 (the one-code distance tree), and never for the code-length
// code.  Unused patterns decode to F_BAD.
inline int build(uint32_t* table, int cap, int root, const uint8_t* lens, int nsym, int kind) {
    int count[16] = {0};
    for (int s = 0; s < nsym; ++s) ++count[lens[s]];
    int maxlen = 15;
    while (maxlen > 0 && !count[maxlen]) --maxlen;
    int left = 1;
    for (int len = 1; len <= 15; ++len) {
        left = 2 * left - count[len];
        if (left < 0) return E_CORRUPT;
    }
    if (left > 0 && (kind == K_CODELEN || maxlen > 1)) return E_CORRUPT;
    uint32_t next_code[16];
    uint32_t code = 0;
    for (int len = 1; len <= 15; ++len) {
        code = (code + (uint32_t)count[len - 1] * (len > 1)) << 1;
        next_code[len] = code;
    }
    const uint32_t root_size = 1u << root, root_mask = root_size - 1u;
    for (uint32_t i = 0; i < root_size; ++i) table[i] = F_BAD | 1u;
    uint8_t deepest[1 << LIT_BITS];                              // per first-level pattern: the longest code that starts with it
    if (maxlen > root) memset(deepest, 0, root_size);
    uint16_t rev[288];
    for (int s = 0; s < nsym; ++s) {
        const int len = lens[s];
        if (!len) continue;
        const uint32_t r = reverse_bits(next_code[len]++, len);
        rev[s] = (uint16_t)r;
        if (len <= root) {
            const uint32_t e = entry_of(kind, s, len);
            for (uint32_t i = r; i < root_size; i += 1u << len) table[i] = e;
        } else if (deepest[r & root_mask] < len) {
            deepest[r & root_mask] = (uint8_t)len;
        }
    }
    if (maxlen <= root) return OK;
    uint32_t used = root_size;
    for (int s = 0; s < nsym; ++s) {
        const int len = lens[s];
        if (len <= root) continue;
        const uint32_t r = rev[s], first = r & root_mask;
        const int sub_bits = deepest[first] - root;
        if (!(table[first] & F_SUB)) {
            if (used + (1u << sub_bits) > (uint32_t)cap) return E_CORRUPT;     // cannot happen (LIT_CAP, DIST_CAP): kept as a bound
            table[first] = (used << 16) | F_SUB | ((uint32_t)sub_bits << 8) | (uint32_t)root;
            for (uint32_t i = 0; i < (1u << sub_bits); ++i) table[used + i] = F_BAD | 1u;
            used += 1u << sub_bits;
        }
        const uint32_t base = table[first] >> 16, e = entry_of(kind, s, len);
        for (uint32_t i = r >> root; i < (1u << sub_bits); i += 1u << (len - root)) table[base + i] = e;
    }
    return OK;
}

inline uint32_t lookup(const uint32_t* table, int root, uint64_t buf) {
    uint32_t e = table[(uint32_t)buf & ((1u << root) - 1u)];
    if (e & F_SUB) e = table[(e >> 16) + ((uint32_t)(buf >> root) & ((1u << ((e >> 8) & 15u)) - 1u))];
    return e;
}

inline uint32_t adler32(const uint8_t* p, size_t n) {
    uint32_t s1 = 1, s2 = 0;
    while (n) {
        size_t run = n < 5552 ? n : 5552;                        // the longest run before s2 could leave 32 bits
        n -= run;
        for (; run >= 16; run -= 16, p += 16) {
            uint32_t t1 = 0, t2 = 0;
            for (int i = 0; i < 16; ++i) {
                t1 += p[i];
                t2 += (uint32_t)(16 - i) * p[i];
            }
            s2 += 16 * s1 + t2;
            s1 += t1;
        }
        for (; run; --run) {
            s1 += *p++;
            s2 += s1;
        }
        s1 %= 65521u;
        s2 %= 65521u;
    }
    return (s2 << 16) | s1;
}

struct Tables {
    uint32_t lit[LIT_CAP];
    uint32_t dist[DIST_CAP];
    int fixed;                       // the two tables hold the fixed code
};

// copy `len` bytes from `dist` back; the caller has checked that dist reaches no further than dst and that `room` >= len
inline uint8_t* copy_match(uint8_t* out, size_t len, size_t dist, size_t room) {
    const uint8_t* from = out - dist;
    if (dist >= 8 && room >= len + 8) {                          // eight bytes at a time; the overshoot stays inside the room
        uint8_t* to = out;
        out += len;
        do {
            memcpy(to, from, 8);
            to += 8;
            from += 8;
        } while (to < out);
    } else if (dist == 1) {
        memset(out, *from, len);
        out += len;
    } else {
        while (len--) *out++ = *from++;
    }
    return out;
}

// One compressed block's symbols.  `out` runs from dst towards lim = dst + raw_bytes.  While the current IDAT payload has eight bytes
// left and the output 274 (a longest match and its overshoot), the state lives in locals, the refill is one unaligned load and up to
// three literals go out per refill; the careful loop behind it takes every symbol that stands near an end.
inline int block(In& in, const Tables& t, uint8_t* dst, uint8_t*& out_ref, uint8_t* lim, char* err) {
    uint8_t* out = out_ref;
    {
        uint64_t buf = in.buf;
        int cnt = in.cnt;
        size_t pos = in.pos;
        const size_t end = in.end;
        const uint8_t* const p = in.p;
        while (end - pos >= 8 && (size_t)(lim - out) >= 274) {
            uint64_t w;
            memcpy(&w, p + pos, 8);
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_BIG_ENDIAN__
            w = __builtin_bswap64(w);
#endif
            buf |= w << cnt;
            pos += (size_t)((63 - cnt) >> 3);
            cnt |= 56;
            uint32_t e = lookup(t.lit, LIT_BITS, buf);
            if (e & F_LIT) {
                buf >>= (e & 255u);
                cnt -= (int)(e & 255u);
                *out++ = (uint8_t)(e >> 16);
                e = lookup(t.lit, LIT_BITS, buf);
                if (e & F_LIT) {
                    buf >>= (e & 255u);
                    cnt -= (int)(e & 255u);
                    *out++ = (uint8_t)(e >> 16);
                    e = lookup(t.lit, LIT_BITS, buf);
                    if (e & F_LIT) {
                        buf >>= (e & 255u);
                        cnt -= (int)(e & 255u);
                        *out++ = (uint8_t)(e >> 16);
                        continue;
                    }
                }
                if (end - pos < 8) break;                        // the careful loop looks this symbol up again
                memcpy(&w, p + pos, 8);
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_BIG_ENDIAN__
                w = __builtin_bswap64(w);
#endif
                buf |= w << cnt;
                pos += (size_t)((63 - cnt) >> 3);
                cnt |= 56;
            }
            if (e & (F_EOB | F_BAD)) break;
            buf >>= (e & 255u);
            cnt -= (int)(e & 255u);
            const uint32_t xl = (e >> 8) & 15u;
            const size_t len = (e >> 16) + ((uint32_t)buf & ((1u << xl) - 1u));
            buf >>= xl;
            cnt -= (int)xl;
            e = lookup(t.dist, DIST_BITS, buf);
            buf >>= (e & 255u);
            cnt -= (int)(e & 255u);
            const uint32_t xd = (e >> 8) & 15u;
            const size_t dist = (e >> 16) + ((uint32_t)buf & ((1u << xd) - 1u));
            buf >>= xd;
            cnt -= (int)xd;
            if (e & F_BAD) return fail(err, E_CORRUPT, "png: undefined distance code");
            if (dist > (size_t)(out - dst)) return fail(err, E_CORRUPT, "png: a distance reaches before the first byte written");
            out = copy_match(out, len, dist, (size_t)(lim - out));
        }
        in.buf = buf;
        in.cnt = cnt;
        in.pos = pos;
    }
    for (;;) {
        in.need(48);
        uint32_t e = lookup(t.lit, LIT_BITS, in.buf);
        in.buf >>= (e & 255u);
        in.cnt -= (int)(e & 255u);
        if (e & F_LIT) {
            if (in.cnt < 0) return fail(err, E_TRUNCATED, "png: the IDAT data ends inside a block");
            if (out == lim) return fail(err, E_CORRUPT, "png: the stream holds more than height * (1 + row_bytes) bytes");
            *out++ = (uint8_t)(e >> 16);
            continue;
        }
        if (e & (F_EOB | F_BAD)) {
            if (in.cnt < 0) return fail(err, E_TRUNCATED, "png: the IDAT data ends inside a block");
            if (e & F_BAD) return fail(err, E_CORRUPT, "png: undefined literal/length code");
            out_ref = out;
            return OK;
        }
        const size_t len = (e >> 16) + in.take((int)((e >> 8) & 15u));
        e = lookup(t.dist, DIST_BITS, in.buf);
        in.buf >>= (e & 255u);
        in.cnt -= (int)(e & 255u);
        const size_t dist = (e >> 16) + in.take((int)((e >> 8) & 15u));
        if (in.cnt < 0) return fail(err, E_TRUNCATED, "png: the IDAT data ends inside a block");
        if (e & F_BAD) return fail(err, E_CORRUPT, "png: undefined distance code");
        if (dist > (size_t)(out - dst)) return fail(err, E_CORRUPT, "png: a distance reaches before the first byte written");
        if (len > (size_t)(lim - out)) return fail(err, E_CORRUPT, "png: the stream holds more than height * (1 + row_bytes) bytes");
        out = copy_match(out, len, dist, (size_t)(lim - out));
    }
}

inline int inflate(const uint8_t* file, long n, uint8_t* dst, long dst_cap, fd_png_info* info, char* err) {
    if (!file || n < 0 || !dst || dst_cap < 0 || !info) return fail(err, E_ARGS, "fd_png_inflate: bad args");
    if (err) err[0] = 0;
    memset(info, 0, sizeof(*info));
    Header h;
    int st = parse(file, (size_t)n, h, err);
    if (st != OK) return st;
    fill_info(h, info);
    if (!h.covered) return E_UNCOVERED;                          // err holds the reason
    if (h.raw_bytes > dst_cap) return fail(err, E_CAPACITY, "fd_png_inflate: dst_cap is below height * (1 + row_bytes)");
    if (!h.first_idat) return fail(err, E_TRUNCATED, "png: the file ends before the first IDAT chunk");

    In in{file, (size_t)n, 0, 0, h.first_idat, 0, 0, 0, OK};
    const char* ends = "png: the IDAT data ends inside the stream";
    in.need(16);
    const uint32_t cmf = in.take(8), flg = in.take(8);
    if (in.cnt < 0) return fail(err, in.status == OK ? E_TRUNCATED : in.status, ends);
    if ((cmf & 15u) != 8 || (cmf >> 4) > 7) return fail(err, E_CORRUPT, "png: zlib header: not deflate with a window of at most 32 KiB");
    if (((cmf << 8) | flg) % 31u) return fail(err, E_CORRUPT, "png: zlib header: FCHECK fails");
    if (flg & 32u) return fail(err, E_CORRUPT, "png: zlib header: preset dictionary");

    uint8_t* out = dst;
    uint8_t* const lim = dst + h.raw_bytes;
    Tables t;
    t.fixed = 0;
    for (int last = 0; !last;) {
        in.need(3);
        last = (int)in.take(1);
        const uint32_t type = in.take(2);
        if (in.cnt < 0) return fail(err, E_TRUNCATED, ends);
        if (type == 3) return fail(err, E_CORRUPT, "png: block type 3");
        if (type == 0) {
            in.take(in.cnt & 7);
            in.need(32);
            const uint32_t len = in.take(16), nlen = in.take(16);
            if (in.cnt < 0) return fail(err, E_TRUNCATED, ends);
            if ((len ^ nlen) != 0xFFFFu) return fail(err, E_CORRUPT, "png: stored block: LEN and NLEN disagree");
            if (len > (size_t)(lim - out)) return fail(err, E_CORRUPT, "png: the stream holds more than height * (1 + row_bytes) bytes");
            uint32_t left = len;
            for (; left && in.cnt >= 8; --left) *out++ = (uint8_t)in.take(8);          // whole bytes the bit buffer already holds
            if (!in.cnt) in.buf = 0;                             // refill() leaves bits of the bytes at `pos` above cnt: pos moves below
            while (left) {
                if (in.pos == in.end && (in.eof || !in.next_chunk())) {
                    in.eof = 1;
                    return fail(err, E_TRUNCATED, ends);
                }
                const size_t run = in.end - in.pos < left ? in.end - in.pos : left;
                memcpy(out, file + in.pos, run);
                out += run;
                in.pos += run;
                left -= (uint32_t)run;
            }
            continue;
        }
        if (type == 1) {
            if (!t.fixed) {
                uint8_t lens[288 + 32];
                memset(lens, 8, 144);
                memset(lens + 144, 9, 112);
                memset(lens + 256, 7, 24);
                memset(lens + 280, 8, 8);
                memset(lens + 288, 5, 32);
                build(t.lit, LIT_CAP, LIT_BITS, lens, 288, K_LITLEN);
                build(t.dist, DIST_CAP, DIST_BITS, lens + 288, 32, K_DIST);
                t.fixed = 1;
            }
        } else {
            t.fixed = 0;
            in.need(14);
            const int nlit = 257 + (int)in.take(5), ndist = 1 + (int)in.take(5), ncl = 4 + (int)in.take(4);
            if (in.cnt < 0) return fail(err, E_TRUNCATED, ends);
            if (nlit > 286 || ndist > 30) return fail(err, E_CORRUPT, "png: dynamic block: too many length or distance codes");
            uint8_t lens[286 + 30];
            uint8_t cl[19] = {0};
            for (int i = 0; i < ncl; ++i) {
                in.need(3);
                cl[CL_ORDER[i]] = (uint8_t)in.take(3);
            }
            if (in.cnt < 0) return fail(err, E_TRUNCATED, ends);
            uint32_t clt[CL_CAP];
            if (build(clt, CL_CAP, 7, cl, 19, K_CODELEN) != OK) return fail(err, E_CORRUPT, "png: dynamic block: the code-length code is not a complete code");
            for (int i = 0; i < nlit + ndist;) {
                in.need(14);
                const uint32_t e = clt[(uint32_t)in.buf & 127u];
                in.take((int)(e & 255u));
                const int sym = (int)(e >> 16);
                int rep = 0, val = 0;
                if (!(e & F_BAD) && sym < 16) {
                    lens[i++] = (uint8_t)sym;
                } else if (!(e & F_BAD)) {
                    if (sym == 16) {
                        if (!i) return in.cnt < 0 ? fail(err, E_TRUNCATED, ends) : fail(err, E_CORRUPT, "png: dynamic block: repeat with no length before it");
                        val = lens[i - 1];
                        rep = 3 + (int)in.take(2);
                    } else if (sym == 17) {
                        rep = 3 + (int)in.take(3);
                    } else {
                        rep = 11 + (int)in.take(7);
                    }
                }
                if (in.cnt < 0) return fail(err, E_TRUNCATED, ends);
                if (e & F_BAD) return fail(err, E_CORRUPT, "png: dynamic block: undefined code-length code");
                if (i + rep > nlit + ndist) return fail(err, E_CORRUPT, "png: dynamic block: a repeat runs past the last code");
                for (; rep; --rep) lens[i++] = (uint8_t)val;
            }
            if (!lens[256]) return fail(err, E_CORRUPT, "png: dynamic block: no end-of-block code");
            if (build(t.lit, LIT_CAP, LIT_BITS, lens, nlit, K_LITLEN) != OK) return fail(err, E_CORRUPT, "png: dynamic block: the literal/length lengths are no Huffman code");
            if (build(t.dist, DIST_CAP, DIST_BITS, lens + nlit, ndist, K_DIST) != OK) return fail(err, E_CORRUPT, "png: dynamic block: the distance lengths are no Huffman code");
        }
        st = block(in, t, dst, out, lim, err);
        if (st != OK) return st;
    }
    if (out != lim) return fail(err, E_TRUNCATED, "png: the stream holds fewer than height * (1 + row_bytes) bytes");
    in.take(in.cnt & 7);
    uint32_t want = 0;
    for (int i = 0; i < 4; ++i) {
        in.need(8);
        want = (want << 8) | in.take(8);
    }
    if (in.cnt < 0) return fail(err, E_TRUNCATED, "png: the IDAT data ends inside the Adler-32 value");
    if (adler32(dst, (size_t)h.raw_bytes) != want) return fail(err, E_CORRUPT, "png: the scanlines fail the stream's Adler-32");
    const size_t stride = (size_t)h.row_bytes + 1;
    for (uint32_t y = 0; y < h.height; ++y)
        if (dst[y * stride] > 4) return fail(err, E_CORRUPT, "png: a scanline's filter type is above 4");
    // the rest of the IDAT run, then every chunk up to IEND: the file must reach its end marker
    size_t pos = in.next;
    for (;;) {
        if (n - (long)pos < 12) return fail(err, E_TRUNCATED, "png: the file ends before IEND");
        if (memcmp(file + pos + 4, "IEND", 4) == 0) {
            if (memcmp(file + pos, IEND, 12) != 0) return fail(err, E_CORRUPT, "png: IEND is not the 12 bytes it has to be");
            return OK;
        }
        const size_t len = be32(file + pos);
        if (len > (size_t)n - pos - 12) return fail(err, E_TRUNCATED, "png: the file ends before IEND");
        pos += 12 + len;
    }
}

}  // namespace fdpng
