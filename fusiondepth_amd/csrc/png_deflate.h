// The host half of the PNG encoder (include/fdhip.h, "PNG outputs"): the layout of the device buffers, the per-block Huffman plan
// and the CRC-32s.  Plain C++: no GPU call, no zlib, no globals but constant tables, no allocation, thread-safe, usable on a machine
// without a GPU (tests/png_enc_host_main.cpp runs it under the address and undefined-behaviour sanitizers).  tests/png_enc_ref.py
// restates every rule below in Python; tests/test_png_enc_cpu.py holds the two to each other field for field.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "fdhip.h"

namespace fdpngenc {

constexpr int ERR_LEN = 256;
constexpr int NSYM = 286;
constexpr int ROWS = FD_PNG_ENC_BLOCK_ROWS;
constexpr int GROUP = FD_PNG_ENC_GROUP_ROWS;
constexpr uint32_t ADLER = 65521u;
constexpr long FILE_FIXED = 57;                                  // signature 8, IHDR 25, IDAT length + type + CRC 12, IEND 12
constexpr long STREAM_AT = 8 + 25 + 8 + 2;                       // the first deflate byte of a file: behind the zlib header

inline int fail(char* err, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, ERR_LEN, fmt, ap);
    va_end(ap);
    return 1;
}

inline long round16(long v) { return (v + 15) / 16 * 16; }

// extra bits of the length symbols 257 .. 285
inline int len_extra(int k) { return k < 8 || k == 28 ? 0 : (k - 4) >> 2; }

// ---- layout ------------------------------------------------------------------------------------------------------------------
// The rule of include/fdhip.h for one descriptor's shape; nullptr when it holds.
inline const char* check_shape(const fd_png_enc_desc& d) {
    if (d.bpp != 1 && d.bpp != 2 && d.bpp != 3) return "bpp is none of 3 (RGB), 1 (grey), 2 (16-bit grey)";
    if (d.width < 1 || d.width > 65535 || d.height < 1 || d.height > 65535) return "width or height outside 1 .. 65535";
    if ((long)d.height * (1 + (long)d.width * d.bpp) > 0x7fffffffL) return "more than 2^31 - 1 scanline bytes in one frame";
    return nullptr;
}

// The one place the batch's layout is computed: the shapes checked, *sz filled from them, and per frame
// each(i, first_row, first_block, first_group, ws_off) - `layout` writes those into the table, `check_layout` compares the table with them.
template <class Each>
inline int walk_layout(const fd_png_enc_desc* desc, int N, fd_png_enc_sizes* sz, char* err, Each each) {
    if (!desc || !sz || N < 1 || N > 65535) return fail(err, "bad args");
    long rows = 0, blocks = 0, raw = 0;
    for (int i = 0; i < N; ++i) {
        const char* why = check_shape(desc[i]);
        if (why) return fail(err, "descriptor %d: %s", i, why);
        rows += desc[i].height;
        blocks += (desc[i].height + ROWS - 1) / ROWS;
        raw += (long)desc[i].height * (1 + (long)desc[i].width * desc[i].bpp);
        if (rows > 0x3fffffffL) return fail(err, "more than 2^30 - 1 scanlines in one batch");
    }
    sz->rows = rows;
    sz->blocks = blocks;
    sz->raw_bytes = raw;
    sz->stat_off = round16((long)N * (long)sizeof(fd_png_enc_desc));
    sz->stat_bytes = round16(blocks * FD_PNG_ENC_HIST * 4 + rows * 8);
    sz->rowbits_off = sz->stat_off + sz->stat_bytes;
    sz->table_off = sz->rowbits_off + round16(rows * 4);
    sz->ws_off = sz->table_off + blocks * (long)sizeof(fd_png_enc_block);
    long row = 0, block = 0, group = 0, at = sz->ws_off;
    for (int i = 0; i < N; ++i) {
        const int st = each(i, (int)row, (int)block, (int)group, at);
        if (st) return st;
        row += desc[i].height;
        block += (desc[i].height + ROWS - 1) / ROWS;
        group += (desc[i].height + GROUP - 1) / GROUP;
        at += round16((long)desc[i].height * (1 + (long)desc[i].width * desc[i].bpp));
    }
    sz->groups = group;
    sz->work_bytes = at;
    return 0;
}

inline int layout(fd_png_enc_desc* desc, int N, fd_png_enc_sizes* sz, char* err) {
    char why[ERR_LEN] = "";
    const int st = walk_layout(desc, N, sz, why, [&](int i, int row, int block, int group, long at) {
        desc[i].first_row = row;
        desc[i].first_block = block;
        desc[i].first_group = group;
        desc[i].ws_off = at;
        return 0;
    });
    return st ? fail(err, "fd_png_enc_layout: %.200s", why) : 0;
}

// The descriptors as `layout` leaves them, checked again: the launchers refuse a table that was changed in between.
inline int check_layout(const fd_png_enc_desc* desc, int N, long work_bytes, fd_png_enc_sizes* sz, char* err) {
    const int st = walk_layout(desc, N, sz, err, [&](int i, int row, int block, int group, long at) {
        if (!desc[i].src) return fail(err, "descriptor %d: src is null", i);
        if (desc[i].first_row != row || desc[i].first_block != block || desc[i].first_group != group || desc[i].ws_off != at)
            return fail(err, "descriptor %d: first_row / first_block / first_group / ws_off are not what fd_png_enc_layout wrote", i);
        return 0;
    });
    if (st) return st;
    if (work_bytes < sz->work_bytes) return fail(err, "work holds %ld bytes, the batch needs %ld", work_bytes, sz->work_bytes);
    return 0;
}

// ---- Huffman -----------------------------------------------------------------------------------------------------------------
// Code lengths of the symbols with a non-zero count, none above `limit`.  The two nodes of smallest (weight, id) are merged until
// one is left; a leaf's id is its symbol, the k-th merged node's is n + k.  (Leaves sorted by (weight, symbol) and the merged nodes
// in the order they were made are two queues whose heads hold those two nodes; on equal weights the leaf has the smaller id.)
// While the deepest leaf is deeper than `limit`, every weight w becomes (w + 1) >> 1 and the tree is built again.  One used symbol
// gets length 1.  n <= 286.
inline void code_lengths(const uint64_t* counts, int n, int limit, uint8_t* lens) {
    uint64_t w[NSYM];
    int leaf[NSYM], used = 0;
    for (int s = 0; s < n; ++s) {
        lens[s] = 0;
        if (counts[s]) {
            w[s] = counts[s];
            leaf[used++] = s;
        }
    }
    if (used == 1) lens[leaf[0]] = 1;
    if (used < 2) return;
    for (;;) {
        std::sort(leaf, leaf + used, [&](int a, int b) { return w[a] != w[b] ? w[a] < w[b] : a < b; });
        uint64_t nw[NSYM];                                       // merged node k: its weight, its parent (an index of a merged node)
        int nparent[NSYM], lparent[NSYM];
        int li = 0, ni = 0, made = 0;
        while (used - li + made - ni > 1) {
            uint64_t sum = 0;
            for (int k = 0; k < 2; ++k) {
                const bool take_leaf = li < used && (ni >= made || w[leaf[li]] <= nw[ni]);
                if (take_leaf) {
                    sum += w[leaf[li]];
                    lparent[li++] = made;
                } else {
                    sum += nw[ni];
                    nparent[ni++] = made;
                }
            }
            nw[made++] = sum;
        }
        int depth[NSYM], deepest = 0;
        depth[made - 1] = 0;
        for (int k = made - 2; k >= 0; --k) depth[k] = depth[nparent[k]] + 1;
        for (int k = 0; k < used; ++k) {
            const int d = depth[lparent[k]] + 1;
            lens[leaf[k]] = (uint8_t)(d > 255 ? 255 : d);
            deepest = d > deepest ? d : deepest;
        }
        if (deepest <= limit) return;
        for (int k = 0; k < used; ++k) w[leaf[k]] = (w[leaf[k]] + 1) >> 1;
    }
}

// The canonical code of every length, bit-reversed for LSB-first emission.
inline void canonical_codes(const uint8_t* lens, int n, uint16_t* codes) {
    unsigned code = 0;
    for (int s = 0; s < n; ++s) codes[s] = 0;
    for (int bits = 1; bits <= 15; ++bits) {
        for (int s = 0; s < n; ++s) {
            if (lens[s] != bits) continue;
            unsigned r = 0;
            for (int k = 0; k < bits; ++k) r |= ((code >> k) & 1u) << (bits - 1 - k);
            codes[s] = (uint16_t)r;
            ++code;
        }
        code <<= 1;
    }
}

struct BitWriter {
    uint32_t* words;
    unsigned n = 0;
    void put(unsigned v, unsigned bits) {                        // bits <= 16; the words were zeroed
        if (!bits) return;
        const uint64_t x = (uint64_t)v << (n & 31);
        words[n >> 5] |= (uint32_t)x;
        if ((n & 31) + bits > 32) words[(n >> 5) + 1] |= (uint32_t)(x >> 32);
        n += bits;
    }
};

// One block from its histogram (hist[0 .. 285] the literal/length counts without the end-of-block symbol, hist[286] its matches).
inline void plan_block(const uint32_t* hist, bool final, fd_png_enc_block* blk) {
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    memset(blk, 0, sizeof(*blk));
    uint64_t counts[NSYM];
    for (int s = 0; s < NSYM; ++s) counts[s] = hist[s];
    counts[256] = 1;
    const uint64_t matches = hist[286];
    code_lengths(counts, NSYM, 15, blk->len);
    canonical_codes(blk->len, NSYM, blk->code);
    int hlit = 257;
    for (int s = 257; s < NSYM; ++s)
        if (blk->len[s]) hlit = s + 1;
    const unsigned dist_len = matches ? 1u : 0u;
    // the greedy run-length form of the hlit + 1 code lengths (tests/png_enc_ref.py: code_length_sequence)
    uint8_t seq_len[NSYM + 1], sym[NSYM + 1], ebits[NSYM + 1], eval[NSYM + 1];
    const int total = hlit + 1;
    for (int s = 0; s < hlit; ++s) seq_len[s] = blk->len[s];
    seq_len[hlit] = (uint8_t)dist_len;
    int ns = 0;
    auto push = [&](int s, int eb, int ev) { sym[ns] = (uint8_t)s; ebits[ns] = (uint8_t)eb; eval[ns] = (uint8_t)ev; ++ns; };
    for (int i = 0; i < total;) {
        const int v = seq_len[i];
        int r = 1;
        while (i + r < total && seq_len[i + r] == v) ++r;
        i += r;
        if (v == 0) {
            while (r > 0) {
                int k = 1;
                if (r >= 11) {
                    k = r < 138 ? r : 138;
                    push(18, 7, k - 11);
                } else if (r >= 3) {
                    k = r;
                    push(17, 3, k - 3);
                } else {
                    push(0, 0, 0);
                }
                r -= k;
            }
        } else {
            push(v, 0, 0);
            --r;
            while (r >= 3) {
                const int k = r < 6 ? r : 6;
                push(16, 2, k - 3);
                r -= k;
            }
            for (; r > 0; --r) push(v, 0, 0);
        }
    }
    uint64_t cl_counts[19] = {0};
    for (int k = 0; k < ns; ++k) ++cl_counts[sym[k]];
    uint8_t cl_lens[19];
    uint16_t cl_codes[19];
    code_lengths(cl_counts, 19, 7, cl_lens);
    int cl_used = 0;
    for (int s = 0; s < 19; ++s) cl_used += cl_lens[s] != 0;
    if (cl_used == 1) cl_lens[cl_lens[0] == 0 ? 0 : 1] = 1;      // a code-length code of one code is incomplete: give it a second
    canonical_codes(cl_lens, 19, cl_codes);
    int hclen = 4;
    for (int k = 4; k < 19; ++k)
        if (cl_lens[order[k]]) hclen = k + 1;
    BitWriter w{blk->header};
    w.put(final ? 1u : 0u, 1);
    w.put(2, 2);
    w.put((unsigned)(hlit - 257), 5);
    w.put(0, 5);
    w.put((unsigned)(hclen - 4), 4);
    for (int k = 0; k < hclen; ++k) w.put(cl_lens[order[k]], 3);
    for (int k = 0; k < ns; ++k) {                               // at most 17 + 57 + 287 * 14 bits: inside FD_PNG_ENC_HEADER_WORDS
        w.put(cl_codes[sym[k]], cl_lens[sym[k]]);
        w.put(eval[k], ebits[k]);
    }
    blk->header_bits = w.n;
    blk->dist_len = dist_len;
    uint64_t bits = w.n + matches * dist_len;
    for (int s = 0; s < NSYM; ++s) bits += counts[s] * (uint64_t)(blk->len[s] + (s >= 257 ? len_extra(s - 257) : 0));
    blk->bits = bits;
}

// stats = what launch A wrote: uint32 [blocks][FD_PNG_ENC_HIST], then uint32 [rows][2].  Fills every block, and per descriptor
// adler, out_off and out_bytes (the files one behind the other from byte 0); *total_bytes = their sum.
inline int plan(fd_png_enc_desc* desc, int N, const uint32_t* stats, fd_png_enc_block* blocks, long* total_bytes, char* err) {
    fd_png_enc_sizes sz;
    if (!stats || !blocks || !total_bytes) return fail(err, "fd_png_enc_plan: bad args");
    char why[ERR_LEN];
    if (check_layout(desc, N, 0x7fffffffffffffffL, &sz, why)) return fail(err, "fd_png_enc_plan: %.200s", why);
    const uint32_t* adler = stats + sz.blocks * FD_PNG_ENC_HIST;
    long off = 0;
    for (int i = 0; i < N; ++i) {
        fd_png_enc_desc& d = desc[i];
        const int nb = (d.height + ROWS - 1) / ROWS;
        uint64_t at = 0;
        for (int k = 0; k < nb; ++k) {
            fd_png_enc_block* blk = blocks + d.first_block + k;
            plan_block(stats + (long)(d.first_block + k) * FD_PNG_ENC_HIST, k == nb - 1, blk);
            blk->bit_off = at;
            at += blk->bits;
        }
        const uint64_t p = (1 + (uint64_t)d.width * d.bpp) % ADLER;
        uint64_t a = 1, b = 0;
        for (int r = 0; r < d.height; ++r) {
            const uint32_t* pr = adler + 2 * (long)(d.first_row + r);
            b = (b + p * a + pr[1] % ADLER) % ADLER;
            a = (a + pr[0] % ADLER) % ADLER;
        }
        d.adler = (uint32_t)((b << 16) | a);
        d.stream_bits = (long)at;
        d.out_off = off;
        d.out_bytes = FILE_FIXED + 2 + (long)((at + 7) / 8) + 4;
        if (d.out_bytes - FILE_FIXED > 0x7fffffffL) return fail(err, "fd_png_enc_plan: frame %d: an IDAT chunk of more than 2^31 - 1 bytes", i);
        off += d.out_bytes;
    }
    *total_bytes = off;
    return 0;
}

// ---- CRC-32 ------------------------------------------------------------------------------------------------------------------
struct CrcTables {
    uint32_t t[8][256];
    CrcTables() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
            t[0][i] = c;
        }
        for (int j = 1; j < 8; ++j)
            for (uint32_t i = 0; i < 256; ++i) t[j][i] = (t[j - 1][i] >> 8) ^ t[0][t[j - 1][i] & 255u];
    }
};

inline uint32_t crc32(const uint8_t* p, size_t n) {              // eight bytes a step
    static const CrcTables T;
    uint32_t c = 0xFFFFFFFFu;
    for (; n >= 8; n -= 8, p += 8) {
        const uint32_t lo = ((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24) ^ c;
        const uint32_t hi = (uint32_t)p[4] | (uint32_t)p[5] << 8 | (uint32_t)p[6] << 16 | (uint32_t)p[7] << 24;
        c = T.t[7][lo & 255u] ^ T.t[6][(lo >> 8) & 255u] ^ T.t[5][(lo >> 16) & 255u] ^ T.t[4][lo >> 24] ^ T.t[3][hi & 255u] ^
            T.t[2][(hi >> 8) & 255u] ^ T.t[1][(hi >> 16) & 255u] ^ T.t[0][hi >> 24];
    }
    for (; n; --n, ++p) c = (c >> 8) ^ T.t[0][(c ^ *p) & 255u];
    return ~c;
}

inline void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

// The three CRC-32 fields of the file of descriptor `d` inside files[0 .. nbytes): IHDR's, IDAT's and IEND's.
inline int finish(uint8_t* files, long nbytes, const fd_png_enc_desc* d, char* err) {
    if (!files || !d) return fail(err, "fd_png_enc_finish: bad args");
    if (d->out_off < 0 || d->out_bytes < FILE_FIXED + 6 || d->out_bytes > nbytes || d->out_off > nbytes - d->out_bytes)
        return fail(err, "fd_png_enc_finish: the file leaves the buffer");
    uint8_t* f = files + d->out_off;
    const long zlen = d->out_bytes - FILE_FIXED;
    put_be32(f + 29, crc32(f + 12, 17));
    put_be32(f + 41 + zlen, crc32(f + 37, (size_t)(4 + zlen)));
    put_be32(f + d->out_bytes - 4, crc32(f + d->out_bytes - 8, 4));
    return 0;
}

}  // namespace fdpngenc
