// The host half of the JPEG encoder (include/fdhip.h, "JPEG outputs"): the quantisation tables of a quality, the Huffman codes of the
// Annex K tables, a file's header bytes and the layout of a batch.  Plain C++: no GPU call, no globals but constant tables, no
// allocation, thread-safe, usable on a machine without a GPU (tests/jpeg_enc_host_main.cpp runs it under the address and
// undefined-behaviour sanitizers).  tests/jpeg_enc_ref.py restates every rule in Python; tests/test_jpeg_enc_cpu.py holds the two to
// each other.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fdhip.h"

namespace fdjpegenc {

constexpr int ERR_LEN = 256;
constexpr int HEADER = FD_JPEG_ENC_HEADER_BYTES;
constexpr long BLOCK_BYTES = FD_JPEG_ENC_BLOCK_BYTES;            // 22 bits of DC + 63 * 26 bits of AC = 1660 bits, rounded up to 16 bytes
constexpr long TILE = FD_JPEG_ENC_TILE_BYTES;

inline int fail(char* err, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, ERR_LEN, fmt, ap);
    va_end(ap);
    return 1;
}

inline long round16(long v) { return (v + 15) / 16 * 16; }

// zigzag position -> natural (row-major) index, and back
static const uint8_t NATURAL[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K, in zigzag order
static const uint8_t QUANT_ZZ[2][64] = {
    {16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24,  22,  22,  24,  49, 35, 37,  29,  40,  58,  51,  61, 60,  57,  51,
     56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99},
    {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
static const uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
static const uint8_t AC_VALS[2][162] = {
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177,
     193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,
     56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106,
     115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
     164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
     212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193,
     9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,
     55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105,
     106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
     162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
     210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};

// What the kernels read: the quantisation tables in natural order and the codes by symbol (length 0: the symbol has no code).
struct Tables {
    uint16_t qt_nat[2][64];
    uint16_t dc_code[2][16];
    uint8_t dc_len[2][16];
    uint16_t ac_code[2][256];
    uint8_t ac_len[2][256];
};
static_assert(sizeof(Tables) == 1888 && sizeof(Tables) % 16 == 0, "the kernels copy the tables 16 bytes at a time");

// ---- rule 4 --------------------------------------------------------------------------------------------------------------------
inline int quant_tables(int quality, uint16_t* zz, char* err) {
    if (!zz || quality < 1 || quality > 100) return fail(err, "fd_jpeg_enc_quant_tables: quality %d outside 1 .. 100", quality);
    const long s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) {
            long v = ((long)QUANT_ZZ[t][k] * s + 50) / 100;
            zz[t * 64 + k] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
    return 0;
}

// BITS and HUFFVAL -> code and length by symbol; `n` symbols, the tables of `size` entries.
inline void huffman_codes(const uint8_t* bits, const uint8_t* vals, int n, uint16_t* code, uint8_t* len, int size) {
    for (int s = 0; s < size; ++s) code[s] = len[s] = 0;
    unsigned c = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1] && k < n; ++i, ++k, ++c) {
            if (vals[k] < size) {
                code[vals[k]] = (uint16_t)c;
                len[vals[k]] = (uint8_t)l;
            }
        }
        c <<= 1;
    }
}

inline int build_tables(int quality, Tables* t, char* err) {
    uint16_t zz[128];
    if (quant_tables(quality, zz, err)) return 1;
    static const uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    for (int k = 0; k < 2; ++k) {
        for (int i = 0; i < 64; ++i) t->qt_nat[k][NATURAL[i]] = zz[k * 64 + i];
        huffman_codes(DC_BITS[k], DC_VALS, 12, t->dc_code[k], t->dc_len[k], 16);
        huffman_codes(AC_BITS[k], AC_VALS[k], 162, t->ac_code[k], t->ac_len[k], 256);
    }
    return 0;
}

// ---- rule 7 --------------------------------------------------------------------------------------------------------------------
inline const char* check_sampling(int hs, int vs) {
    return (hs == 1 && vs == 1) || (hs == 2 && (vs == 1 || vs == 2)) ? nullptr : "sampling is none of 1x1, 2x1, 2x2";
}

// The HEADER bytes of a file; nothing is written when dst_bytes is smaller.
inline int header(int width, int height, int hs, int vs, int quality, uint8_t* dst, long dst_bytes, char* err) {
    if (!dst || dst_bytes < HEADER) return fail(err, "fd_jpeg_enc_header: dst holds %ld bytes, a header takes %d", dst ? dst_bytes : 0L, HEADER);
    if (width < 1 || width > 65535 || height < 1 || height > 65535) return fail(err, "fd_jpeg_enc_header: width or height outside 1 .. 65535");
    if (check_sampling(hs, vs)) return fail(err, "fd_jpeg_enc_header: %s", check_sampling(hs, vs));
    uint16_t zz[128];
    if (quant_tables(quality, zz, err)) return 1;
    uint8_t buf[HEADER];                                          // built here, copied whole: a short dst is never touched
    int at = 0;
    auto put = [&](int v) { buf[at++] = (uint8_t)v; };
    auto marker = [&](int m, int body) {
        put(0xFF);
        put(m);
        put((body + 2) >> 8);
        put((body + 2) & 255);
    };
    put(0xFF);
    put(0xD8);
    marker(0xE0, 14);
    const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int i = 0; i < 14; ++i) put(jfif[i]);
    for (int t = 0; t < 2; ++t) {
        marker(0xDB, 65);
        put(t);
        for (int k = 0; k < 64; ++k) put(zz[t * 64 + k]);
    }
    marker(0xC0, 15);
    const int sof[15] = {8, height >> 8, height & 255, width >> 8, width & 255, 3, 1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1};
    for (int i = 0; i < 15; ++i) put(sof[i]);
    for (int t = 0; t < 2; ++t) {
        marker(0xC4, 1 + 16 + 12);
        put(t);
        for (int i = 0; i < 16; ++i) put(DC_BITS[t][i]);
        for (int i = 0; i < 12; ++i) put(i);
        marker(0xC4, 1 + 16 + 162);
        put(0x10 | t);
        for (int i = 0; i < 16; ++i) put(AC_BITS[t][i]);
        for (int i = 0; i < 162; ++i) put(AC_VALS[t][i]);
    }
    marker(0xDA, 10);
    const int sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    for (int i = 0; i < 10; ++i) put(sos[i]);
    if (at != HEADER) return fail(err, "fd_jpeg_enc_header: built %d bytes", at);
    memcpy(dst, buf, HEADER);
    return 0;
}

// ---- layout --------------------------------------------------------------------------------------------------------------------
struct Geometry {
    int mcus_w, mcus_h;
    long blocks, raw_cap, out_cap;
};

inline const char* geometry(const fd_jpeg_enc_desc& d, Geometry* g) {
    if (d.width < 1 || d.width > 65535 || d.height < 1 || d.height > 65535) return "width or height outside 1 .. 65535";
    if (check_sampling(d.hs, d.vs)) return check_sampling(d.hs, d.vs);
    g->mcus_w = (d.width + 8 * d.hs - 1) / (8 * d.hs);
    g->mcus_h = (d.height + 8 * d.vs - 1) / (8 * d.vs);
    g->blocks = (long)g->mcus_w * g->mcus_h * (d.hs * d.vs + 2);
    g->raw_cap = (g->blocks * BLOCK_BYTES + 8 + TILE - 1) / TILE * TILE;      // 8: the word behind a stream's last is never the next image's
    g->out_cap = HEADER + 2 * g->blocks * BLOCK_BYTES + 2;
    return nullptr;
}

// The one place the batch's layout is computed: *sz from the shapes, and per image each(i, geometry, first_block, first_tile, raw_off).
template <class Each>
inline int walk_layout(const fd_jpeg_enc_desc* desc, int N, fd_jpeg_enc_sizes* sz, char* err, Each each) {
    if (!desc || !sz || N < 1 || N > 65535) return fail(err, "bad args (1 <= N <= 65535)");
    long blocks = 0, tiles = 0, out = 0;
    Geometry g;
    for (int i = 0; i < N; ++i) {
        const char* why = geometry(desc[i], &g);
        if (why) return fail(err, "descriptor %d: %s", i, why);
        blocks += g.blocks;
        tiles += g.raw_cap / TILE;
        out += g.out_cap;
        if (blocks > 0x7fffffffL) return fail(err, "more than 2^31 - 1 blocks in one batch");
    }
    memset(sz, 0, sizeof(*sz));
    sz->blocks = blocks;
    sz->tiles = tiles;
    sz->tab_off = round16((long)N * (long)sizeof(fd_jpeg_enc_desc));
    sz->coef_off = sz->tab_off + (long)sizeof(Tables);
    sz->bits_off = sz->coef_off + blocks * 128;
    sz->pos_off = sz->bits_off + round16(blocks * 4);
    sz->tile_off = sz->pos_off + round16(blocks * 8);
    sz->tilepos_off = sz->tile_off + round16(tiles * 4);
    sz->total_off = sz->tilepos_off + round16(tiles * 8);
    sz->result_off = sz->total_off + (long)N * 16;
    sz->result_bytes = (long)N * (long)sizeof(fd_jpeg_enc_result);
    sz->raw_off = sz->result_off + sz->result_bytes;
    sz->raw_bytes = tiles * TILE;
    sz->work_bytes = sz->raw_off + sz->raw_bytes;
    sz->out_bytes = round16(out);
    long block = 0, tile = 0;
    for (int i = 0; i < N; ++i) {
        geometry(desc[i], &g);
        const int st = each(i, g, block, tile, sz->raw_off + tile * TILE);
        if (st) return st;
        block += g.blocks;
        tile += g.raw_cap / TILE;
    }
    return 0;
}

inline int layout(fd_jpeg_enc_desc* desc, int N, fd_jpeg_enc_sizes* sz, char* err) {
    char why[ERR_LEN] = "";
    const int st = walk_layout(desc, N, sz, why, [&](int i, const Geometry& g, long block, long tile, long raw_off) {
        desc[i].mcus_w = g.mcus_w;
        desc[i].mcus_h = g.mcus_h;
        desc[i].blocks = g.blocks;
        desc[i].raw_cap = g.raw_cap;
        desc[i].out_cap = g.out_cap;
        desc[i].first_block = block;
        desc[i].first_tile = tile;
        desc[i].raw_off = raw_off;
        return 0;
    });
    return st ? fail(err, "fd_jpeg_enc_layout: %.200s", why) : 0;
}

// The descriptors as `layout` leaves them, checked again: the launcher refuses a table that was changed in between.
inline int check_layout(const fd_jpeg_enc_desc* desc, int N, long work_bytes, long out_bytes, fd_jpeg_enc_sizes* sz, char* err) {
    const int st = walk_layout(desc, N, sz, err, [&](int i, const Geometry& g, long block, long tile, long raw_off) {
        const fd_jpeg_enc_desc& d = desc[i];
        if (!d.src) return fail(err, "descriptor %d: src is null", i);
        if (d.mcus_w != g.mcus_w || d.mcus_h != g.mcus_h || d.blocks != g.blocks || d.raw_cap != g.raw_cap || d.out_cap != g.out_cap ||
            d.first_block != block || d.first_tile != tile || d.raw_off != raw_off)
            return fail(err, "descriptor %d: the layout fields are not what fd_jpeg_enc_layout wrote", i);
        return 0;
    });
    if (st) return st;
    if (work_bytes < sz->work_bytes) return fail(err, "work holds %ld bytes, the batch needs %ld", work_bytes, sz->work_bytes);
    if (out_bytes < sz->out_bytes) return fail(err, "out holds %ld bytes, the batch may need %ld", out_bytes, sz->out_bytes);
    return 0;
}

}  // namespace fdjpegenc
