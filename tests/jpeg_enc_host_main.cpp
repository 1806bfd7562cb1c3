// Stand-alone driver of the JPEG encoder's host code (fusiondepth_amd/csrc/jpeg_enc_host.h) for a sanitizer build - not a pytest:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I fusiondepth_amd/csrc \
//       tests/jpeg_enc_host_main.cpp -o jpeg_enc_host_main && ./jpeg_enc_host_main
// Every buffer is a heap block of exactly its size, so a read or write one element outside is a sanitizer report.  Checked: the
// quantisation tables of every quality (range, the formula, refusal outside 1 .. 100); the Huffman codes (complete up to the one
// reserved all-ones code, prefix-free by Kraft's sum, every Annex K symbol coded, a block's worst case inside FD_JPEG_ENC_BLOCK_BYTES);
// the header of 2000 seeded sizes and of the extreme ones (its length, its segment walk, nothing written into a buffer that is one
// byte short); the layout of 400 seeded batches and the extreme ones (regions in order and inside work, every image's stream inside
// the clear, the first-block / first-tile sums, refusal of a changed table and of short buffers).  Exit status 1 on a failed check.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jpeg_enc_host.h"

static int bad = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            bad = 1;                      \
        }                                 \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static void check_tables() {
    char err[fdjpegenc::ERR_LEN];
    for (int q = -2; q <= 103; ++q) {
        uint16_t* zz = (uint16_t*)malloc(128 * sizeof(uint16_t));
        memset(zz, 0xAB, 128 * sizeof(uint16_t));
        const int st = fdjpegenc::quant_tables(q, zz, err);
        if (q < 1 || q > 100) {
            CHECK(st != 0 && zz[0] == 0xABAB && zz[127] == 0xABAB, "quality %d was accepted", q);
        } else {
            CHECK(st == 0, "quality %d: %s", q, err);
            const long s = q < 50 ? 5000 / q : 200 - 2 * q;
            for (int k = 0; k < 128; ++k) {
                long v = ((long)fdjpegenc::QUANT_ZZ[k / 64][k % 64] * s + 50) / 100;
                v = v < 1 ? 1 : (v > 255 ? 255 : v);
                CHECK(zz[k] == v && zz[k] >= 1 && zz[k] <= 255, "quality %d entry %d: %d", q, k, zz[k]);
            }
        }
        free(zz);
    }
    CHECK(fdjpegenc::quant_tables(50, nullptr, err) != 0, "a null table was accepted");
    fdjpegenc::Tables* t = (fdjpegenc::Tables*)malloc(sizeof(fdjpegenc::Tables));
    CHECK(fdjpegenc::build_tables(92, t, err) == 0, "build_tables: %s", err);
    for (int k = 0; k < 2; ++k) {
        double kraft_dc = 0, kraft_ac = 0;
        int n_dc = 0, n_ac = 0, max_dc = 0, max_ac = 0;
        for (int s = 0; s < 16; ++s)
            if (t->dc_len[k][s]) {
                kraft_dc += 1.0 / (double)(1u << t->dc_len[k][s]);
                ++n_dc;
                max_dc = t->dc_len[k][s] > max_dc ? t->dc_len[k][s] : max_dc;
                CHECK(s < 12 && t->dc_code[k][s] < (1u << t->dc_len[k][s]), "DC table %d symbol %d", k, s);
            }
        for (int s = 0; s < 256; ++s)
            if (t->ac_len[k][s]) {
                kraft_ac += 1.0 / (double)(1u << t->ac_len[k][s]);
                ++n_ac;
                max_ac = t->ac_len[k][s] > max_ac ? t->ac_len[k][s] : max_ac;
                CHECK(t->ac_code[k][s] < (1u << t->ac_len[k][s]) - (t->ac_len[k][s] == 16 ? 1u : 0u), "AC table %d symbol %d", k, s);
                CHECK((s & 15) <= 10 && ((s & 15) != 0 || s == 0 || s == 0xF0), "AC table %d codes symbol %d", k, s);
            }
        CHECK(n_dc == 12 && n_ac == 162, "table %d: %d DC and %d AC symbols", k, n_dc, n_ac);
        CHECK(kraft_dc < 1.0 && kraft_ac < 1.0 && kraft_ac > 0.9999, "table %d: Kraft sums %f %f", k, kraft_dc, kraft_ac);
        // a block's worst case: the longest DC code and 11 value bits, 63 times the longest AC code and 10 value bits
        CHECK(max_dc + 11 + 63 * (max_ac + 10) <= 8 * FD_JPEG_ENC_BLOCK_BYTES, "table %d: a block may take %d bits", k, max_dc + 11 + 63 * (max_ac + 10));
        for (int i = 0; i < 64; ++i) CHECK(t->qt_nat[k][i] >= 1 && t->qt_nat[k][i] <= 255, "qt_nat %d %d", k, i);
    }
    int seen[64] = {0};
    for (int i = 0; i < 64; ++i) seen[fdjpegenc::NATURAL[i] & 63]++;
    for (int i = 0; i < 64; ++i) CHECK(seen[i] == 1, "NATURAL is no permutation at %d", i);
    free(t);
}

// the segment walk of a header: every marker and length, the last segment being SOS and ending at the header's end
static void check_header(int w, int h, int hs, int vs, int q) {
    char err[fdjpegenc::ERR_LEN];
    const int H = fdjpegenc::HEADER;
    uint8_t* buf = (uint8_t*)malloc((size_t)H);
    CHECK(fdjpegenc::header(w, h, hs, vs, q, buf, H, err) == 0, "header %dx%d: %s", w, h, err);
    CHECK(buf[0] == 0xFF && buf[1] == 0xD8, "no SOI");
    const int order[10] = {0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA, -1};
    int at = 2, k = 0;
    while (at + 4 <= H && order[k] >= 0) {
        CHECK(buf[at] == 0xFF && buf[at + 1] == order[k], "segment %d of %dx%d is %02x", k, w, h, buf[at + 1]);
        const int n = (buf[at + 2] << 8) | buf[at + 3];
        if (order[k] == 0xC0)
            CHECK(((buf[at + 5] << 8) | buf[at + 6]) == h && ((buf[at + 7] << 8) | buf[at + 8]) == w && buf[at + 11] == ((hs << 4) | vs), "SOF0 of %dx%d", w, h);
        at += 2 + n;
        ++k;
    }
    CHECK(at == H && order[k] < 0, "the segments of %dx%d end at %d", w, h, at);
    free(buf);
    uint8_t* small = (uint8_t*)malloc((size_t)H - 1);
    memset(small, 0x5A, (size_t)H - 1);
    CHECK(fdjpegenc::header(w, h, hs, vs, q, small, H - 1, err) != 0, "a short buffer was accepted");
    for (int i = 0; i < H - 1; ++i)
        if (small[i] != 0x5A) {
            CHECK(false, "a short buffer was written");
            break;
        }
    free(small);
}

static void check_batch(int N, bool extreme) {
    char err[fdjpegenc::ERR_LEN];
    fd_jpeg_enc_desc* desc = (fd_jpeg_enc_desc*)calloc((size_t)N, sizeof(fd_jpeg_enc_desc));
    for (int i = 0; i < N; ++i) {
        const int s = (int)(rnd() % 3);
        desc[i].src = (const void*)desc;                          // never read on the host
        desc[i].hs = s == 0 ? 1 : 2;
        desc[i].vs = s == 2 ? 2 : 1;
        desc[i].width = extreme ? (rnd() % 2 ? 65535 : 1) : 1 + (int)(rnd() % 700);
        desc[i].height = extreme ? (rnd() % 2 ? 65535 : 1) : 1 + (int)(rnd() % 400);
    }
    fd_jpeg_enc_sizes* sz = (fd_jpeg_enc_sizes*)malloc(sizeof(fd_jpeg_enc_sizes));
    const int st = fdjpegenc::layout(desc, N, sz, err);
    if (st != 0) {
        CHECK(extreme && strstr(err, "2^31"), "layout: %s", err);
    } else {
        long block = 0, tile = 0, out = 0;
        for (int i = 0; i < N; ++i) {
            const fd_jpeg_enc_desc& d = desc[i];
            CHECK(d.mcus_w == (d.width + 8 * d.hs - 1) / (8 * d.hs) && d.mcus_h == (d.height + 8 * d.vs - 1) / (8 * d.vs), "MCU grid of %d", i);
            CHECK(d.blocks == (long)d.mcus_w * d.mcus_h * (d.hs * d.vs + 2) && d.first_block == block && d.first_tile == tile, "blocks of %d", i);
            CHECK(d.raw_cap % FD_JPEG_ENC_TILE_BYTES == 0 && d.raw_cap >= d.blocks * FD_JPEG_ENC_BLOCK_BYTES + 8, "raw_cap of %d", i);
            CHECK(d.raw_off == sz->raw_off + tile * FD_JPEG_ENC_TILE_BYTES && d.raw_off % 16 == 0 && d.raw_off + d.raw_cap <= sz->work_bytes, "raw_off of %d", i);
            CHECK(d.out_cap == fdjpegenc::HEADER + 2 * d.blocks * FD_JPEG_ENC_BLOCK_BYTES + 2, "out_cap of %d", i);
            block += d.blocks;
            tile += d.raw_cap / FD_JPEG_ENC_TILE_BYTES;
            out += d.out_cap;
        }
        CHECK(sz->blocks == block && sz->tiles == tile && sz->out_bytes >= out && sz->out_bytes < out + 16, "sums");
        const long offs[10] = {0, sz->tab_off, sz->coef_off, sz->bits_off, sz->pos_off, sz->tile_off, sz->tilepos_off, sz->total_off, sz->result_off, sz->raw_off};
        const long need[9] = {(long)N * 96, (long)sizeof(fdjpegenc::Tables), block * 128, block * 4, block * 8, tile * 4, tile * 8, (long)N * 16, (long)N * 32};
        for (int k = 0; k < 9; ++k) CHECK(offs[k + 1] >= offs[k] + need[k] && offs[k + 1] % 16 == 0, "region %d", k);
        CHECK(sz->work_bytes == sz->raw_off + sz->raw_bytes && sz->raw_bytes == tile * FD_JPEG_ENC_TILE_BYTES, "work_bytes");
        fd_jpeg_enc_sizes again;
        CHECK(fdjpegenc::check_layout(desc, N, sz->work_bytes, sz->out_bytes, &again, err) == 0, "check_layout: %s", err);
        CHECK(memcmp(&again, sz, sizeof(again)) == 0, "check_layout computed other sizes");
        CHECK(fdjpegenc::check_layout(desc, N, sz->work_bytes - 1, sz->out_bytes, &again, err) != 0, "a short work was accepted");
        CHECK(fdjpegenc::check_layout(desc, N, sz->work_bytes, sz->out_bytes - 1, &again, err) != 0, "a short out was accepted");
        const int v = (int)(rnd() % (unsigned)N);
        fd_jpeg_enc_desc keep = desc[v];
        switch (rnd() % 5) {
            case 0: desc[v].first_block += 1; break;
            case 1: desc[v].raw_off -= 16; break;
            case 2: desc[v].width += 16; break;
            case 3: desc[v].src = nullptr; break;
            default: desc[v].raw_cap += FD_JPEG_ENC_TILE_BYTES; break;
        }
        CHECK(fdjpegenc::check_layout(desc, N, sz->work_bytes, sz->out_bytes, &again, err) != 0, "a changed table was accepted");
        desc[v] = keep;
    }
    free(sz);
    free(desc);
}

int main() {
    char err[fdjpegenc::ERR_LEN];
    check_tables();
    for (int k = 0; k < 2000; ++k) {
        const int s = (int)(rnd() % 3);
        check_header(1 + (int)(rnd() % 65535), 1 + (int)(rnd() % 65535), s == 0 ? 1 : 2, s == 2 ? 2 : 1, 1 + (int)(rnd() % 100));
    }
    check_header(1, 1, 1, 1, 1);
    check_header(65535, 65535, 2, 2, 100);
    uint8_t* buf = (uint8_t*)malloc((size_t)fdjpegenc::HEADER);
    const int refused[6][5] = {{0, 4, 2, 2, 50}, {4, 65536, 2, 2, 50}, {4, 4, 1, 2, 50}, {4, 4, 3, 1, 50}, {4, 4, 2, 2, 0}, {4, 4, 2, 2, 101}};
    for (int k = 0; k < 6; ++k)
        CHECK(fdjpegenc::header(refused[k][0], refused[k][1], refused[k][2], refused[k][3], refused[k][4], buf, fdjpegenc::HEADER, err) != 0,
              "header case %d was accepted", k);
    CHECK(fdjpegenc::header(4, 4, 2, 2, 50, nullptr, fdjpegenc::HEADER, err) != 0, "a null dst was accepted");
    free(buf);
    for (int k = 0; k < 400; ++k) check_batch(1 + (int)(rnd() % 40), false);
    for (int k = 0; k < 40; ++k) check_batch(1 + (int)(rnd() % 24), true);
    check_batch(65535, false);
    fd_jpeg_enc_sizes sz;
    fd_jpeg_enc_desc one;
    memset(&one, 0, sizeof(one));
    one.width = one.height = 8;
    one.hs = one.vs = 2;
    CHECK(fdjpegenc::layout(&one, 0, &sz, err) != 0 && fdjpegenc::layout(&one, 65536, &sz, err) != 0 && fdjpegenc::layout(nullptr, 1, &sz, err) != 0 &&
              fdjpegenc::layout(&one, 1, nullptr, err) != 0,
          "bad layout arguments were accepted");
    printf("jpeg_enc_host_main: 106 qualities, 2002 headers, 441 batches: %s\n", bad ? "FAILED" : "ok");
    return bad;
}
