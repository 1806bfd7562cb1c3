// Stand-alone driver of the encoder's host code (fusiondepth_amd/csrc/png_deflate.h) for a sanitizer build - not a pytest:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I fusiondepth_amd/csrc \
//       tests/png_enc_host_main.cpp -o png_enc_host_main && ./png_enc_host_main [histograms.bin]
// histograms.bin (`python tests/png_enc_fixtures.py histograms.bin` writes the fixtures'): uint32 n, then n x FD_PNG_ENC_HIST uint32.
// Every histogram - those of the file, 2000 seeded random ones, and the degenerate ones (all zero, one symbol, every count at
// INT_MAX / 286 and at 2^32 - 1, Fibonacci counts, powers of two) - is planned as the only block of a frame and as one of sixteen
// blocks of a taller frame (a frame whose stream would pass 2^31 - 1 bytes is refused by the plan: those go through plan_block
// alone); each plan is checked (a complete code of at most 15 / 7 bits, a header inside its words, the size formula) and every buffer
// is a heap block of exactly its size, so a read or write one element outside is a sanitizer report.  fd_png_enc_finish runs on
// files of every length around its eight-byte step, against a bit-by-bit CRC-32.  Exit status 1 on a failed check.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "png_deflate.h"

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

static uint32_t crc_slow(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

static void check_block(const fd_png_enc_block& b, const uint32_t* hist, const char* what, int idx) {
    double kraft = 0;
    uint64_t bits = b.header_bits;
    int used = 0;
    for (int s = 0; s < 286; ++s) {
        const uint64_t c = s == 256 ? 1 : hist[s];
        CHECK((c != 0) == (b.len[s] != 0), "%s %d: symbol %d count %llu length %d", what, idx, s, (unsigned long long)c, b.len[s]);
        CHECK(b.len[s] <= 15, "%s %d: length %d", what, idx, b.len[s]);
        if (b.len[s]) {
            kraft += 1.0 / (double)(1u << b.len[s]);
            ++used;
            CHECK(b.code[s] < (1u << b.len[s]), "%s %d: code of symbol %d wider than its length", what, idx, s);
        }
        bits += c * (uint64_t)(b.len[s] + (s >= 257 ? fdpngenc::len_extra(s - 257) : 0));
    }
    bits += (uint64_t)hist[286] * b.dist_len;
    CHECK(used == 1 ? kraft == 0.5 : kraft == 1.0, "%s %d: the code is not complete (%f)", what, idx, kraft);
    CHECK(b.header_bits >= 17 + 12 && b.header_bits <= 32u * FD_PNG_ENC_HEADER_WORDS, "%s %d: header of %u bits", what, idx, b.header_bits);
    for (unsigned k = b.header_bits; k < 32u * FD_PNG_ENC_HEADER_WORDS; ++k)
        if ((b.header[k >> 5] >> (k & 31)) & 1u) {
            CHECK(false, "%s %d: a bit behind the header", what, idx);
            break;
        }
    CHECK(bits == b.bits, "%s %d: bits %llu, formula %llu", what, idx, (unsigned long long)b.bits, (unsigned long long)bits);
    CHECK(b.dist_len == (hist[286] ? 1u : 0u), "%s %d: dist_len", what, idx);
    CHECK(((b.header[0] >> 1) & 3u) == 2u, "%s %d: BTYPE", what, idx);
}

// `hists` as the blocks of frames: each alone (height 1), then sixteen at a time as the blocks of one taller frame
static void run(const std::vector<uint32_t>& hists, const char* what) {
    const int n = (int)(hists.size() / FD_PNG_ENC_HIST);
    char err[fdpngenc::ERR_LEN];
    for (int pass = 0; pass < 2; ++pass) {
        const int per = pass == 0 ? 1 : 16;
        const int N = (n + per - 1) / per;
        fd_png_enc_desc* desc = (fd_png_enc_desc*)calloc((size_t)N, sizeof(fd_png_enc_desc));
        for (int i = 0; i < N; ++i) {
            const int nb = i < N - 1 ? per : n - per * (N - 1);
            desc[i].src = (const void*)desc;                      // never read on the host
            desc[i].width = 1 + (int)(rnd() % 700);
            desc[i].bpp = 1 + (int)(rnd() % 3);
            desc[i].height = 64 * (nb - 1) + 1 + (int)(rnd() % 64);
        }
        fd_png_enc_sizes sz;
        CHECK(fdpngenc::layout(desc, N, &sz, err) == 0, "%s: layout: %s", what, err);
        CHECK(sz.blocks == n, "%s: %ld blocks for %d histograms", what, sz.blocks, n);
        uint32_t* stats = (uint32_t*)malloc((size_t)(sz.blocks * FD_PNG_ENC_HIST + 2 * sz.rows) * 4);   // exactly what the plan reads
        memcpy(stats, hists.data(), hists.size() * 4);
        for (long r = 0; r < 2 * sz.rows; ++r) stats[sz.blocks * FD_PNG_ENC_HIST + r] = r % 7 == 0 ? 0xFFFFFFFFu : rnd();
        fd_png_enc_block* blocks = (fd_png_enc_block*)malloc((size_t)sz.blocks * sizeof(fd_png_enc_block));
        long total = 0;
        CHECK(fdpngenc::plan(desc, N, stats, blocks, &total, err) == 0, "%s: plan: %s", what, err);
        long at = 0;
        for (int i = 0; i < N; ++i) {
            uint64_t bit = 0;
            const int nb = (desc[i].height + 63) / 64;
            for (int k = 0; k < nb; ++k) {
                const fd_png_enc_block& b = blocks[desc[i].first_block + k];
                check_block(b, stats + (long)(desc[i].first_block + k) * FD_PNG_ENC_HIST, what, desc[i].first_block + k);
                CHECK(b.bit_off == bit, "%s: bit_off of block %d", what, k);
                CHECK((b.header[0] & 1u) == (k == nb - 1 ? 1u : 0u), "%s: BFINAL of block %d", what, k);
                bit += b.bits;
            }
            CHECK(desc[i].stream_bits == (long)bit && desc[i].out_off == at && desc[i].out_bytes == 57 + 2 + (long)((bit + 7) / 8) + 4,
                  "%s: file %d", what, i);
            CHECK((desc[i].adler & 0xFFFFu) < 65521u && (desc[i].adler >> 16) < 65521u, "%s: adler of file %d", what, i);
            at += desc[i].out_bytes;
        }
        CHECK(total == at, "%s: total", what);
        free(blocks);
        free(stats);
        free(desc);
    }
}

int main(int argc, char** argv) {
    std::vector<uint32_t> file;
    if (argc > 1) {
        FILE* fh = fopen(argv[1], "rb");
        uint32_t n = 0;
        if (!fh || fread(&n, 4, 1, fh) != 1) {
            fprintf(stderr, "%s: cannot read\n", argv[1]);
            return 2;
        }
        file.resize((size_t)n * FD_PNG_ENC_HIST);
        if (fread(file.data(), 4, file.size(), fh) != file.size()) {
            fprintf(stderr, "%s: short\n", argv[1]);
            return 2;
        }
        fclose(fh);
        run(file, "file");
    }
    std::vector<uint32_t> random;
    for (int k = 0; k < 2000; ++k) {
        std::vector<uint32_t> h(FD_PNG_ENC_HIST, 0);
        const int used = 1 + (int)(rnd() % 286), shape = (int)(rnd() % 4);
        for (int j = 0; j < used; ++j) {
            const int s = (int)(rnd() % 286);
            h[s] = shape == 0 ? 1 + rnd() % 8 : (shape == 1 ? 1u << (rnd() % 16) : (shape == 2 ? rnd() % 100000 : 1 + rnd() % 60000));
        }
        h[256] = rnd();                                           // ignored: the plan sets end-of-block to 1
        h[286] = rnd() % 3 ? rnd() % 1000000 : 0;
        random.insert(random.end(), h.begin(), h.end());
    }
    run(random, "random");
    // the degenerate ones: each through plan_block; those whose stream stays below 2^31 bytes also as frames
    std::vector<uint32_t> odd;
    int degenerate = 0;
    auto add = [&](const std::vector<uint32_t>& h, bool small = true) {
        fd_png_enc_block* b = (fd_png_enc_block*)malloc(sizeof(fd_png_enc_block));
        fdpngenc::plan_block(h.data(), degenerate % 2 == 0, b);
        check_block(*b, h.data(), "plan_block", degenerate++);
        free(b);
        if (small) odd.insert(odd.end(), h.begin(), h.end());
    };
    std::vector<uint32_t> h(FD_PNG_ENC_HIST, 0);
    add(h);                                                       // all zero: end-of-block alone
    h[0] = 1;
    add(h);
    h.assign(FD_PNG_ENC_HIST, (uint32_t)(INT_MAX / 286));
    add(h, false);
    h.assign(FD_PNG_ENC_HIST, 0xFFFFFFFFu);
    add(h, false);
    h.assign(FD_PNG_ENC_HIST, 0);
    uint32_t f0 = 1, f1 = 1;
    for (int s = 0; s < 46; ++s) {
        h[5 * s] = f0;
        const uint32_t f2 = f0 + f1;
        f0 = f1;
        f1 = f2;
    }
    add(h, false);
    h.assign(FD_PNG_ENC_HIST, 0);
    for (int s = 0; s < 200; ++s) h[s] = 1u << ((s * 7) % 10 * 2);
    add(h);
    h.assign(FD_PNG_ENC_HIST, 0);
    h[0] = 3;
    h[285] = h[286] = 40;
    add(h);
    run(odd, "degenerate");

    // fd_png_enc_finish: files of every stream length 0 .. 40 at odd offsets, in a buffer of exactly their size
    for (long zextra = 0; zextra <= 40; ++zextra) {
        fd_png_enc_desc d;
        memset(&d, 0, sizeof(d));
        d.out_off = 3 + zextra % 5;
        d.out_bytes = 57 + 6 + zextra;
        const long nbytes = d.out_off + d.out_bytes;
        uint8_t* buf = (uint8_t*)malloc((size_t)nbytes);
        for (long i = 0; i < nbytes; ++i) buf[i] = (uint8_t)rnd();
        std::vector<uint8_t> before(buf, buf + nbytes);
        char err[fdpngenc::ERR_LEN];
        CHECK(fdpngenc::finish(buf, nbytes, &d, err) == 0, "finish: %s", err);
        uint8_t* f = buf + d.out_off;
        const long zlen = d.out_bytes - 57;
        auto be = [](const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; };
        CHECK(be(f + 29) == crc_slow(f + 12, 17), "finish: IHDR's CRC");
        CHECK(be(f + 41 + zlen) == crc_slow(f + 37, (size_t)(4 + zlen)), "finish: IDAT's CRC at stream length %ld", zlen);
        CHECK(be(f + d.out_bytes - 4) == crc_slow(f + d.out_bytes - 8, 4), "finish: IEND's CRC");
        long changed = 0;
        for (long i = 0; i < nbytes; ++i) changed += buf[i] != before[(size_t)i];
        CHECK(changed <= 12, "finish: wrote %ld bytes", changed);
        d.out_bytes += 1;                                         // one byte past the buffer: refused, nothing written
        CHECK(fdpngenc::finish(buf, nbytes, &d, err) != 0, "finish: a file that leaves the buffer was accepted");
        free(buf);
    }
    printf("png_enc_host_main: %zu file, 2000 random and 7 degenerate histograms, 41 files: %s\n", file.size() / FD_PNG_ENC_HIST,
           bad ? "FAILED" : "ok");
    return bad;
}
