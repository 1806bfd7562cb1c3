// Stand-alone driver of the host entropy decoder (fusiondepth_amd/csrc/jpeg_entropy.h) for a sanitizer build - not a pytest:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I fusiondepth_amd/csrc \
//       tests/jpeg_host_main.cpp -o jpeg_host_main && ./jpeg_host_main file.jpg ...
// Each file named on the command line is probed and decoded whole, as every prefix and as 200 seeded single-byte corruptions.  Every
// input lives in a heap block of exactly its size and the coefficients in a block of exactly coef_cap values, so a read or write one
// byte outside either is a sanitizer report.  Prints one line per file; exit status 1 when a whole file does not decode.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jpeg_entropy.h"

static int run(const uint8_t* src, size_t n, long cap, int* covered) {
    uint8_t* file = (uint8_t*)malloc(n ? n : 1);                  // exactly n bytes: the redzone starts right behind them
    memcpy(file, src, n);
    int16_t* coef = (int16_t*)malloc(cap ? (size_t)cap * 2 : 1);
    uint16_t* qt = (uint16_t*)malloc(192 * 2);
    char err[fdjpeg::ERR_LEN];
    fd_jpeg_info info;
    const int ps = fdjpeg::probe(file, (long)n, &info, err);
    if (covered) *covered = ps == 0 && info.covered;
    const int st = fdjpeg::entropy_decode(file, (long)n, coef, cap, qt, &info, err);
    free(qt);
    free(coef);
    free(file);
    return st;
}

int main(int argc, char** argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* fh = fopen(argv[a], "rb");
        if (!fh) {
            fprintf(stderr, "%s: cannot open\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> data;
        uint8_t chunk[4096];
        size_t got;
        while ((got = fread(chunk, 1, sizeof(chunk), fh)) > 0) data.insert(data.end(), chunk, chunk + got);
        fclose(fh);
        fd_jpeg_info info;
        char err[fdjpeg::ERR_LEN];
        const int ps = fdjpeg::probe(data.data(), (long)data.size(), &info, err);
        const long cap = ps == 0 && info.covered ? info.coef_count : 64;
        int covered = 0;
        const int whole = run(data.data(), data.size(), cap, &covered);
        int by_status[7] = {0, 0, 0, 0, 0, 0, 0};
        for (size_t n = 0; n < data.size(); ++n) ++by_status[run(data.data(), n, cap, nullptr)];
        uint64_t s = 0x9E3779B97F4A7C15ull ^ (uint64_t)data.size();
        for (int k = 0; k < 200 && !data.empty(); ++k) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            std::vector<uint8_t> c = data;
            c[(size_t)((s >> 33) % c.size())] ^= (uint8_t)(1 + ((s >> 12) % 255));
            ++by_status[run(c.data(), c.size(), cap, nullptr)];
            if (k % 4 == 0) ++by_status[run(c.data(), c.size(), cap > 64 ? cap - 64 : 0, nullptr)];      // and a capacity one block short
        }
        printf("%s: %zu bytes, covered %d, whole status %d; prefixes + corruptions by status:", argv[a], data.size(), covered, whole);
        for (int k = 0; k < 7; ++k) printf(" %d:%d", k, by_status[k]);
        printf("\n");
        if (covered && whole != 0) bad = 1;
    }
    return bad;
}
