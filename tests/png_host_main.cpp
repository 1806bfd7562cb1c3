// Stand-alone driver of the host PNG code (fusiondepth_amd/csrc/png_inflate.h) for a sanitizer build - not a pytest:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I fusiondepth_amd/csrc \
//       tests/png_host_main.cpp -o png_host_main && ./png_host_main file.png ...
// Each file named on the command line is probed and inflated whole, as every prefix and as 200 seeded single-byte corruptions.  Every
// input lives in a heap block of exactly its size and `dst` in a block of exactly dst_cap bytes, so a read or write one byte outside
// either is a sanitizer report.  Prints one line per file; exit status 1 when a whole covered file does not inflate, or a prefix does.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "png_inflate.h"

static int run(const uint8_t* src, size_t n, long cap, int* covered) {
    uint8_t* file = (uint8_t*)malloc(n ? n : 1);                  // exactly n bytes: the redzone starts right behind them
    memcpy(file, src, n);
    uint8_t* dst = (uint8_t*)malloc(cap ? (size_t)cap : 1);
    char err[fdpng::ERR_LEN];
    fd_png_info info;
    const int ps = fdpng::probe(file, (long)n, &info, err);
    if (covered) *covered = ps == 0 && info.covered;
    const int st = fdpng::inflate(file, (long)n, dst, cap, &info, err);
    free(dst);
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
        fd_png_info info;
        char err[fdpng::ERR_LEN];
        const int ps = fdpng::probe(data.data(), (long)data.size(), &info, err);
        const long cap = ps == 0 && info.covered ? info.raw_bytes : 64;
        int covered = 0;
        const int whole = run(data.data(), data.size(), cap, &covered);
        int by_status[7] = {0, 0, 0, 0, 0, 0, 0};
        for (size_t n = 0; n < data.size(); ++n) {
            const int st = run(data.data(), n, cap, nullptr);
            ++by_status[st];
            if (st == 0) bad = 1;                                 // only the whole file returns 0
        }
        uint64_t s = 0x9E3779B97F4A7C15ull ^ (uint64_t)data.size();
        for (int k = 0; k < 200 && !data.empty(); ++k) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            std::vector<uint8_t> c = data;
            c[(size_t)((s >> 33) % c.size())] ^= (uint8_t)(1 + ((s >> 12) % 255));
            ++by_status[run(c.data(), c.size(), cap, nullptr)];
            if (k % 4 == 0) ++by_status[run(c.data(), c.size(), cap > 64 ? cap - 64 : 0, nullptr)];      // and a capacity 64 bytes short
        }
        printf("%s: %zu bytes, covered %d, whole status %d; prefixes + corruptions by status:", argv[a], data.size(), covered, whole);
        for (int k = 0; k < 7; ++k) printf(" %d:%d", k, by_status[k]);
        printf("\n");
        if (covered && whole != 0) bad = 1;
    }
    return bad;
}
