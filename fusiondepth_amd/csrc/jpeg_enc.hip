// JPEG outputs (include/fdhip.h, "JPEG outputs"): the C ABI of the host half (csrc/jpeg_enc_host.h) and the seven launches of the encoder.
// Bytes and integer arithmetic throughout; every shared word is combined with an integer atomic, so two calls give the same bytes.
//   k_jpeg_enc_blocks   a wave per 8 blocks in scan order, a lane per row (then per column) of a block: colour, edges, chroma
//                       downsample, forward DCT, quantisation; int16 coefficients in zigzag order, 16 bytes a lane.
//   k_jpeg_enc_bits     a lane per block: the bits its tokens take.
//   k_jpeg_enc_scan     a workgroup per image: exclusive scan of 32-bit counts into 64-bit offsets, and their sum.
//   k_jpeg_enc_emit     a lane per block: the tokens ORed into the cleared stream, 32 bits at a time.
//   k_jpeg_enc_ffcount  a workgroup per tile of the filled stream: its FF bytes.   (k_jpeg_enc_scan again over the tiles.)
//   k_jpeg_enc_stuff    a workgroup per tile: the stuffed bytes behind the room for the header, FF D9, the image's result row.
#include "fd_common.h"
#include "fdhip.h"
#include "jpeg_enc_host.h"

extern "C" int fd_jpeg_enc_quant_tables(int quality, unsigned short* zigzag) {
    char err[fdjpegenc::ERR_LEN] = "";
    const int st = fdjpegenc::quant_tables(quality, zigzag, err);
    if (st != 0) fd_set_error("%s", err);
    return st;
}

extern "C" int fd_jpeg_enc_header(int width, int height, int hs, int vs, int quality, unsigned char* dst, long dst_bytes) {
    char err[fdjpegenc::ERR_LEN] = "";
    const int st = fdjpegenc::header(width, height, hs, vs, quality, dst, dst_bytes, err);
    if (st != 0) fd_set_error("%s", err);
    return st;
}

extern "C" int fd_jpeg_enc_layout(fd_jpeg_enc_desc* desc, int N, fd_jpeg_enc_sizes* sizes) {
    char err[fdjpegenc::ERR_LEN] = "";
    const int st = fdjpegenc::layout(desc, N, sizes, err);
    if (st != 0) fd_set_error("%s", err);
    return st;
}

namespace {

using fdjpegenc::Tables;
constexpr int TILE = FD_JPEG_ENC_TILE_BYTES;
constexpr int HEADER = FD_JPEG_ENC_HEADER_BYTES;
constexpr int BLOCKS_PER_WG = 32;                                // k_jpeg_enc_blocks: 4 waves of 8 blocks
constexpr int SCAN_THREADS = 1024;

__constant__ unsigned char ZIGZAG_OF[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                            41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                            46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// The image that holds batch-wide index `g` of a per-image run whose first index `first(d)` grows with the image: the last one whose
// first index is not above g.
template <class First>
__device__ __forceinline__ int find_image(const fd_jpeg_enc_desc* desc, int N, long g, First first) {
    int lo = 0, hi = N - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first(desc[mid]) <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void load_tables(Tables* dst, const unsigned char* work, long tab_off) {
    const uint4* src = reinterpret_cast<const uint4*>(work + tab_off);
    uint4* d = reinterpret_cast<uint4*>(dst);
    for (int i = threadIdx.x; i < (int)(sizeof(Tables) / 16); i += blockDim.x) d[i] = src[i];
}

// ---- A: rules 1 to 5 ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ycc(const unsigned char* p, int comp) {
    const int r = p[0], g = p[1], b = p[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// sample (yy, xx) of component `comp`'s own plane, the edge rules applied; every pixel read lies inside the image
__device__ __forceinline__ int sample(const fd_jpeg_enc_desc& d, const unsigned char* src, int comp, int yy, int xx) {
    const int W = d.width, H = d.height;
    if (comp == 0 || d.hs == 1) {
        const int sy = min(yy, H - 1), sx = min(xx, W - 1);
        return ycc(src + ((long)sy * W + sx) * 3, comp);
    }
    const int x0 = min(2 * xx, W - 1), x1 = min(2 * xx + 1, W - 1);
    if (d.vs == 1) {
        const unsigned char* row = src + (long)min(yy, H - 1) * W * 3;
        return (ycc(row + 3L * x0, comp) + ycc(row + 3L * x1, comp) + (xx & 1)) >> 1;
    }
    const int i = min(yy, (H + 1) / 2 - 1);                      // the last DOWNSAMPLED row is the one that is replicated
    const unsigned char* r0 = src + (long)(2 * i) * W * 3;
    const unsigned char* r1 = src + (long)min(2 * i + 1, H - 1) * W * 3;
    return (ycc(r0 + 3L * x0, comp) + ycc(r0 + 3L * x1, comp) + ycc(r1 + 3L * x0, comp) + ycc(r1 + 3L * x1, comp) + 1 + (xx & 1)) >> 2;
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of the accurate integer forward DCT over eight values, in place
template <bool FIRST>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
    constexpr int SH = FIRST ? 13 - 2 : 13 + 2;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) * 4;
        d[4] = (t10 - t11) * 4;
    } else {
        d[0] = descale(t10 + t11, 2);
        d[4] = descale(t10 - t11, 2);
    }
    int z1 = (t12 + t13) * 4433;
    d[2] = descale(z1 + t13 * 6270, SH);
    d[6] = descale(z1 - t12 * 15137, SH);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = descale(a4 + z1 + z3, SH);
    d[5] = descale(a5 + z2 + z4, SH);
    d[3] = descale(a6 + z2 + z3, SH);
    d[1] = descale(a7 + z1 + z4, SH);
}

__global__ __launch_bounds__(64 * BLOCKS_PER_WG / 8) void k_jpeg_enc_blocks(unsigned char* __restrict__ work, int N, long tab_off, long coef_off,
                                                                            long total_blocks) {
    __shared__ int pass[BLOCKS_PER_WG][8][9];
    __shared__ __attribute__((aligned(16))) short zz[BLOCKS_PER_WG][64];
    __shared__ unsigned short qt[2][64];
    const fd_jpeg_enc_desc* desc = reinterpret_cast<const fd_jpeg_enc_desc*>(work);
    for (int i = threadIdx.x; i < 128; i += blockDim.x) qt[i >> 6][i & 63] = reinterpret_cast<const Tables*>(work + tab_off)->qt_nat[i >> 6][i & 63];
    const int slot = (int)(threadIdx.x >> 3), r = (int)(threadIdx.x & 7);
    const long gb = (long)blockIdx.x * BLOCKS_PER_WG + slot;
    const bool live = gb < total_blocks;
    int comp = 0;
    bool dc_only = false;
    if (live) {
        const fd_jpeg_enc_desc& d = desc[find_image(desc, N, gb, [](const fd_jpeg_enc_desc& e) { return e.first_block; })];
        const int ny = d.hs * d.vs, per = ny + 2;
        const long b = gb - d.first_block, mcu = b / per;
        const int k = (int)(b % per), my = (int)(mcu / d.mcus_w), mx = (int)(mcu % d.mcus_w);
        int by = my, bx = mx;
        if (k < ny) {
            by = my * d.vs + k / d.hs;
            bx = mx * d.hs + k % d.hs;
            const int bw = (d.width + 7) / 8, bh = (d.height + 7) / 8;
            if (by >= bh) {                                      // rule 5, a dummy row: the LAST block of the row above in this MCU
                dc_only = true;
                by -= 1;
                bx = mx * d.hs + d.hs - 1;
            }
            if (bx >= bw) {                                      // a right-edge dummy: the block to its left
                dc_only = true;
                bx -= 1;
            }
        } else {
            comp = 1 + (k - ny);
        }
        int v[8];
        const unsigned char* src = reinterpret_cast<const unsigned char*>(d.src);
#pragma unroll
        for (int x = 0; x < 8; ++x) v[x] = sample(d, src, comp, by * 8 + r, bx * 8 + x) - 128;
        fdct8<true>(v);
#pragma unroll
        for (int x = 0; x < 8; ++x) pass[slot][r][x] = v[x];
    }
    __syncthreads();
    if (live) {
        int v[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) v[y] = pass[slot][y][r];
        fdct8<false>(v);
        const unsigned short* q = qt[comp ? 1 : 0];
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const int nat = y * 8 + r;
            const unsigned t = q[nat];
            const unsigned a = (unsigned)abs(v[y]) + 4u * t;
            int c = (int)(a / (8u * t));
            c = v[y] < 0 ? -c : c;
            if (dc_only && nat != 0) c = 0;
            zz[slot][ZIGZAG_OF[nat]] = (short)c;
        }
    }
    __syncthreads();
    if (live) reinterpret_cast<uint4*>(work + coef_off)[gb * 8 + r] = reinterpret_cast<const uint4*>(&zz[slot][0])[r];
}

// ---- B and D: one block's tokens ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int category(int v) { return v ? 32 - __clz(abs(v)) : 0; }
__device__ __forceinline__ unsigned low_bits(int v, int n) { return (unsigned)(v < 0 ? v - 1 : v) & ((1u << n) - 1u); }

// The block before `b` (inside the image) of the same component in scan order; -1: none, the predictor is 0.
__device__ __forceinline__ long predecessor(const fd_jpeg_enc_desc& d, long b, int& table) {
    const int ny = d.hs * d.vs, per = ny + 2;
    const int k = (int)(b % per);
    table = k < ny ? 0 : 1;
    if (k > 0 && k < ny) return b - 1;
    if (b < per) return -1;
    return k == 0 ? b - 3 : b - per;                             // the last luma block of the MCU before, or the same chroma block there
}

// on(code, length) for every token of the block, in order; `c` = its 64 coefficients in zigzag order
// An AC value never reaches category 11, for which the tables hold no code: a sample minus 128 lies in [-128, 127], so an AC term of
// the true DCT is at most 128 / 4 * (sum over x of |cos((2x + 1) u pi / 16)|)^2 <= 32 * 5.13^2 < 843 in magnitude, the integer transform
// adds a few units of rounding to eight times that, and the quantiser divides by 8 t with t >= 1: |AC| <= 1023, category 10 at most.
// (The DC difference reaches category 11; the DC tables code it.)
template <class On>
__device__ __forceinline__ void for_tokens(const short (&c)[64], int pred, const Tables& t, int table, On on) {
    const int diff = (int)c[0] - pred;
    int n = category(diff);
    on((unsigned)t.dc_code[table][n], (unsigned)t.dc_len[table][n]);
    on(low_bits(diff, n), (unsigned)n);
    const unsigned short* code = t.ac_code[table];
    const unsigned char* len = t.ac_len[table];
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = c[k];
        if (v == 0) {
            ++run;
        } else {
            for (; run > 15; run -= 16) on((unsigned)code[0xF0], (unsigned)len[0xF0]);
            n = category(v);
            const int s = ((run << 4) | n) & 255;
            on((unsigned)code[s], (unsigned)len[s]);
            on(low_bits(v, n), (unsigned)n);
            run = 0;
        }
    }
    if (run) on((unsigned)code[0], (unsigned)len[0]);
}

__device__ __forceinline__ void load_block(const unsigned char* work, long coef_off, long gb, short (&c)[64]) {
    const uint4* src = reinterpret_cast<const uint4*>(work + coef_off) + gb * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 q = src[i];
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c[i * 8 + 2 * j] = (short)(w[j] & 0xffffu);
            c[i * 8 + 2 * j + 1] = (short)(w[j] >> 16);
        }
    }
}

__global__ __launch_bounds__(256) void k_jpeg_enc_bits(unsigned char* __restrict__ work, int N, long tab_off, long coef_off, long bits_off,
                                                       long total_blocks) {
    __shared__ __attribute__((aligned(16))) Tables tab;      // load_tables stores 16 bytes at a time
    const fd_jpeg_enc_desc* desc = reinterpret_cast<const fd_jpeg_enc_desc*>(work);
    load_tables(&tab, work, tab_off);
    __syncthreads();
    const long gb = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gb >= total_blocks) return;
    const fd_jpeg_enc_desc& d = desc[find_image(desc, N, gb, [](const fd_jpeg_enc_desc& e) { return e.first_block; })];
    int table;
    const long p = predecessor(d, gb - d.first_block, table);
    const int pred = p < 0 ? 0 : (int)reinterpret_cast<const short*>(work + coef_off)[(d.first_block + p) * 64];
    short c[64];
    load_block(work, coef_off, gb, c);
    unsigned bits = 0;
    for_tokens(c, pred, tab, table, [&](unsigned, unsigned n) { bits += n; });
    reinterpret_cast<unsigned*>(work + bits_off)[gb] = bits;
}

// ---- C: exclusive scan per image ------------------------------------------------------------------------------------------------
// which = 0: the image's blocks (counts at cnt_off, one per block); which = 1: its tiles.  pos[first + i] = the sum of the counts
// before i inside the image; totals[2 * image + which] = the sum of all.
__global__ __launch_bounds__(SCAN_THREADS) void k_jpeg_enc_scan(unsigned char* __restrict__ work, long cnt_off, long pos_off, long total_off, int which) {
    __shared__ unsigned long long wave_sum[SCAN_THREADS / 64];
    __shared__ unsigned long long carry;
    const fd_jpeg_enc_desc& d = reinterpret_cast<const fd_jpeg_enc_desc*>(work)[blockIdx.x];
    const long first = which == 0 ? d.first_block : d.first_tile;
    const long n = which == 0 ? d.blocks : d.raw_cap / TILE;
    const unsigned* cnt = reinterpret_cast<const unsigned*>(work + cnt_off) + first;
    unsigned long long* pos = reinterpret_cast<unsigned long long*>(work + pos_off) + first;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (long base = 0; base < n; base += SCAN_THREADS) {
        const long i = base + threadIdx.x;
        const unsigned long long mine = i < n ? cnt[i] : 0ull;
        unsigned long long incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long o = __shfl_up(incl, off, 64);
            incl += lane >= off ? o : 0ull;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        unsigned long long before = carry;
        for (int w = 0; w < wave; ++w) before += wave_sum[w];
        if (i < n) pos[i] = before + incl - mine;
        __syncthreads();
        if (threadIdx.x == SCAN_THREADS - 1) carry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) reinterpret_cast<unsigned long long*>(work + total_off)[2 * blockIdx.x + which] = carry;
}

// ---- D: emission ----------------------------------------------------------------------------------------------------------------
// The cleared streams as 32-bit words, and the room of the one image a lane may write to.  Bit 0 of the stream is the most
// significant bit of byte 0, so a word holds its 32 bits byte-swapped.
struct Sink {
    unsigned* words;             // the image's stream
    unsigned long long nwords;   // its room
    // the low `bits` (1 .. 32) bits of v at bit `at`; nothing outside the room is touched
    __device__ __forceinline__ void put(unsigned long long at, unsigned v, unsigned bits) const {
        const unsigned long long w = at >> 5;
        if (!bits || w + 1 >= nwords) return;
        const unsigned long long x = (unsigned long long)v << (64u - bits - (unsigned)(at & 31ull));
        const unsigned hi = (unsigned)(x >> 32), lo = (unsigned)x;
        if (hi) atomicOr(words + w, __builtin_bswap32(hi));
        if (lo) atomicOr(words + w + 1, __builtin_bswap32(lo));
    }
};

__global__ __launch_bounds__(256) void k_jpeg_enc_emit(unsigned char* __restrict__ work, int N, long tab_off, long coef_off, long pos_off,
                                                       long total_blocks) {
    __shared__ __attribute__((aligned(16))) Tables tab;      // load_tables stores 16 bytes at a time
    const fd_jpeg_enc_desc* desc = reinterpret_cast<const fd_jpeg_enc_desc*>(work);
    load_tables(&tab, work, tab_off);
    __syncthreads();
    const long gb = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gb >= total_blocks) return;
    const fd_jpeg_enc_desc& d = desc[find_image(desc, N, gb, [](const fd_jpeg_enc_desc& e) { return e.first_block; })];
    int table;
    const long p = predecessor(d, gb - d.first_block, table);
    const int pred = p < 0 ? 0 : (int)reinterpret_cast<const short*>(work + coef_off)[(d.first_block + p) * 64];
    short c[64];
    load_block(work, coef_off, gb, c);
    Sink sink;
    sink.words = reinterpret_cast<unsigned*>(work + d.raw_off);
    sink.nwords = (unsigned long long)d.raw_cap / 4ull;
    unsigned long long at = reinterpret_cast<const unsigned long long*>(work + pos_off)[gb];
    unsigned long long acc = 0;                                  // the newest bits lowest; `held` of them wait
    unsigned held = 0;
    for_tokens(c, pred, tab, table, [&](unsigned v, unsigned n) {
        acc = (acc << n) | v;                                    // held <= 31 and n <= 16: never more than 47 bits
        held += n;
        if (held >= 32u) {
            held -= 32u;
            sink.put(at, (unsigned)(acc >> held), 32u);
            at += 32ull;
            acc &= (1ull << held) - 1ull;
        }
    });
    sink.put(at, (unsigned)acc, held);
}

// ---- E: fill, stuffing, FF D9 ---------------------------------------------------------------------------------------------------
// The 16 bytes at byte `at` (a multiple of 16) of an image's stream of `bits` bits, its last byte filled with one-bits; `valid` = how
// many of them belong to the stream.
__device__ __forceinline__ uint4 filled16(const unsigned char* raw, unsigned long long at, unsigned long long bits, int& valid) {
    const unsigned long long nbytes = (bits + 7ull) >> 3;
    valid = at >= nbytes ? 0 : (nbytes - at < 16ull ? (int)(nbytes - at) : 16);
    uint4 q = make_uint4(0, 0, 0, 0);
    if (valid == 0) return q;
    q = *reinterpret_cast<const uint4*>(raw + at);
    if ((bits & 7ull) && nbytes - 1ull - at < 16ull) {
        const unsigned k = (unsigned)(nbytes - 1ull - at);
        const unsigned fill = (0xFFu >> (unsigned)(bits & 7ull)) << (8u * (k & 3u));
        unsigned* w = &q.x;
        w[k >> 2] |= fill;
    }
    return q;
}

__device__ __forceinline__ unsigned byte_of(const uint4& q, int k) {
    const unsigned w = k < 8 ? (k < 4 ? q.x : q.y) : (k < 12 ? q.z : q.w);
    return (w >> (8 * (k & 3))) & 255u;
}

struct TileOf {
    int image;
    long tile;                   // inside the image
};

__device__ __forceinline__ TileOf find_tile(const fd_jpeg_enc_desc* desc, int N) {
    TileOf t;
    t.image = find_image(desc, N, (long)blockIdx.x, [](const fd_jpeg_enc_desc& e) { return e.first_tile; });
    t.tile = (long)blockIdx.x - desc[t.image].first_tile;
    return t;
}

__global__ __launch_bounds__(TILE / 16) void k_jpeg_enc_ffcount(unsigned char* __restrict__ work, int N, long total_off, long tile_off) {
    __shared__ unsigned part[TILE / 16 / 64];
    const fd_jpeg_enc_desc* desc = reinterpret_cast<const fd_jpeg_enc_desc*>(work);
    const TileOf t = find_tile(desc, N);
    const fd_jpeg_enc_desc& d = desc[t.image];
    const unsigned long long bits = reinterpret_cast<const unsigned long long*>(work + total_off)[2 * t.image];
    int valid;
    const uint4 q = filled16(work + d.raw_off, (unsigned long long)t.tile * TILE + 16ull * threadIdx.x, bits, valid);
    unsigned n = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) n += (k < valid && byte_of(q, k) == 255u) ? 1u : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) reinterpret_cast<unsigned*>(work + tile_off)[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(TILE / 16) void k_jpeg_enc_stuff(unsigned char* __restrict__ work, int N, long total_off, long tilepos_off, long result_off,
                                                              unsigned char* __restrict__ out, long out_bytes) {
    __shared__ unsigned long long red[TILE / 16 / 64];
    __shared__ unsigned wave_ff[TILE / 16 / 64];
    const fd_jpeg_enc_desc* desc = reinterpret_cast<const fd_jpeg_enc_desc*>(work);
    const unsigned long long* totals = reinterpret_cast<const unsigned long long*>(work + total_off);
    const TileOf t = find_tile(desc, N);
    const fd_jpeg_enc_desc& d = desc[t.image];
    const unsigned long long bits = totals[2 * t.image], nbytes = (bits + 7ull) >> 3;
    if ((unsigned long long)t.tile * TILE >= nbytes) return;     // the whole workgroup: a tile behind the stream
    // the file's first byte: the sizes of the files before it
    unsigned long long before = 0;
    for (int j = threadIdx.x; j < t.image; j += blockDim.x) before += HEADER + ((totals[2 * j] + 7ull) >> 3) + totals[2 * j + 1] + 2ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off, 64);
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    if (lane == 0) red[wave] = before;
    int valid;
    const unsigned long long at = (unsigned long long)t.tile * TILE + 16ull * threadIdx.x;
    const uint4 q = filled16(work + d.raw_off, at, bits, valid);
    unsigned mine = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) mine += (k < valid && byte_of(q, k) == 255u) ? 1u : 0u;
    unsigned incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_up(incl, off, 64);
        incl += lane >= off ? o : 0u;
    }
    if (lane == 63) wave_ff[wave] = incl;
    __syncthreads();
    const unsigned long long file = red[0] + red[1] + red[2] + red[3];
    unsigned ff = incl - mine;
    for (int w = 0; w < wave; ++w) ff += wave_ff[w];
    const unsigned long long stuffed = totals[2 * t.image + 1];
    const unsigned long long file_bytes = HEADER + nbytes + stuffed + 2ull;
    if (file + file_bytes > (unsigned long long)out_bytes) return;                 // never, with out sized by the layout
    unsigned char* dst = out + file + HEADER;
    unsigned long long o = at + reinterpret_cast<const unsigned long long*>(work + tilepos_off)[blockIdx.x] + ff;
    for (int k = 0; k < valid; ++k) {
        const unsigned b = byte_of(q, k);
        dst[o++] = (unsigned char)b;
        if (b == 255u) dst[o++] = 0;
    }
    if (valid > 0 && at + (unsigned)valid == nbytes) {           // the lane with the stream's last byte
        dst[o] = 0xFF;
        dst[o + 1] = 0xD9;
        fd_jpeg_enc_result* res = reinterpret_cast<fd_jpeg_enc_result*>(work + result_off) + t.image;
        res->out_off = (long)file;
        res->out_bytes = (long)file_bytes;
        res->stream_bits = (long)bits;
        res->stuffed = (long)stuffed;
    }
}

}  // namespace

extern "C" int fd_jpeg_enc_encode(void* work, long work_bytes, const fd_jpeg_enc_desc* desc, int N, int quality, unsigned char* out, long out_bytes,
                                  void* stream) {
    FD_REQUIRE(work && desc && out && ((uintptr_t)work & 15) == 0, "fd_jpeg_enc_encode: bad args (work must be 16-byte aligned)");
    fd_jpeg_enc_sizes sz;
    char err[fdjpegenc::ERR_LEN] = "";
    FD_REQUIRE(fdjpegenc::check_layout(desc, N, work_bytes, out_bytes, &sz, err) == 0, "fd_jpeg_enc_encode: %s", err);
    Tables tab;
    FD_REQUIRE(fdjpegenc::build_tables(quality, &tab, err) == 0, "fd_jpeg_enc_encode: %s", err);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* w = (unsigned char*)work;
    hipError_t e = hipMemcpyAsync(w, desc, (size_t)N * sizeof(fd_jpeg_enc_desc), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(w + sz.tab_off, &tab, sizeof(tab), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(w + sz.raw_off, 0, (size_t)sz.raw_bytes, st);
    FD_REQUIRE(e == hipSuccess, "fd_jpeg_enc_encode: copy or clear failed: %s", hipGetErrorString(e));
    const unsigned per_block = (unsigned)fd_cdiv(sz.blocks, 256);
    hipLaunchKernelGGL(k_jpeg_enc_blocks, dim3((unsigned)fd_cdiv(sz.blocks, BLOCKS_PER_WG)), dim3(64 * BLOCKS_PER_WG / 8), 0, st, w, N, sz.tab_off,
                       sz.coef_off, sz.blocks);
    FD_LAUNCH_CHECK("k_jpeg_enc_blocks");
    hipLaunchKernelGGL(k_jpeg_enc_bits, dim3(per_block), dim3(256), 0, st, w, N, sz.tab_off, sz.coef_off, sz.bits_off, sz.blocks);
    FD_LAUNCH_CHECK("k_jpeg_enc_bits");
    hipLaunchKernelGGL(k_jpeg_enc_scan, dim3((unsigned)N), dim3(SCAN_THREADS), 0, st, w, sz.bits_off, sz.pos_off, sz.total_off, 0);
    FD_LAUNCH_CHECK("k_jpeg_enc_scan");
    hipLaunchKernelGGL(k_jpeg_enc_emit, dim3(per_block), dim3(256), 0, st, w, N, sz.tab_off, sz.coef_off, sz.pos_off, sz.blocks);
    FD_LAUNCH_CHECK("k_jpeg_enc_emit");
    hipLaunchKernelGGL(k_jpeg_enc_ffcount, dim3((unsigned)sz.tiles), dim3(TILE / 16), 0, st, w, N, sz.total_off, sz.tile_off);
    FD_LAUNCH_CHECK("k_jpeg_enc_ffcount");
    hipLaunchKernelGGL(k_jpeg_enc_scan, dim3((unsigned)N), dim3(SCAN_THREADS), 0, st, w, sz.tile_off, sz.tilepos_off, sz.total_off, 1);
    FD_LAUNCH_CHECK("k_jpeg_enc_scan");
    hipLaunchKernelGGL(k_jpeg_enc_stuff, dim3((unsigned)sz.tiles), dim3(TILE / 16), 0, st, w, N, sz.total_off, sz.tilepos_off, sz.result_off, out,
                       out_bytes);
    FD_LAUNCH_CHECK("k_jpeg_enc_stuff");
    return 0;
}
