// FD_HIPCC_FLAGS: -ffp-contract=off
// Raw Velodyne scan -> sparse LiDAR scan (reference sparsify/sparsify.py:32-136: gen_sparse_points + pto_ang_map), for S scans in
// one call.  include/fdhip.h states the arithmetic; in short: a filter box, an angular cell per point (float32 up to the two
// arcsines, float64 after them, as numpy 2 evaluates the reference's expression), the LAST point of a cell wins it, and the
// winners of the selected rows leave in raster order as their original 16 bytes.
//
// Compiled with -ffp-contract=off and spelled with the *_rn intrinsics: x*x + y*y + z*z is three roundings and two more, never
// a fused multiply-add.  The square roots are plain sqrtf, which hipcc rounds correctly by default
// (-fhip-fp32-correctly-rounded-divide-sqrt); HIP's __fsqrt_rn is the hardware approximation, one spacing off often enough to
// turn y / r = -1 into a NaN.  arcsin is evaluated in double on the float32 quotient and rounded once to float32 (numpy's
// float32 arcsin is a few spacings off the correctly rounded value and cannot be matched bit for bit; only points within a few
// spacings of a bin edge can land in the neighbouring cell).
//
// Passes (every launch covers all S scans: grid.y or a search in the offsets table, so the launch count does not depend on S)
//   cells     per point: filter, cell, atomicMax(point index + 1) into the scan's winners table [n_rows * W] (integer, order
//             independent => run-to-run identical)
//   count     per 1024-cell chunk: occupied cells
//   gather    per chunk: its output base = the sum of the chunks before it (fixed order), ranks by wave ballot, one float4 per
//             lane from the winner to its slot; slots past the scan's count are filled with (-1, 0, 0, 0)
// random-sample mode runs count / gather over the compacted list again: n_keep (non-zero float64 norm), then the kept ones.
#include "../../include/fdhip.h"
#include "fd_common.h"

namespace {

constexpr int CHUNK = 1024;              // cells per block in count / gather: 256 threads x 4
constexpr int MAX_H = 1024;              // rows of the angular grid (the row -> output slot table lives in LDS)
typedef unsigned long long u64;

struct RowList { int n; int rows[FD_SPARSIFY_MAX_ROWS]; };

struct CellArgs {
    const float4* pts; const int* off; long total; int S, H, W, cap;
    float x_lo, x_hi, y_lo, y_hi, z_lo, z_hi;
    double rad45, rad2, dphi, dtheta;
};

// int(angle / step) of numpy's float64 -> int64 cast (truncation; NaN and out-of-range give INT64_MIN), then the clamp
__device__ __forceinline__ int bin_of(double angle, double step, int n) {
    const double q = angle / step;
    if (!(q >= 0.0)) return 0;                                            // negative, or NaN
    if (q >= (double)n) return n - 1;
    return (int)q;
}

__global__ void __launch_bounds__(256) k_sp_cells(CellArgs a, RowList rl, unsigned* __restrict__ win, int* __restrict__ cells) {
    __shared__ short slot_of[MAX_H];
    for (int t = threadIdx.x; t < a.H; t += 256) slot_of[t] = -1;
    __syncthreads();
    if ((int)threadIdx.x < rl.n) slot_of[rl.rows[threadIdx.x]] = (short)threadIdx.x;
    __syncthreads();
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.total) return;
    int lo = 0, hi = a.S;                                                 // the scan of point i: the last s with off[s] <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long)a.off[mid] <= i) lo = mid; else hi = mid;
    }
    const long first = a.off[lo];
    if (i < first || i >= (long)a.off[lo + 1]) {                          // an offsets table that does not cover the points
        if (cells) cells[i] = -1;
        return;
    }
    const float4 p = a.pts[i];
    const float x = p.x, y = p.y, z = p.z;
    if (!(x >= a.x_lo && x < a.x_hi && y >= a.y_lo && y < a.y_hi && z >= a.z_lo && z < a.z_hi)) {
        if (cells) cells[i] = -1;
        return;
    }
    const float rr = __fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y));
    const float dd = __fadd_rn(rr, __fmul_rn(z, z));
    float d = sqrtf(dd), r = sqrtf(rr);                                   // correctly rounded: see the note above
    if (d == 0.f) d = 0.000001f;
    if (r == 0.f) r = 0.000001f;
    const float ay = (float)asin((double)__fdiv_rn(y, r));
    const float az = (float)asin((double)__fdiv_rn(z, d));
    const int col = bin_of(a.rad45 - (double)ay, a.dphi, a.W);
    const int row = bin_of(a.rad2 - (double)az, a.dtheta, a.H);
    if (cells) cells[i] = row * a.W + col;
    const int slot = slot_of[row];
    if (slot >= 0) atomicMax(&win[(long)lo * a.cap + (long)slot * a.W + col], (unsigned)(i - first) + 1u);
}

// ------------------------------------------------------------------------------------------------ ordered compaction
// One list of `cap` entries per scan, three uses (STAGE):
//   0 winners  entry c = cell c of the winners table, kept when occupied; the value is the winning point
//   1 n_keep   entry j = compacted point j, counted when its float64 norm is non-zero (count only)
//   2 sample   entry j kept when counted by 1 and u(j) < N * 1.8 / n_keep
struct CompArgs {
    const float4* pts; const int* off; long total;       // stage 0 source
    const unsigned* win;                                 // [S][cap]
    const float4* list; const int* list_n;               // stages 1, 2 source: [S][cap] and its lengths [S]
    const int* nk_part;                                  // stage 2: the chunk counts of stage 1
    const double* uniforms; const u64* keys; u64 seed; double num;
    int cap, nchunk;
};

__device__ __forceinline__ u64 mix64(u64 z) {            // splitmix64's finaliser (Steele, Lea, Flood 2014)
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// counter-based: a function of (seed, scan key, output slot) alone -> [0, 1) on the 2^-53 grid
__device__ __forceinline__ double own_uniform(u64 seed, u64 key, u64 slot) {
    u64 h = mix64(seed + 0x9E3779B97F4A7C15ull);
    h = mix64(h ^ mix64(key + 0xD1B54A32D192ED03ull));
    h = mix64(h + (slot + 1) * 0x9E3779B97F4A7C15ull);
    return (double)(h >> 11) * 0x1.0p-53;
}

__device__ __forceinline__ bool nonzero_norm(float4 p) {
    const double x = p.x, y = p.y, z = p.z, w = p.w;
    return ((x * x + y * y) + z * z) + w * w > 0.0;      // sign only: squares of float32 values neither underflow nor cancel
}

template <int STAGE>
__device__ __forceinline__ bool keep_entry(const CompArgs& a, int s, int c, double prob, float4& v) {
    if (c >= a.cap) return false;
    if (STAGE == 0) {
        const unsigned w = a.win[(long)s * a.cap + c];
        if (w == 0u) return false;
        const long i = (long)a.off[s] + (long)(w - 1u);
        if (i >= a.total) return false;
        v = a.pts[i];
        return true;
    }
    if (c >= a.list_n[s]) return false;
    v = a.list[(long)s * a.cap + c];
    if (!nonzero_norm(v)) return false;
    if (STAGE == 1) return true;
    const double u = a.uniforms ? a.uniforms[(long)s * a.cap + c] : own_uniform(a.seed, a.keys[s], (u64)c);
    return u < prob;
}

// stage 2's probability, the same value in every block of a scan: the chunk counts summed in chunk order
__device__ __forceinline__ double sample_prob(const CompArgs& a, int s) {
    long n_keep = 0;
    for (int k = 0; k < a.nchunk; ++k) n_keep += a.nk_part[s * a.nchunk + k];
    return n_keep > 0 ? a.num / (double)n_keep : 0.0;
}

template <int STAGE>
__global__ void __launch_bounds__(256) k_sp_count(CompArgs a, int* __restrict__ part) {
    __shared__ int wsum[4];
    __shared__ double prob_s;
    const int s = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    if (STAGE == 2) {
        if (tid == 0) prob_s = sample_prob(a, s);
        __syncthreads();
    }
    const double prob = STAGE == 2 ? prob_s : 0.0;
    int n = 0;
    for (int k = 0; k < CHUNK / 256; ++k) {
        float4 v;
        n += keep_entry<STAGE>(a, s, chunk * CHUNK + k * 256 + tid, prob, v) ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, FD_WAVE);
    if ((tid & 63) == 0) wsum[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) part[s * a.nchunk + chunk] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

template <int STAGE>
__global__ void __launch_bounds__(256) k_sp_gather(CompArgs a, const int* __restrict__ part, float4* __restrict__ out,
                                                   int* __restrict__ out_n, int fill) {
    __shared__ int wsum[4];
    __shared__ int base_s, total_s;
    __shared__ double prob_s;
    const int s = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) {
        int b = 0, t = 0;
        for (int k = 0; k < a.nchunk; ++k) {
            const int n = part[s * a.nchunk + k];
            if (k < chunk) b += n;
            t += n;
        }
        base_s = b; total_s = t;
        if (STAGE == 2) prob_s = sample_prob(a, s);
        if (chunk == 0) out_n[s] = t;
    }
    __syncthreads();
    const double prob = STAGE == 2 ? prob_s : 0.0;
    const int total = total_s;
    int base = base_s;
    float4* dst = out + (long)s * a.cap;
    for (int k = 0; k < CHUNK / 256; ++k) {
        float4 v;
        const bool keep = keep_entry<STAGE>(a, s, chunk * CHUNK + k * 256 + tid, prob, v);
        const u64 m = __ballot(keep);
        if (lane == 0) wsum[wv] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wv) before += wsum[w];
            all += wsum[w];
        }
        const int slot = base + before + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && slot < a.cap) dst[slot] = v;                          // slot < total <= cap by construction
        base += all;
        __syncthreads();
    }
    if (fill) {
        for (int k = 0; k < CHUNK / 256; ++k) {
            const int c = chunk * CHUNK + k * 256 + tid;
            if (c >= total && c < a.cap) dst[c] = make_float4(-1.f, 0.f, 0.f, 0.f);
        }
    }
}

inline size_t align256(size_t n) { return (n + 255) / 256 * 256; }

struct SpLayout {
    size_t win, part0, list, list_n, part1, part2, bytes;
    int cap, nchunk;
};

// validates the configuration; false (with the error set) when it cannot be run
bool sp_layout(const fd_sparsify_cfg* c, SpLayout& L) {
    if (!c) { fd_set_error("fd_sparsify: cfg is NULL"); return false; }
    if (c->S < 1 || c->H < 1 || c->H > MAX_H || c->W < 1 || c->n_rows < 1 || c->n_rows > FD_SPARSIFY_MAX_ROWS || c->random_sample < 0) {
        fd_set_error("fd_sparsify: bad cfg (S %d, H %d (1..%d), W %d, n_rows %d (1..%d), random_sample %d)", c->S, c->H, MAX_H, c->W,
                     c->n_rows, FD_SPARSIFY_MAX_ROWS, c->random_sample);
        return false;
    }
    for (int k = 0; k < c->n_rows; ++k) {
        if (c->rows[k] < 0 || c->rows[k] >= c->H) { fd_set_error("fd_sparsify: row %d is outside [0, %d)", c->rows[k], c->H); return false; }
        for (int j = 0; j < k; ++j)
            if (c->rows[j] == c->rows[k]) { fd_set_error("fd_sparsify: row %d is listed twice", c->rows[k]); return false; }
    }
    const long cap = (long)c->n_rows * c->W;
    if (cap * c->S >= (1L << 31) / 4) { fd_set_error("fd_sparsify: S * n_rows * W = %ld is too large", cap * c->S); return false; }
    L.cap = (int)cap;
    L.nchunk = fd_cdiv(cap, CHUNK);
    const size_t parts = align256((size_t)c->S * L.nchunk * 4);
    size_t o = 0;
    L.win = o; o += align256((size_t)c->S * cap * 4);
    L.part0 = o; o += parts;
    L.list = L.list_n = L.part1 = L.part2 = 0;
    if (c->random_sample > 0) {
        L.list = o; o += align256((size_t)c->S * cap * 16);
        L.list_n = o; o += align256((size_t)c->S * 4);
        L.part1 = o; o += parts;
        L.part2 = o; o += parts;
    }
    L.bytes = o;
    return true;
}

}  // namespace

extern "C" long fd_sparsify_ws_bytes(const fd_sparsify_cfg* cfg) {
    SpLayout L;
    return sp_layout(cfg, L) ? (long)L.bytes : 0;
}

extern "C" int fd_sparsify_scans(const float* points, const int* offsets, long total_points, const fd_sparsify_cfg* cfg,
                                 const double* uniforms, const unsigned long long* keys, float* slab, int* counts, int* cells,
                                 void* ws, void* stream) {
    SpLayout L;
    if (!sp_layout(cfg, L)) return -1;
    FD_REQUIRE(offsets && slab && counts && ws && total_points >= 0 && total_points < (1L << 31) && (points || total_points == 0),
               "fd_sparsify_scans: bad args");
    FD_REQUIRE(((uintptr_t)points & 15) == 0 && ((uintptr_t)slab & 15) == 0 && ((uintptr_t)ws & 15) == 0,
               "fd_sparsify_scans: points, slab and ws must be 16-byte aligned");
    FD_REQUIRE(cfg->random_sample == 0 || uniforms || keys, "fd_sparsify_scans: random_sample needs uniforms or keys");
    hipStream_t st = (hipStream_t)stream;
    char* b = (char*)ws;
    unsigned* win = (unsigned*)(b + L.win);
    const int S = cfg->S;
    hipError_t e = hipMemsetAsync(win, 0, (size_t)S * L.cap * 4, st);
    FD_REQUIRE(e == hipSuccess, "fd_sparsify_scans: memset failed: %s", hipGetErrorString(e));
    if (total_points > 0) {
        const double D2R = 3.141592653589793238462643383279502884 / 180.0;       // numpy's radians(): x * (pi / 180)
        CellArgs a;
        a.pts = (const float4*)points; a.off = offsets; a.total = total_points; a.S = S; a.H = cfg->H; a.W = cfg->W; a.cap = L.cap;
        a.x_lo = cfg->x_lo; a.x_hi = cfg->x_hi; a.y_lo = cfg->y_lo; a.y_hi = cfg->y_hi; a.z_lo = cfg->z_lo; a.z_hi = cfg->z_hi;
        a.rad45 = 45.0 * D2R; a.rad2 = 2.0 * D2R;
        a.dphi = (90.0 / (double)cfg->W) * D2R;
        a.dtheta = (0.4 * 64.0 / (double)cfg->H) * D2R;
        RowList rl;
        rl.n = cfg->n_rows;
        for (int k = 0; k < FD_SPARSIFY_MAX_ROWS; ++k) rl.rows[k] = k < cfg->n_rows ? cfg->rows[k] : 0;
        hipLaunchKernelGGL(k_sp_cells, dim3(fd_cdiv(total_points, 256)), dim3(256), 0, st, a, rl, win, cells);
        FD_LAUNCH_CHECK("fd_sparsify_scans(cells)");
    }
    CompArgs c;
    c.pts = (const float4*)points; c.off = offsets; c.total = total_points; c.win = win;
    c.list = nullptr; c.list_n = nullptr; c.nk_part = nullptr;
    c.uniforms = uniforms; c.keys = keys; c.seed = cfg->seed; c.num = (double)cfg->random_sample * 1.8;
    c.cap = L.cap; c.nchunk = L.nchunk;
    const dim3 grid(L.nchunk, S), block(256);
    int* part0 = (int*)(b + L.part0);
    hipLaunchKernelGGL(k_sp_count<0>, grid, block, 0, st, c, part0);
    FD_LAUNCH_CHECK("fd_sparsify_scans(count)");
    if (cfg->random_sample == 0) {
        hipLaunchKernelGGL(k_sp_gather<0>, grid, block, 0, st, c, (const int*)part0, (float4*)slab, counts, 1);
        FD_LAUNCH_CHECK("fd_sparsify_scans(gather)");
        return 0;
    }
    float4* list = (float4*)(b + L.list);
    int* list_n = (int*)(b + L.list_n);
    int* part1 = (int*)(b + L.part1);
    int* part2 = (int*)(b + L.part2);
    hipLaunchKernelGGL(k_sp_gather<0>, grid, block, 0, st, c, (const int*)part0, list, list_n, 0);
    FD_LAUNCH_CHECK("fd_sparsify_scans(gather)");
    c.list = list; c.list_n = list_n; c.nk_part = part1;
    hipLaunchKernelGGL(k_sp_count<1>, grid, block, 0, st, c, part1);
    FD_LAUNCH_CHECK("fd_sparsify_scans(n_keep)");
    hipLaunchKernelGGL(k_sp_count<2>, grid, block, 0, st, c, part2);
    FD_LAUNCH_CHECK("fd_sparsify_scans(sample count)");
    hipLaunchKernelGGL(k_sp_gather<2>, grid, block, 0, st, c, (const int*)part2, (float4*)slab, counts, 1);
    FD_LAUNCH_CHECK("fd_sparsify_scans(sample gather)");
    return 0;
}
