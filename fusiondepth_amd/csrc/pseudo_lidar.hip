// Pseudo-LiDAR point clouds from dense depth maps ("fd_points_export"; include/fdhip.h): Pseudo-LiDAR's project_depth_to_points for N maps
// of different sizes packed back to back - every pixel back-projected into the Velodyne frame in float64, filtered (X >= 0, Z < max_high)
// and the kept points written as float32 (X, Y, Z, 1) in row-major pixel order, the images back to back - in THREE launches whatever N
// is, without atomics of any kind:
//   1 k_points_rows<false>  one workgroup per row of every map, its four waves take the row's 64-pixel segments in turn (wave w: segments
//                           w, w + 4, ...).  Each evaluates the predicate; the ballot population counts are added over the wave's segments
//                           and over the four waves (LDS) -> ONE int per row.
//   2 k_points_scan         one workgroup per map (and one more for the total): the kept points of the maps before it (long), then the
//                           exclusive scan of its row counts - the pattern of k_score_scan (score_lists.h).  starts[n], starts[N].
//                           Unlike there, a workgroup reads the counts of OTHER maps, so the counts are read-only in this launch and
//                           the row starts go to a second array: the result cannot depend on the order the workgroups run in.
//   3 k_points_rows<true>   the same walk, predicate and coordinates recomputed.  A point goes to starts[n] + row start + base + rank:
//                           `base` is carried along the row (the four waves exchange the counts of their segments through LDS, one
//                           barrier per round), rank = the kept lanes below this one (mbcnt of the ballot).  One float4 store per point.
// Store-bound: two reads of 4 B per pixel, 16 B written per kept point.  The stores are the widest there are (16 B per lane), and the
// kept lanes of a segment write one contiguous run, so a wave's store instruction covers up to 1 KiB without holes; `points` is 16-byte
// aligned and every slot is a multiple of 16 bytes from it.  A row per workgroup (not per wave) keeps a single 375 x 1242 map at 1500
// waves instead of 375, and the serial walk along a row at 5 rounds instead of 20; the next round's depth is loaded before the barrier.
// The grid is sized by the chunk's largest map; a workgroup whose row lies outside its own map exits at once, as k_depth_export does.
// Every float64 step is one rounding, in the order fdhip.h states: contraction is off for the whole file, the divisions are IEEE.
#include "../../include/fdhip.h"
#include "fd_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int PL_WAVES = 4;                                       // waves per workgroup: the segments of one row in turn
constexpr int PL_ROUND = PL_WAVES * 64;                           // pixels of a row per round

struct PointsArgs {
    const float* depth; const fd_export_desc* desc; const fd_points_calib* calib;
    int N; long packed_elems; int max_H, max_W; double max_high;
    int* counts;                                                  // [N][max_H]: kept pixels per row; the scan only READS it
    int* row_start;                                               // [N][max_H]: first slot of a row inside its map - a second array,
                                                                  // because the scan's workgroups read the counts of each other's maps
    float* points; long* starts;
};

__device__ __forceinline__ bool points_desc_ok(const fd_export_desc& d, const PointsArgs& a) {
    return d.H > 0 && d.W > 0 && d.H <= a.max_H && d.W <= a.max_W && d.offset >= 0 && d.offset <= a.packed_elems &&
           (long)d.H * d.W <= a.packed_elems - d.offset;
}

// ---------------------------------------------------------------------------------------------- 1, 3: count and write
template <bool WRITE>
__global__ void __launch_bounds__(PL_WAVES * 64) k_points_rows(PointsArgs a) {
    __shared__ int kept[2][PL_WAVES];
    const int n = blockIdx.y, v = blockIdx.x;                     // map, row: uniform over the workgroup, and so is every exit
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const fd_export_desc d = a.desc[n];
    if (!points_desc_ok(d, a) || v >= d.H) return;
    const fd_points_calib c = a.calib[n];
    const int W = d.W;
    const float* row = a.depth + d.offset + (long)v * W;
    const double yv = (double)v - c.c_v;
    const unsigned long long below = (1ull << lane) - 1ull;
    long at = 0;                                                  // first slot of the row
    if (WRITE) at = a.starts[n] + a.row_start[(long)n * a.max_H + v];
    const int rounds = (W + PL_ROUND - 1) / PL_ROUND;             // uniform: every wave meets every barrier
    int count = 0;                                                // !WRITE: this wave's kept pixels; WRITE: the row's so far
    int u = wv * 64 + lane;
    float zf = u < W ? row[u] : 0.f;
    for (int it = 0; it < rounds; ++it, u += PL_ROUND) {
        const bool in = u < W;
        const double z = (double)zf;
        if (it + 1 < rounds) zf = u + PL_ROUND < W ? row[u + PL_ROUND] : 0.f;          // the next round's load, ahead of the barrier
        const double x = (((double)u - c.c_u) * z) / c.f_u + c.b_x;
        const double y = (yv * z) / c.f_v + c.b_y;
        const double X = ((c.A[0] * x + c.A[1] * y) + c.A[2] * z) + c.t[0];
        const double Z = ((c.A[6] * x + c.A[7] * y) + c.A[8] * z) + c.t[2];
        const bool keep = in && X >= 0.0 && Z < a.max_high;       // a NaN falls out through the comparisons
        const unsigned long long m = __ballot(keep);
        const int mine = __popcll(m);
        if (!WRITE) {
            count += mine;
        } else {
            int* k = kept[it & 1];                                // two buffers: the round after next writes this one again, past a barrier
            if (lane == 0) k[wv] = mine;
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < PL_WAVES; ++w) {
                const int kw = k[w];
                before += w < wv ? kw : 0;
                all += kw;
            }
            if (keep) {
                const double Y = ((c.A[3] * x + c.A[4] * y) + c.A[5] * z) + c.t[1];
                const long slot = at + count + before + __popcll(m & below);
                // slot < packed_elems unless descriptors overlap (then their pixels outnumber the buffer): never past the end
                if (slot < a.packed_elems) *reinterpret_cast<float4*>(a.points + 4 * slot) = make_float4((float)X, (float)Y, (float)Z, 1.0f);
            }
            count += all;
        }
    }
    if (!WRITE) {
        if (lane == 0) kept[0][wv] = count;
        __syncthreads();
        if (threadIdx.x == 0) {
            int s = 0;
#pragma unroll
            for (int w = 0; w < PL_WAVES; ++w) s += kept[0][w];
            a.counts[(long)n * a.max_H + v] = s;
        }
    }
}

// ---------------------------------------------------------------------------------------------- 2: scan
// blockIdx.x = n < N: starts[n] and the row starts of map n; blockIdx.x = N: starts[N], the total.
__global__ void __launch_bounds__(1024) k_points_scan(PointsArgs a) {
    __shared__ long red[1024];
    const int n = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    long mine = 0;
    for (int i = wv; i < n; i += 16) {                            // a wave per earlier map, its lanes over the rows
        const fd_export_desc di = a.desc[i];
        if (!points_desc_ok(di, a)) continue;                     // a refused map has no points (its counts were never written)
        const int* ri = a.counts + (long)i * a.max_H;
        for (int r = lane; r < di.H; r += 64) mine += ri[r];
    }
    red[t] = mine;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {                           // integer sums: any order gives the same value
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const long base = red[0];
    __syncthreads();
    if (t == 0) a.starts[n] = base;
    if (n >= a.N) return;                                         // uniform
    const fd_export_desc d = a.desc[n];
    const int R = points_desc_ok(d, a) ? d.H : 0;
    const int* rows = a.counts + (long)n * a.max_H;              // read-only in this launch: other workgroups sum it
    int* first = a.row_start + (long)n * a.max_H;
    const int per = (R + 1023) / 1024;                            // consecutive rows per thread
    const int r0 = t * per < R ? t * per : R, r1 = r0 + per < R ? r0 + per : R;
    long sum = 0;
    for (int r = r0; r < r1; ++r) sum += rows[r];
    red[t] = sum;
    __syncthreads();
    for (int s = 1; s < 1024; s <<= 1) {                          // inclusive scan over the threads' sums
        const long vv = t >= s ? red[t - s] : 0;
        __syncthreads();
        red[t] += vv;
        __syncthreads();
    }
    long run = red[t] - sum;                                      // < 2^30: a map has fewer pixels than that
    for (int r = r0; r < r1; ++r) {
        first[r] = (int)run;
        run += rows[r];
    }
}

inline bool points_sizes_ok(int N, int max_H, int max_W) {
    return N >= 1 && N <= 65535 && max_H > 0 && max_W > 0 && (long)max_H * max_W < (1L << 30);
}

}  // namespace

extern "C" long fd_points_export_ws_bytes(int N, int max_H) {
    if (!points_sizes_ok(N, max_H, 1)) return 0;
    return (2 * (long)N * max_H * (long)sizeof(int) + 15) & ~15L;      // counts and row starts
}

extern "C" int fd_points_export(const float* depth, const fd_export_desc* desc, const fd_points_calib* calib, int N, long packed_elems,
                                int max_H, int max_W, double max_high, void* ws, float* points, long* starts, void* stream) {
    FD_REQUIRE(depth && desc && calib && ws && points && starts && packed_elems > 0, "fd_points_export: bad args");
    FD_REQUIRE(N > 0 && N <= 65535 && max_H > 0 && max_W > 0, "fd_points_export: N must be 1 .. 65535, max_H and max_W positive");
    FD_REQUIRE(points_sizes_ok(N, max_H, max_W) && packed_elems < (1L << 40), "fd_points_export: maps too large");
    FD_REQUIRE(((uintptr_t)points & 15) == 0, "fd_points_export: points must be 16-byte aligned");
    FD_REQUIRE(((uintptr_t)desc & 7) == 0 && ((uintptr_t)calib & 7) == 0 && ((uintptr_t)starts & 7) == 0 && ((uintptr_t)depth & 3) == 0 &&
               ((uintptr_t)ws & 15) == 0, "fd_points_export: desc, calib and starts must be 8-byte aligned, depth 4-byte, ws 16-byte");
    PointsArgs a;
    a.depth = depth; a.desc = desc; a.calib = calib;
    a.N = N; a.packed_elems = packed_elems; a.max_H = max_H; a.max_W = max_W; a.max_high = max_high;
    a.counts = (int*)ws; a.row_start = a.counts + (long)N * max_H;
    a.points = points; a.starts = starts;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(max_H, N);
    hipLaunchKernelGGL((k_points_rows<false>), grid, dim3(PL_WAVES * 64), 0, st, a);
    FD_LAUNCH_CHECK("fd_points_export (count)");
    hipLaunchKernelGGL(k_points_scan, dim3(N + 1), dim3(1024), 0, st, a);
    FD_LAUNCH_CHECK("fd_points_export (scan)");
    hipLaunchKernelGGL((k_points_rows<true>), grid, dim3(PL_WAVES * 64), 0, st, a);
    FD_LAUNCH_CHECK("fd_points_export (write)");
    return 0;
}
