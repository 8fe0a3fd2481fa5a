// The cell bins: the binning kernels that write the workspace (its layout:
// knn_common.hpp; the binned kNN that reads it: knn.hip), and the radius graph
// as an index-order scan and as a binned search (which falls back to the
// scan).  The file map: knn_common.hpp.
#include "knn_common.hpp"

namespace {

constexpr int kBinThreads = 1024;

// The cell of point c in the grid of the header at W.
__device__ __forceinline__ int bin_cell(const uint32_t *__restrict__ W, float2 c) {
    const float *H = (const float *)W;
    return bin_axis(c.y, H[1], H[5], (int)W[8]) * (int)W[7] + bin_axis(c.x, H[0], H[4], (int)W[7]);
}

// Binning is four launches: (1) one workgroup per trajectory reduces the box,
// writes the header and zeroes the cell counts; (2) a thread per point counts
// its cell (atomics on the workspace); (3) one workgroup per trajectory scans
// the counts into the cell starts and the scatter cursors; (4) a thread per
// point takes a slot of its cell.  The order of the points inside a cell
// depends on the schedule; the search's answer does not ((key, index) is a
// total order).
__global__ __launch_bounds__(kBinThreads) void knn_bin_box_kernel(const float2 *__restrict__ src, int n_per,
                                                                  uint32_t *__restrict__ ws) {
    constexpr int NW = kBinThreads / 64;
    __shared__ float red[NW][5];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BinLayout lay = bins_layout(n_per);
    const float2 *P = src + (int64_t)b * n_per;
    uint32_t *W = ws + (int64_t)b * lay.stride;
    int *cur = (int *)(W + lay.cur);

    float mnx = 3.0e38f, mny = 3.0e38f, mxx = -3.0e38f, mxy = -3.0e38f, mabs = 0.0f;
    for (int i = tid; i < n_per; i += kBinThreads) {
        const float2 c = P[i];
        mnx = fminf(mnx, c.x);
        mny = fminf(mny, c.y);
        mxx = fmaxf(mxx, c.x);
        mxy = fmaxf(mxy, c.y);
        mabs = fmaxf(mabs, fmaxf(fabsf(c.x), fabsf(c.y)));
    }
    mnx = -wave_max_full(-mnx);
    mny = -wave_max_full(-mny);
    mxx = wave_max_full(mxx);
    mxy = wave_max_full(mxy);
    mabs = wave_max_full(mabs);
    if (lane == 0) {
        red[wave][0] = mnx;
        red[wave][1] = mny;
        red[wave][2] = mxx;
        red[wave][3] = mxy;
        red[wave][4] = mabs;
    }
    __syncthreads();
    float x0 = red[0][0], y0 = red[0][1], x1 = red[0][2], y1 = red[0][3], ma = red[0][4];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        x0 = fminf(x0, red[w][0]);
        y0 = fminf(y0, red[w][1]);
        x1 = fmaxf(x1, red[w][2]);
        y1 = fmaxf(y1, red[w][3]);
        ma = fmaxf(ma, red[w][4]);
    }
    // eps bounds, on either axis, how far outside its cell's nominal box
    // [o + c h, o + (c + 1) h] a point can lie plus the rounding of that box's
    // sides as the search forms them: the cell index carries a relative error
    // <= 3 2^-24 and h one of 2^-23 (together < 3e-7 of the extent), a side
    // o + c h an absolute one <= 2^-22 of the largest coordinate.
    const float ex = x1 - x0, ey = y1 - y0;
    const float eps = (1.0e-5f * fmaxf(ex, ey) + 2.0e-6f * ma) * kUp;
    const bool ok = isfinite(ex) && isfinite(ey) && isfinite(eps);
    int gx = lay.G, gy = lay.G;
    float hx = ex / gx, hy = ey / gy;
    float ihx = 1.0f / hx, ihy = 1.0f / hy;
    if (!ok || !(ex > 0.0f) || !isfinite(ihx)) {
        gx = 1;
        hx = ihx = 0.0f;
    }
    if (!ok || !(ey > 0.0f) || !isfinite(ihy)) {
        gy = 1;
        hy = ihy = 0.0f;
    }
    const int nc = gx * gy;
    if (tid == 0) {
        float *H = (float *)W;
        H[0] = x0;
        H[1] = y0;
        H[2] = hx;
        H[3] = hy;
        H[4] = ihx;
        H[5] = ihy;
        H[6] = ok ? eps : 0.0f;
        W[7] = (uint32_t)gx;
        W[8] = (uint32_t)gy;
        W[9] = (uint32_t)n_per;
    }
    for (int c = tid; c < nc; c += kBinThreads) cur[c] = 0;
}

__global__ __launch_bounds__(256) void knn_bin_count_kernel(const float2 *__restrict__ src, int n_per,
                                                            uint32_t *__restrict__ ws) {
    const BinLayout lay = bins_layout(n_per);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_per) return;
    uint32_t *W = ws + (int64_t)blockIdx.y * lay.stride;
    atomicAdd((int *)(W + lay.cur) + bin_cell(W, src[(int64_t)blockIdx.y * n_per + i]), 1);
}

// exclusive scan of the counts: a contiguous chunk of cells per thread
__global__ __launch_bounds__(kBinThreads) void knn_bin_scan_kernel(int n_per, uint32_t *__restrict__ ws) {
    constexpr int NW = kBinThreads / 64;
    __shared__ int wsum[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BinLayout lay = bins_layout(n_per);
    uint32_t *W = ws + (int64_t)blockIdx.x * lay.stride;
    int *start = (int *)(W + lay.start);
    int *cur = (int *)(W + lay.cur);
    const int nc = (int)W[7] * (int)W[8];
    const int chunk = (nc + kBinThreads - 1) / kBinThreads;
    const int c0 = min(tid * chunk, nc), c1 = min(c0 + chunk, nc);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += cur[c];
    int inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int run = inc - sum;
    for (int w = 0; w < wave; ++w) run += wsum[w];
    for (int c = c0; c < c1; ++c) {  // this thread's own cells: the count becomes the cursor
        const int v = cur[c];
        start[c] = run;
        cur[c] = run;
        run += v;
    }
    if (tid == 0) start[nc] = n_per;
}

__global__ __launch_bounds__(256) void knn_bin_scatter_kernel(const float2 *__restrict__ src, int n_per,
                                                              uint32_t *__restrict__ ws) {
    const BinLayout lay = bins_layout(n_per);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_per) return;
    uint32_t *W = ws + (int64_t)blockIdx.y * lay.stride;
    const float2 c = src[(int64_t)blockIdx.y * n_per + i];
    const int pos = atomicAdd((int *)(W + lay.cur) + bin_cell(W, c), 1);
    if ((unsigned)pos < (unsigned)n_per) {  // always: the counts are these same cells'
        ((float2 *)(W + lay.sp))[pos] = c;
        ((int32_t *)(W + lay.si))[pos] = i;
    }
}

// torch_cluster radius_graph(x, r, batch, loop=False, max_num_neighbors)
// (reference data_creator_2d.py:257-258): radius(x, x, ..., max_num_neighbors
// + 1) scans the query's segment in index order and keeps the first w = max_nn
// + 1 points with d2 < r2 (the query itself included), then the self loop is
// dropped.  One wave per query, 64 candidates per step, ballot order = index
// order; stops once w points were taken.  nbr [n, w] global sources ascending,
// padded with -1; deg [n] = entries kept (w - 1 or w).
// The hit predicate of both radius kernels, on the same floats: fp32 squared
// distance (the graph key) strictly below r2, compared as raw bits (NaN and
// infinite keys order above every finite r2: no hit).
__device__ __forceinline__ bool radius_hit(float2 p, float2 q, float r2) {
    return key_f32(p, q) < __float_as_uint(r2);
}

// torch_cluster squares r on the host in double and hands the kernel a float
inline float radius_r2(float r) { return (float)((double)r * (double)r); }

// The index-order scan of one query (local index q, point qp) over its
// trajectory's points P, by one wave: the row and its degree as described
// above.  Returns the number of points examined (whole steps of 64, clipped to
// n_per).
__device__ __forceinline__ int radius_scan(const float2 *__restrict__ P, int n_per, float2 qp, int q, int b,
                                           float r2, int w, int32_t *__restrict__ row,
                                           int32_t *__restrict__ deg_out, int lane, uint64_t below) {
    int taken = 0, kept = 0, j0 = 0;
    for (; j0 < n_per && taken < w; j0 += 64) {
        const int j = j0 + lane;
        const bool hit = j < n_per && radius_hit(P[j], qp, r2);
        const uint64_t hm = __ballot(hit);
        const bool take = hit && taken + __popcll(hm & below) < w;
        const uint64_t tm = __ballot(take);
        const uint64_t km = __ballot(take && j != q);  // self loop dropped
        if (take && j != q) row[kept + __popcll(km & below)] = b * n_per + j;
        taken += __popcll(tm);
        kept += __popcll(km);
    }
    for (int e = kept + lane; e < w; e += 64) row[e] = -1;
    if (lane == 0) *deg_out = kept;
    return min(j0, n_per);
}

__global__ __launch_bounds__(256) void radius_kernel(const float2 *__restrict__ pts, int n_per,
                                                     float r2, int w, int32_t *__restrict__ nbr,
                                                     int32_t *__restrict__ deg) {
    const int b = blockIdx.y;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (q >= n_per) return;  // wave-uniform: no barrier below
    const float2 *P = pts + (int64_t)b * n_per;
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const int64_t g = (int64_t)b * n_per + q;
    radius_scan(P, n_per, P[q], q, b, r2, w, nbr + g * w, deg + g, lane, below);
}

// radius_kernel's table from the cell bins of pos (mmpde_knn_bin): the cost of
// a query follows the number of points near it, not the trajectory's size.
// One wave per query, four per workgroup.
//  1. Reach.  A hit has fp32 key f < r2, and f >= d^2 (1 - 2^-22) - 2^-126 for
//     the exact distance d of the two fp32 points (KeyTraits<true>), so
//     d < R0 = sqrtf(r2) kUp^2 + 1e-18 (sqrtf's 2^-24 and the 2^-63 of the
//     absolute term are inside the kUp = 1 + 2^-20 factors and the 1e-18).
//     R = (R0 + eps) kUp with the header's eps: eps >= 2^-19 of the largest
//     coordinate and R 2^-20 cover the rounding of q -+ R (<= 2^-24 (|q| + R)),
//     so fl(q.x - R) <= p.x <= fl(q.x + R) for every hit p, and likewise in y;
//     eps also is how far outside its cell's nominal box a point can lie.
//  2. Block.  bin_axis is monotone in the coordinate (a rounded difference, a
//     product with ih >= 0, a clamp, a truncation) and is the function that
//     binned p, so p's cell lies in [bin_axis(q.x - R), bin_axis(q.x + R)] x
//     [bin_axis(q.y - R), bin_axis(q.y + R)]: every hit is in the block.  Each
//     block row is one contiguous range of the sorted copy.
//  3. Fallback.  A block of more than kRadiusScanNum / kRadiusScanDen of the
//     grid's cells (known without a load: a radius that covers much of the
//     domain), or whose point count, summed from the cell starts before any
//     point is read, exceeds that share of n_per (a heavy cell), runs
//     radius_scan on the original points: its early exit at w hits makes it
//     the cheaper path there.  The share is the measured break-even
//     (profiles/radius_times.txt: the scan and the binned path cost the same
//     at blocks of about 14 % of the trajectory, from 9216 to 65536 points).
//  4. Otherwise the block's hits arrive in bin order.  `best` holds the 64
//     smallest original indices seen so far, ascending in lane order (~0u:
//     none).  Hits below the current w-th smallest are compacted into a
//     128-entry LDS list; each full batch of 64 is sorted descending and
//     merged: min(best, batch) per lane is bitonic and holds the 64 smallest
//     of the 128, one bitonic merge sorts it.  Any number of hits gives the w
//     smallest indices exactly; nothing is truncated.
//  5. Lanes < w of best are the first w hits in index order; the self loop is
//     dropped and the row padded as radius_scan does.
// A header that was not written for this n_per ends the wave before any
// indexed read; starts and indices are clamped into range.
constexpr int kRadiusScanNum = 1, kRadiusScanDen = 8;

__device__ __forceinline__ uint32_t radius_merge64(uint32_t best, uint32_t v, int lane) {
    const uint32_t desc = ~wave_sort64(~v, lane);
    uint32_t m = min(best, desc);
#pragma unroll
    for (int s = 5; s >= 0; --s) {  // (a counted loop: xor_lane needs j to fold to a constant)
        const int j = 1 << s;
        const uint32_t o = xor_lane(m, j, lane);
        m = (lane & j) == 0 ? min(m, o) : max(m, o);
    }
    return m;
}

__global__ __launch_bounds__(256) void radius_binned_kernel(const float2 *__restrict__ pts,
                                                            const uint32_t *__restrict__ bins,
                                                            const BinLayout lay, int n_per, float r2, int w,
                                                            int32_t *__restrict__ nbr,
                                                            int32_t *__restrict__ deg,
                                                            unsigned long long *__restrict__ stats) {
    __shared__ uint32_t sHit[4][128];
    const int b = blockIdx.y;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + wave;
    if (qi >= n_per) return;  // wave-uniform: no workgroup barrier below
    // lay = bins_layout(n_per) from the host: its grid-size loop would run in every wave
    const float2 *P = pts + (int64_t)b * n_per;
    const float2 q = P[qi];
    const uint32_t *W = bins + (int64_t)b * lay.stride;
    const float2 *SP = (const float2 *)(W + lay.sp);
    const int32_t *SI = (const int32_t *)(W + lay.si);
    const int *start = (const int *)(W + lay.start);
    // The header's words in four independent 8-byte loads beside the query's
    // point, and the block (arithmetic only, harmless on a foreign header)
    // before the branch on the header: one memory round trip ahead of the
    // fallback's scan, not three.
    const uint2 *H2 = (const uint2 *)W;
    const uint2 h0 = H2[0], h2 = H2[2], h3 = H2[3], h4 = H2[4];
    const float x0 = __uint_as_float(h0.x), y0 = __uint_as_float(h0.y);
    const float ihx = __uint_as_float(h2.x), ihy = __uint_as_float(h2.y), eps = __uint_as_float(h3.x);
    const int gx = (int)h3.y, gy = (int)h4.x;
    const float R = (sqrtf(r2) * kUp * kUp + 1.0e-18f + eps) * kUp;
    const int cxlo = bin_axis(q.x - R, x0, ihx, gx), cxhi = bin_axis(q.x + R, x0, ihx, gx);
    const int cylo = bin_axis(q.y - R, y0, ihy, gy), cyhi = bin_axis(q.y + R, y0, ihy, gy);
    // (bin_axis is monotone, so cxlo <= cxhi and cylo <= cyhi; a non-finite query hits nothing either way)
    const int ncell = (cxhi - cxlo + 1) * (cyhi - cylo + 1);
    // ncell < 1 never holds for a grid this n_per's binning wrote
    if ((gx < 1) | (gx > lay.G) | (gy < 1) | (gy > lay.G) | ((int)h4.y != n_per) | (ncell < 1)) return;
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    auto range_lo = [&](int c) { return min(max(start[c], 0), n_per); };
    const int64_t g = (int64_t)b * n_per + qi;
    int32_t *row = nbr + g * w;

    bool scan = ncell * kRadiusScanDen > gx * gy * kRadiusScanNum;
    int total = 0;
    if (!scan) {
        for (int y = cylo + lane; y <= cyhi; y += 64)
            total += max(range_lo(y * gx + cxhi + 1) - range_lo(y * gx + cxlo), 0);
#pragma unroll
        for (int j = 1; j <= 32; j <<= 1) total += (int)xor_lane((uint32_t)total, j, lane);
        scan = (int64_t)total * kRadiusScanDen > (int64_t)n_per * kRadiusScanNum;
    }
    if (scan) {
        const int seen = radius_scan(P, n_per, q, qi, b, r2, w, row, deg + g, lane, below);
        if (stats && lane == 0) {
            atomicAdd(&stats[0], (unsigned long long)seen);
            atomicAdd(&stats[1], 1ull);
        }
        return;
    }

    uint32_t best = ~0u;
    uint32_t *list = sHit[wave];
    int m = 0;
    for (int y = cylo; y <= cyhi; ++y) {
        const int lo = range_lo(y * gx + cxlo), len = range_lo(y * gx + cxhi + 1) - lo;
        for (int o0 = 0; o0 < len; o0 += 64) {
            const int o = o0 + lane;
            uint32_t idx = ~0u;
            bool hit = false;
            if (o < len) {
                idx = (uint32_t)min(max(SI[lo + o], 0), n_per - 1);
                hit = radius_hit(SP[lo + o], q, r2);
            }
            // lane w - 1 of best: the w-th smallest so far (~0u: fewer than w)
            hit = hit && idx < lane_value(best, w - 1);
            const uint64_t hm = __ballot(hit);
            if (hit) list[m + __popcll(hm & below)] = idx;  // m < 64: at most 127
            m += __popcll(hm);
            if (m >= 64) {
                wave_lds_sync();
                const uint32_t v = list[lane];
                const uint32_t rest = lane + 64 < m ? list[lane + 64] : ~0u;
                best = radius_merge64(best, v, lane);
                wave_lds_sync();
                list[lane] = rest;
                m -= 64;
            }
        }
    }
    if (m > 0) {
        wave_lds_sync();
        best = radius_merge64(best, lane < m ? list[lane] : ~0u, lane);
    }
    const bool take = lane < w && best != ~0u;
    const bool keep = take && (int)best != qi;  // self loop dropped
    const uint64_t km = __ballot(keep);
    const int kept = __popcll(km);
    if (keep) row[__popcll(km & below)] = b * n_per + (int)best;
    for (int e = kept + lane; e < w; e += 64) row[e] = -1;
    if (lane == 0) {
        deg[g] = kept;
        if (stats) atomicAdd(&stats[0], (unsigned long long)total);
    }
}

}  // namespace

extern "C" int mmpde_knn_bins_grid(int64_t n_per) {
    return n_per < 1 || n_per > kTiledMax ? 0 : bins_grid(n_per);
}

extern "C" int64_t mmpde_knn_bins_bytes(int64_t batches, int64_t n_per) {
    if (batches < 1 || batches > 65535 || n_per < 1 || n_per > kTiledMax) return 0;
    return batches * bins_layout(n_per).stride * (int64_t)sizeof(uint32_t);
}

extern "C" int mmpde_knn_bin(const float *src, int64_t batches, int64_t n_per, void *bins, int64_t bins_bytes,
                             mmpde_stream_t stream) {
    MMPDE_REQUIRE(src && bins && batches >= 1 && batches <= 65535 && n_per >= 1 && n_per <= kTiledMax &&
                  batches * n_per <= INT32_MAX && ((uintptr_t)bins & 7) == 0 &&
                  bins_bytes >= mmpde_knn_bins_bytes(batches, n_per));
    hipStream_t st = as_stream(stream);
    const float2 *p = (const float2 *)src;
    uint32_t *w = (uint32_t *)bins;
    const dim3 per_traj((unsigned)batches), per_point(ceil_div(n_per, 256), (unsigned)batches);
    hipLaunchKernelGGL(knn_bin_box_kernel, per_traj, dim3(kBinThreads), 0, st, p, (int)n_per, w);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(knn_bin_count_kernel, per_point, dim3(256), 0, st, p, (int)n_per, w);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(knn_bin_scan_kernel, per_traj, dim3(kBinThreads), 0, st, (int)n_per, w);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(knn_bin_scatter_kernel, per_point, dim3(256), 0, st, p, (int)n_per, w);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

extern "C" int mmpde_radius_graph(const float *pos, int64_t batches, int64_t n_per, float r,
                                  int max_num_neighbors, int32_t *nbr_out, int32_t *degree_out,
                                  mmpde_stream_t stream) {
    MMPDE_REQUIRE(pos && nbr_out && degree_out);
    MMPDE_REQUIRE(batches > 0 && batches <= 65535 && n_per > 0 && n_per <= INT32_MAX &&
                  batches * n_per <= INT32_MAX && max_num_neighbors > 0 && r > 0.0f);
    hipLaunchKernelGGL(radius_kernel, dim3((unsigned)ceil_div(n_per, 4), (unsigned)batches),
                       dim3(256), 0, as_stream(stream), (const float2 *)pos, (int)n_per, radius_r2(r),
                       max_num_neighbors + 1, nbr_out, degree_out);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

extern "C" int mmpde_radius_graph_binned(const float *pos, const void *bins, int64_t batches, int64_t n_per,
                                         float r, int max_num_neighbors, int32_t *nbr_out,
                                         int32_t *degree_out, int64_t *stats, mmpde_stream_t stream) {
    MMPDE_REQUIRE(pos && bins && nbr_out && degree_out && ((uintptr_t)bins & 7) == 0);
    // the selection is one value per lane: w = max_num_neighbors + 1 <= 64
    MMPDE_REQUIRE(batches > 0 && batches <= 65535 && n_per > 0 && n_per <= kTiledMax &&
                  max_num_neighbors > 0 && max_num_neighbors + 1 <= 64 && r > 0.0f);
    hipLaunchKernelGGL(radius_binned_kernel, dim3((unsigned)ceil_div(n_per, 4), (unsigned)batches),
                       dim3(256), 0, as_stream(stream), (const float2 *)pos, (const uint32_t *)bins,
                       bins_layout(n_per), (int)n_per, radius_r2(r), max_num_neighbors + 1, nbr_out, degree_out,
                       (unsigned long long *)stats);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}
