// The kNN searches that select with knn_finish.  The full search: every query
// against its trajectory's whole point set, in registers (knn_kernel), in LDS
// (knn_large_kernel) or streamed through LDS in tiles (knn_tiled_kernel), and
// launch_knn, which picks among them.  The binned search (knn_binned_kernel):
// only the cells around the query, from the workspace knn_bins.hip writes.
// The algorithm, the file map and why these share a file: knn_common.hpp.
#include "knn_common.hpp"

namespace {

// miss != nullptr (the candidate path's fallback, grid.x = ceil(n_q / QPB)):
// miss[b n_q + i] != 0 marks the queries of trajectory b the table could not
// answer.  Every workgroup counts the trajectory's flags and ranks them in
// index order (wave ballots, no atomics).  With more than half missed it
// answers its own QPB queries as the plain search does (re-answering a few is
// harmless: same result); otherwise the missed queries of ranks x, x + grid.x,
// ... (at most QPB), so a few misses spread over many workgroups; with none it
// returns before staging the points.  Workgroup 0 records the count.
template <int CPL, bool QUERY, int QPB = kQueriesPerBlock>
__global__ __launch_bounds__(256) void knn_kernel(const float2 *__restrict__ pts,
                                                  const float2 *__restrict__ qry, int n_src,
                                                  int n_q, int k, int32_t *__restrict__ out,
                                                  int32_t *__restrict__ degenerate,
                                                  const uint8_t *__restrict__ miss = nullptr,
                                                  float *__restrict__ cells = nullptr,
                                                  int role = 0) {
    typedef KeyTraits<QUERY> KT;
    typedef typename KT::key_t key_t;
    __shared__ float2 sP[CPL * 64];
    __shared__ key_t sKey[4][kCap];
    __shared__ int sIdx[4][kCap];
    __shared__ int sSel[4][64];

    const int b = blockIdx.y;
    int q_count = n_q;  // queries of this trajectory to answer
    __shared__ int sList[QPB];
    // QUERY ties are counted for the queries the candidate kernel did not
    // answer (its miss flags, valid unless the trajectory skipped the table)
    const uint8_t *miss_cnt = miss;
    if (miss && cell_skipped(cells, b)[role]) {  // workgroup-uniform: the plain search
        miss_cnt = nullptr;
        if (blockIdx.x == 0 && threadIdx.x == 0) cell_last_miss(cells, b)[role] = n_q;
        miss = nullptr;
    }
    if (miss) {
        if (!cell_any_miss(cells, b)[role]) {  // workgroup-uniform
            if (blockIdx.x == 0 && threadIdx.x == 0) cell_last_miss(cells, b)[role] = 0;
            return;
        }
        __shared__ int sWave[4];
        const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
        const int gx = (int)gridDim.x, x = (int)blockIdx.x;
        const uint64_t below_l = l == 0 ? 0ull : (~0ull >> (64 - l));
        int total = 0;  // misses before the current chunk
        for (int c0 = 0; c0 < n_q; c0 += 256) {
            const int i = c0 + tid;
            const bool f = i < n_q && miss[(int64_t)b * n_q + i];
            const uint64_t bal = __ballot(f);
            if (l == 0) sWave[w] = __popcll(bal);
            __syncthreads();
            int before = total;
            for (int v = 0; v < w; ++v) before += sWave[v];
            const int r = before + __popcll(bal & below_l);  // rank of this miss
            if (f && r % gx == x && r / gx < QPB) sList[r / gx] = i;
            total += sWave[0] + sWave[1] + sWave[2] + sWave[3];
            __syncthreads();  // sWave is rewritten by the next chunk
        }
        if (x == 0 && tid == 0) cell_last_miss(cells, b)[role] = total;
        if (2 * total > n_q) {
            miss = nullptr;  // most missed: the plain search's own queries
        } else {
            q_count = total > x ? min((total - x + gx - 1) / gx, QPB) : 0;  // entries of this workgroup
            if (q_count == 0) return;  // workgroup-uniform: nothing to answer
        }
    }
    const float2 *P = pts + (int64_t)b * n_src;
    for (int i = threadIdx.x; i < n_src; i += 256) sP[i] = P[i];
    __syncthreads();

    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int kk = QUERY ? k : k + 1;
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const int q_beg = miss ? 0 : (int)blockIdx.x * QPB;
    const int q_end = miss ? q_count : min((int)(blockIdx.x + 1) * QPB, n_q);

    for (int qe = q_beg + wave; qe < q_end; qe += 4) {
        const int qi = miss ? sList[qe] : qe;
        const float2 q = QUERY ? qry[(int64_t)b * n_q + qi] : sP[qi];
        uint32_t fkey[CPL];
        uint32_t lmin = ~0u;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int j = lane + 64 * c;
            fkey[c] = (j < n_src) ? key_f32(sP[j], q) : ~0u;
            lmin = fkey[c] < lmin ? fkey[c] : lmin;
        }
        // U = kk-th smallest of the 64 lane minima.  At least kk points have
        // key <= U (one per lane whose minimum is <= U), so every key of the
        // answer, ties included, is <= U: the answer is exactly the first kk
        // of C = {key <= U} in (key, index) order.  (Query: the filter is on
        // the fp32 key, with the margin of filter_threshold; exact fp64 keys
        // are formed for C only.)  C is small (~2 kk on a mesh), so it is
        // compacted into LDS and sorted.
        const uint32_t thr = KT::filter_threshold(lane_value(wave_sort64(lmin, lane), kk - 1));
        // Compaction (order is free: the list is sorted or ranked next): every
        // lane's candidates as a bit mask, the wave's exclusive prefix of their
        // counts from the counts' bit planes (ballot + mbcnt, no LDS), then each
        // lane writes its own few entries.
        uint64_t cm = 0;
#pragma unroll
        for (int c = 0; c < CPL; ++c) cm |= (uint64_t)(fkey[c] <= thr) << c;
        const int cnt = __popcll(cm);
        int m = 0, pidx = 0;
#pragma unroll
        for (int bit = 0; bit < 6; ++bit) {  // cnt <= CPL <= 64 < 2^7: bit 6 only for 64
            const uint64_t plane = __ballot((cnt >> bit) & 1);
            m += __popcll(plane) << bit;
            pidx += __popcll(plane & below) << bit;
        }
        {
            const uint64_t plane = __ballot(cnt >> 6);
            m += __popcll(plane) << 6;
            pidx += __popcll(plane & below) << 6;
        }
        while (cm) {
            const int c = __builtin_ctzll(cm);
            cm &= cm - 1;
            if (pidx < kCap) sIdx[wave][pidx] = lane + 64 * c;
            ++pidx;
        }
        knn_finish<QUERY>(sP, sKey[wave], sIdx[wave], sSel[wave], m, q, kk, k, qi, b, n_src, n_q, CPL, lane,
                          below, out, degenerate, !miss_cnt || miss_cnt[(int64_t)b * n_q + qi] != 0);
    }
}

// Trajectories of more than 4096 points (up to kLargeMax): the same search
// with the point set in dynamic LDS (one workgroup per CU) and the keys
// recomputed from LDS instead of held in registers -- pass 1 the lane minima,
// pass 2 the compaction of C in chunks of 64 columns -- so any size fits the
// register budget.  64 queries per workgroup amortise the staging.  Same
// selection (knn_finish), same results as knn_kernel.
constexpr int kLargeMax = 16384;
constexpr int kLargeQueries = 64;

template <bool QUERY>
__global__ __launch_bounds__(256) void knn_large_kernel(const float2 *__restrict__ pts,
                                                        const float2 *__restrict__ qry, int n_src,
                                                        int n_q, int k, int32_t *__restrict__ out,
                                                        int32_t *__restrict__ degenerate) {
    typedef KeyTraits<QUERY> KT;
    typedef typename KT::key_t key_t;
    extern __shared__ float2 sP[];
    __shared__ key_t sKey[4][kCap];
    __shared__ int sIdx[4][kCap];
    __shared__ int sSel[4][64];

    const int b = blockIdx.y;
    const float2 *P = pts + (int64_t)b * n_src;
    for (int i = threadIdx.x; i < n_src; i += 256) sP[i] = P[i];
    __syncthreads();

    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int kk = QUERY ? k : k + 1;
    const int cpl = (n_src + 63) / 64;
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const int q_end = min((int)(blockIdx.x + 1) * kLargeQueries, n_q);
    for (int qi = blockIdx.x * kLargeQueries + wave; qi < q_end; qi += 4) {
        const float2 q = QUERY ? qry[(int64_t)b * n_q + qi] : sP[qi];
        uint32_t lmin = ~0u;
        for (int c = 0; c < cpl; ++c) {
            const int j = lane + 64 * c;
            const uint32_t f = (j < n_src) ? key_f32(sP[j], q) : ~0u;
            lmin = f < lmin ? f : lmin;
        }
        const uint32_t thr = KT::filter_threshold(lane_value(wave_sort64(lmin, lane), kk - 1));
        int m = 0;
        for (int c0 = 0; c0 < cpl; c0 += 64) {
            const int cn = min(64, cpl - c0);
            uint64_t cm = 0;
            for (int c = 0; c < cn; ++c) {
                const int j = lane + 64 * (c0 + c);
                cm |= (uint64_t)(j < n_src && key_f32(sP[j], q) <= thr) << c;
            }
            const int cnt = __popcll(cm);
            int tot = 0, pidx = 0;
#pragma unroll
            for (int bit = 0; bit < 7; ++bit) {  // cnt <= 64 < 2^7
                const uint64_t plane = __ballot((cnt >> bit) & 1);
                tot += __popcll(plane) << bit;
                pidx += __popcll(plane & below) << bit;
            }
            pidx += m;
            while (cm) {
                const int c = __builtin_ctzll(cm);
                cm &= cm - 1;
                if (pidx < kCap) sIdx[wave][pidx] = lane + 64 * (c0 + c);
                ++pidx;
            }
            m += tot;
        }
        knn_finish<QUERY>(sP, sKey[wave], sIdx[wave], sSel[wave], m, q, kk, k, qi, b, n_src, n_q, cpl, lane,
                          below, out, degenerate);
    }
}

template <bool QUERY>
int launch_knn_large(const float2 *p, const float2 *q, int64_t batches, int ns, int nq, int k, int32_t *out,
                     int32_t *degenerate, hipStream_t st) {
    const size_t lds = (size_t)ns * sizeof(float2);
    const hipError_t e =
        hipFuncSetAttribute((const void *)knn_large_kernel<QUERY>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
    if (e != hipSuccess) return MMPDE_ERR_HIP_BASE - (int)e;
    dim3 grid(ceil_div(nq, kLargeQueries), (unsigned)batches);
    hipLaunchKernelGGL(knn_large_kernel<QUERY>, grid, dim3(256), lds, st, p, q, ns, nq, k, out, degenerate);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

// Trajectories of more than kLargeMax points (up to kTiledMax, a 256 x 256
// grid): the set no longer fits one CU's LDS, so it streams through a tile of
// kTile points, twice -- pass 1 the lane minima of the fp32 filter key over
// every tile, then thr exactly as above (the bound "at least kk points have
// key <= U" counts one point per lane, however the points were cut into
// tiles: every point is still seen by exactly one lane); pass 2 the
// compaction of C = {key <= thr} into one LDS list per query, its true size m
// counted past kCap.  Then knn_finish with the trajectory's global
// pointer in place of the LDS copy: candidate coordinates and the overflow
// path's radix select read global memory (rare, slow, exact; (key, index)
// order does not know about tiles).  Same results as knn_large_kernel.
// A wave owns kTiledQW queries for the whole kernel: their minima, thresholds
// and list sizes live in registers across the tiles (compile-time indices:
// the query loops are unrolled), and every point read from LDS is applied to
// kTiledQB of them, so the kernel is bound by the key arithmetic and not by
// one ds_read_b64 per key.  75 KB of LDS: two workgroups per CU.
// Which lane sees which point is free (the bound needs a partition, nothing
// more), and it decides how tight U is: with lane = j % 64, a row-major
// lattice whose width is a multiple of 64 (128 x 128, 192 x 192, 256 x 256)
// puts a whole grid line on one lane, the 36 nearest lanes then reach 18 cells
// out, C holds ~1000 points and EVERY query overflows into the radix select.
// So column c of a tile is rotated by c lanes (tiled_point): neighbouring grid
// lines fall on different lanes and C is ~80-110 points on those lattices.
constexpr int kTile = 4096;                    // points: 64 columns x 64 lanes, one mask bit per column
constexpr int kTiledQueries = 32;              // per workgroup
constexpr int kTiledQW = kTiledQueries / 4;    // per wave
constexpr int kTiledQB = 4;                    // queries per loaded point
static_assert(kTile == 64 * 64 && kTile <= kLargeMax && kTiledQW % kTiledQB == 0, "knn_tiled_kernel's shape");
// dynamic LDS: tile | lists [kTiledQueries][kCap] | sKey [4][kCap] (8-byte keys) | sSel [4][64] | q, m per query
constexpr int kTiledOffList = kTile * 8;
constexpr int kTiledOffKey = kTiledOffList + kTiledQueries * kCap * 4;
constexpr int kTiledOffSel = kTiledOffKey + 4 * kCap * 8;
constexpr int kTiledOffQ = kTiledOffSel + 4 * 64 * 4;
constexpr int kTiledOffM = kTiledOffQ + kTiledQueries * 8;
constexpr int kTiledLds = kTiledOffM + kTiledQueries * 4;

// Tile-local index of the point that lane `lane` reads in column c (slot
// lane + 64 c of the tile): column c rotated by c lanes.
__device__ __forceinline__ int tiled_point(int lane, int c) { return 64 * c + ((lane - c) & 63); }

// One tile's candidates of one query (bit c of cm: the point of column c on
// this lane) appended to its list at m, in any order (knn_large_kernel's
// prefix of the per-lane counts); most tiles hold none.
__device__ __forceinline__ void tiled_append(uint64_t cm, int t0, int *list, int &m, int lane, uint64_t below) {
    if (__ballot(cm != 0ull) == 0ull) return;  // wave-uniform
    const int cnt = __popcll(cm);
    int tot = 0, pidx = m;
#pragma unroll
    for (int bit = 0; bit < 7; ++bit) {  // cnt <= 64 < 2^7
        const uint64_t plane = __ballot((cnt >> bit) & 1);
        tot += __popcll(plane) << bit;
        pidx += __popcll(plane & below) << bit;
    }
    while (cm) {
        const int c = __builtin_ctzll(cm);
        cm &= cm - 1;
        if (pidx < kCap) list[pidx] = t0 + tiled_point(lane, c);
        ++pidx;
    }
    m += tot;
}

template <bool QUERY>
__global__ __launch_bounds__(256, 2) void knn_tiled_kernel(const float2 *__restrict__ pts,
                                                           const float2 *__restrict__ qry, int n_src,
                                                           int n_q, int k, int32_t *__restrict__ out,
                                                           int32_t *__restrict__ degenerate) {
    typedef KeyTraits<QUERY> KT;
    typedef typename KT::key_t key_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char tiled_lds[];
    float2 *sT = (float2 *)tiled_lds;

    const int b = blockIdx.y;
    const float2 *P = pts + (int64_t)b * n_src;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int kk = QUERY ? k : k + 1;
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const int qbase = (int)blockIdx.x * kTiledQueries + wave * kTiledQW;
    int *lists = (int *)(tiled_lds + kTiledOffList) + wave * kTiledQW * kCap;
    float2 *sQ = (float2 *)(tiled_lds + kTiledOffQ) + wave * kTiledQW;
    int *sM = (int *)(tiled_lds + kTiledOffM) + wave * kTiledQW;

    // queries past n_q (the last workgroup) repeat the last one and are not written
    float2 q[kTiledQW];
    uint32_t lmin[kTiledQW];
#pragma unroll
    for (int u = 0; u < kTiledQW; ++u) {
        const int qi = min(qbase + u, n_q - 1);
        q[u] = QUERY ? qry[(int64_t)b * n_q + qi] : P[qi];
        lmin[u] = ~0u;
    }
    // A tile goes global -> registers -> LDS, and the next tile's loads are
    // issued before the current one is searched, so they land behind its
    // arithmetic.  The last tile's unused slots take the previous tile's points
    // of the same slot, hence the same lane (n_src > kTile): a lane's minimum
    // over its own points with one repeated is its minimum, so pass 1 tests no
    // bound; pass 2 masks those slots out (valid).
    float2 nxt[kTile / 256];
    auto fetch = [&](int t0) {
        const int tn = min(kTile, n_src - t0);
#pragma unroll
        for (int i = 0; i < kTile / 256; ++i) {
            const int j = (int)threadIdx.x + 256 * i;
            nxt[i] = P[j < tn ? t0 + j : t0 + j - kTile];
        }
    };
    auto stage = [&](int t0) {
        __syncthreads();  // the previous tile's readers
#pragma unroll
        for (int i = 0; i < kTile / 256; ++i) {
            const int j = (int)threadIdx.x + 256 * i;  // column j >> 6, rotated by as many lanes
            sT[(j & ~63) + ((j + (j >> 6)) & 63)] = nxt[i];
        }
        __syncthreads();
        if (t0 + kTile < n_src) fetch(t0 + kTile);
    };
    fetch(0);
    for (int t0 = 0; t0 < n_src; t0 += kTile) {
        stage(t0);
#pragma unroll
        for (int g = 0; g < kTiledQW; g += kTiledQB) {
#pragma unroll 8
            for (int c = 0; c < kTile / 64; ++c) {
                const float2 p = sT[lane + 64 * c];
#pragma unroll
                for (int u = 0; u < kTiledQB; ++u) {
                    const uint32_t f = key_f32(p, q[g + u]);
                    lmin[g + u] = f < lmin[g + u] ? f : lmin[g + u];
                }
            }
        }
    }
    fetch(0);  // pass 2's first tile, behind the sorts
    uint32_t thr[kTiledQW];
    int m[kTiledQW];
#pragma unroll
    for (int u = 0; u < kTiledQW; ++u) {
        thr[u] = KT::filter_threshold(lane_value(wave_sort64(lmin[u], lane), kk - 1));
        m[u] = 0;
    }
    for (int t0 = 0; t0 < n_src; t0 += kTile) {
        const int tn = min(kTile, n_src - t0);
        stage(t0);
        uint64_t valid = ~0ull;  // bit c: this lane's slot of column c holds a point of this tile
        if (tn < kTile) {
            valid = 0ull;
            for (int c = 0; c < kTile / 64; ++c) valid |= (uint64_t)(tiled_point(lane, c) < tn) << c;
        }
#pragma unroll
        for (int g = 0; g < kTiledQW; g += kTiledQB) {
            uint64_t cm[kTiledQB];
#pragma unroll
            for (int u = 0; u < kTiledQB; ++u) cm[u] = 0ull;
            for (int c0 = 0; c0 < kTile / 64; c0 += 8) {
                uint32_t w[kTiledQB];
#pragma unroll
                for (int u = 0; u < kTiledQB; ++u) w[u] = 0u;
#pragma unroll
                for (int cc = 0; cc < 8; ++cc) {
                    const float2 p = sT[lane + 64 * (c0 + cc)];
#pragma unroll
                    for (int u = 0; u < kTiledQB; ++u)
                        w[u] |= (uint32_t)(key_f32(p, q[g + u]) <= thr[g + u]) << cc;
                }
#pragma unroll
                for (int u = 0; u < kTiledQB; ++u) cm[u] |= (uint64_t)w[u] << c0;
            }
#pragma unroll
            for (int u = 0; u < kTiledQB; ++u) tiled_append(cm[u] & valid, t0, lists + (g + u) * kCap, m[g + u], lane, below);
        }
    }
    // one copy of the selection code: the per-query registers go through LDS
#pragma unroll
    for (int u = 0; u < kTiledQW; ++u)
        if (lane == 0) {
            sQ[u] = q[u];
            sM[u] = m[u];
        }
    wave_lds_sync();
    const int cpl = (n_src + 63) / 64;
#pragma unroll 1
    for (int u = 0; u < kTiledQW && qbase + u < n_q; ++u)
        knn_finish<QUERY>(P, (key_t *)(tiled_lds + kTiledOffKey) + wave * kCap, lists + u * kCap,
                          (int *)(tiled_lds + kTiledOffSel) + wave * 64, sM[u], sQ[u], kk, k, qbase + u, b, n_src,
                          n_q, cpl, lane, below, out, degenerate);
}

template <bool QUERY>
int launch_knn_tiled(const float2 *p, const float2 *q, int64_t batches, int ns, int nq, int k, int32_t *out,
                     int32_t *degenerate, hipStream_t st) {
    const hipError_t e =
        hipFuncSetAttribute((const void *)knn_tiled_kernel<QUERY>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            kTiledLds);
    if (e != hipSuccess) return MMPDE_ERR_HIP_BASE - (int)e;
    dim3 grid(ceil_div(nq, kTiledQueries), (unsigned)batches);
    hipLaunchKernelGGL(knn_tiled_kernel<QUERY>, grid, dim3(256), kTiledLds, st, p, q, ns, nq, k, out, degenerate);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

__global__ void edge_index_kernel(const int32_t *__restrict__ nbr, int64_t n, int k,
                                  int64_t *__restrict__ ei) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ne = n * k;
    if (e < ne) {
        ei[e] = nbr[e];
        ei[ne + e] = e / k;
    }
}

// One wave per query (QUERY as in knn_kernel), 16 queries per workgroup.
//  1. the query's cell (cx, cy), clamped into the grid;
//  2. ring r adds the cells of the block [cx - r, cx + r] x [cy - r, cy + r]
//     (clipped) not yet scanned: the two end rows, each one contiguous range of
//     the sorted copy, and the two end cells of the rows between.  Scanned
//     point number t goes to lane t % 64, which keeps its smallest fp32 key;
//  3. every unscanned point lies in a cell beyond one of the block's sides that
//     still has cells beyond it, hence at least D = (the smallest distance from
//     the query to such a side) - eps away (bin kernel: eps), rounded down;
//  4. with cnt >= kk points scanned, U = the kk-th smallest lane minimum bounds
//     the kk-th smallest fp32 key of the whole set from above (min(cnt, 64) >=
//     kk lanes hold a point), thr = filter_threshold(U) as in knn_kernel;
//  5. stop when sqrt(thr) < D with the margins below (an unscanned point's
//     fp32 key is then above thr: it is no candidate), or when the block is
//     the whole grid;
//  6. the block's points with fp32 key <= thr, as original indices, are
//     compacted into the wave's list (block rows are contiguous ranges);
//  7. knn_finish with the trajectory's global pointer (as knn_tiled_kernel):
//     the same sorts, overflow select, counters and output.
// C = {fp32 key <= thr} is exactly the set the full-scan kernels would select
// with this thr, and any valid U gives the same answer.
// A header that was not written for this n_src (bins of another set) ends the
// wave before any indexed read; starts and indices are clamped into range.
template <bool QUERY>
__global__ __launch_bounds__(256) void knn_binned_kernel(const float2 *__restrict__ pts,
                                                         const float2 *__restrict__ qry,
                                                         const uint32_t *__restrict__ bins, int n_src,
                                                         int n_q, int k, int32_t *__restrict__ out,
                                                         int32_t *__restrict__ degenerate,
                                                         unsigned long long *__restrict__ stats) {
    typedef KeyTraits<QUERY> KT;
    typedef typename KT::key_t key_t;
    __shared__ key_t sKey[4][kCap];
    __shared__ int sIdx[4][kCap];
    __shared__ int sSel[4][64];

    const int b = blockIdx.y;
    const BinLayout lay = bins_layout(n_src);
    const float2 *P = pts + (int64_t)b * n_src;
    const uint32_t *W = bins + (int64_t)b * lay.stride;
    const float *H = (const float *)W;
    const float2 *SP = (const float2 *)(W + lay.sp);
    const int32_t *SI = (const int32_t *)(W + lay.si);
    const int *start = (const int *)(W + lay.start);
    const float x0 = H[0], y0 = H[1], hx = H[2], hy = H[3], ihx = H[4], ihy = H[5], eps = H[6];
    const int gx = (int)W[7], gy = (int)W[8];
    if (gx < 1 || gx > lay.G || gy < 1 || gy > lay.G || (int)W[9] != n_src) return;  // workgroup-uniform

    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int kk = QUERY ? k : k + 1;
    const int cpl = (n_src + 63) / 64;
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    auto range_lo = [&](int c) { return min(max(start[c], 0), n_src); };
    const int q_end = min((int)(blockIdx.x + 1) * kQueriesPerBlock, n_q);

    for (int qi = blockIdx.x * kQueriesPerBlock + wave; qi < q_end; qi += 4) {
        const float2 q = QUERY ? qry[(int64_t)b * n_q + qi] : P[qi];
        const int cx = bin_axis(q.x, x0, ihx, gx), cy = bin_axis(q.y, y0, ihy, gy);
        uint32_t lmin = ~0u, thr = ~0u;
        int cnt = 0;
        // points [lo, hi) of the sorted copy, the t-th scanned on lane t % 64
        auto scan = [&](int lo, int hi) {
            const int len = hi - lo;
            for (int o = (lane - cnt) & 63; o < len; o += 64) {
                const uint32_t f = key_f32(SP[lo + o], q);
                lmin = f < lmin ? f : lmin;
            }
            cnt += max(len, 0);
        };
        int cxlo, cxhi, cylo, cyhi;
        for (int r = 0;; ++r) {
            cxlo = max(cx - r, 0);
            cxhi = min(cx + r, gx - 1);
            cylo = max(cy - r, 0);
            cyhi = min(cy + r, gy - 1);
            for (int y = cylo; y <= cyhi; ++y) {
                const int row = y * gx;
                if (y == cy - r || y == cy + r) {
                    scan(range_lo(row + cxlo), range_lo(row + cxhi + 1));
                } else {
                    if (cx - r >= 0) scan(range_lo(row + cx - r), range_lo(row + cx - r + 1));
                    if (cx + r <= gx - 1) scan(range_lo(row + cx + r), range_lo(row + cx + r + 1));
                }
            }
            const bool whole = cxlo == 0 && cxhi == gx - 1 && cylo == 0 && cyhi == gy - 1;
            if (cnt >= kk) {
                const uint32_t u = lane_value(wave_sort64(lmin, lane), kk - 1);
                thr = KT::filter_threshold(u);
                if (whole) break;
                float d = 3.0e38f;
                if (cxlo > 0) d = fminf(d, q.x - (x0 + (float)cxlo * hx));
                if (cxhi < gx - 1) d = fminf(d, (x0 + (float)(cxhi + 1) * hx) - q.x);
                if (cylo > 0) d = fminf(d, q.y - (y0 + (float)cylo * hy));
                if (cyhi < gy - 1) d = fminf(d, (y0 + (float)(cyhi + 1) * hy) - q.y);
                d = (d - eps) * kDown;
                // An unscanned point is >= d away, so its fp32 key is >= d^2 (1 -
                // 2^-22) - 2^-126 (KeyTraits<true>), which exceeds thr when
                // sqrt(thr) kUp^2 < d and d^2 2^-19 covers the absolute term.
                // NaN (a non-finite query or thr) compares false: no stop.
                const float s = sqrtf(__uint_as_float(thr)) * kUp * kUp;
                if (u != ~0u && d > 1.0e-15f && s < d) break;
            } else if (whole) {
                thr = ~0u;  // fewer than kk points in the bins (not this set's): every point a candidate
                break;
            }
        }
        int m = 0;
        for (int y = cylo; y <= cyhi; ++y) {
            const int lo = range_lo(y * gx + cxlo), hi = range_lo(y * gx + cxhi + 1);
            for (int o0 = 0; o0 < hi - lo; o0 += 64) {
                const int o = o0 + lane;
                const bool sel = o < hi - lo && key_f32(SP[lo + o], q) <= thr;
                const uint64_t sm = __ballot(sel);
                const int pidx = m + __popcll(sm & below);
                if (sel && pidx < kCap) sIdx[wave][pidx] = min(max(SI[lo + o], 0), n_src - 1);
                m += __popcll(sm);
            }
        }
        if (stats && lane == 0) {
            atomicAdd(&stats[0], (unsigned long long)cnt);
            if (m > kCap) atomicAdd(&stats[1], 1ull);
        }
        knn_finish<QUERY>(P, sKey[wave], sIdx[wave], sSel[wave], m, q, kk, k, qi, b, n_src, n_q, cpl, lane, below,
                          out, degenerate);
    }
}

template <bool QUERY>
int launch_knn_binned(const float *pts, const float *qry, const void *bins, int64_t batches, int64_t n_src,
                      int64_t n_q, int k, int32_t *out, int32_t *degenerate, int64_t *stats, hipStream_t st) {
    const int kk = QUERY ? k : k + 1;
    // launch_knn's limits
    if (k < 1 || kk > 64 || n_src < kk || n_src > kTiledMax || n_q < 1 || batches < 1 || batches > 65535 ||
        n_q > INT32_MAX / 64 || batches * n_src > INT32_MAX)
        return MMPDE_ERR_INVALID_ARG;
    dim3 grid(ceil_div(n_q, kQueriesPerBlock), (unsigned)batches);
    hipLaunchKernelGGL(knn_binned_kernel<QUERY>, grid, dim3(256), 0, st, (const float2 *)pts, (const float2 *)qry,
                       (const uint32_t *)bins, (int)n_src, (int)n_q, k, out, degenerate,
                       (unsigned long long *)stats);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

}  // namespace

namespace mmpde_detail {

template <bool QUERY>
int launch_knn(const float *pts, const float *qry, int64_t batches, int64_t n_src, int64_t n_q,
               int k, int32_t *out, int32_t *degenerate, hipStream_t st, const uint8_t *miss,
               float *cells, int role) {
    const int kk = QUERY ? k : k + 1;
    if (k < 1 || kk > 64 || n_src < kk || n_src > kTiledMax || n_q < 1 || batches < 1 ||
        batches > 65535 || n_q > INT32_MAX / 64)
        return MMPDE_ERR_INVALID_ARG;
    // the miss mode is knn_kernel's alone, and reads the flags' record
    if (miss && (n_src > 4096 || !cells)) return MMPDE_ERR_INVALID_ARG;
    // the graph's indices are global int32
    if (n_src > kLargeMax && batches * n_src > INT32_MAX) return MMPDE_ERR_INVALID_ARG;
    dim3 grid(ceil_div(n_q, kQueriesPerBlock), (unsigned)batches);
    const int cpl = ceil_div(n_src, 64);
    const float2 *p = (const float2 *)pts;
    const float2 *q = (const float2 *)qry;
    const int ns = (int)n_src, nq = (int)n_q;
    if (n_src > kLargeMax) return launch_knn_tiled<QUERY>(p, q, batches, ns, nq, k, out, degenerate, st);
    if (n_src > 4096) return launch_knn_large<QUERY>(p, q, batches, ns, nq, k, out, degenerate, st);
#define MMPDE_KNN_CASE(C)                                                                     \
    if (cpl <= C) {                                                                           \
        hipLaunchKernelGGL((knn_kernel<C, QUERY>), grid, dim3(256), 0, st, p, q, ns, nq, k, out, \
                           degenerate, miss, cells, role);                                    \
        MMPDE_RET_LAUNCH();                                                                   \
        return MMPDE_OK;                                                                      \
    }
    MMPDE_KNN_CASE(4)
    MMPDE_KNN_CASE(8)
    MMPDE_KNN_CASE(16)
    MMPDE_KNN_CASE(24)
    MMPDE_KNN_CASE(32)
    MMPDE_KNN_CASE(40)
    MMPDE_KNN_CASE(48)
    MMPDE_KNN_CASE(56)
    MMPDE_KNN_CASE(64)
#undef MMPDE_KNN_CASE
    return MMPDE_ERR_UNSUPPORTED;
}

template int launch_knn<false>(const float *, const float *, int64_t, int64_t, int64_t, int, int32_t *,
                               int32_t *, hipStream_t, const uint8_t *, float *, int);
template int launch_knn<true>(const float *, const float *, int64_t, int64_t, int64_t, int, int32_t *,
                              int32_t *, hipStream_t, const uint8_t *, float *, int);

}  // namespace mmpde_detail

extern "C" int mmpde_knn_graph(const float *pos, int64_t batches, int64_t n_per, int k,
                               int32_t *nbr_out, int32_t *degenerate, mmpde_stream_t stream) {
    MMPDE_REQUIRE(pos && nbr_out);
    return mmpde_detail::launch_knn<false>(pos, nullptr, batches, n_per, n_per, k, nbr_out, degenerate,
                             as_stream(stream));
}

extern "C" int mmpde_knn_query(const float *src, const float *qry, int64_t batches,
                               int64_t n_src, int64_t n_qry, int k, int32_t *idx_out, int32_t *ties,
                               mmpde_stream_t stream) {
    MMPDE_REQUIRE(src && qry && idx_out);
    return mmpde_detail::launch_knn<true>(src, qry, batches, n_src, n_qry, k, idx_out, ties, as_stream(stream));
}

extern "C" int mmpde_edge_index_from_nbr(const int32_t *nbr, int64_t n, int k,
                                         int64_t *edge_index, mmpde_stream_t stream) {
    MMPDE_REQUIRE(nbr && edge_index && n > 0 && k > 0);
    const int64_t ne = n * k;
    hipLaunchKernelGGL(edge_index_kernel, dim3(ceil_div(ne, 256)), dim3(256), 0,
                       as_stream(stream), nbr, n, k, edge_index);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

extern "C" int mmpde_knn_graph_binned(const float *pos, const void *bins, int64_t batches, int64_t n_per, int k,
                                      int32_t *nbr_out, int32_t *degenerate, int64_t *stats,
                                      mmpde_stream_t stream) {
    MMPDE_REQUIRE(pos && bins && nbr_out && ((uintptr_t)bins & 7) == 0);
    return launch_knn_binned<false>(pos, nullptr, bins, batches, n_per, n_per, k, nbr_out, degenerate, stats,
                                    as_stream(stream));
}

extern "C" int mmpde_knn_query_binned(const float *src, const void *bins, const float *qry, int64_t batches,
                                      int64_t n_src, int64_t n_qry, int k, int32_t *idx_out, int32_t *ties,
                                      int64_t *stats, mmpde_stream_t stream) {
    MMPDE_REQUIRE(src && bins && qry && idx_out && ((uintptr_t)bins & 7) == 0);
    return launch_knn_binned<true>(src, qry, bins, batches, n_src, n_qry, k, idx_out, ties, stats,
                                   as_stream(stream));
}
