// The moved-mesh candidate table: the table and its displacement record, the
// candidate kernel, the skip threshold; what the table cannot answer goes to
// launch_knn's miss mode (knn.hip).  The file map: knn_common.hpp.
#include "knn_common.hpp"

namespace {

// ---------------------------------------------------------------------------
// Moving-mesh kNN from a static candidate list (exact, with a fallback).
// The DMM moves every node x_i = xi_i + d_i only a little, so the answer for a
// query q near a fixed reference point r_p (graph: r_p = xi_p, q = x_p; query:
// r_p = the fixed query point, q = qry_p) is almost always among cand[p] = the
// 128 nearest of r_p in the fixed mesh xi ((key, index) order).  A point j
// outside cand[p] has |xi_j - r_p| >= R = sqrt(key of cand[p][127]) (up to
// rounding), hence |x_j - q| >= max(R - |q - r_p|, dist(q, cell(xi_j))) -
// |d_j|, where cell(xi_j) is the point's cell in a 16 x 16 grid over the box of
// xi and |d_j| <= dcell[cell] = the largest displacement of that cell's points
// (mmpde_knn_moved_cells, per trajectory and step).  L = the minimum of that
// bound over the cells.  If the kk-th candidate distance is below L (every
// bound with a 2^-20 relative margin, which covers the fp32 rounding), no
// non-candidate can enter the first kk in (key, index) order, so the
// candidates sorted by (key, index) ARE the answer, ties included.  Otherwise
// the query joins its trajectory's fallback list, which knn_kernel answers.  A
// far-moved node only weakens the bound of the queries near its cell.
// ---------------------------------------------------------------------------
constexpr int kCandN = 128;

// Ascending bitonic sort of the 4096 slots of s (LDS) by a workgroup of 256
// threads; s is written and a barrier passed before the call, and the sorted
// slots are visible to every thread after it.
template <typename T>
__device__ __forceinline__ void block_sort4096(T *s) {
    for (int size = 2; size <= 4096; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < 2048; t += 256) {
                const int i = 2 * t - (t & (stride - 1)), l = i + stride;
                const T a = s[i], c = s[l];
                if ((a > c) == ((i & size) == 0)) {
                    s[i] = c;
                    s[l] = a;
                }
            }
            __syncthreads();
        }
}

// cand[p] = the kCandN nearest of r_p in xi, (key, index) order: one
// workgroup per point, (key << 32 | index) pairs bitonic-sorted in LDS.  Built
// once per fixed mesh (and query set).
__global__ __launch_bounds__(256) void knn_table_kernel(const float2 *__restrict__ xi,
                                                        const float2 *__restrict__ ref, int n_per,
                                                        int32_t *__restrict__ cand) {
    __shared__ uint64_t sk[4096];
    const int p = blockIdx.x;
    const float2 q = ref[p];
    for (int j = threadIdx.x; j < 4096; j += 256)
        sk[j] = j < n_per ? (((uint64_t)key_f32(xi[j], q) << 32) | (uint32_t)j) : ~0ull;
    __syncthreads();
    block_sort4096(sk);
    if (threadIdx.x < kCandN) cand[(int64_t)p * kCandN + threadIdx.x] = (int32_t)(uint32_t)sk[threadIdx.x];
}

// Per trajectory b (one workgroup each): the box of xi (x0, y0, cell sizes
// hx, hy, their inverses, a margin eps that covers the rounding of the cell
// assignment) and dcell[c] >= max |x_bj - xi_j| over the points j with xi_j in
// cell c (-1: empty cell).  rec[b] = {dcell[256], box[8]}.
// 1024 threads (16 waves): the point loops are 2.5 iterations per thread at
// N = 2521, and the median is a rank count (256 broadcast LDS reads per cell)
// instead of a 36-stage bitonic network with a barrier per stage.
constexpr int kCellThreads = 1024;
__global__ __launch_bounds__(kCellThreads) void knn_cells_kernel(const float2 *__restrict__ x,
                                                                 const float2 *__restrict__ xi, int n_per,
                                                                 float *__restrict__ rec) {
    constexpr int NW = kCellThreads / 64;
    __shared__ float red[NW][4];
    __shared__ uint32_t cell[kCells];
    __shared__ float srt[kCells];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float mnx = 3.0e38f, mny = 3.0e38f, mxx = -3.0e38f, mxy = -3.0e38f;
    for (int i = tid; i < n_per; i += kCellThreads) {
        const float2 c = xi[i];
        mnx = fminf(mnx, c.x);
        mny = fminf(mny, c.y);
        mxx = fmaxf(mxx, c.x);
        mxy = fmaxf(mxy, c.y);
    }
    mnx = -wave_max_full(-mnx);
    mny = -wave_max_full(-mny);
    mxx = wave_max_full(mxx);
    mxy = wave_max_full(mxy);
    if (lane == 0) {
        red[wave][0] = mnx;
        red[wave][1] = mny;
        red[wave][2] = mxx;
        red[wave][3] = mxy;
    }
    if (tid < kCells) cell[tid] = 0u;  // empty
    __syncthreads();
    float x0 = red[0][0], y0 = red[0][1], x1 = red[0][2], y1 = red[0][3];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        x0 = fminf(x0, red[w][0]);
        y0 = fminf(y0, red[w][1]);
        x1 = fmaxf(x1, red[w][2]);
        y1 = fmaxf(y1, red[w][3]);
    }
    const float hx = (x1 - x0) / kCellG, hy = (y1 - y0) / kCellG;
    const float ihx = hx > 0.0f ? 1.0f / hx : 0.0f, ihy = hy > 0.0f ? 1.0f / hy : 0.0f;
    for (int i = tid; i < n_per; i += kCellThreads) {
        const float2 a = x[(int64_t)b * n_per + i], c = xi[i];
        const float dx = a.x - c.x, dy = a.y - c.y;
        const float d = sqrtf(dx * dx + dy * dy) * kUp;
        const int cx = min(max((int)((c.x - x0) * ihx), 0), kCellG - 1);
        const int cy = min(max((int)((c.y - y0) * ihy), 0), kCellG - 1);
        // non-negative floats order like their bits; stored as bits + 1 so
        // that 0 marks an empty cell
        atomicMax(&cell[cy * kCellG + cx], __float_as_uint(d) + 1u);
    }
    __syncthreads();
    float *r = rec + (int64_t)b * kCellRec;
    // cells on threads 0 .. 255 (waves 0 - 3)
    const uint32_t v = tid < kCells ? cell[tid] : 0u;
    const float dc = v == 0u ? -1.0f : __uint_as_float(v - 1u);
    if (tid < kCells) {
        r[tid] = dc;
        // the median over the non-empty cells of their largest displacement (the
        // statistic skip_above is compared with), empty cells last
        srt[tid] = v == 0u ? 3.0e38f : dc;
    }
    const float dall = wave_max_full(fmaxf(dc, 0.0f));
    const int nonempty = __popcll(__ballot(v != 0u));
    __syncthreads();  // red (read above) and srt
    if (lane == 0 && wave < kCells / 64) {
        red[wave][0] = dall;
        red[wave][1] = __int_as_float(nonempty);
    }
    __syncthreads();
    const int ne = __float_as_int(red[0][1]) + __float_as_int(red[1][1]) + __float_as_int(red[2][1]) +
                   __float_as_int(red[3][1]);
    if (tid < kCells) {
        // rank of this cell's value in (value, cell) order; the one of rank
        // ne / 2 is element ne / 2 of the sorted list
        const float mine = srt[tid];
        int rank = 0;
        for (int u = 0; u < kCells; ++u) {
            const float o = srt[u];
            rank += (o < mine || (o == mine && u < tid)) ? 1 : 0;
        }
        if (ne > 0 && rank == ne / 2) r[kCells + 6] = mine;
    }
    if (tid == 0) {
        const float eps = 1.0e-5f * fmaxf(x1 - x0, y1 - y0);
        r[kCells + 0] = x0;
        r[kCells + 1] = y0;
        r[kCells + 2] = hx;
        r[kCells + 3] = hy;
        r[kCells + 4] = eps;
        r[kCells + 5] = fmaxf(fmaxf(red[0][0], red[1][0]), fmaxf(red[2][0], red[3][0]));
        if (ne == 0) r[kCells + 6] = 0.0f;
        for (int i = 0; i < 2; ++i) {
            cell_last_miss(rec, b)[i] = 0;
            cell_any_miss(rec, b)[i] = 0;
            cell_skipped(rec, b)[i] = 0;
        }
    }
}

// Lower bounds on |x_j - q| over every j outside cand[p] (see above), <= 0 when
// they prove nothing; every rounding step errs downward.  R = the 128th
// candidate's distance from r_p, rq = R - |q - r_p|.  The global bound takes
// the trajectory's largest displacement; the per-cell bound, per cell, the
// distance from q to the cell's box (widened by eps) less the cell's largest
// displacement (never below the global one, costlier: only when that fails).
__device__ __forceinline__ float cand_rq(const float2 *__restrict__ xi, float2 rp, int n_per,
                                         const int32_t *__restrict__ cr, float2 q) {
    const int jl = min(max(cr[kCandN - 1], 0), n_per - 1);
    const float R = sqrtf(__uint_as_float(key_f32(xi[jl], rp))) * kDown;
    const float ddx = q.x - rp.x, ddy = q.y - rp.y;
    const float dq = sqrtf(ddx * ddx + ddy * ddy) * kUp;
    return (R - dq * kUp) * kDown;
}

__device__ __forceinline__ float cand_bound_global(float rq, const float *__restrict__ rec) {
    return (rq - rec[kCells + 5] * kUp) * kDown;
}

__device__ __forceinline__ float cand_bound_cells(float rq, float2 q, const float *__restrict__ rec, int lane) {
    const float x0 = rec[kCells], y0 = rec[kCells + 1], hx = rec[kCells + 2], hy = rec[kCells + 3];
    const float eps = rec[kCells + 4];
    float L = 3.0e38f;
    // every cell's record loaded first (a load whose value decides a branch
    // is waited for at once: one memory round trip per cell group otherwise),
    // then the bound of each occupied cell (dc >= 0) taken by a select
    float dcs[kCells / 64];
#pragma unroll
    for (int t = 0; t < kCells / 64; ++t) dcs[t] = rec[lane + 64 * t];
#pragma unroll
    for (int t = 0; t < kCells / 64; ++t) {
        const int c = lane + 64 * t;
        const float dc = dcs[t];
        const int cx = c % kCellG, cy = c / kCellG;
        const float lx = x0 + cx * hx - eps, ux = x0 + (cx + 1) * hx + eps;
        const float ly = y0 + cy * hy - eps, uy = y0 + (cy + 1) * hy + eps;
        const float ex = fmaxf(fmaxf(lx - q.x, q.x - ux), 0.0f);
        const float ey = fmaxf(fmaxf(ly - q.y, q.y - uy), 0.0f);
        const float dist = sqrtf(ex * ex + ey * ey) * kDown;
        const float bound = (fmaxf(dist, rq) - dc * kUp) * kDown;
        L = dc >= 0.0f ? fminf(L, bound) : L;
    }
    return -wave_max(-L);
}

// One wave per query point: the 128 candidates' keys (two per lane), those that
// can be among the first kk selected and sorted by (key, index) -- 64 wide in
// one register when at most 64 remain, else the 128-wide sort of all; the
// first kk are the answer when the kk-th candidate is closer than the bound.
// QUERY = false: the moved-mesh graph
// (fp32 keys, self dropped, global indices, as knn_finish's graph branch; ref =
// xi); true: the kNN query of qry onto the moved mesh (fp64 keys, local
// indices; ref = the fixed query points the table was built for).
template <bool QUERY>
__global__ __launch_bounds__(256) void knn_cand_kernel(const float2 *__restrict__ x,
                                                       const float2 *__restrict__ qry,
                                                       const float2 *__restrict__ xi,
                                                       const float2 *__restrict__ ref, int n_per,
                                                       int64_t n_tot, int k,
                                                       const int32_t *__restrict__ cand,
                                                       const float *__restrict__ cells,
                                                       int32_t *__restrict__ out,
                                                       int32_t *__restrict__ degenerate,
                                                       uint8_t *__restrict__ miss, float skip_above) {
    typedef KeyTraits<QUERY> KT;
    typedef typename KT::key_t key_t;
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n_tot) return;  // wave-uniform
    const int b = (int)(p / n_per);
    const int pl = (int)(p - (int64_t)b * n_per);
    const float *rec = cells + (int64_t)b * kCellRec;
    // a trajectory whose median cell displacement exceeds skip_above does not
    // try the table: the fallback answers all its queries (wave-uniform)
    if (skip_above > 0.0f && rec[kCells + 6] > skip_above) {
        if (pl == 0 && lane == 0) cell_skipped(cells, b)[QUERY ? 1 : 0] = 1;
        return;
    }
    const float2 *X = x + (int64_t)b * n_per;
    const float2 q = QUERY ? qry[p] : X[pl];
    const int32_t *cr = cand + (int64_t)pl * kCandN;
    const float2 rp = ref[pl];
    const float rq = cand_rq(xi, rp, n_per, cr, q);
    const int kk = QUERY ? k : k + 1;
    // a query the table cannot answer is flagged for the fallback
    auto give_up = [&]() {
        if (lane == 0) {
            miss[p] = 1;
            cell_any_miss(cells, b)[QUERY ? 1 : 0] = 1;
        }
    };

    // Given up (wave-uniform) when the bound proves nothing, or when already
    // the unmoved kk-th candidate lies beyond it: the moved one then almost
    // never passes, and the sort would be wasted.  A heuristic only -- the
    // test after the sort decides.  The per-cell bound only when the global
    // one fails.
    const int jk = min(max(cr[kk - 1], 0), n_per - 1);
    const float dk0 = sqrtf(__uint_as_float(key_f32(xi[jk], rp)));
    float L = cand_bound_global(rq, rec);
    bool cells_done = false;
    if (!(L > 0.0f) || dk0 >= L) {
        L = cand_bound_cells(rq, q, rec, lane);
        cells_done = true;
        if (!(L > 0.0f) || dk0 >= L) {
            give_up();
            return;
        }
    }
    int i0 = min(max(cr[lane], 0), n_per - 1), i1 = min(max(cr[64 + lane], 0), n_per - 1);
    key_t k0 = 0, k1 = 0;
    bool sorted = false, tie = false;  // tie: as knn_finish's (QUERY)
    // Select before sorting.  The candidates come in the unmoved mesh's
    // distance order and the mesh moves little, so U = the largest moved fp32
    // key among the first kk candidates bounds the kk-th smallest key tightly:
    // kk candidates have key <= U.  With thr = filter_threshold(U) every
    // selected key (<= thr) is below every other, so the selected set C (m
    // elements, kk <= m) sorted by (fp32 key, index) is the first m of the
    // 128-wide sort; and (QUERY, the proof above filter_threshold) every point
    // whose fp64 key is at most the kk-th smallest fp64 key is in C, so C
    // sorted by (fp64 key, index) starts with the 128-wide sort's first kk,
    // followed by a point that ties rank kk - 1 whenever one exists.  With
    // m <= 64, C is packed one per lane -- the selected second-register
    // elements move into unselected first-register lanes through this wave's
    // LDS list (written at their rank, read by free-lane rank: no atomics, the
    // same packing whatever the schedule), the other lanes get the maximal key
    // -- and sorted by the 64-wide one-register network: 21 compare-exchange
    // stages on one (key, index) pair instead of 27 on two.  Lanes < m then
    // hold what the 128-wide sort leaves there.  m > 64: the 128-wide sort.
    __shared__ uint32_t sMoveF[4][64];
    __shared__ int sMoveI[4][64];
    const uint32_t f0 = key_f32(X[i0], q), f1 = key_f32(X[i1], q);
    const uint32_t thr = KT::filter_threshold(wave_umax(lane < kk ? f0 : 0u, lane));
    const bool s0 = f0 <= thr, s1 = f1 <= thr;
    const uint64_t b0 = __ballot(s0), b1 = __ballot(s1);
    const int m1 = __popcll(b1), m = __popcll(b0) + m1;
    const bool narrow = m <= 64;  // wave-uniform
    uint32_t cf = s0 ? f0 : 0xffffffffu;  // C, one per lane: fp32 key (maximal: none) and index
    int ci = i0;                          // (always a valid point index)
    if (narrow) {
        const int wv = threadIdx.x >> 6;
        const uint32_t lo0 = (uint32_t)b0, hi0 = (uint32_t)(b0 >> 32), lo1 = (uint32_t)b1, hi1 = (uint32_t)(b1 >> 32);
        if (s1) {
            const int r = (int)__builtin_amdgcn_mbcnt_hi(hi1, __builtin_amdgcn_mbcnt_lo(lo1, 0u));
            sMoveF[wv][r] = f1;
            sMoveI[wv][r] = i1;
        }
        wave_lds_sync();
        const int fr = (int)__builtin_amdgcn_mbcnt_hi(~hi0, __builtin_amdgcn_mbcnt_lo(~lo0, 0u));
        if (!s0 && fr < m1) {
            cf = sMoveF[wv][fr];
            ci = sMoveI[wv][fr];
        }
    }
    if constexpr (QUERY) if (kk < 64) {
        // sklearn's fp64 order, found by the cheaper fp32 (key, index) sort and
        // checked exactly: ranks 0 .. kk-1 must be in fp64 (key, index) order
        // (adjacent pairs compared on their exact keys), and the fp32 key of
        // rank kk must exceed rank kk-1's by the 64-ulp filter margin
        // (KeyTraits<true>::filter_threshold: the fp32 key is within 2^-22
        // relative of the fp64 one), so no later candidate's fp64 key can be
        // below rank kk-1's.  Otherwise (ties, near-ties) the fp64 sort below.
        uint32_t g0 = narrow ? cf : f0, g1 = f1;
        int j0 = narrow ? ci : i0, j1 = i1;
        if (narrow) wave_sort64_ki(g0, j0, lane);
        else wave_sort128(g0, j0, g1, j1, lane);
        const uint64_t e0 = KT::key(X[j0], q);
        const uint64_t en = __shfl(e0, (lane + 1) & 63, 64);
        const int jn = __shfl(j0, (lane + 1) & 63, 64);
        const bool pair_ok = lane >= kk - 1 || ki_less(e0, j0, en, jn);
        // rank kk's fp32 key: with m == kk it is not in C but the smallest key outside it
        const uint32_t fk = m == kk ? wave_umin(min(s0 ? 0xffffffffu : f0, s1 ? 0xffffffffu : f1), lane)
                                    : lane_value(g0, kk);
        const uint32_t fk1 = lane_value(g0, kk - 1);
        if (__ballot(!pair_ok) == 0ull && fk > KT::filter_threshold(fk1)) {
            k0 = e0;
            i0 = j0;
            sorted = true;
            // rank kk's fp64 key exceeds rank kk - 1's (the margin): ties only inside
            tie = __ballot(lane < kk - 1 && e0 == en) != 0ull;
        }
    }
    if (!sorted && narrow) {
        // C by exact key.  Rank kk, when m > kk, sits in lane kk; with m == kk no
        // point outside C ties rank kk - 1 (QUERY: its fp32 key exceeds the
        // filter margin over every selected one's), so lane kk - 1 reports none.
        i0 = ci;
        if constexpr (QUERY) k0 = cf == 0xffffffffu ? ~key_t(0) : KT::key(X[ci], q);
        else k0 = cf;
        wave_sort64_ki(k0, i0, lane);
        if (QUERY) {
            const key_t n0 = (key_t)__shfl((unsigned long long)k0, (lane + 1) & 63, 64);
            tie = __ballot(lane < kk && lane + 1 < m && k0 == n0) != 0ull;
        }
    } else if (!sorted) {
        k0 = KT::key(X[i0], q);
        k1 = KT::key(X[i1], q);
        wave_sort128(k0, i0, k1, i1, lane);
        if (QUERY) {  // element lane + 1 (lane 63: element 64, k1 of lane 0)
            const key_t n0 = (key_t)__shfl((unsigned long long)k0, (lane + 1) & 63, 64);
            const key_t n1 = lane_value(k1, 0);
            tie = __ballot(lane < kk && k0 == (lane == 63 ? n1 : n0)) != 0ull;
        }
    }
    const key_t key_kk = lane_value(k0, kk - 1);
    float d_kk;
    if constexpr (QUERY)
        d_kk = (float)sqrt(__longlong_as_double((long long)key_kk)) * kUp;
    else
        d_kk = sqrtf(__uint_as_float(key_kk)) * kUp;
    if (!(d_kk < L) && !cells_done) L = cand_bound_cells(rq, q, rec, lane);
    if (!(d_kk < L)) {  // same on every lane
        give_up();
        return;
    }
    if (lane == 0) miss[p] = 0;
    const int mi = i0, rank = lane;
    if (QUERY) {
        if (lane < kk) out[p * k + rank] = mi;
        if (tie && lane == 0 && degenerate) atomicAdd(degenerate, 1);
    } else {
        const uint64_t smask = __ballot(lane < kk && mi == pl);
        const bool has_self = smask != 0ull;
        const int self_rank = has_self ? lane_value(rank, __ffsll((unsigned long long)smask) - 1) : kk;
        const int pos = rank - ((has_self && rank > self_rank) ? 1 : 0);
        if (lane < kk && !(has_self && mi == pl) && pos < k) out[p * k + pos] = b * n_per + mi;
        if (!has_self && lane == 0 && degenerate) atomicAdd(degenerate, 1);
    }
}

}  // namespace

extern "C" int mmpde_knn_candidates(const float *xi, const float *ref, int64_t n_per, int32_t *cand_out,
                                    mmpde_stream_t stream) {
    MMPDE_REQUIRE(xi && cand_out && n_per >= kCandN && n_per <= 4096);
    hipLaunchKernelGGL(knn_table_kernel, dim3((unsigned)n_per), dim3(256), 0, as_stream(stream),
                       (const float2 *)xi, (const float2 *)(ref ? ref : xi), (int)n_per, cand_out);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

extern "C" int64_t mmpde_knn_moved_cells_bytes(int64_t batches) {
    return batches < 0 ? 0 : batches * kCellRec * (int64_t)sizeof(float);
}

extern "C" int mmpde_knn_moved_cells(const float *pos, const float *xi, int64_t batches, int64_t n_per,
                                     float *cells_out, mmpde_stream_t stream) {
    MMPDE_REQUIRE(pos && xi && cells_out && batches >= 1 && batches <= 65535 && n_per >= 1 &&
                  n_per <= INT32_MAX);
    hipLaunchKernelGGL(knn_cells_kernel, dim3((unsigned)batches), dim3(kCellThreads), 0, as_stream(stream),
                       (const float2 *)pos, (const float2 *)xi, (int)n_per, cells_out);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

// The median over reference points p of R128(p) - R_kk(p) (the 128th and the
// kk-th candidate distance of r_p in xi), times `scale`.  One workgroup,
// bitonic sort in LDS.
__global__ __launch_bounds__(256) void knn_margin_kernel(const float2 *__restrict__ xi,
                                                         const float2 *__restrict__ ref, int n_per,
                                                         const int32_t *__restrict__ cand, int kk,
                                                         float scale, float *__restrict__ out) {
    __shared__ float sm[4096];
    for (int p = threadIdx.x; p < 4096; p += 256) {
        float m = 3.0e38f;
        if (p < n_per) {
            const float2 r = ref[p];
            const int32_t *cr = cand + (int64_t)p * kCandN;
            const int j1 = min(max(cr[kCandN - 1], 0), n_per - 1), jk = min(max(cr[kk - 1], 0), n_per - 1);
            m = sqrtf(__uint_as_float(key_f32(xi[j1], r))) - sqrtf(__uint_as_float(key_f32(xi[jk], r)));
        }
        sm[p] = m;
    }
    __syncthreads();
    block_sort4096(sm);
    if (threadIdx.x == 0) out[0] = scale * sm[n_per / 2];
}

__global__ void knn_misses_kernel(const float *__restrict__ cells, int batches, int32_t *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * batches) out[i] = cell_last_miss(cells, i >> 1)[i & 1];
}

extern "C" int mmpde_knn_table_misses(const float *cells, int64_t batches, int32_t *misses_out,
                                      mmpde_stream_t stream) {
    MMPDE_REQUIRE(cells && misses_out && batches >= 1 && batches <= 65535);
    hipLaunchKernelGGL(knn_misses_kernel, dim3(ceil_div(2 * batches, 256)), dim3(256), 0, as_stream(stream),
                       cells, (int)batches, misses_out);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

extern "C" int mmpde_knn_skip_threshold(const float *xi, const float *ref, int64_t n_per, const int32_t *cand,
                                        int kk, int moved_queries, float *out, mmpde_stream_t stream) {
    MMPDE_REQUIRE(xi && cand && out && n_per >= kCandN && n_per <= 4096 && kk >= 1 && kk <= kCandN);
    // a moved query spends the margin twice (its own offset and its
    // neighbours' displacement), a query at its reference point once
    hipLaunchKernelGGL(knn_margin_kernel, dim3(1), dim3(256), 0, as_stream(stream), (const float2 *)xi,
                       (const float2 *)(ref ? ref : xi), (int)n_per, cand, kk, moved_queries ? 0.5f : 1.0f,
                       out);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

extern "C" int64_t mmpde_knn_graph_cand_scratch_bytes(int64_t batches, int64_t n_per) {
    return batches * n_per;  // the miss flags
}

// The candidate path: the candidate kernel, then the full search for the
// queries it could not answer (knn_kernel's miss mode: its cost follows the
// number of such queries, and is the plain search's when most missed).
template <bool QUERY>
static int knn_cand_launch(const float *pos, const float *qry, const float *xi, const float *ref,
                           const float *cells, float skip_above, int64_t batches, int64_t n_per, int k,
                           const int32_t *cand, int32_t *out, int32_t *degenerate, void *scratch,
                           hipStream_t st) {
    uint8_t *miss = (uint8_t *)scratch;
    const int64_t n_tot = batches * n_per;
    const float2 *x = (const float2 *)pos, *q = (const float2 *)qry, *x0 = (const float2 *)xi;
    hipLaunchKernelGGL(knn_cand_kernel<QUERY>, dim3((unsigned)ceil_div(n_tot, 4)), dim3(256), 0, st, x, q, x0,
                       (const float2 *)ref, (int)n_per, n_tot, k, cand, cells, out, degenerate, miss,
                       skip_above);
    MMPDE_RET_LAUNCH();
    // n_src = n_q = n_per; the graph's queries are the points themselves
    return mmpde_detail::launch_knn<QUERY>(pos, QUERY ? qry : pos, batches, n_per, n_per, k, out, degenerate,
                                           st, miss, (float *)cells, QUERY ? 1 : 0);
}

static bool cand_path_applies(int64_t batches, int64_t n_per, int kk) {
    // the answer inside the first 64 sorted candidates; the register kernels' sizes
    return kk >= 1 && kk <= 64 && n_per >= kCandN && n_per <= 4096 && batches >= 1 && batches <= 65535 &&
           batches * n_per <= INT32_MAX;
}

extern "C" int mmpde_knn_graph_cand(const float *pos, const float *xi, const float *cells, float skip_above,
                                    int64_t batches, int64_t n_per, int k, const int32_t *cand, int32_t *nbr_out,
                                    int32_t *degenerate, void *scratch, mmpde_stream_t stream) {
    MMPDE_REQUIRE(pos && xi && cells && cand && nbr_out && scratch);
    hipStream_t st = as_stream(stream);
    if (k < 1 || !cand_path_applies(batches, n_per, k + 1))
        return mmpde_detail::launch_knn<false>(pos, nullptr, batches, n_per, n_per, k, nbr_out, degenerate, st);
    return knn_cand_launch<false>(pos, nullptr, xi, xi, cells, skip_above, batches, n_per, k, cand, nbr_out,
                                  degenerate, scratch, st);
}

extern "C" int mmpde_knn_query_cand(const float *src, const float *qry, const float *xi, const float *ref,
                                    const float *cells, float skip_above, int64_t batches, int64_t n_per, int k,
                                    const int32_t *cand, int32_t *idx_out, int32_t *ties, void *scratch,
                                    mmpde_stream_t stream) {
    MMPDE_REQUIRE(src && qry && xi && cells && cand && idx_out && scratch);
    hipStream_t st = as_stream(stream);
    if (!cand_path_applies(batches, n_per, k))
        return mmpde_detail::launch_knn<true>(src, qry, batches, n_per, n_per, k, idx_out, ties, st);
    return knn_cand_launch<true>(src, qry, xi, ref ? ref : xi, cells, skip_above, batches, n_per, k, cand,
                                 idx_out, ties, scratch, st);
}
