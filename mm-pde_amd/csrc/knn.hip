// Batched exact k-nearest-neighbour search for gfx950.
//
// Replaces torch_cluster.knn_graph (reference data_creator_2d.py:260,
// mesh/dmm_model.py:228) and sklearn NearestNeighbors.kneighbors
// (data_creator_2d.py:66-78).  One wave per query; the trajectory's point set
// (<= 4096 points, <= 32 KB) is staged once per workgroup in LDS; every lane
// keeps CPL fp32 squared distances in registers (larger sets, up to 16384
// points: knn_large_kernel below; up to 65536: knn_tiled_kernel, which streams
// the set through LDS in tiles; knn_binned_kernel, far below, scans only the
// cells of a uniform grid around the query).  Selection: U = the kk-th
// smallest of the 64 per-lane minima (a 64-wide bitonic sort across the wave)
// bounds the kk-th smallest key from above; the points with key <= U (a few
// dozen on a mesh; for the fp64 query key, fp32 key <= U plus a proven
// rounding margin) are compacted into a per-wave LDS list, their exact keys
// formed, and sorted by (key, index) with a 128-wide two-per-lane bitonic
// network.  Longer lists are ranked exhaustively; lists past kCap fall back to
// a full bitwise radix select over all exact keys with ties at the threshold
// taken in index order.  Every way the result is exactly the
// (distance, index)-ordered list of the reference's insertion sort,
// independent of scheduling.
//
// Distance keys (must match oracle/knn_oracle.c bit for bit):
//   graph: d2 = fmaf(dy, dy, dx*dx) in fp32  (torch_cluster under nvcc fmad)
//   query: d2 = dx*dx + dy*dy in fp64        (sklearn float64 rdist)
// Non-negative IEEE values order like their bit patterns, so keys are the
// raw bits.
#include <type_traits>

#include "common.hpp"

namespace {

constexpr int kQueriesPerBlock = 16;  // 4 per wave
constexpr int kCap = 256;             // LDS list of candidates with key <= U, per wave

// Moved-mesh displacement record (mmpde_knn_moved_cells), per trajectory:
// dcell[kCells] (-1: empty cell), box (x0, y0, hx, hy, eps), the largest
// displacement, then per role (0: graph, 1: query) the count of queries the
// candidate table could not answer in the last call (written by the
// fallback; diagnostics).
constexpr int kCellG = 16;                           // cells per axis
constexpr int kCells = kCellG * kCellG;
constexpr int kCellRec = kCells + 16;                // floats per trajectory record
__device__ __forceinline__ int32_t *cell_last_miss(const float *cells, int b) {
    return (int32_t *)(cells + (int64_t)b * kCellRec + kCells + 8);  // [role]
}
// set (plain stores of 1) by knn_cand_kernel when any query of the trajectory
// missed, zeroed with the record: a fallback workgroup of a trajectory without
// misses returns at once
__device__ __forceinline__ int32_t *cell_any_miss(const float *cells, int b) {
    return (int32_t *)(cells + (int64_t)b * kCellRec + kCells + 10);  // [role]
}
// set by knn_cand_kernel when the trajectory skipped the table (skip_above):
// the fallback then answers all its queries without reading the flags
__device__ __forceinline__ int32_t *cell_skipped(const float *cells, int b) {
    return (int32_t *)(cells + (int64_t)b * kCellRec + kCells + 12);  // [role]
}

// fp32 squared distance as raw bits: the graph key, and the query's filter key.
__device__ __forceinline__ uint32_t key_f32(float2 p, float2 q) {
#pragma clang fp contract(off)
    float dx = p.x - q.x;
    float dy = p.y - q.y;
    float a = dx * dx;
    return __float_as_uint(fmaf(dy, dy, a));
}

template <bool QUERY>
struct KeyTraits;

template <>
struct KeyTraits<false> {
    typedef uint32_t key_t;
    static constexpr int kTopBit = 30;  // valid keys are < 2^31
    __device__ static key_t key(float2 p, float2 q) { return key_f32(p, q); }
    // the filter key is the key itself
    __device__ static uint32_t filter_threshold(uint32_t u) { return u; }
};

template <>
struct KeyTraits<true> {
    typedef uint64_t key_t;
    static constexpr int kTopBit = 62;  // valid keys are < 2^63
    __device__ static key_t key(float2 p, float2 q) {
#pragma clang fp contract(off)
        double dx = (double)p.x - (double)q.x;
        double dy = (double)p.y - (double)q.y;
        double a = dx * dx;
        double c = dy * dy;
        return (key_t)__double_as_longlong(a + c);
    }
    // Candidates are filtered on the fp32 key f, whose relative error against
    // the fp64 key is <= 2^-22 (<= 4 ulp: two rounded differences, two
    // rounded products / one fma); an absolute 2^-126 covers denormal
    // flushing.  If u is the kk-th smallest fp32 lane minimum, at least kk
    // points have fp64 key <= u (1 + 2^-22) + 2^-126, hence so does every
    // point of the answer, whose fp32 key is then <= u + ~9 ulp.  A 64-ulp
    // margin over max(u, min normal) keeps every answer point a candidate.
    __device__ static uint32_t filter_threshold(uint32_t u) {
        return u >= 0x7f000000u ? 0xfffffffeu : (u < 0x00800000u ? 0x00800000u : u) + 64u;
    }
};

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// v of lane ^ j without the LDS pipe (ds_bpermute's round trip would sit on
// every step of the sorting networks): DPP quad_perm for j = 1, 2; DPP
// row_shl / row_shr by j plus a select for j = 4, 8 (row_shl:j reads lane + j);
// v_permlane16_swap / v_permlane32_swap of v with itself for j = 16, 32 (the
// swap moves odd rows of its first operand with even rows of its second /
// the upper half of the first with the lower half of the second).  j must fold
// to a constant: the networks below are fully unrolled.
__device__ __forceinline__ uint32_t xor_lane(uint32_t v, int j, int lane) {
    const int x = (int)v;
    switch (j) {
    case 1:
        return (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false);  // [1,0,3,2]
    case 2:
        return (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false);  // [2,3,0,1]
    case 4: {
        const int up = __builtin_amdgcn_update_dpp(0, x, 0x104, 0xF, 0xF, false);
        const int dn = __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, false);
        return (uint32_t)((lane & 4) ? dn : up);
    }
    case 8: {
        const int up = __builtin_amdgcn_update_dpp(0, x, 0x108, 0xF, 0xF, false);
        const int dn = __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, false);
        return (uint32_t)((lane & 8) ? dn : up);
    }
    case 16: {
        const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
        return (lane & 16) ? r[0] : r[1];
    }
    default: {  // 32
        const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return (lane & 32) ? r[0] : r[1];
    }
    }
}

// v of lane l, l wave-uniform (a kernel argument or from a ballot): v_readlane
// into an SGPR instead of a ds_bpermute round trip (the same value).
template <typename T>
__device__ __forceinline__ T lane_value(T v, int l) {
    if constexpr (sizeof(T) == 8) {
        const uint64_t u = (uint64_t)v;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, l);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l);
        return (T)(((uint64_t)hi << 32) | lo);
    } else {
        return (T)__builtin_amdgcn_readlane((int)v, l);
    }
}

template <typename K>
__device__ __forceinline__ K shfl_xor_key(K v, int m, int lane) {
    if constexpr (sizeof(K) == 8) {
        const uint32_t lo = xor_lane((uint32_t)v, m, lane);
        const uint32_t hi = xor_lane((uint32_t)(v >> 32), m, lane);
        return ((K)hi << 32) | lo;
    } else {
        return xor_lane(v, m, lane);
    }
}

// Maximum / minimum of v over the wave's 64 lanes (all active), on every lane.
__device__ __forceinline__ uint32_t wave_umax(uint32_t v, int lane) {
#pragma unroll
    for (int j = 1; j <= 32; j <<= 1) v = max(v, xor_lane(v, j, lane));
    return v;
}
__device__ __forceinline__ uint32_t wave_umin(uint32_t v, int lane) {
#pragma unroll
    for (int j = 1; j <= 32; j <<= 1) v = min(v, xor_lane(v, j, lane));
    return v;
}

// Bitonic sort of one key per lane across the wave, ascending in lane order.
template <typename K>
__device__ __forceinline__ K wave_sort64(K v, int lane) {
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int j = size >> 1; j > 0; j >>= 1) {
            const K o = shfl_xor_key(v, j, lane);
            const bool keep_min = ((lane & j) == 0) == ((lane & size) == 0);
            v = keep_min ? (o < v ? o : v) : (o < v ? v : o);
        }
    }
    return v;
}

__device__ __forceinline__ bool ki_less(uint32_t ka, int ia, uint32_t kb, int ib) {
    // 31-bit keys and 12-bit indices: one 64-bit compare
    return (((uint64_t)ka << 32) | (uint32_t)ia) < (((uint64_t)kb << 32) | (uint32_t)ib);
}
__device__ __forceinline__ bool ki_less(uint64_t ka, int ia, uint64_t kb, int ib) {
    return ka < kb || (ka == kb && ia < ib);
}

// One compare-exchange step of the 128-wide network on register r of this
// lane against lane ^ j (same register), keeping the min iff keep_min.
template <typename K>
__device__ __forceinline__ void cx_lane(K &k, int &i, int j, bool keep_min, int lane) {
    const K ok = shfl_xor_key(k, j, lane);
    const int oi = (int)xor_lane((uint32_t)i, j, lane);
    const bool take = ki_less(ok, oi, k, i) == keep_min;
    k = take ? ok : k;
    i = take ? oi : i;
}

// Bitonic sort of 64 (key, index) pairs, one per lane, ordered
// lexicographically (the reference's tie order).  Ascending in lane.
template <typename K>
__device__ __forceinline__ void wave_sort64_ki(K &k, int &i, int lane) {
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int j = size >> 1; j > 0; j >>= 1)
            cx_lane(k, i, j, ((lane & j) == 0) == ((lane & size) == 0), lane);
    }
}

// Bitonic sort of 128 (key, index) pairs ordered lexicographically (the
// reference's tie order), two per lane: element p lives in lane p & 63,
// register p >> 6.  Ascending in p.
template <typename K>
__device__ __forceinline__ void wave_sort128(K &k0, int &i0, K &k1, int &i1, int lane) {
#pragma unroll
    for (int size = 2; size <= 128; size <<= 1) {
#pragma unroll
        for (int j = size >> 1; j > 0; j >>= 1) {
            if (j == 64) {  // size == 128: partners are the lane's own two registers
                const bool sw = ki_less(k1, i1, k0, i0);
                const K tk = k0;
                const int ti = i0;
                k0 = sw ? k1 : k0;
                i0 = sw ? i1 : i0;
                k1 = sw ? tk : k1;
                i1 = sw ? ti : i1;
            } else {
                // element p = lane (+64): ascending block iff (p & size) == 0
                const bool lower = (lane & j) == 0;
                cx_lane(k0, i0, j, lower == ((lane & size) == 0), lane);
                cx_lane(k1, i1, j, lower == (((lane + 64) & size) == 0), lane);
            }
        }
    }
}

// Selection and output of one query once the candidates C = {key <= thr} (m
// of them, indices in sIdx) are compacted: sort / rank C by (key, index), or
// the radix-select fallback over all cpl x 64 keys when C overflows kCap; then
// the k answers in (key, index) order (the graph variant drops the self point).
// sKey / sIdx / sSel: this wave's LDS lists.
template <bool QUERY>
__device__ __forceinline__ void knn_finish(const float2 *sP, typename KeyTraits<QUERY>::key_t *sKey,
                                           int *sIdx, int *sSel, int m, float2 q, int kk, int k, int qi,
                                           int b, int n_src, int n_q, int cpl, int lane, uint64_t below,
                                           int32_t *__restrict__ out, int32_t *__restrict__ degenerate,
                                           bool count_tie = true) {
    typedef KeyTraits<QUERY> KT;
    typedef typename KT::key_t key_t;
    key_t mk = ~key_t(0);
    int mi = 0x7fffffff;
    int rank = lane;
    // QUERY: an exact fp64 distance tie inside the first kk (order) or between
    // ranks kk - 1 and kk (set): the inputs on which sklearn's order is its
    // KD-tree's traversal, not (distance, index) -- counted in *degenerate
    bool tie = false;
    if (m <= 64) {
        // The common case (a mesh point's list holds ~1.5 kk): one pair per
        // lane, one 64-wide bitonic sort.
        wave_lds_sync();
        key_t k0 = ~key_t(0);
        int i0 = 0x7fffffff;
        if (lane < m) {
            i0 = sIdx[lane];
            k0 = KT::key(sP[i0], q);
        }
        wave_sort64_ki(k0, i0, lane);
        if (lane < kk) mi = i0;
        if (QUERY) {
            const key_t kn = (key_t)__shfl((unsigned long long)k0, (lane + 1) & 63, 64);
            tie = __ballot(lane < kk && lane + 1 < m && k0 == kn) != 0ull;
        }
    } else if (m <= 128) {
        // Two pairs per lane, one 128-wide bitonic sort.
        wave_lds_sync();
        key_t k0 = ~key_t(0), k1 = ~key_t(0);
        int i0 = 0x7fffffff, i1 = 0x7fffffff;
        if (lane < m) {
            i0 = sIdx[lane];
            k0 = KT::key(sP[i0], q);
        }
        if (lane + 64 < m) {
            i1 = sIdx[lane + 64];
            k1 = KT::key(sP[i1], q);
        }
        wave_sort128(k0, i0, k1, i1, lane);
        if (lane < kk) mi = i0;
        if (QUERY) {  // element lane + 1: lane 63's is element 64 (k1 of lane 0)
            const key_t n0 = (key_t)__shfl((unsigned long long)k0, (lane + 1) & 63, 64);
            const key_t n1 = lane_value(k1, 0);
            tie = __ballot(lane < kk && k0 == (lane == 63 ? n1 : n0)) != 0ull;
        }
    } else if (m <= kCap) {
        wave_lds_sync();
        for (int i = lane; i < m; i += 64) sKey[i] = KT::key(sP[sIdx[i]], q);
        wave_lds_sync();
        for (int i = lane; i < m; i += 64) {
            const key_t ki = sKey[i];
            const int ii = sIdx[i];
            int rk = 0, eq_after = 0;
            for (int f = 0; f < m; ++f) {
                const key_t fk = sKey[f];
                const int fi = sIdx[f];
                rk += (fk < ki) || (fk == ki && fi < ii);
                eq_after += fk == ki && fi > ii;
            }
            if (rk < kk) sSel[rk] = ii;
            tie = tie || (QUERY && rk < kk && eq_after > 0);
        }
        tie = __ballot(tie) != 0ull;
        wave_lds_sync();
        if (lane < kk) mi = sSel[lane];
    } else {
        // Fallback for adversarial point sets (hundreds of ties): full
        // radix select on all exact keys, recomputed from LDS per use so
        // that this rare path does not set the kernel's register budget.
        auto key_at = [&](int c) -> key_t {
            const int j = lane + 64 * c;
            return (j < n_src) ? KT::key(sP[j], q) : ~key_t(0);
        };
        key_t T = 0;
        for (int bit = KT::kTopBit; bit >= 0; --bit) {
            const key_t Tc = T | (key_t(1) << bit);
            int cnt = 0;
#pragma unroll 4
            for (int c = 0; c < cpl; ++c) cnt += __popcll(__ballot(key_at(c) < Tc));
            if (cnt <= kk - 1) T = Tc;
        }
        int mlt = 0;
#pragma unroll 4
        for (int c = 0; c < cpl; ++c) mlt += __popcll(__ballot(key_at(c) < T));
        const int need = kk - mlt;  // >= 1 candidates equal to T, taken in index order
        int base = 0, eq_taken = 0;
#pragma unroll 4
        for (int c = 0; c < cpl; ++c) {
            const key_t kc = key_at(c);
            const bool lt = kc < T;
            const bool eq = kc == T;
            const uint64_t em = __ballot(eq);
            const int eqrank = eq_taken + __popcll(em & below);
            const bool sel = lt || (eq && eqrank < need);
            eq_taken += __popcll(em);
            const uint64_t sm = __ballot(sel);
            if (sel) {
                const int pidx = base + __popcll(sm & below);
                sKey[pidx] = kc;
                sIdx[pidx] = lane + 64 * c;
            }
            base += __popcll(sm);
        }
        wave_lds_sync();
        if (lane < kk) {
            mk = sKey[lane];
            mi = sIdx[lane];
        }
        rank = 0;
        int dup = 0;
        for (int f = 0; f < kk; ++f) {
            const key_t fk = sKey[f];
            const int fi = sIdx[f];
            rank += (fk < mk) || (fk == mk && fi < mi);
            dup += fk == mk && fi != mi;
        }
        // ties inside the first kk, or more points at the kk-th key than taken
        tie = __ballot(lane < kk && dup > 0) != 0ull || eq_taken > need;
    }
    wave_lds_sync();  // the next query overwrites sKey / sIdx / sSel
    const int64_t row = ((int64_t)b * n_q + qi) * k;
    if (QUERY) {
        if (lane < kk) out[row + rank] = mi;
        if (tie && count_tie && lane == 0 && degenerate) atomicAdd(degenerate, 1);
    } else {
        const uint64_t smask = __ballot(lane < kk && mi == qi);
        const bool has_self = smask != 0ull;
        const int self_rank = has_self ? lane_value(rank, __ffsll((unsigned long long)smask) - 1) : kk;
        const int pos = rank - ((has_self && rank > self_rank) ? 1 : 0);
        if (lane < kk && !(has_self && mi == qi) && pos < k)
            out[row + pos] = b * n_src + mi;
        if (!has_self && lane == 0 && degenerate) atomicAdd(degenerate, 1);
    }
}

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
constexpr int kTiledMax = 65536;
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

template <bool QUERY>
int launch_knn(const float *pts, const float *qry, int64_t batches, int64_t n_src, int64_t n_q,
               int k, int32_t *out, int32_t *degenerate, hipStream_t st) {
    const int kk = QUERY ? k : k + 1;
    if (k < 1 || kk > 64 || n_src < kk || n_src > kTiledMax || n_q < 1 || batches < 1 ||
        batches > 65535 || n_q > INT32_MAX / 64)
        return MMPDE_ERR_INVALID_ARG;
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
                           degenerate);                                                       \
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
constexpr float kUp = 1.0f + 1.0f / 1048576.0f, kDown = 1.0f - 1.0f / 1048576.0f;

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
    for (int size = 2; size <= 4096; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < 2048; t += 256) {
                const int i = 2 * t - (t & (stride - 1)), l = i + stride;
                const uint64_t a = sk[i], c = sk[l];
                if ((a > c) == ((i & size) == 0)) {
                    sk[i] = c;
                    sk[l] = a;
                }
            }
            __syncthreads();
        }
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

__global__ void edge_index_kernel(const int32_t *__restrict__ nbr, int64_t n, int k,
                                  int64_t *__restrict__ ei) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ne = n * k;
    if (e < ne) {
        ei[e] = nbr[e];
        ei[ne + e] = e / k;
    }
}

// ---------------------------------------------------------------------------
// Cell-binned exact kNN: the cost of a query follows the local point density,
// not the trajectory's size.  mmpde_knn_bin sorts every trajectory's points
// into a uniform grid over their own bounding box (so it does not matter how
// far a mesh has moved); knn_binned_kernel scans the cells around a query ring
// by ring until a distance bound proves that no unscanned point can be a
// candidate, then hands the candidates to knn_finish like knn_tiled_kernel.
//
// Workspace, per trajectory (4-byte words, stride even so that every float2
// stays 8-byte aligned): header [kBinHdr] | sorted points float2 [n_per] |
// their original local indices [n_per] | cell starts [G G + 1] | cell cursors
// [G G] (the counts, then the scatter positions).  Header: x0, y0, hx, hy,
// 1/hx, 1/hy, eps, gx, gy (the grid actually used: G per axis, 1 on an axis
// of zero or non-finite extent), n_per.
// ---------------------------------------------------------------------------
constexpr int kBinHdr = 16;
constexpr int kBinGMax = 128;      // 65536 points at kBinPerCell
constexpr int kBinPerCell = 4;     // points per cell the grid is sized for
constexpr int kBinThreads = 1024;

// cells per axis for a trajectory of n_per points: floor(sqrt(n_per / kBinPerCell))
__host__ __device__ inline int bins_grid(int64_t n_per) {
    int g = 1;
    while (g < kBinGMax && (int64_t)(g + 1) * (g + 1) * kBinPerCell <= n_per) ++g;
    return g;
}

struct BinLayout {
    int G;
    int64_t sp, si, start, cur, stride;  // word offsets in a trajectory's record
};
__host__ __device__ inline BinLayout bins_layout(int64_t n_per) {
    BinLayout l;
    l.G = bins_grid(n_per);
    const int64_t nc = (int64_t)l.G * l.G;
    l.sp = kBinHdr;
    l.si = l.sp + 2 * n_per;
    l.start = l.si + n_per;
    l.cur = l.start + nc + 1;
    l.stride = (l.cur + nc + 1) & ~(int64_t)1;
    return l;
}

// The cell of coordinate v on an axis of g cells from o, inverse cell size ih
// (0 when g == 1); NaN and anything outside the box land in an end cell.
__device__ __forceinline__ int bin_axis(float v, float o, float ih, int g) {
    const float t = (v - o) * ih;
    return (int)fminf(fmaxf(t, 0.0f), (float)(g - 1));
}

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

extern "C" int mmpde_knn_graph(const float *pos, int64_t batches, int64_t n_per, int k,
                               int32_t *nbr_out, int32_t *degenerate, mmpde_stream_t stream) {
    MMPDE_REQUIRE(pos && nbr_out);
    return launch_knn<false>(pos, nullptr, batches, n_per, n_per, k, nbr_out, degenerate,
                             as_stream(stream));
}

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
    for (int size = 2; size <= 4096; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < 2048; t += 256) {
                const int i = 2 * t - (t & (stride - 1)), l = i + stride;
                const float a = sm[i], c = sm[l];
                if ((a > c) == ((i & size) == 0)) {
                    sm[i] = c;
                    sm[l] = a;
                }
            }
            __syncthreads();
        }
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
    dim3 grid(ceil_div(n_per, kQueriesPerBlock), (unsigned)batches);
    const int ns = (int)n_per, cpl = ceil_div(n_per, 64);
#define MMPDE_KNN_FALLBACK(C)                                                                         \
    if (cpl <= C) {                                                                                   \
        hipLaunchKernelGGL((knn_kernel<C, QUERY, kQueriesPerBlock>), grid, dim3(256), 0, st, x, QUERY ? q : x, ns, \
                           ns, k, out, degenerate, (const uint8_t *)miss, (float *)cells, QUERY ? 1 : 0); \
        MMPDE_RET_LAUNCH();                                                                           \
        return MMPDE_OK;                                                                              \
    }
    MMPDE_KNN_FALLBACK(4)
    MMPDE_KNN_FALLBACK(8)
    MMPDE_KNN_FALLBACK(16)
    MMPDE_KNN_FALLBACK(24)
    MMPDE_KNN_FALLBACK(32)
    MMPDE_KNN_FALLBACK(40)
    MMPDE_KNN_FALLBACK(48)
    MMPDE_KNN_FALLBACK(56)
    MMPDE_KNN_FALLBACK(64)
#undef MMPDE_KNN_FALLBACK
    return MMPDE_ERR_UNSUPPORTED;
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
        return launch_knn<false>(pos, nullptr, batches, n_per, n_per, k, nbr_out, degenerate, st);
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
        return launch_knn<true>(src, qry, batches, n_per, n_per, k, idx_out, ties, st);
    return knn_cand_launch<true>(src, qry, xi, ref ? ref : xi, cells, skip_above, batches, n_per, k, cand,
                                 idx_out, ties, scratch, st);
}

extern "C" int mmpde_knn_query(const float *src, const float *qry, int64_t batches,
                               int64_t n_src, int64_t n_qry, int k, int32_t *idx_out, int32_t *ties,
                               mmpde_stream_t stream) {
    MMPDE_REQUIRE(src && qry && idx_out);
    return launch_knn<true>(src, qry, batches, n_src, n_qry, k, idx_out, ties, as_stream(stream));
}

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

extern "C" int mmpde_edge_index_from_nbr(const int32_t *nbr, int64_t n, int k,
                                         int64_t *edge_index, mmpde_stream_t stream) {
    MMPDE_REQUIRE(nbr && edge_index && n > 0 && k > 0);
    const int64_t ne = n * k;
    hipLaunchKernelGGL(edge_index_kernel, dim3(ceil_div(ne, 256)), dim3(256), 0,
                       as_stream(stream), nbr, n, k, edge_index);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}
