// Batched exact k-nearest-neighbour search for gfx950.
//
// Replaces torch_cluster.knn_graph (reference data_creator_2d.py:260,
// mesh/dmm_model.py:228) and sklearn NearestNeighbors.kneighbors
// (data_creator_2d.py:66-78).  One wave per query; the trajectory's point set
// (<= 4096 points, <= 32 KB) is staged once per workgroup in LDS; every lane
// keeps CPL fp32 squared distances in registers (larger sets, up to 16384
// points: knn_large_kernel; up to 65536: knn_tiled_kernel, which streams the
// set through LDS in tiles; knn_binned_kernel scans only the cells of a
// uniform grid around the query).  Selection: U = the kk-th
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
//
// Where what lives:
//   knn_common.hpp  (this file) what more than one file uses: keys, wave
//                   exchanges and sorting networks, knn_finish, the layouts
//                   of the displacement record and of the bins workspace,
//                   launch_knn's declaration
//   knn.hip         every search that selects with knn_finish: the full
//                   search (knn_kernel, knn_large_kernel, knn_tiled_kernel),
//                   launch_knn with its cpl ladder, the binned search
//                   (knn_binned_kernel); the edge index
//   knn_cand.hip    the moved-mesh candidate table, its displacement record
//                   and skip threshold; misses fall back to launch_knn
//   knn_bins.hip    the binning kernels that write the workspace, and the
//                   radius graph (index-order scan and binned)
// The helpers here have internal linkage, so the optimiser specialises them,
// before it inlines them, on what their callers in the same translation unit
// pass (value ranges: lane in [0, 64) and the like).  Which kernels share a
// file therefore shows in their code: knn_binned_kernel, whose lambdas hold
// `lane` by reference, hides that range from knn_finish and the sorting
// networks, and the knn_kernel family compiled without it beside them needs a
// dozen more SGPR spills.  That is why the binned search sits in knn.hip.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace {

constexpr int kQueriesPerBlock = 16;  // 4 per wave
constexpr int kCap = 256;             // LDS list of candidates with key <= U, per wave
constexpr int kTiledMax = 65536;      // the largest trajectory any search takes (knn_tiled_kernel, the bins)

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

// one step of outward / inward rounding: the 2^-20 relative margin of every
// distance bound (the candidate table's, the bins'), which covers the fp32
// rounding of the few operations each bound is built from
constexpr float kUp = 1.0f + 1.0f / 1048576.0f, kDown = 1.0f - 1.0f / 1048576.0f;

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

}  // namespace

namespace mmpde_detail {
// The full search of n_q queries per trajectory over its n_src points, by the
// kernel its size asks for (knn.hip; instantiated there for both QUERY
// values).  miss / cells / role: knn_kernel's miss mode, the candidate path's
// fallback (n_src <= 4096 only).
template <bool QUERY>
__attribute__((visibility("hidden"))) int launch_knn(const float *pts, const float *qry, int64_t batches,
                                                     int64_t n_src, int64_t n_q, int k, int32_t *out,
                                                     int32_t *degenerate, hipStream_t st,
                                                     const uint8_t *miss = nullptr, float *cells = nullptr,
                                                     int role = 0);
}  // namespace mmpde_detail
