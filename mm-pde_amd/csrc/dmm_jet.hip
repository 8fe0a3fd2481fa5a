// The Monge-Ampere jet of the DMM head and its first-order gradients on gfx950:
// what the Adam and LBFGS phases of DMM training (reference mesh/dmm_utils.py
// train_MA_res) need of the head, without autograd through out_nn.
//
//   a = T0 xi + t0_b,  h = tanh a                              (th <= 64)
//   P = W_o0[:, L:] T1 [L', th],  c_b = W_o0[:, :L] branch_b + W_o0[:, L:] t1_b + b_o0
//   v_0 = h, v_d = h' T0[:,d], v_de = h'' T0[:,d] T0[:,e]
//   z = P v_0 + c_b, z_d = P v_d, z_de = P v_de, s = tanh z
//   phi = w_o.s + b_o1, phi_d = w_o.(s' z_d), phi_de = w_o.(s' z_de + s'' z_d z_e)
//
// A tile is 16 consecutive rows of one trajectory (the last of a trajectory
// partial), its six v tables [16, th] in LDS.  The three products run on the
// exact-f32 MFMA (v_mfma_f32_16x16x4_f32) with th padded to a multiple of 16:
//   forward   z_* = P v_*                 one workgroup per tile, k over its waves
//   rows      dv_* = P^T dz_*             one workgroup per tile; z recomputed
//   columns   dP = sum dz_* (x) v_*       workgroup (g, 64 features) walks tiles
//                                         g, g + G, ...; z recomputed
// No [n, L'] table exists anywhere.  Every sum has a fixed order (in-lane over
// registers and tiles, lanes by a fixed butterfly, waves and workgroups in index
// order); there are no atomics.
#include "common.hpp"

namespace {

constexpr int kTileRows = 16;
constexpr int kVStride = 68;     // floats per v row in LDS (64 + 4: b128 reads of 16 rows spread over the banks)
constexpr int kColGroups = 128;  // G of the columns kernel

inline bool al16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
inline bool al4(const void *p) { return ((uintptr_t)p & 3u) == 0; }
inline int64_t r4(int64_t v) { return (v + 3) & ~int64_t(3); }
inline int pad16(int th) { return (th + 15) & ~15; }

struct JetCot {
    const float *g[6];
};
struct JetOut {
    float *o[6];
};

typedef float VTab[kTileRows][kVStride];

struct JetTile {
    int64_t b, row0;
    int nvalid;
};
__device__ __forceinline__ JetTile jet_tile(int64_t tile, int64_t per, int64_t tpb) {
    JetTile t;
    t.b = tile / tpb;
    const int64_t r0 = (tile - t.b * tpb) * kTileRows;
    t.row0 = t.b * per + r0;
    t.nvalid = (int)(per - r0 < kTileRows ? per - r0 : kTileRows);
    return t;
}

// the six v tables of a tile, zero for m >= th; rows past nvalid take xi = 0
__device__ __forceinline__ void jet_fill_v(VTab *V, const float *__restrict__ t0w, const float *__restrict__ t0b,
                                           int th, int thp, const float2 *__restrict__ grid, const JetTile &t) {
    for (int e = threadIdx.x; e < kTileRows * thp; e += 256) {
        const int r = e / thp, m = e - r * thp;
        float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f, v3 = 0.0f, v4 = 0.0f, v5 = 0.0f;
        if (m < th) {
            const float2 x = r < t.nvalid ? grid[t.row0 + r] : make_float2(0.0f, 0.0f);
            const float p = t0w[2 * m], q = t0w[2 * m + 1];
            const float h = tanhf(p * x.x + q * x.y + t0b[m]);
            const float h1 = 1.0f - h * h, h2 = -2.0f * h * h1;
            v0 = h;
            v1 = h1 * p;
            v2 = h1 * q;
            v3 = h2 * p * p;
            v4 = h2 * p * q;
            v5 = h2 * q * q;
        }
        V[0][r][m] = v0;
        V[1][r][m] = v1;
        V[2][r][m] = v2;
        V[3][r][m] = v3;
        V[4][r][m] = v4;
        V[5][r][m] = v5;
    }
}

// z_c of 16 rows x 16 features (k0 ..), c < NC, from LDS v and the padded P
// [L', thp].  With li = lane & 15, g = lane >> 4:
//   KMAJOR:  acc[c][reg] = z_c(row li,          feature k0 + 4 g + reg)
//   else:    acc[c][reg] = z_c(row 4 g + reg,   feature k0 + li)
// Lane group g supplies m = 16 S + 4 g + q at step (S, q): one b128 load of P and
// of each v row per four MFMAs.
template <int NC, bool KMAJOR>
__device__ __forceinline__ void jet_z(const VTab *V, const float *__restrict__ pm, int k0, int thp, int li, int g,
                                      f32x4 (&acc)[6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) acc[c] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float *prow = pm + (int64_t)(k0 + li) * thp + 4 * g;
    for (int S = 0; S < thp; S += 16) {
        const float4 pv = *(const float4 *)(prow + S);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float4 vv = *(const float4 *)&V[c][li][S + 4 * g];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                acc[c] = KMAJOR ? mfma16(f4c(pv, q), f4c(vv, q), acc[c]) : mfma16(f4c(vv, q), f4c(pv, q), acc[c]);
        }
    }
}

// One (row, feature): cotangents of z_* (times w) and the w_o gradient term a0.
// z[0] is the pre-activation (c_b added).
__device__ __forceinline__ void jet_point_bwd(const float (&z)[6], float w, const float (&g)[6], float (&dz)[6],
                                              float &a0) {
    const float s = tanhf(z[0]);
    const float s1 = 1.0f - s * s, s2 = -2.0f * s * s1, s3 = -2.0f * (s1 * s1 + s * s2);
    const float l1 = g[1] * z[1] + g[2] * z[2];
    const float l2 = g[3] * z[3] + g[4] * z[4] + g[5] * z[5];
    const float q2 = g[3] * z[1] * z[1] + g[4] * z[1] * z[2] + g[5] * z[2] * z[2];
    a0 = g[0] * s + s1 * (l1 + l2) + s2 * q2;
    dz[0] = w * (g[0] * s1 + s2 * (l1 + l2) + s3 * q2);
    dz[1] = w * (g[1] * s1 + s2 * (2.0f * g[3] * z[1] + g[4] * z[2]));
    dz[2] = w * (g[2] * s1 + s2 * (g[4] * z[1] + 2.0f * g[5] * z[2]));
    dz[3] = w * g[3] * s1;
    dz[4] = w * g[4] * s1;
    dz[5] = w * g[5] * s1;
}

// sum over the 256 threads of a block in a fixed order; result in every thread
__device__ __forceinline__ float jet_block_sum(float v, float *sh) {
    v = wave_sum_full(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// sum over the four 16-lane groups of a wave (lanes l, l ^ 16, l ^ 32, l ^ 48)
__device__ __forceinline__ float jet_group_sum(float v) {
    v += xor_lane_f<16>(v);
    v += xor_lane_f<32>(v);
    return v;
}

// ---------------------------------------------------------------------------
// P and c_b
// ---------------------------------------------------------------------------
// pm[k][m] = sum_j W_o0[k][L + j] T1[j][m] for m < th, 0 up to thp
__global__ __launch_bounds__(256) void jet_pm_kernel(const float *__restrict__ o0w, const float *__restrict__ t1w,
                                                     int L, int Lp, int th, int thp, float *__restrict__ pm) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Lp * thp) return;
    const int k = e / thp, m = e - k * thp;
    float acc = 0.0f;
    if (m < th) {
        const float *wt = o0w + (int64_t)k * 2 * L + L;
        for (int j = 0; j < L; ++j) acc = __fmaf_rn(wt[j], t1w[(int64_t)j * th + m], acc);
    }
    pm[e] = acc;
}

// cb[b][k] = W_o0[k][:L] . branch_b + W_o0[k][L:] . t1_b + b_o0[k]; one wave per (b, k)
__global__ __launch_bounds__(256) void jet_cb_kernel(const float *__restrict__ o0w, const float *__restrict__ o0b,
                                                     const float *__restrict__ t1b,
                                                     const float *__restrict__ branch, int64_t B, int L, int Lp,
                                                     float *__restrict__ cb) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= B * Lp) return;  // wave-uniform
    const int64_t b = e / Lp;
    const int k = (int)(e - b * Lp);
    const float *wr = o0w + (int64_t)k * 2 * L;
    const float *br = branch + b * L;
    float acc = 0.0f;
    for (int j = lane; j < L; j += 64) acc = __fmaf_rn(wr[j], br[j], acc);
    for (int j = lane; j < L; j += 64) acc = __fmaf_rn(wr[L + j], t1b[j], acc);
    acc = wave_sum_full(acc);
    if (lane == 0) cb[e] = acc + o0b[k];
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <bool SECOND>
__global__ __launch_bounds__(256) void jet_fwd_kernel(const float2 *__restrict__ grid, int64_t per, int64_t tpb,
                                                      const float *__restrict__ pm, const float *__restrict__ cb,
                                                      const float *__restrict__ wo, const float *__restrict__ bo,
                                                      const float *__restrict__ t0w, const float *__restrict__ t0b,
                                                      int th, int thp, int Lp, JetOut out) {
    constexpr int NC = SECOND ? 6 : 3;
    __shared__ __attribute__((aligned(16))) float V[6][kTileRows][kVStride];
    __shared__ float red[4][6][kTileRows];
    const JetTile t = jet_tile(blockIdx.x, per, tpb);
    jet_fill_v(V, t0w, t0b, th, thp, grid, t);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
    const float *cbb = cb + t.b * Lp;
    float ph[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int kt = wv; kt < Lp / 16; kt += 4) {
        f32x4 acc[6];
        jet_z<NC, true>(V, pm, kt * 16, thp, li, g, acc);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int k = kt * 16 + 4 * g + reg;
            const float w = wo[k];
            const float s = tanhf(acc[0][reg] + cbb[k]);
            const float s1 = 1.0f - s * s;
            const float zx = acc[1][reg], zy = acc[2][reg];
            ph[0] = __fmaf_rn(w, s, ph[0]);
            ph[1] = __fmaf_rn(w, s1 * zx, ph[1]);
            ph[2] = __fmaf_rn(w, s1 * zy, ph[2]);
            if (SECOND) {
                const float s2 = -2.0f * s * s1;
                ph[3] = __fmaf_rn(w, __fmaf_rn(s1, acc[3][reg], s2 * zx * zx), ph[3]);
                ph[4] = __fmaf_rn(w, __fmaf_rn(s1, acc[4][reg], s2 * zx * zy), ph[4]);
                ph[5] = __fmaf_rn(w, __fmaf_rn(s1, acc[5][reg], s2 * zy * zy), ph[5]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float v = jet_group_sum(ph[c]);
        if (g == 0) red[wv][c][li] = v;
    }
    __syncthreads();
    if (threadIdx.x < NC * kTileRows) {
        const int c = threadIdx.x / kTileRows, r = threadIdx.x % kTileRows;
        if (r < t.nvalid && out.o[c]) {
            float v = (red[0][c][r] + red[1][c][r]) + (red[2][c][r] + red[3][c][r]);
            if (c == 0 && bo) v += bo[0];
            out.o[c][t.row0 + r] = v;
        }
    }
}

// ---------------------------------------------------------------------------
// backward, rows: dv_* = P^T dz_*, then through v to T0 and t0_b, per tile
// ---------------------------------------------------------------------------
// t0part [tiles][3][64]: sums over the tile's rows of d/dT0[m][0], d/dT0[m][1], d/dt0_b[m]
template <int MT>
__global__ __launch_bounds__(256) void jet_bwd_rows_kernel(const float2 *__restrict__ grid, int64_t per,
                                                           int64_t tpb, const float *__restrict__ pm,
                                                           const float *__restrict__ cb,
                                                           const float *__restrict__ wo,
                                                           const float *__restrict__ t0w,
                                                           const float *__restrict__ t0b, int th, int Lp, JetCot cot,
                                                           float *__restrict__ t0part) {
    constexpr int thp = MT * 16;
    __shared__ __attribute__((aligned(16))) float V[6][kTileRows][kVStride];
    __shared__ float dV[6][kTileRows][64];
    __shared__ float gsh[6][kTileRows];
    const JetTile t = jet_tile(blockIdx.x, per, tpb);
    jet_fill_v(V, t0w, t0b, th, thp, grid, t);
    if (threadIdx.x < 6 * kTileRows) {
        const int c = threadIdx.x / kTileRows, r = threadIdx.x % kTileRows;
        gsh[c][r] = (cot.g[c] && r < t.nvalid) ? cot.g[c][t.row0 + r] : 0.0f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
    const float *cbb = cb + t.b * Lp;
    float gl[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) gl[c] = gsh[c][li];
    f32x4 accv[6][MT];
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) accv[c][mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int kt = wv; kt < Lp / 16; kt += 4) {
        const int k0 = kt * 16;
        f32x4 acc[6];
        jet_z<6, true>(V, pm, k0, thp, li, g, acc);
        float dz[6][4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int k = k0 + 4 * g + reg;
            const float z[6] = {acc[0][reg] + cbb[k], acc[1][reg], acc[2][reg], acc[3][reg], acc[4][reg], acc[5][reg]};
            float d[6], a0;
            jet_point_bwd(z, wo[k], gl, d, a0);
#pragma unroll
            for (int c = 0; c < 6; ++c) dz[c][reg] = d[c];
        }
        // dv_c^T[m][row] += sum_k P[k][m] dz_c(row, k): A = P[k0 + 4 g + reg][16 mt + li], B = this lane's dz
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const float a = pm[(int64_t)(k0 + 4 * g + reg) * thp + mt * 16 + li];
#pragma unroll
                for (int c = 0; c < 6; ++c) accv[c][mt] = mfma16(a, dz[c][reg], accv[c][mt]);
            }
    }
    // the four waves' partial dv, added in wave order; accv[c][mt][reg] is dv_c(row li, m = 16 mt + 4 g + reg)
    for (int ww = 0; ww < 4; ++ww) {
        if (wv == ww) {
#pragma unroll
            for (int c = 0; c < 6; ++c)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        float *p = &dV[c][li][mt * 16 + 4 * g + reg];
                        *p = ww == 0 ? accv[c][mt][reg] : *p + accv[c][mt][reg];
                    }
        }
        __syncthreads();
    }
    if (threadIdx.x < th) {
        const int m = threadIdx.x;
        const float p = t0w[2 * m], q = t0w[2 * m + 1];
        float dp = 0.0f, dq = 0.0f, da = 0.0f;
        for (int r = 0; r < t.nvalid; ++r) {
            const float2 x = grid[t.row0 + r];
            const float h = V[0][r][m];
            const float h1 = 1.0f - h * h, h2 = -2.0f * h * h1, h3 = -2.0f * (h1 * h1 + h * h2);
            const float d0 = dV[0][r][m], d1 = dV[1][r][m], d2 = dV[2][r][m], d3 = dV[3][r][m], d4 = dV[4][r][m],
                        d5 = dV[5][r][m];
            const float a = d0 * h1 + h2 * (d1 * p + d2 * q) + h3 * (d3 * p * p + d4 * p * q + d5 * q * q);
            dp += d1 * h1 + h2 * (2.0f * d3 * p + d4 * q) + a * x.x;
            dq += d2 * h1 + h2 * (d4 * p + 2.0f * d5 * q) + a * x.y;
            da += a;
        }
        float *o = t0part + (int64_t)blockIdx.x * 192 + m;
        o[0] = dp;
        o[64] = dq;
        o[128] = da;
    }
}

// ---------------------------------------------------------------------------
// backward, columns: dP, dw_o and the per-tile sums of dz (for c_b)
// ---------------------------------------------------------------------------
// grid (G, L' / 64): wave w of workgroup (gx, by) owns features by * 64 + w * 16 ..
// and walks tiles gx, gx + G, ...  dppart [G][L'][thp], dwpart [G][L'],
// dcbtile [tiles][L'].
template <int MT>
__global__ __launch_bounds__(256) void jet_bwd_cols_kernel(const float2 *__restrict__ grid, int64_t per,
                                                           int64_t tpb, int64_t tiles,
                                                           const float *__restrict__ pm,
                                                           const float *__restrict__ cb,
                                                           const float *__restrict__ wo,
                                                           const float *__restrict__ t0w,
                                                           const float *__restrict__ t0b, int th, int Lp, JetCot cot,
                                                           float *__restrict__ dppart, float *__restrict__ dwpart,
                                                           float *__restrict__ dcbtile) {
    constexpr int thp = MT * 16;
    __shared__ __attribute__((aligned(16))) float V[6][kTileRows][kVStride];
    __shared__ float gsh[6][kTileRows];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
    const int k0 = blockIdx.y * 64 + wv * 16;
    const float w = wo[k0 + li];
    f32x4 accp[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) accp[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float dwacc = 0.0f;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const JetTile t = jet_tile(tile, per, tpb);
        __syncthreads();  // the previous tile's readers are done
        jet_fill_v(V, t0w, t0b, th, thp, grid, t);
        if (threadIdx.x < 6 * kTileRows) {
            const int c = threadIdx.x / kTileRows, r = threadIdx.x % kTileRows;
            gsh[c][r] = (cot.g[c] && r < t.nvalid) ? cot.g[c][t.row0 + r] : 0.0f;
        }
        __syncthreads();
        f32x4 acc[6];
        jet_z<6, false>(V, pm, k0, thp, li, g, acc);
        const float cbk = cb[t.b * Lp + k0 + li];
        float dz[6][4];
        float dsum = 0.0f;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int r = 4 * g + reg;
            const float z[6] = {acc[0][reg] + cbk, acc[1][reg], acc[2][reg], acc[3][reg], acc[4][reg], acc[5][reg]};
            const float gl[6] = {gsh[0][r], gsh[1][r], gsh[2][r], gsh[3][r], gsh[4][r], gsh[5][r]};
            float d[6], a0;
            jet_point_bwd(z, w, gl, d, a0);
            dwacc += a0;
            dsum += d[0];
#pragma unroll
            for (int c = 0; c < 6; ++c) dz[c][reg] = d[c];
        }
        dsum = jet_group_sum(dsum);
        if (g == 0) dcbtile[tile * Lp + k0 + li] = dsum;
        // dP[k][m] += sum_(c, row) dz_c(row, k) v_c(row, m): A = this lane's dz, B = v_c[4 g + reg][16 mt + li]
#pragma unroll
        for (int c = 0; c < 6; ++c)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    accp[mt] = mfma16(dz[c][reg], V[c][4 * g + reg][mt * 16 + li], accp[mt]);
    }
    dwacc = jet_group_sum(dwacc);
    if (g == 0) dwpart[(int64_t)blockIdx.x * Lp + k0 + li] = dwacc;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
            dppart[((int64_t)blockIdx.x * Lp + k0 + 4 * g + reg) * thp + mt * 16 + li] = accp[mt][reg];
}

// ---------------------------------------------------------------------------
// backward, the small chain rules
// ---------------------------------------------------------------------------
// dst[e] = sum_p src[p][e], p in order
__global__ __launch_bounds__(256) void jet_sum_parts_kernel(const float *__restrict__ src, int parts, int64_t count,
                                                            float *__restrict__ dst) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    float acc = 0.0f;
    for (int p = 0; p < parts; ++p) acc += src[(int64_t)p * count + e];
    dst[e] = acc;
}

// dcb[b][k] = sum over the tiles of trajectory b
__global__ __launch_bounds__(256) void jet_dcb_kernel(const float *__restrict__ dcbtile, int64_t B, int64_t tpb,
                                                      int Lp, float *__restrict__ dcb) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= B * Lp) return;
    const int64_t b = e / Lp;
    const int k = (int)(e - b * Lp);
    float acc = 0.0f;
    for (int64_t c = 0; c < tpb; ++c) acc += dcbtile[(b * tpb + c) * Lp + k];
    dcb[e] = acc;
}

// db_o0[k] = sum_b dcb[b][k]
__global__ __launch_bounds__(256) void jet_dc0_kernel(const float *__restrict__ dcb, int64_t B, int Lp,
                                                      float *__restrict__ db_o0) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= Lp) return;
    float acc = 0.0f;
    for (int64_t b = 0; b < B; ++b) acc += dcb[b * Lp + k];
    db_o0[k] = acc;
}

// dW_o0[k][j]: j < L: sum_b dcb[b][k] branch[b][j]; else sum_m dP[k][m] T1[j - L][m] + db_o0[k] t1_b[j - L]
__global__ __launch_bounds__(256) void jet_dwo0_kernel(const float *__restrict__ dcb, const float *__restrict__ dp,
                                                       const float *__restrict__ dc0,
                                                       const float *__restrict__ branch,
                                                       const float *__restrict__ t1w, const float *__restrict__ t1b,
                                                       int64_t B, int L, int Lp, int th, int thp,
                                                       float *__restrict__ dw) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)Lp * 2 * L) return;
    const int k = (int)(e / (2 * L)), j = (int)(e - (int64_t)k * 2 * L);
    float acc = 0.0f;
    if (j < L) {
        for (int64_t b = 0; b < B; ++b) acc = __fmaf_rn(dcb[b * Lp + k], branch[b * L + j], acc);
    } else {
        const int jj = j - L;
        for (int m = 0; m < th; ++m) acc = __fmaf_rn(dp[(int64_t)k * thp + m], t1w[(int64_t)jj * th + m], acc);
        acc = __fmaf_rn(dc0[k], t1b[jj], acc);
    }
    dw[e] = acc;
}

// dT1[j][m] = sum_k W_o0[k][L + j] dP[k][m]; dt1_b[j] = sum_k W_o0[k][L + j] db_o0[k] (thread m = th)
__global__ __launch_bounds__(256) void jet_dt1_kernel(const float *__restrict__ o0w, const float *__restrict__ dp,
                                                      const float *__restrict__ dc0, int L, int Lp, int th, int thp,
                                                      float *__restrict__ dt1, float *__restrict__ dt1b) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= L * (th + 1)) return;
    const int j = e / (th + 1), m = e - j * (th + 1);
    const float *wt = o0w + L + j;
    float acc = 0.0f;
    if (m < th) {
        for (int k = 0; k < Lp; ++k) acc = __fmaf_rn(wt[(int64_t)k * 2 * L], dp[(int64_t)k * thp + m], acc);
        dt1[(int64_t)j * th + m] = acc;
    } else {
        for (int k = 0; k < Lp; ++k) acc = __fmaf_rn(wt[(int64_t)k * 2 * L], dc0[k], acc);
        dt1b[j] = acc;
    }
}

// d_branch[b][j] = sum_k dcb[b][k] W_o0[k][j]
__global__ __launch_bounds__(256) void jet_dbranch_kernel(const float *__restrict__ dcb,
                                                          const float *__restrict__ o0w, int64_t B, int L, int Lp,
                                                          float *__restrict__ db) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= B * L) return;
    const int64_t b = e / L;
    const int j = (int)(e - b * L);
    float acc = 0.0f;
    for (int k = 0; k < Lp; ++k) acc = __fmaf_rn(dcb[b * Lp + k], o0w[(int64_t)k * 2 * L + j], acc);
    db[e] = acc;
}

// block m < th: dT0[m][0], dT0[m][1], dt0_b[m] over the tiles; block th: db_o1 = sum of phi's cotangent
__global__ __launch_bounds__(256) void jet_dt0_kernel(const float *__restrict__ t0part, int64_t tiles, int th,
                                                      const float *__restrict__ g0, int64_t n,
                                                      float *__restrict__ dt0, float *__restrict__ dt0b,
                                                      float *__restrict__ dbo1) {
    __shared__ float sh[4];
    if ((int)blockIdx.x == th) {
        float a = 0.0f;
        if (g0)
            for (int64_t i = threadIdx.x; i < n; i += 256) a += g0[i];
        a = jet_block_sum(a, sh);
        if (threadIdx.x == 0) dbo1[0] = a;
        return;
    }
    const int m = blockIdx.x;
    float a = 0.0f, b = 0.0f, c = 0.0f;
    for (int64_t t = threadIdx.x; t < tiles; t += 256) {
        const float *p = t0part + t * 192 + m;
        a += p[0];
        b += p[64];
        c += p[128];
    }
    a = jet_block_sum(a, sh);
    b = jet_block_sum(b, sh);
    c = jet_block_sum(c, sh);
    if (threadIdx.x == 0) {
        dt0[2 * m] = a;
        dt0[2 * m + 1] = b;
        dt0b[m] = c;
    }
}

// workspace, in floats: P [L', thp], c_b [B, L'] (both calls), then the
// backward's partial sums
struct JetWs {
    float *pm, *cb, *dppart, *dwpart, *dcbtile, *t0part, *dp, *dcb;
    int64_t floats;
};
JetWs jet_carve(float *ws, int64_t B, int64_t tiles, int Lp, int thp) {
    JetWs w;
    float *p = ws;
    auto take = [&](int64_t nf) {
        float *q = p;
        p += r4(nf);
        return q;
    };
    const int64_t G = tiles < kColGroups ? tiles : kColGroups;
    w.pm = take((int64_t)Lp * thp);
    w.cb = take(B * Lp);
    w.dppart = take(G * Lp * thp);
    w.dwpart = take(G * Lp);
    w.dcbtile = take(tiles * Lp);
    w.t0part = take(tiles * 192);
    w.dp = take((int64_t)Lp * thp);
    w.dcb = take(B * Lp);
    w.floats = (p - ws) + 64;
    return w;
}

inline int64_t jet_tiles_per(int64_t per) { return (per + kTileRows - 1) / kTileRows; }

int jet_prepare(const float *branch, int64_t B, const mmpde_dmm_head *hd, const JetWs &w, int thp, hipStream_t st) {
    const int L = hd->latent, Lp = hd->hidden, th = hd->th;
    hipLaunchKernelGGL(jet_pm_kernel, dim3((unsigned)ceil_div((int64_t)Lp * thp, 256)), dim3(256), 0, st, hd->o0_w,
                       hd->t1_w, L, Lp, th, thp, w.pm);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(jet_cb_kernel, dim3((unsigned)ceil_div(B * Lp, 4)), dim3(256), 0, st, hd->o0_w, hd->o0_b,
                       hd->t1_b, branch, B, L, Lp, w.cb);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

bool jet_args_ok(const float *branch, int64_t B, const float *grid, int64_t n, const mmpde_dmm_head *hd,
                 const void *workspace) {
    return branch && grid && hd && workspace && B > 0 && n > 0 && n % B == 0 && al16(workspace) &&
           ((uintptr_t)grid & 7u) == 0 && al4(branch);
}

}  // namespace

extern "C" int64_t mmpde_dmm_jet_workspace_bytes(int64_t batches, int64_t n_grid, int latent, int hidden, int th) {
    if (batches <= 0 || n_grid <= 0 || latent <= 0 || hidden <= 0 || th <= 0 || th > 64 || n_grid % batches != 0)
        return 0;
    const int64_t tiles = batches * jet_tiles_per(n_grid / batches);
    return jet_carve(nullptr, batches, tiles, hidden, pad16(th)).floats * (int64_t)sizeof(float);
}

extern "C" int mmpde_dmm_jet(const float *branch, int64_t batches, const float *grid, int64_t n_grid,
                             const mmpde_dmm_head *hd, const float *o1_b, void *workspace,
                             const mmpde_dmm_jet_out *out, mmpde_stream_t stream) {
    MMPDE_REQUIRE(jet_args_ok(branch, batches, grid, n_grid, hd, workspace) && out && al4(o1_b));
    MMPDE_REQUIRE(al4(out->phi) && al4(out->phi_x) && al4(out->phi_y) && al4(out->phi_xx) && al4(out->phi_xy) &&
                  al4(out->phi_yy));
    if (!mmpde_detail::dmm_head_ok(hd)) return MMPDE_ERR_UNSUPPORTED;
    const int64_t per = n_grid / batches, tpb = jet_tiles_per(per), tiles = batches * tpb;
    MMPDE_REQUIRE(tiles <= INT32_MAX);
    hipStream_t st = as_stream(stream);
    const int thp = pad16(hd->th);
    const JetWs w = jet_carve((float *)workspace, batches, tiles, hd->hidden, thp);
    const int rc = jet_prepare(branch, batches, hd, w, thp, st);
    if (rc) return rc;
    const JetOut o{{out->phi, out->phi_x, out->phi_y, out->phi_xx, out->phi_xy, out->phi_yy}};
    const bool second = out->phi_xx || out->phi_xy || out->phi_yy;
    if (second)
        hipLaunchKernelGGL(jet_fwd_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, st, (const float2 *)grid, per,
                           tpb, w.pm, w.cb, hd->o1_w, o1_b, hd->t0_w, hd->t0_b, hd->th, thp, hd->hidden, o);
    else
        hipLaunchKernelGGL(jet_fwd_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, st, (const float2 *)grid, per,
                           tpb, w.pm, w.cb, hd->o1_w, o1_b, hd->t0_w, hd->t0_b, hd->th, thp, hd->hidden, o);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

namespace {
template <int MT>
int jet_grad_launch(const float *grid, int64_t per, int64_t tpb, int64_t tiles, const mmpde_dmm_head *hd,
                    const JetWs &w, const JetCot &cot, hipStream_t st) {
    const int Lp = hd->hidden;
    hipLaunchKernelGGL(jet_bwd_rows_kernel<MT>, dim3((unsigned)tiles), dim3(256), 0, st, (const float2 *)grid, per,
                       tpb, w.pm, w.cb, hd->o1_w, hd->t0_w, hd->t0_b, hd->th, Lp, cot, w.t0part);
    MMPDE_RET_LAUNCH();
    const unsigned G = (unsigned)(tiles < kColGroups ? tiles : kColGroups);
    hipLaunchKernelGGL(jet_bwd_cols_kernel<MT>, dim3(G, (unsigned)(Lp / 64)), dim3(256), 0, st, (const float2 *)grid,
                       per, tpb, tiles, w.pm, w.cb, hd->o1_w, hd->t0_w, hd->t0_b, hd->th, Lp, cot, w.dppart, w.dwpart,
                       w.dcbtile);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}
}  // namespace

extern "C" int mmpde_dmm_jet_grad(const float *branch, int64_t batches, const float *grid, int64_t n_grid,
                                  const mmpde_dmm_head *hd, const float *o1_b, void *workspace,
                                  const mmpde_dmm_jet_cot *cot, const mmpde_dmm_jet_grads *gr,
                                  mmpde_stream_t stream) {
    (void)o1_b;  // phi's gradient does not depend on its bias
    MMPDE_REQUIRE(jet_args_ok(branch, batches, grid, n_grid, hd, workspace) && cot && gr);
    MMPDE_REQUIRE(al4(cot->phi) && al4(cot->phi_x) && al4(cot->phi_y) && al4(cot->phi_xx) && al4(cot->phi_xy) &&
                  al4(cot->phi_yy));
    MMPDE_REQUIRE(gr->d_branch && gr->d_t0_w && gr->d_t0_b && gr->d_t1_w && gr->d_t1_b && gr->d_o0_w && gr->d_o0_b &&
                  gr->d_o1_w && gr->d_o1_b);
    MMPDE_REQUIRE(al4(gr->d_branch) && al4(gr->d_t0_w) && al4(gr->d_t0_b) && al4(gr->d_t1_w) && al4(gr->d_t1_b) &&
                  al4(gr->d_o0_w) && al4(gr->d_o0_b) && al4(gr->d_o1_w) && al4(gr->d_o1_b));
    if (!mmpde_detail::dmm_head_ok(hd)) return MMPDE_ERR_UNSUPPORTED;
    const int64_t per = n_grid / batches, tpb = jet_tiles_per(per), tiles = batches * tpb;
    MMPDE_REQUIRE(tiles <= INT32_MAX);
    hipStream_t st = as_stream(stream);
    const int L = hd->latent, Lp = hd->hidden, th = hd->th, thp = pad16(th);
    const JetWs w = jet_carve((float *)workspace, batches, tiles, Lp, thp);
    int rc = jet_prepare(branch, batches, hd, w, thp, st);
    if (rc) return rc;
    const JetCot c{{cot->phi, cot->phi_x, cot->phi_y, cot->phi_xx, cot->phi_xy, cot->phi_yy}};
    switch (thp / 16) {
        case 1: rc = jet_grad_launch<1>(grid, per, tpb, tiles, hd, w, c, st); break;
        case 2: rc = jet_grad_launch<2>(grid, per, tpb, tiles, hd, w, c, st); break;
        case 3: rc = jet_grad_launch<3>(grid, per, tpb, tiles, hd, w, c, st); break;
        default: rc = jet_grad_launch<4>(grid, per, tpb, tiles, hd, w, c, st); break;
    }
    if (rc) return rc;
    const int G = (int)(tiles < kColGroups ? tiles : kColGroups);
    hipLaunchKernelGGL(jet_sum_parts_kernel, dim3((unsigned)ceil_div((int64_t)Lp * thp, 256)), dim3(256), 0, st,
                       w.dppart, G, (int64_t)Lp * thp, w.dp);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(jet_sum_parts_kernel, dim3((unsigned)ceil_div(Lp, 256)), dim3(256), 0, st, w.dwpart, G,
                       (int64_t)Lp, gr->d_o1_w);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(jet_dcb_kernel, dim3((unsigned)ceil_div(batches * Lp, 256)), dim3(256), 0, st, w.dcbtile,
                       batches, tpb, Lp, w.dcb);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(jet_dc0_kernel, dim3((unsigned)ceil_div(Lp, 256)), dim3(256), 0, st, w.dcb, batches, Lp,
                       gr->d_o0_b);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(jet_dwo0_kernel, dim3((unsigned)ceil_div((int64_t)Lp * 2 * L, 256)), dim3(256), 0, st, w.dcb,
                       w.dp, gr->d_o0_b, branch, hd->t1_w, hd->t1_b, batches, L, Lp, th, thp, gr->d_o0_w);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(jet_dt1_kernel, dim3((unsigned)ceil_div((int64_t)L * (th + 1), 256)), dim3(256), 0, st,
                       hd->o0_w, w.dp, gr->d_o0_b, L, Lp, th, thp, gr->d_t1_w, gr->d_t1_b);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(jet_dbranch_kernel, dim3((unsigned)ceil_div(batches * L, 256)), dim3(256), 0, st, w.dcb,
                       hd->o0_w, batches, L, Lp, gr->d_branch);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(jet_dt0_kernel, dim3((unsigned)(th + 1)), dim3(256), 0, st, w.t0part, tiles, th, cot->phi,
                       n_grid, gr->d_t0_w, gr->d_t0_b, gr->d_o1_b);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}
