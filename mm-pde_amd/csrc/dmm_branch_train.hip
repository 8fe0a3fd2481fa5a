// DMM graph branch in train() mode on gfx950 (reference mesh/dmm_model.py:94-142,
// 197-210 under model.train()): the tanh GNN layer and the decoding DenseNet
// [4, 128, 1], forward and backward.  The BatchNorms on batch statistics, the
// embedding and output_mlp run on the row kernels (train_rows.hip, rgemm.hip).
//
// GNN layer (hidden 4), target i with sources j = nbr[i, 0..k):
//     in_ij = cat(h_i, h_j, u_i - u_j, g_i - g_j)            [11]
//     m1 = tanh(W1 in + B1),  m2 = tanh(W2 m1 + B2),  m_i = mean_j m2
//     up1 = tanh(V1 cat(h_i, m_i) + C1),  upd_i = tanh(V2 up1 + C2)
// The forward writes upd; the residual and the BatchNorm are the caller's.
// Backward from d_upd, nothing kept from the forward (every pass recomputes what
// it needs from h):
//   update pass   per target: m_i again, then dz2 = d_upd (1 - upd^2), dz1 =
//                 (V2^T dz2)(1 - up1^2), d_cat = V1^T dz1 -> d_h (direct part),
//                 d_m / k, and the 56 sums of update_net_1/2;
//   message pass  per edge: m1, m2 again, d2 = d_m / k (1 - m2^2), d1 =
//                 (W2^T d2)(1 - m1^2) -> the 68 sums of message_net_1/2, the
//                 target side d_h_i += W1[:, 0:4]^T sum_j d1, and d1 itself to
//                 the one per-edge workspace [B N k, 4];
//   source pass   per node j: d_h_j += W1[:, 4:8]^T (sum of d1 over the edges
//                 that read j as source, in reverse-adjacency order).
// Four lanes per target as in dmm.hip's eval kernels, the trajectory's h, u and
// the grid staged in LDS (28 B per node) up to 120 KiB, global reads above.
// Weight gradients: per-lane sums, a fixed lane butterfly (DPP), the waves added
// in index order in LDS, one partial row per workgroup, and a finishing kernel
// that adds the rows in a fixed order.  No atomics: the same bits on every run,
// and a trajectory's rows do not depend on the batch it sits in.
//
// Decoder d = W1 tanh(W0 h + b0) + b1: forward and d_h with four lanes per node
// (32 hidden units each); the weight sums with one lane per hidden unit over a
// chunk of nodes read from LDS (broadcast reads, no cross-lane reduction), one
// partial row per workgroup.  No [n, 128] table in either direction.
#include "common.hpp"

namespace {

constexpr int kTargets = 128;      // targets per workgroup: 512 threads, four lanes each
constexpr int kLayerGrads = MMPDE_DMM_GNN_TRAIN_GRADS;
constexpr int kMsgGrads = 68;      // W1 44, B1 4, W2 16, B2 4
constexpr int kUpdGrads = 56;      // V1 32, C1 4, V2 16, C2 4
constexpr int kDecGrads = MMPDE_DMM_DECODE_TRAIN_GRADS;
constexpr int kDecLd = 772;        // partial row stride of the decoder
constexpr int kDecChunk = 1024;    // nodes per workgroup of the decoder's weight pass
constexpr int kSrcNodes = 64;      // nodes per workgroup of the source pass

// offsets into the layer's 124 floats (weights in LDS, gradients in the same order)
constexpr int oW1 = 0, oB1 = 44, oW2 = 48, oB2 = 64, oV1 = 68, oC1 = 100, oV2 = 104, oC2 = 120;

__device__ __forceinline__ void load_layer(float *w, const mmpde_dmm_gnn_weights &p) {
    const int t = threadIdx.x;
    if (t < 44) w[oW1 + t] = p.msg1_w[t];
    if (t < 32) w[oV1 + t] = p.upd1_w[t];
    if (t < 16) {
        w[oW2 + t] = p.msg2_w[t];
        w[oV2 + t] = p.upd2_w[t];
    }
    if (t < 4) {
        w[oB1 + t] = p.msg1_b[t];
        w[oB2 + t] = p.msg2_b[t];
        w[oC1 + t] = p.upd1_b[t];
        w[oC2 + t] = p.upd2_b[t];
    }
}

// the trajectory's nodes: LDS copies (LDS) or the global arrays at the trajectory's base
template <bool LDS>
struct Traj {
    const float4 *h;
    const float *u;
    const float2 *g;
};

template <bool LDS>
__device__ __forceinline__ Traj<LDS> stage(float4 *dyn, const float4 *__restrict__ h, const float *__restrict__ u,
                                           const float2 *__restrict__ grid, int64_t base, int n_per) {
    if constexpr (LDS) {
        float4 *sh = dyn;
        float2 *sg = (float2 *)(sh + n_per);
        float *su = (float *)(sg + n_per);
        for (int t = threadIdx.x; t < n_per; t += 512) {
            sh[t] = h[base + t];
            sg[t] = grid[t];
            su[t] = u[base + t];
        }
        return {sh, su, sg};
    } else {
        return {h + base, u + base, grid};
    }
}

// the message nets on one edge: m1 = tanh(W1 in + B1), m2 = tanh(W2 m1 + B2)
__device__ __forceinline__ void edge_fwd(const float *w, const float (&in)[11], float (&m1)[4], float (&m2)[4]) {
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        float v = w[oB1 + o];
#pragma unroll
        for (int t = 0; t < 11; ++t) v += w[oW1 + o * 11 + t] * in[t];
        m1[o] = tanhf(v);
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        float v = w[oB2 + o];
#pragma unroll
        for (int t = 0; t < 4; ++t) v += w[oW2 + o * 4 + t] * m1[t];
        m2[o] = tanhf(v);
    }
}

__device__ __forceinline__ void edge_input(const float (&hi)[4], float ui, float2 gi, float4 hj, float uj, float2 gj,
                                           float (&in)[11]) {
    in[0] = hi[0], in[1] = hi[1], in[2] = hi[2], in[3] = hi[3];
    in[4] = hj.x, in[5] = hj.y, in[6] = hj.z, in[7] = hj.w;
    in[8] = ui - uj, in[9] = gi.x - gj.x, in[10] = gi.y - gj.y;
}

__device__ __forceinline__ int nbr_at(const int32_t *nr, int e, int k, int n_per) {
    return (int)min((uint32_t)nr[min(e, k - 1)], (uint32_t)(n_per - 1));
}

// cat(h_i, mean_j m2) of target p (every lane of the quad returns it): lane `sub` takes edges sub, sub + 4,
// ..., the quad's sums meet by two xor exchanges.  The next neighbour index is loaded a trip ahead.
template <bool LDS>
__device__ __forceinline__ void node_cat(const Traj<LDS> &tr, const float *w, const int32_t *nr, int k, int n_per,
                                         int sub, const float (&hi)[4], float ui, float2 gi, float (&cat)[8]) {
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
    int jn = nbr_at(nr, sub, k, n_per);
    for (int e = sub; e < k; e += 4) {
        const int j = jn;
        jn = nbr_at(nr, e + 4, k, n_per);
        float in[11], m1[4], m2[4];
        edge_input(hi, ui, gi, tr.h[j], tr.u[j], tr.g[j], in);
        edge_fwd(w, in, m1, m2);
#pragma unroll
        for (int o = 0; o < 4; ++o) sum[o] += m2[o];
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        sum[o] += xor_lane_f<1>(sum[o]);
        sum[o] += xor_lane_f<2>(sum[o]);
        cat[o] = hi[o];
        cat[4 + o] = sum[o] / (float)k;
    }
}

// up1 = tanh(V1 cat + C1), upd = tanh(V2 up1 + C2)
__device__ __forceinline__ void node_update(const float *w, const float (&cat)[8], float (&up1)[4], float (&upd)[4]) {
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        float v = w[oC1 + o];
#pragma unroll
        for (int t = 0; t < 8; ++t) v += w[oV1 + o * 8 + t] * cat[t];
        up1[o] = tanhf(v);
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        float v = w[oC2 + o];
#pragma unroll
        for (int t = 0; t < 4; ++t) v += w[oV2 + o * 4 + t] * up1[t];
        upd[o] = tanhf(v);
    }
}

// Workgroup (x, b): targets [128 x, 128 x + 128) of trajectory b.  A quad past the trajectory's end repeats
// its last node (every lane stays active for the DPP exchanges) and stores nothing.
template <bool LDS>
__global__ __launch_bounds__(512) void gnn_train_fwd_kernel(const float4 *__restrict__ h,
                                                            const float *__restrict__ u,
                                                            const float2 *__restrict__ grid,
                                                            const int32_t *__restrict__ nbr, int k, int n_per,
                                                            mmpde_dmm_gnn_weights wp, float4 *__restrict__ upd_out) {
    extern __shared__ float4 dyn[];
    __shared__ float w[kLayerGrads];
    load_layer(w, wp);
    const int64_t base = (int64_t)blockIdx.y * n_per;
    const Traj<LDS> tr = stage<LDS>(dyn, h, u, grid, base, n_per);
    __syncthreads();
    const int p0 = blockIdx.x * kTargets + (threadIdx.x >> 2);
    const bool live = p0 < n_per;
    const int p = live ? p0 : n_per - 1;
    const int sub = threadIdx.x & 3;
    const float4 hi4 = tr.h[p];
    const float hi[4] = {hi4.x, hi4.y, hi4.z, hi4.w};
    float cat[8], up1[4], upd[4];
    node_cat<LDS>(tr, w, nbr + (int64_t)p * k, k, n_per, sub, hi, tr.u[p], tr.g[p], cat);
    node_update(w, cat, up1, upd);
    if (live && sub == 0) upd_out[base + p] = make_float4(upd[0], upd[1], upd[2], upd[3]);
}

// v of lanes l, l ^ 4, l ^ 8, ..., l ^ 60 added by a fixed butterfly
__device__ __forceinline__ float quads_sum(float v) {
    v += xor_lane_f<32>(v);
    v += xor_lane_f<16>(v);
    v += xor_lane_f<8>(v);
    v += xor_lane_f<4>(v);
    return v;
}

// The update pass.  Lane `sub` of a quad owns row `sub` of the four update-net gradients (14 sums).
template <bool LDS>
__global__ __launch_bounds__(512) void gnn_train_upd_kernel(const float4 *__restrict__ h,
                                                            const float *__restrict__ u,
                                                            const float2 *__restrict__ grid,
                                                            const int32_t *__restrict__ nbr, int k, int n_per,
                                                            mmpde_dmm_gnn_weights wp,
                                                            const float4 *__restrict__ d_upd,
                                                            float4 *__restrict__ d_h, float4 *__restrict__ d_m,
                                                            float *__restrict__ partial) {
    extern __shared__ float4 dyn[];
    __shared__ float w[kLayerGrads];
    __shared__ float red[8][kUpdGrads];
    load_layer(w, wp);
    const int64_t base = (int64_t)blockIdx.y * n_per;
    const Traj<LDS> tr = stage<LDS>(dyn, h, u, grid, base, n_per);
    __syncthreads();
    const int p0 = blockIdx.x * kTargets + (threadIdx.x >> 2);
    const bool live = p0 < n_per;
    const int p = live ? p0 : n_per - 1;
    const int sub = threadIdx.x & 3;
    const float4 hi4 = tr.h[p];
    const float hi[4] = {hi4.x, hi4.y, hi4.z, hi4.w};
    float cat[8], up1[4], upd[4];
    node_cat<LDS>(tr, w, nbr + (int64_t)p * k, k, n_per, sub, hi, tr.u[p], tr.g[p], cat);
    node_update(w, cat, up1, upd);
    const float4 du4 = d_upd[base + p];
    const float du[4] = {live ? du4.x : 0.f, live ? du4.y : 0.f, live ? du4.z : 0.f, live ? du4.w : 0.f};
    float dz2[4], dz1[4], dcat[8];
#pragma unroll
    for (int o = 0; o < 4; ++o) dz2[o] = du[o] * (1.0f - upd[o] * upd[o]);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float v = 0.0f;
#pragma unroll
        for (int o = 0; o < 4; ++o) v += w[oV2 + o * 4 + t] * dz2[o];
        dz1[t] = v * (1.0f - up1[t] * up1[t]);
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        float v = 0.0f;
#pragma unroll
        for (int o = 0; o < 4; ++o) v += w[oV1 + o * 8 + t] * dz1[o];
        dcat[t] = v;
    }
    if (live && sub == 0) {
        const float kf = (float)k;
        d_h[base + p] = make_float4(dcat[0], dcat[1], dcat[2], dcat[3]);
        d_m[base + p] = make_float4(dcat[4] / kf, dcat[5] / kf, dcat[6] / kf, dcat[7] / kf);
    }
    // row `sub`: dV1[sub, 0:8], dC1[sub], dV2[sub, 0:4], dC2[sub]
    const float z1 = sub == 0 ? dz1[0] : sub == 1 ? dz1[1] : sub == 2 ? dz1[2] : dz1[3];
    const float z2 = sub == 0 ? dz2[0] : sub == 1 ? dz2[1] : sub == 2 ? dz2[2] : dz2[3];
    float a[14];
#pragma unroll
    for (int t = 0; t < 8; ++t) a[t] = z1 * cat[t];
    a[8] = z1;
#pragma unroll
    for (int t = 0; t < 4; ++t) a[9 + t] = z2 * up1[t];
    a[13] = z2;
#pragma unroll
    for (int t = 0; t < 14; ++t) a[t] = quads_sum(a[t]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < 4) {
        float *r = red[wave] - oV1;  // the update nets' part of the row starts at oV1
#pragma unroll
        for (int t = 0; t < 8; ++t) r[oV1 + lane * 8 + t] = a[t];
        r[oC1 + lane] = a[8];
#pragma unroll
        for (int t = 0; t < 4; ++t) r[oV2 + lane * 4 + t] = a[9 + t];
        r[oC2 + lane] = a[13];
    }
    __syncthreads();
    if (threadIdx.x < kUpdGrads) {
        float s = red[0][threadIdx.x];
#pragma unroll
        for (int v = 1; v < 8; ++v) s += red[v][threadIdx.x];
        const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        partial[wg * kLayerGrads + oV1 + threadIdx.x] = s;
    }
}

// The message pass.  Every lane keeps the 68 message-net sums of its own edges.
template <bool LDS>
__global__ __launch_bounds__(512) void gnn_train_msg_kernel(const float4 *__restrict__ h,
                                                            const float *__restrict__ u,
                                                            const float2 *__restrict__ grid,
                                                            const int32_t *__restrict__ nbr, int k, int n_per,
                                                            mmpde_dmm_gnn_weights wp,
                                                            const float4 *__restrict__ d_m,
                                                            float4 *__restrict__ d_h, float4 *__restrict__ edge,
                                                            float *__restrict__ partial) {
    extern __shared__ float4 dyn[];
    __shared__ float w[kLayerGrads];
    __shared__ float red[8][kMsgGrads];
    load_layer(w, wp);
    const int64_t base = (int64_t)blockIdx.y * n_per;
    const Traj<LDS> tr = stage<LDS>(dyn, h, u, grid, base, n_per);
    __syncthreads();
    const int p0 = blockIdx.x * kTargets + (threadIdx.x >> 2);
    const bool live = p0 < n_per;
    const int p = live ? p0 : n_per - 1;
    const int sub = threadIdx.x & 3;
    const float4 hi4 = tr.h[p];
    const float hi[4] = {hi4.x, hi4.y, hi4.z, hi4.w};
    const float ui = tr.u[p];
    const float2 gi = tr.g[p];
    const float4 dm4 = d_m[base + p];
    const float dm[4] = {live ? dm4.x : 0.f, live ? dm4.y : 0.f, live ? dm4.z : 0.f, live ? dm4.w : 0.f};
    float acc[kMsgGrads];
#pragma unroll
    for (int t = 0; t < kMsgGrads; ++t) acc[t] = 0.0f;
    float ts[4] = {0.f, 0.f, 0.f, 0.f};
    const int32_t *nr = nbr + (int64_t)p * k;
    float4 *er = edge + (base + p) * k;
    int jn = nbr_at(nr, sub, k, n_per);
    for (int e = sub; e < k; e += 4) {
        const int j = jn;
        jn = nbr_at(nr, e + 4, k, n_per);
        float in[11], m1[4], m2[4], d2[4], d1[4];
        edge_input(hi, ui, gi, tr.h[j], tr.u[j], tr.g[j], in);
        edge_fwd(w, in, m1, m2);
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            d2[o] = dm[o] * (1.0f - m2[o] * m2[o]);
            acc[oB2 + o] += d2[o];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[oW2 + o * 4 + t] += d2[o] * m1[t];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float v = 0.0f;
#pragma unroll
            for (int o = 0; o < 4; ++o) v += w[oW2 + o * 4 + t] * d2[o];
            d1[t] = v * (1.0f - m1[t] * m1[t]);
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            ts[o] += d1[o];
#pragma unroll
            for (int t = 4; t < 11; ++t) acc[oW1 + o * 11 + t] += d1[o] * in[t];
        }
        if (live) er[e] = make_float4(d1[0], d1[1], d1[2], d1[3]);
    }
    // h_i is the same on every edge of the target: dW1[:, 0:4] = (sum_j d1) (x) h_i, dB1 = sum_j d1
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        acc[oB1 + o] = ts[o];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[oW1 + o * 11 + t] = ts[o] * hi[t];
    }
    // the target side: d_h_i += W1[:, 0:4]^T sum_j d1
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        ts[o] += xor_lane_f<1>(ts[o]);
        ts[o] += xor_lane_f<2>(ts[o]);
    }
    if (live && sub == 0) {
        float4 d = d_h[base + p];
        float dt[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float v = 0.0f;
#pragma unroll
            for (int o = 0; o < 4; ++o) v += w[oW1 + o * 11 + t] * ts[o];
            dt[t] = v;
        }
        d_h[base + p] = make_float4(d.x + dt[0], d.y + dt[1], d.z + dt[2], d.w + dt[3]);
    }
#pragma unroll
    for (int t = 0; t < kMsgGrads; ++t) acc[t] = wave_sum_full(acc[t]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < kMsgGrads; ++t) red[wave][t] = acc[t];
    }
    __syncthreads();
    if (threadIdx.x < kMsgGrads) {
        float s = red[0][threadIdx.x];
#pragma unroll
        for (int v = 1; v < 8; ++v) s += red[v][threadIdx.x];
        const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        partial[wg * kLayerGrads + threadIdx.x] = s;
    }
}

// The source pass: four lanes per node, lane `sub` adds entries sub, sub + 4, ... of the node's reverse list.
__global__ __launch_bounds__(256) void gnn_train_src_kernel(const float4 *__restrict__ edge,
                                                            const int64_t *__restrict__ rev_off,
                                                            const int64_t *__restrict__ rev_edge, int k, int n_per,
                                                            const float *__restrict__ w1,
                                                            float4 *__restrict__ d_h) {
    __shared__ float ws[16];  // W1[o, 4 + t]
    if (threadIdx.x < 16) ws[threadIdx.x] = w1[(threadIdx.x >> 2) * 11 + 4 + (threadIdx.x & 3)];
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.y * n_per;
    const int p0 = blockIdx.x * kSrcNodes + (threadIdx.x >> 2);
    const bool live = p0 < n_per;
    const int sub = threadIdx.x & 3;
    const float4 *eb = edge + base * k;
    const int64_t slots = (int64_t)n_per * k;  // the capacity of rev_edge
    const int64_t q0 = live ? max(rev_off[p0], (int64_t)0) : 0, q1 = live ? min(rev_off[p0 + 1], slots) : 0;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t q = q0 + sub; q < q1; q += 4) {
        const int64_t slot = rev_edge[q];
        if (slot < 0 || slot >= slots) continue;  // a foreign list never reads outside the workspace
        const float4 d = eb[slot];
        s[0] += d.x, s[1] += d.y, s[2] += d.z, s[3] += d.w;
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        s[o] += xor_lane_f<1>(s[o]);
        s[o] += xor_lane_f<2>(s[o]);
    }
    if (live && sub == 0) {
        float4 d = d_h[base + p0];
        float dt[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float v = 0.0f;
#pragma unroll
            for (int o = 0; o < 4; ++o) v += ws[o * 4 + t] * s[o];
            dt[t] = v;
        }
        d_h[base + p0] = make_float4(d.x + dt[0], d.y + dt[1], d.z + dt[2], d.w + dt[3]);
    }
}

// out[c] = sum over the partial rows of column c: thread t adds rows t, t + 256, ... in order, then a fixed
// tree over the 256 threads.  One workgroup per column.
__global__ __launch_bounds__(256) void col_sum_kernel(const float *__restrict__ partial, int64_t rows, int ld,
                                                      float *__restrict__ out) {
    __shared__ float s[256];
    const int c = blockIdx.x;
    float v = 0.0f;
    for (int64_t r = threadIdx.x; r < rows; r += 256) v += partial[r * ld + c];
    s[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[c] = s[0];
}

// ---------------------------------------------------------------------------
// decoding_mlp DenseNet([4, 128, 1])
// ---------------------------------------------------------------------------
struct DecW {
    float W0[512], B0[128], W1[128];
    __device__ __forceinline__ void load(const float *w0, const float *b0, const float *w1) {
        for (int t = threadIdx.x; t < 512; t += 256) W0[t] = w0[t];
        if (threadIdx.x < 128) {
            B0[threadIdx.x] = b0[threadIdx.x];
            W1[threadIdx.x] = w1[threadIdx.x];
        }
    }
};

// four lanes per node, lane `sub` takes hidden units sub, sub + 4, ...  d_out null: the forward (out[i] = d);
// else d_h[i] = d_out[i] W0^T (W1 (1 - z^2)).
__global__ __launch_bounds__(256) void decode_train_kernel(const float4 *__restrict__ h, int64_t n_tot,
                                                           const float *__restrict__ w0,
                                                           const float *__restrict__ b0,
                                                           const float *__restrict__ w1,
                                                           const float *__restrict__ b1,
                                                           const float *__restrict__ d_out,
                                                           float *__restrict__ out, float4 *__restrict__ d_h) {
    __shared__ DecW w;
    w.load(w0, b0, w1);
    __syncthreads();
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 2;
    const bool live = i0 < n_tot;
    const int64_t i = live ? i0 : n_tot - 1;
    const int sub = threadIdx.x & 3;
    const float4 hv = h[i];
    if (!d_out) {
        float acc = 0.0f;
        for (int j = sub; j < 128; j += 4) {
            const float z = tanhf(w.B0[j] + w.W0[4 * j] * hv.x + w.W0[4 * j + 1] * hv.y + w.W0[4 * j + 2] * hv.z +
                                  w.W0[4 * j + 3] * hv.w);
            acc += w.W1[j] * z;
        }
        acc += xor_lane_f<1>(acc);
        acc += xor_lane_f<2>(acc);
        if (live && sub == 0) out[i] = acc + b1[0];
        return;
    }
    const float dd = d_out[i];
    float g4[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = sub; j < 128; j += 4) {
        const float z = tanhf(w.B0[j] + w.W0[4 * j] * hv.x + w.W0[4 * j + 1] * hv.y + w.W0[4 * j + 2] * hv.z +
                              w.W0[4 * j + 3] * hv.w);
        const float g = dd * w.W1[j] * (1.0f - z * z);
#pragma unroll
        for (int c = 0; c < 4; ++c) g4[c] += g * w.W0[4 * j + c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        g4[c] += xor_lane_f<1>(g4[c]);
        g4[c] += xor_lane_f<2>(g4[c]);
    }
    if (live && sub == 0) d_h[i] = make_float4(g4[0], g4[1], g4[2], g4[3]);
}

// The decoder's weight sums: thread (half, j) owns hidden unit j and the nodes half, half + 2, ... of the
// workgroup's chunk; half 1's sums are added to half 0's in LDS.  Row: dW0 [128, 4], db0 [128], dW1 [128], db1.
__global__ __launch_bounds__(256) void decode_train_w_kernel(const float4 *__restrict__ h, int64_t n_tot,
                                                             const float *__restrict__ w0,
                                                             const float *__restrict__ b0,
                                                             const float *__restrict__ w1,
                                                             const float *__restrict__ d_out,
                                                             float *__restrict__ partial) {
    __shared__ float4 sh[kDecChunk];
    __shared__ float sd[kDecChunk];
    __shared__ float other[128][7];
    const int64_t first = (int64_t)blockIdx.x * kDecChunk;
    for (int t = threadIdx.x; t < kDecChunk; t += 256) {
        const bool in = first + t < n_tot;
        const int64_t r = in ? first + t : n_tot - 1;
        const float4 hv = h[r];
        const float dv = d_out[r];
        sh[t] = hv;
        sd[t] = in ? dv : 0.0f;
    }
    const int j = threadIdx.x & 127, half = threadIdx.x >> 7;
    const float4 wj = ((const float4 *)w0)[j];
    const float bj = b0[j], oj = w1[j];
    __syncthreads();
    float a[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int t = half; t < kDecChunk; t += 2) {
        const float4 hv = sh[t];
        const float dd = sd[t];
        const float z = tanhf(bj + wj.x * hv.x + wj.y * hv.y + wj.z * hv.z + wj.w * hv.w);
        const float g = dd * oj * (1.0f - z * z);
        a[0] += g * hv.x, a[1] += g * hv.y, a[2] += g * hv.z, a[3] += g * hv.w;
        a[4] += g;
        a[5] += dd * z;
        a[6] += dd;
    }
    if (half == 1) {
#pragma unroll
        for (int t = 0; t < 7; ++t) other[j][t] = a[t];
    }
    __syncthreads();
    if (half == 0) {
        float *row = partial + (int64_t)blockIdx.x * kDecLd;
#pragma unroll
        for (int t = 0; t < 7; ++t) a[t] += other[j][t];
#pragma unroll
        for (int c = 0; c < 4; ++c) row[4 * j + c] = a[c];
        row[512 + j] = a[4];
        row[640 + j] = a[5];
        if (j == 0) row[768] = a[6];
    }
}

inline bool al16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
inline bool al8(const void *p) { return ((uintptr_t)p & 7u) == 0; }
inline bool al4(const void *p) { return ((uintptr_t)p & 3u) == 0; }
inline int64_t up4(int64_t f) { return (f + 3) & ~int64_t(3); }

// staging bytes of the LDS kernels (0: too large, the global-read kernels), as dmm.hip's dmm_gnn_lds_bytes
size_t lds_bytes(int64_t n_per) {
    const int64_t b = n_per * (16 + 8 + 4);
    return b <= 120 * 1024 ? (size_t)b : 0;
}

bool weights_ok(const mmpde_dmm_gnn_weights *w) {
    const float *p[8] = {w->msg1_w, w->msg1_b, w->msg2_w, w->msg2_b, w->upd1_w, w->upd1_b, w->upd2_w, w->upd2_b};
    for (const float *q : p)
        if (!q || !al4(q)) return false;
    return true;
}

template <typename K>
bool lds_allow(K kernel, size_t lds) {
    return lds <= 64 * 1024 ||
           hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
}

int64_t layer_groups(int64_t batches, int64_t n_per) { return batches * ((n_per + kTargets - 1) / kTargets); }

}  // namespace

extern "C" int64_t mmpde_dmm_gnn_train_workspace_bytes(int64_t batches, int64_t n_per, int k) {
    if (batches < 1 || n_per < 1 || k < 1) return 0;
    const int64_t nt = batches * n_per;
    return (4 * nt + up4(layer_groups(batches, n_per) * kLayerGrads) + 4 * nt * k) * (int64_t)sizeof(float);
}

extern "C" int mmpde_dmm_gnn_train_forward(const float *h, const float *u, const float *grid, int64_t batches,
                                           int64_t n_per, const int32_t *nbr, int k, int hidden,
                                           const mmpde_dmm_gnn_weights *w, float *upd, mmpde_stream_t stream) {
    MMPDE_REQUIRE(h && u && grid && nbr && w && upd && weights_ok(w));
    MMPDE_REQUIRE(al16(h) && al16(upd) && al8(grid) && al4(u) && al4(nbr));
    MMPDE_REQUIRE(batches >= 1 && n_per >= 1 && n_per < ((int64_t)1 << 31) / 64);
    if (hidden != 4 || k < 1 || batches > 65535) return MMPDE_ERR_UNSUPPORTED;
    hipStream_t st = as_stream(stream);
    const dim3 g((unsigned)ceil_div(n_per, kTargets), (unsigned)batches);
    size_t lds = lds_bytes(n_per);
    if (lds && !lds_allow(gnn_train_fwd_kernel<true>, lds)) lds = 0;
    if (lds) {
        hipLaunchKernelGGL(gnn_train_fwd_kernel<true>, g, dim3(512), lds, st, (const float4 *)h, u,
                           (const float2 *)grid, nbr, k, (int)n_per, *w, (float4 *)upd);
    } else {
        hipLaunchKernelGGL(gnn_train_fwd_kernel<false>, g, dim3(512), 0, st, (const float4 *)h, u,
                           (const float2 *)grid, nbr, k, (int)n_per, *w, (float4 *)upd);
    }
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

extern "C" int mmpde_dmm_gnn_train_backward(const float *h, const float *u, const float *grid, int64_t batches,
                                            int64_t n_per, const int32_t *nbr, int k, int hidden,
                                            const int64_t *rev_off, const int64_t *rev_edge,
                                            const mmpde_dmm_gnn_weights *w, const float *d_upd, float *d_h,
                                            float *grads, void *workspace, mmpde_stream_t stream) {
    MMPDE_REQUIRE(h && u && grid && nbr && rev_off && rev_edge && w && d_upd && d_h && grads && workspace &&
                  weights_ok(w));
    MMPDE_REQUIRE(al16(h) && al16(d_upd) && al16(d_h) && al16(workspace) && al8(grid) && al8(rev_off) &&
                  al8(rev_edge) && al4(u) && al4(nbr) && al4(grads));
    MMPDE_REQUIRE(batches >= 1 && n_per >= 1 && n_per < ((int64_t)1 << 31) / 64);
    if (hidden != 4 || k < 1 || batches > 65535) return MMPDE_ERR_UNSUPPORTED;
    hipStream_t st = as_stream(stream);
    const int64_t nt = batches * n_per, groups = layer_groups(batches, n_per);
    float4 *d_m = (float4 *)workspace;
    float *partial = (float *)(d_m + nt);
    float4 *edge = (float4 *)(partial + up4(groups * kLayerGrads));
    const dim3 g((unsigned)ceil_div(n_per, kTargets), (unsigned)batches);
    size_t lds = lds_bytes(n_per);
    if (lds && !(lds_allow(gnn_train_upd_kernel<true>, lds) && lds_allow(gnn_train_msg_kernel<true>, lds))) lds = 0;
    if (lds) {
        hipLaunchKernelGGL(gnn_train_upd_kernel<true>, g, dim3(512), lds, st, (const float4 *)h, u,
                           (const float2 *)grid, nbr, k, (int)n_per, *w, (const float4 *)d_upd, (float4 *)d_h, d_m,
                           partial);
        MMPDE_RET_LAUNCH();
        hipLaunchKernelGGL(gnn_train_msg_kernel<true>, g, dim3(512), lds, st, (const float4 *)h, u,
                           (const float2 *)grid, nbr, k, (int)n_per, *w, (const float4 *)d_m, (float4 *)d_h, edge,
                           partial);
    } else {
        hipLaunchKernelGGL(gnn_train_upd_kernel<false>, g, dim3(512), 0, st, (const float4 *)h, u,
                           (const float2 *)grid, nbr, k, (int)n_per, *w, (const float4 *)d_upd, (float4 *)d_h, d_m,
                           partial);
        MMPDE_RET_LAUNCH();
        hipLaunchKernelGGL(gnn_train_msg_kernel<false>, g, dim3(512), 0, st, (const float4 *)h, u,
                           (const float2 *)grid, nbr, k, (int)n_per, *w, (const float4 *)d_m, (float4 *)d_h, edge,
                           partial);
    }
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(gnn_train_src_kernel, dim3((unsigned)ceil_div(n_per, kSrcNodes), (unsigned)batches),
                       dim3(256), 0, st, (const float4 *)edge, rev_off, rev_edge, k, (int)n_per, w->msg1_w,
                       (float4 *)d_h);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(col_sum_kernel, dim3(kLayerGrads), dim3(256), 0, st, partial, groups, kLayerGrads, grads);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

extern "C" int64_t mmpde_dmm_decode_train_workspace_bytes(int64_t n_tot) {
    if (n_tot < 1) return 0;
    return (n_tot + kDecChunk - 1) / kDecChunk * kDecLd * (int64_t)sizeof(float);
}

extern "C" int mmpde_dmm_decode_train_forward(const float *h, int64_t n_tot, int hidden, const float *w0,
                                              const float *b0, const float *w1, const float *b1, float *out,
                                              mmpde_stream_t stream) {
    MMPDE_REQUIRE(h && w0 && b0 && w1 && b1 && out && n_tot >= 1 && n_tot < ((int64_t)1 << 36));
    MMPDE_REQUIRE(al16(h) && al16(w0) && al4(b0) && al4(w1) && al4(b1) && al4(out));
    if (hidden != 4) return MMPDE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(decode_train_kernel, dim3((unsigned)ceil_div(4 * n_tot, 256)), dim3(256), 0,
                       as_stream(stream), (const float4 *)h, n_tot, w0, b0, w1, b1, (const float *)nullptr, out,
                       (float4 *)nullptr);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

extern "C" int mmpde_dmm_decode_train_backward(const float *h, int64_t n_tot, int hidden, const float *w0,
                                               const float *b0, const float *w1, const float *d_out, float *d_h,
                                               float *grads, void *workspace, mmpde_stream_t stream) {
    MMPDE_REQUIRE(h && w0 && b0 && w1 && d_out && d_h && grads && workspace && n_tot >= 1 &&
                  n_tot < ((int64_t)1 << 36));
    MMPDE_REQUIRE(al16(h) && al16(w0) && al16(d_h) && al16(workspace) && al4(b0) && al4(w1) && al4(d_out) &&
                  al4(grads));
    if (hidden != 4) return MMPDE_ERR_UNSUPPORTED;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(decode_train_kernel, dim3((unsigned)ceil_div(4 * n_tot, 256)), dim3(256), 0, st,
                       (const float4 *)h, n_tot, w0, b0, w1, (const float *)nullptr, d_out, (float *)nullptr,
                       (float4 *)d_h);
    MMPDE_RET_LAUNCH();
    const int64_t groups = (n_tot + kDecChunk - 1) / kDecChunk;
    hipLaunchKernelGGL(decode_train_w_kernel, dim3((unsigned)groups), dim3(256), 0, st, (const float4 *)h, n_tot,
                       w0, b0, w1, d_out, (float *)workspace);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(col_sum_kernel, dim3(kDecGrads), dim3(256), 0, st, (const float *)workspace, groups, kDecLd,
                       grads);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}
