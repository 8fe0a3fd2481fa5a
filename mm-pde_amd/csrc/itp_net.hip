// ItpNet interpolation on gfx950 for any --itpnet_node widths and depths
// (reference interpolate.py:5-30,77-93 with the weighted sum of
// data_creator_2d.py:80-83): the shape-generic twin of itp.hip's kernel, which
// keeps serving the default 62 -> 128 -> 64 -> 30.
//
//   X[q]  = [n0x, n0y, ..., n29x, n29y, qx, qy]                   (62)
//   W[q]  = L_{n-1}(tanh(... tanh(L_0(X[q]))))    (62 -> h_1 -> ... -> 30, n <= 5 Linears)
//   out   = (addend + sum_e W[q, e] * vals[b, idx[q, e]]) + addend2
// The scheme is itp.hip's: one wave owns 16 queries and runs the layers
// transposed (features on accumulator rows, queries on lanes) with exact-fp32
// v_mfma_f32_16x16x4_f32.  Lane (g, q) = (l >> 4, l & 15) holds rows 4 g + i of
// each 16-row accumulator tile, the B operand of the next layer's K step (t, i)
// when that layer's K order is k = 16 t + 4 g + i: the pack permutes K so, and
// the activations stay in registers from the gather to the weighted sum.
//
// Every width is zero-padded to 16-row tiles (the pack writes the zeros; a
// padded unit is tanh(0 + 0) = 0 and meets zero columns in the next layer).  A
// layer with T_in input and T_out output tiles is the image
//   [rt < T_out][t < T_in][lane < 64][i < 4]  floats, then  [16 T_out]  biases,
// so a lane's four A operands of steps (t, 0..3) are one 16-byte load and a
// wave's load is 1 KB contiguous.  The 62 inputs (padded to 64) are four
// "tiles" as well: input tile t register i is K step s = 4 t + i, whose lane
// group g holds input 4 s + g, exactly itp.hip's xin[s] (layer 0's image is
// packed in that order).  Every layer is then the same loop.
//
// The tile arrays need compile-time indices: the kernel is instantiated for at
// most TMAX = 4, 8, 16 tiles (the widest layer), the K loop is unrolled to TMAX
// with wave-uniform t < T_in guards, and the finished output tile is filed
// under its (wave-uniform, run-time) index by an unrolled select.  Each output
// tile is one accumulator chain starting from the bias, K steps in order: at
// [128, 64] the same operations in the same order as itp.hip's kernel.
// A operands come straight from the packed image (L2-resident, <= 0.9 MB,
// wave-private loads): no LDS, no barrier.  The loads of up to eight K tiles
// are issued before their first MFMA (steps beyond T_in re-read the last one).
#include "common.hpp"

namespace {

constexpr int kNb = 30;            // ItpNet.n (interpolate.py:8)
constexpr int kIn = 2 * kNb + 2;   // 62
constexpr int kNetThreads = 256;   // MMPDE_ITP_NET_THREADS: four waves, one tile each per trip
constexpr int kNetBlocksPerCu = 4;

static_assert(kNetThreads == MMPDE_ITP_NET_THREADS && kNetBlocksPerCu == MMPDE_ITP_NET_BLOCKS_PER_CU,
              "launch geometry documented in mmpde_hip.h");

// tile counts of the layer boundaries: tiles[0] = 4 (the 62 inputs), tiles[l + 1]
// = ceil(widths[l + 1] / 16); widths kept for the pack
struct NetShape {
    int n_layers;
    int widths[MMPDE_ITP_MAX_LAYERS + 1];
    int tiles[MMPDE_ITP_MAX_LAYERS + 1];
};

// false for a shape outside the limits of mmpde_hip.h
bool net_shape(const mmpde_itp_net *net, NetShape &s) {
    if (!net || net->n_layers < 1 || net->n_layers > MMPDE_ITP_MAX_LAYERS) return false;
    if (net->widths[0] != kIn || net->widths[net->n_layers] != kNb) return false;
    s.n_layers = net->n_layers;
    for (int l = 0; l <= MMPDE_ITP_MAX_LAYERS; ++l) s.widths[l] = s.tiles[l] = 0;
    for (int l = 0; l <= net->n_layers; ++l) {
        const int w = net->widths[l];
        if (w < 1 || w > MMPDE_ITP_MAX_WIDTH) return false;
        s.widths[l] = w;
        s.tiles[l] = (w + 15) / 16;
    }
    return true;
}

int64_t net_floats(const NetShape &s) {
    int64_t n = 0;
    for (int l = 0; l < s.n_layers; ++l) n += (int64_t)s.tiles[l + 1] * (s.tiles[l] * 256 + 16);
    return n;
}

int net_max_tiles(const NetShape &s) {
    int m = 0;
    for (int l = 0; l <= s.n_layers; ++l) m = s.tiles[l] > m ? s.tiles[l] : m;
    return m;
}

struct NetParams {
    const float *w[MMPDE_ITP_MAX_LAYERS];
    const float *b[MMPDE_ITP_MAX_LAYERS];
};

// One thread per float of the image, padding included (every element is
// written).  Lane l of a 16x16x4 A operand: row l & 15, k-index g = l >> 4 of
// the K step.  Layer 0's step s = 4 t + i is inputs 4 s + g (the gather's
// order); the others' step (t, i) is inputs 16 t + 4 g + i.
__global__ void itp_net_pack_kernel(NetShape s, NetParams p, int64_t total, float *__restrict__ pk) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    int64_t f = e;
    float v = 0.0f;
    for (int l = 0; l < s.n_layers; ++l) {
        const int tin = s.tiles[l], tout = s.tiles[l + 1];
        const int win = s.widths[l], wout = s.widths[l + 1];
        const int64_t nw = (int64_t)tout * tin * 256;
        if (f < nw) {
            const int i = (int)(f & 3), lane = (int)(f >> 2) & 63;
            const int blk = (int)(f >> 8), t = blk % tin, rt = blk / tin;
            const int g = lane >> 4;
            const int k = l == 0 ? 16 * t + 4 * i + g : 16 * t + 4 * g + i;
            const int row = 16 * rt + (lane & 15);
            if (row < wout && k < win) v = p.w[l][(int64_t)row * win + k];
            break;
        }
        f -= nw;
        if (f < 16 * tout) {
            if (f < wout) v = p.b[l][f];
            break;
        }
        f -= 16 * tout;
    }
    pk[e] = v;
}

template <int TMAX>
__global__ __launch_bounds__(kNetThreads, 2) void itp_net_kernel(
    const float *__restrict__ src, const float *__restrict__ vals, const float *__restrict__ qry,
    const int32_t *__restrict__ idx, int64_t batches, int64_t n_src, int64_t n_qry, NetShape shp,
    const float *__restrict__ pk, const float *__restrict__ addend, const float *__restrict__ addend2,
    float *__restrict__ out) {
    static_assert(TMAX >= 4, "the 62 inputs are four tiles");
    constexpr int kChunk = TMAX < 8 ? TMAX : 8;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int g = lane >> 4;
    const int64_t tiles_per_b = (n_qry + 15) / 16;
    const int64_t n_tiles = tiles_per_b * batches;

    // trip r of wave w of workgroup b: tile (4 r + w) G + b, G = gridDim.x
    for (int64_t tile = (int64_t)wave * gridDim.x + blockIdx.x; tile < n_tiles;
         tile += (int64_t)gridDim.x * (kNetThreads / 64)) {
        const int64_t b = tile / tiles_per_b;
        const int64_t q0 = (tile - b * tiles_per_b) * 16;
        int64_t q = q0 + (lane & 15);
        const bool valid = q < n_qry;
        if (!valid) q = n_qry - 1;
        const int64_t qrow = b * n_qry + q;
        const int32_t *ir = idx + qrow * kNb;
        const float2 *sp = (const float2 *)src + b * n_src;

        // layer 0's B operand of K step s = 4 t + i: input 4 s + g (neighbour
        // 2 s + g / 2, coordinate g & 1; step 15: the query's coordinates, then 0)
        f32x4 cur[TMAX];
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int s = 4 * t + i;
                float x = 0.0f;
                if (s < 15) {
                    const float2 p = sp[min((uint32_t)ir[2 * s + (g >> 1)], (uint32_t)(n_src - 1))];
                    x = (g & 1) ? p.y : p.x;
                } else if (s == 15) {
                    const float2 p = ((const float2 *)qry)[qrow];
                    x = g == 0 ? p.x : g == 1 ? p.y : 0.0f;
                }
                cur[t][i] = x;
            }
        // the neighbour values of this lane's outputs o = 16 r2 + 4 g + i and the
        // epilogue's addends (a missing one reads the query array in its place
        // and is dropped below), all in flight under the layers
        const float *vb = vals + b * n_src;
        float nv[8];
#pragma unroll
        for (int r2 = 0; r2 < 2; ++r2)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int o = min(16 * r2 + 4 * g + i, kNb - 1);
                nv[4 * r2 + i] = vb[min((uint32_t)ir[o], (uint32_t)(n_src - 1))];
            }
        const float ad1 = (addend ? addend : qry)[qrow];
        const float ad2 = (addend2 ? addend2 : qry)[qrow];

        const float *img = pk;
        int tin = 4;
#pragma unroll 1
        for (int l = 0; l < shp.n_layers; ++l) {
            const int tout = min(shp.tiles[l + 1], TMAX);
            const float *bias = img + (int64_t)tout * tin * 256;
            const bool hidden = l + 1 < shp.n_layers;
            f32x4 nxt[TMAX];
#pragma unroll
            for (int u = 0; u < TMAX; ++u) nxt[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
            for (int rt = 0; rt < tout; ++rt) {
                const float4 *wp = (const float4 *)img + (int64_t)rt * tin * 64 + lane;
                const float4 bv = *(const float4 *)(bias + 16 * rt + 4 * g);
                f32x4 acc = {bv.x, bv.y, bv.z, bv.w};
                // kChunk K tiles at a time: their loads all issued, then their MFMAs
                // (16 tiles of operands in flight beside 32 tiles of activations spill)
#pragma unroll
                for (int c = 0; c < TMAX; c += kChunk) {
                    if (c < tin) {
                        float4 w[kChunk];
#pragma unroll
                        for (int t = 0; t < kChunk; ++t) w[t] = wp[min(c + t, tin - 1) * 64];
#pragma unroll
                        for (int t = 0; t < kChunk; ++t)
                            if (c + t < tin) {
                                acc = mfma16(w[t].x, cur[c + t][0], acc);
                                acc = mfma16(w[t].y, cur[c + t][1], acc);
                                acc = mfma16(w[t].z, cur[c + t][2], acc);
                                acc = mfma16(w[t].w, cur[c + t][3], acc);
                            }
                    }
                }
                if (hidden) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = tanhf(acc[i]);
                }
#pragma unroll
                for (int u = 0; u < TMAX; ++u)
                    if (u == rt) nxt[u] = acc;
            }
#pragma unroll
            for (int u = 0; u < TMAX; ++u) cur[u] = nxt[u];
            img = bias + 16 * tout;
            tin = tout;
        }
        // weighted sum of the neighbour values (data_creator_2d.py:83): this lane's
        // outputs o = 16 r2 + 4 g + i, then the 4 lanes of the query
        float sum = 0.0f;
#pragma unroll
        for (int r2 = 0; r2 < 2; ++r2)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int o = 16 * r2 + 4 * g + i;
                if (o < kNb) sum += cur[r2][i] * nv[4 * r2 + i];
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        if (g == 0 && valid) {
            float o = addend ? ad1 + sum : sum;
            if (addend2) o = o + ad2;  // (interp + res) + model(graph_uniform)
            out[qrow] = o;
        }
    }
}

}  // namespace

extern "C" int64_t mmpde_itp_net_pack_bytes(const mmpde_itp_net *net) {
    NetShape s;
    if (!net_shape(net, s)) return 0;
    return net_floats(s) * (int64_t)sizeof(float);
}

extern "C" int mmpde_itp_net_pack(const mmpde_itp_net *net, void *packed, int64_t packed_bytes,
                                  mmpde_stream_t stream) {
    NetShape s;
    MMPDE_REQUIRE(net_shape(net, s));
    MMPDE_REQUIRE(packed && (((uintptr_t)packed) & 15u) == 0);
    const int64_t total = net_floats(s);
    MMPDE_REQUIRE(packed_bytes >= total * (int64_t)sizeof(float));
    NetParams p;
    for (int l = 0; l < MMPDE_ITP_MAX_LAYERS; ++l) {
        p.w[l] = l < s.n_layers ? net->w[l] : nullptr;
        p.b[l] = l < s.n_layers ? net->b[l] : nullptr;
        MMPDE_REQUIRE(l >= s.n_layers || (p.w[l] && p.b[l]));
    }
    hipLaunchKernelGGL(itp_net_pack_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), s, p,
                       total, (float *)packed);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

extern "C" int mmpde_itp_interp_net(const float *src, const float *vals, const float *qry,
                                    const int32_t *idx, int64_t batches, int64_t n_src, int64_t n_qry,
                                    const mmpde_itp_net *shape, const void *packed, int64_t packed_bytes,
                                    const float *addend, const float *addend2, float *out,
                                    mmpde_stream_t stream) {
    MMPDE_REQUIRE(src && vals && qry && idx && shape && packed && out);
    NetShape s;
    MMPDE_REQUIRE(net_shape(shape, s));
    MMPDE_REQUIRE((((uintptr_t)packed) & 15u) == 0);
    // the kernel never reads past an image built for another shape
    MMPDE_REQUIRE(packed_bytes >= net_floats(s) * (int64_t)sizeof(float));
    MMPDE_REQUIRE(batches > 0 && n_src >= kNb && n_qry > 0);
    const int64_t tiles = ((n_qry + 15) / 16) * batches;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        cus = 256;
    int64_t blocks = (int64_t)kNetBlocksPerCu * cus;
    const int64_t need = (tiles + kNetThreads / 64 - 1) / (kNetThreads / 64);
    if (blocks > need) blocks = need;
    const int tmax = net_max_tiles(s);
    auto kern = tmax <= 4 ? itp_net_kernel<4> : tmax <= 8 ? itp_net_kernel<8> : itp_net_kernel<16>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kNetThreads), 0, as_stream(stream), src, vals, qry, idx,
                       batches, n_src, n_qry, s, (const float *)packed, addend, addend2, out);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}
