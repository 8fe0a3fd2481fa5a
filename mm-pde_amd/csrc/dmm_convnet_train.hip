// DMM array branch in train() mode on gfx950 (reference mesh/dmm_model.py:48-81
// under model.train()): ConvNet's convolution stack, forward and backward, for
// u [B, s, s]:
//     x1 = tanh(c0(u))           1 -> 8,  5x5, stride 2, pad 2    [8,  o1, o1]
//     x2 = tanh(c1(x1))          8 -> 16, 5x5, stride 1, pad 2    [16, o1, o1]
//     x3 = tanh(x1 + c2(x2))     16 -> 8, 5x5, stride 1, pad 2    [8,  o1, o1]
//     x4 = tanh(c3(x3))          8 -> 1,  5x5, stride 2, pad 2    [o2, o2] = f
// o1 = (s - 1) / 2 + 1, o2 = (o1 - 1) / 2 + 1.  fc2 / fc3 run on the few-row
// kernels (ops.FewRowsMlp).
//
// One workgroup of 512 threads per field, everything in LDS: the 6833 weights,
// u and x1, x2, x3 as planes with a zero halo (two cells on every side, and a
// row stride rounded up to the widest strip a thread computes), so that no tap
// tests a bound: a tap outside the image reads a stored zero.  The plane stride
// is odd, so the same cell of different channels lies in different banks.  The
// four layers are chained inside the launch; every output is a chain of fp32
// FMAs over (input channel, ky, kx) in that order.
//
// Backward from d_f, nothing kept from the forward: the same launch recomputes
// x1..x4, then walks back in place --
//     dz4 = d_f (1 - x4^2);                     d c3 = dz4 (*) x3
//     x3 <- dz3 = (c3^T dz4)(1 - x3^2);         d c2 = dz3 (*) x2
//     x2 <- dz2 = (c2^T dz3)(1 - x2^2);         d c1 = dz2 (*) x1
//     x1 <- dz1 = (dz3 + c1^T dz2)(1 - x1^2);   d c0 = dz1 (*) u
// (dz3 reaches x1 through the residual).  The stride-1 transposes are the same
// strip convolution on the flipped kernel; c3's stride-2 transpose tests the
// parity of each tap.  A weight gradient is one thread per (out channel, in
// channel, part of the rows) holding the 25 taps in registers, then a fixed
// xor butterfly over the parts (adjacent lanes); the bias gradients ride along.
// Each field leaves its 6833 sums in its own workspace row and a second kernel
// adds the rows in field order.  No atomics, no memset: the same bits on every
// run, and a field's forward does not depend on the batch it sits in.
#include "common.hpp"

namespace {

constexpr int kThreads = 512;
constexpr int kGrads = MMPDE_DMM_CONVNET_TRAIN_GRADS;
constexpr int kRow = 6836;                  // floats per field in the workspace (16-B multiple)
constexpr int kLdsFloats = 160 * 1024 / 4;  // LDS of one CU, all of it one workgroup's
// offsets of the eight tensors in the weight image and in a gradient row
constexpr int oW0 = 0, oB0 = 200, oW1 = 208, oB1 = 3408, oW2 = 3424, oB2 = 6624, oW3 = 6632, oB3 = 6832;
static_assert(oB3 + 1 == kGrads && kGrads <= kRow, "gradient row layout");

__host__ __device__ constexpr int rup(int a, int m) { return (a + m - 1) / m * m; }

// LDS layout in floats for resolution s.  u: (s + 4)^2.  x1, x2, x3: rows o1 + 4, row stride pw1 = the widest
// strip reach (strips of 3 outputs in the stride-1 convolutions, chunks of 4 in their weight gradients) + 4.
struct Geo {
    int s, o1, o2, pwu, pw1, ps1;
    int w, u, a, b, c, f, d4, total;
};
__host__ __device__ constexpr Geo make_geo(int s) {
    Geo g{};
    g.s = s;
    g.o1 = (s - 1) / 2 + 1;
    g.o2 = (g.o1 - 1) / 2 + 1;
    g.pwu = s + 4;
    const int r3 = rup(g.o1, 3), r4 = rup(g.o1, 4);
    g.pw1 = (r3 > r4 ? r3 : r4) + 4;
    g.ps1 = ((g.o1 + 4) * g.pw1) | 1;
    g.w = 0;
    g.u = kRow;
    g.a = g.u + g.pwu * g.pwu;
    g.b = g.a + 8 * g.ps1;
    g.c = g.b + 16 * g.ps1;
    g.f = g.c + 8 * g.ps1;
    g.d4 = g.f + g.o2 * g.o2;
    g.total = g.d4 + g.o2 * g.o2;
    return g;
}
// the largest S with every s <= S inside the LDS of one CU
constexpr int max_s() {
    int s = 1;
    while (make_geo(s + 1).total <= kLdsFloats) ++s;
    return s;
}
static_assert(max_s() == MMPDE_DMM_CONVNET_TRAIN_MAX_S, "MMPDE_DMM_CONVNET_TRAIN_MAX_S follows from the LDS layout");
static_assert(make_geo(48).total <= kLdsFloats, "the reference's Burgers resolution");

// 5x5 convolution over haloed LDS planes: out(o, y, x) = sum_{i, ky, kx} weight(o, i, ky, kx) in[i][y S + ky][x S +
// kx] in haloed coordinates, a thread per (CG output channels, row, strip of SW outputs).  FLIP: the transposed
// stride-1 convolution, in = the NI planes of dz, weight(o, i, tap) = w[i][o][24 - tap].  epi(o, y, x, sum) for
// x < ow only: the halo is never written.
template <int NI, int NO, int S, int CG, int SW, bool FLIP, class Epi>
__device__ __forceinline__ void conv5(const float *in, int pwi, int psi, const float *w, int oh, int ow, Epi epi) {
    static_assert(NO % CG == 0, "channel groups");
    constexpr int WN = (SW - 1) * S + 5;
    const int nstrip = (ow + SW - 1) / SW;
    const int items = (NO / CG) * oh * nstrip;
    for (int it = threadIdx.x; it < items; it += kThreads) {
        const int xs = it % nstrip, t2 = it / nstrip;
        const int y = t2 % oh, cog = t2 / oh;
        float acc[CG][SW];
#pragma unroll
        for (int c = 0; c < CG; ++c)
#pragma unroll
            for (int p = 0; p < SW; ++p) acc[c][p] = 0.0f;
        const float *base = in + (y * S) * pwi + xs * SW * S;
        for (int i = 0; i < NI; ++i) {
#pragma unroll
            for (int ky = 0; ky < 5; ++ky) {
                const float *row = base + i * psi + ky * pwi;
                float win[WN];
#pragma unroll
                for (int t = 0; t < WN; ++t) win[t] = row[t];
#pragma unroll
                for (int kx = 0; kx < 5; ++kx) {
#pragma unroll
                    for (int c = 0; c < CG; ++c) {
                        const int o = cog * CG + c;
                        const float wv = FLIP ? w[(i * NO + o) * 25 + 24 - (ky * 5 + kx)]
                                              : w[(o * NI + i) * 25 + ky * 5 + kx];
#pragma unroll
                        for (int p = 0; p < SW; ++p) acc[c][p] = fmaf(wv, win[p * S + kx], acc[c][p]);
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < CG; ++c)
#pragma unroll
            for (int p = 0; p < SW; ++p) {
                const int x = xs * SW + p;
                if (x < ow) epi(cog * CG + c, y, x, acc[c][p]);
            }
    }
}

// Weight and bias gradient of a 5x5 convolution: gw[(o NI + i) 25 + tap] = sum_{y, x} dz[o][y][x] in[i][y S + ky][x S
// + kx], gb[o] = sum dz[o].  dz points at output (0, 0) of plane 0 (row stride pwo, plane stride pso), `in` at the
// haloed origin.  Thread = (o, i, part): part takes rows part, part + PARTS, ...; x in chunks of CH outputs.  A chunk
// may run past ow: there dz reads a stored zero of the halo (CH > 1 only for haloed dz planes) and `in` stays inside
// its row.  The parts are adjacent lanes: a fixed butterfly adds them.
template <int NO, int NI, int S, int CH, int PARTS>
__device__ __forceinline__ void wgrad5(const float *dz, int pwo, int pso, const float *in, int pwi, int psi, int oh,
                                       int ow, float *gw, float *gb) {
    static_assert(NO * NI * PARTS == kThreads && PARTS <= 64, "one thread per (o, i, part)");
    constexpr int WN = (CH - 1) * S + 5;
    const int part = threadIdx.x % PARTS, pair = threadIdx.x / PARTS;
    const int i = pair % NI, o = pair / NI;
    float acc[25];
#pragma unroll
    for (int t = 0; t < 25; ++t) acc[t] = 0.0f;
    float accb = 0.0f;
    const int nch = (ow + CH - 1) / CH;
    for (int y = part; y < oh; y += PARTS) {
        for (int c = 0; c < nch; ++c) {
            const float *dr = dz + o * pso + y * pwo + c * CH;
            float d[CH];
#pragma unroll
            for (int p = 0; p < CH; ++p) {
                d[p] = dr[p];
                accb += d[p];
            }
            const float *base = in + i * psi + (y * S) * pwi + c * CH * S;
#pragma unroll
            for (int ky = 0; ky < 5; ++ky) {
                float win[WN];
#pragma unroll
                for (int t = 0; t < WN; ++t) win[t] = base[ky * pwi + t];
#pragma unroll
                for (int kx = 0; kx < 5; ++kx)
#pragma unroll
                    for (int p = 0; p < CH; ++p) acc[ky * 5 + kx] = fmaf(d[p], win[p * S + kx], acc[ky * 5 + kx]);
            }
        }
    }
#pragma unroll
    for (int off = PARTS / 2; off >= 1; off >>= 1) {
#pragma unroll
        for (int t = 0; t < 25; ++t) acc[t] += __shfl_xor(acc[t], off, 64);
        accb += __shfl_xor(accb, off, 64);
    }
    if (part == 0) {
#pragma unroll
        for (int t = 0; t < 25; ++t) gw[pair * 25 + t] = acc[t];
        if (i == 0) gb[o] = accb;
    }
}

// One field per workgroup.  BWD false: f_out[field] = x4.  BWD true: partial[field] = the field's 6833 gradient sums.
template <bool BWD>
__global__ __launch_bounds__(kThreads) void convnet_train_kernel(const float *__restrict__ u, int s,
                                                                 mmpde_dmm_convnet_weights wp,
                                                                 const float *__restrict__ d_f,
                                                                 float *__restrict__ f_out,
                                                                 float *__restrict__ partial) {
    extern __shared__ float lds[];
    const Geo g = make_geo(s);
    const int tid = threadIdx.x;
    const int64_t field = blockIdx.x;
    const int o1 = g.o1, o2 = g.o2, pw1 = g.pw1, ps1 = g.ps1, pwu = g.pwu;
    float *W = lds + g.w, *U = lds + g.u, *A = lds + g.a, *Bq = lds + g.b, *C = lds + g.c, *F = lds + g.f;
    const int in1 = 2 * pw1 + 2;   // output (0, 0) of a haloed plane

    for (int j = tid; j < kGrads; j += kThreads) {
        float v;
        if (j < oB0) v = wp.c0_w[j - oW0];
        else if (j < oW1) v = wp.c0_b[j - oB0];
        else if (j < oB1) v = wp.c1_w[j - oW1];
        else if (j < oW2) v = wp.c1_b[j - oB1];
        else if (j < oB2) v = wp.c2_w[j - oW2];
        else if (j < oW3) v = wp.c2_b[j - oB2];
        else if (j < oB3) v = wp.c3_w[j - oW3];
        else v = wp.c3_b[0];
        W[j] = v;
    }
    for (int j = g.u + tid; j < g.f; j += kThreads) lds[j] = 0.0f;   // u, x1, x2, x3 with their halos
    __syncthreads();
    const float *uf = u + field * (int64_t)s * s;
    for (int j = tid; j < s * s; j += kThreads) U[(j / s + 2) * pwu + j % s + 2] = uf[j];
    __syncthreads();

    conv5<1, 8, 2, 4, 1, false>(U, pwu, 0, W + oW0, o1, o1, [&](int o, int y, int x, float v) {
        A[o * ps1 + in1 + y * pw1 + x] = tanhf(v + W[oB0 + o]);
    });
    __syncthreads();
    conv5<8, 16, 1, 8, 3, false>(A, pw1, ps1, W + oW1, o1, o1, [&](int o, int y, int x, float v) {
        Bq[o * ps1 + in1 + y * pw1 + x] = tanhf(v + W[oB1 + o]);
    });
    __syncthreads();
    conv5<16, 8, 1, 4, 3, false>(Bq, pw1, ps1, W + oW2, o1, o1, [&](int o, int y, int x, float v) {
        const int e = o * ps1 + in1 + y * pw1 + x;
        C[e] = tanhf(A[e] + (v + W[oB2 + o]));
    });
    __syncthreads();
    conv5<8, 1, 2, 1, 1, false>(C, pw1, ps1, W + oW3, o2, o2, [&](int, int y, int x, float v) {
        const float t = tanhf(v + W[oB3]);
        if constexpr (BWD) F[y * o2 + x] = t;
        else f_out[field * (int64_t)o2 * o2 + y * o2 + x] = t;
    });
    if constexpr (BWD) {
        float *D4 = lds + g.d4;
        float *row = partial + field * (int64_t)kRow;
        __syncthreads();
        const float *df = d_f + field * (int64_t)o2 * o2;
        for (int j = tid; j < o2 * o2; j += kThreads) D4[j] = df[j] * (1.0f - F[j] * F[j]);
        __syncthreads();
        wgrad5<1, 8, 2, 1, 64>(D4, o2, 0, C, pw1, ps1, o2, o2, row + oW3, row + oB3);
        __syncthreads();
        // x3 <- dz3: c3's transposed stride-2 convolution, a tap only where (Y + 2 - ky) and (X + 2 - kx) are even
        for (int e = tid; e < 8 * o1 * o1; e += kThreads) {
            const int X = e % o1, t2 = e / o1;
            const int Y = t2 % o1, ci = t2 / o1;
            float v = 0.0f;
#pragma unroll
            for (int ky = 0; ky < 5; ++ky) {
                const int ty = Y + 2 - ky;
                if (ty < 0 || (ty & 1) || (ty >> 1) >= o2) continue;
#pragma unroll
                for (int kx = 0; kx < 5; ++kx) {
                    const int tx = X + 2 - kx;
                    if (tx < 0 || (tx & 1) || (tx >> 1) >= o2) continue;
                    v = fmaf(D4[(ty >> 1) * o2 + (tx >> 1)], W[oW3 + ci * 25 + ky * 5 + kx], v);
                }
            }
            const int q = ci * ps1 + in1 + Y * pw1 + X;
            C[q] = v * (1.0f - C[q] * C[q]);
        }
        __syncthreads();
        wgrad5<8, 16, 1, 4, 4>(C + in1, pw1, ps1, Bq, pw1, ps1, o1, o1, row + oW2, row + oB2);
        __syncthreads();
        conv5<8, 16, 1, 8, 3, true>(C, pw1, ps1, W + oW2, o1, o1, [&](int o, int y, int x, float v) {
            const int e = o * ps1 + in1 + y * pw1 + x;
            Bq[e] = v * (1.0f - Bq[e] * Bq[e]);
        });
        __syncthreads();
        wgrad5<16, 8, 1, 4, 4>(Bq + in1, pw1, ps1, A, pw1, ps1, o1, o1, row + oW1, row + oB1);
        __syncthreads();
        conv5<16, 8, 1, 4, 3, true>(Bq, pw1, ps1, W + oW1, o1, o1, [&](int o, int y, int x, float v) {
            const int e = o * ps1 + in1 + y * pw1 + x;
            A[e] = (v + C[e]) * (1.0f - A[e] * A[e]);
        });
        __syncthreads();
        wgrad5<8, 1, 2, 1, 64>(A + in1, pw1, ps1, U, pwu, 0, o1, o1, row + oW0, row + oB0);
    }
}

// grads[j] = partial[0][j] + partial[1][j] + ... in field order
__global__ __launch_bounds__(256) void convnet_grad_sum_kernel(const float *__restrict__ partial, int64_t batches,
                                                               float *__restrict__ grads) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= kGrads) return;
    float v = partial[j];
    for (int64_t b = 1; b < batches; ++b) v += partial[b * kRow + j];
    grads[j] = v;
}

inline bool al4(const void *p) { return ((uintptr_t)p & 3u) == 0; }
inline bool al16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

bool weights_ok(const mmpde_dmm_convnet_weights *w) {
    const float *p[8] = {w->c0_w, w->c0_b, w->c1_w, w->c1_b, w->c2_w, w->c2_b, w->c3_w, w->c3_b};
    for (const float *q : p)
        if (!q || !al4(q)) return false;
    return true;
}

template <typename K>
bool lds_allow(K kernel, size_t lds) {
    return lds <= 64 * 1024 ||
           hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
}

constexpr int64_t kMaxBatches = (int64_t)1 << 24;

}  // namespace

extern "C" int64_t mmpde_dmm_convnet_train_workspace_bytes(int64_t batches) {
    if (batches < 1 || batches > kMaxBatches) return 0;
    return batches * kRow * (int64_t)sizeof(float);
}

extern "C" int mmpde_dmm_convnet_train_forward(const float *u, int64_t batches, int s,
                                               const mmpde_dmm_convnet_weights *w, float *f,
                                               mmpde_stream_t stream) {
    MMPDE_REQUIRE(u && w && f && weights_ok(w) && al4(u) && al4(f));
    MMPDE_REQUIRE(batches >= 1 && s >= 1);
    if (s > MMPDE_DMM_CONVNET_TRAIN_MAX_S || batches > kMaxBatches) return MMPDE_ERR_UNSUPPORTED;
    const size_t lds = (size_t)make_geo(s).total * sizeof(float);
    if (!lds_allow(convnet_train_kernel<false>, lds)) return MMPDE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(convnet_train_kernel<false>, dim3((unsigned)batches), dim3(kThreads), lds, as_stream(stream), u,
                       s, *w, (const float *)nullptr, f, (float *)nullptr);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

extern "C" int mmpde_dmm_convnet_train_backward(const float *u, int64_t batches, int s,
                                                const mmpde_dmm_convnet_weights *w, const float *d_f,
                                                float *grads, void *workspace, int64_t workspace_bytes,
                                                mmpde_stream_t stream) {
    MMPDE_REQUIRE(u && w && d_f && grads && workspace && weights_ok(w));
    MMPDE_REQUIRE(al4(u) && al4(d_f) && al4(grads) && al16(workspace));
    MMPDE_REQUIRE(batches >= 1 && s >= 1);
    if (s > MMPDE_DMM_CONVNET_TRAIN_MAX_S || batches > kMaxBatches) return MMPDE_ERR_UNSUPPORTED;
    MMPDE_REQUIRE(workspace_bytes >= mmpde_dmm_convnet_train_workspace_bytes(batches));
    hipStream_t st = as_stream(stream);
    const size_t lds = (size_t)make_geo(s).total * sizeof(float);
    if (!lds_allow(convnet_train_kernel<true>, lds)) return MMPDE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(convnet_train_kernel<true>, dim3((unsigned)batches), dim3(kThreads), lds, st, u, s, *w, d_f,
                       (float *)nullptr, (float *)workspace);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(convnet_grad_sum_kernel, dim3((unsigned)ceil_div(kGrads, 256)), dim3(256), 0, st,
                       (const float *)workspace, batches, grads);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}
