// The random-feature phase of DMM training on gfx950 (reference
// mesh/dmm_utils.py:785-1076 and random_feature_torch2, :351-388): the last
// Linear of out_nn is refitted on the Monge-Ampere loss with every other
// weight frozen, so phi = w . s(b, xi) + b_o2 with s = second_out, the tanh
// layer under it, as fixed features.
//
// 1. mmpde_dmm_rf_features: s and its derivatives in xi, per feature.  With
//    z_k = P[b,k] + Q[i,k], J = dQ/dxi and K = dJ/dxi (dmm.hip):
//        s_k    = tanh z_k
//        s_k,d  = (1 - s_k^2) J[i,k,d]
//        s_k,de = (1 - s_k^2) K[i,k,de] - 2 s_k (1 - s_k^2) J[i,k,d] J[i,k,e]
//    which is what mesh_hess contracts with w_o, kept per k.  The reference gets
//    these from 6 L' autograd.grad calls per batch (:883-905).
// 2. mmpde_rf_objective: f(w) and df/dw of random_feature_torch2.
// 3. mmpde_sym_matvec / mmpde_bfgs_update: the two O(n^2) steps of BFGS on the
//    inverse Hessian.
// Every sum runs in a fixed order (lane-strided partials, the wave butterfly,
// then a fixed sequence over waves); there are no atomics.
#include "common.hpp"

namespace {

inline bool al16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
inline bool al4(const void *p) { return ((uintptr_t)p & 3u) == 0; }

// ---------------------------------------------------------------------------
// 1. feature derivatives
// ---------------------------------------------------------------------------
// one thread per (row, feature); every output nullable
__global__ __launch_bounds__(256) void rf_features_kernel(const float *__restrict__ s,
                                                          const float2 *__restrict__ jac,
                                                          const float *__restrict__ kmat, int64_t total,
                                                          float *__restrict__ sx, float *__restrict__ sy,
                                                          float *__restrict__ sxx, float *__restrict__ sxy,
                                                          float *__restrict__ syy) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const float t = s[e];
    const float g = 1.0f - t * t;
    const float2 j = jac[e];
    if (sx) sx[e] = g * j.x;
    if (sy) sy[e] = g * j.y;
    if (kmat) {
        const float g2 = -2.0f * t * g;
        const float ax = g2 * j.x, ay = g2 * j.y;
        const float *k = kmat + e * 3;
        if (sxx) sxx[e] = __fmaf_rn(g, k[0], ax * j.x);
        if (sxy) sxy[e] = __fmaf_rn(g, k[1], ax * j.y);
        if (syy) syy[e] = __fmaf_rn(g, k[2], ay * j.y);
    }
}

// floats past dmm_phi_floats: K [n, L', 3] then an s scratch [n, L']
int64_t rf_extra_floats(int64_t n_grid, int hidden) { return 4 * n_grid * hidden + 64; }

// ---------------------------------------------------------------------------
// 2. the objective
// ---------------------------------------------------------------------------
// dot of one table row with w: lane-strided partials, then the butterfly
__device__ __forceinline__ float row_dot(const float *__restrict__ row, const float *__restrict__ w, int n,
                                         int lane) {
    float a = 0.0f;
    for (int k = lane; k < n; k += 64) a = __fmaf_rn(row[k], w[k], a);
    return wave_sum_full(a);
}

// p = F w.  Wave r < M: the five interior tables of row r -> pin[t * M + r] (t = x,
// y, xx, xy, yy) and the smoother's query x + (p_x, p_y); wave M + side * Mb + j:
// boundary row j of that side -> pb[side * Mb + j].
__global__ __launch_bounds__(256) void rf_apply_kernel(mmpde_rf_problem pb, const float *__restrict__ w,
                                                       float *__restrict__ pin, float *__restrict__ pbd,
                                                       float2 *__restrict__ qry) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n = pb.hidden;
    if (r < pb.m) {
        const float *tab[5] = {pb.so_x, pb.so_y, pb.so_xx, pb.so_xy, pb.so_yy};
        float v[5];
#pragma unroll
        for (int t = 0; t < 5; ++t) v[t] = row_dot(tab[t] + r * n, w, n, lane);
        if (lane == 0) {
#pragma unroll
            for (int t = 0; t < 5; ++t) pin[t * pb.m + r] = v[t];
            qry[r] = make_float2(pb.x[2 * r] + v[0], pb.x[2 * r + 1] + v[1]);
        }
    } else if (r < pb.m + 4 * pb.mb) {
        const int64_t j = r - pb.m;
        const int side = (int)(j / pb.mb);
        const float *tab = side == 0 ? pb.b_x0 : side == 1 ? pb.b_x1 : side == 2 ? pb.b_y0 : pb.b_y1;
        const float v = row_dot(tab + (j - side * pb.mb) * n, w, n, lane);
        if (lane == 0) pbd[j] = v;
    }
}

// sum over the 256 threads of a block in a fixed order; result in every thread
__device__ __forceinline__ float block_sum(float v, float *sh) {
    v = wave_sum_full(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// One workgroup: the loss terms of every row, their sums, f, and df/dp.
//   a = ux (1 + pxx) + uy pxy,  c = ux pxy + uy (1 + pyy),  r = sqrt(a^2 + c^2)
//   m = 1 + r / (0.01 alpha_b), D = (1 + pxx)(1 + pyy) - pxy^2, LHS = m D
// dp [5, M]: slots 0, 1 take df/d(ux), df/d(uy) (the smoother's VJP turns them
// into df/dp_x, df/dp_y: p_x, p_y reach the loss only through its query),
// slots 2..4 df/dp_xx, df/dp_xy, df/dp_yy.  scal: f-side scalars for the g kernel.
__global__ __launch_bounds__(256) void rf_point_kernel(mmpde_rf_problem pb, const float *__restrict__ w,
                                                       const float *__restrict__ pin,
                                                       const float *__restrict__ pbd,
                                                       const float *__restrict__ uxq,
                                                       const float *__restrict__ uyq, float *__restrict__ dp,
                                                       float *__restrict__ scal, float *__restrict__ f,
                                                       float *__restrict__ parts, float *__restrict__ lhs) {
    __shared__ float sh[4];
    const int64_t M = pb.m;
    const int64_t per = M / pb.bu;
    const float invM = 1.0f / (float)M;
    float li = 0.0f, lc = 0.0f, lb = 0.0f, ww = 0.0f;
    for (int64_t i = threadIdx.x; i < M; i += 256) {
        const int64_t b = i / per;
        const float pxx = pin[2 * M + i], pxy = pin[3 * M + i], pyy = pin[4 * M + i];
        const float ux = uxq[i], uy = uyq[i];
        const float hx = 1.0f + pxx, hy = 1.0f + pyy;
        const float a = ux * hx + uy * pxy, c = ux * pxy + uy * hy;
        const float r = sqrtf(a * a + c * c);
        const float ia = 1.0f / (0.01f * pb.alpha[b]);
        const float m = 1.0f + r * ia;
        const float D = hx * hy - pxy * pxy;
        const float L = m * D;
        const float irhs = 1.0f / pb.rhs[b];
        const float e = L * irhs - 1.0f;
        li += e * e;
        const float cx = fminf(0.0f, hx), cy = fminf(0.0f, hy);
        lc += cx * cx + cy * cy;
        if (lhs) lhs[i] = L;
        const float gL = pb.w0 * 2.0f * e * irhs * invM;
        const float dD = gL * m;
        // sqrt has no derivative at a = c = 0 (autograd: NaN); contribute 0 there
        const float dr = r > 0.0f ? gL * D * ia / r : 0.0f;
        const float da = dr * a, dc = dr * c;
        dp[i] = da * hx + dc * pxy;
        dp[M + i] = da * pxy + dc * hy;
        dp[2 * M + i] = da * ux + dD * hy + pb.w2 * 2.0f * cx * invM;
        dp[3 * M + i] = da * uy + dc * ux - 2.0f * dD * pxy;
        dp[4 * M + i] = dc * uy + dD * hx + pb.w2 * 2.0f * cy * invM;
    }
    for (int64_t j = threadIdx.x; j < 4 * pb.mb; j += 256) lb += pbd[j] * pbd[j];
    for (int k = threadIdx.x; k < pb.hidden; k += 256) ww += w[k] * w[k];
    li = block_sum(li, sh) * invM;
    lc = block_sum(lc, sh) * invM;
    lb = block_sum(lb, sh) / (4.0f * (float)pb.mb);
    ww = block_sum(ww, sh);
    if (threadIdx.x == 0) {
        parts[0] = li;
        parts[1] = lb;
        parts[2] = lc;
        *f = pb.convex_rel * ww * ww + pb.w1 * lb + pb.w0 * li + pb.w2 * lc;
        scal[0] = 4.0f * pb.convex_rel * ww;
        scal[1] = pb.w1 * 2.0f / (4.0f * (float)pb.mb);
    }
}

// g[k] = sum_rows F[row][k] df/dp[row] + 4 convex_rel (sum w^2) w[k].  64 columns
// per workgroup, its four waves taking rows 0, 4, ..; 1, 5, ..; ... of every
// table in turn, their partial sums added in a fixed order.
__global__ __launch_bounds__(256) void rf_grad_kernel(mmpde_rf_problem pb, const float *__restrict__ w,
                                                      const float *__restrict__ dp,
                                                      const float2 *__restrict__ gqx,
                                                      const float2 *__restrict__ gqy,
                                                      const float *__restrict__ pbd,
                                                      const float *__restrict__ scal, float *__restrict__ g) {
    __shared__ float sh[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + lane;
    const int n = pb.hidden;
    const int64_t M = pb.m;
    float acc = 0.0f;
    if (k < n) {
        for (int64_t i = wv; i < M; i += 4) {
            const float2 a = gqx[i], b = gqy[i];
            acc = __fmaf_rn(pb.so_x[i * n + k], a.x + b.x, acc);
            acc = __fmaf_rn(pb.so_y[i * n + k], a.y + b.y, acc);
            acc = __fmaf_rn(pb.so_xx[i * n + k], dp[2 * M + i], acc);
            acc = __fmaf_rn(pb.so_xy[i * n + k], dp[3 * M + i], acc);
            acc = __fmaf_rn(pb.so_yy[i * n + k], dp[4 * M + i], acc);
        }
        const float cb = scal[1];
        const float *tab[4] = {pb.b_x0, pb.b_x1, pb.b_y0, pb.b_y1};
#pragma unroll
        for (int s = 0; s < 4; ++s)
            for (int64_t j = wv; j < pb.mb; j += 4)
                acc = __fmaf_rn(tab[s][j * n + k], cb * pbd[s * pb.mb + j], acc);
    }
    sh[wv][lane] = acc;
    __syncthreads();
    if (wv == 0 && k < n)
        g[k] = ((sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane])) + scal[0] * w[k];
}

// floats of the objective's workspace: p_in [5, M], p_b [4 Mb], query [M, 2],
// ux, uy at the query [M] each, dp [5, M], the two smoother VJPs [M, 2] each,
// scalars
int64_t rf_objective_floats(int64_t m, int64_t mb) {
    auto r4 = [](int64_t v) { return (v + 3) & ~int64_t(3); };
    return r4(5 * m) + r4(4 * mb) + r4(2 * m) + 2 * r4(m) + r4(5 * m) + 2 * r4(2 * m) + 64;
}

// ---------------------------------------------------------------------------
// 3. BFGS on the inverse Hessian
// ---------------------------------------------------------------------------
// out[i] = scale * sum_j H[i][j] v[j]; one wave per row
__global__ __launch_bounds__(256) void sym_matvec_kernel(const float *__restrict__ H,
                                                         const float *__restrict__ v, int n, float scale,
                                                         float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;  // wave-uniform
    const float d = row_dot(H + (int64_t)i * n, v, n, lane);
    if (lane == 0) out[i] = scale * d;
}

// sc[0] = rho = 1 / y.s, sc[1] = rho^2 y.Hy + rho, sc[2] = y.s; one workgroup
__global__ __launch_bounds__(256) void bfgs_scalars_kernel(const float *__restrict__ s,
                                                           const float *__restrict__ y,
                                                           const float *__restrict__ hy, int n,
                                                           float *__restrict__ sc) {
    __shared__ float sh[4];
    float ys = 0.0f, yhy = 0.0f;
    for (int k = threadIdx.x; k < n; k += 256) {
        ys = __fmaf_rn(y[k], s[k], ys);
        yhy = __fmaf_rn(y[k], hy[k], yhy);
    }
    ys = block_sum(ys, sh);
    yhy = block_sum(yhy, sh);
    if (threadIdx.x == 0) {
        const float rho = 1.0f / ys;
        sc[0] = rho;
        sc[1] = rho * rho * yhy + rho;
        sc[2] = ys;
    }
}

// H_ij += -rho (s_i Hy_j + Hy_i s_j) + (rho^2 yHy + rho) s_i s_j: the expansion of
// (I - rho s y^T) H (I - rho y s^T) + rho s s^T for a symmetric H.  Products and
// the sum of the two cross terms are rounded one by one, so element (i, j) and
// (j, i) see the same operands in an order that commutes: H stays symmetric
// bit for bit.  Skipped when y.s <= 1e-10 (or NaN).
__global__ __launch_bounds__(256) void bfgs_rank2_kernel(float *__restrict__ H, const float *__restrict__ s,
                                                         const float *__restrict__ hy,
                                                         const float *__restrict__ sc, int n) {
#pragma clang fp contract(off)  // s_i Hy_j + Hy_i s_j must not become fma(s_i, Hy_j, Hy_i s_j)
    if (!(sc[2] > 1e-10f)) return;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)n * n) return;
    const int i = (int)(e / n), j = (int)(e - (int64_t)i * n);
    const float a = s[i] * hy[j], b = hy[i] * s[j];
    const float cross = a + b;
    const float ss = s[i] * s[j];
    H[e] = __fmaf_rn(sc[1], ss, __fmaf_rn(-sc[0], cross, H[e]));
}

}  // namespace

extern "C" int64_t mmpde_dmm_rf_features_workspace_bytes(int64_t batches, int64_t n_grid, int latent,
                                                         int hidden, int th) {
    if (batches <= 0 || n_grid <= 0 || latent <= 0 || hidden <= 0 || th <= 0) return 0;
    const int64_t head = (mmpde_detail::dmm_phi_floats(batches, n_grid, latent, hidden, th) + 3) & ~int64_t(3);
    return (head + rf_extra_floats(n_grid, hidden)) * (int64_t)sizeof(float);
}

extern "C" int mmpde_dmm_rf_features(const float *branch, int64_t batches, const float *grid, int64_t n_grid,
                                     const mmpde_dmm_head *hd, void *workspace, const mmpde_dmm_rf_out *out,
                                     mmpde_stream_t stream) {
    MMPDE_REQUIRE(branch && grid && hd && workspace && out && batches > 0 && n_grid > 0);
    MMPDE_REQUIRE(n_grid % batches == 0 && al16(workspace) && ((uintptr_t)grid & 7u) == 0);
    MMPDE_REQUIRE(al4(branch) && al4(out->s) && al4(out->s_x) && al4(out->s_y) && al4(out->s_xx) &&
                  al4(out->s_xy) && al4(out->s_yy));
    if (!mmpde_detail::dmm_head_ok(hd)) return MMPDE_ERR_UNSUPPORTED;
    hipStream_t st = as_stream(stream);
    const int Lp = hd->hidden;
    float *ws = (float *)workspace;
    float *extra = ws + ((mmpde_detail::dmm_phi_floats(batches, n_grid, hd->latent, Lp, hd->th) + 3) & ~int64_t(3));
    const bool second = out->s_xx || out->s_xy || out->s_yy;
    const bool first = second || out->s_x || out->s_y;
    mmpde_detail::DmmPhiTables t;
    int rc = mmpde_detail::dmm_phi_tables(branch, batches, grid, n_grid, hd, ws, second ? extra : nullptr, &t, st);
    if (rc) return rc;
    float *s = out->s ? out->s : extra + 3 * n_grid * Lp;
    // s is mmpde_dmm_phi's second_out, from its own kernel
    rc = mmpde_detail::dmm_phi_rows(t, hd, nullptr, n_grid, n_grid / batches, nullptr, s, st);
    if (rc || !first) return rc;
    const int64_t total = n_grid * Lp;
    hipLaunchKernelGGL(rf_features_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, st, s, t.jac, t.k,
                       total, out->s_x, out->s_y, out->s_xx, out->s_xy, out->s_yy);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

extern "C" int64_t mmpde_rf_objective_workspace_bytes(int64_t m, int64_t mb) {
    if (m <= 0 || mb <= 0) return 0;
    return rf_objective_floats(m, mb) * (int64_t)sizeof(float);
}

extern "C" int mmpde_rf_objective(const float *w, const mmpde_rf_problem *pb, void *workspace, float *f,
                                  float *g, float *parts, float *lhs, mmpde_stream_t stream) {
    MMPDE_REQUIRE(w && pb && workspace && f && g && parts && al16(workspace));
    MMPDE_REQUIRE(pb->so_x && pb->so_y && pb->so_xx && pb->so_xy && pb->so_yy && pb->b_x0 && pb->b_x1 &&
                  pb->b_y0 && pb->b_y1 && pb->x && pb->ux && pb->uy && pb->alpha && pb->rhs && pb->lattice);
    MMPDE_REQUIRE(pb->m > 0 && pb->mb > 0 && pb->hidden > 0 && pb->bu > 0 && pb->n >= 2 && pb->m % pb->bu == 0);
    MMPDE_REQUIRE(al4(w) && al4(f) && al4(g) && al4(parts) && al4(lhs) && ((uintptr_t)pb->x & 7u) == 0 &&
                  ((uintptr_t)pb->lattice & 7u) == 0);
    const int64_t M = pb->m, Mb = pb->mb;
    auto r4 = [](int64_t v) { return (v + 3) & ~int64_t(3); };
    float *p = (float *)workspace;
    auto take = [&](int64_t nf) {
        float *q = p;
        p += r4(nf);
        return q;
    };
    float *pin = take(5 * M), *pbd = take(4 * Mb), *qry = take(2 * M), *uxq = take(M), *uyq = take(M);
    float *dp = take(5 * M), *gqx = take(2 * M), *gqy = take(2 * M), *scal = take(8);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(rf_apply_kernel, dim3((unsigned)ceil_div(M + 4 * Mb, 4)), dim3(256), 0, st, *pb, w, pin,
                       pbd, (float2 *)qry);
    MMPDE_RET_LAUNCH();
    const int64_t np = (int64_t)pb->n * pb->n;
    const float scale = (float)pb->n;
    int rc = mmpde_softmax_interp(pb->lattice, np, 1, pb->ux, pb->bu, qry, M, scale, uxq, stream);
    if (rc) return rc;
    rc = mmpde_softmax_interp(pb->lattice, np, 1, pb->uy, pb->bu, qry, M, scale, uyq, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(rf_point_kernel, dim3(1), dim3(256), 0, st, *pb, w, pin, pbd, uxq, uyq, dp, scal, f, parts,
                       lhs);
    MMPDE_RET_LAUNCH();
    rc = mmpde_softmax_interp_grad(pb->lattice, np, 1, pb->ux, pb->bu, qry, M, scale, dp, gqx, stream);
    if (rc) return rc;
    rc = mmpde_softmax_interp_grad(pb->lattice, np, 1, pb->uy, pb->bu, qry, M, scale, dp + M, gqy, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(rf_grad_kernel, dim3((unsigned)ceil_div(pb->hidden, 64)), dim3(256), 0, st, *pb, w, dp,
                       (const float2 *)gqx, (const float2 *)gqy, pbd, scal, g);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

extern "C" int mmpde_sym_matvec(const float *H, const float *g, int n, float *d_out, float scale,
                                mmpde_stream_t stream) {
    MMPDE_REQUIRE(H && g && d_out && n >= 1 && n <= MMPDE_BFGS_MAX_N && al4(H) && al4(g) && al4(d_out));
    hipLaunchKernelGGL(sym_matvec_kernel, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, as_stream(stream), H, g,
                       n, scale, d_out);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

extern "C" int64_t mmpde_bfgs_update_workspace_bytes(int n) {
    if (n < 1 || n > MMPDE_BFGS_MAX_N) return 0;
    return (((int64_t)n + 3) / 4 * 4 + 8) * (int64_t)sizeof(float);
}

extern "C" int mmpde_bfgs_update(float *H, const float *s, const float *y, int n, void *workspace,
                                 mmpde_stream_t stream) {
    MMPDE_REQUIRE(H && s && y && workspace && n >= 1 && n <= MMPDE_BFGS_MAX_N && al4(H) && al4(s) && al4(y) &&
                  al16(workspace));
    hipStream_t st = as_stream(stream);
    float *hy = (float *)workspace, *sc = hy + ((int64_t)n + 3) / 4 * 4;
    hipLaunchKernelGGL(sym_matvec_kernel, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, st, H, y, n, 1.0f, hy);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(bfgs_scalars_kernel, dim3(1), dim3(256), 0, st, s, y, hy, n, sc);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(bfgs_rank2_kernel, dim3((unsigned)ceil_div((int64_t)n * n, 256)), dim3(256), 0, st, H, s, hy,
                       sc, n);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}
