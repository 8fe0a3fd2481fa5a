// Mesh quality of the rollout's moved mesh: the equidistributed quantity of the
// reference's evaluate / evaluate_tri (mesh/dmm_utils.py:1162-1284), monitor
// function at each moved cell's centre times the cell's area, as per-trajectory
// statistics, and the discrete fold check beside it: the signed area of every
// moved cell against the same cell of the fixed grid.
//
// The monitor field lives on the n x n unit lattice, flat 'xy' order (point
// i n + j = (x_j, y_i), x_j = j / (n - 1); dmm_utils.py:241-243):
//     alpha = sum sqrt(ux^2 + uy^2) / (n - 1)^2
//     m     = 1 + sqrt(ux^2 + uy^2) / (0.01 alpha)          (dmm_utils.py:209-210)
//     rhs   = sum m / (n - 1)^2
// from forward differences of array data (dmm_utils.py:215-225, scaled by s - 1
// as sample_train_data does, :36-37) or from a gradient field already on the
// lattice (point data: mmpde_softmax_interp_grad's, dmm_utils.py:128-139).  A
// constant field has alpha = 0 and gives NaN, as the reference does.
//
// m at a cell centre is the reference's `interpolate` (dmm_utils.py:233-249):
// softmax weights of -n |p_j - c| over all n^2 lattice points, no window.  The
// largest exponent is known before the sum (the lattice point nearest the
// centre, found per axis), so the sums need no running maximum.
//
// Every sum is taken in an order fixed by the shapes of one trajectory alone: a
// trajectory's outputs do not depend on the batch around it, nor on the run.
#include "common.hpp"

namespace {

// ---------------------------------------------------------------------------
// Monitor field.  One workgroup per trajectory; the two sums in thread-strided
// order, wave butterfly, then the four waves' partials in wave order.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float block_sum_256(float v, float *s4) {
    v = wave_sum_full(v);
    __syncthreads();  // s4 may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

// GRAD = false: src = u [B, n, n], ux / uy its forward differences along the
// first / second lattice axis times n - 1, last row / column repeated.
// GRAD = true: src = (ux, uy) [B, n n, 2].
template <bool GRAD>
__global__ __launch_bounds__(256) void monitor_kernel(const float *__restrict__ src, int n,
                                                      float *__restrict__ m_out,
                                                      float *__restrict__ alpha_out,
                                                      float *__restrict__ rhs_out) {
    __shared__ float s4[4];
    const int n2 = n * n;
    const int64_t base = (int64_t)blockIdx.x * n2;
    const float *s = src + (GRAD ? 2 * base : base);
    float *m = m_out + base;
    const float scale = (float)(n - 1);
    const float cells = scale * scale;
    // |grad u| into m, and its sum
    float acc = 0.0f;
    for (int e = threadIdx.x; e < n2; e += 256) {
        float ux, uy;
        if (GRAD) {
            const float2 g = ((const float2 *)s)[e];
            ux = g.x;
            uy = g.y;
        } else {
            const int i = e / n, j = e - i * n;
            const int ii = min(i, n - 2), jj = min(j, n - 2);
            ux = (s[(ii + 1) * n + j] - s[ii * n + j]) * scale;
            uy = (s[i * n + jj + 1] - s[i * n + jj]) * scale;
        }
        const float g = sqrtf(ux * ux + uy * uy);
        m[e] = g;
        acc += g;
    }
    const float alpha = block_sum_256(acc, s4) / cells;
    const float den = 0.01f * alpha;
    acc = 0.0f;
    for (int e = threadIdx.x; e < n2; e += 256) {  // each thread rereads its own stores
        const float v = 1.0f + m[e] / den;
        m[e] = v;
        acc += v;
    }
    const float rhs = block_sum_256(acc, s4) / cells;
    if (threadIdx.x == 0) {
        alpha_out[blockIdx.x] = alpha;
        rhs_out[blockIdx.x] = rhs;
    }
}

// ---------------------------------------------------------------------------
// Cells.
// ---------------------------------------------------------------------------
struct CellGeom {
    float cx, cy, area, sgn;  // centre, the reference's area, signed area
};

// Vertex v of a cell, its index clamped into the trajectory (the host cannot
// check a device table; a wrong index reads a wrong node, never out of bounds).
__device__ __forceinline__ float2 cell_vertex(const float2 *__restrict__ pts, const int4 c, int v, int n_per) {
    const int idx = v == 0 ? c.x : v == 1 ? c.y : v == 2 ? c.z : c.w;
    return pts[min((uint32_t)idx, (uint32_t)(n_per - 1))];
}

// arity 4, vertices (bl, br, tl, tr) (dmm_utils.py:1264-1267): area = the
// product of the diagonals / 2 (:1269-1272; not the true area of a general
// quadrilateral, kept as the reference has it), centre = the vertices' mean
// (:1273), signed area = (tr - bl) x (tl - br) / 2.
// arity 3 (dmm_utils.py:1192-1198): area = |cross| / 2 of the edge vectors from
// vertex 0 (the reference's determinant form, with less cancellation), centroid
// = the vertices' mean, signed area = cross / 2.
template <int ARITY>
__device__ __forceinline__ CellGeom cell_geom(const float2 *__restrict__ pts, const int4 c, int n_per) {
    CellGeom g;
    const float2 a = cell_vertex(pts, c, 0, n_per), b = cell_vertex(pts, c, 1, n_per);
    const float2 d = cell_vertex(pts, c, 2, n_per);
    if (ARITY == 4) {
        const float2 e = cell_vertex(pts, c, 3, n_per);
        const float p1x = a.x - e.x, p1y = a.y - e.y;  // bl - tr
        const float p2x = b.x - d.x, p2y = b.y - d.y;  // br - tl
        g.area = sqrtf(p1x * p1x + p1y * p1y) * sqrtf(p2x * p2x + p2y * p2y) / 2.0f;
        g.cx = (((a.x + b.x) + d.x) + e.x) / 4.0f;
        g.cy = (((a.y + b.y) + d.y) + e.y) / 4.0f;
        // (tr - bl) x (tl - br) = (-p1) x (-p2) = p1 x p2
        g.sgn = 0.5f * (p1x * p2y - p1y * p2x);
    } else {
        const float e1x = b.x - a.x, e1y = b.y - a.y, e2x = d.x - a.x, e2y = d.y - a.y;
        const float cr = e1x * e2y - e2x * e1y;
        g.area = 0.5f * fabsf(cr);
        g.cx = ((a.x + b.x) + d.x) / 3.0f;
        g.cy = ((a.y + b.y) + d.y) / 3.0f;
        g.sgn = 0.5f * cr;
    }
    return g;
}

// Lattice floats staged per tile of whole rows (32 KiB; n <= 90: the whole field)
constexpr int kTileFloats = 8192;
constexpr int kCellsPerBlock = 64;  // 256 threads: four lanes per cell

static inline int tile_rows(int n) { return n * n <= kTileFloats ? n : (kTileFloats / n > 0 ? kTileFloats / n : 1); }

// mg[b, c] = m_b(centre of cell c of trajectory b) * area.  Workgroup (x, b)
// takes 64 cells of trajectory b, four lanes per cell: lane `sub` of the quad
// takes lattice columns sub, sub + 4, ... of every row, the quad's sums meet by
// two xor exchanges.  The trajectory's m is staged in LDS by row tiles beside
// the lattice coordinates float(i) / float(n - 1) (unit_lattice's own bits).
template <int ARITY>
__global__ __launch_bounds__(256) void cell_mg_kernel(const float2 *__restrict__ mesh,
                                                      const int4 *__restrict__ cells, int n_cells,
                                                      int n_per, const float *__restrict__ m, int n,
                                                      int rows_per_tile, float *__restrict__ mg) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sx = smem;                    // [n] lattice coordinates
    float *sm = smem + ((n + 3) & ~3);   // [rows_per_tile, n]
    const int b = blockIdx.y;
    const int cell = blockIdx.x * kCellsPerBlock + (threadIdx.x >> 2);
    const int sub = threadIdx.x & 3;
    // threads past the table keep a valid cell: every lane stays for the barriers
    // and the quad exchanges, only the store is skipped
    const int4 c = cells[min(cell, n_cells - 1)];
    const CellGeom g = cell_geom<ARITY>(mesh + (int64_t)b * n_per, c, n_per);
    for (int i = threadIdx.x; i < n; i += 256) sx[i] = (float)i / (float)(n - 1);
    __syncthreads();
    // the largest exponent: the lattice point nearest the centre, per axis (a
    // NaN centre takes point 0 and then carries its NaN through every term)
    const float nf = (float)n, top = (float)(n - 1);
    const int jn = (int)fminf(fmaxf(rintf(g.cx * top), 0.0f), top);
    const int in = (int)fminf(fmaxf(rintf(g.cy * top), 0.0f), top);
    const float ddx = g.cx - sx[jn], ddy = g.cy - sx[in];
    const float smax = -nf * sqrtf(ddx * ddx + ddy * ddy);
    const float *mb = m + (int64_t)b * n * n;
    float z = 0.0f, zv = 0.0f;
    for (int r0 = 0; r0 < n; r0 += rows_per_tile) {
        const int nr = min(rows_per_tile, n - r0);
        if (r0) __syncthreads();  // the previous tile has been read
        for (int t = threadIdx.x; t < nr * n; t += 256) sm[t] = mb[r0 * n + t];
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            const float dy = g.cy - sx[r0 + r];
            const float dy2 = dy * dy;
            const float *row = sm + r * n;
            for (int j = sub; j < n; j += 4) {
                const float dx = g.cx - sx[j];
                const float e = __expf(-nf * sqrtf(dx * dx + dy2) - smax);
                z += e;
                zv += e * row[j];
            }
        }
    }
    z += xor_lane_f<1>(z);
    z += xor_lane_f<2>(z);
    zv += xor_lane_f<1>(zv);
    zv += xor_lane_f<2>(zv);
    if (sub == 0 && cell < n_cells) mg[(int64_t)b * n_cells + cell] = zv / z * g.area;
}

// One workgroup per trajectory: mean, unbiased std (two passes: the squares of
// the deviations from the mean), max - min of mg; the cells that are not
// positively oriented against the same cell of the fixed grid (signed area <= 0
// or NaN) and the smallest signed moved area / fixed area.  A NaN in mg makes
// the three statistics NaN, a NaN ratio makes area_ratio_min NaN.  Sums in
// thread-strided order, wave butterfly, the four waves in order; every output
// nullable, none read but inverted_total.
template <int ARITY>
__global__ __launch_bounds__(256) void cell_stats_kernel(const float *__restrict__ mg,
                                                         const float2 *__restrict__ mesh,
                                                         const float2 *__restrict__ xi,
                                                         const int4 *__restrict__ cells, int n_cells,
                                                         int n_per, mmpde_mesh_quality_io io) {
    __shared__ float s4[4], smn[4], smx[4], srt[4];
    __shared__ int scnt[4], snan[4];
    const int b = blockIdx.x;
    const float *v = mg + (int64_t)b * n_cells;
    const float2 *pts = mesh + (int64_t)b * n_per;
    float sum = 0.0f, mn = INFINITY, mx = -INFINITY, rt = INFINITY;
    int cnt = 0, nan = 0;  // nan bit 0: mg, bit 1: ratio
    for (int c = threadIdx.x; c < n_cells; c += 256) {
        const float x = v[c];
        sum += x;
        mn = fminf(mn, x);
        mx = fmaxf(mx, x);
        const int4 cc = cells[c];
        const float moved = cell_geom<ARITY>(pts, cc, n_per).sgn;
        const float fixed = cell_geom<ARITY>(xi, cc, n_per).sgn;
        const float ratio = moved / fixed;
        cnt += !((fixed < 0.0f ? -moved : moved) > 0.0f);
        rt = fminf(rt, ratio);
        nan |= (x != x ? 1 : 0) | (ratio != ratio ? 2 : 0);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        rt = fminf(rt, __shfl_xor(rt, o, 64));
        cnt += __shfl_xor(cnt, o, 64);
        nan |= __shfl_xor(nan, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        smn[w] = mn;
        smx[w] = mx;
        srt[w] = rt;
        scnt[w] = cnt;
        snan[w] = nan;
    }
    const float mean = block_sum_256(sum, s4) / (float)n_cells;  // its barriers publish the arrays above
    float ss = 0.0f;
    for (int c = threadIdx.x; c < n_cells; c += 256) {
        const float d = v[c] - mean;
        ss += d * d;
    }
    ss = block_sum_256(ss, s4);
    if (threadIdx.x == 0) {
        const float qnan = __builtin_nanf("");
        mn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
        mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
        rt = fminf(fminf(srt[0], srt[1]), fminf(srt[2], srt[3]));
        cnt = scnt[0] + scnt[1] + scnt[2] + scnt[3];
        nan = snan[0] | snan[1] | snan[2] | snan[3];
        if (io.mean) io.mean[b] = mean;
        if (io.std) io.std[b] = sqrtf(ss / (float)(n_cells - 1));  // one cell: 0 / 0, as torch.std
        if (io.range) io.range[b] = (nan & 1) ? qnan : mx - mn;
        if (io.inverted) io.inverted[b] = cnt;
        if (io.area_ratio_min) io.area_ratio_min[b] = (nan & 2) ? qnan : rt;
        if (io.inverted_total) io.inverted_total[b] += cnt;
    }
}

int64_t quality_ws_floats(int64_t batches, int64_t n_cells) { return (batches * n_cells + 3) & ~int64_t(3); }

template <int ARITY>
int launch_quality(const float *mesh, const float *xi, int64_t batches, int64_t n_per, const int32_t *cells,
                   int64_t n_cells, const float *m, int n, const mmpde_mesh_quality_io &io, float *mg,
                   hipStream_t st) {
    const int rpt = tile_rows(n);
    const size_t lds = (size_t)(((n + 3) & ~3) + rpt * n) * sizeof(float);
    const dim3 grid((unsigned)ceil_div(n_cells, kCellsPerBlock), (unsigned)batches);
    hipLaunchKernelGGL(cell_mg_kernel<ARITY>, grid, dim3(256), lds, st, (const float2 *)mesh,
                       (const int4 *)cells, (int)n_cells, (int)n_per, m, n, rpt, mg);
    MMPDE_RET_LAUNCH();
    hipLaunchKernelGGL(cell_stats_kernel<ARITY>, dim3((unsigned)batches), dim3(256), 0, st, mg,
                       (const float2 *)mesh, (const float2 *)xi, (const int4 *)cells, (int)n_cells,
                       (int)n_per, io);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

bool monitor_ok(const void *src, int64_t batches, int n, const void *m, const void *alpha, const void *rhs) {
    return src && m && alpha && rhs && batches >= 1 && batches <= INT32_MAX && n >= 2 &&
           n <= MMPDE_MESH_QUALITY_MAX_N;
}

}  // namespace

extern "C" int mmpde_mesh_monitor_array(const float *u, int64_t batches, int n, float *m_out,
                                        float *alpha_out, float *rhs_out, mmpde_stream_t stream) {
    MMPDE_REQUIRE(monitor_ok(u, batches, n, m_out, alpha_out, rhs_out));
    hipLaunchKernelGGL(monitor_kernel<false>, dim3((unsigned)batches), dim3(256), 0, as_stream(stream), u,
                       n, m_out, alpha_out, rhs_out);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

extern "C" int mmpde_mesh_monitor_grad(const float *grad, int64_t batches, int n, float *m_out,
                                       float *alpha_out, float *rhs_out, mmpde_stream_t stream) {
    MMPDE_REQUIRE(monitor_ok(grad, batches, n, m_out, alpha_out, rhs_out) && ((uintptr_t)grad & 7u) == 0);
    hipLaunchKernelGGL(monitor_kernel<true>, dim3((unsigned)batches), dim3(256), 0, as_stream(stream), grad,
                       n, m_out, alpha_out, rhs_out);
    MMPDE_RET_LAUNCH();
    return MMPDE_OK;
}

extern "C" int64_t mmpde_mesh_quality_workspace_bytes(int64_t batches, int64_t n_cells) {
    return batches >= 1 && n_cells >= 1 ? quality_ws_floats(batches, n_cells) * (int64_t)sizeof(float) : 0;
}

extern "C" int mmpde_mesh_quality(const float *mesh, const float *xi, int64_t batches, int64_t n_per,
                                  const int32_t *cells, int64_t n_cells, int arity, const float *m, int n,
                                  const mmpde_mesh_quality_io *io, void *workspace, mmpde_stream_t stream) {
    MMPDE_REQUIRE(mesh && xi && cells && m && io && (io->mg || workspace));
    MMPDE_REQUIRE(arity == 3 || arity == 4);
    MMPDE_REQUIRE(n_cells >= 1 && n_cells <= INT32_MAX && n >= 2 && n <= MMPDE_MESH_QUALITY_MAX_N);
    MMPDE_REQUIRE(n_per >= arity && n_per <= INT32_MAX && batches >= 1 && batches <= 65535);
    MMPDE_REQUIRE((((uintptr_t)mesh | (uintptr_t)xi) & 7u) == 0 && ((uintptr_t)cells & 15u) == 0);
    float *mg = io->mg ? io->mg : (float *)workspace;
    return arity == 4 ? launch_quality<4>(mesh, xi, batches, n_per, cells, n_cells, m, n, *io, mg,
                                          as_stream(stream))
                      : launch_quality<3>(mesh, xi, batches, n_per, cells, n_cells, m, n, *io, mg,
                                          as_stream(stream));
}
