// gridding.hip -- GRNet's Gridding layer and Gridding loss: every point spreads its mass trilinearly over the eight vertices of
// its cell of a regular R^3 grid; the loss is the L1 difference of two such grids.  include/rfops.h states the contract,
// DESIGN.md 5.3l the layout and the measurements.
//
//   exact    the per-axis weight is quantised to RF_GR_Q = 512 steps (q0 + q1 = 512), a vertex weight is the INTEGER
//            W = qx qy qz <= 2^27 and every grid value an integer sum: no order of arrival can change a bit.
//   overflow G(v) <= 65536 points * 2^27 = 2^43.  D(v) = mu1 G1(v) - mu2 G2(v) with mu <= 65536 (the other cloud's count in
//            DENSITY mode): |D(v)| <= 2^16 * 2^16 * 2^27 = 2^59.  sum_v |D(v)| <= mu1 sum G1 + mu2 sum G2
//            <= 2 * 2^16 * 2^16 * 2^27 = 2^60: everything fits an int64 with three bits to spare.
//   bin      one workgroup per (sample, cloud) sorts the inside points by the brick (GR_E^3 vertices) of their cell: an LDS
//            histogram, a scan, a scatter through LDS cursors.  A record is one 64-bit word: the cell (3 x 8 bits) and the three
//            q1 (3 x 10 bits).  The order inside a brick's list depends on arrival; nothing reads it -- every consumer adds
//            integers.
//   brick    one workgroup per (sample, brick).  A brick's vertices receive from the cells of its own brick and of its up to
//            seven lower neighbours, so it walks at most 8 lists per cloud and keeps what lands in its own vertex range: cloud 1
//            adds +mu1 W, cloud 2 adds -mu2 W into the same int64 LDS word (ds_add_u64, two's complement).  The difference grid
//            exists only there.  A brick whose lists are all empty leaves before it clears any LDS.  Epilogue: sum |D| over the
//            brick as one int64 partial (a plain store), and with gradients sign(D) as one byte per vertex; the Gridding layer
//            is the same kernel writing the float grid instead.
//   finish   adds the brick partials (integers: any order) and rounds the loss once; per point gathers the eight signs and
//            forms both gradients in double.  Only bricks that hold a point's vertices are read, and those are never empty.
//
// No float atomics, no hipMemset, no sum whose order is left open.  Every loop bound is a count or a list length that the bin
// kernel derived from counts; a non-finite coordinate fails the inside test and never moves a memory access.
#include "brick_sort.hpp"  // gr_brick_sort and the sort's constants and layout; gridding.hpp's GrBox, gr_axis, gr_nb, GR_E

namespace {

constexpr int GR_E3 = GR_E * GR_E * GR_E;
constexpr int GR_BRICK_TPB = 256, GR_PT_TPB = 256;
constexpr double GR_Q3 = 134217728.0;    // RF_GR_Q^3
static_assert(RF_GR_Q == 512, "a record holds three q1 of 10 bits");

__device__ __forceinline__ unsigned gr_q1(float t) { return (unsigned)(int)rintf(t * 512.0f); }

// ------------------------------------------------------------------------------------------------ bin
struct GrBin {
    int n, m, clouds;  // clouds: 2 (the loss) or 1 (the layer; m = 0)
    GrBox g;
    const float *xyz1, *xyz2;
    const int *len1, *len2;
    unsigned *starts;            // (b, clouds, nb^3 + 1): where every brick's list begins; the last entry is the inside count
    unsigned long long *recs;    // (b, n + m): cloud 1's lists, then cloud 2's
    int *inside;                 // (b, clouds)
};

// gr_brick_sort by the cell, the record carrying the three q1.  grid (clouds, b)
__global__ __launch_bounds__(GR_BIN_TPB) void gr_bin_kernel(GrBin a) {
    const int cloud = blockIdx.x, s = blockIdx.y;
    const int np = cloud ? a.m : a.n;
    const int L = rf::ragged_count(cloud ? a.len2 : a.len1, s, np);
    const float *__restrict__ xyz = (cloud ? a.xyz2 : a.xyz1) + (size_t)s * np * 3;
    const GrBox g = a.g;
    const int nb = gr_nb(g.R), nb3 = nb * nb * nb;
    unsigned *__restrict__ st = a.starts + ((size_t)s * a.clouds + cloud) * (nb3 + 1);
    unsigned long long *__restrict__ rec = a.recs + (size_t)s * ((size_t)a.n + a.m) + (cloud ? a.n : 0);
    int *inside = a.inside + ((size_t)s * a.clouds + cloud);
    gr_brick_sort(L, g.R, st, rec, inside, [&](int i, int &ix, int &iy, int &iz, unsigned long long &word) {
        float tx, ty, tz;
        const bool in = gr_axis(xyz[(size_t)i * 3], g, ix, tx) & gr_axis(xyz[(size_t)i * 3 + 1], g, iy, ty) &
                        gr_axis(xyz[(size_t)i * 3 + 2], g, iz, tz);
        const unsigned lo = (unsigned)ix | (unsigned)iy << 8 | (unsigned)iz << 16 | gr_q1(tx) << 24;  // (q1x: bits 24 .. 33)
        const unsigned long long hi = (unsigned long long)(gr_q1(tx) >> 8) | (unsigned long long)gr_q1(ty) << 2 |
                                      (unsigned long long)gr_q1(tz) << 12;
        word = (unsigned long long)lo | hi << 32;
        return in;
    });
}

// ------------------------------------------------------------------------------------------------ brick
struct GrBrick {
    int n, m, R, mode;
    const int *len1, *len2;
    const unsigned *starts;
    const unsigned long long *recs;
    long long *partial;   // (b, nb^3)            OUT 0, 1
    signed char *sign;    // (b, R, R, R)         OUT 1
    float *grid;          // (b, R, R, R)         OUT 2
};

// OUT 0: the loss's partial; 1: and sign(D) per vertex; 2: the float grid of one cloud.  grid (nb^3, b)
template <int OUT>
__global__ __launch_bounds__(GR_BRICK_TPB) void gr_brick_kernel(GrBrick a) {
    __shared__ long long acc[GR_E3];
    __shared__ long long wsum[GR_BRICK_TPB / 64];
    constexpr int NC = OUT == 2 ? 1 : 2;
    const int br = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int R = a.R, nb = gr_nb(R), nb3 = nb * nb * nb;
    const int bz = br % nb, by = (br / nb) % nb, bx = br / (nb * nb);
    const unsigned *__restrict__ st = a.starts + (size_t)s * NC * (nb3 + 1);
    const size_t vbase = (size_t)s * R * R * R;

    unsigned any = 0;
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int d = 0; d < 8; d++) {
            const int nx = bx - (d >> 2), ny = by - ((d >> 1) & 1), nz = bz - (d & 1);
            if (nx < 0 || ny < 0 || nz < 0) continue;
            const int q = (nx * nb + ny) * nb + nz;
            any |= st[c * (nb3 + 1) + q + 1] - st[c * (nb3 + 1) + q];
        }
    if (!any) {  // nothing can land here (uniform over the workgroup)
        if (OUT == 2) {
            for (int l = tid; l < GR_E3; l += GR_BRICK_TPB) {
                const int gx = bx * GR_E + (l >> 8), gy = by * GR_E + ((l >> 4) & 15), gz = bz * GR_E + (l & 15);
                if (gx < R && gy < R && gz < R) a.grid[vbase + ((size_t)gx * R + gy) * R + gz] = 0.f;
            }
        } else if (tid == 0) {
            a.partial[(size_t)s * nb3 + br] = 0;
        }
        return;
    }

    for (int l = tid; l < GR_E3; l += GR_BRICK_TPB) acc[l] = 0;
    __syncthreads();
    int mu[2] = {1, -1};
    if (OUT != 2 && a.mode == RF_GR_DENSITY) {
        mu[0] = rf::ragged_count(a.len2, s, a.m);
        mu[1] = -rf::ragged_count(a.len1, s, a.n);
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const unsigned long long *__restrict__ rec = a.recs + (size_t)s * ((size_t)a.n + a.m) + (c ? a.n : 0);
        const int mult = mu[c];
#pragma unroll 1
        for (int d = 0; d < 8; d++) {
            const int nx = bx - (d >> 2), ny = by - ((d >> 1) & 1), nz = bz - (d & 1);
            if (nx < 0 || ny < 0 || nz < 0) continue;
            const int q = (nx * nb + ny) * nb + nz;
            const unsigned lo = st[c * (nb3 + 1) + q], hi = st[c * (nb3 + 1) + q + 1];
            for (unsigned r = lo + tid; r < hi; r += GR_BRICK_TPB) {
                const unsigned long long w = rec[r];
                const unsigned wl = (unsigned)w, wh = (unsigned)(w >> 32);
                // the cell relative to this brick's first vertex: -1 ... 15 per axis
                const int cx = (int)(wl & 255u) - bx * GR_E, cy = (int)((wl >> 8) & 255u) - by * GR_E,
                          cz = (int)((wl >> 16) & 255u) - bz * GR_E;
                const int q1x = (int)((wl >> 24) | (wh & 3u) << 8), q1y = (int)((wh >> 2) & 1023u), q1z = (int)((wh >> 12) & 1023u);
                const int qx[2] = {RF_GR_Q - q1x, q1x}, qy[2] = {RF_GR_Q - q1y, q1y}, qz[2] = {RF_GR_Q - q1z, q1z};
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const int ex = e >> 2, ey = (e >> 1) & 1, ez = e & 1;
                    const int lx = cx + ex, ly = cy + ey, lz = cz + ez;
                    const int W = qx[ex] * qy[ey] * qz[ez];
                    if ((unsigned)lx < (unsigned)GR_E && (unsigned)ly < (unsigned)GR_E && (unsigned)lz < (unsigned)GR_E && W != 0)
                        atomicAdd((unsigned long long *)&acc[(lx * GR_E + ly) * GR_E + lz],
                                  (unsigned long long)((long long)W * (long long)mult));  // one 32 x 32 -> 64 multiply per pair
                }
            }
        }
    }
    __syncthreads();
    long long sabs = 0;
    for (int l = tid; l < GR_E3; l += GR_BRICK_TPB) {
        const long long D = acc[l];
        const int gx = bx * GR_E + (l >> 8), gy = by * GR_E + ((l >> 4) & 15), gz = bz * GR_E + (l & 15);
        const bool in = gx < R && gy < R && gz < R;  // (words past the grid's end stayed 0)
        if (OUT < 2) sabs += D < 0 ? -D : D;
        if (OUT == 1 && in) a.sign[vbase + ((size_t)gx * R + gy) * R + gz] = (signed char)((D > 0) - (D < 0));
        if (OUT == 2 && in) a.grid[vbase + ((size_t)gx * R + gy) * R + gz] = (float)((double)D / GR_Q3);
    }
    if (OUT < 2) {
        sabs = rf::wave_sum(sabs);
        if ((tid & 63) == 0) wsum[tid >> 6] = sabs;
        __syncthreads();
        if (tid == 0) a.partial[(size_t)s * nb3 + br] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    }
}

// ------------------------------------------------------------------------------------------------ gather
// sum_{d = 0..7, dz fastest} val(v + d) sigma_a(d) prod_{k != a} w_k(d_k) for the three axes a, in double, from +0
template <class F>
__device__ __forceinline__ void gr_gather(int ix, int iy, int iz, float tx, float ty, float tz, int R, F val, double &ax, double &ay,
                                          double &az) {
    const double wx[2] = {(double)(1.0f - tx), (double)tx}, wy[2] = {(double)(1.0f - ty), (double)ty},
                 wz[2] = {(double)(1.0f - tz), (double)tz};
    ax = 0.0, ay = 0.0, az = 0.0;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        const int dx = d >> 2, dy = (d >> 1) & 1, dz = d & 1;
        const double v = val(((size_t)(ix + dx) * R + (iy + dy)) * R + (iz + dz));
        ax += (dx ? v : -v) * (wy[dy] * wz[dz]);
        ay += (dy ? v : -v) * (wx[dx] * wz[dz]);
        az += (dz ? v : -v) * (wx[dx] * wy[dy]);
    }
}

struct GrFin {
    int n, m, mode;
    GrBox g;
    const float *xyz1, *xyz2;
    const int *len1, *len2;
    const long long *partial;
    const signed char *sign;
    float *loss, *grad1, *grad2;
};

// grid (1, b) for the loss alone, (ceil((n + m) / GR_PT_TPB), b) with gradients: a thread per point, cloud 1's first
__global__ __launch_bounds__(GR_PT_TPB) void gr_finish_kernel(GrFin a) {
    __shared__ long long wsum[GR_PT_TPB / 64];
    const int s = blockIdx.y, tid = threadIdx.x, n = a.n, m = a.m;
    const GrBox g = a.g;
    const int R = g.R, nb = gr_nb(R), nb3 = nb * nb * nb;
    const int L1 = rf::ragged_count(a.len1, s, n), L2 = rf::ragged_count(a.len2, s, m);
    const double r3 = (double)R * (double)R * (double)R;
    if (blockIdx.x == 0) {
        long long t = 0;
        for (int k = tid; k < nb3; k += GR_PT_TPB) t += a.partial[(size_t)s * nb3 + k];
        t = rf::wave_sum(t);
        if ((tid & 63) == 0) wsum[tid >> 6] = t;
        __syncthreads();
        if (tid == 0) {
            const long long S = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
            const double den = a.mode == RF_GR_DENSITY ? (double)L1 * (double)L2 : r3;
            a.loss[s] = (float)((double)S / GR_Q3 / den);
        }
    }
    if (!a.grad1) return;
    const int p = blockIdx.x * GR_PT_TPB + tid;
    if (p >= n + m) return;
    const bool second = p >= n;
    const int i = second ? p - n : p, L = second ? L2 : L1;
    const float *__restrict__ x = (second ? a.xyz2 + (size_t)s * m * 3 : a.xyz1 + (size_t)s * n * 3) + (size_t)i * 3;
    float *__restrict__ out = (second ? a.grad2 + (size_t)s * m * 3 : a.grad1 + (size_t)s * n * 3) + (size_t)i * 3;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (i < L) {
        int ix, iy, iz;
        float tx, ty, tz;
        const bool in = gr_axis(x[0], g, ix, tx) & gr_axis(x[1], g, iy, ty) & gr_axis(x[2], g, iz, tz);
        if (in) {
            const signed char *__restrict__ sg = a.sign + (size_t)s * R * R * R;
            double ax, ay, az;
            if (second)
                gr_gather(ix, iy, iz, tx, ty, tz, R, [&](size_t v) { return -(double)(int)sg[v]; }, ax, ay, az);
            else
                gr_gather(ix, iy, iz, tx, ty, tz, R, [&](size_t v) { return (double)(int)sg[v]; }, ax, ay, az);
            const double c = a.mode == RF_GR_DENSITY ? 1.0 / (double)L : 1.0 / r3;
            const double f = (double)g.inv_h * c;
            g0 = (float)(ax * f), g1 = (float)(ay * f), g2 = (float)(az * f);
        }
    }
    out[0] = g0, out[1] = g1, out[2] = g2;
}

struct GrLayerGrad {
    int n;
    GrBox g;
    const float *xyz;
    const int *len;
    const float *gg;
    float *out;
};

// grid (ceil(n / GR_PT_TPB), b)
__global__ __launch_bounds__(GR_PT_TPB) void gr_layer_grad_kernel(GrLayerGrad a) {
    const int s = blockIdx.y, i = blockIdx.x * GR_PT_TPB + threadIdx.x, n = a.n;
    if (i >= n) return;
    const GrBox g = a.g;
    const int R = g.R, L = rf::ragged_count(a.len, s, n);
    const float *__restrict__ x = a.xyz + ((size_t)s * n + i) * 3;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (i < L) {
        int ix, iy, iz;
        float tx, ty, tz;
        const bool in = gr_axis(x[0], g, ix, tx) & gr_axis(x[1], g, iy, ty) & gr_axis(x[2], g, iz, tz);
        if (in) {
            const float *__restrict__ gg = a.gg + (size_t)s * R * R * R;
            double ax, ay, az;
            gr_gather(ix, iy, iz, tx, ty, tz, R, [&](size_t v) { return (double)gg[v]; }, ax, ay, az);
            g0 = (float)((double)g.inv_h * ax), g1 = (float)((double)g.inv_h * ay), g2 = (float)((double)g.inv_h * az);
        }
    }
    float *__restrict__ out = a.out + ((size_t)s * n + i) * 3;
    out[0] = g0, out[1] = g1, out[2] = g2;
}

// ------------------------------------------------------------------------------------------------ host
struct GrLayout {
    size_t starts, recs, partial, sign, total;
};

// clouds 2: the loss (partials, and the sign grid with gradients); clouds 1: the layer (m = 0, neither)
GrLayout gr_layout(int b, int n, int m, int res, int clouds, bool want_grad) {
    const size_t nb = gr_nb(res), nb3 = nb * nb * nb;
    const GrSortLayout sort = gr_sort_layout((size_t)b * clouds, (size_t)b * ((size_t)n + (size_t)m), res);
    GrLayout l;
    l.starts = sort.starts;
    l.recs = sort.recs;
    l.partial = sort.total;
    l.sign = l.partial + (clouds == 2 ? rf::align256((size_t)b * nb3 * sizeof(long long)) : 0);
    l.total = l.sign + (clouds == 2 && want_grad ? rf::align256((size_t)b * res * res * res) : 0);
    return l;
}

}  // namespace

extern "C" {

size_t rf_gridding_loss_workspace_bytes(int b, int n, int m, int res, int want_grad) {
    if (!gr_sizes_ok(b, n, res) || !gr_sizes_ok(b, m, res)) return 0;
    return gr_layout(b, n, m, res, 2, want_grad != 0).total;
}

int rf_gridding_loss(int b, int n, int m, int res, float lo, float hi, int mode, const float *xyz1, const float *xyz2,
                     const int *len1, const int *len2, float *loss, int *inside, float *grad1, float *grad2, void *workspace,
                     size_t workspace_bytes, rf_stream_t stream) {
    if (b < 0 || n < 0 || m < 0 || res < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!gr_sizes_ok(b, n, res) || !gr_sizes_ok(b, m, res)) return RF_EINVAL;
    if (!gr_box_ok(lo, hi)) return RF_EINVAL;
    if (mode != RF_GR_COUNTS && mode != RF_GR_DENSITY) return RF_EINVAL;
    if (!rf::tensors_ok({xyz1, xyz2, loss, inside}, {grad1, grad2, len1, len2})) return RF_EINVAL;
    if ((grad1 == nullptr) != (grad2 == nullptr) || !rf::workspace_ok(workspace)) return RF_EINVAL;
    const bool grad = grad1 != nullptr;
    const GrLayout l = gr_layout(b, n, m, res, 2, grad);
    if (workspace_bytes < l.total) return RF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;

    char *w = (char *)workspace;
    unsigned *starts = (unsigned *)(w + l.starts);
    unsigned long long *recs = (unsigned long long *)(w + l.recs);
    long long *partial = (long long *)(w + l.partial);
    signed char *sign = grad ? (signed char *)(w + l.sign) : nullptr;
    const GrBox g = gr_box(res, lo, hi);
    const int nb = gr_nb(res), nb3 = nb * nb * nb;

    const GrBin bin{n, m, 2, g, xyz1, xyz2, len1, len2, starts, recs, inside};
    RF_LAUNCH("gridding_bin", gr_bin_kernel, dim3(2, b), dim3(GR_BIN_TPB), 0, st, bin);
    const GrBrick br{n, m, res, mode, len1, len2, starts, recs, partial, sign, nullptr};
    if (grad) {
        RF_LAUNCH("gridding_brick", gr_brick_kernel<1>, dim3(nb3, b), dim3(GR_BRICK_TPB), 0, st, br);
    } else {
        RF_LAUNCH("gridding_brick", gr_brick_kernel<0>, dim3(nb3, b), dim3(GR_BRICK_TPB), 0, st, br);
    }
    const GrFin fin{n, m, mode, g, xyz1, xyz2, len1, len2, partial, sign, loss, grad1, grad2};
    const int fx = grad ? rf::ceil_div((long)n + m, GR_PT_TPB) : 1;
    RF_LAUNCH("gridding_finish", gr_finish_kernel, dim3(fx, b), dim3(GR_PT_TPB), 0, st, fin);
    return RF_OK;
}

size_t rf_gridding_workspace_bytes(int b, int n, int res) {
    if (!gr_sizes_ok(b, n, res)) return 0;
    return gr_layout(b, n, 0, res, 1, false).total;
}

int rf_gridding(int b, int n, int res, float lo, float hi, const float *xyz, const int *len, float *grid, int *inside,
                void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (b < 0 || n < 0 || res < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!gr_sizes_ok(b, n, res)) return RF_EINVAL;
    if (!gr_box_ok(lo, hi)) return RF_EINVAL;
    if (!rf::tensors_ok({xyz, grid, inside}, {len}) || !rf::workspace_ok(workspace)) return RF_EINVAL;
    const GrLayout l = gr_layout(b, n, 0, res, 1, false);
    if (workspace_bytes < l.total) return RF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;

    char *w = (char *)workspace;
    unsigned *starts = (unsigned *)(w + l.starts);
    unsigned long long *recs = (unsigned long long *)(w + l.recs);
    const GrBox g = gr_box(res, lo, hi);
    const int nb = gr_nb(res), nb3 = nb * nb * nb;
    const GrBin bin{n, 0, 1, g, xyz, nullptr, len, nullptr, starts, recs, inside};
    RF_LAUNCH("gridding_bin", gr_bin_kernel, dim3(1, b), dim3(GR_BIN_TPB), 0, st, bin);
    const GrBrick br{n, 0, res, RF_GR_COUNTS, len, nullptr, starts, recs, nullptr, nullptr, grid};
    RF_LAUNCH("gridding_brick", gr_brick_kernel<2>, dim3(nb3, b), dim3(GR_BRICK_TPB), 0, st, br);
    return RF_OK;
}

int rf_gridding_grad(int b, int n, int res, float lo, float hi, const float *xyz, const int *len, const float *grad_grid,
                     float *grad_xyz, rf_stream_t stream) {
    if (b < 0 || n < 0 || res < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!gr_sizes_ok(b, n, res)) return RF_EINVAL;
    if (!gr_box_ok(lo, hi)) return RF_EINVAL;
    if (!rf::tensors_ok({xyz, grad_grid, grad_xyz}, {len})) return RF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const GrLayerGrad a{n, gr_box(res, lo, hi), xyz, len, grad_grid, grad_xyz};
    RF_LAUNCH("gridding_grad", gr_layer_grad_kernel, dim3(rf::ceil_div(n, GR_PT_TPB), b), dim3(GR_PT_TPB), 0, st, a);
    return RF_OK;
}

}  // extern "C"
