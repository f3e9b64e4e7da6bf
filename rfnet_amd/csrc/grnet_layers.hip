// grnet_layers.hip -- the two GRNet layers that bring a voxel grid back to points: Gridding Reverse (a (b, R, R, R) occupancy
// volume -> one point per cell, as a padded batch with device counts) and Cubic Feature Sampling (the feature vectors at the
// eight vertices of every point's cell, from a (b, c, R, R, R) volume).  include/rfops.h states the contract, DESIGN.md 5.3m the
// layout and the measurements.  The geometry is gridding.hpp's; the sort and the scatter of the backward are brick_sort.hpp's.
//
//   cfs forward   the plain gather: a workgroup takes CFS_FWD_PTS points, their vertices go through LDS, and the threads run over
//                 the (point, corner, channel) elements of the output in memory order -- coalesced stores, strided plane reads.
//   cfs backward  no float atomics in memory and no memset: gr_brick_sort sorts the points by the brick (GR_E^3 vertices) of their
//                 cell, the record carrying the point index; one workgroup per (sample, sub-brick of GR_SUB_E^3 vertices, chunk
//                 of GR_CHUNK channels) runs gr_subbrick_scatter over the lists that can reach its vertices, a wave taking one
//                 record per step with a lane per (corner, channel) -- eight reads of GR_CHUNK contiguous floats of grad_feat --
//                 and adding into LDS doubles (ds_add_f64); every element of grad_vol is then stored once, zeros where nothing
//                 fell.  The order of the additions is the order of arrival: the contract says what that leaves open.
//   reverse       count the valid cells per tile of GV_TILE cells, scan the tile counts of a sample in one workgroup, write: the
//                 valid cells keep their cell order, so the placement is a pure function of the grid.  Three launches, no atomics.
//   reverse grad  a gather per vertex over its up to eight cells, in double.
#include "brick_sort.hpp"

namespace {

// ------------------------------------------------------------------------------------------------ cubic feature sampling
constexpr int CFS_FWD_PTS = 32, CFS_TPB = 256;

struct CfsFwd {
    int n, c;
    GrBox g;
    const float *xyz;
    const int *len;
    const unsigned *vol;  // the floats, moved as words: a copy keeps every bit
    unsigned *feat;
    int *inside;
};

// the first vertex of the point's cell, or -1 for a point outside the box
__device__ __forceinline__ int cfs_vertex(const float *__restrict__ x, const GrBox &g) {
    int ix, iy, iz;
    float tx, ty, tz;
    const bool in = gr_axis(x[0], g, ix, tx) & gr_axis(x[1], g, iy, ty) & gr_axis(x[2], g, iz, tz);
    return in ? (ix * g.R + iy) * g.R + iz : -1;
}

// grid (ceil(n / CFS_FWD_PTS), b)
__global__ __launch_bounds__(CFS_TPB) void cfs_gather_kernel(CfsFwd a) {
    __shared__ int vtx[CFS_FWD_PTS];
    __shared__ unsigned wcnt[CFS_TPB / 64];
    const int s = blockIdx.y, tid = threadIdx.x, n = a.n, c = a.c;
    const GrBox g = a.g;
    const int R = g.R, L = rf::ragged_count(a.len, s, n);
    const float *__restrict__ xyz = a.xyz + (size_t)s * n * 3;
    const int p0 = blockIdx.x * CFS_FWD_PTS;
    if (tid < CFS_FWD_PTS) {
        const int i = p0 + tid;
        vtx[tid] = i < L ? cfs_vertex(xyz + (size_t)i * 3, g) : -1;
    }
    if (blockIdx.x == 0) {  // the inside count of the sample
        unsigned cnt = 0;
        for (int i = tid; i < L; i += CFS_TPB) cnt += cfs_vertex(xyz + (size_t)i * 3, g) >= 0;
        cnt = rf::wave_add_u32(cnt);
        if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) a.inside[s] = (int)((wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]));
    const int np = n - p0 < CFS_FWD_PTS ? n - p0 : CFS_FWD_PTS, row = 8 * c, total = np * row;
    const size_t R3 = (size_t)R * R * R;
    const unsigned *__restrict__ vol = a.vol + (size_t)s * c * R3;
    unsigned *__restrict__ feat = a.feat + ((size_t)s * n + p0) * row;
    for (int e = tid; e < total; e += CFS_TPB) {
        const int p = e / row, k = e - p * row, d = k / c, ch = k - d * c;
        const int v = vtx[p];
        unsigned w = 0u;  // +0.0f
        if (v >= 0) w = vol[(size_t)ch * R3 + (size_t)(v + (((d >> 2) * R + ((d >> 1) & 1)) * R + (d & 1)))];
        feat[e] = w;
    }
}

// gr_brick_sort by the cell, the record carrying the point index.  grid (b)
__global__ __launch_bounds__(GR_BIN_TPB) void cfs_bin_kernel(GrSortCloud a) {
    const int s = blockIdx.x, n = a.n;
    const int L = rf::ragged_count(a.len, s, n);
    const float *__restrict__ xyz = a.xyz + (size_t)s * n * 3;
    const GrBox g = a.g;
    const int nb = gr_nb(g.R), nb3 = nb * nb * nb;
    unsigned *__restrict__ st = a.starts + (size_t)s * (nb3 + 1);
    unsigned long long *__restrict__ rec = a.recs + (size_t)s * n;
    gr_brick_sort(L, g.R, st, rec, nullptr, [&](int i, int &ix, int &iy, int &iz, unsigned long long &word) {
        float tx, ty, tz;
        const bool in = gr_axis(xyz[(size_t)i * 3], g, ix, tx) & gr_axis(xyz[(size_t)i * 3 + 1], g, iy, ty) &
                        gr_axis(xyz[(size_t)i * 3 + 2], g, iz, tz);
        word = gr_index_record(ix, iy, iz, i);
        return in;
    });
}

struct CfsBrick {
    int n, c, R;
    const unsigned *starts;
    const unsigned long long *recs;
    const float *gf;  // (b, n, 8, c)
    float *gv;        // (b, c, R, R, R)
};

// gr_subbrick_scatter of grad_feat's (corner, channel) elements.  grid (ceil(R / GR_SUB_E)^3 * ceil(c / GR_CHUNK), b), the channel
// chunk fastest
__global__ __launch_bounds__(GR_SUB_TPB) void cfs_brick_kernel(CfsBrick a) {
    const int s = blockIdx.y;
    const int R = a.R, c = a.c, n = a.n;
    const int nb = gr_nb(R), nb3 = nb * nb * nb;
    const size_t R3 = (size_t)R * R * R;
    const unsigned *__restrict__ st = a.starts + (size_t)s * (nb3 + 1);
    const unsigned long long *__restrict__ rec = a.recs + (size_t)s * n;
    const float *__restrict__ gf = a.gf + (size_t)s * n * 8 * c;
    gr_subbrick_scatter(blockIdx.x, R, c, st, rec, a.gv + (size_t)s * c * R3,
                        [&](int i, int d, int ch) { return (double)gf[((size_t)i * 8 + d) * c + ch]; });
}

// ------------------------------------------------------------------------------------------------ gridding reverse
constexpr int GV_TILE = 256, GV_TPB = GV_TILE, GV_SCAN_TPB = 1024;

// The sums of a cell, in the contract's order: S over the eight corners from w_0, T_a over the four corners with d_a = 1.
struct GvCell {
    double S, Tx, Ty, Tz;
};

__device__ __forceinline__ GvCell gv_cell(const float *__restrict__ g, int R, int ix, int iy, int iz) {
    double w[8];
#pragma unroll
    for (int d = 0; d < 8; d++) w[d] = (double)g[((size_t)(ix + (d >> 2)) * R + (iy + ((d >> 1) & 1))) * R + (iz + (d & 1))];
    GvCell c;
    c.S = ((((((w[0] + w[1]) + w[2]) + w[3]) + w[4]) + w[5]) + w[6]) + w[7];
    c.Tx = ((w[4] + w[5]) + w[6]) + w[7];
    c.Ty = ((w[2] + w[3]) + w[6]) + w[7];
    c.Tz = ((w[1] + w[3]) + w[5]) + w[7];
    return c;
}

__device__ __forceinline__ bool gv_valid(double S, float eps) { return S >= (double)eps && S < (double)INFINITY; }  // a NaN fails

struct Gv {
    int R, compact;
    float eps;
    double lo, h;  // (double)lo and h_d = ((double)hi - (double)lo) / (double)(R - 1)
    const float *grid;
    unsigned *tiles;  // (b, nt): the valid cells of every tile, then their exclusive prefix
    float *points;
    int *row, *count;
};

__device__ __forceinline__ void gv_split(int cell, int R, int &ix, int &iy, int &iz) {
    const int C = R - 1;
    iz = cell % C, iy = (cell / C) % C, ix = cell / (C * C);
}

// the valid cells of this thread's wave before this lane, and the wave's total
__device__ __forceinline__ unsigned gv_rank(bool valid, unsigned &total) {
    const unsigned long long m = __ballot(valid);
    total = (unsigned)__popcll(m);
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
}

// grid (nt, b)
__global__ __launch_bounds__(GV_TPB) void gv_count_kernel(Gv a) {
    __shared__ unsigned wtot[GV_TPB / 64];
    const int s = blockIdx.y, tid = threadIdx.x, R = a.R, C = R - 1, M = C * C * C;
    const int cell = blockIdx.x * GV_TILE + tid;
    bool valid = false;
    if (cell < M) {
        int ix, iy, iz;
        gv_split(cell, R, ix, iy, iz);
        valid = gv_valid(gv_cell(a.grid + (size_t)s * R * R * R, R, ix, iy, iz).S, a.eps);
    }
    unsigned total;
    gv_rank(valid, total);
    if ((tid & 63) == 0) wtot[tid >> 6] = total;
    __syncthreads();
    if (tid == 0) a.tiles[(size_t)s * gridDim.x + blockIdx.x] = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
}

// exclusive prefix of a sample's tile counts, in place, and the sample's count.  grid (b)
__global__ __launch_bounds__(GV_SCAN_TPB) void gv_scan_kernel(unsigned *tiles, int nt, int *count) {
    __shared__ unsigned wtot[GV_SCAN_TPB / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    unsigned *__restrict__ t = tiles + (size_t)s * nt;
    const int per = (nt + GV_SCAN_TPB - 1) / GV_SCAN_TPB, k0 = tid * per, k1 = k0 + per < nt ? k0 + per : nt;
    unsigned sum = 0;
    for (int k = k0; k < k1; k++) sum += t[k];
    const unsigned incl = rf::wave_incl_scan(sum);
    if ((tid & 63) == 63) wtot[tid >> 6] = incl;
    __syncthreads();
    unsigned run = incl - sum;
    for (int w = 0; w < (tid >> 6); w++) run += wtot[w];
    for (int k = k0; k < k1; k++) {
        const unsigned v = t[k];
        t[k] = run;
        run += v;
    }
    if (tid == GV_SCAN_TPB - 1) count[s] = (int)run;  // (the last thread's run ends at the total, whether or not it owns tiles)
}

// grid (nt, b)
__global__ __launch_bounds__(GV_TPB) void gv_write_kernel(Gv a) {
    __shared__ unsigned wtot[GV_TPB / 64];
    const int s = blockIdx.y, tid = threadIdx.x, R = a.R, C = R - 1, M = C * C * C;
    const int cell = blockIdx.x * GV_TILE + tid;
    bool valid = false;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (cell < M) {
        int ix, iy, iz;
        gv_split(cell, R, ix, iy, iz);
        const GvCell c = gv_cell(a.grid + (size_t)s * R * R * R, R, ix, iy, iz);
        valid = gv_valid(c.S, a.eps);
        if (valid) {
            px = (float)(a.lo + ((double)ix + c.Tx / c.S) * a.h);
            py = (float)(a.lo + ((double)iy + c.Ty / c.S) * a.h);
            pz = (float)(a.lo + ((double)iz + c.Tz / c.S) * a.h);
        }
    }
    unsigned total;
    unsigned rank = gv_rank(valid, total);
    if ((tid & 63) == 0) wtot[tid >> 6] = total;
    __syncthreads();
    if (cell >= M) return;
    float *__restrict__ pts = a.points + (size_t)s * M * 3;
    int *__restrict__ row = a.row + (size_t)s * M;
    if (!a.compact) {
        row[cell] = valid ? cell : -1;
        pts[(size_t)cell * 3] = px, pts[(size_t)cell * 3 + 1] = py, pts[(size_t)cell * 3 + 2] = pz;
        return;
    }
    for (int w = 0; w < (tid >> 6); w++) rank += wtot[w];
    const unsigned r = a.tiles[(size_t)s * gridDim.x + blockIdx.x] + rank;  // < the sample's count <= M for a valid cell
    row[cell] = valid ? (int)r : -1;
    if (valid) pts[(size_t)r * 3] = px, pts[(size_t)r * 3 + 1] = py, pts[(size_t)r * 3 + 2] = pz;
    // the rows from the count on belong to nobody: the thread of the cell with that number clears them
    if (cell >= a.count[s]) pts[(size_t)cell * 3] = 0.f, pts[(size_t)cell * 3 + 1] = 0.f, pts[(size_t)cell * 3 + 2] = 0.f;
}

struct GvGrad {
    int R;
    double h;
    const float *grid;
    const int *row;
    const float *gp;  // (b, M, 3)
    float *out;       // (b, R, R, R)
};

// grid (ceil(R^3 / GV_TPB), b): a thread per vertex
__global__ __launch_bounds__(GV_TPB) void gv_grad_kernel(GvGrad a) {
    const int s = blockIdx.y, R = a.R, C = R - 1, M = C * C * C, R3 = R * R * R;
    const int v = blockIdx.x * GV_TPB + threadIdx.x;
    if (v >= R3) return;
    const int z = v % R, y = (v / R) % R, x = v / (R * R);
    const float *__restrict__ g = a.grid + (size_t)s * R3;
    const int *__restrict__ row = a.row + (size_t)s * M;
    const float *__restrict__ gp = a.gp + (size_t)s * M * 3;
    double acc = 0.0;
#pragma unroll 1
    for (int d = 0; d < 8; d++) {
        const int dx = d >> 2, dy = (d >> 1) & 1, dz = d & 1;
        const int cx = x - dx, cy = y - dy, cz = z - dz;
        if (cx < 0 || cy < 0 || cz < 0 || cx >= C || cy >= C || cz >= C) continue;
        const int r = row[(cx * C + cy) * C + cz];
        if ((unsigned)r >= (unsigned)M) continue;  // an invalid cell; a corrupt entry never moves a load
        const GvCell c = gv_cell(g, R, cx, cy, cz);
        const double t0 = ((double)dx - c.Tx / c.S) * (double)gp[(size_t)r * 3];
        const double t1 = ((double)dy - c.Ty / c.S) * (double)gp[(size_t)r * 3 + 1];
        const double t2 = ((double)dz - c.Tz / c.S) * (double)gp[(size_t)r * 3 + 2];
        acc += (a.h / c.S) * ((t0 + t1) + t2);
    }
    a.out[(size_t)s * R3 + v] = (float)acc;
}

int gv_tiles(int res) {
    const long M = (long)(res - 1) * (res - 1) * (res - 1);
    return (int)((M + GV_TILE - 1) / GV_TILE);
}

bool gv_sizes_ok(int b, int res) { return b >= 1 && b <= 65535 && res >= 2 && res <= RF_GR_MAX_RES; }

}  // namespace

extern "C" {

int rf_cubic_feature_sampling(int b, int n, int c, int res, float lo, float hi, const float *xyz, const int *len, const float *vol,
                              float *feat, int *inside, rf_stream_t stream) {
    if (b < 0 || n < 0 || c < 0 || res < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!gr_sizes_ok(b, n, c, res)) return RF_EINVAL;
    if (!gr_box_ok(lo, hi)) return RF_EINVAL;
    if (!rf::tensors_ok({xyz, vol, feat, inside}, {len})) return RF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const CfsFwd a{n, c, gr_box(res, lo, hi), xyz, len, (const unsigned *)vol, (unsigned *)feat, inside};
    RF_LAUNCH("cfs_gather", cfs_gather_kernel, dim3(rf::ceil_div(n, CFS_FWD_PTS), b), dim3(CFS_TPB), 0, st, a);
    return RF_OK;
}

size_t rf_cubic_feature_sampling_grad_workspace_bytes(int b, int n, int res) {
    if (!gr_sizes_ok(b, n, res)) return 0;
    return gr_sort_layout(b, n, res).total;
}

int rf_cubic_feature_sampling_grad(int b, int n, int c, int res, float lo, float hi, const float *xyz, const int *len,
                                   const float *grad_feat, float *grad_vol, void *workspace, size_t workspace_bytes,
                                   rf_stream_t stream) {
    if (b < 0 || n < 0 || c < 0 || res < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!gr_sizes_ok(b, n, c, res)) return RF_EINVAL;
    if (!gr_box_ok(lo, hi)) return RF_EINVAL;
    if (!rf::tensors_ok({xyz, grad_feat, grad_vol}, {len}) || !rf::workspace_ok(workspace)) return RF_EINVAL;
    const GrSortLayout l = gr_sort_layout(b, n, res);
    if (workspace_bytes < l.total) return RF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;

    char *w = (char *)workspace;
    unsigned *starts = (unsigned *)(w + l.starts);
    unsigned long long *recs = (unsigned long long *)(w + l.recs);
    const GrSortCloud bin{n, gr_box(res, lo, hi), xyz, len, starts, recs};
    RF_LAUNCH("cfs_bin", cfs_bin_kernel, dim3(b), dim3(GR_BIN_TPB), 0, st, bin);
    const int nsb = rf::ceil_div(res, GR_SUB_E), nchunk = rf::ceil_div(c, GR_CHUNK);
    const CfsBrick br{n, c, res, starts, recs, grad_feat, grad_vol};
    RF_LAUNCH("cfs_brick", cfs_brick_kernel, dim3(nsb * nsb * nsb * nchunk, b), dim3(GR_SUB_TPB), 0, st, br);
    return RF_OK;
}

size_t rf_gridding_reverse_workspace_bytes(int b, int res) {
    if (!gv_sizes_ok(b, res)) return 0;
    return rf::align256((size_t)b * gv_tiles(res) * sizeof(unsigned));
}

int rf_gridding_reverse(int b, int res, float lo, float hi, float eps, int compact, const float *grid, float *points, int *row,
                        int *count, void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (b < 0 || res < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!gv_sizes_ok(b, res)) return RF_EINVAL;
    if (!gr_box_ok(lo, hi)) return RF_EINVAL;
    if (!(isfinite(eps) && eps > 0.f)) return RF_EINVAL;
    if (compact != 0 && compact != 1) return RF_EINVAL;
    if (!rf::tensors_ok({grid, points, row, count}) || !rf::workspace_ok(workspace)) return RF_EINVAL;
    if (workspace_bytes < rf_gridding_reverse_workspace_bytes(b, res)) return RF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;

    const int nt = gv_tiles(res);
    unsigned *tiles = (unsigned *)workspace;
    const double h = ((double)hi - (double)lo) / (double)(res - 1);
    const Gv a{res, compact, eps, (double)lo, h, grid, tiles, points, row, count};
    RF_LAUNCH("gridding_reverse_count", gv_count_kernel, dim3(nt, b), dim3(GV_TPB), 0, st, a);
    RF_LAUNCH("gridding_reverse_scan", gv_scan_kernel, dim3(b), dim3(GV_SCAN_TPB), 0, st, tiles, nt, count);
    RF_LAUNCH("gridding_reverse_write", gv_write_kernel, dim3(nt, b), dim3(GV_TPB), 0, st, a);
    return RF_OK;
}

int rf_gridding_reverse_grad(int b, int res, float lo, float hi, const float *grid, const int *row, const float *grad_points,
                             float *grad_grid, rf_stream_t stream) {
    if (b < 0 || res < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!gv_sizes_ok(b, res)) return RF_EINVAL;
    if (!gr_box_ok(lo, hi)) return RF_EINVAL;
    if (!rf::tensors_ok({grid, row, grad_points, grad_grid})) return RF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const double h = ((double)hi - (double)lo) / (double)(res - 1);
    const GvGrad a{res, h, grid, row, grad_points, grad_grid};
    RF_LAUNCH("gridding_reverse_grad", gv_grad_kernel, dim3(rf::ceil_div((long)res * res * res, GV_TPB), b), dim3(GV_TPB), 0, st, a);
    return RF_OK;
}

}  // extern "C"
