// point_voxel.hip -- the point-voxel pair of PVCNN-style networks: average voxelization (per-point feature vectors averaged into
// the voxel nearest to each point) and trilinear devoxelization (a (b, c, R, R, R) feature volume interpolated back at every
// point), both with gradients.  include/rfops.h states the contract, DESIGN.md 5.3o the layout and the measurements.  The geometry
// is gridding.hpp's, shared with gridding.hip and grnet_layers.hip; the lattice points of PVCNN's voxel grid are its vertices.
//
//   voxelize        no float atomics in memory and no memset: the inside points are counting-sorted by the brick (GR_E^3
//                   vertices) of their NEAREST vertex, the record carrying that vertex and the point index; one workgroup per
//                   (sample, sub-brick of GR_SUB_E^3 vertices, chunk of GR_CHUNK channels) walks its own brick's list only, compacts
//                   the records of its sub-brick through LDS, and a wave then takes eight of them per step with a lane per
//                   (record, channel) -- eight reads of GR_CHUNK contiguous floats of feat -- adding into LDS doubles and LDS
//                   integer counts; every element of vol is stored once as sum / count, the chunk-0 workgroup stores cnt.
//   voxelize grad   the plain gather: grad_vol[ch][k_i] / cnt[k_i], k_i recomputed from xyz.
//   devoxelize      the plain gather, cfs_gather_kernel's shape: a workgroup takes PV_PTS points, cell and t go through LDS, the
//                   threads run over the (point, channel) elements of the output in memory order; eight plane reads, a double sum.
//   devoxelize grad grad_vol is gr_subbrick_scatter's walk of up to eight lists over a sort by the brick of the CELL, a record per
//                   step with a lane per (corner, channel), the weight recomputed from xyz[i] and one read of grad_feat[i][ch];
//                   grad_xyz is a gather with eight lanes per point, lane d summing g_d over the channels in ascending order.
//
// Every kernel with a (tile, sample) grid takes its logical place from rf::place_2d (lane_rows.hpp): the workgroups of one sample --
// which read the same volume, and in the scatter kernels the chunk workgroups of one sub-brick, which read the same rows of
// features -- share one XCD's L2 (profiles/point_voxel_ab.txt).
// Both sorts are brick_sort.hpp's gr_brick_sort, the one that grnet_layers.hip runs, with the vertex or the cell as the key; the
// devoxelize backward's scatter is its gr_subbrick_scatter, placed by rf::place_2d.
#include "brick_sort.hpp"
#include "lane_rows.hpp"

namespace {

constexpr int PV_TPB = 256, PV_PTS = 32;

struct PvPoint {
    int ix, iy, iz;  // the cell
    float tx, ty, tz;
};

// the point's cell and t, false for a point outside the box (its fields are then not to be used)
__device__ __forceinline__ bool pv_point(const float *__restrict__ x, const GrBox &g, PvPoint &p) {
    const bool inx = gr_axis(x[0], g, p.ix, p.tx), iny = gr_axis(x[1], g, p.iy, p.ty), inz = gr_axis(x[2], g, p.iz, p.tz);
    return inx & iny & inz;
}

// the nearest vertex: i + (t >= 0.5f), in 0 ... R - 1 because i <= R - 2
__device__ __forceinline__ void pv_nearest(const PvPoint &p, int &kx, int &ky, int &kz) {
    kx = p.ix + (p.tx >= 0.5f ? 1 : 0), ky = p.iy + (p.ty >= 0.5f ? 1 : 0), kz = p.iz + (p.tz >= 0.5f ? 1 : 0);
}

// W_d = ((double)w_x(d_x) * (double)w_y(d_y)) * (double)w_z(d_z) with w(0) = 1.0f - t and w(1) = t in fp32
__device__ __forceinline__ double pv_weight(const PvPoint &p, int dx, int dy, int dz) {
    const float wx = dx ? p.tx : 1.0f - p.tx, wy = dy ? p.ty : 1.0f - p.ty, wz = dz ? p.tz : 1.0f - p.tz;
    return ((double)wx * (double)wy) * (double)wz;
}

// ------------------------------------------------------------------------------------------------ the counting sort
// gr_brick_sort, the record carrying the point index; the key is the cell, or with NEAREST the nearest vertex.  grid (b)
template <bool NEAREST>
__global__ __launch_bounds__(GR_BIN_TPB) void pv_bin_kernel(GrSortCloud a) {
    const int s = blockIdx.x, n = a.n;
    const int L = rf::ragged_count(a.len, s, n);
    const float *__restrict__ xyz = a.xyz + (size_t)s * n * 3;
    const GrBox g = a.g;
    const int nb = gr_nb(g.R), nb3 = nb * nb * nb;
    unsigned *__restrict__ st = a.starts + (size_t)s * (nb3 + 1);
    unsigned long long *__restrict__ rec = a.recs + (size_t)s * n;
    gr_brick_sort(L, g.R, st, rec, nullptr, [&](int i, int &kx, int &ky, int &kz, unsigned long long &word) {
        PvPoint p;
        const bool in = pv_point(xyz + (size_t)i * 3, g, p);
        if (NEAREST)
            pv_nearest(p, kx, ky, kz);
        else
            kx = p.ix, ky = p.iy, kz = p.iz;
        word = gr_index_record(kx, ky, kz, i);
        return in;
    });
}

// ------------------------------------------------------------------------------------------------ average voxelization
struct PvVox {
    int n, c, R;
    const unsigned *starts;
    const unsigned long long *recs;
    const float *feat;  // (b, n, c)
    float *vol;         // (b, c, R, R, R)
    int *cnt;           // (b, R, R, R)
    int *inside;        // (b)
};

// grid (ceil(R / GR_SUB_E)^3 * ceil(c / GR_CHUNK), b), the channel chunk fastest
__global__ __launch_bounds__(PV_TPB) void pv_vox_kernel(PvVox a) {
    __shared__ double acc[GR_SUB_E3 * GR_CHUNK];  // [vertex][channel]
    __shared__ unsigned num[GR_SUB_E3];
    __shared__ unsigned slot[PV_TPB];  // a wave's 64: the records of this sub-brick among the 64 it has just read
    int s, bx;
    rf::place_2d<false>(bx, s);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = a.R, c = a.c, n = a.n;
    const int nsb = (R + GR_SUB_E - 1) / GR_SUB_E, nchunk = (c + GR_CHUNK - 1) / GR_CHUNK;
    const int nb = gr_nb(R), nb3 = nb * nb * nb;
    const int sbi = bx / nchunk, ch0 = (bx - sbi * nchunk) * GR_CHUNK;
    const int sz = sbi % nsb, sy = (sbi / nsb) % nsb, sx = sbi / (nsb * nsb);
    const unsigned *__restrict__ st = a.starts + (size_t)s * (nb3 + 1);
    const size_t R3 = (size_t)R * R * R;
    if (bx == 0 && tid == 0) a.inside[s] = (int)st[nb3];

    // the key of the sort is the vertex: the records that reach this sub-brick are in its own brick's list
    const int q = ((sx >> 1) * nb + (sy >> 1)) * nb + (sz >> 1);
    const unsigned lo = st[q], hi = st[q + 1];
    const bool any = hi > lo;  // (uniform over the workgroup)
    if (any) {
        for (int l = tid; l < GR_SUB_E3 * GR_CHUNK; l += PV_TPB) acc[l] = 0.0;
        for (int l = tid; l < GR_SUB_E3; l += PV_TPB) num[l] = 0u;
        __syncthreads();
        const unsigned long long *__restrict__ rec = a.recs + (size_t)s * n;
        const float *__restrict__ feat = a.feat + (size_t)s * n * c;
        const int grp = lane >> 3, ch = lane & 7;
        const bool chok = ch0 + ch < c;
        unsigned *__restrict__ mine = slot + wave * 64;
        for (unsigned r0 = lo + wave * 64; r0 < hi; r0 += PV_TPB) {  // uniform over the wave
            const unsigned r = r0 + lane;
            const unsigned long long w = r < hi ? rec[r] : 0ull;
            const int lx = (int)((unsigned)w & 255u) - sx * GR_SUB_E, ly = (int)((unsigned)(w >> 8) & 255u) - sy * GR_SUB_E,
                      lz = (int)((unsigned)(w >> 16) & 255u) - sz * GR_SUB_E;
            const bool keep = r < hi && (unsigned)lx < (unsigned)GR_SUB_E && (unsigned)ly < (unsigned)GR_SUB_E && (unsigned)lz < (unsigned)GR_SUB_E;
            const unsigned long long mask = __ballot(keep);
            const int kept = __popcll(mask);
            const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
            // the local vertex (< GR_SUB_E3) and the point index (< n: written by the bin kernel from a row below the count)
            if (keep) mine[rank] = ((unsigned)(w >> 24) & 0xFFFFu) | (unsigned)((lx * GR_SUB_E + ly) * GR_SUB_E + lz) << 16;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int j = grp; j < kept; j += 8) {  // eight records per step, a lane per (record, channel)
                const unsigned k = mine[j];
                const int i = (int)(k & 0xFFFFu), v = (int)(k >> 16) & (GR_SUB_E3 - 1);
                if (ch == 0) atomicAdd(&num[v], 1u);
                if (chok) atomicAdd(&acc[v * GR_CHUNK + ch], (double)feat[(size_t)i * c + ch0 + ch]);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        __syncthreads();
    }
    float *__restrict__ vol = a.vol + ((size_t)s * c + ch0) * R3;
    for (int e = tid; e < GR_SUB_E3 * GR_CHUNK; e += PV_TPB) {
        const int chh = e / GR_SUB_E3, l = e % GR_SUB_E3;
        const int gx = sx * GR_SUB_E + l / (GR_SUB_E * GR_SUB_E), gy = sy * GR_SUB_E + (l / GR_SUB_E) % GR_SUB_E, gz = sz * GR_SUB_E + l % GR_SUB_E;
        if (ch0 + chh < c && gx < R && gy < R && gz < R) {
            const unsigned k = any ? num[l] : 0u;
            vol[(size_t)chh * R3 + ((size_t)gx * R + gy) * R + gz] = k ? (float)(acc[l * GR_CHUNK + chh] / (double)k) : 0.f;
        }
    }
    if (ch0 == 0) {
        int *__restrict__ cnt = a.cnt + (size_t)s * R3;
        for (int l = tid; l < GR_SUB_E3; l += PV_TPB) {
            const int gx = sx * GR_SUB_E + l / (GR_SUB_E * GR_SUB_E), gy = sy * GR_SUB_E + (l / GR_SUB_E) % GR_SUB_E, gz = sz * GR_SUB_E + l % GR_SUB_E;
            if (gx < R && gy < R && gz < R) cnt[((size_t)gx * R + gy) * R + gz] = any ? (int)num[l] : 0;
        }
    }
}

struct PvVoxGrad {
    int n, c;
    GrBox g;
    const float *xyz;
    const int *len;
    const int *cnt;   // (b, R, R, R): the forward's
    const float *gv;  // (b, c, R, R, R)
    float *gf;        // (b, n, c)
};

// grid (ceil(n / PV_PTS), b)
__global__ __launch_bounds__(PV_TPB) void pv_vox_grad_kernel(PvVoxGrad a) {
    __shared__ int vtx[PV_PTS];
    __shared__ int num[PV_PTS];
    int s, bx;
    rf::place_2d<false>(bx, s);
    const int tid = threadIdx.x, n = a.n, c = a.c;
    const GrBox g = a.g;
    const int R = g.R, L = rf::ragged_count(a.len, s, n);
    const size_t R3 = (size_t)R * R * R;
    const int p0 = bx * PV_PTS;
    if (tid < PV_PTS) {
        const int i = p0 + tid;
        int v = -1, k = 0;
        if (i < L) {
            PvPoint p;
            if (pv_point(a.xyz + ((size_t)s * n + i) * 3, g, p)) {
                int kx, ky, kz;
                pv_nearest(p, kx, ky, kz);
                v = (kx * R + ky) * R + kz;
                k = a.cnt[(size_t)s * R3 + v];
            }
        }
        vtx[tid] = v, num[tid] = k;
    }
    __syncthreads();
    const int np = n - p0 < PV_PTS ? n - p0 : PV_PTS, total = np * c;
    const float *__restrict__ gv = a.gv + (size_t)s * c * R3;
    float *__restrict__ gf = a.gf + ((size_t)s * n + p0) * c;
#pragma unroll 4
    for (int e = tid; e < total; e += PV_TPB) {
        const int p = e / c, ch = e - p * c;
        const int v = vtx[p], k = num[p];
        const bool ok = v >= 0 && k >= 1;
        const float w = gv[(size_t)ch * R3 + (size_t)(ok ? v : 0)];  // an unconditional load, so that several are in flight
        gf[e] = ok ? (float)((double)w / (double)k) : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ trilinear devoxelization
struct PvDevox {
    int n, c;
    GrBox g;
    const float *xyz;
    const int *len;
    const float *vol;  // (b, c, R, R, R)
    float *feat;       // (b, n, c)
    int *inside;
};

// grid (ceil(n / PV_PTS), b)
__global__ __launch_bounds__(PV_TPB) void pv_devox_kernel(PvDevox a) {
    __shared__ int vtx[PV_PTS];
    __shared__ float tt[PV_PTS * 3];
    __shared__ unsigned wcnt[PV_TPB / 64];
    int s, bx;
    rf::place_2d<false>(bx, s);
    const int tid = threadIdx.x, n = a.n, c = a.c;
    const GrBox g = a.g;
    const int R = g.R, L = rf::ragged_count(a.len, s, n);
    const float *__restrict__ xyz = a.xyz + (size_t)s * n * 3;
    const int p0 = bx * PV_PTS;
    if (tid < PV_PTS) {
        const int i = p0 + tid;
        PvPoint p;
        const bool in = i < L && pv_point(xyz + (size_t)i * 3, g, p);
        vtx[tid] = in ? (p.ix * R + p.iy) * R + p.iz : -1;
        tt[tid * 3] = in ? p.tx : 0.f, tt[tid * 3 + 1] = in ? p.ty : 0.f, tt[tid * 3 + 2] = in ? p.tz : 0.f;
    }
    if (bx == 0) {  // the inside count of the sample
        unsigned cnt = 0;
        for (int i = tid; i < L; i += PV_TPB) {
            PvPoint p;
            cnt += pv_point(xyz + (size_t)i * 3, g, p);
        }
        cnt = rf::wave_add_u32(cnt);
        if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
    }
    __syncthreads();
    if (bx == 0 && tid == 0) a.inside[s] = (int)((wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]));
    const int np = n - p0 < PV_PTS ? n - p0 : PV_PTS, total = np * c;
    const size_t R3 = (size_t)R * R * R;
    const float *__restrict__ vol = a.vol + (size_t)s * c * R3;
    float *__restrict__ feat = a.feat + ((size_t)s * n + p0) * c;
    for (int e = tid; e < total; e += PV_TPB) {
        const int p = e / c, ch = e - p * c;
        const int v = vtx[p];
        float o = 0.f;
        if (v >= 0) {
            PvPoint q;
            q.tx = tt[p * 3], q.ty = tt[p * 3 + 1], q.tz = tt[p * 3 + 2];
            const float *__restrict__ pl = vol + (size_t)ch * R3 + (size_t)v;
            double sum = 0.0;
#pragma unroll
            for (int d = 0; d < 8; d++) {
                const int dx = d >> 2, dy = (d >> 1) & 1, dz = d & 1;
                sum += pv_weight(q, dx, dy, dz) * (double)pl[((size_t)dx * R + dy) * R + dz];
            }
            o = (float)sum;
        }
        feat[e] = o;
    }
}

struct PvBrick {
    int n, c;
    GrBox g;
    const unsigned *starts;
    const unsigned long long *recs;
    const float *xyz;
    const float *gf;  // (b, n, c)
    float *gv;        // (b, c, R, R, R)
};

// gr_subbrick_scatter of grad_feat times the corner's weight, recomputed from xyz.  grid (ceil(R / GR_SUB_E)^3 *
// ceil(c / GR_CHUNK), b), the channel chunk fastest
__global__ __launch_bounds__(GR_SUB_TPB) void pv_devox_brick_kernel(PvBrick a) {
    int s, bx;
    rf::place_2d<false>(bx, s);
    const GrBox g = a.g;
    const int R = g.R, c = a.c, n = a.n;
    const int nb = gr_nb(R), nb3 = nb * nb * nb;
    const size_t R3 = (size_t)R * R * R;
    const unsigned *__restrict__ st = a.starts + (size_t)s * (nb3 + 1);
    const unsigned long long *__restrict__ rec = a.recs + (size_t)s * n;
    const float *__restrict__ xyz = a.xyz + (size_t)s * n * 3;
    const float *__restrict__ gf = a.gf + (size_t)s * n * c;
    gr_subbrick_scatter(bx, R, c, st, rec, a.gv + (size_t)s * c * R3, [&](int i, int d, int ch) {
        PvPoint p;
        pv_point(xyz + (size_t)i * 3, g, p);  // inside: the bin kernel kept it; only t is used
        return pv_weight(p, d >> 2, (d >> 1) & 1, d & 1) * (double)gf[(size_t)i * c + ch];
    });
}

struct PvXyzGrad {
    int n, c;
    GrBox g;
    const float *xyz;
    const int *len;
    const float *vol;  // (b, c, R, R, R)
    const float *gf;   // (b, n, c)
    float *out;        // (b, n, 3)
};

// grid (ceil(n / PV_PTS), b): eight lanes per point, lane d sums g_d over the channels; lanes 0 ... 2 then form one axis each
__global__ __launch_bounds__(PV_TPB) void pv_devox_xyz_kernel(PvXyzGrad a) {
    int s, bx;
    rf::place_2d<false>(bx, s);
    const int tid = threadIdx.x, n = a.n, c = a.c;
    const int i = bx * PV_PTS + (tid >> 3), d = tid & 7;
    const GrBox g = a.g;
    const int R = g.R, L = rf::ragged_count(a.len, s, n);
    const size_t R3 = (size_t)R * R * R;
    PvPoint p;
    p.ix = p.iy = p.iz = 0, p.tx = p.ty = p.tz = 0.f;
    bool in = false;
    if (i < L) in = pv_point(a.xyz + ((size_t)s * n + i) * 3, g, p);
    double gd = 0.0;
    if (in) {
        const float *__restrict__ pl = a.vol + (size_t)s * c * R3 + ((size_t)(p.ix + (d >> 2)) * R + (p.iy + ((d >> 1) & 1))) * R + (p.iz + (d & 1));
        const float *__restrict__ gf = a.gf + ((size_t)s * n + i) * c;
        for (int ch = 0; ch < c; ch++) gd += (double)gf[ch] * (double)pl[(size_t)ch * R3];
    }
    const double wx[2] = {(double)(1.0f - p.tx), (double)p.tx}, wy[2] = {(double)(1.0f - p.ty), (double)p.ty},
                 wz[2] = {(double)(1.0f - p.tz), (double)p.tz};
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < 8; e++) {  // (every lane takes part in the shuffles)
        const int ex = e >> 2, ey = (e >> 1) & 1, ez = e & 1;
        const double v = __shfl(gd, (tid & 56) + e, 64);
        const bool up = d == 0 ? ex : (d == 1 ? ey : ez);
        const double w = d == 0 ? wy[ey] * wz[ez] : (d == 1 ? wx[ex] * wz[ez] : wx[ex] * wy[ey]);
        acc += (up ? v : -v) * w;
    }
    if (i < n && d < 3) a.out[((size_t)s * n + i) * 3 + d] = in ? (float)((double)g.inv_h * acc) : 0.f;
}

}  // namespace

extern "C" {

size_t rf_voxelize_mean_workspace_bytes(int b, int n, int res) {
    if (!gr_sizes_ok(b, n, res)) return 0;
    return gr_sort_layout(b, n, res).total;
}

int rf_voxelize_mean(int b, int n, int c, int res, float lo, float hi, const float *xyz, const int *len, const float *feat, float *vol,
                     int *cnt, int *inside, void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (b < 0 || n < 0 || c < 0 || res < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!gr_sizes_ok(b, n, c, res)) return RF_EINVAL;
    if (!gr_box_ok(lo, hi)) return RF_EINVAL;
    if (!rf::tensors_ok({xyz, feat, vol, cnt, inside}, {len}) || !rf::workspace_ok(workspace)) return RF_EINVAL;
    const GrSortLayout l = gr_sort_layout(b, n, res);
    if (workspace_bytes < l.total) return RF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;

    char *w = (char *)workspace;
    unsigned *starts = (unsigned *)(w + l.starts);
    unsigned long long *recs = (unsigned long long *)(w + l.recs);
    const GrSortCloud bin{n, gr_box(res, lo, hi), xyz, len, starts, recs};
    RF_LAUNCH("voxelize_bin", pv_bin_kernel<true>, dim3(b), dim3(GR_BIN_TPB), 0, st, bin);
    const int nsb = rf::ceil_div(res, GR_SUB_E), nchunk = rf::ceil_div(c, GR_CHUNK);
    const PvVox vx{n, c, res, starts, recs, feat, vol, cnt, inside};
    RF_LAUNCH("voxelize_brick", pv_vox_kernel, dim3(nsb * nsb * nsb * nchunk, b), dim3(PV_TPB), 0, st, vx);
    return RF_OK;
}

int rf_voxelize_mean_grad(int b, int n, int c, int res, float lo, float hi, const float *xyz, const int *len, const int *cnt,
                          const float *grad_vol, float *grad_feat, rf_stream_t stream) {
    if (b < 0 || n < 0 || c < 0 || res < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!gr_sizes_ok(b, n, c, res)) return RF_EINVAL;
    if (!gr_box_ok(lo, hi)) return RF_EINVAL;
    if (!rf::tensors_ok({xyz, cnt, grad_vol, grad_feat}, {len})) return RF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const PvVoxGrad a{n, c, gr_box(res, lo, hi), xyz, len, cnt, grad_vol, grad_feat};
    RF_LAUNCH("voxelize_grad", pv_vox_grad_kernel, dim3(rf::ceil_div(n, PV_PTS), b), dim3(PV_TPB), 0, st, a);
    return RF_OK;
}

int rf_trilinear_devoxelize(int b, int n, int c, int res, float lo, float hi, const float *xyz, const int *len, const float *vol,
                            float *feat, int *inside, rf_stream_t stream) {
    if (b < 0 || n < 0 || c < 0 || res < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!gr_sizes_ok(b, n, c, res)) return RF_EINVAL;
    if (!gr_box_ok(lo, hi)) return RF_EINVAL;
    if (!rf::tensors_ok({xyz, vol, feat, inside}, {len})) return RF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const PvDevox a{n, c, gr_box(res, lo, hi), xyz, len, vol, feat, inside};
    RF_LAUNCH("devoxelize", pv_devox_kernel, dim3(rf::ceil_div(n, PV_PTS), b), dim3(PV_TPB), 0, st, a);
    return RF_OK;
}

size_t rf_trilinear_devoxelize_grad_workspace_bytes(int b, int n, int res) {
    if (!gr_sizes_ok(b, n, res)) return 0;
    return gr_sort_layout(b, n, res).total;
}

int rf_trilinear_devoxelize_grad(int b, int n, int c, int res, float lo, float hi, const float *xyz, const int *len, const float *vol,
                                 const float *grad_feat, float *grad_vol, float *grad_xyz, void *workspace, size_t workspace_bytes,
                                 rf_stream_t stream) {
    if (b < 0 || n < 0 || c < 0 || res < 0) return RF_EINVAL;
    if (b == 0) return RF_OK;
    if (!gr_sizes_ok(b, n, c, res)) return RF_EINVAL;
    if (!gr_box_ok(lo, hi)) return RF_EINVAL;
    // (grad_xyz may be NULL: it is then not computed)
    if (!rf::tensors_ok({xyz, vol, grad_feat, grad_vol}, {grad_xyz, len}) || !rf::workspace_ok(workspace)) return RF_EINVAL;
    const GrSortLayout l = gr_sort_layout(b, n, res);
    if (workspace_bytes < l.total) return RF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;

    char *w = (char *)workspace;
    unsigned *starts = (unsigned *)(w + l.starts);
    unsigned long long *recs = (unsigned long long *)(w + l.recs);
    const GrBox g = gr_box(res, lo, hi);
    const GrSortCloud bin{n, g, xyz, len, starts, recs};
    RF_LAUNCH("devoxelize_bin", pv_bin_kernel<false>, dim3(b), dim3(GR_BIN_TPB), 0, st, bin);
    const int nsb = rf::ceil_div(res, GR_SUB_E), nchunk = rf::ceil_div(c, GR_CHUNK);
    const PvBrick br{n, c, g, starts, recs, xyz, grad_feat, grad_vol};
    RF_LAUNCH("devoxelize_brick", pv_devox_brick_kernel, dim3(nsb * nsb * nsb * nchunk, b), dim3(GR_SUB_TPB), 0, st, br);
    if (grad_xyz) {
        const PvXyzGrad xg{n, c, g, xyz, len, vol, grad_feat, grad_xyz};
        RF_LAUNCH("devoxelize_xyz_grad", pv_devox_xyz_kernel, dim3(rf::ceil_div(n, PV_PTS), b), dim3(PV_TPB), 0, st, xg);
    }
    return RF_OK;
}

}  // extern "C"
