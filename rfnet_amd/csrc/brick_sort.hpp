// brick_sort.hpp -- what the grid ops share beyond gridding.hpp's geometry, ONCE: the counting sort of a cloud's inside points into
// bricks of GR_E^3 vertices (gridding.hip, grnet_layers.hip, point_voxel.hip) and the walk that scatters the sorted records into
// one sub-brick of GR_SUB_E^3 vertices for a chunk of GR_CHUNK channels (the Cubic Feature Sampling backward and the
// devoxelize backward), with the host's layout of "starts + recs".  DESIGN.md 5.3l and 5.3m describe both.
#pragma once
#include "gridding.hpp"

constexpr int GR_BIN_TPB = 1024;  // the sort: one workgroup per cloud
constexpr int GR_MAX_NB3 = 4096;  // (RF_GR_MAX_RES / GR_E)^3 bricks per sample at most
constexpr int GR_SUB_TPB = 256;   // the scatter: one workgroup per (sub-brick, channel chunk)
constexpr int GR_SUB_E = 8, GR_SUB_E3 = GR_SUB_E * GR_SUB_E * GR_SUB_E;  // vertices per sub-brick edge
constexpr int GR_CHUNK = 8;       // channels per workgroup: 8 corners (or records) x 8 channels = one wave per step
static_assert(RF_GR_MAX_RES == 256 && GR_MAX_NB3 == (RF_GR_MAX_RES / GR_E) * (RF_GR_MAX_RES / GR_E) * (RF_GR_MAX_RES / GR_E), "");
static_assert(GR_MAX_NB3 == 4 * GR_BIN_TPB, "the scan of gr_brick_sort gives a thread four bins");
static_assert(GR_E == 2 * GR_SUB_E && 8 * GR_CHUNK == 64 && GR_SUB_E3 * GR_CHUNK * sizeof(double) == 32768, "");
static_assert(RF_GR_MAX_POINTS <= 65536 && GR_SUB_E3 <= 65536, "a record holds 3 x 8 bits of key and 16 bits of point index");

// One cloud of a sort whose record carries the point index: the arguments of cfs_bin_kernel and pv_bin_kernel.
struct GrSortCloud {
    int n;
    GrBox g;
    const float *xyz;
    const int *len;
    unsigned *starts;          // (b, nb^3 + 1): where every brick's list begins; the last entry is the inside count
    unsigned long long *recs;  // (b, n): the key (3 x 8 bits) and the point index (16 bits, from bit 24)
};

// the record of GrSortCloud; i < 65536
__device__ __forceinline__ unsigned long long gr_index_record(int kx, int ky, int kz, int i) {
    return (unsigned long long)((unsigned)kx | (unsigned)ky << 8 | (unsigned)kz << 16) | (unsigned long long)(unsigned)i << 24;
}

// The counting sort of one cloud, by a workgroup of GR_BIN_TPB threads: an LDS histogram over the bricks, an exclusive scan, a
// scatter through LDS cursors.  point(i, kx, ky, kz, word) says for row i < L whether the point is inside and gives the key
// (a cell or a vertex, < R per axis) and the finished 64-bit record.  st receives the nb^3 list starts and the inside count,
// which also goes to *inside where that is not null; rec receives the records, a list's order being the order of arrival.
template <class P>
__device__ __forceinline__ void gr_brick_sort(int L, int R, unsigned *__restrict__ st, unsigned long long *__restrict__ rec, int *inside,
                                              P point) {
    __shared__ unsigned hist[GR_MAX_NB3];
    __shared__ unsigned wtot[GR_BIN_TPB / 64];
    const int tid = threadIdx.x;
    const int nb = gr_nb(R), nb3 = nb * nb * nb;

    for (int k = tid; k < nb3; k += GR_BIN_TPB) hist[k] = 0;
    __syncthreads();
    for (int i = tid; i < L; i += GR_BIN_TPB) {
        int kx, ky, kz;
        unsigned long long word;
        if (point(i, kx, ky, kz, word)) atomicAdd(&hist[((kx / GR_E) * nb + ky / GR_E) * nb + kz / GR_E], 1u);  // k <= R - 1: a brick < nb
    }
    __syncthreads();
    // exclusive scan over the bins: a thread owns four consecutive bins, a wave by DPP, the waves in order
    unsigned cn[4], tsum = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int idx = tid * 4 + k;
        cn[k] = idx < nb3 ? hist[idx] : 0u;
        tsum += cn[k];
    }
    const unsigned incl = rf::wave_incl_scan(tsum);
    if ((tid & 63) == 63) wtot[tid >> 6] = incl;
    __syncthreads();
    unsigned run = incl - tsum;
    for (int w = 0; w < (tid >> 6); w++) run += wtot[w];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int idx = tid * 4 + k;
        if (idx < nb3) hist[idx] = run, st[idx] = run;  // the bin's cursor and its start
        run += cn[k];
    }
    if (tid == GR_BIN_TPB - 1) {
        st[nb3] = run;
        if (inside) *inside = (int)run;
    }
    __syncthreads();
    for (int i = tid; i < L; i += GR_BIN_TPB) {
        int kx, ky, kz;
        unsigned long long word;
        if (point(i, kx, ky, kz, word)) {
            const unsigned pos = atomicAdd(&hist[((kx / GR_E) * nb + ky / GR_E) * nb + kz / GR_E], 1u);
            rec[pos] = word;  // pos < the inside count <= L
        }
    }
}

// The scatter of a cloud sorted by the brick of the CELL (records of GrSortCloud) into one sub-brick, by a workgroup of
// GR_SUB_TPB threads: bx is the workgroup's logical place in (sub-brick, channel chunk), the chunk fastest; st and rec are the
// sample's lists, gv the sample's (c, R, R, R) volume.  A wave takes one record per step with a lane per (corner d, channel ch)
// and adds term(i, d, ch) for the record's point i into LDS doubles; every element of the sub-brick's part of gv is then stored
// once, zeros where nothing fell.  The order of the additions is the order of arrival.
template <class T>
__device__ __forceinline__ void gr_subbrick_scatter(int bx, int R, int c, const unsigned *__restrict__ st,
                                                    const unsigned long long *__restrict__ rec, float *__restrict__ gv, T term) {
    __shared__ double acc[GR_SUB_E3 * GR_CHUNK];  // [vertex][channel]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nsb = (R + GR_SUB_E - 1) / GR_SUB_E, nchunk = (c + GR_CHUNK - 1) / GR_CHUNK;
    const int nb = gr_nb(R);
    const int sbi = bx / nchunk, ch0 = (bx - sbi * nchunk) * GR_CHUNK;
    const int sz = sbi % nsb, sy = (sbi / nsb) % nsb, sx = sbi / (nsb * nsb);
    const size_t R3 = (size_t)R * R * R;
    gv += (size_t)ch0 * R3;

    // The cells that reach this sub-brick's vertices are those of its own brick and, where the sub-brick is the lower half of its
    // brick along an axis, of the lower neighbour along that axis: at most eight lists.
    auto list = [&](int d, unsigned &lo, unsigned &hi) {
        const int dx = d >> 2, dy = (d >> 1) & 1, dz = d & 1;
        const int nx = (sx >> 1) - dx, ny = (sy >> 1) - dy, nz = (sz >> 1) - dz;
        const bool skip = (dx && ((sx & 1) || nx < 0)) || (dy && ((sy & 1) || ny < 0)) || (dz && ((sz & 1) || nz < 0));
        const int q = skip ? 0 : (nx * nb + ny) * nb + nz;
        lo = st[q], hi = skip ? lo : st[q + 1];
    };
    unsigned any = 0;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        unsigned lo, hi;
        list(d, lo, hi);
        any |= hi - lo;
    }
    if (any) {  // (uniform over the workgroup)
        for (int l = tid; l < GR_SUB_E3 * GR_CHUNK; l += GR_SUB_TPB) acc[l] = 0.0;
        __syncthreads();
        const int d = lane >> 3, ch = lane & 7, dx = d >> 2, dy = (d >> 1) & 1, dz = d & 1;
        const bool chok = ch0 + ch < c;
#pragma unroll 1
        for (int q = 0; q < 8; q++) {
            unsigned lo, hi;
            list(q, lo, hi);
            for (unsigned r0 = lo + wave * 64; r0 < hi; r0 += GR_SUB_TPB) {  // uniform over the wave
                const unsigned r = r0 + lane;
                const unsigned long long w = r < hi ? rec[r] : 0ull;
                // the cell relative to this sub-brick's first vertex: kept iff -1 ... 7 on every axis
                const int cx = (int)((unsigned)w & 255u) - sx * GR_SUB_E + 1, cy = (int)((unsigned)(w >> 8) & 255u) - sy * GR_SUB_E + 1,
                          cz = (int)((unsigned)(w >> 16) & 255u) - sz * GR_SUB_E + 1;
                const bool keep = r < hi && (unsigned)cx <= (unsigned)GR_SUB_E && (unsigned)cy <= (unsigned)GR_SUB_E &&
                                  (unsigned)cz <= (unsigned)GR_SUB_E;
                const unsigned key = ((unsigned)(w >> 24) & 0xFFFFu) | (unsigned)cx << 16 | (unsigned)cy << 20 | (unsigned)cz << 24;
                unsigned long long mask = __ballot(keep);
                while (mask) {  // a record per step, a lane per (corner, channel)
                    const int j = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const unsigned k = (unsigned)__shfl((int)key, j, 64);
                    const int i = (int)(k & 0xFFFFu);  // < n: written by the bin kernel from a row below the count
                    const int lx = (int)((k >> 16) & 15u) - 1 + dx, ly = (int)((k >> 20) & 15u) - 1 + dy,
                              lz = (int)((k >> 24) & 15u) - 1 + dz;
                    if ((unsigned)lx < (unsigned)GR_SUB_E && (unsigned)ly < (unsigned)GR_SUB_E && (unsigned)lz < (unsigned)GR_SUB_E && chok)
                        atomicAdd(&acc[((lx * GR_SUB_E + ly) * GR_SUB_E + lz) * GR_CHUNK + ch], term(i, d, ch0 + ch));
                }
            }
        }
        __syncthreads();
    }
    for (int e = tid; e < GR_SUB_E3 * GR_CHUNK; e += GR_SUB_TPB) {
        const int chh = e / GR_SUB_E3, l = e % GR_SUB_E3;
        const int gx = sx * GR_SUB_E + l / (GR_SUB_E * GR_SUB_E), gy = sy * GR_SUB_E + (l / GR_SUB_E) % GR_SUB_E,
                  gz = sz * GR_SUB_E + l % GR_SUB_E;
        if (ch0 + chh < c && gx < R && gy < R && gz < R)
            gv[(size_t)chh * R3 + ((size_t)gx * R + gy) * R + gz] = any ? (float)acc[l * GR_CHUNK + chh] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ host
struct GrSortLayout {
    size_t starts, recs, total;
};

// the workspace of a sort: the starts of `lists` lists of nb^3 + 1 entries, then `records` records
inline GrSortLayout gr_sort_layout(size_t lists, size_t records, int res) {
    const size_t nb = gr_nb(res), nb3 = nb * nb * nb;
    GrSortLayout l;
    l.starts = 0;
    l.recs = l.starts + rf::align256(lists * (nb3 + 1) * sizeof(unsigned));
    l.total = l.recs + rf::align256(records * sizeof(unsigned long long));
    return l;
}

// one cloud of n rows per sample
inline GrSortLayout gr_sort_layout(int b, int n, int res) { return gr_sort_layout((size_t)b, (size_t)b * (size_t)n, res); }

inline bool gr_sizes_ok(int b, int n, int c, int res) { return gr_sizes_ok(b, n, res) && c >= 1 && c <= RF_CFS_MAX_CHANNELS; }
