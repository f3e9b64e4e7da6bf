// gridding.hpp -- the grid geometry of include/rfops.h's gridding section, ONCE: the box, the per-axis cell rule and the brick
// count.  gridding.hip (the Gridding layer and loss), grnet_layers.hip (Gridding Reverse, Cubic Feature Sampling) and
// point_voxel.hip (average voxelize, trilinear devoxelize) share it through brick_sort.hpp, which adds their common sort and scatter.
#pragma once
#include "common.hpp"

constexpr int GR_E = 16;  // vertices per brick edge of the counting sort: (RF_GR_MAX_RES / GR_E)^3 = 4096 bins fit one workgroup

struct GrBox {
    float lo, inv_h, top;  // top = (float)(R - 1)
    int R;
};

__host__ __device__ __forceinline__ int gr_nb(int R) { return (R + GR_E - 1) / GR_E; }

// one axis of the contract: u = (x - lo) * inv_h (two roundings), inside iff 0 <= u <= R - 1 (a NaN fails), the cell
// i = min(floor(u), R - 2) and t = u - i in [0, 1]
__device__ __forceinline__ bool gr_axis(float x, const GrBox &g, int &i, float &t) {
    const float u = (x - g.lo) * g.inv_h;
    const bool in = u >= 0.f && u <= g.top;
    const int k = in ? (int)floorf(u) : 0;
    i = k < g.R - 2 ? k : g.R - 2;
    t = u - (float)i;
    return in;
}

inline bool gr_sizes_ok(int b, int n, int res) {
    return b >= 1 && b <= 65535 && n >= 1 && n <= RF_GR_MAX_POINTS && res >= 2 && res <= RF_GR_MAX_RES;
}

inline bool gr_box_ok(float lo, float hi) { return isfinite(lo) && isfinite(hi) && lo < hi; }

inline GrBox gr_box(int res, float lo, float hi) {
    GrBox g;
    g.lo = lo;
    g.inv_h = (float)((double)(res - 1) / ((double)hi - (double)lo));
    g.top = (float)(res - 1);
    g.R = res;
    return g;
}
