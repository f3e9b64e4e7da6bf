// chamfer_cross.hip -- the Chamfer MATRIX of two collections of clouds: for every cloud i of xyz1 (s clouds) and every
// cloud j of xyz2 (r clouds) the six numbers a set metric needs (the halves of CD-L1 and CD-L2, the squared directed
// Hausdorff distances), without ever forming the s * r expanded pairs.  include/rfops.h states the contract; DESIGN.md
// 5.3h the measurements.
//
//   sort     each collection ONCE (rfp::sort_sets, per-cloud counts, no non-finite flag), one collection in the self case
//   boxes    one wave per cloud: the cloud's box, the union of its superblock boxes
//   sweep    a wave keeps one 64-record superblock of sorted cloud i in registers and goes through a strip of partner
//            clouds j; per partner a boxed walk (nearest candidate superblock first, then every superblock whose bound is
//            not beyond the wave's largest running minimum, 16-record blocks tested before they are scanned) with ONE
//            running minimum per lane: no index, no tie state.  Then one wave reduction and one record per (i, j, superblock)
//   reduce   one wave per (pair, direction) adds the records up and writes three columns
//
// The sums.  The order of a sorted cloud's records inside one sort key is whatever the sort's atomics gave, so WHICH points a
// superblock holds may differ between two calls (and between a collection sorted once or twice): a float sum per superblock
// would not be reproducible.  Every sum here is therefore an INTEGER sum -- exact, hence free of any order: a distance is put
// on a fixed-point grid that is a function of the pair alone (a power of two taken from the joint box of the two clouds, 111
// bits below it) and split into five 26-bit limbs; the wave adds limbs with 32-bit adds (64 * 2^26 = 2^32), the reduce kernel in
// 64 bits.  A value loses bits only when it is below 2^-88 of that power of two.  No float atomics, no float sum of more than
// one term anywhere.
#include "common.hpp"
#include "nn_pruned.hpp"

namespace {

constexpr int CX_WAVES = 4;   // waves per workgroup, each on its own (no barrier, no LDS)
constexpr int CX_STRIP = 8;   // partner clouds a wave goes through with its queries in registers
constexpr int CX_REC = 12;    // 32-bit words per (i, j, superblock) record: 5 limbs of sum d, 5 of sum sqrtf(d), max bits, 0
constexpr int CX_LIMBS = 5;
constexpr int CX_LIMB_BITS = 26;
constexpr unsigned CX_LIMB_MASK = (1u << CX_LIMB_BITS) - 1u;
// fixed point: a value v < 2^(eref - 125) (eref a biased fp32 exponent) is held as v * 2^(236 - eref) < 2^111
constexpr int CX_FIX = 236;

// one sorted collection, as the sweep sees it
struct CxSide {
    const float *xyz;   // (clouds, nsb * 64, 3)
    const int *orig;    // (clouds, nsb * 64)
    const float *b16;   // (clouds, nsb, 24)
    const float *b64;   // (clouds, nsb, 8)
    const float *cbox;  // (clouds, 8) lo.xyz, 0, hi.xyz, 0 of the whole cloud
    const int *len;     // (clouds) or NULL
    int clouds, nfull, nsb;
};

// ---- wave minimum / maximum of floats (uniform results), none of them NaN.  -inf marks a lane that takes no part in a max, +inf
// one that takes no part in a min.  Local on purpose: with rf::wave_min_f32 / rf::wave_max_f32 (wave.hpp) the sweep is slower,
// 414 against 290 us at 32 x 32 clouds of 2048 points (profiles/wave_primitives_ab.txt).
// The integer reductions are rf::wave_add_u32 / rf::wave_max_u32.
#define CX_ROR(n) (0x120 + (n))
__device__ __forceinline__ float cx_wave_fmax(float v) {
#define CX_STEP(n) v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CX_ROR(n), 0xf, 0xf, false)))
    CX_STEP(8);
    CX_STEP(4);
    CX_STEP(2);
    CX_STEP(1);
#undef CX_STEP
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}
__device__ __forceinline__ float cx_wave_fmin(float v) {
#define CX_STEP(n) v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CX_ROR(n), 0xf, 0xf, false)))
    CX_STEP(8);
    CX_STEP(4);
    CX_STEP(2);
    CX_STEP(1);
#undef CX_STEP
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fminf(fminf(r0, r1), fminf(r2, r3));
}
#undef CX_ROR

// ---- the fixed-point grid of a pair ----------------------------------------------------------------------------------------
// The biased exponent of the squared diagonal D of the joint box of cloud i of xyz1 (a) and cloud j of xyz2 (b): every
// distance of the pair is below 2^(e - 125) (D < 2^(e - 126), and the roundings of D and of a distance are a few ulps).  The
// expression is symmetric in a and b and is evaluated by the sweep and by the reduce kernel alike.
__device__ __forceinline__ int cx_pair_exp(const float *__restrict__ a, const float *__restrict__ b) {
    const float ex = fmaxf(a[4], b[4]) - fminf(a[0], b[0]);
    const float ey = fmaxf(a[5], b[5]) - fminf(a[1], b[1]);
    const float ez = fmaxf(a[6], b[6]) - fminf(a[2], b[2]);
    const float D = (ex * ex + ey * ey) + ez * ez;
    return (int)((__float_as_uint(D) >> 23) & 255u);
}
// sqrtf of such a distance is below 2^(e' - 125) with e' - 125 = ceil((e - 125) / 2)
__device__ __forceinline__ int cx_sqrt_exp(int e) { return (e + 132) / 2 - 3; }

// v >= 0 (the sign is not read) as floor(v * 2^(CX_FIX - eref)) in five 26-bit limbs.  The shift is clamped, so that a value
// the bound does not hold for (a cloud with non-finite coordinates) stays below 2^111 as well.
__device__ __forceinline__ void cx_fixed(float v, int eref, unsigned (&l)[CX_LIMBS]) {
    const unsigned bits = __float_as_uint(v);
    int e = (int)((bits >> 23) & 255u);
    unsigned m = bits & 0x7FFFFFu;
    if (e != 0) m |= 0x800000u;
    else e = 1;
    int sh = e - eref + (CX_FIX - 150);  // v = m * 2^(e - 150)
    sh = sh > 87 ? 87 : sh;
    if (sh < 0) {
        m = sh > -24 ? m >> (-sh) : 0u;
        sh = 0;
    }
    const unsigned long long mm = m;
    const unsigned long long lo = sh < 64 ? mm << sh : 0ull;
    const unsigned long long hi = sh == 0 ? 0ull : (sh < 64 ? mm >> (64 - sh) : mm << (sh - 64));
    l[0] = (unsigned)lo & CX_LIMB_MASK;
    l[1] = (unsigned)(lo >> 26) & CX_LIMB_MASK;
    l[2] = (unsigned)((lo >> 52) | (hi << 12)) & CX_LIMB_MASK;
    l[3] = (unsigned)(hi >> 14) & CX_LIMB_MASK;
    l[4] = (unsigned)(hi >> 40) & CX_LIMB_MASK;
}

// ---- the cloud boxes -------------------------------------------------------------------------------------------------------
// One wave per cloud: the union of its superblock boxes (an empty superblock has lo = +inf, hi = -inf and changes nothing).
// min and max are free of any order, so the box is a function of the cloud's valid points alone.
__global__ __launch_bounds__(64) void chamfer_cross_boxes_kernel(const float *__restrict__ b64a, int clouds_a, int nsb_a,
                                                                 const float *__restrict__ b64b, int nsb_b,
                                                                 float *__restrict__ cbox) {
    const int ci = blockIdx.x, lane = threadIdx.x;
    const bool second = ci >= clouds_a;
    const int nsb = second ? nsb_b : nsb_a;
    const float *__restrict__ bx = second ? b64b + (size_t)(ci - clouds_a) * nsb * 8 : b64a + (size_t)ci * nsb * 8;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int g = lane; g < nsb; g += 64) {
        const float4 l4 = *(const float4 *)(bx + (size_t)g * 8), h4 = *(const float4 *)(bx + (size_t)g * 8 + 4);
        lo[0] = fminf(lo[0], l4.x), lo[1] = fminf(lo[1], l4.y), lo[2] = fminf(lo[2], l4.z);
        hi[0] = fmaxf(hi[0], h4.x), hi[1] = fmaxf(hi[1], h4.y), hi[2] = fmaxf(hi[2], h4.z);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        lo[k] = cx_wave_fmin(lo[k]);
        hi[k] = cx_wave_fmax(hi[k]);
    }
    if (lane == 0) {
        float *__restrict__ o = cbox + (size_t)ci * 8;
        o[0] = lo[0], o[1] = lo[1], o[2] = lo[2], o[3] = 0.f;
        o[4] = hi[0], o[5] = hi[1], o[6] = hi[2], o[7] = 0.f;
    }
}

// ---- the sweep -------------------------------------------------------------------------------------------------------------
// squared distance from a box (plo, phi; a point when they coincide) to a box, the FUSED expression of the distance itself on
// the per-axis gaps max(lo - phi, plo - hi, 0).  Every candidate c of the box and every query p of the other have
// |fl(c - p)| >= gap on each axis (rounding is monotone), and squares and fmaf are monotone in non-negative arguments: bound
// <= d in fp32, exactly.  An empty box is at +inf.
__device__ __forceinline__ float cx_gap(float a, float b) { return fmaxf(fmaxf(a, b), 0.f); }
__device__ __forceinline__ float cx_bound(float lx, float ly, float lz, float hx, float hy, float hz, float pxl, float pyl,
                                          float pzl, float pxh, float pyh, float pzh) {
    const float gx = cx_gap(lx - pxh, pxl - hx), gy = cx_gap(ly - pyh, pyl - hy), gz = cx_gap(lz - pzh, pzl - hz);
    return rf::d2_fma(gx, gy, gz);
}

// Q: the collection the wave's queries come from, C: the collection of the partners.  DIR 0: Q is xyz1 (pair index
// qi * C.clouds + cj), DIR 1: Q is xyz2 (pair index cj * Q.clouds + qi).  grid (tiles * strips, Q.clouds).
// Every loop bound is a count: superblocks of a cloud, 64 pending lanes, 4 blocks, 16 records.
template <int DIR>
__global__ __launch_bounds__(CX_WAVES * 64) void chamfer_cross_sweep_kernel(CxSide Q, CxSide C, unsigned *__restrict__ rec) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tiles = (Q.nsb + CX_WAVES - 1) / CX_WAVES;
    const int strip = blockIdx.x / tiles;
    const int sb = (blockIdx.x - strip * tiles) * CX_WAVES + wave;
    if (sb >= Q.nsb) return;
    const int qi = blockIdx.y;
    const size_t qsb = (size_t)qi * Q.nsb + sb;
    const size_t qr = qsb * 64 + lane;
    const float qx = Q.xyz[qr * 3], qy = Q.xyz[qr * 3 + 1], qz = Q.xyz[qr * 3 + 2];
    const bool valid = Q.orig[qr] != -1;  // a padding record is no query
    const bool any = __ballot(valid) != 0ull;
    const float *__restrict__ qb = Q.b64 + qsb * 8;  // (uniform)
    const float qlx = qb[0], qly = qb[1], qlz = qb[2], qhx = qb[4], qhy = qb[5], qhz = qb[6];
    const float *__restrict__ qcb = Q.cbox + (size_t)qi * 8;

    const int j1 = min(C.clouds, (strip + 1) * CX_STRIP);
    for (int cj = strip * CX_STRIP; cj < j1; cj++) {
        const float *__restrict__ cxyz = C.xyz + (size_t)cj * C.nsb * 192;
        const float *__restrict__ cb16 = C.b16 + (size_t)cj * C.nsb * 24;
        const float *__restrict__ cb64 = C.b64 + (size_t)cj * C.nsb * 8;
        const int nsb = C.nsb;
        float best = INFINITY;  // the lane's running minimum: all there is of a "list"

        // one candidate superblock: the lanes' bounds to its four 16-record blocks against their running minima, then the
        // records of the blocks some lane needs (uniform addresses: scalar loads).  A padding record (+inf) gives +inf or
        // NaN, which fminf never takes.
        auto visit = [&](int g, bool test) {
            unsigned bm = 0xFu;
            if (test) {
                const float *__restrict__ bx = cb16 + (size_t)g * 24;
                const float pr = valid ? best : -INFINITY;
                bm = 0u;
#pragma unroll
                for (int blk = 0; blk < 4; blk++) {
                    const float lb = cx_bound(bx[blk * 6], bx[blk * 6 + 1], bx[blk * 6 + 2], bx[blk * 6 + 3],
                                              bx[blk * 6 + 4], bx[blk * 6 + 5], qx, qy, qz, qx, qy, qz);
                    if (__ballot(lb <= pr) != 0ull) bm |= 1u << blk;  // (uniform)
                }
                if (bm == 0u) return;
            }
            const float *__restrict__ cp = cxyz + (size_t)g * 192;
#pragma unroll 1
            for (int blk = 0; blk < 4; blk++) {
                if (!((bm >> blk) & 1u)) continue;
                const float *__restrict__ p = cp + blk * 48;
#pragma unroll
                for (int u = 0; u < 16; u++)
                    best = fminf(best, rf::d2_fma(p[u * 3] - qx, p[u * 3 + 1] - qy, p[u * 3 + 2] - qz));  // other - own
            }
        };

        if (any) {
            // 1. lanes <-> candidate superblocks: the one nearest to the wave's box goes first
            float near = INFINITY;
            int arg = 0;
            for (int r0 = 0; r0 < nsb; r0 += 64) {
                const int g = r0 + lane;
                float lb = INFINITY;
                if (g < nsb) {
                    const float4 lo = *(const float4 *)(cb64 + (size_t)g * 8), hi = *(const float4 *)(cb64 + (size_t)g * 8 + 4);
                    lb = cx_bound(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, qlx, qly, qlz, qhx, qhy, qhz);
                }
                if (lb < near) near = lb, arg = g;
            }
            const float wmin = cx_wave_fmin(near == near ? near : INFINITY);
            const unsigned long long at = __ballot(near == wmin);
            const int seed = at != 0ull ? __builtin_amdgcn_readlane(arg, __builtin_ctzll(at)) : 0;  // arg < nsb always
            visit(seed, false);
            // 2. every other superblock whose box is not beyond the wave's largest running minimum (which shrinks as the visits
            //    go), 64 superblocks at a time, nearest box first; the first box beyond it ends the round
            float wk = cx_wave_fmax(valid ? best : -INFINITY);
            for (int r0 = 0; r0 < nsb; r0 += 64) {
                const int g = r0 + lane;
                float lb = INFINITY;
                if (g < nsb && g != seed) {
                    const float4 lo = *(const float4 *)(cb64 + (size_t)g * 8), hi = *(const float4 *)(cb64 + (size_t)g * 8 + 4);
                    lb = cx_bound(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, qlx, qly, qlz, qhx, qhy, qhz);
                }
                bool pend = g < nsb && g != seed && lb <= wk && lb != INFINITY;
                while (__ballot(pend) != 0ull) {  // (uniform; a visit clears one of at most 64 pending lanes)
                    const float wmin2 = cx_wave_fmin(pend ? lb : INFINITY);
                    if (!(wmin2 <= wk)) break;
                    const unsigned long long who = __ballot(pend && lb == wmin2);
                    if (who == 0ull) break;
                    const int jn = __builtin_ctzll(who);
                    pend = pend && lane != jn;
                    visit(r0 + jn, true);
                    wk = cx_wave_fmax(valid ? best : -INFINITY);
                }
            }
        }

        // the wave's part of the pair: exact integer sums of d and sqrtf(d) on the pair's grid, and the max
        const float dv = valid ? best : 0.f;
        const int e1 = DIR == 0 ? cx_pair_exp(qcb, C.cbox + (size_t)cj * 8) : cx_pair_exp(C.cbox + (size_t)cj * 8, qcb);
        unsigned ld[CX_LIMBS], ls[CX_LIMBS];
        cx_fixed(dv, e1, ld);
        cx_fixed(sqrtf(dv), cx_sqrt_exp(e1), ls);
        unsigned word = 0u;
#pragma unroll
        for (int k = 0; k < CX_LIMBS; k++) {
            const unsigned a = rf::wave_add_u32(ld[k]), b = rf::wave_add_u32(ls[k]);
            word = lane == k ? a : (lane == CX_LIMBS + k ? b : word);
        }
        const unsigned mx = rf::wave_max_u32(__float_as_uint(dv));  // bits of non-negative floats order as the floats do
        word = lane == 2 * CX_LIMBS ? mx : word;
        const size_t pair = DIR == 0 ? (size_t)qi * C.clouds + cj : (size_t)cj * Q.clouds + qi;
        if (lane < CX_REC) rec[(pair * Q.nsb + sb) * CX_REC + lane] = word;
    }
}

// ---- the reduce ------------------------------------------------------------------------------------------------------------
struct CxReduce {
    int s, r, n, m, nsb1, nsb2;
    const float *cbox1, *cbox2;
    const int *len1, *len2;
    const unsigned *rec1, *rec2;  // self: rec2 == rec1 and direction 2 of (i, j) is direction 1 of (j, i)
    int self;
    float *out;
};

// the integer sum_k t[k] * 2^(26 k) on the grid of eref, divided by the count.  Integers and one fixed sequence of double
// operations: the same bits whoever added the limbs up.  A single term (count 1, nothing truncated) comes back exactly.
__device__ __forceinline__ float cx_mean(const unsigned long long (&t)[CX_LIMBS], int eref, int count) {
    double v = 0.0;
#pragma unroll
    for (int k = CX_LIMBS - 1; k >= 0; k--) v = v * (double)(1u << CX_LIMB_BITS) + (double)t[k];
    return (float)(ldexp(v, eref - CX_FIX) / (double)count);
}

// one wave per (pair, direction); grid (ceil(2 r / CX_WAVES), s)
__global__ __launch_bounds__(CX_WAVES * 64) void chamfer_cross_reduce_kernel(CxReduce a) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * CX_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= 2 * a.r) return;
    const int i = blockIdx.y, j = w >> 1, dir = w & 1;
    const int nsb = dir && !a.self ? a.nsb2 : a.nsb1;
    const size_t pair = dir && a.self ? (size_t)j * a.r + i : (size_t)i * a.r + j;
    const unsigned *__restrict__ rp = (dir ? a.rec2 : a.rec1) + pair * nsb * CX_REC;
    unsigned long long td[CX_LIMBS] = {0, 0, 0, 0, 0}, ts[CX_LIMBS] = {0, 0, 0, 0, 0};
    unsigned mx = 0u;
    for (int g = lane; g < nsb; g += 64) {
        const uint4 x = *(const uint4 *)(rp + (size_t)g * CX_REC), y = *(const uint4 *)(rp + (size_t)g * CX_REC + 4),
                    z = *(const uint4 *)(rp + (size_t)g * CX_REC + 8);
        td[0] += x.x, td[1] += x.y, td[2] += x.z, td[3] += x.w, td[4] += y.x;
        ts[0] += y.y, ts[1] += y.z, ts[2] += y.w, ts[3] += z.x, ts[4] += z.y;
        mx = max(mx, z.z);
    }
#pragma unroll
    for (int k = 0; k < CX_LIMBS; k++) {
        td[k] = rf::wave_sum(td[k]);
        ts[k] = rf::wave_sum(ts[k]);
    }
    mx = rf::wave_max_u32(mx);
    if (lane == 0) {
        const int e1 = cx_pair_exp(a.cbox1 + (size_t)i * 8, a.cbox2 + (size_t)j * 8);
        const int L = dir ? rf::ragged_count(a.len2, j, a.m) : rf::ragged_count(a.len1, i, a.n);
        float *__restrict__ o = a.out + ((size_t)i * a.r + j) * RF_CX_NCOL;
        o[0 + dir] = cx_mean(ts, cx_sqrt_exp(e1), L);
        o[2 + dir] = cx_mean(td, e1, L);
        o[4 + dir] = __uint_as_float(mx);
    }
}

size_t cx_rec_bytes(int s, int r, int npad) { return (size_t)s * (size_t)r * (size_t)(npad / 64) * CX_REC * sizeof(unsigned); }

// sorted(s, n) | sorted(r, m) | cloud boxes (s + r, 8) | records of direction 1 | records of direction 2
struct CxLayout {
    size_t sorted1, sorted2, cbox, rec1, rec2, total;
};
CxLayout cx_layout(int s, int r, int n, int m) {
    rf::Layout w;
    CxLayout l;
    l.sorted1 = w.add(rfp::sorted_bytes(s, n));
    l.sorted2 = w.add(rfp::sorted_bytes(r, m));
    l.cbox = w.add(((size_t)s + (size_t)r) * 8 * sizeof(float));
    l.rec1 = w.add(cx_rec_bytes(s, r, rfp::sorted_npad(n)));
    l.rec2 = w.add(cx_rec_bytes(s, r, rfp::sorted_npad(m)));
    l.total = w.total;
    return l;
}

}  // namespace

extern "C" {

size_t rf_chamfer_cross_workspace_bytes(int s, int r, int n, int m) {
    if (s <= 0 || r <= 0 || n <= 0 || m <= 0 || n > rfp::kMaxPoints || m > rfp::kMaxPoints) return 0;
    return cx_layout(s, r, n, m).total;
}

int rf_chamfer_cross(int s, int r, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2,
                     float *out, void *workspace, size_t workspace_bytes, rf_stream_t stream) {
    if (s < 0 || r < 0 || n < 0 || m < 0) return RF_EINVAL;
    if (s == 0 || r == 0) return RF_OK;
    if (n < 1 || m < 1 || n > rfp::kMaxPoints || m > rfp::kMaxPoints || s > 65535 || r > 65535) return RF_EINVAL;
    if (!rf::tensors_ok({xyz1, xyz2, out}, {len1, len2}) || !rf::workspace_ok(workspace)) return RF_EINVAL;
    const CxLayout l = cx_layout(s, r, n, m);
    if (workspace_bytes < l.total) return RF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;

    const bool self = xyz1 == xyz2 && len1 == len2 && s == r && n == m;
    char *w = (char *)workspace;
    const rfp::Sorted s1 = rfp::sorted_view(s, n, w + l.sorted1);
    const rfp::Sorted s2 = self ? s1 : rfp::sorted_view(r, m, w + l.sorted2);
    float *cbox = (float *)(w + l.cbox);
    unsigned *rec1 = (unsigned *)(w + l.rec1);
    unsigned *rec2 = self ? rec1 : (unsigned *)(w + l.rec2);

    // the sorts: each collection once, with its counts; no ball query reads these sets (flag = false)
    if (int e = rfp::sort_sets(s, 1, &n, &xyz1, &s1, st, nullptr, len1 ? &len1 : nullptr, false)) return e;
    if (!self)
        if (int e = rfp::sort_sets(r, 1, &m, &xyz2, &s2, st, nullptr, len2 ? &len2 : nullptr, false)) return e;

    const int nsb1 = s1.npad / 64, nsb2 = s2.npad / 64;
    float *cbox2 = self ? cbox : cbox + (size_t)s * 8;
    RF_LAUNCH("chamfer_cross_boxes", chamfer_cross_boxes_kernel, dim3(self ? s : s + r), dim3(64), 0, st, s1.box64, s, nsb1,
              s2.box64, nsb2, cbox);

    const CxSide a{s1.xyz, s1.orig, s1.box16, s1.box64, cbox, len1, s, n, nsb1};
    const CxSide b{s2.xyz, s2.orig, s2.box16, s2.box64, cbox2, len2, r, m, nsb2};
    {
        const unsigned gx = (unsigned)rf::ceil_div(nsb1, CX_WAVES) * (unsigned)rf::ceil_div(r, CX_STRIP);
        RF_LAUNCH("chamfer_cross_sweep", chamfer_cross_sweep_kernel<0>, dim3(gx, s), dim3(CX_WAVES * 64), 0, st, a, b, rec1);
    }
    if (!self) {  // (self: direction 2 of (i, j) is direction 1 of (j, i), bit for bit -- the sums have no order)
        const unsigned gx = (unsigned)rf::ceil_div(nsb2, CX_WAVES) * (unsigned)rf::ceil_div(s, CX_STRIP);
        RF_LAUNCH("chamfer_cross_sweep", chamfer_cross_sweep_kernel<1>, dim3(gx, r), dim3(CX_WAVES * 64), 0, st, b, a, rec2);
    }
    const CxReduce ra{s, r, n, m, nsb1, nsb2, cbox, cbox2, len1, len2, rec1, rec2, self ? 1 : 0, out};
    RF_LAUNCH("chamfer_cross_reduce", chamfer_cross_reduce_kernel, dim3(rf::ceil_div(2L * r, CX_WAVES), s),
              dim3(CX_WAVES * 64), 0, st, ra);
    return RF_OK;
}

}  // extern "C"
