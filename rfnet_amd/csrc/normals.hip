// normals.hip -- surface normals by PCA of every point's k-neighbourhood, and the normal consistency of two clouds.
// include/rfops.h states the contract ("surface normals"); DESIGN.md 5.3r the measurements.
//
//   rf_local_pca              per query the eigen-decomposition of the covariance of the points its idx row names
//   rf_nn_normal_consistency  the means of |n1 . n2[idx1]| and n1 . n2[idx1] in both directions
//
// rf_local_pca is one lane per query: the covariance (6 doubles) and the eigenvectors (9) live in registers, the
// cyclic Jacobi sweeps are fully unrolled, and every double operation is the one the header spells (-ffp-contract=off:
// no product is fused into a sum).  The workgroup's block of idx rows is contiguous in memory; it is staged in LDS with
// coalesced loads and each lane then walks its own row there, twice (the mean, then the centred products): a lane's
// own loads from idx would be 64 rows apart.  The points are gathered from global memory both times (a sample's
// workgroups sit on one XCD, so the second gather is an L2 hit at worst).
#include <initializer_list>

#include "lane_rows.hpp"

namespace {

constexpr int PCA_TPB = 256;
constexpr int PCA_MAX_K = RF_PCA_MAX_K;

struct PcaArgs {
    int n, m, k;
    const float *xyz;
    const int *idx, *len1, *len2;
    const float *viewpoint;
    float *normals, *eigenvalues, *axes;
};

// Steps 3-5 are __host__ too: compiled for the host they are the same IEEE operations, so the arithmetic can be held to the
// numpy restatement (tests/test_normals_host.py) bit for bit where there is no GPU.
// One Jacobi rotation of the pair (p, q), r the third index, on the symmetric A and the columns p, q of V (rfops.h step 3).
__host__ __device__ __forceinline__ void pca_rotate(double &app, double &aqq, double &apq, double &arp, double &arq,
                                                    double &v0p, double &v0q, double &v1p, double &v1q, double &v2p,
                                                    double &v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp, arq = rq;
    const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
    const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
    const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
    v0p = a0, v0q = b0, v1p = a1, v1q = b1, v2p = a2, v2q = b2;
}

// (value, vector) pairs in ascending order of (value, original position): a strict compare keeps equal values in place
__host__ __device__ __forceinline__ void pca_order(double &wa, double &wb, double &xa, double &ya, double &za, double &xb,
                                                   double &yb, double &zb) {
    if (wa > wb) {
        double t;
        t = wa, wa = wb, wb = t;
        t = xa, xa = xb, xb = t;
        t = ya, ya = yb, yb = t;
        t = za, za = zb, zb = t;
    }
}

// the canonical sign: the component of largest magnitude positive, a tie to the lowest axis, a zero vector as it is
__host__ __device__ __forceinline__ void pca_sign(double &x, double &y, double &z) {
    double lead = x;
    if (fabs(y) > fabs(lead)) lead = y;
    if (fabs(z) > fabs(lead)) lead = z;
    if (lead < 0.0) x = -x, y = -y, z = -z;
}

// Steps 3-5 of rfops.h without the viewpoint: six cyclic sweeps on the symmetric A, the eigenpairs in ascending order of
// (value, position) as (w, (x, y, z)), every vector with the canonical sign.
__host__ __device__ __forceinline__ void pca_eigen(double a00, double a01, double a02, double a11, double a12, double a22,
                                                   double &w0, double &w1, double &w2, double &x0, double &y0, double &z0,
                                                   double &x1, double &y1, double &z1, double &x2, double &y2, double &z2) {
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll
    for (int sweep = 0; sweep < 6; sweep++) {
        pca_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), r = 2
        pca_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
        pca_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
    }
    // eigenvalue w is A_ww, its vector column w of V; three compare-and-swaps of neighbours sort them by (value, w)
    w0 = a00, w1 = a11, w2 = a22;
    x0 = v00, y0 = v10, z0 = v20, x1 = v01, y1 = v11, z1 = v21, x2 = v02, y2 = v12, z2 = v22;
    pca_order(w0, w1, x0, y0, z0, x1, y1, z1);
    pca_order(w1, w2, x1, y1, z1, x2, y2, z2);
    pca_order(w0, w1, x0, y0, z0, x1, y1, z1);
    pca_sign(x0, y0, z0);
    pca_sign(x1, y1, z1);
    pca_sign(x2, y2, z2);
}

__global__ __launch_bounds__(PCA_TPB) void local_pca_kernel(PcaArgs a, int bpb) {
    extern __shared__ int pca_idx[];  // [rows of this workgroup][k | 1]: an odd stride, the lanes' rows on distinct banks
    int bi, bx;
    rf::place_1d(bpb, bi, bx);
    const int k = a.k, stride = k | 1;
    const int L1 = rf::ragged_count(a.len1, bi, a.n), L2 = rf::ragged_count(a.len2, bi, a.m);
    const int j0 = bx * PCA_TPB, j = j0 + (int)threadIdx.x;
    // the idx rows of this workgroup's valid queries: one contiguous block of `rows * k` ints
    const int rows = min(PCA_TPB, L2 - j0);
    if (rows > 0) {
        const int *__restrict__ src = a.idx + ((size_t)bi * a.m + j0) * k;
        for (int e = threadIdx.x; e < rows * k; e += PCA_TPB) {
            const int r = e / k;
            pca_idx[r * stride + (e - r * k)] = src[e];
        }
    }
    __syncthreads();
    if (j >= a.m) return;
    const size_t q = (size_t)bi * a.m + j;
    float *__restrict__ nrm = a.normals + q * 3;
    float *__restrict__ eig = a.eigenvalues + q * 3;
    float *__restrict__ axes = a.axes ? a.axes + q * 9 : nullptr;
    if (j >= L2) {  // a padded query: zeros
        for (int c = 0; c < 3; c++) nrm[c] = 0.f, eig[c] = 0.f;
        if (axes)
            for (int c = 0; c < 9; c++) axes[c] = 0.f;
        return;
    }
    const int kv = min(k, L1);
    const int *__restrict__ row = pca_idx + threadIdx.x * stride;
    const float *__restrict__ pts = a.xyz + (size_t)bi * a.n * 3;
    // A skipped slot adds +0.0: the sums start at +0.0 and a sum of doubles that started there is never -0.0, so adding +0.0
    // is the identity on them, NaN and inf included -- the loads of a trip stay unconditional (at row 0, which exists).
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int used = 0;
#pragma unroll 4
    for (int t = 0; t < kv; t++) {
        const int i = row[t];
        const bool ok = (unsigned)i < (unsigned)L1;
        const float *__restrict__ p = pts + (size_t)(ok ? i : 0) * 3;
        const float x = p[0], y = p[1], z = p[2];
        sx = sx + (ok ? (double)x : 0.0);
        sy = sy + (ok ? (double)y : 0.0);
        sz = sz + (ok ? (double)z : 0.0);
        used += ok;
    }
    const double cnt = (double)used;
    const double mx = sx / cnt, my = sy / cnt, mz = sz / cnt;
    double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
#pragma unroll 4
    for (int t = 0; t < kv; t++) {
        const int i = row[t];
        const bool ok = (unsigned)i < (unsigned)L1;
        const float *__restrict__ p = pts + (size_t)(ok ? i : 0) * 3;
        const double dx = (double)p[0] - mx, dy = (double)p[1] - my, dz = (double)p[2] - mz;
        cxx = cxx + (ok ? dx * dx : 0.0);
        cxy = cxy + (ok ? dx * dy : 0.0);
        cxz = cxz + (ok ? dx * dz : 0.0);
        cyy = cyy + (ok ? dy * dy : 0.0);
        cyz = cyz + (ok ? dy * dz : 0.0);
        czz = czz + (ok ? dz * dz : 0.0);
    }
    double a00 = cxx / cnt, a01 = cxy / cnt, a02 = cxz / cnt, a11 = cyy / cnt, a12 = cyz / cnt, a22 = czz / cnt;
    const bool finite = used > 0 && isfinite(a00) && isfinite(a01) && isfinite(a02) && isfinite(a11) && isfinite(a12) &&
                        isfinite(a22);
    if (!finite) {  // a non-finite neighbourhood: canonical quiet NaNs, a zero frame
        const float qnan = __uint_as_float(0x7fc00000u);
        for (int c = 0; c < 3; c++) nrm[c] = 0.f, eig[c] = qnan;
        if (axes)
            for (int c = 0; c < 9; c++) axes[c] = 0.f;
        return;
    }
    double w0, w1, w2, x0, y0, z0, x1, y1, z1, x2, y2, z2;
    pca_eigen(a00, a01, a02, a11, a12, a22, w0, w1, w2, x0, y0, z0, x1, y1, z1, x2, y2, z2);
    if (a.viewpoint) {
        const float *__restrict__ vp = a.viewpoint + (size_t)bi * 3;
        const double side = (((double)vp[0] - mx) * x0 + ((double)vp[1] - my) * y0) + ((double)vp[2] - mz) * z0;
        if (side < 0.0) x0 = -x0, y0 = -y0, z0 = -z0;
    }
    nrm[0] = (float)x0, nrm[1] = (float)y0, nrm[2] = (float)z0;
    eig[0] = (float)w0, eig[1] = (float)w1, eig[2] = (float)w2;
    if (axes) {
        axes[0] = (float)x0, axes[1] = (float)y0, axes[2] = (float)z0;
        axes[3] = (float)x1, axes[4] = (float)y1, axes[5] = (float)z1;
        axes[6] = (float)x2, axes[7] = (float)y2, axes[8] = (float)z2;
    }
}

// ---- normal consistency: one workgroup per (sample, direction), chamfer_metrics.hip's reduction shape in double
constexpr int NC_TPB = 1024;
constexpr int NC_NW = NC_TPB / 64;
constexpr int NC_U = 4;  // points per thread and trip, each into a partial sum of its own

struct NcArgs {
    int n, m;
    const float *nrm1, *nrm2;
    const int *idx1, *idx2, *len1, *len2;
    float *out;
};

__global__ __launch_bounds__(NC_TPB) void normal_consistency_kernel(NcArgs a) {
    __shared__ double part[2][NC_NW];
    const int tid = threadIdx.x;
    const int bi = blockIdx.x >> 1, dir = blockIdx.x & 1;
    const int full = dir ? a.m : a.n, other = dir ? a.n : a.m;
    const int L = rf::ragged_count(dir ? a.len2 : a.len1, bi, full);
    const int Lo = rf::ragged_count(dir ? a.len1 : a.len2, bi, other);
    const float *__restrict__ own = (dir ? a.nrm2 : a.nrm1) + (size_t)bi * full * 3;
    const float *__restrict__ oth = (dir ? a.nrm1 : a.nrm2) + (size_t)bi * other * 3;
    const int *__restrict__ ix = (dir ? a.idx2 : a.idx1) + (size_t)bi * full;
    double sa[NC_U] = {0.0, 0.0, 0.0, 0.0}, ss[NC_U] = {0.0, 0.0, 0.0, 0.0};
    for (int j = tid; j < L; j += NC_U * NC_TPB) {
#pragma unroll
        for (int u = 0; u < NC_U; u++) {
            const int jj = j + u * NC_TPB;
            const int i = jj < L ? ix[jj] : -1;
            const bool ok = (unsigned)i < (unsigned)Lo;  // (a slot behind the count is not read; an index outside: +0)
            const float *__restrict__ p = own + (size_t)(ok ? jj : 0) * 3;
            const float *__restrict__ o = oth + (size_t)(ok ? i : 0) * 3;
            const float px = p[0], py = p[1], pz = p[2], ox = o[0], oy = o[1], oz = o[2];
            const bool zero = (px == 0.f && py == 0.f && pz == 0.f) || (ox == 0.f && oy == 0.f && oz == 0.f);
            double d = ((double)px * (double)ox + (double)py * (double)oy) + (double)pz * (double)oz;
            d = ok && !zero ? d : 0.0;
            sa[u] += fabs(d);
            ss[u] += d;
        }
    }
    auto add = [](double x, double y) { return x + y; };
    const double wa = rf::wave_reduce((sa[0] + sa[1]) + (sa[2] + sa[3]), add);
    const double ws = rf::wave_reduce((ss[0] + ss[1]) + (ss[2] + ss[3]), add);
    if ((tid & 63) == 0) part[0][tid >> 6] = wa, part[1][tid >> 6] = ws;
    __syncthreads();
    if (tid == 0) {
        double ta = part[0][0], ts = part[1][0];
#pragma unroll
        for (int w = 1; w < NC_NW; w++) ta += part[0][w], ts += part[1][w];
        float *__restrict__ out = a.out + (size_t)bi * 4;
        out[0 + dir] = (float)(ta / (double)L);
        out[2 + dir] = (float)(ts / (double)L);
    }
}

}  // namespace

extern "C" {

int rf_local_pca(int b, int n, int m, int k, const float *xyz, const int *idx, const int *len1, const int *len2,
                 const float *viewpoint, float *normals, float *eigenvalues, float *axes, rf_stream_t stream) {
    if (b == 0) return RF_OK;
    if (b < 0 || b > 65535 || n < 1 || n > 65536 || m < 1 || m > 65536 || k < 1 || k > PCA_MAX_K) return RF_EINVAL;
    if (!rf::tensors_ok({xyz, idx, normals, eigenvalues}, {len1, len2, viewpoint, axes})) return RF_EINVAL;
    const int bpb = rf::ceil_div(m, PCA_TPB);
    const PcaArgs a{n, m, k, xyz, idx, len1, len2, viewpoint, normals, eigenvalues, axes};
    if (int dv = rf::require_device()) return dv;
    // (at most PCA_TPB * 65 ints = 65 KiB: above the 64 KiB a kernel gets without asking)
    RF_HIP(hipFuncSetAttribute((const void *)local_pca_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               PCA_TPB * (PCA_MAX_K | 1) * (int)sizeof(int)));
    RF_LAUNCH("local_pca", local_pca_kernel, dim3((unsigned)bpb * (unsigned)b), dim3(PCA_TPB),
              sizeof(int) * (size_t)PCA_TPB * (k | 1), (hipStream_t)stream, a, bpb);
    return RF_OK;
}

int rf_nn_normal_consistency(int b, int n, int m, const float *nrm1, const float *nrm2, const int *idx1, const int *idx2,
                             const int *len1, const int *len2, float *out, rf_stream_t stream) {
    if (b == 0) return RF_OK;
    if (b < 0 || n < 1 || m < 1 || b > 65535) return RF_EINVAL;
    if (!rf::tensors_ok({nrm1, nrm2, idx1, idx2, out}, {len1, len2})) return RF_EINVAL;
    const NcArgs a{n, m, nrm1, nrm2, idx1, idx2, len1, len2, out};
    RF_LAUNCH("nn_normal_consistency", normal_consistency_kernel, dim3(2 * b), dim3(NC_TPB), 0, (hipStream_t)stream, a);
    return RF_OK;
}

}  // extern "C"
