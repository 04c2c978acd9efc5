// Per-point attributes on the upsampled cloud (puflow_amd/attributes.py; the reference has no counterpart).
//   pf_attr_blend / _ragged  - the columns a scan carries after x y z, moved to the output points: every output point blends
//                              the rows of its K nearest input points (pf_knn_large's idx / d2) by inverse squared distance,
//                              column segment by column segment (lin / unit / near).
//   pf_normals_pca / _ragged - a normal per output point from the covariance of its own K-neighbourhood: moments and a cyclic
//                              Jacobi solve in double, rounded to float32 once, oriented to a viewpoint or away from the centroid.
// One lane per point, no LDS in the per-point kernels, no atomics, no barrier across workgroups: every point is independent (the
// neighbour search in front of these kernels costs orders of magnitude more).  A cloud's rows depend on nothing but the cloud:
// the dense and the ragged kernels inline the same per-point functions.  All stores are plain vector stores.
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"

namespace {

constexpr int AT_T = 256;
constexpr int AT_MAXB = 64;                 // clouds per ragged launch (their tables travel as kernel arguments)

struct AttrPlan {                           // the column segments, in column order
    int nseg;
    unsigned char kind[PF_ATTR_MAX_C], start[PF_ATTR_MAX_C], cols[PF_ATTR_MAX_C];
};

// one output point: its K neighbours irow / drow (ordered by distance) in the cloud's attribute rows attr [N,C] -> orow [C]
__device__ __forceinline__ void attr_blend_point(const int* __restrict__ irow, const float* __restrict__ drow,
                                                 const float* __restrict__ attr, int N, int K, int C, const AttrPlan& plan,
                                                 float* __restrict__ orow) {
    int id[PF_ATTR_MAX_K];
    float w[PF_ATTR_MAX_K];
#pragma unroll
    for (int k = 0; k < PF_ATTR_MAX_K; ++k) {
        const int j = k < K ? irow[k] : 0;
        id[k] = (unsigned)j < (unsigned)N ? j : 0;                         // an index from elsewhere never reads out of bounds
        w[k] = 0.f;
    }
    const float* a0 = attr + (size_t)id[0] * C;
    const float d0 = drow[0];
    if (!(d0 > 0.f)) {                                                     // the point IS input point id[0]: its row, bit for bit
        for (int c = 0; c < C; ++c) orow[c] = a0[c];
        return;
    }
    // w_k = (1 / d2_k) / sum_j (1 / d2_j), formed as d2_0 / d2_k so that a denormal distance cannot overflow: w_0 = 1 >= w_k
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < PF_ATTR_MAX_K; ++k)
        if (k < K) { w[k] = __fdiv_rn(d0, drow[k]); s = __fadd_rn(s, w[k]); }
    const float r = __fdiv_rn(1.f, s);
#pragma unroll
    for (int k = 0; k < PF_ATTR_MAX_K; ++k) w[k] = __fmul_rn(w[k], r);
    for (int g = 0; g < plan.nseg; ++g) {
        const int c0 = plan.start[g], nc = plan.cols[g];
        if (plan.kind[g] == PF_ATTR_NEAR) {
            for (int c = c0; c < c0 + nc; ++c) orow[c] = a0[c];
        } else if (plan.kind[g] == PF_ATTR_LIN) {
            for (int c = c0; c < c0 + nc; ++c) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < PF_ATTR_MAX_K; ++k)
                    if (k < K) acc = fmaf(w[k], attr[(size_t)id[k] * C + c], acc);
                orow[c] = acc;
            }
        } else {                                                           // PF_ATTR_UNIT: 3 columns, a direction up to sign
            const float x0 = a0[c0], y0 = a0[c0 + 1], z0 = a0[c0 + 2];
            float bx = 0.f, by = 0.f, bz = 0.f;
#pragma unroll
            for (int k = 0; k < PF_ATTR_MAX_K; ++k)
                if (k < K) {
                    const float* a = attr + (size_t)id[k] * C + c0;
                    const float x = a[0], y = a[1], z = a[2];
                    const float dot = fmaf(z, z0, fmaf(y, y0, __fmul_rn(x, x0)));
                    const float ws = dot < 0.f ? -w[k] : w[k];             // flipped to neighbour 0's side
                    bx = fmaf(ws, x, bx); by = fmaf(ws, y, by); bz = fmaf(ws, z, bz);
                }
            const float len = __fsqrt_rn(fmaf(bz, bz, fmaf(by, by, __fmul_rn(bx, bx))));
            if (len > 0.f && len <= 3.4028234663852886e38f) {
                orow[c0] = __fdiv_rn(bx, len); orow[c0 + 1] = __fdiv_rn(by, len); orow[c0 + 2] = __fdiv_rn(bz, len);
            } else {                                                       // nothing to normalise: neighbour 0's vector as it is
                orow[c0] = x0; orow[c0 + 1] = y0; orow[c0 + 2] = z0;
            }
        }
    }
}

__global__ __launch_bounds__(AT_T) void attr_blend_kernel(const int* __restrict__ idx, const float* __restrict__ d2,
                                                          const float* __restrict__ attr, long long total, int N, int M, int K,
                                                          int C, const AttrPlan plan, float* __restrict__ out) {
    const long long q = (long long)blockIdx.x * AT_T + threadIdx.x;
    if (q >= total) return;
    const long long b = q / M;
    attr_blend_point(idx + (size_t)q * K, d2 + (size_t)q * K, attr + (size_t)b * N * C, N, K, C, plan, out + (size_t)q * C);
}

struct AttrRaggedTab {
    int roff[AT_MAXB];                      // first input point of the cloud
    int n[AT_MAXB];                         // its input points
    int q0[AT_MAXB + 1];                    // its first output point (outputs of all clouds are stored back to back)
};
static_assert(sizeof(AttrRaggedTab) + sizeof(AttrPlan) + 128 <= 4096, "the kernel argument block");

__global__ __launch_bounds__(AT_T) void attr_blend_ragged_kernel(const int* __restrict__ idx, const float* __restrict__ d2,
                                                                 const float* __restrict__ attr, const AttrRaggedTab t, int nc,
                                                                 int K, int C, const AttrPlan plan, float* __restrict__ out) {
    const long long q = (long long)t.q0[0] + (long long)blockIdx.x * AT_T + threadIdx.x;
    if (q >= t.q0[nc]) return;
    int c = 0;
    while (c + 1 < nc && q >= t.q0[c + 1]) ++c;
    attr_blend_point(idx + (size_t)q * K, d2 + (size_t)q * K, attr + (size_t)t.roff[c] * C, t.n[c], K, C, plan,
                     out + (size_t)q * C);
}

// ---- PCA normals ----------------------------------------------------------------------------------------------------------
// The centroid of one cloud in double with a fixed order (thread t adds points t, t + 256, ... in order, then a binary tree):
// the orientation reference when no viewpoint is given.  One workgroup per cloud.
__device__ __forceinline__ void centroid_body(const float* __restrict__ p, int M, double* __restrict__ cen) {
    __shared__ double red[3][AT_T];
    const int tid = threadIdx.x;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int i = tid; i < M; i += AT_T) { sx += (double)p[(size_t)i * 3]; sy += (double)p[(size_t)i * 3 + 1]; sz += (double)p[(size_t)i * 3 + 2]; }
    red[0][tid] = sx; red[1][tid] = sy; red[2][tid] = sz;
    __syncthreads();
    for (int s = AT_T / 2; s > 0; s >>= 1) {
        if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; red[2][tid] += red[2][tid + s]; }
        __syncthreads();
    }
    if (tid == 0) { cen[0] = red[0][0] / M; cen[1] = red[1][0] / M; cen[2] = red[2][0] / M; }
}

__global__ __launch_bounds__(AT_T) void centroid_kernel(const float* __restrict__ pts, int M, double* __restrict__ cen) {
    centroid_body(pts + (size_t)blockIdx.x * M * 3, M, cen + (size_t)blockIdx.x * 3);
}

struct NrmTab { int off[AT_MAXB + 1]; };                                   // cloud c = points [off[c], off[c + 1])

__global__ __launch_bounds__(AT_T) void centroid_ragged_kernel(const float* __restrict__ pts, const NrmTab t,
                                                               double* __restrict__ cen) {
    const int c = blockIdx.x;
    centroid_body(pts + (size_t)t.off[c] * 3, t.off[c + 1] - t.off[c], cen + (size_t)c * 3);
}

// one Jacobi rotation of the symmetric 3x3 matrix a (p < q) that zeroes a[p][q]; v collects the rotations (columns = vectors)
__device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3], int p, int q) {
    const double apq = a[p][q];
    if (apq == 0.0) return;
    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const int r = 3 - p - q;
    a[p][p] -= t * apq; a[q][q] += t * apq;
    a[p][q] = a[q][p] = 0.0;
    const double arp = a[r][p], arq = a[r][q];
    a[r][p] = a[p][r] = c * arp - s * arq;
    a[r][q] = a[q][r] = s * arp + c * arq;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double vp = v[i][p], vq = v[i][q];
        v[i][p] = c * vp - s * vq;
        v[i][q] = s * vp + c * vq;
    }
}

constexpr int PCA_SWEEPS = 8;               // cyclic Jacobi converges quadratically: a 3x3 is at rounding level after 4 - 5

// one point p of the cloud pts [M,3] with its K neighbours irow; (rx, ry, rz): the viewpoint (toward: the normal looks at it) or
// the cloud's centroid (the normal looks away from it)
__device__ __forceinline__ void normal_point(const float* __restrict__ pts, int M, const int* __restrict__ irow, int K,
                                             const float* __restrict__ p, bool toward, double rx, double ry, double rz,
                                             float* __restrict__ nrow, float* __restrict__ vrow) {
    double mx = 0.0, my = 0.0, mz = 0.0;
    for (int k = 0; k < K; ++k) {
        int j = irow[k];
        j = (unsigned)j < (unsigned)M ? j : 0;
        mx += (double)pts[(size_t)j * 3]; my += (double)pts[(size_t)j * 3 + 1]; mz += (double)pts[(size_t)j * 3 + 2];
    }
    mx /= K; my /= K; mz /= K;
    double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
    for (int k = 0; k < K; ++k) {
        int j = irow[k];
        j = (unsigned)j < (unsigned)M ? j : 0;
        const double dx = (double)pts[(size_t)j * 3] - mx, dy = (double)pts[(size_t)j * 3 + 1] - my, dz = (double)pts[(size_t)j * 3 + 2] - mz;
        xx += dx * dx; xy += dx * dy; xz += dx * dz; yy += dy * dy; yz += dy * dz; zz += dz * dz;
    }
    const double tr = xx + yy + zz;
    if (!(tr > 0.0) || !(tr <= 1.7976931348623157e308)) {                  // all moments 0 (or not finite): no plane to fit
        nrow[0] = 0.f; nrow[1] = 0.f; nrow[2] = 1.f; vrow[0] = 0.f;
        return;
    }
    const double sc = 1.0 / tr;                                            // eigenvalues of the scaled matrix sum to 1
    double a[3][3] = {{xx * sc, xy * sc, xz * sc}, {xy * sc, yy * sc, yz * sc}, {xz * sc, yz * sc, zz * sc}};
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < PCA_SWEEPS; ++sweep) {
        jacobi_rotate(a, v, 0, 1);
        jacobi_rotate(a, v, 0, 2);
        jacobi_rotate(a, v, 1, 2);
    }
    const double l0 = a[0][0], l1 = a[1][1], l2 = a[2][2];
    double lam, nx, ny, nz;                                                 // the smallest eigenvalue (lowest index wins ties)
    if (l0 <= l1 && l0 <= l2) { lam = l0; nx = v[0][0]; ny = v[1][0]; nz = v[2][0]; }
    else if (l1 <= l2) { lam = l1; nx = v[0][1]; ny = v[1][1]; nz = v[2][1]; }
    else { lam = l2; nx = v[0][2]; ny = v[1][2]; nz = v[2][2]; }
    const double inv = 1.0 / sqrt(nx * nx + ny * ny + nz * nz);
    nx *= inv; ny *= inv; nz *= inv;
    double ox = rx - (double)p[0], oy = ry - (double)p[1], oz = rz - (double)p[2];      // the direction the normal has to agree with
    if (!toward) { ox = -ox; oy = -oy; oz = -oz; }
    if (nx * ox + ny * oy + nz * oz < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    const double var = lam / (l0 + l1 + l2);
    nrow[0] = (float)nx; nrow[1] = (float)ny; nrow[2] = (float)nz;
    vrow[0] = (float)fmin(fmax(var, 0.0), 1.0 / 3.0);
}

struct View { double x, y, z; int given; };

__global__ __launch_bounds__(AT_T) void normals_pca_kernel(const float* __restrict__ pts, const int* __restrict__ idx,
                                                           long long total, int M, int K, const View view,
                                                           const double* __restrict__ cen, float* __restrict__ normal,
                                                           float* __restrict__ variation) {
    const long long q = (long long)blockIdx.x * AT_T + threadIdx.x;
    if (q >= total) return;
    const long long b = q / M;
    const bool g = view.given != 0;
    const double* c3 = cen + (size_t)b * 3;                                 // read only without a viewpoint
    normal_point(pts + (size_t)b * M * 3, M, idx + (size_t)q * K, K, pts + (size_t)q * 3, g, g ? view.x : c3[0], g ? view.y : c3[1],
                 g ? view.z : c3[2], normal + (size_t)q * 3, variation + q);
}

__global__ __launch_bounds__(AT_T) void normals_pca_ragged_kernel(const float* __restrict__ pts, const int* __restrict__ idx,
                                                                  const NrmTab t, int nc, int K, const View view,
                                                                  const double* __restrict__ cen, float* __restrict__ normal,
                                                                  float* __restrict__ variation) {
    const long long q = (long long)t.off[0] + (long long)blockIdx.x * AT_T + threadIdx.x;
    if (q >= t.off[nc]) return;
    int c = 0;
    while (c + 1 < nc && q >= t.off[c + 1]) ++c;
    const bool g = view.given != 0;
    const double* c3 = cen + (size_t)c * 3;                                 // read only without a viewpoint
    normal_point(pts + (size_t)t.off[c] * 3, t.off[c + 1] - t.off[c], idx + (size_t)q * K, K, pts + (size_t)q * 3, g,
                 g ? view.x : c3[0], g ? view.y : c3[1], g ? view.z : c3[2], normal + (size_t)q * 3, variation + q);
}

// the column plan of the ABI (host arrays) -> the kernels' argument; PF_OK or the error the entry point returns
int make_plan(const int* seg_kind, const int* seg_cols, int nseg, int C, AttrPlan* plan) {
    if (C < 1 || C > PF_ATTR_MAX_C) return PF_ERR_UNSUPPORTED;
    if (nseg < 1 || nseg > PF_ATTR_MAX_C) return PF_ERR_SHAPE;
    int c = 0;
    for (int g = 0; g < nseg; ++g) {
        const int kind = seg_kind[g], n = seg_cols[g];
        if (kind != PF_ATTR_LIN && kind != PF_ATTR_UNIT && kind != PF_ATTR_NEAR) return PF_ERR_UNSUPPORTED;
        if (n < 1 || n > C - c || (kind == PF_ATTR_UNIT && n != 3)) return PF_ERR_SHAPE;
        plan->kind[g] = (unsigned char)kind; plan->start[g] = (unsigned char)c; plan->cols[g] = (unsigned char)n;
        c += n;
    }
    if (c != C) return PF_ERR_SHAPE;
    plan->nseg = nseg;
    return PF_OK;
}

View make_view(const float* viewpoint) {
    View v = {0.0, 0.0, 0.0, 0};
    if (viewpoint) { v.x = viewpoint[0]; v.y = viewpoint[1]; v.z = viewpoint[2]; v.given = 1; }
    return v;
}

constexpr long long AT_MAX_ROWS = 0x7fffffffll / 64;                       // rows x (K <= 64 | C <= 16 | 3) stays an int anywhere

}  // namespace

extern "C" int pf_attr_blend(const int* idx, const float* d2, const float* attr, int B, int N, int M, int K, int C,
                             const int* seg_kind, const int* seg_cols, int nseg, float* out, void* stream) {
    if (!idx || !d2 || !attr || !seg_kind || !seg_cols || !out) return PF_ERR_NULL;
    if (K < 1 || K > PF_ATTR_MAX_K) return PF_ERR_UNSUPPORTED;
    AttrPlan plan = {};
    const int rc = make_plan(seg_kind, seg_cols, nseg, C, &plan);
    if (rc != PF_OK) return rc;
    if (B <= 0 || N <= 0 || M <= 0 || K > N) return PF_ERR_SHAPE;
    const long long total = (long long)B * M;
    if (total > AT_MAX_ROWS || (long long)B * N > AT_MAX_ROWS) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(attr_blend_kernel, dim3((unsigned)((total + AT_T - 1) / AT_T)), dim3(AT_T), 0, (hipStream_t)stream, idx, d2,
                       attr, total, N, M, K, C, plan, out);
    return pf_last_launch_status();
}

extern "C" int pf_attr_blend_ragged(const int* idx, const float* d2, const float* attr, const int* n, const int* m, int B, int K,
                                    int C, const int* seg_kind, const int* seg_cols, int nseg, float* out, void* stream) {
    if (!idx || !d2 || !attr || !n || !m || !seg_kind || !seg_cols || !out) return PF_ERR_NULL;
    if (K < 1 || K > PF_ATTR_MAX_K) return PF_ERR_UNSUPPORTED;
    AttrPlan plan = {};
    const int rc = make_plan(seg_kind, seg_cols, nseg, C, &plan);
    if (rc != PF_OK) return rc;
    if (B <= 0) return PF_ERR_SHAPE;
    long long nt = 0, mt = 0;
    for (int i = 0; i < B; ++i) {
        if (n[i] <= 0 || m[i] <= 0 || K > n[i]) return PF_ERR_SHAPE;
        nt += n[i]; mt += m[i];
    }
    if (nt > AT_MAX_ROWS || mt > AT_MAX_ROWS) return PF_ERR_SHAPE;
    long long roff = 0, q = 0;
    for (int c0 = 0; c0 < B; c0 += AT_MAXB) {
        AttrRaggedTab t;
        const int nc = B - c0 < AT_MAXB ? B - c0 : AT_MAXB;
        t.q0[0] = (int)q;
        for (int c = 0; c < nc; ++c) {
            t.roff[c] = (int)roff; t.n[c] = n[c0 + c];
            roff += n[c0 + c]; q += m[c0 + c];
            t.q0[c + 1] = (int)q;
        }
        hipLaunchKernelGGL(attr_blend_ragged_kernel, dim3((unsigned)((t.q0[nc] - t.q0[0] + AT_T - 1) / AT_T)), dim3(AT_T), 0,
                           (hipStream_t)stream, idx, d2, attr, t, nc, K, C, plan, out);
    }
    return pf_last_launch_status();
}

extern "C" int pf_normals_pca(const float* pts, const int* idx, int B, int M, int K, const float* viewpoint, double* centroid,
                              float* normal, float* variation, void* stream) {
    if (!pts || !idx || !normal || !variation || (!viewpoint && !centroid)) return PF_ERR_NULL;
    if (K < PF_NORMALS_MIN_K || K > PF_NORMALS_MAX_K) return PF_ERR_UNSUPPORTED;
    if (B <= 0 || M <= 0 || K > M) return PF_ERR_SHAPE;
    const long long total = (long long)B * M;
    if (total > AT_MAX_ROWS) return PF_ERR_SHAPE;
    if (!viewpoint) hipLaunchKernelGGL(centroid_kernel, dim3(B), dim3(AT_T), 0, (hipStream_t)stream, pts, M, centroid);
    hipLaunchKernelGGL(normals_pca_kernel, dim3((unsigned)((total + AT_T - 1) / AT_T)), dim3(AT_T), 0, (hipStream_t)stream, pts, idx,
                       total, M, K, make_view(viewpoint), centroid, normal, variation);
    return pf_last_launch_status();
}

extern "C" int pf_normals_pca_ragged(const float* pts, const int* idx, const int* m, int B, int K, const float* viewpoint,
                                     double* centroid, float* normal, float* variation, void* stream) {
    if (!pts || !idx || !m || !normal || !variation || (!viewpoint && !centroid)) return PF_ERR_NULL;
    if (K < PF_NORMALS_MIN_K || K > PF_NORMALS_MAX_K) return PF_ERR_UNSUPPORTED;
    if (B <= 0) return PF_ERR_SHAPE;
    long long mt = 0;
    for (int i = 0; i < B; ++i) {
        if (m[i] <= 0 || K > m[i]) return PF_ERR_SHAPE;
        mt += m[i];
    }
    if (mt > AT_MAX_ROWS) return PF_ERR_SHAPE;
    long long off = 0;
    for (int c0 = 0; c0 < B; c0 += AT_MAXB) {
        NrmTab t;
        const int nc = B - c0 < AT_MAXB ? B - c0 : AT_MAXB;
        for (int c = 0; c < nc; ++c) { t.off[c] = (int)off; off += m[c0 + c]; }
        t.off[nc] = (int)off;
        double* cen = centroid ? centroid + (size_t)c0 * 3 : nullptr;
        if (!viewpoint) hipLaunchKernelGGL(centroid_ragged_kernel, dim3(nc), dim3(AT_T), 0, (hipStream_t)stream, pts, t, cen);
        hipLaunchKernelGGL(normals_pca_ragged_kernel, dim3((unsigned)((t.off[nc] - t.off[0] + AT_T - 1) / AT_T)), dim3(AT_T), 0,
                           (hipStream_t)stream, pts, idx, t, nc, K, make_view(viewpoint), cen, normal, variation);
    }
    return pf_last_launch_status();
}
