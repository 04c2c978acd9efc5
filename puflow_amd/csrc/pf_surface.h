// Device code shared by the uniformity kernels (eval_uniform.hip) and the surface-reach kernels (surface_reach.hip): the closest
// point of a triangle, the seed-relative squared distance of the disks, and the lookup of a face in a source's reach row.
#pragma once
#include <hip/hip_runtime.h>

// ---- closest point of a triangle ------------------------------------------------------------------------------------------
// The triangle (a, b, c) is given relative to the query point; the result is the closest point, relative to it too.  The same
// Voronoi-region classification as eval_metrics.hip's tri_d2 (Ericson 5.1.5), which returns only the distance.  on_face
// (nullable): whether the result is the foot of the normal inside the triangle - what surface_reach.hip asks before plane_d2.
__device__ __forceinline__ void seg_closest(double ax, double ay, double az, double bx, double by, double bz, double* q) {
    const double ex = bx - ax, ey = by - ay, ez = bz - az;
    const double ee = ex * ex + ey * ey + ez * ez;
    double t = ee > 0.0 ? -(ax * ex + ay * ey + az * ez) / ee : 0.0;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    q[0] = ax + t * ex; q[1] = ay + t * ey; q[2] = az + t * ez;
}

__device__ __forceinline__ void tri_closest(double ax, double ay, double az, double bx, double by, double bz, double cx,
                                            double cy, double cz, double* q, bool* on_face = nullptr) {
    if (on_face) *on_face = false;
    const double abx = bx - ax, aby = by - ay, abz = bz - az;
    const double acx = cx - ax, acy = cy - ay, acz = cz - az;
    const double d1 = -(abx * ax + aby * ay + abz * az), d2 = -(acx * ax + acy * ay + acz * az);
    if (d1 <= 0.0 && d2 <= 0.0) { q[0] = ax; q[1] = ay; q[2] = az; return; }                        // vertex a
    const double d3 = -(abx * bx + aby * by + abz * bz), d4 = -(acx * bx + acy * by + acz * bz);
    if (d3 >= 0.0 && d4 <= d3) { q[0] = bx; q[1] = by; q[2] = bz; return; }                          // vertex b
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {                                                       // edge ab
        const double den = d1 - d3, t = den > 0.0 ? d1 / den : 0.0;
        q[0] = ax + t * abx; q[1] = ay + t * aby; q[2] = az + t * abz;
        return;
    }
    const double d5 = -(abx * cx + aby * cy + abz * cz), d6 = -(acx * cx + acy * cy + acz * cz);
    if (d6 >= 0.0 && d5 <= d6) { q[0] = cx; q[1] = cy; q[2] = cz; return; }                          // vertex c
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {                                                       // edge ac
        const double den = d2 - d6, t = den > 0.0 ? d2 / den : 0.0;
        q[0] = ax + t * acx; q[1] = ay + t * acy; q[2] = az + t * acz;
        return;
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {                                             // edge bc
        const double den = (d4 - d3) + (d5 - d6), t = den > 0.0 ? (d4 - d3) / den : 0.0;
        q[0] = bx + t * (cx - bx); q[1] = by + t * (cy - by); q[2] = bz + t * (cz - bz);
        return;
    }
    const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    const double nn = nx * nx + ny * ny + nz * nz;
    if (!(va + vb + vc > 0.0) || !(nn > 0.0)) {                                                       // degenerate: its edges
        double e[3][3];
        seg_closest(ax, ay, az, bx, by, bz, e[0]);
        seg_closest(bx, by, bz, cx, cy, cz, e[1]);
        seg_closest(cx, cy, cz, ax, ay, az, e[2]);
        int k = 0;
        double best = e[0][0] * e[0][0] + e[0][1] * e[0][1] + e[0][2] * e[0][2];
        for (int i = 1; i < 3; ++i) {
            const double d = e[i][0] * e[i][0] + e[i][1] * e[i][1] + e[i][2] * e[i][2];
            if (d < best) { best = d; k = i; }
        }
        q[0] = e[k][0]; q[1] = e[k][1]; q[2] = e[k][2];
        return;
    }
    if (on_face) *on_face = true;
    const double h = (nx * ax + ny * ay + nz * az) / nn;                                              // face: the foot of the normal
    q[0] = h * nx; q[1] = h * ny; q[2] = h * nz;
}

// The squared distance from the origin to the plane of the triangle (a, b, c), (n . a)^2 / |n|^2, for a point so close to the
// plane that n . a is all cancellation (a source on its own face: the plain double sum is rounding noise there).  The normal's
// components and the sum are carried as unevaluated pairs hi + lo (error-free products by fma, error-free sums), so the result
// has the relative accuracy of double wherever it is above 1e-30 of the triangle's size squared.  fp32 inputs: the corner
// differences are exact in double and their pairwise products fit 53 bits.
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

__device__ __forceinline__ double plane_d2(double ax, double ay, double az, double bx, double by, double bz, double cx,
                                           double cy, double cz) {
    const double u[3] = {bx - ax, by - ay, bz - az}, v[3] = {cx - ax, cy - ay, cz - az}, a[3] = {ax, ay, az};
    double sum = 0.0, err = 0.0, nn = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        const double p = u[j] * v[k], pe = __builtin_fma(u[j], v[k], -p), q = u[k] * v[j], qe = __builtin_fma(u[k], v[j], -q);
        double nh, nl;
        two_sum(p, -q, nh, nl);                                   // n_i = nh + nl (+ pe - qe, zero for fp32 corners)
        nl += pe - qe;
        nn += nh * nh;
        const double t = nh * a[i], te = __builtin_fma(nh, a[i], -t);
        double s2, e2;
        two_sum(sum, t, s2, e2);
        sum = s2;
        err += e2 + te + nl * a[i];
    }
    const double na = sum + err;
    return na * na / nn;
}

// |q - seed|^2 in fp32, the seed subtracted first, so the squares are of O(r) numbers: the one expression every disk test and
// every surface distance uses
__device__ __forceinline__ float seed_d2(const float* __restrict__ q, float sx, float sy, float sz) {
    const float dx = q[0] - sx, dy = q[1] - sy, dz = q[2] - sz;
    return dx * dx + dy * dy + dz * dz;
}

// The reach CSR of pf_reach_fill / pf_reach_relax: row s lists the candidate faces of source s in ascending index with their
// bottleneck values.  b2 of face f for that source: its entry, +inf when the row does not hold it (any f, in range or not).
struct PfReach {
    const int* face;                 // [N] the face every point lies on
    const long long* off;            // [S+1]
    const int* rface;                // [nnz]
    const float* rb2;                // [nnz]
};

__device__ __forceinline__ int reach_find(const int* __restrict__ row, int n, int f) {
    int lo = 0, hi = n;              // the first k with row[k] >= f
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (row[mid] < f) lo = mid + 1; else hi = mid;
    }
    return lo < n && row[lo] == f ? lo : -1;
}

__device__ __forceinline__ float reach_b2(const PfReach& R, int s, int f) {
    const long long a = R.off[s], n = R.off[s + 1] - a;
    const int k = reach_find(R.rface + a, n > 0 ? (int)n : 0, f);
    return k < 0 ? INFINITY : R.rb2[a + k];
}
