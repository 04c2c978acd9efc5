// Point-to-triangle arithmetic shared by the two closest-triangle searches (eval_metrics.hip: tiles of 64 triangles and their
// boxes; tri_grid.hip: a uniform grid of the triangles).  Both must return the same bits, so the distance, the seed window and
// the final distance are written here once.  The build contracts per source expression (-ffp-contract=on), hence a function
// of this header rounds the same way in every kernel that calls it.  Device code only, everything inlined.
#pragma once
#include <hip/hip_runtime.h>

// Squared distance from the origin to the segment [a, b] (coordinates relative to the query point).
template <typename T>
__device__ __forceinline__ T seg_d2(T ax, T ay, T az, T bx, T by, T bz) {
    const T ex = bx - ax, ey = by - ay, ez = bz - az;
    const T ee = ex * ex + ey * ey + ez * ez;
    T t = ee > T(0) ? -(ax * ex + ay * ey + az * ez) / ee : T(0);
    t = t < T(0) ? T(0) : (t > T(1) ? T(1) : t);
    const T qx = ax + t * ex, qy = ay + t * ey, qz = az + t * ez;
    return qx * qx + qy * qy + qz * qz;
}

// Squared distance from the origin (the query point) to the triangle (a, b, c), given relative to the query: the closest
// point is found by classifying the query into the Voronoi regions of the vertices, the edges and the face (barycentric
// sign tests; Ericson, Real-Time Collision Detection 5.1.5).  In the face region the distance is the plane distance
// (n.a)^2 / |n|^2, which keeps its relative precision for points on or next to the surface.  A degenerate triangle (no face
// region) is the closest of its three edges.
template <typename T>
__device__ __forceinline__ T tri_d2(T ax, T ay, T az, T bx, T by, T bz, T cx, T cy, T cz) {
    const T abx = bx - ax, aby = by - ay, abz = bz - az;
    const T acx = cx - ax, acy = cy - ay, acz = cz - az;
    const T d1 = -(abx * ax + aby * ay + abz * az), d2 = -(acx * ax + acy * ay + acz * az);
    if (d1 <= T(0) && d2 <= T(0)) return ax * ax + ay * ay + az * az;                        // vertex a
    const T d3 = -(abx * bx + aby * by + abz * bz), d4 = -(acx * bx + acy * by + acz * bz);
    if (d3 >= T(0) && d4 <= d3) return bx * bx + by * by + bz * bz;                          // vertex b
    const T vc = d1 * d4 - d3 * d2;
    if (vc <= T(0) && d1 >= T(0) && d3 <= T(0)) {                                            // edge ab
        const T den = d1 - d3, t = den > T(0) ? d1 / den : T(0);
        const T qx = ax + t * abx, qy = ay + t * aby, qz = az + t * abz;
        return qx * qx + qy * qy + qz * qz;
    }
    const T d5 = -(abx * cx + aby * cy + abz * cz), d6 = -(acx * cx + acy * cy + acz * cz);
    if (d6 >= T(0) && d5 <= d6) return cx * cx + cy * cy + cz * cz;                          // vertex c
    const T vb = d5 * d2 - d1 * d6;
    if (vb <= T(0) && d2 >= T(0) && d6 <= T(0)) {                                            // edge ac
        const T den = d2 - d6, t = den > T(0) ? d2 / den : T(0);
        const T qx = ax + t * acx, qy = ay + t * acy, qz = az + t * acz;
        return qx * qx + qy * qy + qz * qz;
    }
    const T va = d3 * d6 - d5 * d4;
    if (va <= T(0) && d4 - d3 >= T(0) && d5 - d6 >= T(0)) {                                  // edge bc
        const T den = (d4 - d3) + (d5 - d6), t = den > T(0) ? (d4 - d3) / den : T(0);
        const T qx = bx + t * (cx - bx), qy = by + t * (cy - by), qz = bz + t * (cz - bz);
        return qx * qx + qy * qy + qz * qz;
    }
    const T nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    const T nn = nx * nx + ny * ny + nz * nz;
    if (!(va + vb + vc > T(0)) || !(nn > T(0))) {                                             // degenerate: its edges
        const T e0 = seg_d2(ax, ay, az, bx, by, bz), e1 = seg_d2(bx, by, bz, cx, cy, cz), e2 = seg_d2(cx, cy, cz, ax, ay, az);
        const T e = e0 < e1 ? e0 : e1;
        return e < e2 ? e : e2;
    }
    const T na = nx * ax + ny * ay + nz * az;                                                 // face
    return na * na / nn;
}

constexpr int PM_SEED = 64;      // triangles of the seed window around a point's place in the triangle order

__device__ __forceinline__ float tri_d2_rel(const float* t, float px, float py, float pz) {
    return tri_d2<float>(t[0] - px, t[1] - py, t[2] - pz, t[3] - px, t[4] - py, t[5] - pz, t[6] - px, t[7] - py, t[8] - pz);
}

// The seed window [f0, f1) of point p of P: PM_SEED triangles around seed[p] (seed null: around p F / P), clipped to the
// triangle list; c = the clamped seed itself, the face reported when no triangle of the window has a distance below +inf.
__device__ __forceinline__ void pm_seed_window(const int* __restrict__ seed, int p, int P, int F, long long& c, long long& f0,
                                               long long& f1) {
    c = seed ? (long long)seed[p] : (long long)p * F / P;
    c = c < 0 ? 0 : (c >= F ? F - 1 : c);
    f0 = c - PM_SEED / 2;
    f0 = f0 < 0 ? 0 : f0;
    f1 = f0 + PM_SEED < F ? f0 + PM_SEED : F;
}

// the winner's distance again in double: what both searches report
__device__ __forceinline__ float tri_dist_final(const float* t, double px, double py, double pz) {
    const double d2 = tri_d2<double>(t[0] - px, t[1] - py, t[2] - pz, t[3] - px, t[4] - py, t[5] - pz, t[6] - px, t[7] - py,
                                     t[8] - pz);
    return (float)sqrt(d2);
}

// shapes both searches take
inline bool pm_shape_ok(int P, int F) { return P > 0 && F > 0 && P <= (1 << 26) && F <= (1 << 28); }
