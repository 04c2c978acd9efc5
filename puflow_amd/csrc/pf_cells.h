// The cell function of the uniform grids (knn_grid.hip: a grid of points; tri_grid.hip: a grid of triangle boxes) and the
// bound their ring searches stop on.  Device code only, everything inlined.
//
// cell_a(x) = clamp((int)floorf((x - lo_a) * inv_h), 0, G_a - 1), unfused fp32, is MONOTONE in x (subtraction, multiplication by
// a positive constant, floor and clamp all are).  The stopping rules rest on that and on nothing else - kg_face_bound below.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ int kg_cell(float x, float lo, float inv_h, int G) {
#pragma clang fp contract(off)
    const float t = floorf(__fmul_rn(__fsub_rn(x, lo), inv_h));
    return (int)fminf(fmaxf(t, 0.f), (float)(G - 1));                   // clamped as a float: a far query cannot overflow the int
}

// What the cells NOT yet visited can still hold, along one axis.  The visited block spans the cells c - r .. c + r of the axis
// (clipped to 0 .. G - 1).  Returns a lower bound of the COMPUTED d2 of every reference beyond the block's two faces of this
// axis (+inf when both faces are the grid's ends) and sets `face` when at least one face is interior.
//   low face (c - r > 0): unvisited references have cell(x) < c - r.  Take any float E with cell(E) >= c - r: by monotony
//   x >= E would give cell(x) >= c - r, so x < E.  With q >= E: q - x > q - E >= 0, rounding is monotone, so the kernel's
//   dx = fl(q - x) >= fl(q - E) =: gap, fl(dx dx) >= fl(gap gap), and adding the other two non-negative squares cannot go below
//   it (fl(a + b) >= a for b >= 0).  Hence d2 >= fl(gap gap) EXACTLY, no relative allowance.  E is the edge lo + (c - r) h moved
//   up by 2^-20 of the magnitudes involved (about 8 ulps: the roundings of x - lo, of (.) inv_h, of inv_h = fl(1 / h) and of the
//   edge itself are under 5), and cell(E) >= c - r is CHECKED here: if it ever failed the face would give 0 and the search go on.
//   The high face is the mirror image.  Exactness therefore never depends on the size of the slack, only speed does.
__device__ __forceinline__ float kg_face_bound(float q, float lo, float h, float inv_h, int G, int c, int r, bool& face) {
#pragma clang fp contract(off)
    float b = INFINITY;
    const int lc = c - r, hc = c + r;
    if (lc > 0) {
        face = true;
        float E = __fadd_rn(lo, __fmul_rn((float)lc, h));
        E = __fadd_rn(E, __fmul_rn(fmaxf(fabsf(lo), fabsf(E)), 0x1p-20f));
        const float gap = __fsub_rn(q, E);
        b = fminf(b, (kg_cell(E, lo, inv_h, G) >= lc && gap > 0.f) ? __fmul_rn(gap, gap) : 0.f);
    }
    if (hc < G - 1) {
        face = true;
        float E = __fadd_rn(lo, __fmul_rn((float)(hc + 1), h));
        E = __fsub_rn(E, __fmul_rn(fmaxf(fabsf(lo), fabsf(E)), 0x1p-20f));
        const float gap = __fsub_rn(E, q);
        b = fminf(b, (kg_cell(E, lo, inv_h, G) <= hc && gap > 0.f) ? __fmul_rn(gap, gap) : 0.f);
    }
    return b;
}
