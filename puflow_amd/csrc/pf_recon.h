// What the two layouts of the surface reconstruction share (csrc/recon.hip: dense arrays over the box; csrc/recon_sparse.hip:
// 8 x 8 x 8 blocks around the band): the cell of a point, the generated triangle table of marching tetrahedra, the sign pattern of
// a tet and the vertex arithmetic.  The contract is in puflow_hip.h.  Everything here has internal linkage: each source holds
// its own copy of the table in constant memory.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int RC_T = 256;

inline unsigned rc_blocks(long long n) { return (unsigned)((n + RC_T - 1) / RC_T); }

// (number of entries of g that are <= p) - 1, clamped to 0 .. D - 2: a binary search in the table itself.  D <= 2^26: 27 halvings.
__device__ __forceinline__ int rc_cell(const float* __restrict__ g, int D, float p) {
    int lo = 0, hi = D;
    for (int it = 0; it < 27 && lo < hi; ++it) {
        const int mid = (lo + hi) >> 1;
        if (g[mid] <= p) lo = mid + 1; else hi = mid;
    }
    return min(max(lo - 1, 0), D - 2);
}

// ---- marching tetrahedra -----------------------------------------------------------------------------------------------------
// A cell (lower corner c) is six tets along its main diagonal: for the permutations pi of (x, y, z) in lexicographic order,
// v0 = c, v1 = v0 + e_pi0, v2 = v1 + e_pi1, v3 = c + (1, 1, 1).  The table below is GENERATED from that rule at compile time:
// per tet and sign pattern (bit v: vertex v inside) the triangles as tet edges, in the order that makes the triangle of the
// edges' MIDPOINTS look at the outside - decided in integers, so a vertex that an exact 0 puts on a corner changes nothing.
struct MtTable {
    unsigned char corner[6][4];             // cube corner (x | y << 1 | z << 2) of every tet vertex
    unsigned char ntri[6][16];
    unsigned char edge[6][16][2][3];        // owner's cube corner << 3 | edge class
};

struct MtI3 { int x, y, z; };
constexpr MtI3 mt_sub(MtI3 a, MtI3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
constexpr MtI3 mt_add(MtI3 a, MtI3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
constexpr MtI3 mt_cross(MtI3 a, MtI3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
constexpr int mt_dot(MtI3 a, MtI3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

constexpr MtI3 mt_vertex(int tet, int v) {
    constexpr int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    int o[3] = {0, 0, 0};
    for (int s = 0; s < (v < 3 ? v : 3); ++s) o[perm[tet][s]] = 1;
    return {o[0], o[1], o[2]};
}
// edge classes by offset: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1) = 0 .. 6
constexpr int mt_class(MtI3 d) {
    constexpr int of_bits[8] = {-1, 0, 1, 3, 2, 4, 5, 6};
    return of_bits[d.x | d.y << 1 | d.z << 2];
}

struct MtEdge { int i, j; };                // tet vertices, i < j
constexpr MtEdge mt_edge(int a, int b) { return a < b ? MtEdge{a, b} : MtEdge{b, a}; }

constexpr void mt_put(MtTable& t, int tet, int mask, int slot, MtEdge e0, MtEdge e1, MtEdge e2, MtI3 direction) {
    const MtI3 m0 = mt_add(mt_vertex(tet, e0.i), mt_vertex(tet, e0.j)), m1 = mt_add(mt_vertex(tet, e1.i), mt_vertex(tet, e1.j)),
               m2 = mt_add(mt_vertex(tet, e2.i), mt_vertex(tet, e2.j));       // twice the midpoints
    if (mt_dot(mt_cross(mt_sub(m1, m0), mt_sub(m2, m0)), direction) < 0) { const MtEdge s = e1; e1 = e2; e2 = s; }
    const MtEdge e[3] = {e0, e1, e2};
    for (int k = 0; k < 3; ++k) {
        const MtI3 a = mt_vertex(tet, e[k].i), b = mt_vertex(tet, e[k].j);
        t.edge[tet][mask][slot][k] = (unsigned char)((a.x | a.y << 1 | a.z << 2) << 3 | mt_class(mt_sub(b, a)));
    }
}

constexpr MtTable mt_make_table() {
    MtTable t = {};
    for (int tet = 0; tet < 6; ++tet) {
        for (int v = 0; v < 4; ++v) {
            const MtI3 p = mt_vertex(tet, v);
            t.corner[tet][v] = (unsigned char)(p.x | p.y << 1 | p.z << 2);
        }
        for (int mask = 1; mask < 15; ++mask) {
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
            for (int v = 0; v < 4; ++v) {
                if (mask >> v & 1) in[ni++] = v; else out[no++] = v;
            }
            if (ni == 2) {                                                  // inside a < b, outside c < d: (ac, ad, bd), (ac, bd, bc)
                const int a = in[0], b = in[1], c = out[0], d = out[1];
                const MtI3 dir = mt_sub(mt_add(mt_vertex(tet, c), mt_vertex(tet, d)), mt_add(mt_vertex(tet, a), mt_vertex(tet, b)));
                mt_put(t, tet, mask, 0, mt_edge(a, c), mt_edge(a, d), mt_edge(b, d), dir);
                mt_put(t, tet, mask, 1, mt_edge(a, c), mt_edge(b, d), mt_edge(b, c), dir);
                t.ntri[tet][mask] = 2;
            } else {                                                        // the three edges at the lone corner
                const int lone = ni == 1 ? in[0] : out[0];
                const int* o = ni == 1 ? out : in;
                const MtI3 L = mt_vertex(tet, lone);
                MtI3 dir = mt_add(mt_add(mt_vertex(tet, o[0]), mt_vertex(tet, o[1])), mt_vertex(tet, o[2]));
                dir = mt_sub(dir, MtI3{3 * L.x, 3 * L.y, 3 * L.z});                             // from the lone corner to the others ...
                if (ni != 1) dir = MtI3{-dir.x, -dir.y, -dir.z};                                // ... which is outwards when it is inside
                mt_put(t, tet, mask, 0, mt_edge(lone, o[0]), mt_edge(lone, o[1]), mt_edge(lone, o[2]), dir);
                t.ntri[tet][mask] = 1;
            }
        }
    }
    return t;
}

__constant__ const MtTable mt_table = mt_make_table();

// the sign pattern of a tet (bit v: vertex v inside) from the inside bits of the cell's 8 corners (bit x | y << 1 | z << 2)
__device__ __forceinline__ int mt_mask(int bits, int tet) {
    int mask = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) mask |= ((bits >> mt_table.corner[tet][v]) & 1) << v;
    return mask;
}

// the triangles of a cell with these inside bits
__device__ __forceinline__ int mt_triangles(int bits) {
    int n = 0;
    if (bits > 0 && bits < 255)
        for (int tet = 0; tet < 6; ++tet) n += mt_table.ntri[tet][mt_mask(bits, tet)];
    return n;
}

// edge class -> offset bits (x | y << 1 | z << 2): 0..6 = (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1)
__device__ __forceinline__ int mt_offset_bits(int cls) { return cls < 3 ? 1 << cls : (cls == 3 ? 3 : cls == 4 ? 5 : cls == 5 ? 6 : 7); }

// vertex of edge id 7 a + class, a < b = a + offset(class): g[a] + t (g[b] - g[a]), t = f_a / (f_a - f_b), every operation rounded
__device__ __forceinline__ float mt_lerp(float ga, float gb, float t) {
#pragma clang fp contract(off)
    return __fadd_rn(ga, __fmul_rn(t, __fsub_rn(gb, ga)));
}

}  // namespace
