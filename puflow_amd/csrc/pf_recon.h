// What the two layouts of the surface reconstruction share (csrc/recon.hip: dense arrays over the box; csrc/recon_sparse.hip:
// 8 x 8 x 8 blocks around the band): the cell of a point, the generated triangle table of marching tetrahedra, the sign pattern of
// a tet and - written once over "the flag and value at a corner, in this layout" (the last section) - the 4 x 4 x 4 stamp of a
// point, the inside bits of a cell, the triangles of a cell and the vertex of an edge id.  A source keeps what is its layout's:
// addressing, block keys and links, tiles.  The contract is in puflow_hip.h.  Everything here has internal linkage: each source
// holds its own copy of the table in constant memory.  Like the kernels that use them the rules are one lane per item, without
// atomics, with constant loop bounds, and check every index they form from a list (offsets, edge ids) before they use it.
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

// ---- written once over "the flag and value at a corner, in this layout" ------------------------------------------------------
// A layout hands the three rules below a functor and keeps its addressing to itself:
//   a cell:   flagged(b), inside(b) - corner b (x | y << 1 | z << 2) of the cell is in the band / has f < 0 there; inside(b) is
//             asked only once all eight are flagged, so f is read at active corners only and the flags come first
//   an edge:  ends(i, j, k, i2, j2, k2, fa, fb) - f at both end corners of an edge of the grid, false if one is not held
//   a point:  put(i, j, k) - flag that corner of the grid
// A further layout (a grown block list, say - not built) supplies these three and gets the extraction as it stands.

// a point count that the kernels can index with int: N > 0 and 3 N <= INT_MAX
inline bool rc_count_ok(int N) { return N > 0 && (long long)N * 3 <= 0x7fffffffll; }

// the global index of corner b (x | y << 1 | z << 2) of the cell with lower corner c
template <typename C, typename I>
__device__ __forceinline__ C rc_corner(C c, int b, I Dx, I Dy) { return c + (b & 1) + ((b >> 1) & 1) * Dx + ((b >> 2) & 1) * Dx * Dy; }

// the 4 x 4 x 4 corners around the cell of a point, those inside the box
template <typename Put>
__device__ __forceinline__ void rc_stamp(int cx, int cy, int cz, int Dx, int Dy, int Dz, Put put) {
    for (int dz = -1; dz <= 2; ++dz)
        for (int dy = -1; dy <= 2; ++dy)
            for (int dx = -1; dx <= 2; ++dx) {
                const int i = cx + dx, j = cy + dy, k = cz + dz;
                if ((unsigned)i < (unsigned)Dx && (unsigned)j < (unsigned)Dy && (unsigned)k < (unsigned)Dz) put(i, j, k);
            }
}

// the inside bits (f < 0) of a cell's 8 corners, bit x | y << 1 | z << 2; -1: one of them is not flagged - no active cell
template <typename Cell>
__device__ __forceinline__ int mt_cell_bits(const Cell& cell) {
    bool all = true;
#pragma unroll
    for (int b = 0; b < 8; ++b) all = all && cell.flagged(b);
    if (!all) return -1;
    int bits = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) bits |= (cell.inside(b) ? 1 : 0) << b;
    return bits;
}

// the triangles of the cell with GLOBAL corner index c and these inside bits, as edge ids 7 owner + class, from offset *first
// on (read for a cell with triangles only)
template <typename I>
__device__ __forceinline__ void mt_emit_cell(int bits, I c, I Dx, I Dy, const long long* first, long long T, long long* edge_ids) {
    if (bits <= 0 || bits >= 255) return;
    long long t = *first;
    for (int tet = 0; tet < 6; ++tet) {
        const int mask = mt_mask(bits, tet), n = mt_table.ntri[tet][mask];
        for (int s = 0; s < n; ++s, ++t) {
            if (t < 0 || t >= T) return;                                    // offsets that are not this field's prefix sum: a wrong mesh
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int e = mt_table.edge[tet][mask][s][k];
                const long long owner = rc_corner((long long)c, e >> 3, Dx, Dy);
                edge_ids[t * 3 + k] = 7 * owner + (e & 7);
            }
        }
    }
}

// the vertex of edge id `id` of a D_x x D_y x D_z grid; (0, 0, 0) for an id that is no edge of it or whose ends are not held.
// I: an integer that holds a corner index of the grid.
template <typename I, typename Ends>
__device__ __forceinline__ void mt_vertex_of(long long id, int Dx, int Dy, int Dz, const float* __restrict__ gx,
                                             const float* __restrict__ gy, const float* __restrict__ gz, Ends ends,
                                             float* __restrict__ vert) {
    const I DxDy = (I)Dx * Dy;
    float x = 0.f, y = 0.f, z = 0.f;
    if (id >= 0 && id < 7ll * DxDy * Dz) {
        const I a = (I)(id / 7);
        const int ob = mt_offset_bits((int)(id % 7));
        const int i = (int)(a % Dx), j = (int)((a / Dx) % Dy), k = (int)(a / DxDy);
        const int i2 = i + (ob & 1), j2 = j + ((ob >> 1) & 1), k2 = k + ((ob >> 2) & 1);
        float fa, fb;
        if (i2 < Dx && j2 < Dy && k2 < Dz && ends(i, j, k, i2, j2, k2, fa, fb)) {
            const float t = __fdiv_rn(fa, __fsub_rn(fa, fb));
            x = mt_lerp(gx[i], gx[i2], t); y = mt_lerp(gy[j], gy[j2], t); z = mt_lerp(gz[k], gz[k2], t);
        }
    }
    vert[0] = x; vert[1] = y; vert[2] = z;
}

}  // namespace
