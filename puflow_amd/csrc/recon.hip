// A triangle mesh from an oriented cloud (DESIGN.md 8e "Surface from an oriented cloud"; the contract is in puflow_hip.h):
// a band of grid corners around the points (pf_recon_mark), an IMLS value at those corners from the K nearest oriented points
// (pf_imls), and the zero set by marching tetrahedra with vertices named by grid-edge id (pf_mtet_count / _emit / _vertices).
//
// Corner coordinates come from three fp32 tables the host made and are never recomputed here.  One lane per point, query, cell
// or vertex; no LDS, no atomics, no lane-to-lane traffic; every loop has a constant or host-given bound.  All writers of the band
// store the same byte, the triangles go where a host-side prefix sum put them and the vertices where torch.unique's order put
// them, so the mesh is the same bits from run to run.
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"

namespace {

constexpr int RC_T = 256;

// ---- the band ----------------------------------------------------------------------------------------------------------------
// (number of entries of g that are <= p) - 1, clamped to 0 .. D - 2: a binary search in the table itself.  D <= 2^26: 27 halvings.
__device__ __forceinline__ int rc_cell(const float* __restrict__ g, int D, float p) {
    int lo = 0, hi = D;
    for (int it = 0; it < 27 && lo < hi; ++it) {
        const int mid = (lo + hi) >> 1;
        if (g[mid] <= p) lo = mid + 1; else hi = mid;
    }
    return min(max(lo - 1, 0), D - 2);
}

__global__ __launch_bounds__(RC_T) void recon_mark_kernel(const float* __restrict__ pts, int N, const float* __restrict__ gx,
                                                          const float* __restrict__ gy, const float* __restrict__ gz, int Dx, int Dy,
                                                          int Dz, unsigned char* __restrict__ flags) {
    const int p = blockIdx.x * RC_T + threadIdx.x;
    if (p >= N) return;
    const int cx = rc_cell(gx, Dx, pts[(size_t)p * 3 + 0]), cy = rc_cell(gy, Dy, pts[(size_t)p * 3 + 1]),
              cz = rc_cell(gz, Dz, pts[(size_t)p * 3 + 2]);
    for (int dz = -1; dz <= 2; ++dz)
        for (int dy = -1; dy <= 2; ++dy)
            for (int dx = -1; dx <= 2; ++dx) {
                const int i = cx + dx, j = cy + dy, k = cz + dz;
                if ((unsigned)i < (unsigned)Dx && (unsigned)j < (unsigned)Dy && (unsigned)k < (unsigned)Dz)
                    flags[((size_t)k * Dy + j) * Dx + i] = 1;
            }
}

// ---- the implicit value ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RC_T) void imls_kernel(const float* __restrict__ query, const float* __restrict__ pts,
                                                    const float* __restrict__ normals, const int* __restrict__ idx, int Q, int N,
                                                    int K, double inv_s2, float* __restrict__ f) {
    const int q = blockIdx.x * RC_T + threadIdx.x;
    if (q >= Q) return;
    const double x = query[(size_t)q * 3 + 0], y = query[(size_t)q * 3 + 1], z = query[(size_t)q * 3 + 2];
    const int* row = idx + (size_t)q * K;
    double d20 = 0.0, num = 0.0, den = 0.0;
    for (int k = 0; k < K; ++k) {
        const int j = min(max(row[k], 0), N - 1);                           // a list from elsewhere cannot make this read outside
        const double dx = x - (double)pts[(size_t)j * 3 + 0], dy = y - (double)pts[(size_t)j * 3 + 1],
                     dz = z - (double)pts[(size_t)j * 3 + 2];
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (k == 0) d20 = d2;
        const double w = exp(-(d2 - d20) * inv_s2);
        const double t = (double)normals[(size_t)j * 3 + 0] * dx + (double)normals[(size_t)j * 3 + 1] * dy +
                         (double)normals[(size_t)j * 3 + 2] * dz;
        num += w * t;
        den += w;
    }
    f[q] = (float)(num / den);
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

// the inside bits (f < 0) of the 8 corners of cell c, bit x | y << 1 | z << 2; -1: c is no active cell
__device__ __forceinline__ int mt_cell_bits(const float* __restrict__ f, const unsigned char* __restrict__ flags, int c, int Dx, int Dy,
                                            int Dz) {
    const int i = c % Dx, j = (c / Dx) % Dy, k = c / (Dx * Dy);
    if (i >= Dx - 1 || j >= Dy - 1 || k >= Dz - 1) return -1;
    int bits = 0;
    bool all = true;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int o = c + (b & 1) + ((b >> 1) & 1) * Dx + ((b >> 2) & 1) * Dx * Dy;
        all = all && flags[o] != 0;
    }
    if (!all) return -1;                                                    // f is read at active corners only
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int o = c + (b & 1) + ((b >> 1) & 1) * Dx + ((b >> 2) & 1) * Dx * Dy;
        bits |= (f[o] < 0.f ? 1 : 0) << b;
    }
    return bits;
}

__device__ __forceinline__ int mt_mask(int bits, int tet) {
    int mask = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) mask |= ((bits >> mt_table.corner[tet][v]) & 1) << v;
    return mask;
}

__global__ __launch_bounds__(RC_T) void mtet_count_kernel(const float* __restrict__ f, const unsigned char* __restrict__ flags,
                                                          int Dx, int Dy, int Dz, int* __restrict__ count) {
    const int c = blockIdx.x * RC_T + threadIdx.x;
    if (c >= Dx * Dy * Dz) return;
    const int bits = mt_cell_bits(f, flags, c, Dx, Dy, Dz);
    int n = 0;
    if (bits > 0 && bits < 255)
        for (int tet = 0; tet < 6; ++tet) n += mt_table.ntri[tet][mt_mask(bits, tet)];
    count[c] = n;
}

__global__ __launch_bounds__(RC_T) void mtet_emit_kernel(const float* __restrict__ f, const unsigned char* __restrict__ flags, int Dx,
                                                         int Dy, int Dz, const long long* __restrict__ first, long long T,
                                                         long long* __restrict__ edge_ids) {
    const int c = blockIdx.x * RC_T + threadIdx.x;
    if (c >= Dx * Dy * Dz) return;
    const int bits = mt_cell_bits(f, flags, c, Dx, Dy, Dz);
    if (bits <= 0 || bits >= 255) return;
    long long t = first[c];
    for (int tet = 0; tet < 6; ++tet) {
        const int mask = mt_mask(bits, tet), n = mt_table.ntri[tet][mask];
        for (int s = 0; s < n; ++s, ++t) {
            if (t < 0 || t >= T) return;                                    // offsets that are not this field's prefix sum: a wrong mesh
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int e = mt_table.edge[tet][mask][s][k], o = e >> 3;
                const long long owner = (long long)c + (o & 1) + ((o >> 1) & 1) * Dx + ((o >> 2) & 1) * Dx * Dy;
                edge_ids[t * 3 + k] = 7 * owner + (e & 7);
            }
        }
    }
}

// vertex of edge id 7 a + class, a < b = a + offset(class): g[a] + t (g[b] - g[a]), t = f_a / (f_a - f_b), every operation rounded
__device__ __forceinline__ float mt_lerp(float ga, float gb, float t) {
#pragma clang fp contract(off)
    return __fadd_rn(ga, __fmul_rn(t, __fsub_rn(gb, ga)));
}

__global__ __launch_bounds__(RC_T) void mtet_vertices_kernel(const long long* __restrict__ edge_ids, long long V,
                                                             const float* __restrict__ f, const float* __restrict__ gx,
                                                             const float* __restrict__ gy, const float* __restrict__ gz, int Dx, int Dy,
                                                             int Dz, float* __restrict__ verts) {
    const long long v = (long long)blockIdx.x * RC_T + threadIdx.x;
    if (v >= V) return;
    const long long id = edge_ids[v];
    float x = 0.f, y = 0.f, z = 0.f;
    if (id >= 0 && id < 7ll * Dx * Dy * Dz) {
        const int a = (int)(id / 7), cls = (int)(id % 7);
        // class -> offset bits: 0..6 = (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1)
        const int ob = cls < 3 ? 1 << cls : (cls == 3 ? 3 : cls == 4 ? 5 : cls == 5 ? 6 : 7);
        const int i = a % Dx, j = (a / Dx) % Dy, k = a / (Dx * Dy);
        const int i2 = i + (ob & 1), j2 = j + ((ob >> 1) & 1), k2 = k + ((ob >> 2) & 1);
        if (i2 < Dx && j2 < Dy && k2 < Dz) {                                // an id that is no edge of the box: (0, 0, 0)
            const float fa = f[a], fb = f[((size_t)k2 * Dy + j2) * Dx + i2];
            const float t = __fdiv_rn(fa, __fsub_rn(fa, fb));
            x = mt_lerp(gx[i], gx[i2], t); y = mt_lerp(gy[j], gy[j2], t); z = mt_lerp(gz[k], gz[k2], t);
        }
    }
    verts[v * 3 + 0] = x; verts[v * 3 + 1] = y; verts[v * 3 + 2] = z;
}

// PF_OK, or what the entry points return for a box that is no box / over the cap
int rc_box(int Dx, int Dy, int Dz) {
    if (Dx < 2 || Dy < 2 || Dz < 2) return PF_ERR_SHAPE;
    if ((long long)Dx * Dy * Dz > PF_RECON_MAX_CORNERS) return PF_ERR_UNSUPPORTED;
    return PF_OK;
}

inline unsigned rc_blocks(long long n) { return (unsigned)((n + RC_T - 1) / RC_T); }

}  // namespace

extern "C" int pf_recon_mark(const float* pts, int N, const float* gx, const float* gy, const float* gz, int Dx, int Dy, int Dz,
                             unsigned char* flags, void* stream) {
    if (!pts || !gx || !gy || !gz || !flags) return PF_ERR_NULL;
    if (N <= 0 || (long long)N * 3 > 0x7fffffffll) return PF_ERR_SHAPE;
    const int rc = rc_box(Dx, Dy, Dz);
    if (rc != PF_OK) return rc;
    if (hipMemsetAsync(flags, 0, (size_t)Dx * Dy * Dz, (hipStream_t)stream) != hipSuccess) return PF_ERR_LAUNCH;
    hipLaunchKernelGGL(recon_mark_kernel, dim3(rc_blocks(N)), dim3(RC_T), 0, (hipStream_t)stream, pts, N, gx, gy, gz, Dx, Dy, Dz, flags);
    return pf_last_launch_status();
}

extern "C" int pf_imls(const float* query, const float* pts, const float* normals, const int* idx, int Q, int N, int K,
                       double sigma_h, float* f, void* stream) {
    if (!query || !pts || !normals || !idx || !f) return PF_ERR_NULL;
    if (K < 1 || K > PF_KNN_GRID_MAX_K) return PF_ERR_UNSUPPORTED;
    if (Q <= 0 || N <= 0 || K > N || (long long)N * 3 > 0x7fffffffll || (long long)Q * 3 > 0x7fffffffll || !(sigma_h > 0.0) ||
        !(1.0 / (sigma_h * sigma_h) < HUGE_VAL))
        return PF_ERR_SHAPE;
    hipLaunchKernelGGL(imls_kernel, dim3(rc_blocks(Q)), dim3(RC_T), 0, (hipStream_t)stream, query, pts, normals, idx, Q, N, K,
                       1.0 / (sigma_h * sigma_h), f);
    return pf_last_launch_status();
}

extern "C" int pf_mtet_table(unsigned char* out, int bytes) {
    static_assert(sizeof(MtTable) == PF_MTET_TABLE_BYTES, "table layout");
    if (!out) return PF_ERR_NULL;
    if (bytes < PF_MTET_TABLE_BYTES) return PF_ERR_SHAPE;
    constexpr MtTable t = mt_make_table();
    const unsigned char* src = reinterpret_cast<const unsigned char*>(&t);
    for (int i = 0; i < PF_MTET_TABLE_BYTES; ++i) out[i] = src[i];
    return PF_MTET_TABLE_BYTES;
}

extern "C" int pf_mtet_count(const float* f, const unsigned char* flags, int Dx, int Dy, int Dz, int* count, void* stream) {
    if (!f || !flags || !count) return PF_ERR_NULL;
    const int rc = rc_box(Dx, Dy, Dz);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(mtet_count_kernel, dim3(rc_blocks((long long)Dx * Dy * Dz)), dim3(RC_T), 0, (hipStream_t)stream, f, flags, Dx, Dy,
                       Dz, count);
    return pf_last_launch_status();
}

extern "C" int pf_mtet_emit(const float* f, const unsigned char* flags, int Dx, int Dy, int Dz, const long long* first, long long T,
                            long long* edge_ids, void* stream) {
    if (!f || !flags || !first || !edge_ids) return PF_ERR_NULL;
    const int rc = rc_box(Dx, Dy, Dz);
    if (rc != PF_OK) return rc;
    if (T <= 0 || T > 12ll * Dx * Dy * Dz) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(mtet_emit_kernel, dim3(rc_blocks((long long)Dx * Dy * Dz)), dim3(RC_T), 0, (hipStream_t)stream, f, flags, Dx, Dy,
                       Dz, first, T, edge_ids);
    return pf_last_launch_status();
}

extern "C" int pf_mtet_vertices(const long long* edge_ids, long long V, const float* f, const float* gx, const float* gy,
                                const float* gz, int Dx, int Dy, int Dz, float* verts, void* stream) {
    if (!edge_ids || !f || !gx || !gy || !gz || !verts) return PF_ERR_NULL;
    const int rc = rc_box(Dx, Dy, Dz);
    if (rc != PF_OK) return rc;
    if (V <= 0 || V > 7ll * Dx * Dy * Dz) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(mtet_vertices_kernel, dim3(rc_blocks(V)), dim3(RC_T), 0, (hipStream_t)stream, edge_ids, V, f, gx, gy, gz, Dx, Dy,
                       Dz, verts);
    return pf_last_launch_status();
}
