// A triangle mesh from an oriented cloud (DESIGN.md 8e "Surface from an oriented cloud"; the contract is in puflow_hip.h):
// a band of grid corners around the points (pf_recon_mark), an IMLS value at those corners from the K nearest oriented points
// (pf_imls), and the zero set by marching tetrahedra with vertices named by grid-edge id (pf_mtet_count / _emit / _vertices).
// Between the value and the extraction the host may grow the band where the zero set leaves it (pf_recon_grow, "closing holes").
//
// This is the dense layout: flags and values are arrays over the box, corner (i, j, k) at (k D_y + j) D_x + i, and every corner
// of the box is held.  The stamp of a point, the inside bits and triangles of a cell and the vertex of an edge id are pf_recon.h's,
// shared with csrc/recon_sparse.hip; the kernels here are index setup plus a call.  Band growth alone is written against dense
// addresses (its neighbour reads are c +- a stride); growth over a block list is not built.
//
// Corner coordinates come from three fp32 tables the host made and are never recomputed here.  One lane per point, query, cell
// or vertex; no LDS, no atomics, no lane-to-lane traffic; every loop has a constant or host-given bound.  All writers of the band
// store the same byte, the triangles go where a host-side prefix sum put them and the vertices where torch.unique's order put
// them, so the mesh is the same bits from run to run.
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"
#include "pf_recon.h"

namespace {

// ---- the band ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RC_T) void recon_mark_kernel(const float* __restrict__ pts, int N, const float* __restrict__ gx,
                                                          const float* __restrict__ gy, const float* __restrict__ gz, int Dx, int Dy,
                                                          int Dz, unsigned char* __restrict__ flags) {
    const int p = blockIdx.x * RC_T + threadIdx.x;
    if (p >= N) return;
    rc_stamp(rc_cell(gx, Dx, pts[(size_t)p * 3 + 0]), rc_cell(gy, Dy, pts[(size_t)p * 3 + 1]), rc_cell(gz, Dz, pts[(size_t)p * 3 + 2]),
             Dx, Dy, Dz, [=](int i, int j, int k) { flags[((size_t)k * Dy + j) * Dx + i] = 1; });
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

// ---- marching tetrahedra (the table and the rules over a cell, an edge: pf_recon.h) ------------------------------------------
// the dense layout's cell: corner b of the cell with lower corner c is flags / f at rc_corner(c, b)
struct RcCell {
    const float* __restrict__ f;
    const unsigned char* __restrict__ flags;
    int c, Dx, Dy;
    __device__ __forceinline__ bool flagged(int b) const { return flags[rc_corner(c, b, Dx, Dy)] != 0; }
    __device__ __forceinline__ bool inside(int b) const { return f[rc_corner(c, b, Dx, Dy)] < 0.f; }
};

// the inside bits of cell c; -1: c is no cell of the box or no active one
__device__ __forceinline__ int rc_cell_bits(const float* __restrict__ f, const unsigned char* __restrict__ flags, int c, int Dx, int Dy,
                                            int Dz) {
    const int i = c % Dx, j = (c / Dx) % Dy, k = c / (Dx * Dy);
    if (i >= Dx - 1 || j >= Dy - 1 || k >= Dz - 1) return -1;
    return mt_cell_bits(RcCell{f, flags, c, Dx, Dy});
}

__global__ __launch_bounds__(RC_T) void mtet_count_kernel(const float* __restrict__ f, const unsigned char* __restrict__ flags,
                                                          int Dx, int Dy, int Dz, int* __restrict__ count) {
    const int c = blockIdx.x * RC_T + threadIdx.x;
    if (c >= Dx * Dy * Dz) return;
    count[c] = mt_triangles(rc_cell_bits(f, flags, c, Dx, Dy, Dz));
}

__global__ __launch_bounds__(RC_T) void mtet_emit_kernel(const float* __restrict__ f, const unsigned char* __restrict__ flags, int Dx,
                                                         int Dy, int Dz, const long long* __restrict__ first, long long T,
                                                         long long* __restrict__ edge_ids) {
    const int c = blockIdx.x * RC_T + threadIdx.x;
    if (c >= Dx * Dy * Dz) return;
    mt_emit_cell(rc_cell_bits(f, flags, c, Dx, Dy, Dz), c, Dx, Dy, first + c, T, edge_ids);
}

__global__ __launch_bounds__(RC_T) void mtet_vertices_kernel(const long long* __restrict__ edge_ids, long long V,
                                                             const float* __restrict__ f, const float* __restrict__ gx,
                                                             const float* __restrict__ gy, const float* __restrict__ gz, int Dx, int Dy,
                                                             int Dz, float* __restrict__ verts) {
    const long long v = (long long)blockIdx.x * RC_T + threadIdx.x;
    if (v >= V) return;
    mt_vertex_of<int>(edge_ids[v], Dx, Dy, Dz, gx, gy, gz, [=](int i, int j, int k, int i2, int j2, int k2, float& fa, float& fb) {
        fa = f[((size_t)k * Dy + j) * Dx + i]; fb = f[((size_t)k2 * Dy + j2) * Dx + i2];           // every corner of the box is held
        return true;
    }, verts + v * 3);
}

// ---- band growth at the exits (the rule: puflow_hip.h "closing holes") --------------------------------------------------------
// One lane per cell.  A face can only be shared with an active neighbour when its four corners - corners of this cell - are
// flagged, so a cell far from the band leaves after its own 8 flag bytes; the neighbour's other four flags and the face's four
// values are read for the faces that pass.  Every index is a corner of this cell or of a neighbour checked to be a cell.
__global__ __launch_bounds__(RC_T) void recon_grow_kernel(const float* __restrict__ f, const unsigned char* __restrict__ flags, int Dx,
                                                          int Dy, int Dz, unsigned char* __restrict__ added) {
    const int c = blockIdx.x * RC_T + threadIdx.x;
    if (c >= Dx * Dy * Dz) return;
    const int pos[3] = {c % Dx, (c / Dx) % Dy, c / (Dx * Dy)}, dim[3] = {Dx, Dy, Dz}, step[3] = {1, Dx, Dx * Dy};
    if (pos[0] >= Dx - 1 || pos[1] >= Dy - 1 || pos[2] >= Dz - 1) return;
    int own = 0;                                                            // bit x | y << 1 | z << 2: that corner is flagged
#pragma unroll
    for (int b = 0; b < 8; ++b) own |= (flags[rc_corner(c, b, Dx, Dy)] != 0 ? 1 : 0) << b;
    if (own == 255) return;                                                 // active: no exit
    bool exit = false;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int s = 0; s < 2; ++s) {                                       // the neighbour below (s = 0) / above (s = 1) along axis a
            int face = 0;
#pragma unroll
            for (int b = 0; b < 8; ++b)
                if (((b >> a) & 1) == s) face |= 1 << b;
            const int n = pos[a] + (s ? 1 : -1), far = s ? step[a] : -step[a];
            if ((own & face) != face || n < 0 || n > dim[a] - 2) continue;
            bool all = true;
            int inside = 0;
#pragma unroll
            for (int b = 0; b < 8; ++b)
                if (((b >> a) & 1) == s) all = all && flags[rc_corner(c, b, Dx, Dy) + far] != 0;
            if (!all) continue;                                             // f is read at the corners of an active cell only
#pragma unroll
            for (int b = 0; b < 8; ++b)
                if (((b >> a) & 1) == s) inside += f[rc_corner(c, b, Dx, Dy)] < 0.f ? 1 : 0;
            exit = exit || (inside != 0 && inside != 4);
        }
    if (!exit) return;
#pragma unroll
    for (int b = 0; b < 8; ++b) added[rc_corner(c, b, Dx, Dy)] = 1;
}

// PF_OK, or what the entry points return for a box that is no box / over the cap
int rc_box(int Dx, int Dy, int Dz) {
    if (Dx < 2 || Dy < 2 || Dz < 2) return PF_ERR_SHAPE;
    if ((long long)Dx * Dy * Dz > PF_RECON_MAX_CORNERS) return PF_ERR_UNSUPPORTED;
    return PF_OK;
}

}  // namespace

extern "C" int pf_recon_mark(const float* pts, int N, const float* gx, const float* gy, const float* gz, int Dx, int Dy, int Dz,
                             unsigned char* flags, void* stream) {
    if (!pts || !gx || !gy || !gz || !flags) return PF_ERR_NULL;
    if (!rc_count_ok(N)) return PF_ERR_SHAPE;
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
    if (!rc_count_ok(Q) || !rc_count_ok(N) || K > N || !(sigma_h > 0.0) ||
        !(1.0 / (sigma_h * sigma_h) < HUGE_VAL))
        return PF_ERR_SHAPE;
    hipLaunchKernelGGL(imls_kernel, dim3(rc_blocks(Q)), dim3(RC_T), 0, (hipStream_t)stream, query, pts, normals, idx, Q, N, K,
                       1.0 / (sigma_h * sigma_h), f);
    return pf_last_launch_status();
}

extern "C" int pf_recon_grow(const float* f, const unsigned char* flags, int Dx, int Dy, int Dz, unsigned char* added, void* stream) {
    if (!f || !flags || !added) return PF_ERR_NULL;
    const int rc = rc_box(Dx, Dy, Dz);
    if (rc != PF_OK) return rc;
    if (hipMemsetAsync(added, 0, (size_t)Dx * Dy * Dz, (hipStream_t)stream) != hipSuccess) return PF_ERR_LAUNCH;
    hipLaunchKernelGGL(recon_grow_kernel, dim3(rc_blocks((long long)Dx * Dy * Dz)), dim3(RC_T), 0, (hipStream_t)stream, f, flags, Dx, Dy,
                       Dz, added);
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
