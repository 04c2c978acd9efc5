// The surface reconstruction's block-sparse layout (DESIGN.md 8e "Block-sparse band"; the contract is in puflow_hip.h): the
// same virtual grid, cell rule, tets, edge ids and vertex arithmetic as csrc/recon.hip (shared through pf_recon.h), with the flags
// and the implicit value held per 8 x 8 x 8 block of corners, [NB, 512], for the blocks that the band touches only.  The
// ascending list of distinct block keys is the layout: a block is found by a binary search in it (32 halvings, a constant), its
// 7 upper neighbours through a link table made once.  Memory and work follow the band, never D_x D_y D_z.  What the layout
// supplies to pf_recon.h's rules: the byte (flag, sign) of a corner of a block's 9 x 9 x 9 tile (rs_corner_byte, through the links),
// f at both ends of an edge (one search, then a link), and the store of a stamped corner into one of a point's 8 blocks.  A grown
// block list (band growth on this layout) would be one more writer of the list and is not built.
//
// One lane per point, block link, cell or vertex; pf_mtet_count_sparse is one workgroup per block with a 9 x 9 x 9 tile of
// (flag, sign) bytes in LDS.  No atomics, no lane-to-lane traffic but that tile; every loop has a constant or host-given bound;
// every index that comes from a list (keys, links, slots, offsets, ids) is clamped or checked, so a list that is not this cloud's
// gives a wrong mesh and never an access outside the arrays.
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"
#include "pf_recon.h"

namespace {

constexpr int RS_B = PF_RECON_BLOCK, RS_SLOTS = RS_B * RS_B * RS_B;
static_assert(RS_B == 8 && RS_SLOTS == 512, "the slot rule (k & 7) << 6 | (j & 7) << 3 | (i & 7) is written for 8");

struct RsGrid {
    int Dx, Dy, Dz;                         // corners per axis of the virtual grid
    int NBx, NBy, NBz;                      // blocks per axis
    int NB;                                 // listed blocks
};

// position of key in the ascending list, -1 if it is not there.  NB <= 2^21: 22 halvings would do.
__device__ __forceinline__ int rs_find(const long long* __restrict__ blocks, int NB, long long key) {
    int lo = 0, hi = NB;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = (lo + hi) >> 1;
        if (blocks[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < NB && blocks[lo] == key) ? lo : -1;
}

__device__ __forceinline__ long long rs_key(const RsGrid& g, int bi, int bj, int bk) { return ((long long)bk * g.NBy + bj) * g.NBx + bi; }

// block coordinates of a listed key; false for a key that names no block of this grid
__device__ __forceinline__ bool rs_block_of(const RsGrid& g, long long key, int& bi, int& bj, int& bk) {
    if (key < 0 || key >= (long long)g.NBx * g.NBy * g.NBz) return false;
    bi = (int)(key % g.NBx); bj = (int)((key / g.NBx) % g.NBy); bk = (int)(key / ((long long)g.NBx * g.NBy));
    return true;
}

// a link from the table: a list position or -1
__device__ __forceinline__ int rs_link(const int* __restrict__ links, const RsGrid& g, int b, int o) {
    const int n = links[(size_t)b * 8 + o];
    return (n >= 0 && n < g.NB) ? n : -1;
}

// ---- the block list ------------------------------------------------------------------------------------------------------------
// the first and last corner of a point's 4 corners along one axis, inside the box
struct RsSpan { int lo, hi; };
__device__ __forceinline__ RsSpan rs_span(const float* __restrict__ g, int D, float p) {
    const int c = rc_cell(g, D, p);
    return {max(c - 1, 0), min(c + 2, D - 1)};
}

__global__ __launch_bounds__(RC_T) void block_keys_kernel(const float* __restrict__ pts, int N, const float* __restrict__ gx,
                                                          const float* __restrict__ gy, const float* __restrict__ gz, RsGrid g,
                                                          long long* __restrict__ keys) {
    const int p = blockIdx.x * RC_T + threadIdx.x;
    if (p >= N) return;
    const RsSpan sx = rs_span(gx, g.Dx, pts[(size_t)p * 3 + 0]), sy = rs_span(gy, g.Dy, pts[(size_t)p * 3 + 1]),
                 sz = rs_span(gz, g.Dz, pts[(size_t)p * 3 + 2]);
#pragma unroll
    for (int o = 0; o < 8; ++o)
        keys[(size_t)p * 8 + o] = rs_key(g, ((o & 1) ? sx.hi : sx.lo) >> 3, ((o & 2) ? sy.hi : sy.lo) >> 3, ((o & 4) ? sz.hi : sz.lo) >> 3);
}

__global__ __launch_bounds__(RC_T) void block_links_kernel(const long long* __restrict__ blocks, RsGrid g, int* __restrict__ links) {
    const int b = blockIdx.x * RC_T + threadIdx.x;
    if (b >= g.NB) return;
    int bi = 0, bj = 0, bk = 0;
    const bool ok = rs_block_of(g, blocks[b], bi, bj, bk);
    links[(size_t)b * 8] = b;
#pragma unroll
    for (int o = 1; o < 8; ++o) {
        const int ni = bi + (o & 1), nj = bj + ((o >> 1) & 1), nk = bk + ((o >> 2) & 1);
        links[(size_t)b * 8 + o] = (ok && ni < g.NBx && nj < g.NBy && nk < g.NBz) ? rs_find(blocks, g.NB, rs_key(g, ni, nj, nk)) : -1;
    }
}

// ---- the band ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RC_T) void mark_sparse_kernel(const float* __restrict__ pts, int N, const float* __restrict__ gx,
                                                           const float* __restrict__ gy, const float* __restrict__ gz,
                                                           const long long* __restrict__ blocks, RsGrid g,
                                                           unsigned char* __restrict__ flags) {
    const int p = blockIdx.x * RC_T + threadIdx.x;
    if (p >= N) return;
    const int cx = rc_cell(gx, g.Dx, pts[(size_t)p * 3 + 0]), cy = rc_cell(gy, g.Dy, pts[(size_t)p * 3 + 1]),
              cz = rc_cell(gz, g.Dz, pts[(size_t)p * 3 + 2]);
    const int bx = max(cx - 1, 0) >> 3, by = max(cy - 1, 0) >> 3, bz = max(cz - 1, 0) >> 3;         // the lower block per axis
    const bool two_x = (min(cx + 2, g.Dx - 1) >> 3) != bx, two_y = (min(cy + 2, g.Dy - 1) >> 3) != by,
               two_z = (min(cz + 2, g.Dz - 1) >> 3) != bz;
    int at[8];                                                              // the at most 8 blocks, found once
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        const bool here = (!(o & 1) || two_x) && (!(o & 2) || two_y) && (!(o & 4) || two_z);
        at[o] = here ? rs_find(blocks, g.NB, rs_key(g, bx + (o & 1), by + ((o >> 1) & 1), bz + ((o >> 2) & 1))) : -1;
    }
    rc_stamp(cx, cy, cz, g.Dx, g.Dy, g.Dz, [=](int i, int j, int k) {
        const int o = ((i >> 3) - bx) | ((j >> 3) - by) << 1 | ((k >> 3) - bz) << 2;                // 4 corners span at most 2 blocks
        int b = -1;
#pragma unroll
        for (int q = 0; q < 8; ++q) b = (q == o) ? at[q] : b;               // a select chain: at[] stays in registers
        if (b >= 0) flags[(size_t)b * RS_SLOTS + ((k & 7) << 6 | (j & 7) << 3 | (i & 7))] = 1;
    });
}

// ---- marching tetrahedra ---------------------------------------------------------------------------------------------------------
// One workgroup per listed block: a 9 x 9 x 9 tile of the block's corners and the first layer of its 7 upper neighbours, one
// byte per corner (bit 0: flagged, bit 1: f < 0, read at flagged corners only), then 512 cells that read LDS only.
constexpr int RS_TILE = 9 * 9 * 9;

// the byte of corner (x, y, z), 0 .. 8 per axis, of block b at block coordinates (bi, bj, bk)
__device__ __forceinline__ int rs_corner_byte(const float* __restrict__ f, const unsigned char* __restrict__ flags,
                                              const int* __restrict__ links, const RsGrid& g, int b, int bi, int bj, int bk, int x, int y,
                                              int z) {
    if (bi * 8 + x >= g.Dx || bj * 8 + y >= g.Dy || bk * 8 + z >= g.Dz) return 0;                  // beyond the grid: no corner
    const int n = rs_link(links, g, b, (x >> 3) | (y >> 3) << 1 | (z >> 3) << 2);
    if (n < 0) return 0;
    const size_t at = (size_t)n * RS_SLOTS + ((z & 7) << 6 | (y & 7) << 3 | (x & 7));
    if (flags[at] == 0) return 0;
    return 1 | (f[at] < 0.f ? 2 : 0);
}

// the block layout's cell: the bytes of its 8 corners, fetched once from byte(x, y, z) over the tile's coordinates
struct RsCell {
    int v[8];
    __device__ __forceinline__ bool flagged(int b) const { return (v[b] & 1) != 0; }
    __device__ __forceinline__ bool inside(int b) const { return (v[b] & 2) != 0; }
};
template <typename Byte>
__device__ __forceinline__ int rs_cell_bits(Byte byte, int x, int y, int z) {
    RsCell cell;
#pragma unroll
    for (int b = 0; b < 8; ++b) cell.v[b] = byte(x + (b & 1), y + ((b >> 1) & 1), z + ((b >> 2) & 1));
    return mt_cell_bits(cell);
}

__global__ __launch_bounds__(RS_SLOTS) void count_sparse_kernel(const float* __restrict__ f, const unsigned char* __restrict__ flags,
                                                                const long long* __restrict__ blocks, const int* __restrict__ links,
                                                                RsGrid g, int* __restrict__ count) {
    __shared__ unsigned char tile[RS_TILE + 3];
    const int b = blockIdx.x, s = threadIdx.x;
    int bi = 0, bj = 0, bk = 0;
    const bool ok = rs_block_of(g, blocks[b], bi, bj, bk);                  // uniform over the workgroup
    for (int e = s; e < RS_TILE; e += RS_SLOTS)
        tile[e] = ok ? (unsigned char)rs_corner_byte(f, flags, links, g, b, bi, bj, bk, e % 9, (e / 9) % 9, e / 81) : 0;
    __syncthreads();
    const int bits = rs_cell_bits([&](int x, int y, int z) { return (int)tile[(z * 9 + y) * 9 + x]; }, s & 7, (s >> 3) & 7, s >> 6);
    count[(size_t)b * RS_SLOTS + s] = mt_triangles(bits);
}

// one lane per listed cell, in the order of the list
__global__ __launch_bounds__(RC_T) void emit_sparse_kernel(const float* __restrict__ f, const unsigned char* __restrict__ flags,
                                                           const long long* __restrict__ blocks, const int* __restrict__ links, RsGrid g,
                                                           const long long* __restrict__ cells, const long long* __restrict__ first,
                                                           long long M, long long T, long long* __restrict__ edge_ids) {
    const long long m = (long long)blockIdx.x * RC_T + threadIdx.x;
    if (m >= M) return;
    const long long cell = cells[m];
    if (cell < 0 || cell >= (long long)g.NB * RS_SLOTS) return;
    const int b = (int)(cell >> 9), s = (int)(cell & 511);
    int bi = 0, bj = 0, bk = 0;
    if (!rs_block_of(g, blocks[b], bi, bj, bk)) return;
    const int x = s & 7, y = (s >> 3) & 7, z = s >> 6;
    const int bits = rs_cell_bits([&](int cx, int cy, int cz) { return rs_corner_byte(f, flags, links, g, b, bi, bj, bk, cx, cy, cz); },
                                  x, y, z);
    const long long Dx = g.Dx, DxDy = (long long)g.Dx * g.Dy;
    const long long c = (long long)(bk * 8 + z) * DxDy + (long long)(bj * 8 + y) * Dx + (bi * 8 + x);       // the GLOBAL corner index
    mt_emit_cell(bits, c, Dx, (long long)g.Dy, first + m, T, edge_ids);
}

__global__ __launch_bounds__(RC_T) void vertices_sparse_kernel(const long long* __restrict__ edge_ids, long long V,
                                                               const float* __restrict__ f, const long long* __restrict__ blocks,
                                                               const int* __restrict__ links, const float* __restrict__ gx,
                                                               const float* __restrict__ gy, const float* __restrict__ gz, RsGrid g,
                                                               float* __restrict__ verts) {
    const long long v = (long long)blockIdx.x * RC_T + threadIdx.x;
    if (v >= V) return;
    mt_vertex_of<long long>(edge_ids[v], g.Dx, g.Dy, g.Dz, gx, gy, gz, [=](int i, int j, int k, int i2, int j2, int k2, float& fa, float& fb) {
        const int ba = rs_find(blocks, g.NB, rs_key(g, i >> 3, j >> 3, k >> 3));                    // one search: the upper end is a link away
        const int bb = ba < 0 ? -1 : rs_link(links, g, ba, ((i2 >> 3) - (i >> 3)) | ((j2 >> 3) - (j >> 3)) << 1 | ((k2 >> 3) - (k >> 3)) << 2);
        if (bb < 0) return false;                                           // a corner in no listed block
        fa = f[(size_t)ba * RS_SLOTS + ((k & 7) << 6 | (j & 7) << 3 | (i & 7))];
        fb = f[(size_t)bb * RS_SLOTS + ((k2 & 7) << 6 | (j2 & 7) << 3 | (i2 & 7))];
        return true;
    }, verts + v * 3);
}

// PF_OK and the grid, or what the entry points return for a grid that is none / over the caps
int rs_grid(int Dx, int Dy, int Dz, int NB, RsGrid* g) {
    if (Dx < 2 || Dy < 2 || Dz < 2 || NB <= 0) return PF_ERR_SHAPE;
    if (Dx > PF_RECON_SPARSE_MAX_AXIS || Dy > PF_RECON_SPARSE_MAX_AXIS || Dz > PF_RECON_SPARSE_MAX_AXIS ||
        NB > PF_RECON_SPARSE_MAX_BLOCKS)
        return PF_ERR_UNSUPPORTED;
    *g = RsGrid{Dx, Dy, Dz, (Dx + RS_B - 1) / RS_B, (Dy + RS_B - 1) / RS_B, (Dz + RS_B - 1) / RS_B, NB};
    if ((long long)NB > (long long)g->NBx * g->NBy * g->NBz) return PF_ERR_SHAPE;                  // more blocks than the grid has
    return PF_OK;
}

}  // namespace

extern "C" int pf_recon_block_keys(const float* pts, int N, const float* gx, const float* gy, const float* gz, int Dx, int Dy, int Dz,
                                   long long* keys, void* stream) {
    if (!pts || !gx || !gy || !gz || !keys) return PF_ERR_NULL;
    if (!rc_count_ok(N)) return PF_ERR_SHAPE;
    RsGrid g;
    const int rc = rs_grid(Dx, Dy, Dz, 1, &g);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(block_keys_kernel, dim3(rc_blocks(N)), dim3(RC_T), 0, (hipStream_t)stream, pts, N, gx, gy, gz, g, keys);
    return pf_last_launch_status();
}

extern "C" int pf_recon_block_links(const long long* blocks, int NB, int Dx, int Dy, int Dz, int* links, void* stream) {
    if (!blocks || !links) return PF_ERR_NULL;
    RsGrid g;
    const int rc = rs_grid(Dx, Dy, Dz, NB, &g);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(block_links_kernel, dim3(rc_blocks(NB)), dim3(RC_T), 0, (hipStream_t)stream, blocks, g, links);
    return pf_last_launch_status();
}

extern "C" int pf_recon_mark_sparse(const float* pts, int N, const float* gx, const float* gy, const float* gz, int Dx, int Dy, int Dz,
                                    const long long* blocks, int NB, unsigned char* flags, void* stream) {
    if (!pts || !gx || !gy || !gz || !blocks || !flags) return PF_ERR_NULL;
    if (!rc_count_ok(N)) return PF_ERR_SHAPE;
    RsGrid g;
    const int rc = rs_grid(Dx, Dy, Dz, NB, &g);
    if (rc != PF_OK) return rc;
    if (hipMemsetAsync(flags, 0, (size_t)NB * RS_SLOTS, (hipStream_t)stream) != hipSuccess) return PF_ERR_LAUNCH;
    hipLaunchKernelGGL(mark_sparse_kernel, dim3(rc_blocks(N)), dim3(RC_T), 0, (hipStream_t)stream, pts, N, gx, gy, gz, blocks, g, flags);
    return pf_last_launch_status();
}

extern "C" int pf_mtet_count_sparse(const float* f, const unsigned char* flags, const long long* blocks, const int* links, int NB,
                                    int Dx, int Dy, int Dz, int* count, void* stream) {
    if (!f || !flags || !blocks || !links || !count) return PF_ERR_NULL;
    RsGrid g;
    const int rc = rs_grid(Dx, Dy, Dz, NB, &g);
    if (rc != PF_OK) return rc;
    hipLaunchKernelGGL(count_sparse_kernel, dim3((unsigned)NB), dim3(RS_SLOTS), 0, (hipStream_t)stream, f, flags, blocks, links, g, count);
    return pf_last_launch_status();
}

extern "C" int pf_mtet_emit_sparse(const float* f, const unsigned char* flags, const long long* blocks, const int* links, int NB,
                                   int Dx, int Dy, int Dz, const long long* cells, const long long* first, long long M, long long T,
                                   long long* edge_ids, void* stream) {
    if (!f || !flags || !blocks || !links || !cells || !first || !edge_ids) return PF_ERR_NULL;
    RsGrid g;
    const int rc = rs_grid(Dx, Dy, Dz, NB, &g);
    if (rc != PF_OK) return rc;
    if (M <= 0 || M > (long long)NB * RS_SLOTS || T <= 0 || T > 12 * M) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(emit_sparse_kernel, dim3(rc_blocks(M)), dim3(RC_T), 0, (hipStream_t)stream, f, flags, blocks, links, g, cells,
                       first, M, T, edge_ids);
    return pf_last_launch_status();
}

extern "C" int pf_mtet_vertices_sparse(const long long* edge_ids, long long V, const float* f, const long long* blocks, const int* links,
                                       int NB, const float* gx, const float* gy, const float* gz, int Dx, int Dy, int Dz, float* verts,
                                       void* stream) {
    if (!edge_ids || !f || !blocks || !links || !gx || !gy || !gz || !verts) return PF_ERR_NULL;
    RsGrid g;
    const int rc = rs_grid(Dx, Dy, Dz, NB, &g);
    if (rc != PF_OK) return rc;
    if (V <= 0 || V > 7ll * NB * RS_SLOTS) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(vertices_sparse_kernel, dim3(rc_blocks(V)), dim3(RC_T), 0, (hipStream_t)stream, edge_ids, V, f, blocks, links, gx,
                       gy, gz, g, verts);
    return pf_last_launch_status();
}
