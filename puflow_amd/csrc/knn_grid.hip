// Exact small-K nearest neighbours over a uniform grid (DESIGN.md 8e "The grid search"): the search behind --attr_search grid.
// Returns, bit for bit, what pf_knn_large returns - the K smallest keys (d2 bits << 32 | index), d2 the unfused fp32
// ((dx*dx)+(dy*dy))+(dz*dz) of sqd() in patch_ops.hip - but reads tens of candidates per query instead of the whole cloud.
//
// Per cloud, in the caller's workspace: a 64-byte header (box, cell edge, cell counts), the references sorted by cell as
// (x, y, z, index bits) and the cells' first positions.  Five launches per 64 clouds: box + header, histogram, scan, scatter,
// search.  Integer atomics only (histogram and scatter cursors); the order of the points inside a cell is whatever the scatter
// made it and cannot show, because the output is ordered by key.
//
// cell_a(x) = clamp((int)floorf((x - lo_a) * inv_h), 0, G_a - 1), unfused fp32, is MONOTONE in x (subtraction, multiplication by
// a positive constant, floor and clamp all are).  The stopping rule rests on that and on nothing else - kg_cell and kg_face_bound
// of pf_cells.h, which the grid of triangles (tri_grid.hip) shares.
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"
#include "pf_cells.h"
#include "pf_wave.h"

namespace {

constexpr int KG_MAXB = 64;             // clouds per launch (PF_RAGGED_MAXB of patch_ops.hip)
constexpr int KG_GMAX = 256;            // cells per axis, at most
constexpr int KG_CELLS_PER_POINT = 2;   // g = the smallest integer with g^3 >= 2 N: cells of the cube the longest extent spans
constexpr int KG_T = 256;               // search: four queries (waves) per workgroup
constexpr int KG_SCAN_T = 1024;
constexpr int KG_HEADER = 64;           // bytes

struct KgHeader {                       // written by kg_setup_kernel, read by every later kernel of the cloud
    float lo[3];
    float inv_h;
    int G[3];
    int ncells;
    float h;
    int pad[7];
};
static_assert(sizeof(KgHeader) == KG_HEADER, "header layout");

struct KgTab {
    long long woff[KG_MAXB];            // the cloud's workspace, in bytes from ws
    int roff[KG_MAXB];                  // first reference of the cloud
    int n[KG_MAXB];                     // its references
    int g[KG_MAXB];                     // kg_axis_cells(n)
    int q0[KG_MAXB + 1];                // its first query (queries and outputs of all clouds back to back)
};

__host__ __device__ inline int kg_axis_cells(long long n) {
    int g = 1;
    while (g < KG_GMAX && (long long)g * g * g < KG_CELLS_PER_POINT * n) ++g;
    return g;
}
// header | float4 pts[n] | int cstart[g^3 + 1] | int cursor[g^3], rounded up to 16 bytes
inline long long kg_cloud_bytes(int n) {
    const long long g = kg_axis_cells(n), cells = g * g * g;
    const long long b = KG_HEADER + 16ll * n + 4ll * (2 * cells + 1);
    return (b + 15) & ~15ll;
}
__device__ __forceinline__ const KgHeader* kg_header(const char* w) { return reinterpret_cast<const KgHeader*>(w); }
__device__ __forceinline__ float4* kg_pts(char* w) { return reinterpret_cast<float4*>(w + KG_HEADER); }
__device__ __forceinline__ int* kg_cstart(char* w, int n) { return reinterpret_cast<int*>(w + KG_HEADER + 16ll * n); }
__device__ __forceinline__ int* kg_cursor(char* w, int n, int g) { return kg_cstart(w, n) + (g * g * g + 1); }

__device__ __forceinline__ float kg_sqd(float ax, float ay, float az, float bx, float by, float bz) {      // sqd() of patch_ops.hip
#pragma clang fp contract(off)
    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// ---- 1. box, cell edge, cell counts; histogram cleared.  One workgroup per cloud.  min / max are exact and order-free.
__global__ __launch_bounds__(256) void kg_setup_kernel(const float* __restrict__ ref, const KgTab t, char* __restrict__ ws) {
#pragma clang fp contract(off)
    __shared__ float red[4][6];
    __shared__ int s_ncells;
    const int c = blockIdx.x, tid = threadIdx.x, n = t.n[c], g = t.g[c];
    const float* p = ref + (size_t)t.roff[c] * 3;
    char* w = ws + t.woff[c];
    float lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
    for (int i = tid; i < n; i += 256) {
        const float x = p[i * 3 + 0], y = p[i * 3 + 1], z = p[i * 3 + 2];
        lx = fminf(lx, x); ly = fminf(ly, y); lz = fminf(lz, z);
        hx = fmaxf(hx, x); hy = fmaxf(hy, y); hz = fmaxf(hz, z);
    }
    lx = pf_xor_min<1, 32>(lx); ly = pf_xor_min<1, 32>(ly); lz = pf_xor_min<1, 32>(lz);
    hx = pf_xor_max<1, 32>(hx); hy = pf_xor_max<1, 32>(hy); hz = pf_xor_max<1, 32>(hz);
    if ((tid & 63) == 0) {
        float* r = red[tid >> 6];
        r[0] = lx; r[1] = ly; r[2] = lz; r[3] = hx; r[4] = hy; r[5] = hz;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 4; ++k) {
            lx = fminf(lx, red[k][0]); ly = fminf(ly, red[k][1]); lz = fminf(lz, red[k][2]);
            hx = fmaxf(hx, red[k][3]); hy = fmaxf(hy, red[k][4]); hz = fmaxf(hz, red[k][5]);
        }
        const float e = fmaxf(fmaxf(__fsub_rn(hx, lx), __fsub_rn(hy, ly)), __fsub_rn(hz, lz));
        const float ma = fmaxf(fmaxf(fmaxf(fabsf(lx), fabsf(hx)), fmaxf(fabsf(ly), fabsf(hy))), fmaxf(fabsf(lz), fabsf(hz)));
        // the floor: 16 ulps of the largest |coordinate| (a cell narrower than the coordinates' own grain sorts nothing and makes
        // the face bounds useless), and a positive number for a cloud that is one point at the origin
        float h = __fdiv_rn(e, (float)g);
        h = fmaxf(h, __fmul_rn(ma, 0x1p-19f));
        h = fmaxf(h, 0x1p-100f);
        const float inv_h = __fdiv_rn(1.f, h);
        KgHeader* hd = reinterpret_cast<KgHeader*>(w);
        hd->lo[0] = lx; hd->lo[1] = ly; hd->lo[2] = lz;
        hd->inv_h = inv_h;
        hd->h = h;
        const int Gx = kg_cell(hx, lx, inv_h, g) + 1, Gy = kg_cell(hy, ly, inv_h, g) + 1, Gz = kg_cell(hz, lz, inv_h, g) + 1;
        hd->G[0] = Gx; hd->G[1] = Gy; hd->G[2] = Gz;
        hd->ncells = Gx * Gy * Gz;                                      // <= g^3
        s_ncells = Gx * Gy * Gz;
    }
    __syncthreads();
    int* cs = kg_cstart(w, n);
    const int nce = s_ncells;
    for (int i = tid; i <= nce; i += 256) cs[i] = 0;
}

// ---- 2. histogram: grid (point blocks, clouds)
__global__ __launch_bounds__(256) void kg_count_kernel(const float* __restrict__ ref, const KgTab t, char* __restrict__ ws) {
    const int c = blockIdx.y, n = t.n[c], i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    char* w = ws + t.woff[c];
    const KgHeader* hd = kg_header(w);
    const float* p = ref + ((size_t)t.roff[c] + i) * 3;
    const int cx = kg_cell(p[0], hd->lo[0], hd->inv_h, hd->G[0]), cy = kg_cell(p[1], hd->lo[1], hd->inv_h, hd->G[1]),
              cz = kg_cell(p[2], hd->lo[2], hd->inv_h, hd->G[2]);
    atomicAdd(kg_cstart(w, n) + ((cz * hd->G[1] + cy) * hd->G[0] + cx), 1);
}

// ---- 3. exclusive scan of the histogram in place (cstart[ncells] = n), copied to the scatter cursors.  One workgroup per cloud.
__global__ __launch_bounds__(KG_SCAN_T) void kg_scan_kernel(const KgTab t, char* __restrict__ ws) {
    __shared__ int wsum[KG_SCAN_T / 64];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = t.n[c];
    char* w = ws + t.woff[c];
    const int nce = kg_header(w)->ncells;
    int* cs = kg_cstart(w, n);
    int* cur = kg_cursor(w, n, t.g[c]);
    int carry = 0;
    for (int base = 0; base < nce; base += KG_SCAN_T) {
        const int i = base + tid;
        const int v = i < nce ? cs[i] : 0;
        int x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(x, d);
            if (lane >= d) x += o;
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < KG_SCAN_T / 64; ++k) {
            const int s = wsum[k];
            before += k < wv ? s : 0;
            tot += s;
        }
        if (i < nce) {
            const int ex = carry + before + x - v;
            cs[i] = ex;
            cur[i] = ex;
        }
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) cs[nce] = carry;
}

// ---- 4. scatter: the references in cell order, each with its index inside the cloud
__global__ __launch_bounds__(256) void kg_scatter_kernel(const float* __restrict__ ref, const KgTab t, char* __restrict__ ws) {
    const int c = blockIdx.y, n = t.n[c], i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    char* w = ws + t.woff[c];
    const KgHeader* hd = kg_header(w);
    const float* p = ref + ((size_t)t.roff[c] + i) * 3;
    const float x = p[0], y = p[1], z = p[2];
    const int cx = kg_cell(x, hd->lo[0], hd->inv_h, hd->G[0]), cy = kg_cell(y, hd->lo[1], hd->inv_h, hd->G[1]),
              cz = kg_cell(z, hd->lo[2], hd->inv_h, hd->G[2]);
    const int pos = atomicAdd(kg_cursor(w, n, t.g[c]) + ((cz * hd->G[1] + cy) * hd->G[0] + cx), 1);
    if ((unsigned)pos < (unsigned)n) kg_pts(w)[pos] = make_float4(x, y, z, __int_as_float(i));
}

// ---- 5. search (the stopping bound: kg_face_bound of pf_cells.h)
__device__ __forceinline__ unsigned long long kg_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long kg_max(unsigned long long a, unsigned long long b) { return a < b ? b : a; }

// One wave per query.  `best`: the 64 smallest keys so far, ascending over the lanes (lane i holds the i-th; ~0 = none).
// Candidates come 64 at a time, gathered from all the cell runs of (a part of) a shell; a batch none of whose keys is below the
// K-th is dropped after one ballot, another is sorted descending over the lanes, min'ed lane by lane with `best` (the 64 smallest
// of the 128, as a bitonic sequence) and merged.
__global__ __launch_bounds__(KG_T) void kg_search_kernel(const float* __restrict__ query, const KgTab t, int nc, int K,
                                                        char* __restrict__ ws, int* __restrict__ idx_out,
                                                        float* __restrict__ dist_out) {
    const int lane = threadIdx.x & 63;
    const int wq = blockIdx.x * (KG_T / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wq >= t.q0[nc] - t.q0[0]) return;                               // wave-uniform
    const int q = t.q0[0] + wq;
    int c = 0;
    while (c + 1 < nc && q >= t.q0[c + 1]) ++c;
    const int n = t.n[c];
    char* w = ws + t.woff[c];
    const KgHeader* hd = kg_header(w);
    const float4* __restrict__ pts = kg_pts(w);
    const int* __restrict__ cs = kg_cstart(w, n);
    const float lox = hd->lo[0], loy = hd->lo[1], loz = hd->lo[2], inv_h = hd->inv_h, h = hd->h;
    const int Gx = hd->G[0], Gy = hd->G[1], Gz = hd->G[2];
    const float qx = query[(size_t)q * 3 + 0], qy = query[(size_t)q * 3 + 1], qz = query[(size_t)q * 3 + 2];
    const int cx = kg_cell(qx, lox, inv_h, Gx), cy = kg_cell(qy, loy, inv_h, Gy), cz = kg_cell(qz, loz, inv_h, Gz);

    unsigned long long best = ~0ull, kth = ~0ull;
    for (int r = 0;; ++r) {
        // shell r: the cells at Chebyshev distance exactly r, clipped to the grid.  x is the fastest cell index, so a row of the
        // shell's top, bottom, front and back is one run of sorted points; the other rows give their two end cells.  Entry
        // e = 2 (row) + side: a full run (side 0 of a boundary row), one end cell, or nothing.
        const int x0 = max(cx - r, 0), x1 = min(cx + r, Gx - 1), y0 = max(cy - r, 0), y1 = min(cy + r, Gy - 1),
                  z0 = max(cz - r, 0), z1 = min(cz + r, Gz - 1);
        const int ny = y1 - y0 + 1, nent = 2 * ny * (z1 - z0 + 1);
        for (int e0 = 0; e0 < nent; e0 += 64) {
            const int e = e0 + lane;
            int s = 0, cnt = 0;
            if (e < nent) {
                const int row = e >> 1, side = e & 1;
                const int z = z0 + row / ny, y = y0 + row % ny;
                int xa, xb;                                             // cells xa .. xb of the row; xb < xa: none
                if (abs(z - cz) == r || abs(y - cy) == r) {
                    xa = side == 0 ? x0 : 1;
                    xb = side == 0 ? x1 : 0;
                } else {
                    xa = side == 0 ? cx - r : cx + r;
                    xb = (side == 0 ? cx - r >= 0 : cx + r < Gx) ? xa : xa - 1;
                }
                if (xb >= xa) {
                    const int base = (z * Gy + y) * Gx;
                    s = cs[base + xa];
                    cnt = cs[base + xb + 1] - s;
                }
            }
            int P = cnt;                                                // inclusive prefix over the lanes
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(P, d);
                if (lane >= d) P += o;
            }
            const int total = __builtin_amdgcn_readlane(P, 63);
            for (int b = 0; b < total; b += 64) {
                const int j = b + lane;                                 // candidate j of this batch of entries
                int L = 0;                                              // its entry: the first lane with P > j
#pragma unroll
                for (int step = 32; step > 0; step >>= 1)
                    if (__shfl(P, L + step - 1) <= j) L += step;
                const int first = __shfl(s, L) + (j - (__shfl(P, L) - __shfl(cnt, L)));
                unsigned long long key = ~0ull;
                if (j < total) {
                    const float4 p = pts[first];
                    key = ((unsigned long long)__float_as_uint(kg_sqd(qx, qy, qz, p.x, p.y, p.z)) << 32) | __float_as_uint(p.w);
                }
                if (__ballot(key < kth) == 0ull) continue;
#pragma unroll
                for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
                    for (int m = k >> 1; m > 0; m >>= 1) {              // bitonic sort, descending
                        const unsigned long long o = __shfl_xor(key, m);
                        key = (((lane & m) == 0) != ((lane & k) == 0)) ? kg_min(key, o) : kg_max(key, o);
                    }
                best = kg_min(best, key);
#pragma unroll
                for (int m = 32; m > 0; m >>= 1) {                      // bitonic merge, ascending
                    const unsigned long long o = __shfl_xor(best, m);
                    best = (lane & m) == 0 ? kg_min(best, o) : kg_max(best, o);
                }
                kth = __shfl(best, K - 1);
            }
        }
        bool face = false;
        const float bound = fminf(fminf(kg_face_bound(qx, lox, h, inv_h, Gx, cx, r, face), kg_face_bound(qy, loy, h, inv_h, Gy, cy, r, face)),
                                  kg_face_bound(qz, loz, h, inv_h, Gz, cz, r, face));
        if (!face) break;                                               // the block is the grid: every reference has been seen
        // keys are distinct; d2_K < bound <= d2 of everything unvisited puts all of it behind the K-th.  Equality does not: an
        // unvisited point at the same distance with a smaller index would come first.  (~0: fewer than K found - never below.)
        if ((unsigned)(kth >> 32) < __float_as_uint(bound)) break;
    }
    if (lane < K) {
        const size_t o = (size_t)q * K + lane;
        idx_out[o] = (int)(unsigned)(best & 0xffffffffull);
        if (dist_out) dist_out[o] = __uint_as_float((unsigned)(best >> 32));
    }
}

// B clouds (n[i] references, m[i] queries, stored back to back) in launches of up to KG_MAXB clouds
int kg_run(const float* ref, const float* query, const int* n, const int* m, int uniform_n, int uniform_m, int B, int K, void* ws,
           int* idx_out, float* dist_out, hipStream_t s) {
    long long woff = 0, roff = 0, qoff = 0;
    for (int c0 = 0; c0 < B; c0 += KG_MAXB) {
        const int nc = B - c0 < KG_MAXB ? B - c0 : KG_MAXB;
        KgTab t;
        int maxn = 0;
        for (int i = 0; i < nc; ++i) {
            const int ni = n ? n[c0 + i] : uniform_n, mi = m ? m[c0 + i] : uniform_m;
            t.woff[i] = woff; t.roff[i] = (int)roff; t.n[i] = ni; t.g[i] = kg_axis_cells(ni); t.q0[i] = (int)qoff;
            woff += kg_cloud_bytes(ni); roff += ni; qoff += mi;
            if (ni > maxn) maxn = ni;
        }
        t.q0[nc] = (int)qoff;
        for (int i = nc; i < KG_MAXB; ++i) { t.woff[i] = 0; t.roff[i] = 0; t.n[i] = 0; t.g[i] = 1; t.q0[i + 1] = (int)qoff; }
        const int nq = t.q0[nc] - t.q0[0];
        char* w = static_cast<char*>(ws);
        hipLaunchKernelGGL(kg_setup_kernel, dim3(nc), dim3(256), 0, s, ref, t, w);
        hipLaunchKernelGGL(kg_count_kernel, dim3((maxn + 255) / 256, nc), dim3(256), 0, s, ref, t, w);
        hipLaunchKernelGGL(kg_scan_kernel, dim3(nc), dim3(KG_SCAN_T), 0, s, t, w);
        hipLaunchKernelGGL(kg_scatter_kernel, dim3((maxn + 255) / 256, nc), dim3(256), 0, s, ref, t, w);
        hipLaunchKernelGGL(kg_search_kernel, dim3((nq + KG_T / 64 - 1) / (KG_T / 64)), dim3(KG_T), 0, s, query, t, nc, K, w, idx_out,
                           dist_out);
        const int rc = pf_last_launch_status();
        if (rc != PF_OK) return rc;
    }
    return PF_OK;
}

}  // namespace

extern "C" long long pf_knn_grid_ws_bytes(const int* n, int B) {
    if (!n) return PF_ERR_NULL;
    if (B <= 0) return PF_ERR_SHAPE;
    long long tot = 0;
    for (int i = 0; i < B; ++i) {
        if (n[i] <= 0) return PF_ERR_SHAPE;
        tot += kg_cloud_bytes(n[i]);
    }
    return tot;
}

extern "C" int pf_knn_grid(const float* ref, const float* query, int B, int N, int M, int K, void* ws, long long ws_bytes,
                           int* idx_out, float* dist_out, void* stream) {
    if (!ref || !query || !ws || !idx_out) return PF_ERR_NULL;
    if (B <= 0 || N <= 0 || M <= 0) return PF_ERR_SHAPE;
    if (K < 1 || K > PF_KNN_GRID_MAX_K) return PF_ERR_UNSUPPORTED;
    if (K > N || (long long)B * N * 3 > 0x7fffffffll || (long long)B * M * 3 > 0x7fffffffll || ((size_t)ws & 15) != 0) return PF_ERR_SHAPE;
    if (ws_bytes < (long long)B * kg_cloud_bytes(N)) return PF_ERR_WORKSPACE;
    return kg_run(ref, query, nullptr, nullptr, N, M, B, K, ws, idx_out, dist_out, (hipStream_t)stream);
}

extern "C" int pf_knn_grid_ragged(const float* ref, const float* query, const int* n, const int* m, int B, int K, void* ws,
                                  long long ws_bytes, int* idx_out, float* dist_out, void* stream) {
    if (!ref || !query || !n || !m || !ws || !idx_out) return PF_ERR_NULL;
    if (B <= 0) return PF_ERR_SHAPE;
    for (int i = 0; i < B; ++i)
        if (n[i] <= 0 || m[i] <= 0) return PF_ERR_SHAPE;
    if (K < 1 || K > PF_KNN_GRID_MAX_K) return PF_ERR_UNSUPPORTED;
    long long nt = 0, mt = 0, need = 0;
    for (int i = 0; i < B; ++i) {
        if (K > n[i]) return PF_ERR_SHAPE;
        nt += n[i]; mt += m[i]; need += kg_cloud_bytes(n[i]);
    }
    if (nt * 3 > 0x7fffffffll || mt * 3 > 0x7fffffffll || ((size_t)ws & 15) != 0) return PF_ERR_SHAPE;
    if (ws_bytes < need) return PF_ERR_WORKSPACE;
    return kg_run(ref, query, n, m, 0, 0, B, K, ws, idx_out, dist_out, (hipStream_t)stream);
}
