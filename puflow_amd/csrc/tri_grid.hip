// Exact closest triangle over a uniform grid of the triangles (DESIGN.md section 10 "The triangle grid"): the search behind
// point_to_mesh_distance(search="grid") and the mesh scorer.  Returns, bit for bit, what pf_point_mesh_dist(brute = 1) returns -
// the arithmetic (tri_d2, the seed window, the final distance in double) is that of pf_tri.h, which both sources include - but
// evaluates the triangles of a few cells around the query instead of all of them.
//
// In the caller's workspace: a 96-byte header (box, cell edge, cell counts, totals), the cells' first pair positions, the scatter
// cursors, the oversize list and the (cell, triangle) pair list.  Seven launches: init, box, header, histogram, scan, scatter,
// search (pf_point_mesh_grid_count stops after the scan).  Integer atomics only, in the build only: box corners as order-preserving
// integers, histogram, scatter cursors, oversize append.  The order inside a cell and inside the oversize list is whatever the
// atomics made it and cannot show: the search keeps the lexicographic minimum (distance, index) of what beats the seed window,
// which does not depend on the order the candidates come in.
//
// The cell function and the stopping bound are kg_cell / kg_face_bound of pf_cells.h (shared with knn_grid.hip).  A triangle is
// registered in every cell of the block cell(min corner) .. cell(max corner) of its bounding box; by monotony of the cell function
// every vertex, hence every point of the triangle, has its cell inside that block.  After ring r a triangle not met yet has a block
// disjoint from the visited one along some axis, so ALL its points lie beyond that face: kg_face_bound's gap bounds the true
// distance from below, and the margin below covers the rounding of the fp32 triangle distance.
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"
#include "pf_cells.h"
#include "pf_tri.h"
#include "pf_wave.h"

namespace {

constexpr int TG_GMAX = 256;            // cells per axis, at most
constexpr int TG_CELLS_PER_TRI = 2;     // g = the smallest integer with g^3 >= 2 F
constexpr int TG_MAXCELLS = 64;         // a triangle whose box touches more cells goes to the oversize list
constexpr int TG_T = 256;               // search: four queries (waves) per workgroup
constexpr int TG_SCAN_T = 1024;
constexpr int TG_BOX_BLOCKS = 2048;
constexpr int TG_HEADER = 96;           // bytes
static_assert(PM_SEED <= 64, "one lane per triangle of the seed window");

struct TgHeader {                       // written by the build kernels, read by every later kernel
    float lo[3];
    float inv_h;
    int G[3];
    int ncells;
    float h;
    float amax;                         // the largest |coordinate| of the box
    unsigned enc[6];                    // the box while it is reduced: order-preserving integers, lo xyz (min) and hi xyz (max)
    int nover;                          // oversize triangles
    int pad0;
    long long npairs;                   // (cell, triangle) pairs
    int pad1[4];
};
static_assert(sizeof(TgHeader) == TG_HEADER, "header layout");

__host__ __device__ inline int tg_axis_cells(long long F) {
    int g = 1;
    while (g < TG_GMAX && (long long)g * g * g < TG_CELLS_PER_TRI * F) ++g;
    return g;
}

// header | int cstart[NC + 1] | int cursor[NC] | int over[F] | int pairs[cap], NC = g^3; rounded up to 16 bytes
struct TgLayout {
    long long nc, cstart, cursor, over, pairs, total;
};
__host__ __device__ inline TgLayout tg_layout(int F, long long cap) {
    TgLayout L;
    const long long g = tg_axis_cells(F);
    L.nc = g * g * g;
    L.cstart = TG_HEADER;
    L.cursor = L.cstart + 4 * (L.nc + 1);
    L.over = L.cursor + 4 * L.nc;
    L.pairs = L.over + 4ll * F;
    L.total = (L.pairs + 4 * (cap > 0 ? cap : 1) + 15) & ~15ll;
    return L;
}

// floats as unsigned integers of the same order (min / max by integer atomics are exact and order-free)
__device__ __forceinline__ unsigned tg_enc(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float tg_dec(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }

// ---- 1. histogram cleared, box and totals reset
__global__ __launch_bounds__(256) void tg_init_kernel(char* __restrict__ ws, long long nclear) {
    int* cs = reinterpret_cast<int*>(ws + TG_HEADER);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nclear; i += (long long)gridDim.x * 256) cs[i] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        TgHeader* hd = reinterpret_cast<TgHeader*>(ws);
        hd->enc[0] = hd->enc[1] = hd->enc[2] = 0xffffffffu;
        hd->enc[3] = hd->enc[4] = hd->enc[5] = 0u;
        hd->nover = 0;
        hd->npairs = 0;
    }
}

// ---- 2. the fp32 box of all vertices
__global__ __launch_bounds__(256) void tg_box_kernel(const float* __restrict__ tris, int F, char* __restrict__ ws) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < F; f += (long long)gridDim.x * 256) {
        const float* t = tris + f * 9;
#pragma unroll
        for (int v = 0; v < 9; ++v) {
            lo[v % 3] = fminf(lo[v % 3], t[v]);
            hi[v % 3] = fmaxf(hi[v % 3], t[v]);
        }
    }
    TgHeader* hd = reinterpret_cast<TgHeader*>(ws);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float l = pf_xor_min<1, 32>(lo[a]), h = pf_xor_max<1, 32>(hi[a]);
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&hd->enc[a], tg_enc(l));
            atomicMax(&hd->enc[3 + a], tg_enc(h));
        }
    }
}

// ---- 3. cell edge and cell counts (one thread)
__global__ void tg_header_kernel(char* __restrict__ ws, int g) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    TgHeader* hd = reinterpret_cast<TgHeader*>(ws);
    const float lx = tg_dec(hd->enc[0]), ly = tg_dec(hd->enc[1]), lz = tg_dec(hd->enc[2]);
    const float hx = tg_dec(hd->enc[3]), hy = tg_dec(hd->enc[4]), hz = tg_dec(hd->enc[5]);
    const float e = fmaxf(fmaxf(__fsub_rn(hx, lx), __fsub_rn(hy, ly)), __fsub_rn(hz, lz));
    const float ma = fmaxf(fmaxf(fmaxf(fabsf(lx), fabsf(hx)), fmaxf(fabsf(ly), fabsf(hy))), fmaxf(fabsf(lz), fabsf(hz)));
    // the floor: 16 ulps of the largest |coordinate| (a cell narrower than the coordinates' own grain sorts nothing and makes
    // the face bounds useless), and a positive number for a mesh that is one point at the origin
    float h = __fdiv_rn(e, (float)g);
    h = fmaxf(h, __fmul_rn(ma, 0x1p-19f));
    h = fmaxf(h, 0x1p-100f);
    const float inv_h = __fdiv_rn(1.f, h);
    hd->lo[0] = lx; hd->lo[1] = ly; hd->lo[2] = lz;
    hd->inv_h = inv_h;
    hd->h = h;
    hd->amax = ma;
    const int Gx = kg_cell(hx, lx, inv_h, g) + 1, Gy = kg_cell(hy, ly, inv_h, g) + 1, Gz = kg_cell(hz, lz, inv_h, g) + 1;
    hd->G[0] = Gx; hd->G[1] = Gy; hd->G[2] = Gz;
    hd->ncells = Gx * Gy * Gz;                                          // <= g^3
}

// the block of cells a triangle's box touches: c0[a] .. c1[a] on axis a (inside the grid: kg_cell clamps)
__device__ __forceinline__ int tg_block(const float* __restrict__ t, const TgHeader* hd, int (&c0)[3], int (&c1)[3]) {
    int n = 1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int u = kg_cell(t[a], hd->lo[a], hd->inv_h, hd->G[a]), v = kg_cell(t[3 + a], hd->lo[a], hd->inv_h, hd->G[a]),
                  w = kg_cell(t[6 + a], hd->lo[a], hd->inv_h, hd->G[a]);
        c0[a] = min(u, min(v, w));
        c1[a] = max(u, max(v, w));
        n *= c1[a] - c0[a] + 1;                                         // <= 256^3
    }
    return n;
}

// ---- 4. histogram; the oversize triangles appended to their list
__global__ __launch_bounds__(256) void tg_count_kernel(const float* __restrict__ tris, int F, char* __restrict__ ws, TgLayout L) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    TgHeader* hd = reinterpret_cast<TgHeader*>(ws);
    int* cs = reinterpret_cast<int*>(ws + L.cstart);
    int c0[3], c1[3];
    if (tg_block(tris + f * 9, hd, c0, c1) > TG_MAXCELLS) {
        const int pos = atomicAdd(&hd->nover, 1);
        if ((unsigned)pos < (unsigned)F) reinterpret_cast<int*>(ws + L.over)[pos] = (int)f;
        return;
    }
    const int Gx = hd->G[0], Gy = hd->G[1];
    for (int z = c0[2]; z <= c1[2]; ++z)                                // at most TG_MAXCELLS cells in all
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[0]; x <= c1[0]; ++x) atomicAdd(cs + ((z * Gy + y) * Gx + x), 1);
}

// ---- 5. exclusive scan of the histogram in place (cstart[ncells] = the pairs), copied to the scatter cursors.  One workgroup.
// The running total is 64-bit; positions beyond an int are stored as INT_MAX (the entry points refuse such a mesh's pair count).
__global__ __launch_bounds__(TG_SCAN_T) void tg_scan_kernel(char* __restrict__ ws, TgLayout L, long long* __restrict__ info) {
    __shared__ long long wsum[TG_SCAN_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    TgHeader* hd = reinterpret_cast<TgHeader*>(ws);
    const long long nce = min((long long)hd->ncells, L.nc);
    int* cs = reinterpret_cast<int*>(ws + L.cstart);
    int* cur = reinterpret_cast<int*>(ws + L.cursor);
    long long carry = 0;
    for (long long base = 0; base < nce; base += TG_SCAN_T) {           // nce <= L.nc, the host's bound
        const long long i = base + tid;
        const long long v = i < nce ? cs[i] : 0;
        long long x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long o = __shfl_up(x, d);
            if (lane >= d) x += o;
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        long long before = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < TG_SCAN_T / 64; ++k) {
            const long long s = wsum[k];
            before += k < wv ? s : 0;
            tot += s;
        }
        if (i < nce) {
            const long long ex = carry + before + x - v;
            const int e = (int)min(ex, 0x7fffffffll);
            cs[i] = e;
            cur[i] = e;
        }
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) {
        cs[nce] = (int)min(carry, 0x7fffffffll);
        hd->npairs = carry;
        if (info) {
            info[0] = carry;
            info[1] = min((long long)max(hd->nover, 0), (L.pairs - L.over) / 4);       // at most F
            info[2] = hd->G[0]; info[3] = hd->G[1]; info[4] = hd->G[2];
            info[5] = L.cstart; info[6] = L.over; info[7] = L.pairs;
        }
    }
}

// ---- 6. scatter: every (cell, triangle) pair into its cell's run.  Nothing when the list was sized for fewer pairs.
__global__ __launch_bounds__(256) void tg_scatter_kernel(const float* __restrict__ tris, int F, char* __restrict__ ws, TgLayout L,
                                                         long long cap) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const TgHeader* hd = reinterpret_cast<const TgHeader*>(ws);
    if (hd->npairs > cap) return;
    int* cur = reinterpret_cast<int*>(ws + L.cursor);
    int* pairs = reinterpret_cast<int*>(ws + L.pairs);
    int c0[3], c1[3];
    if (tg_block(tris + f * 9, hd, c0, c1) > TG_MAXCELLS) return;
    const int Gx = hd->G[0], Gy = hd->G[1];
    for (int z = c0[2]; z <= c1[2]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[0]; x <= c1[0]; ++x) {
                const int pos = atomicAdd(cur + ((z * Gy + y) * Gx + x), 1);
                if (pos >= 0 && pos < cap) pairs[pos] = (int)f;
            }
}

// ---- 7. search.  One wave per query; the state (best, face, from_seed) is wave-uniform.
// A candidate beats the state when d < best, or when d == best, the state is not the seed window's and its index is lower
// (pm_seed_kernel / pm_search_kernel / pm_final_kernel: the window's first minimiser stays unless something is strictly
// nearer, and then the lowest index of the nearest wins).  Each lane keeps the smallest key (d bits << 32 | index; d >= 0, so
// the bits order like the values) of the candidates that beat the state; the wave's minimum becomes the new state.
__global__ __launch_bounds__(TG_T) void tg_search_kernel(const float* __restrict__ pts, int P, const float* __restrict__ tris, int F,
                                                        const int* __restrict__ seed, const char* __restrict__ ws, TgLayout L,
                                                        long long cap, float* __restrict__ dist, int* __restrict__ face,
                                                        int* __restrict__ cand) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (TG_T / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (q >= P) return;                                                 // wave-uniform
    const TgHeader* hd = reinterpret_cast<const TgHeader*>(ws);
    const int* __restrict__ cs = reinterpret_cast<const int*>(ws + L.cstart);
    const int* __restrict__ over = reinterpret_cast<const int*>(ws + L.over);
    const int* __restrict__ pairs = reinterpret_cast<const int*>(ws + L.pairs);
    const float px = pts[(size_t)q * 3], py = pts[(size_t)q * 3 + 1], pz = pts[(size_t)q * 3 + 2];
    const unsigned long long NONE = ~0ull;
    auto wave_min = [](unsigned long long a, unsigned long long b) { return a < b ? a : b; };

    // the seed window: its first minimiser
    long long c, f0, f1;
    pm_seed_window(seed, q, P, F, c, f0, f1);
    unsigned long long key = NONE;
    if (f0 + lane < f1) {
        const float d = tri_d2_rel(tris + (f0 + lane) * 9, px, py, pz);
        if (d < INFINITY) key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)(f0 + lane);
    }
    key = pf_xor_reduce<1, 32>(key, wave_min);
    float best = key == NONE ? INFINITY : __uint_as_float((unsigned)(key >> 32));
    int bf = key == NONE ? (int)c : (int)(unsigned)(key & 0xffffffffull);
    bool from_seed = true;
    long long ncand = f1 - f0;

    auto eval = [&](int f) -> unsigned long long {
        f = min(max(f, 0), F - 1);
        const float d = tri_d2_rel(tris + (size_t)f * 9, px, py, pz);
        const bool wins = d < best || (d == best && !from_seed && f < bf);
        return wins ? (((unsigned long long)__float_as_uint(d) << 32) | (unsigned)f) : NONE;
    };
    auto settle = [&](unsigned long long k) {
        k = pf_xor_reduce<1, 32>(k, wave_min);
        if (k != NONE) {
            best = __uint_as_float((unsigned)(k >> 32));
            bf = (int)(unsigned)(k & 0xffffffffull);
            from_seed = false;
        }
    };

    // the oversize list - or, when the pair list was sized for fewer pairs than the mesh has, every triangle
    const bool all = hd->npairs > cap;
    const int nover = all ? F : min(max(hd->nover, 0), F);
    key = NONE;
    for (int i = lane; i < nover; i += 64) key = wave_min(key, eval(all ? i : over[i]));
    settle(key);
    ncand += nover;

    const float lox = hd->lo[0], loy = hd->lo[1], loz = hd->lo[2], inv_h = hd->inv_h, h = hd->h;
    const int Gx = min(max(hd->G[0], 1), TG_GMAX), Gy = min(max(hd->G[1], 1), TG_GMAX), Gz = min(max(hd->G[2], 1), TG_GMAX);
    const int icap = (int)min(cap, 0x7fffffffll);
    const int cx = kg_cell(px, lox, inv_h, Gx), cy = kg_cell(py, loy, inv_h, Gy), cz = kg_cell(pz, loz, inv_h, Gz);
    const float sc = fmaxf(fmaxf(fabsf(px), fabsf(py)), fmaxf(fabsf(pz), hd->amax)) * 1.9073486328125e-6f;     // 2^-19 x scale
    for (int r = 0; r <= TG_GMAX && !all && (long long)Gx * Gy * Gz <= L.nc; ++r) {
        // shell r: the cells at Chebyshev distance exactly r, clipped to the grid.  x is the fastest cell index, so a row of the
        // shell's top, bottom, front and back is one run of the pair list; the other rows give their two end cells.  Entry
        // e = 2 (row) + side: a full run (side 0 of a boundary row), one end cell, or nothing.
        const int x0 = max(cx - r, 0), x1 = min(cx + r, Gx - 1), y0 = max(cy - r, 0), y1 = min(cy + r, Gy - 1),
                  z0 = max(cz - r, 0), z1 = min(cz + r, Gz - 1);
        const int ny = y1 - y0 + 1, nent = 2 * ny * (z1 - z0 + 1);
        key = NONE;
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
                    s = min(max(cs[base + xa], 0), icap);               // a run inside the pair list, whatever the words hold
                    cnt = min(max(cs[base + xb + 1] - s, 0), icap - s);
                }
            }
            int S = cnt;                                                // inclusive prefix over the lanes
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(S, d);
                if (lane >= d) S += o;
            }
            const int total = __builtin_amdgcn_readlane(S, 63);         // the runs are disjoint: <= the pairs, an int
            for (int b = 0; b < total; b += 64) {
                const int j = b + lane;                                 // candidate j of this batch of entries
                int Ln = 0;                                             // its entry: the first lane with S > j
#pragma unroll
                for (int step = 32; step > 0; step >>= 1)
                    if (__shfl(S, Ln + step - 1) <= j) Ln += step;
                const int first = __shfl(s, Ln) + (j - (__shfl(S, Ln) - __shfl(cnt, Ln)));
                if (j < total) key = wave_min(key, eval(pairs[min(max(first, 0), max(icap - 1, 0))]));
            }
            ncand += max(total, 0);
        }
        settle(key);
        bool inner = false;
        const float bound = fminf(fminf(kg_face_bound(px, lox, h, inv_h, Gx, cx, r, inner), kg_face_bound(py, loy, h, inv_h, Gy, cy, r, inner)),
                                  kg_face_bound(pz, loz, h, inv_h, Gz, cz, r, inner));
        if (!inner) break;                                              // the block is the grid: every triangle has been seen
        // everything not met lies beyond `bound`; the margin is pm_search_kernel's for its boxes (1 + 2^-12 and 2^-19 of the
        // scale, above the rounding of the fp32 triangle distance).  Never on equality.
        if (bound > best * 1.000244140625f + sc * sc) break;
    }
    if (lane == 0) {
        dist[q] = tri_dist_final(tris + (size_t)bf * 9, px, py, pz);
        if (face) face[q] = bf;
        if (cand) cand[q] = (int)min(ncand, 0x7fffffffll);
    }
}

int tg_args_ok(const void* ws, int F) { return pm_shape_ok(1, F) && ((size_t)ws & 15) == 0; }

// init .. scan; info (nullable, device): pf_point_mesh_grid_count's record
void tg_build(const float* tris, int F, char* w, const TgLayout& L, long long* info, hipStream_t s) {
    const int fb = (F + 255) / 256;
    const long long clear_blocks = (L.nc + 1 + 255) / 256;
    hipLaunchKernelGGL(tg_init_kernel, dim3((unsigned)(clear_blocks < 4096 ? clear_blocks : 4096)), dim3(256), 0, s, w, L.nc + 1);
    hipLaunchKernelGGL(tg_box_kernel, dim3(fb < TG_BOX_BLOCKS ? fb : TG_BOX_BLOCKS), dim3(256), 0, s, tris, F, w);
    hipLaunchKernelGGL(tg_header_kernel, dim3(1), dim3(64), 0, s, w, tg_axis_cells(F));
    hipLaunchKernelGGL(tg_count_kernel, dim3(fb), dim3(256), 0, s, tris, F, w, L);
    hipLaunchKernelGGL(tg_scan_kernel, dim3(1), dim3(TG_SCAN_T), 0, s, w, L, info);
}

}  // namespace

extern "C" long long pf_point_mesh_grid_ws_bytes(int P, int F, long long pairs) {
    if (!pm_shape_ok(P, F) || pairs < 0) return PF_ERR_SHAPE;
    if (pairs > 0x7fffffffll) return PF_ERR_UNSUPPORTED;
    return tg_layout(F, pairs).total;
}

extern "C" int pf_point_mesh_grid_count(const float* tris, int F, void* ws, long long ws_bytes, long long* info, void* stream) {
    if (!tris || !ws || !info) return PF_ERR_NULL;
    if (!tg_args_ok(ws, F)) return PF_ERR_SHAPE;
    const TgLayout L = tg_layout(F, 0);
    if (ws_bytes < L.total) return PF_ERR_WORKSPACE;
    tg_build(tris, F, static_cast<char*>(ws), L, info, (hipStream_t)stream);
    return pf_last_launch_status();
}

extern "C" int pf_point_mesh_grid(const float* pts, int P, const float* tris, int F, const int* seed, float* dist, int* face,
                                  int* cand, void* ws, long long ws_bytes, long long pairs, void* stream) {
    if (!pts || !tris || !dist || !ws) return PF_ERR_NULL;
    if (!pm_shape_ok(P, F) || pairs < 0 || ((size_t)ws & 15) != 0) return PF_ERR_SHAPE;
    if (pairs > 0x7fffffffll) return PF_ERR_UNSUPPORTED;
    const TgLayout L = tg_layout(F, pairs);
    if (ws_bytes < L.total) return PF_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* w = static_cast<char*>(ws);
    tg_build(tris, F, w, L, nullptr, s);
    hipLaunchKernelGGL(tg_scatter_kernel, dim3((F + 255) / 256), dim3(256), 0, s, tris, F, w, L, pairs);
    hipLaunchKernelGGL(tg_search_kernel, dim3((P + TG_T / 64 - 1) / (TG_T / 64)), dim3(TG_T), 0, s, pts, P, tris, F, seed, w, L, pairs,
                       dist, face, cand);
    return pf_last_launch_status();
}
