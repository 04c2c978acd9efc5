// Evaluation metrics of the reference's scoring step (evaluation/evaluate.py, evaluation/evaluation_code/evaluation.cpp):
//   pf_approxmatch_emd  - Fan et al.'s multi-level soft assignment ("approx-match" EMD, tf_ops/approxmatch), the cost / n;
//   pf_point_mesh_dist  - distance of every point to the closest point of a triangle soup (what evaluation.cpp:224-232 gets
//                         from CGAL's AABB tree: the "P2F" column).
// CD / Hausdorff and the JSD occupancy lookup are pf_nn1 (knn.hip).  Both entry points are deterministic: every sum is a
// per-workgroup partial followed by a fixed-order reduction, no float atomics, and a cloud's grid slice does not depend on
// how many clouds share the launch.
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"
#include "pf_tri.h"

namespace {

// ---- approx-match -------------------------------------------------------------------------------------------------------
// The match matrix is never stored: every level recomputes e_kl = exp(level |a_k - b_l|^2) in three sweeps,
//   A (rows):    s_k  = sum_l e_kl satR_l                           -> ratioL_k = satL_k / (1e-9 + s_k)
//   B (columns): C_l  = sum_k e_kl ratioL_k                         -> ss_l = 1e-9 + satR_l C_l, r_l = min(satR_l / ss_l, 1),
//                                                                      q_l = satR_l r_l, satR_l -= q_l C_l  (= sum_k w_kl)
//   C (rows):    W_k  = sum_l e_kl q_l,  D_k = sum_l e_kl q_l |a_k - b_l|
//                                                                   -> satL_k -= ratioL_k W_k, cost_k += ratioL_k D_k
// with w_kl = e_kl satR_l ratioL_k r_l (tf_approxmatch.cpp:31-82 in that algebra).  A sweep workgroup owns AM_T points of one
// side and one tile of AM_C points of the other side (staged in LDS with their weight); its per-point sums over that tile go to
// part[b][tile][point]; a reduction kernel adds the tiles in index order in double.  The saturations live in double.
constexpr int AM_T = 256;
constexpr int AM_C = 256;

template <bool COST>
__global__ __launch_bounds__(AM_T) void am_sweep_kernel(const float* __restrict__ P, int np, const float* __restrict__ Q,
                                                        const float* __restrict__ wq, int nq, float level,
                                                        float* __restrict__ part, float* __restrict__ part_cost) {
    __shared__ float4 sq[AM_C];
    const int b = blockIdx.z, tile = blockIdx.y, ntile = gridDim.y;
    const int q0 = tile * AM_C, cnt = min(AM_C, nq - q0);
    for (int i = threadIdx.x; i < cnt; i += AM_T) {
        const size_t g = (size_t)b * nq + q0 + i;
        sq[i] = make_float4(Q[g * 3], Q[g * 3 + 1], Q[g * 3 + 2], wq[g]);
    }
    __syncthreads();
    const int p = blockIdx.x * AM_T + threadIdx.x;
    const size_t gp = (size_t)b * np + (p < np ? p : np - 1);
    const float px = P[gp * 3], py = P[gp * 3 + 1], pz = P[gp * 3 + 2];
    float s = 0.f, c = 0.f;
    for (int i = 0; i < cnt; ++i) {
        const float4 v = sq[i];
        const float dx = px - v.x, dy = py - v.y, dz = pz - v.z;
        const float d2 = dx * dx + dy * dy + dz * dz;
        const float e = __expf(level * d2) * v.w;
        s += e;
        if (COST) c += e * __builtin_sqrtf(d2);
    }
    if (p < np) {
        const size_t o = ((size_t)b * ntile + tile) * np + p;
        part[o] = s;
        if (COST) part_cost[o] = c;
    }
}

__global__ void am_init_kernel(int n, int m, int B, double sl, double sr, double* satL, double* satR, float* satRf,
                               double* costk) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < (long long)B * n) { satL[t] = sl; costk[t] = 0.0; }
    if (t < (long long)B * m) { satR[t] = sr; satRf[t] = (float)sr; }
}

// after sweep A
__global__ void am_reduce_rows_kernel(const float* __restrict__ part, int ntile, int n, const double* __restrict__ satL,
                                      float* __restrict__ ratioL) {
    const int k = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (k >= n) return;
    double s = 1e-9;
    for (int t = 0; t < ntile; ++t) s += (double)part[((size_t)b * ntile + t) * n + k];
    const size_t g = (size_t)b * n + k;
    ratioL[g] = (float)(satL[g] / s);
}

// after sweep B
__global__ void am_reduce_cols_kernel(const float* __restrict__ part, int ntile, int m, double* __restrict__ satR,
                                      float* __restrict__ satRf, float* __restrict__ q) {
    const int l = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (l >= m) return;
    double C = 0.0;
    for (int t = 0; t < ntile; ++t) C += (double)part[((size_t)b * ntile + t) * m + l];
    const size_t g = (size_t)b * m + l;
    const double sr = satR[g];
    const double r = fmin(sr / (1e-9 + sr * C), 1.0);
    // the column's left-over capacity from the double q: where r < 1 it is satR 1e-9 / ss, far below the float rounding of
    // q (which sweep C multiplies by) - with that float q here the left-overs are rounding noise, and the rows' mass the
    // next levels route to them moves the cost of clustered clouds by 1e-3
    const double qd = sr * r;
    const double left = fmax(sr - qd * C, 0.0);
    q[g] = (float)qd;
    satR[g] = left;
    satRf[g] = (float)left;
}

// after sweep C
__global__ void am_reduce_final_kernel(const float* __restrict__ part, const float* __restrict__ part_cost, int ntile, int n,
                                       const float* __restrict__ ratioL, double* __restrict__ satL, double* __restrict__ costk) {
    const int k = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (k >= n) return;
    double W = 0.0, D = 0.0;
    for (int t = 0; t < ntile; ++t) {
        const size_t o = ((size_t)b * ntile + t) * n + k;
        W += (double)part[o];
        D += (double)part_cost[o];
    }
    const size_t g = (size_t)b * n + k;
    const double rl = (double)ratioL[g];
    satL[g] = fmax(satL[g] - rl * W, 0.0);
    costk[g] += rl * D;
}

// cost[b] = sum_k cost_k / n: one workgroup per cloud, fixed tree
__global__ __launch_bounds__(256) void am_cost_kernel(const double* __restrict__ costk, int n, float* __restrict__ out) {
    __shared__ double sh[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    for (int k = tid; k < n; k += 256) s += costk[(size_t)b * n + k];
    sh[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) sh[tid] += sh[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[b] = (float)(sh[0] / (double)n);
}

struct AmLayout {                // workspace offsets in floats (the doubles first: 8-byte aligned for an aligned ws)
    long long satL, satR, costk, satRf, ratioL, q, part, part_cost, total;
};

AmLayout am_layout(int B, int n, int m) {
    const long long tA = (m + AM_C - 1) / AM_C, tB = (n + AM_C - 1) / AM_C;
    const long long Bn = (long long)B * n, Bm = (long long)B * m;
    AmLayout L;
    L.satL = 0;
    L.satR = L.satL + 2 * Bn;
    L.costk = L.satR + 2 * Bm;
    L.satRf = L.costk + 2 * Bn;
    L.ratioL = L.satRf + Bm;
    L.q = L.ratioL + Bn;
    L.part = L.q + Bm;
    const long long pa = tA * Bn, pb = tB * Bm;
    L.part_cost = L.part + (pa > pb ? pa : pb);
    L.total = L.part_cost + pa;
    return L;
}

bool am_shape_ok(int B, int n, int m, int top) {
    return B > 0 && B <= 65535 && n > 0 && m > 0 && n <= (1 << 22) && m <= (1 << 22) && top >= -2 && top <= 15;
}

// ---- point to triangle ---------------------------------------------------------------------------------------------------
// seg_d2, tri_d2, tri_d2_rel, the seed window and the final distance: pf_tri.h, shared with tri_grid.hip
constexpr int PM_TILE = 64;      // triangles per tile = lanes of the one-wave workgroup that stages it
constexpr int PM_WAVES = 8192;   // waves the search grid aims at (points / 64 x triangle chunks)

// box [lo.xyz, 0, hi.xyz, 0] of every tile of PM_TILE consecutive triangles
__global__ void pm_box_kernel(const float* __restrict__ tris, int F, int T, float* __restrict__ box) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const int f1 = min(F, (t + 1) * PM_TILE);
    for (int f = t * PM_TILE; f < f1; ++f)
        for (int v = 0; v < 9; ++v) {
            const float x = tris[(size_t)f * 9 + v];
            lo[v % 3] = fminf(lo[v % 3], x);
            hi[v % 3] = fmaxf(hi[v % 3], x);
        }
    float* o = box + (size_t)t * 8;
    o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = 0.f;
    o[4] = hi[0]; o[5] = hi[1]; o[6] = hi[2]; o[7] = 0.f;
}

// upper bound of every point's distance: the closest of PM_SEED triangles around its seed index
__global__ void pm_seed_kernel(const float* __restrict__ pts, int P, const float* __restrict__ tris, int F,
                               const int* __restrict__ seed, float* __restrict__ sd2, int* __restrict__ sf) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float px = pts[(size_t)p * 3], py = pts[(size_t)p * 3 + 1], pz = pts[(size_t)p * 3 + 2];
    long long c, f0, f1;
    pm_seed_window(seed, p, P, F, c, f0, f1);
    float best = INFINITY;
    int bf = (int)c;
    for (long long f = f0; f < f1; ++f) {
        const float d = tri_d2_rel(tris + f * 9, px, py, pz);
        if (d < best) { best = d; bf = (int)f; }
    }
    sd2[p] = best;
    sf[p] = bf;
}

// one wave: 64 consecutive points x the tiles of one chunk.  A tile is staged in LDS only when its box is, for at least one
// lane, not farther than that lane's current best (with a margin above the rounding of both computations, so a skipped tile
// never holds a strictly better triangle: the result is the brute-force one, bit for bit).
__global__ __launch_bounds__(64) void pm_search_kernel(const float* __restrict__ pts, int P, const float* __restrict__ tris,
                                                       int F, const float* __restrict__ box, int T, int tpc, int brute,
                                                       const float* __restrict__ sd2, const int* __restrict__ sf,
                                                       float* __restrict__ pd2, int* __restrict__ pf) {
    __shared__ float4 st[PM_TILE * 3];
    const int lane = threadIdx.x, chunk = blockIdx.y;
    const int p = blockIdx.x * 64 + lane;
    const int pp = p < P ? p : P - 1;
    const float px = pts[(size_t)pp * 3], py = pts[(size_t)pp * 3 + 1], pz = pts[(size_t)pp * 3 + 2];
    const float pm = fmaxf(fabsf(px), fmaxf(fabsf(py), fabsf(pz)));
    float best = sd2[pp];
    int bf = sf[pp];
    const int t0 = chunk * tpc, t1 = min(T, t0 + tpc);
    for (int t = t0; t < t1; ++t) {
        if (!brute) {
            const float* bx = box + (size_t)t * 8;
            const float lx = bx[0], ly = bx[1], lz = bx[2], hx = bx[4], hy = bx[5], hz = bx[6];
            const float gx = fmaxf(fmaxf(lx - px, px - hx), 0.f);
            const float gy = fmaxf(fmaxf(ly - py, py - hy), 0.f);
            const float gz = fmaxf(fmaxf(lz - pz, pz - hz), 0.f);
            const float bd2 = gx * gx + gy * gy + gz * gz;
            const float sc = fmaxf(pm, fmaxf(fmaxf(fmaxf(fabsf(lx), fabsf(hx)), fmaxf(fabsf(ly), fabsf(hy))),
                                             fmaxf(fabsf(lz), fabsf(hz)))) * 1.9073486328125e-6f;     // 2^-19 x scale
            const bool need = p < P && bd2 <= best * 1.000244140625f + sc * sc;                     // 1 + 2^-12
            if (!__any(need)) continue;
        }
        const int f = t * PM_TILE + lane;
        __syncthreads();                                   // the previous tile's reads are done
        if (f < F) {
            const float* src = tris + (size_t)f * 9;
            st[lane * 3] = make_float4(src[0], src[1], src[2], src[3]);
            st[lane * 3 + 1] = make_float4(src[4], src[5], src[6], src[7]);
            st[lane * 3 + 2] = make_float4(src[8], 0.f, 0.f, 0.f);
        }
        __syncthreads();
        const int cnt = min(PM_TILE, F - t * PM_TILE);
        for (int i = 0; i < cnt; ++i) {
            const float4 a = st[i * 3], b = st[i * 3 + 1], c = st[i * 3 + 2];
            const float d = tri_d2<float>(a.x - px, a.y - py, a.z - pz, a.w - px, b.x - py, b.y - pz, b.z - px, b.w - py,
                                          c.x - pz);
            if (d < best) { best = d; bf = t * PM_TILE + i; }
        }
    }
    if (p < P) {
        pd2[(size_t)chunk * P + p] = best;
        pf[(size_t)chunk * P + p] = bf;
    }
}

// the chunks' results in chunk order (strict <: the first minimum), then the winner's distance again in double
__global__ void pm_final_kernel(const float* __restrict__ pts, int P, const float* __restrict__ tris, int nchunk,
                                const float* __restrict__ pd2, const int* __restrict__ pf, float* __restrict__ dist,
                                int* __restrict__ face) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    float best = pd2[p];
    int bf = pf[p];
    for (int c = 1; c < nchunk; ++c) {
        const float d = pd2[(size_t)c * P + p];
        if (d < best) { best = d; bf = pf[(size_t)c * P + p]; }
    }
    const double px = pts[(size_t)p * 3], py = pts[(size_t)p * 3 + 1], pz = pts[(size_t)p * 3 + 2];
    dist[p] = tri_dist_final(tris + (size_t)bf * 9, px, py, pz);
    if (face) face[p] = bf;
}

struct PmLayout {
    int T, tpc, nchunk;
    long long box, sd2, sf, pd2, pf, total;
};

PmLayout pm_layout(int P, int F) {
    PmLayout L;
    L.T = (F + PM_TILE - 1) / PM_TILE;
    const int groups = (P + 63) / 64;
    int want = (PM_WAVES + groups - 1) / groups;
    want = want < 1 ? 1 : (want > L.T ? L.T : want);
    L.tpc = (L.T + want - 1) / want;
    L.nchunk = (L.T + L.tpc - 1) / L.tpc;
    L.box = 0;
    L.sd2 = L.box + (long long)L.T * 8;
    L.sf = L.sd2 + P;
    L.pd2 = L.sf + P;
    L.pf = L.pd2 + (long long)L.nchunk * P;
    L.total = L.pf + (long long)L.nchunk * P;
    return L;
}

}  // namespace

extern "C" long long pf_approxmatch_ws_floats(int B, int n, int m, int top) {
    if (!am_shape_ok(B, n, m, top)) return PF_ERR_SHAPE;
    return am_layout(B, n, m).total;
}

extern "C" int pf_approxmatch_emd(const float* xyz1, const float* xyz2, int B, int n, int m, int top, float* cost,
                                  float* ws, long long ws_floats, void* stream) {
    if (!xyz1 || !xyz2 || !cost || !ws) return PF_ERR_NULL;
    if (!am_shape_ok(B, n, m, top)) return PF_ERR_SHAPE;
    if (((size_t)ws & 7) != 0) return PF_ERR_SHAPE;
    const AmLayout L = am_layout(B, n, m);
    if (ws_floats < L.total) return PF_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double* satL = (double*)(ws + L.satL);
    double* satR = (double*)(ws + L.satR);
    double* costk = (double*)(ws + L.costk);
    float *satRf = ws + L.satRf, *ratioL = ws + L.ratioL, *q = ws + L.q, *part = ws + L.part, *partc = ws + L.part_cost;
    const int mx = n > m ? n : m;
    const long long nm = (long long)B * mx;
    hipLaunchKernelGGL(am_init_kernel, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, s, n, m, B, (double)(mx / n),
                       (double)(mx / m), satL, satR, satRf, costk);
    const int tA = (m + AM_C - 1) / AM_C, tB = (n + AM_C - 1) / AM_C;
    const dim3 gA((n + AM_T - 1) / AM_T, tA, B), gB((m + AM_T - 1) / AM_T, tB, B);
    const dim3 rN((n + 255) / 256, B), rM((m + 255) / 256, B);
    for (int j = top; j >= -2; --j) {
        const float level = j == -2 ? 0.f : -powf(4.0f, (float)j);
        hipLaunchKernelGGL(am_sweep_kernel<false>, gA, dim3(AM_T), 0, s, xyz1, n, xyz2, satRf, m, level, part, nullptr);
        hipLaunchKernelGGL(am_reduce_rows_kernel, rN, dim3(256), 0, s, part, tA, n, satL, ratioL);
        hipLaunchKernelGGL(am_sweep_kernel<false>, gB, dim3(AM_T), 0, s, xyz2, m, xyz1, ratioL, n, level, part, nullptr);
        hipLaunchKernelGGL(am_reduce_cols_kernel, rM, dim3(256), 0, s, part, tB, m, satR, satRf, q);
        hipLaunchKernelGGL(am_sweep_kernel<true>, gA, dim3(AM_T), 0, s, xyz1, n, xyz2, q, m, level, part, partc);
        hipLaunchKernelGGL(am_reduce_final_kernel, rN, dim3(256), 0, s, part, partc, tA, n, ratioL, satL, costk);
    }
    hipLaunchKernelGGL(am_cost_kernel, dim3(B), dim3(256), 0, s, costk, n, cost);
    return pf_last_launch_status();
}

extern "C" long long pf_point_mesh_ws_floats(int P, int F) {
    if (!pm_shape_ok(P, F)) return PF_ERR_SHAPE;
    return pm_layout(P, F).total;
}

extern "C" int pf_point_mesh_dist(const float* pts, int P, const float* tris, int F, const int* seed, int brute, float* dist,
                                  int* face, float* ws, long long ws_floats, void* stream) {
    if (!pts || !tris || !dist || !ws) return PF_ERR_NULL;
    if (!pm_shape_ok(P, F)) return PF_ERR_SHAPE;
    const PmLayout L = pm_layout(P, F);
    if (ws_floats < L.total) return PF_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float *box = ws + L.box, *sd2 = ws + L.sd2, *pd2 = ws + L.pd2;
    int *sf = (int*)(ws + L.sf), *pf = (int*)(ws + L.pf);
    hipLaunchKernelGGL(pm_box_kernel, dim3((L.T + 255) / 256), dim3(256), 0, s, tris, F, L.T, box);
    hipLaunchKernelGGL(pm_seed_kernel, dim3((P + 255) / 256), dim3(256), 0, s, pts, P, tris, F, seed, sd2, sf);
    hipLaunchKernelGGL(pm_search_kernel, dim3((P + 63) / 64, L.nchunk), dim3(64), 0, s, pts, P, tris, F, box, L.T, L.tpc,
                       brute ? 1 : 0, sd2, sf, pd2, pf);
    hipLaunchKernelGGL(pm_final_kernel, dim3((P + 255) / 256), dim3(256), 0, s, pts, P, tris, L.nchunk, pd2, pf, dist, face);
    return pf_last_launch_status();
}
