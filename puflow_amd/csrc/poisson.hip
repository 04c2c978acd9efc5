// Poisson-disk ("blue noise") point sets by weighted sample elimination (Yuksel 2015): a pool of s candidates on a surface of
// area A is thinned to exactly m by removing, one at a time, the candidate with the largest weight and taking its share off
// its neighbours' weights.  B pools stored back to back go through together; a pool's result depends on that pool alone.
//   pf_poisson_pools      - HOST: the per-pool table (offsets, radii as the fp32 constants the kernels compare with);
//   pf_poisson_degree     - neighbours of every candidate (d2 < R2, same pool), brute force over the pool through LDS tiles;
//   pf_poisson_graph      - the CSR rows (ascending neighbour index), the integer edge weights q and w_i = sum_j q_ij;
//   pf_poisson_rounds     - n rounds of the elimination for every pool, three launches a round, no grid barrier;
//   pf_poisson_eliminate_wg - the same rounds for pools of at most PF_POISSON_WG_MAX candidates, one workgroup per pool looping
//                           inside one launch (the rounds of a pool need only that pool's workgroup).
// The sequential process is not run.  A phase fixes tau = the (k+1)-th largest alive key, k the removals still due; a round
// removes, all at once, every alive candidate whose key exceeds tau and the keys of all its alive neighbours.  Keys only fall,
// so such a local maximum is removed by the sequential run before any neighbour and at its current weight; at most k keys
// exceed tau, so a phase cannot remove too many.  The key (w, smaller index first) is a strict total order: the kept set is
// unique and both paths return it.  Weights are integers: the atomic subtractions commute, no float atomics anywhere.
#include <hip/hip_runtime.h>
#include <cmath>
#include "pf_api_internal.h"
#include "pf_wave.h"

namespace {

typedef unsigned long long u64;

constexpr int PG_T = 256;                       // graph / select / apply: one thread per candidate
constexpr int PE_T = 1024;                      // one workgroup per pool: round bookkeeping, tau, the single-workgroup path
constexpr int PE_W = PE_T / 64;
constexpr int PATH_WG = 1;

struct PoolScratch {                            // LDS of the per-pool workgroup
    int hist[256];
    int wsum[PE_W];
    int cnt[2];
    int go;
    int sel;
    int rank;
    u64 prefix;
};

// the elimination's state (w, state) changes under other waves between barriers: it is read and written with PF_LD / PF_ST,
// never served from a stale line

// larger key = removed earlier: the weight, then the smaller index
__device__ __forceinline__ u64 make_key(unsigned w, int i) { return ((u64)w << 32) | (u64)(0xFFFFFFFFu - (unsigned)i); }

// ---- the graph ------------------------------------------------------------------------------------------------------------
// q_ij of a pair at squared distance d2 < R2; every operation a separate fp32 rounding, the square root correctly rounded
__device__ __forceinline__ unsigned edge_weight(float d2, float inv, float lo) {
    const float d = sqrtf(d2);
    const float x = fmaxf(__fsub_rn(1.0f, __fmul_rn(fmaxf(d, lo), inv)), 0.0f);
    const float x2 = __fmul_rn(x, x), x4 = __fmul_rn(x2, x2), x8 = __fmul_rn(x4, x4);
    return (unsigned)rintf(__fmul_rn(x8, 65536.0f));
}

template <bool FILL>
__global__ __launch_bounds__(PG_T) void graph_kernel(const float* __restrict__ pts, const PfPoissonPool* __restrict__ pools,
                                                     const long long* __restrict__ offsets, int* __restrict__ deg,
                                                     int* __restrict__ nbr, int* __restrict__ q, unsigned* __restrict__ w,
                                                     int* __restrict__ status) {
    __shared__ float sx[PG_T], sy[PG_T], sz[PG_T];
    const PfPoissonPool P = pools[blockIdx.y];
    const int tid = threadIdx.x, i = blockIdx.x * PG_T + tid;
    if (blockIdx.x * PG_T >= P.s) return;        // the whole workgroup: the grid is sized for the largest pool
    const bool live = i < P.s;
    const float* __restrict__ p = pts + (size_t)P.off * 3;
    float ax = 0.f, ay = 0.f, az = 0.f;
    long long e = 0, cap = 0;
    if (live) {
        ax = p[(size_t)i * 3]; ay = p[(size_t)i * 3 + 1]; az = p[(size_t)i * 3 + 2];
        if (FILL) { e = offsets[P.off + i]; cap = offsets[P.off + i + 1]; }
    }
    int cnt = 0;
    u64 wsum = 0;
    for (int j0 = 0; j0 < P.s; j0 += PG_T) {
        __syncthreads();
        if (j0 + tid < P.s) {
            sx[tid] = p[(size_t)(j0 + tid) * 3]; sy[tid] = p[(size_t)(j0 + tid) * 3 + 1]; sz[tid] = p[(size_t)(j0 + tid) * 3 + 2];
        }
        __syncthreads();
        const int n = min(PG_T, P.s - j0);
        if (live)
            for (int jj = 0; jj < n; ++jj) {
                const float dx = __fsub_rn(sx[jj], ax), dy = __fsub_rn(sy[jj], ay), dz = __fsub_rn(sz[jj], az);
                const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                if (d2 < P.R2 && j0 + jj != i) {
                    ++cnt;
                    if (FILL) {
                        const unsigned qq = edge_weight(d2, P.inv, P.lo);
                        if (e < cap) { nbr[e] = j0 + jj; q[e] = (int)qq; ++e; }   // a row too short is filled, not overrun
                        wsum += qq;
                    }
                }
            }
    }
    if (!live) return;
    if (!FILL) {
        deg[P.off + i] = cnt;
        if (cnt >= 65535) atomicOr(status, PF_POISSON_ST_DEGREE);
    } else {
        w[P.off + i] = (unsigned)wsum;
        if (wsum > 0xFFFFFFFFull) atomicOr(status, PF_POISSON_ST_WEIGHT);
    }
}

// ---- one round, in three steps --------------------------------------------------------------------------------------------
// state[i]: bit 0 = alive, bit 1 = picked for removal in this round.  All indices are inside the pool.

// Step 1, the pool's workgroup (PE_T threads): is the phase over, is the pool done, the next tau.  Returns whether steps 2 and
// 3 have work in this round.  Ends on a barrier.
__device__ bool round_begin(const PfPoissonPool& P, const unsigned* w, const int* state, PfPoissonState* st, int* keep,
                            PoolScratch& sm) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    w += P.off; state += P.off;
    if (tid == 0) { sm.cnt[0] = 0; sm.cnt[1] = 0; sm.go = 0; }
    __syncthreads();
    if (st->done) return false;                  // uniform: nobody writes it before the next barrier
    const u64 tau = st->tau;
    const int phases = st->phases;
    int alive = 0, above = 0;
    for (int i = tid; i < P.s; i += PE_T)
        if (PF_LD(state + i) & 1) { ++alive; above += make_key(PF_LD(w + i), i) > tau; }
    for (int o = 32; o > 0; o >>= 1) { alive += __shfl_down(alive, o); above += __shfl_down(above, o); }
    if (lane == 0) { atomicAdd(&sm.cnt[0], alive); atomicAdd(&sm.cnt[1], above); }
    __syncthreads();
    alive = sm.cnt[0]; above = sm.cnt[1];
    if (phases > 0 && above > 0) {               // the phase goes on
        __syncthreads();
        if (tid == 0) st->rounds += 1;
        return true;
    }
    const int k = alive - P.m;
    if (k <= 0) {                                // done: the alive indices in ascending order
        int base = 0;
        for (int i0 = 0; i0 < P.s; i0 += PE_T) {
            const int i = i0 + tid;
            const bool in = i < P.s && (PF_LD(state + i) & 1);
            const u64 b = __ballot(in);
            if (lane == 0) sm.wsum[wave] = __popcll(b);
            __syncthreads();
            int off = 0, tot = 0;
#pragma unroll
            for (int v = 0; v < PE_W; ++v) { const int c = sm.wsum[v]; off += v < wave ? c : 0; tot += c; }
            const int rank = base + off + __popcll(b & ((1ull << lane) - 1ull));
            if (in && rank < P.m) keep[P.out_off + rank] = i;
            base += tot;
            __syncthreads();
        }
        if (tid == 0) { st->done = 1; st->alive = alive; }
        return false;
    }
    // tau = the (k+1)-th largest alive key: most significant byte first, 256 bins a pass
    if (tid == 0) { sm.prefix = 0; sm.rank = k + 1; }
    for (int b = 7; b >= 0; --b) {
        if (tid < 256) sm.hist[tid] = 0;
        __syncthreads();
        const u64 prefix = sm.prefix;
        for (int i = tid; i < P.s; i += PE_T)
            if (PF_LD(state + i) & 1) {
                const u64 key = make_key(PF_LD(w + i), i);
                if (b == 7 || (key >> (8 * (b + 1))) == (prefix >> (8 * (b + 1)))) atomicAdd(&sm.hist[(int)((key >> (8 * b)) & 255)], 1);
            }
        __syncthreads();
        if (tid == 0) {
            int c = 0, r = sm.rank, bin = 255;
            for (; bin > 0; --bin) {
                if (c + sm.hist[bin] >= r) break;
                c += sm.hist[bin];
            }
            sm.rank = r - c;
            sm.prefix = prefix | ((u64)bin << (8 * b));
        }
        __syncthreads();
    }
    if (tid == 0) { st->tau = sm.prefix; st->k = k; st->alive = alive; st->phases = phases + 1; st->rounds += 1; }
    __syncthreads();
    return true;
}

// Step 2, candidate i: picked when alive, above tau and above every alive neighbour.  Reads keys, writes its own state only.
__device__ __forceinline__ void round_select(const PfPoissonPool& P, u64 tau, const long long* __restrict__ offsets,
                                             const int* __restrict__ nbr, const unsigned* w, int* state, int i) {
    if (!(PF_LD(state + P.off + i) & 1)) return;
    const u64 key = make_key(PF_LD(w + P.off + i), i);
    if (key <= tau) return;
    const long long e1 = offsets[P.off + i + 1];
    for (long long e = offsets[P.off + i]; e < e1; ++e) {
        const int j = nbr[e];
        if ((unsigned)j >= (unsigned)P.s) continue;                       // a foreign graph: never outside the pool
        if ((PF_LD(state + P.off + j) & 1) && make_key(PF_LD(w + P.off + j), j) > key) return;
    }
    PF_ST(state + P.off + i, 3);
}

// Step 3, candidate i if picked: dies, and its alive neighbours lose q_ij.  No two neighbours are picked in one round.
__device__ __forceinline__ void round_apply(const PfPoissonPool& P, const long long* __restrict__ offsets,
                                            const int* __restrict__ nbr, const int* __restrict__ q, unsigned* w, int* state,
                                            int i) {
    if (PF_LD(state + P.off + i) != 3) return;
    PF_ST(state + P.off + i, 0);
    const long long e1 = offsets[P.off + i + 1];
    for (long long e = offsets[P.off + i]; e < e1; ++e) {
        const int j = nbr[e];
        if ((unsigned)j >= (unsigned)P.s) continue;
        if (PF_LD(state + P.off + j) & 1) atomicSub(w + P.off + j, (unsigned)q[e]);
    }
}

__global__ __launch_bounds__(PE_T) void begin_kernel(const PfPoissonPool* __restrict__ pools, const unsigned* w, const int* state,
                                                     PfPoissonState* st, int* keep, int round_id, int* unfinished) {
    __shared__ PoolScratch sm;
    const PfPoissonPool P = pools[blockIdx.x];
    if (P.path == PATH_WG) return;
    if (round_begin(P, w, state, st + blockIdx.x, keep, sm) && threadIdx.x == 0) PF_ST(unfinished, round_id + 1);
}

__global__ __launch_bounds__(PG_T) void select_kernel(const PfPoissonPool* __restrict__ pools, const PfPoissonState* __restrict__ st,
                                                      const long long* __restrict__ offsets, const int* __restrict__ nbr,
                                                      const unsigned* w, int* state) {
    const PfPoissonPool P = pools[blockIdx.y];
    const int i = blockIdx.x * PG_T + threadIdx.x;
    if (P.path == PATH_WG || i >= P.s || st[blockIdx.y].done) return;
    round_select(P, st[blockIdx.y].tau, offsets, nbr, w, state, i);
}

__global__ __launch_bounds__(PG_T) void apply_kernel(const PfPoissonPool* __restrict__ pools, const PfPoissonState* __restrict__ st,
                                                     const long long* __restrict__ offsets, const int* __restrict__ nbr,
                                                     const int* __restrict__ q, unsigned* w, int* state) {
    const PfPoissonPool P = pools[blockIdx.y];
    const int i = blockIdx.x * PG_T + threadIdx.x;
    if (P.path == PATH_WG || i >= P.s || st[blockIdx.y].done) return;
    round_apply(P, offsets, nbr, q, w, state, i);
}

// the three steps in a loop, one workgroup per pool: its barriers order them (the pool's state is touched by no other workgroup)
__global__ __launch_bounds__(PE_T) void eliminate_wg_kernel(const PfPoissonPool* __restrict__ pools, const long long* __restrict__ offsets,
                                                            const int* __restrict__ nbr, const int* __restrict__ q, unsigned* w,
                                                            int* state, PfPoissonState* st, int* keep) {
    __shared__ PoolScratch sm;
    const PfPoissonPool P = pools[blockIdx.x];
    if (P.path != PATH_WG) return;
    PfPoissonState* s = st + blockIdx.x;
    for (int guard = 0; guard <= P.s; ++guard) {  // every round removes at least one candidate
        if (!round_begin(P, w, state, s, keep, sm)) break;
        const u64 tau = s->tau;
        for (int i = threadIdx.x; i < P.s; i += PE_T) round_select(P, tau, offsets, nbr, w, state, i);
        __syncthreads();
        for (int i = threadIdx.x; i < P.s; i += PE_T) round_apply(P, offsets, nbr, q, w, state, i);
        __syncthreads();
    }
}

__global__ void init_state_kernel(const PfPoissonPool* __restrict__ pools, int* state) {
    const PfPoissonPool P = pools[blockIdx.y];
    const int i = blockIdx.x * PG_T + threadIdx.x;
    if (i < P.s) state[P.off + i] = 1;
}

bool shape_ok(int B, int max_s, long long total) {
    return B > 0 && B <= 65535 && max_s > 0 && total >= max_s && total <= PF_POISSON_MAX_TOTAL;
}

}  // namespace

extern "C" int pf_poisson_params(double area, int s, int m, double* r_max, double* r_min, float* consts) {
    if (!(area > 0.0) || !(area < 1e30) || m < 1 || m > s) return PF_ERR_SHAPE;
    const double t = (double)m / (double)s;
    const double rmax = std::sqrt(area / (2.0 * std::sqrt(3.0) * (double)m));
    const double rmin = rmax * (1.0 - t * std::sqrt(t)) * 0.65;
    if (r_max) *r_max = rmax;
    if (r_min) *r_min = rmin;
    if (consts) {
        consts[0] = (float)((2.0 * rmax) * (2.0 * rmax));
        consts[1] = (float)(1.0 / (2.0 * rmax));
        consts[2] = (float)(2.0 * rmin);
    }
    return PF_OK;
}

extern "C" int pf_poisson_pools(const int* s, const int* m, const double* area, int B, int flags, PfPoissonPool* pools) {
    if (!s || !m || !area || !pools) return PF_ERR_NULL;
    if (B <= 0 || B > 65535) return PF_ERR_SHAPE;
    long long off = 0, out = 0;
    for (int b = 0; b < B; ++b) {
        float c[3];
        if (s[b] < 1) return PF_ERR_SHAPE;
        const int rc = pf_poisson_params(area[b], s[b], m[b], nullptr, nullptr, c);
        if (rc != PF_OK) return rc;
        if (off + s[b] > PF_POISSON_MAX_TOTAL) return PF_ERR_SHAPE;
        PfPoissonPool& P = pools[b];
        P.off = (int)off; P.s = s[b]; P.m = m[b]; P.out_off = (int)out;
        P.R2 = c[0]; P.inv = c[1]; P.lo = c[2];
        P.path = (s[b] <= PF_POISSON_WG_MAX && !(flags & PF_POISSON_NO_WG)) ? PATH_WG : 0;
        off += s[b]; out += m[b];
    }
    return PF_OK;
}

extern "C" int pf_poisson_degree(const float* pts, const PfPoissonPool* pools, int B, int max_s, long long total, int* deg,
                                 int* status, void* stream) {
    if (!pts || !pools || !deg || !status) return PF_ERR_NULL;
    if (!shape_ok(B, max_s, total)) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(graph_kernel<false>, dim3((max_s + PG_T - 1) / PG_T, B), dim3(PG_T), 0, (hipStream_t)stream, pts, pools,
                       (const long long*)nullptr, deg, (int*)nullptr, (int*)nullptr, (unsigned*)nullptr, status);
    return pf_last_launch_status();
}

extern "C" int pf_poisson_graph(const float* pts, const PfPoissonPool* pools, int B, int max_s, long long total,
                                const long long* offsets, int* nbr, int* q, unsigned* w, int* status, void* stream) {
    if (!pts || !pools || !offsets || !nbr || !q || !w || !status) return PF_ERR_NULL;
    if (!shape_ok(B, max_s, total)) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(graph_kernel<true>, dim3((max_s + PG_T - 1) / PG_T, B), dim3(PG_T), 0, (hipStream_t)stream, pts, pools,
                       offsets, (int*)nullptr, nbr, q, w, status);
    return pf_last_launch_status();
}

extern "C" int pf_poisson_begin(const PfPoissonPool* pools, int B, int max_s, long long total, int* state, PfPoissonState* st,
                                void* stream) {
    if (!pools || !state || !st) return PF_ERR_NULL;
    if (!shape_ok(B, max_s, total)) return PF_ERR_SHAPE;
    if (hipMemsetAsync(st, 0, sizeof(PfPoissonState) * (size_t)B, (hipStream_t)stream) != hipSuccess) return PF_ERR_LAUNCH;
    hipLaunchKernelGGL(init_state_kernel, dim3((max_s + PG_T - 1) / PG_T, B), dim3(PG_T), 0, (hipStream_t)stream, pools, state);
    return pf_last_launch_status();
}

extern "C" int pf_poisson_eliminate_wg(const PfPoissonPool* pools, int B, const long long* offsets, const int* nbr, const int* q,
                                       unsigned* w, int* state, PfPoissonState* st, int* keep, void* stream) {
    if (!pools || !offsets || !nbr || !q || !w || !state || !st || !keep) return PF_ERR_NULL;
    if (B <= 0 || B > 65535) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(eliminate_wg_kernel, dim3(B), dim3(PE_T), 0, (hipStream_t)stream, pools, offsets, nbr, q, w, state, st, keep);
    return pf_last_launch_status();
}

extern "C" int pf_poisson_rounds(const PfPoissonPool* pools, int B, int max_s, long long total, const long long* offsets,
                                 const int* nbr, const int* q, unsigned* w, int* state, PfPoissonState* st, int* keep,
                                 int round0, int n_rounds, int* unfinished, void* stream) {
    if (!pools || !offsets || !nbr || !q || !w || !state || !st || !keep || !unfinished) return PF_ERR_NULL;
    if (!shape_ok(B, max_s, total) || round0 < 0 || n_rounds < 1 || n_rounds > 4096 || round0 > (1 << 30)) return PF_ERR_SHAPE;
    const dim3 grid((max_s + PG_T - 1) / PG_T, B);
    for (int r = round0; r < round0 + n_rounds; ++r) {
        hipLaunchKernelGGL(begin_kernel, dim3(B), dim3(PE_T), 0, (hipStream_t)stream, pools, w, state, st, keep, r, unfinished);
        hipLaunchKernelGGL(select_kernel, grid, dim3(PG_T), 0, (hipStream_t)stream, pools, st, offsets, nbr, w, state);
        hipLaunchKernelGGL(apply_kernel, grid, dim3(PG_T), 0, (hipStream_t)stream, pools, st, offsets, nbr, q, w, state);
    }
    return pf_last_launch_status();
}
