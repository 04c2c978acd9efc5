// Consistent signs for estimated normals (DESIGN.md 8e "Orientation by propagation"): the second half of Hoppe et al. 1992.
// The neighbour graph {i, j : j in i's list or i in j's list, i != j} gets the weights w = max(0, 1 - |n_i . n_j|) (unfused fp32),
// its edges the strict order (w, min(i, j), max(i, j)); the minimum spanning forest under a strict order is unique, so the signs
// carried along it (a relative flip across an edge exactly when n_i . n_j < 0) are the same whatever finds the forest.  Here:
// Boruvka rounds on the device, a flip bit per vertex relative to its component's root.
//
// State per vertex, in the caller's workspace: comp (its component's root, a vertex), flip (its sign relative to that root),
// link (root << 1 | parity: the component forest of the round), and per root the round's smallest offer best_w / best_e.
// A round:  scan<0>  every directed slot (i, idx[i][k]) across two components offers its weight bits to both (atomicMin, 32 bit;
//                    the far end's only where the slot has no mirror image in the neighbour's list, which offers the same)
//           scan<1>  the slots that tie on that weight offer (min << 32 | max) (atomicMin, 64 bit)
//           hook     every root links to the root across its chosen edge, with the parity flip[a] ^ flip[b] ^ (d_ab < 0).  Under
//                    the strict order a cycle of such links is two roots that chose the SAME edge; the smaller root stays root.
//           jump     link[x] = seven links further on, parities XORed: every launch makes the links 8 times longer, and
//                    ceil((ceil(log2 M) - round) / 3) launches reach the roots, because the round starts with at most
//                    M / 2^round components.  Every value link ever holds is (an ancestor, the parity to it), so a launch may
//                    read what a neighbour thread has already advanced.
//           relabel  comp[x] = root of comp[x], flip[x] ^= parity; the offers are cleared
// ceil(log2 M) rounds always suffice (components with an edge across at least halve).  Nothing is read back: the launches are
// enqueued for that bound, a round that finds no edge across two components leaves active[round] 0 and every later launch
// returns at its first load.  The two loops in these kernels have seven steps each (a binary search, the hops of a jump); no spin,
// no barrier: a mistake gives wrong signs, never a kernel that stays.  (no_mutual_kernel loops K times, K from the host.)
// Integer atomics only (minima, and the OR that builds the mirror mask): the same bits from run to run.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <vector>
#include "pf_api_internal.h"
#include "pf_wave.h"

namespace {

constexpr int NO_MAXB = 64;             // clouds per setup launch (the table travels as a kernel argument)
constexpr int NO_T = 256;
constexpr int NO_FLAGS = 64;            // active[round]; round < 31

struct NoTab {
    int off[NO_MAXB + 1];               // first point of each cloud of the launch, and the end of the last
};

struct NoWs {
    unsigned long long* mutual;         // [T] bit k: the point is in the list of its k-th neighbour too
    unsigned long long* best_e;         // [T] per root: the smallest (min << 32 | max) among its lightest edges; then the seed key
    int* comp;                          // [T]
    unsigned* link;                     // [T] parent << 1 | parity; after the rounds, per root: the component's final flip
    unsigned* best_w;                   // [T] per root: the smallest weight bits; after the rounds: the component's smallest index
    int* cbase;                         // [T] first point of the vertex's cloud
    int* cend;                          // [T] one past its last
    int* active;                        // [NO_FLAGS]
    unsigned char* flip;                // [T]
};

inline long long no_bytes(long long T) { return (37 * T + 4 * NO_FLAGS + 15) & ~15ll; }

inline NoWs no_carve(void* ws, long long T) {
    NoWs w;
    char* p = static_cast<char*>(ws);
    w.mutual = reinterpret_cast<unsigned long long*>(p); p += 8 * T;
    w.best_e = reinterpret_cast<unsigned long long*>(p); p += 8 * T;
    w.comp = reinterpret_cast<int*>(p); p += 4 * T;
    w.link = reinterpret_cast<unsigned*>(p); p += 4 * T;
    w.best_w = reinterpret_cast<unsigned*>(p); p += 4 * T;
    w.cbase = reinterpret_cast<int*>(p); p += 4 * T;
    w.cend = reinterpret_cast<int*>(p); p += 4 * T;
    w.active = reinterpret_cast<int*>(p); p += 4 * NO_FLAGS;
    w.flip = reinterpret_cast<unsigned char*>(p);
    return w;
}

inline int no_rounds(int maxm) {        // the smallest L with 2^L >= maxm
    int L = 0;
    while ((1ll << L) < maxm) ++L;
    return L;
}

__device__ __forceinline__ float no_dot(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}
__device__ __forceinline__ float no_edge_dot(const float* __restrict__ nrm, int i, int j) {
    const float* a = nrm + (size_t)i * 3;
    const float* b = nrm + (size_t)j * 3;
    return no_dot(a[0], a[1], a[2], b[0], b[1], b[2]);
}
__device__ __forceinline__ unsigned no_weight_bits(float d) {
#pragma clang fp contract(off)
    return __float_as_uint(fmaxf(0.f, __fsub_rn(1.f, fabsf(d))));       // >= +0: the bits order as unsigned
}

// ---- setup: every vertex its own component; one launch per NO_MAXB clouds, the first also clears the round flags
__global__ __launch_bounds__(NO_T) void no_setup_kernel(const NoTab t, int nc, int first, NoWs w) {
    const int p = t.off[0] + blockIdx.x * NO_T + threadIdx.x;
    if (first && blockIdx.x == 0 && threadIdx.x < NO_FLAGS) w.active[threadIdx.x] = 0;
    if (p >= t.off[nc]) return;
    int lo = 0, hi = nc;                                                // the cloud c with off[c] <= p < off[c + 1]
#pragma unroll
    for (int s = 0; s < 7; ++s) {                                       // 2^7 > NO_MAXB
        const int mid = (lo + hi) >> 1;
        if (mid > lo && t.off[mid] <= p) lo = mid; else if (mid > lo) hi = mid;
    }
    w.cbase[p] = t.off[lo];
    w.cend[p] = t.off[lo + 1];
    w.comp[p] = p;
    w.flip[p] = 0;
    w.link[p] = (unsigned)p << 1;
    w.best_w[p] = ~0u;
    w.best_e[p] = ~0ull;
    w.mutual[p] = 0ull;
}

// ---- bit k of mutual[i]: slot (i, k) has its mirror image, i in the list of idx[i][k].  That slot makes the same offer (the dot is
// bitwise symmetric) to both ends' components, so only one of the two needs to reach each.  K <= 64 = the bits of the word.
// One lane per slot reads the neighbour's K entries (K from the host); the bits of a point's slots are ORed in the wave.
__global__ __launch_bounds__(NO_T) void no_mutual_kernel(const int* __restrict__ idx, long long slots, int K, NoWs w) {
    const long long s = (long long)blockIdx.x * NO_T + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int i = -1;
    unsigned long long bits = 0;
    if (s < slots) {
        i = slots <= 0x7fffffffll ? (int)((unsigned)s / (unsigned)K) : (int)(s / K);
        const int base = w.cbase[i], li = i - base;
        const int l = idx[s];
        if ((unsigned)l < (unsigned)(w.cend[i] - base) && l != li) {
            const int* __restrict__ row = idx + (size_t)(base + l) * K;
            bool found = false;
            for (int t = 0; t < K; ++t) found |= row[t] == li;
            if (found) bits = 1ull << (int)(s - (long long)i * K);
        }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {                                  // OR over the rest of the point's run of lanes
        const unsigned long long o = __shfl_down(bits, d);
        const int oi = __shfl_down(i, d);
        if (lane + d < 64 && oi == i) bits |= o;
    }
    const int before = __shfl_up(i, 1);
    if (i >= 0 && (lane == 0 || before != i) && bits != 0ull) atomicOr(&w.mutual[i], bits);      // a run per wave the point is in
}

// the smallest v among the lanes from this one to the end of its run of equal `run` values (runs are contiguous in the wave)
template <class T>
__device__ __forceinline__ T no_run_min(T v, int run, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_down(v, d);
        const int orun = __shfl_down(run, d);
        if (lane + d < 64 && orun == run && o < v) v = o;
    }
    return v;
}

// ---- the slot scan.  PASS 0: weights; PASS 1: (min, max) among the slots that tie on the chosen weight.
// Device-scope atomics execute at the memory side, one 64-byte request per scattered lane: they, not the gathers, set the pace.
// So the K slots of a point, which share its component, are reduced in the wave first (one offer per point and wave), the far
// end's component gets an offer only from a slot without a mirror image (the mirror image makes it at its own end), and an
// offer is only sent where it would still win: the words only ever fall, so a value read here - however stale - that is already
// at or below the offer proves that the atomic would change nothing.
template <int PASS>
__global__ __launch_bounds__(NO_T) void no_scan_kernel(const float* __restrict__ nrm, const int* __restrict__ idx, long long slots,
                                                       int K, int round, NoWs w) {
    using Offer = typename std::conditional<PASS == 0, unsigned, unsigned long long>::type;
    if (PASS == 0 ? (round > 0 && w.active[round - 1] == 0) : w.active[round] == 0) return;
    const long long s = (long long)blockIdx.x * NO_T + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool cross = false;
    int i = -1, ci = -1;
    Offer mine = ~(Offer)0;
    if (s < slots) {
        i = slots <= 0x7fffffffll ? (int)((unsigned)s / (unsigned)K) : (int)(s / K);
        ci = w.comp[i];
        const bool mirrored = (w.mutual[i] >> (int)(s - (long long)i * K)) & 1ull;
        const int base = w.cbase[i];
        const int l = idx[s];
        if ((unsigned)l < (unsigned)(w.cend[i] - base) && base + l != i) {      // an index outside the cloud is no edge
            const int j = base + l;
            const int cj = w.comp[j];
            if (ci != cj) {
                cross = true;
                const unsigned wb = no_weight_bits(no_edge_dot(nrm, i, j));
                if (PASS == 0) {
                    mine = (Offer)wb;
                    if (!mirrored && wb < PF_LD(&w.best_w[cj])) atomicMin(&w.best_w[cj], wb);
                } else {
                    const unsigned long long key = ((unsigned long long)(unsigned)min(i, j) << 32) | (unsigned)max(i, j);
                    if (w.best_w[ci] == wb) mine = (Offer)key;
                    if (!mirrored && w.best_w[cj] == wb && key < PF_LD(&w.best_e[cj])) atomicMin(&w.best_e[cj], key);
                }
            }
        }
    }
    const Offer best = no_run_min(mine, i, lane);
    const int before = __shfl_up(i, 1);
    if (i >= 0 && (lane == 0 || before != i) && best != ~(Offer)0) {            // the first lane of the point's slots in this wave
        if (PASS == 0) {
            if (best < PF_LD(&w.best_w[ci])) atomicMin(&w.best_w[ci], (unsigned)best);
        } else {
            if (best < PF_LD(&w.best_e[ci])) atomicMin(&w.best_e[ci], (unsigned long long)best);
        }
    }
    // all workgroups write the same 1: plain stores, visible to the next launch
    if (PASS == 0 && __syncthreads_or(cross) && threadIdx.x == 0 && w.active[round] == 0) w.active[round] = 1;
}

// ---- hook: every root with an edge across links to the root at the edge's other end
__global__ __launch_bounds__(NO_T) void no_hook_kernel(const float* __restrict__ nrm, int T, int round, NoWs w) {
    if (w.active[round] == 0) return;
    const int c = blockIdx.x * NO_T + threadIdx.x;
    if (c >= T || w.comp[c] != c) return;
    const unsigned long long e = w.best_e[c];
    if (e == ~0ull) return;                                             // a finished component
    const int u = (int)(e >> 32), v = (int)(e & 0xffffffffull);
    const int cu = w.comp[u], cv = w.comp[v];
    const int other = cu == c ? cv : cu;
    if ((cu != c && cv != c) || other == c) return;
    if (w.best_e[other] == e && c < other) return;                      // both chose this edge: the smaller root stays
    const unsigned par = (unsigned)(w.flip[u] ^ w.flip[v]) ^ (no_edge_dot(nrm, u, v) < 0.f ? 1u : 0u);
    w.link[c] = ((unsigned)other << 1) | par;
}

// ---- pointer jumping on the round's component forest: NO_HOPS further links from where link[x] points.  Before launch t every
// link spans at least min(depth, (NO_HOPS + 1)^t) forest edges (values of the launch before; a value a neighbour thread has
// already advanced spans more), so after it at least (NO_HOPS + 1)^(t + 1): a root's link to itself spans nothing and ends the walk.
constexpr int NO_HOPS = 7;              // 8 = 2^NO_HOP_BITS times further per launch
constexpr int NO_HOP_BITS = 3;
__global__ __launch_bounds__(NO_T) void no_jump_kernel(int T, int round, NoWs w) {
    if (w.active[round] == 0) return;
    const int x = blockIdx.x * NO_T + threadIdx.x;
    if (x >= T || w.comp[x] != x) return;                               // the round's roots only; comp is not written here
    const unsigned e = w.link[x];
    unsigned cur = e >> 1, par = e & 1u;
    if (cur == (unsigned)x) return;
#pragma unroll 1
    for (int h = 0; h < NO_HOPS; ++h) {
        const unsigned g = PF_LD(&w.link[cur]);
        par ^= g & 1u;
        if ((g >> 1) == cur) break;                                     // a root
        cur = g >> 1;
    }
    PF_ST(&w.link[x], (cur << 1) | par);
}

__global__ __launch_bounds__(NO_T) void no_relabel_kernel(int T, int round, NoWs w) {
    if (w.active[round] == 0) return;
    const int x = blockIdx.x * NO_T + threadIdx.x;
    if (x >= T) return;
    const unsigned e = w.link[w.comp[x]];
    w.comp[x] = (int)(e >> 1);
    w.flip[x] ^= (unsigned char)(e & 1u);
    w.best_w[x] = ~0u;
    w.best_e[x] = ~0ull;
}

// ---- after the rounds: the seed (largest z, or nearest to the viewpoint; the lowest index among equals) and the smallest
// index of every component.  best_e / best_w are all ones here: the last relabel that ran left them so.
__global__ __launch_bounds__(NO_T) void no_seed_kernel(const float* __restrict__ pts, int T, int has_view, float vx, float vy, float vz,
                                                       NoWs w) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * NO_T + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int c = -1;
    unsigned long long key = ~0ull;
    unsigned local = ~0u;
    if (x < T) {
        const float* p = pts + (size_t)x * 3;
        unsigned hi;
        if (has_view) {
            const float dx = __fsub_rn(p[0], vx), dy = __fsub_rn(p[1], vy), dz = __fsub_rn(p[2], vz);
            hi = __float_as_uint(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));    // >= 0
        } else {
            const unsigned b = __float_as_uint(__fadd_rn(p[2], 0.f));   // -0 -> +0: equal as numbers, equal as keys
            hi = ~((b & 0x80000000u) ? ~b : (b | 0x80000000u));         // descending z as ascending unsigned
        }
        c = w.comp[x];
        key = ((unsigned long long)hi << 32) | (unsigned)x;
        local = (unsigned)(x - w.cbase[x]);
    }
    // a whole component is often thousands of points, all after one word: runs of one component in the wave send one offer
    key = no_run_min(key, c, lane);
    local = no_run_min(local, c, lane);
    const int before = __shfl_up(c, 1);
    if (c >= 0 && (lane == 0 || before != c)) {
        if (key < PF_LD(&w.best_e[c])) atomicMin(&w.best_e[c], key);
        if (local < PF_LD(&w.best_w[c])) atomicMin(&w.best_w[c], local);
    }
}

// the component's flip: the seed's output must satisfy the sign condition
__global__ __launch_bounds__(NO_T) void no_sign_kernel(const float* __restrict__ pts, const float* __restrict__ nrm, int T, int has_view,
                                                       float vx, float vy, float vz, NoWs w) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * NO_T + threadIdx.x;
    if (c >= T || w.comp[c] != c) return;
    const int s = (int)(w.best_e[c] & 0xffffffffull);
    if ((unsigned)s >= (unsigned)T) return;
    const float sg = w.flip[s] ? -1.f : 1.f;
    const float* n = nrm + (size_t)s * 3;
    float t;
    if (has_view) {
        const float* p = pts + (size_t)s * 3;
        t = no_dot(__fmul_rn(sg, n[0]), __fmul_rn(sg, n[1]), __fmul_rn(sg, n[2]), __fsub_rn(vx, p[0]), __fsub_rn(vy, p[1]),
                   __fsub_rn(vz, p[2]));
    } else {
        t = __fmul_rn(sg, n[2]);
    }
    w.link[c] = t < 0.f ? 1u : (t == 0.f ? (unsigned)w.flip[s] : 0u);    // an exact 0: the seed keeps the sign it came with
}

__global__ __launch_bounds__(NO_T) void no_write_kernel(const float* nrm, int T, NoWs w, float* out, int* __restrict__ comp_out) {
    const int x = blockIdx.x * NO_T + threadIdx.x;
    if (x >= T) return;
    const int c = w.comp[x];
    const unsigned m = (((unsigned)w.flip[x] ^ w.link[c]) & 1u) << 31;
    const float a = nrm[(size_t)x * 3 + 0], b = nrm[(size_t)x * 3 + 1], d = nrm[(size_t)x * 3 + 2];      // out may be nrm
    out[(size_t)x * 3 + 0] = __uint_as_float(__float_as_uint(a) ^ m);
    out[(size_t)x * 3 + 1] = __uint_as_float(__float_as_uint(b) ^ m);
    out[(size_t)x * 3 + 2] = __uint_as_float(__float_as_uint(d) ^ m);
    if (comp_out) comp_out[x] = (int)w.best_w[c];
}

// B clouds of m[i] points stored back to back (T in all, the largest maxm)
int no_run(const float* pts, const float* nrm, const int* idx, const int* m, int B, long long T, int maxm, int K, const float* view,
           void* ws, float* out, int* comp_out, hipStream_t s) {
    const NoWs w = no_carve(ws, T);
    const int n = (int)T;
    long long off = 0;
    for (int c0 = 0; c0 < B; c0 += NO_MAXB) {
        const int nc = B - c0 < NO_MAXB ? B - c0 : NO_MAXB;
        NoTab t;
        for (int i = 0; i < nc; ++i) { t.off[i] = (int)off; off += m[c0 + i]; }
        for (int i = nc; i <= NO_MAXB; ++i) t.off[i] = (int)off;
        hipLaunchKernelGGL(no_setup_kernel, dim3((t.off[nc] - t.off[0] + NO_T - 1) / NO_T), dim3(NO_T), 0, s, t, nc, c0 == 0 ? 1 : 0, w);
    }
    const dim3 vg((n + NO_T - 1) / NO_T), tb(NO_T);
    const long long slots = T * K;
    const dim3 sg((unsigned)((slots + NO_T - 1) / NO_T));
    hipLaunchKernelGGL(no_mutual_kernel, sg, tb, 0, s, idx, slots, K, w);
    const int L = no_rounds(maxm);
    for (int r = 0; r < L; ++r) {
        hipLaunchKernelGGL(no_scan_kernel<0>, sg, tb, 0, s, nrm, idx, slots, K, r, w);
        hipLaunchKernelGGL(no_scan_kernel<1>, sg, tb, 0, s, nrm, idx, slots, K, r, w);
        hipLaunchKernelGGL(no_hook_kernel, vg, tb, 0, s, nrm, n, r, w);
        // the round starts with at most maxm / 2^r components per cloud: links of 2^(L - r) edges reach every root
        for (int j = 0; j < (L - r + NO_HOP_BITS - 1) / NO_HOP_BITS; ++j) hipLaunchKernelGGL(no_jump_kernel, vg, tb, 0, s, n, r, w);
        hipLaunchKernelGGL(no_relabel_kernel, vg, tb, 0, s, n, r, w);
    }
    const int hv = view ? 1 : 0;
    const float vx = view ? view[0] : 0.f, vy = view ? view[1] : 0.f, vz = view ? view[2] : 0.f;
    hipLaunchKernelGGL(no_seed_kernel, vg, tb, 0, s, pts, n, hv, vx, vy, vz, w);
    hipLaunchKernelGGL(no_sign_kernel, vg, tb, 0, s, pts, nrm, n, hv, vx, vy, vz, w);
    hipLaunchKernelGGL(no_write_kernel, vg, tb, 0, s, nrm, n, w, out, comp_out);
    return pf_last_launch_status();
}

}  // namespace

extern "C" long long pf_normals_orient_ws_bytes(const int* m, int B) {
    if (!m) return PF_ERR_NULL;
    if (B <= 0) return PF_ERR_SHAPE;
    long long T = 0;
    for (int i = 0; i < B; ++i) {
        if (m[i] <= 0) return PF_ERR_SHAPE;
        T += m[i];
    }
    return no_bytes(T);
}

extern "C" int pf_normals_orient_ragged(const float* pts, const float* normal_in, const int* idx, const int* m, int B, int K,
                                        const float* viewpoint, void* ws, long long ws_bytes, float* normal_out, int* comp_out,
                                        void* stream) {
    if (!pts || !normal_in || !idx || !m || !ws || !normal_out) return PF_ERR_NULL;
    if (B <= 0) return PF_ERR_SHAPE;
    for (int i = 0; i < B; ++i)
        if (m[i] <= 0) return PF_ERR_SHAPE;
    if (K < 2 || K > PF_KNN_GRID_MAX_K) return PF_ERR_UNSUPPORTED;
    long long T = 0;
    int maxm = 0;
    for (int i = 0; i < B; ++i) {
        if (K > m[i]) return PF_ERR_SHAPE;
        T += m[i];
        if (m[i] > maxm) maxm = m[i];
    }
    if (T * 3 > 0x7fffffffll || ((size_t)ws & 15) != 0) return PF_ERR_SHAPE;
    if (ws_bytes < no_bytes(T)) return PF_ERR_WORKSPACE;
    return no_run(pts, normal_in, idx, m, B, T, maxm, K, viewpoint, ws, normal_out, comp_out, (hipStream_t)stream);
}

extern "C" int pf_normals_orient(const float* pts, const float* normal_in, const int* idx, int B, int M, int K, const float* viewpoint,
                                 void* ws, long long ws_bytes, float* normal_out, int* comp_out, void* stream) {
    if (!pts || !normal_in || !idx || !ws || !normal_out) return PF_ERR_NULL;
    if (B <= 0 || M <= 0) return PF_ERR_SHAPE;
    if (K < 2 || K > PF_KNN_GRID_MAX_K) return PF_ERR_UNSUPPORTED;
    if (K > M || (long long)B * M * 3 > 0x7fffffffll || ((size_t)ws & 15) != 0) return PF_ERR_SHAPE;
    if (ws_bytes < no_bytes((long long)B * M)) return PF_ERR_WORKSPACE;
    const std::vector<int> m((size_t)B, M);
    return no_run(pts, normal_in, idx, m.data(), B, (long long)B * M, M, K, viewpoint, ws, normal_out, comp_out, (hipStream_t)stream);
}
