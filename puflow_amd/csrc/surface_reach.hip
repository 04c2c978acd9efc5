// Surface-connected neighbourhoods: the bottleneck field of a mesh around source points.
// For a source s on face f0, d2(f) is the squared distance from s to the closest point of triangle f (the Voronoi-region
// classification of pf_surface.h in double, relative to s, rounded once to fp32), and
//     b2(f) = min over face paths f0 = g0 .. gk = f of max_i d2(g_i)          (faces adjacent when they share a welded vertex):
// the squared radius of the smallest ball around s inside which f is connected to f0 along the surface.
//   pf_reach_count / _fill - per source the candidate faces, d2 <= r2_stop: counts, then a CSR row in ascending face index with
//                            each face's d2 (order from wave ballots and prefix counts, like pf_disk_fill);
//   pf_reach_relax         - b2 of every candidate, by sweeps of  b2(f) <- min(b2(f), max(d2(f), b2(g))), g adjacent to f;
//   pf_reach_point_d2      - max(|q - s|^2, b2(face(q))) of every (source, point) pair.
// The fixed point.  Every value the relaxation stores is the bottleneck of a real path from f0, so it never falls below b2;
// values only fall (an unsigned atomicMin on the fp32 bit pattern: non-negative floats order as unsigned integers); and after
// a sweep that lowered nothing, b2(f) <= max(d2(f), b2(g)) holds for every adjacent pair of candidates, which by induction
// along a best path gives value <= b2.  The end state is therefore b2 itself - the least fixed point of the sweep above its
// start - whatever the sweep order, the wave scheduling, S or the grid: a source's row depends on that source alone, and a
// repeat gives the same bits.  A path of bottleneck <= r2_stop uses only faces with d2 <= r2_stop, all of them candidates: every
// finite value of a row is exact, and a candidate not reached inside the ball of r2_stop stays +inf.
// One workgroup per source, no grid barrier, no co-residency requirement, no float arithmetic atomics; at most row length + 1
// sweeps (a sweep that lowers something makes at least one more face final), then PF_REACH_ST_ITER.
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"
#include "pf_surface.h"
#include "pf_wave.h"

namespace {

constexpr int SR_T = 256;                       // threads per source
constexpr int SR_W = SR_T / 64;
constexpr int SR_LDS = PF_REACH_LDS_FACES;      // row entries staged in LDS
constexpr unsigned SR_INF = 0x7f800000u;

// d2 of face f for the source (px, py, pz); a face index outside [0, F) is never read: +inf
__device__ __forceinline__ float face_d2(const float* __restrict__ tris, int F, int f, double px, double py, double pz) {
    if ((unsigned)f >= (unsigned)F) return INFINITY;
    const float* t = tris + (size_t)f * 9;
    double q[3];
    bool on_face;
    tri_closest(t[0] - px, t[1] - py, t[2] - pz, t[3] - px, t[4] - py, t[5] - pz, t[6] - px, t[7] - py, t[8] - pz, q, &on_face);
    const double d2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
    // the foot of the normal next to the source itself (its own face, coplanar neighbours): n . a cancels, see plane_d2
    if (on_face && d2 < 1e-12 * (t[0] - px) * (t[0] - px) + 1e-12 * (t[1] - py) * (t[1] - py) + 1e-12 * (t[2] - pz) * (t[2] - pz))
        return (float)plane_d2(t[0] - px, t[1] - py, t[2] - pz, t[3] - px, t[4] - py, t[5] - pz, t[6] - px, t[7] - py, t[8] - pz);
    return (float)d2;
}

// FILL = false: counts[s]; true: the row.  A source whose own face is no candidate (or no face at all) has no row.
template <bool FILL>
__global__ __launch_bounds__(SR_T) void reach_sweep_kernel(const float* __restrict__ tris, int F, const float* __restrict__ src,
                                                           const int* __restrict__ src_face, const float* __restrict__ r2_stop,
                                                           int* __restrict__ counts, const long long* __restrict__ offsets,
                                                           int* __restrict__ rface, float* __restrict__ rd2,
                                                           int* __restrict__ status) {
    __shared__ int wsum[SR_W];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double px = src[(size_t)s * 3], py = src[(size_t)s * 3 + 1], pz = src[(size_t)s * 3 + 2];
    const float stop = r2_stop[s];
    if (!(face_d2(tris, F, src_face[s], px, py, pz) <= stop)) {      // uniform over the workgroup
        if (!FILL && tid == 0) { counts[s] = 0; atomicOr(status, PF_REACH_ST_START); }
        return;
    }
    long long row = 0, cap = 0, base = 0;
    if (FILL) { row = offsets[s]; cap = offsets[s + 1] - row; }       // a row too short for its candidates is filled, not overrun
    for (int i0 = 0; i0 < F; i0 += SR_T) {                            // uniform trip count: the ballots see whole waves
        const int i = i0 + tid;
        const float d2 = i < F ? face_d2(tris, F, i, px, py, pz) : INFINITY;
        const bool in = d2 <= stop;
        const unsigned long long m = __ballot(in);
        if (!FILL) { base += __popcll(m); continue; }
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < SR_W; ++w) { const int v = wsum[w]; off += w < wave ? v : 0; tot += v; }
        const long long rank = base + off + __popcll(m & ((1ull << lane) - 1ull));
        if (in && rank < cap) { rface[row + rank] = i; rd2[row + rank] = d2; }
        base += tot;
        __syncthreads();
    }
    if (!FILL) {
        if (lane == 0) wsum[wave] = (int)base;
        __syncthreads();
        if (tid == 0) {
            int c = 0;
            for (int w = 0; w < SR_W; ++w) c += wsum[w];
            counts[s] = c;
        }
    }
}

// Loads and stores of the values go to the level of the memory every wave of the workgroup reads (agent scope: a row worked
// on in global memory is not served from a stale cache line; in LDS the scope changes nothing).
__device__ __forceinline__ void init_row(unsigned* w, const unsigned* __restrict__ d2b, int n, int k0) {
    for (int k = threadIdx.x; k < n; k += SR_T)
        PF_ST(w + k, k == k0 ? d2b[k] : SR_INF);
}

// The sweeps over one row; w holds the bit patterns of the row's values (LDS or global: the same code).  Returns the sweeps
// made, the last of which lowered nothing - or limit + 1.
__device__ __forceinline__ int relax_row(unsigned* w, const int* __restrict__ rf, const unsigned* __restrict__ d2b, int n,
                                         const long long* __restrict__ adj_off, const int* __restrict__ adj, int limit,
                                         int* changed) {
    const int tid = threadIdx.x;
    for (int sweep = 1; sweep <= limit; ++sweep) {
        if (tid == 0) *changed = 0;
        __syncthreads();
        bool any = false;
        for (int k = tid; k < n; k += SR_T) {
            const unsigned mine = d2b[k];
            unsigned cur = PF_LD(w + k);
            if (cur <= mine) continue;                                // already its own d2: nothing lower exists
            const int f = rf[k];
            unsigned best = cur;
            for (long long e = adj_off[f]; e < adj_off[f + 1]; ++e) {
                const int kg = reach_find(rf, n, adj[e]);
                if (kg < 0) continue;
                const unsigned g = PF_LD(w + kg);
                const unsigned v = g > mine ? g : mine;
                best = v < best ? v : best;
            }
            if (best < cur) { atomicMin(w + k, best); any = true; }
        }
        if (any) *changed = 1;                                        // racing stores of the same value
        __syncthreads();
        const int c = *changed;
        __syncthreads();
        if (!c) return sweep;
    }
    return limit + 1;
}

__global__ __launch_bounds__(SR_T) void reach_relax_kernel(const long long* __restrict__ offsets, const int* __restrict__ rface,
                                                           const float* __restrict__ rd2, int F,
                                                           const long long* __restrict__ adj_off, const int* __restrict__ adj,
                                                           const int* __restrict__ src_face, float* __restrict__ rb2,
                                                           int* __restrict__ sweeps, int* __restrict__ status) {
    __shared__ unsigned lw[SR_LDS];
    __shared__ int changed;
    const int s = blockIdx.x, tid = threadIdx.x;
    const long long row = offsets[s], nl = offsets[s + 1] - row;
    const int n = nl > 0 && nl <= F ? (int)nl : 0;                   // a row holds distinct faces
    if (n == 0) { if (tid == 0 && sweeps) sweeps[s] = 0; return; }
    const int* rf = rface + row;
    const unsigned* d2b = reinterpret_cast<const unsigned*>(rd2 + row);
    unsigned* gw = reinterpret_cast<unsigned*>(rb2 + row);
    const int k0 = reach_find(rf, n, src_face[s]);
    const bool lds = n <= SR_LDS;
    bool bad = false;                                                 // a face index the adjacency does not cover: such a row is
    for (int k = tid; k < n; k += SR_T) bad |= (unsigned)rf[k] >= (unsigned)F;   // never relaxed, all +inf, PF_REACH_ST_ROW
    if (lds) init_row(lw, d2b, n, k0); else init_row(gw, d2b, n, k0);
    if (tid == 0) changed = 0;
    __syncthreads();
    if (bad) changed = 1;
    __syncthreads();
    const bool badrow = changed != 0, skip = badrow || k0 < 0;
    __syncthreads();
    int done = 0;
    if (!skip) done = lds ? relax_row(lw, rf, d2b, n, adj_off, adj, n + 1, &changed)
                          : relax_row(gw, rf, d2b, n, adj_off, adj, n + 1, &changed);
    if (lds)
        for (int k = tid; k < n; k += SR_T) gw[k] = lw[k];
    if (skip) {
        __syncthreads();
        for (int k = tid; k < n; k += SR_T) gw[k] = SR_INF;
    }
    if (tid == 0) {
        if (sweeps) sweeps[s] = done;
        if (skip) atomicOr(status, badrow ? PF_REACH_ST_ROW : PF_REACH_ST_START);
        else if (done > n + 1) atomicOr(status, PF_REACH_ST_ITER);
    }
}

__global__ void reach_point_d2_kernel(const float* __restrict__ pts, int N, const float* __restrict__ src, int S, PfReach R,
                                      float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)S * N) return;
    const int s = (int)(t / N), i = (int)(t % N);
    const float d2 = seed_d2(pts + (size_t)i * 3, src[(size_t)s * 3], src[(size_t)s * 3 + 1], src[(size_t)s * 3 + 2]);
    out[t] = fmaxf(d2, reach_b2(R, s, R.face[i]));
}

bool reach_shape_ok(int F, int S) { return F > 0 && S > 0 && F <= (1 << 28) && S <= (1 << 24); }

}  // namespace

extern "C" int pf_reach_lds_faces() { return SR_LDS; }

extern "C" int pf_reach_count(const float* tris, int F, const float* src, const int* src_face, const float* r2_stop, int S,
                              int* counts, int* status, void* stream) {
    if (!tris || !src || !src_face || !r2_stop || !counts || !status) return PF_ERR_NULL;
    if (!reach_shape_ok(F, S)) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(reach_sweep_kernel<false>, dim3(S), dim3(SR_T), 0, (hipStream_t)stream, tris, F, src, src_face, r2_stop,
                       counts, (const long long*)nullptr, (int*)nullptr, (float*)nullptr, status);
    return pf_last_launch_status();
}

extern "C" int pf_reach_fill(const float* tris, int F, const float* src, const int* src_face, const float* r2_stop, int S,
                             const long long* offsets, int* rface, float* rd2, int* status, void* stream) {
    if (!tris || !src || !src_face || !r2_stop || !offsets || !rface || !rd2 || !status) return PF_ERR_NULL;
    if (!reach_shape_ok(F, S)) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(reach_sweep_kernel<true>, dim3(S), dim3(SR_T), 0, (hipStream_t)stream, tris, F, src, src_face, r2_stop,
                       (int*)nullptr, offsets, rface, rd2, status);
    return pf_last_launch_status();
}

extern "C" int pf_reach_relax(const long long* offsets, const int* rface, const float* rd2, int F,
                              const long long* face_adj_offsets, const int* face_adj, const int* src_face, int S, float* rb2,
                              int* sweeps, int* status, void* stream) {
    if (!offsets || !rface || !rd2 || !face_adj_offsets || !face_adj || !src_face || !rb2 || !status) return PF_ERR_NULL;
    if (!reach_shape_ok(F, S)) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(reach_relax_kernel, dim3(S), dim3(SR_T), 0, (hipStream_t)stream, offsets, rface, rd2, F, face_adj_offsets,
                       face_adj, src_face, rb2, sweeps, status);
    return pf_last_launch_status();
}

extern "C" int pf_reach_point_d2(const float* pts, int N, const int* pts_face, const float* src, int S,
                                 const long long* offsets, const int* rface, const float* rb2, float* out, void* stream) {
    if (!pts || !pts_face || !src || !offsets || !rface || !rb2 || !out) return PF_ERR_NULL;
    if (N <= 0 || S <= 0 || N > (1 << 26) || S > (1 << 24) || (long long)N * S > (1ll << 40)) return PF_ERR_SHAPE;
    const long long blocks = ((long long)N * S + 255) / 256;
    if (blocks > 0x7fffffffll) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(reach_point_d2_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pts, N, src, S,
                       PfReach{pts_face, offsets, rface, rb2}, out);
    return pf_last_launch_status();
}
