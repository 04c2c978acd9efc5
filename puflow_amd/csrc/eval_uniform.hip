// Uniformity of an upsampled cloud on its mesh (PU-GAN's measure; the reference's evaluation/evaluate.py:105-165
// analyze_uniform, with the disks its CGAL binary was meant to write - evaluation.cpp calculate_density - made here):
//   pf_tri_closest_points - the closest point of a given triangle to every point (the "mapped" points, evaluation.cpp:225-228);
//   pf_mesh_sample        - S seed points on the surface, area-weighted, from Philox-4x32-10 (key = seed, counter = s);
//   pf_disk_count / _fill - the mapped points inside the Euclidean balls of J nested radii around every seed: counts, then a
//                           CSR of the largest ball's members in ascending index order with each member's level;
//   pf_disk_count_reach / _fill_reach - the same kernels with the surface distance max(|q - s|^2, b2(face(q))) in place of
//                           |q - s|^2, b2 from the seed's row of a reach CSR (surface_reach.hip);
//   pf_disk_uniformity    - per (seed, radius): member count and the mean of (d - d^)^2 / d^ over the members, d the distance
//                           to the nearest other member of the same disk.
// One workgroup per seed everywhere a seed is swept; ordered compaction by wave ballots and prefix counts, sums in double in
// a fixed order, no float atomics: a repeat gives the same bits, and a seed's result does not depend on the seeds beside it.
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"
#include "pf_philox.h"
#include "pf_surface.h"

namespace {

constexpr int DU_T = 256;                       // threads per seed
constexpr int DU_W = DU_T / 64;
constexpr int DU_J = PF_DISK_MAX_RADII;
constexpr int DU_TILE = PF_DISK_TILE;           // members staged in LDS at a time

__global__ void closest_points_kernel(const float* __restrict__ pts, int P, const float* __restrict__ tris, int F,
                                      const int* __restrict__ face, float* __restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int f = face[p];
    float* o = out + (size_t)p * 3;
    if ((unsigned)f >= (unsigned)F) { o[0] = o[1] = o[2] = __builtin_nanf(""); return; }   // never read outside the mesh
    const double px = pts[(size_t)p * 3], py = pts[(size_t)p * 3 + 1], pz = pts[(size_t)p * 3 + 2];
    const float* t = tris + (size_t)f * 9;
    double q[3];
    tri_closest(t[0] - px, t[1] - py, t[2] - pz, t[3] - px, t[4] - py, t[5] - pz, t[6] - px, t[7] - py, t[8] - pz, q);
    o[0] = (float)(px + q[0]); o[1] = (float)(py + q[1]); o[2] = (float)(pz + q[2]);
}

// ---- seeds ----------------------------------------------------------------------------------------------------------------
// Seed s: words (x0, x1, x2) of counter (s, 0, 0, 0) -> u0, u1, u2.  Face: the first f with cum[f] > u0 * cum[F-1] (double;
// zero-area faces are never taken).  Position: (1 - sqrt(u1)) a + sqrt(u1) (1 - u2) b + sqrt(u1) u2 c, in double.
__global__ void mesh_sample_kernel(const float* __restrict__ tris, int F, const double* __restrict__ cum, int S, unsigned k0,
                                   unsigned k1, float* __restrict__ seeds, int* __restrict__ face, float* __restrict__ uni) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const U4 w = philox((unsigned)s, 0u, 0u, 0u, k0, k1);
    const float u0 = u01(w.x), u1 = u01(w.y), u2 = u01(w.z);
    const double target = (double)u0 * cum[F - 1];
    int lo = 0, hi = F - 1;                      // the answer is in [lo, hi]; F - 1 when no cum[f] exceeds the target
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (cum[mid] > target) hi = mid; else lo = mid + 1;
    }
    const float* t = tris + (size_t)lo * 9;
    const double r = sqrt((double)u1), wa = 1.0 - r, wb = r * (1.0 - (double)u2), wc = r * (double)u2;
#pragma unroll
    for (int c = 0; c < 3; ++c) seeds[(size_t)s * 3 + c] = (float)(wa * t[c] + wb * t[3 + c] + wc * t[6 + c]);
    face[s] = lo;
    uni[(size_t)s * 3] = u0; uni[(size_t)s * 3 + 1] = u1; uni[(size_t)s * 3 + 2] = u2;
}

// ---- disks ----------------------------------------------------------------------------------------------------------------
struct R2 { float v[DU_J]; };                   // squared radii, ascending; unused slots hold the largest
struct RD { double v[DU_J]; };                  // the radii themselves

// the smallest j with D2 <= r_j^2, J when the point is outside every disk.  D2 = |q - seed|^2 (pf_surface.h seed_d2); REACH:
// the larger of that and the bottleneck value of the point's face in the seed's reach row (+inf for a face not in it)
template <bool REACH>
__device__ __forceinline__ int disk_level(const float* __restrict__ mapped, int i, int s, float sx, float sy, float sz,
                                          const R2& r2, int J, const PfReach& R) {
    float d2 = seed_d2(mapped + (size_t)i * 3, sx, sy, sz);
    if (REACH) d2 = fmaxf(d2, reach_b2(R, s, R.face[i]));
    int lev = J;
#pragma unroll
    for (int j = DU_J - 1; j >= 0; --j)
        if (j < J && d2 <= r2.v[j]) lev = j;
    return lev;
}

template <bool REACH>
__global__ __launch_bounds__(DU_T) void disk_count_kernel(const float* __restrict__ mapped, int N, const float* __restrict__ seeds,
                                                          R2 r2, int J, int* __restrict__ counts, PfReach R) {
    __shared__ int wcnt[DU_W][DU_J];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float sx = seeds[(size_t)s * 3], sy = seeds[(size_t)s * 3 + 1], sz = seeds[(size_t)s * 3 + 2];
    int cnt[DU_J];
#pragma unroll
    for (int j = 0; j < DU_J; ++j) cnt[j] = 0;
    for (int i0 = 0; i0 < N; i0 += DU_T) {       // uniform trip count: the ballots see whole waves
        const int i = i0 + tid;
        const int lev = i < N ? disk_level<REACH>(mapped, i, s, sx, sy, sz, r2, J, R) : J;
#pragma unroll
        for (int j = 0; j < DU_J; ++j) cnt[j] += __popcll(__ballot(lev <= j));
    }
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < DU_J; ++j) wcnt[wave][j] = cnt[j];
    __syncthreads();
    if (tid < J) {
        int c = 0;
        for (int w = 0; w < DU_W; ++w) c += wcnt[w][tid];
        counts[(size_t)s * J + tid] = c;
    }
}

template <bool REACH>
__global__ __launch_bounds__(DU_T) void disk_fill_kernel(const float* __restrict__ mapped, int N, const float* __restrict__ seeds,
                                                         R2 r2, int J, const long long* __restrict__ offsets,
                                                         int* __restrict__ member, int* __restrict__ level, PfReach R) {
    __shared__ int wsum[DU_W];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float sx = seeds[(size_t)s * 3], sy = seeds[(size_t)s * 3 + 1], sz = seeds[(size_t)s * 3 + 2];
    const long long row = offsets[s], cap = offsets[s + 1] - row;        // a row too short for its disk is filled, not overrun
    long long base = 0;
    for (int i0 = 0; i0 < N; i0 += DU_T) {
        const int i = i0 + tid;
        const int lev = i < N ? disk_level<REACH>(mapped, i, s, sx, sy, sz, r2, J, R) : J;
        const bool in = lev < J;
        const unsigned long long m = __ballot(in);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < DU_W; ++w) { const int v = wsum[w]; off += w < wave ? v : 0; tot += v; }
        const long long rank = base + off + __popcll(m & ((1ull << lane) - 1ull));
        if (in && rank < cap) { member[row + rank] = i; level[row + rank] = lev; }
        base += tot;
        __syncthreads();
    }
}

// ---- the statistic --------------------------------------------------------------------------------------------------------
// Row s of the CSR: members k = 0 .. n-1 (point index, level).  Member k belongs to disk j when level_k <= j.  Thread t owns
// members t, t + 256, ...; for each it sweeps every member of the row (staged DU_TILE at a time in LDS; a row longer than a
// tile is re-staged per pass over it) and keeps, per j, the smallest squared distance to another member of disk j.  Members
// are staged as stored: the difference of two fp32 coordinates is correctly rounded wherever the origin lies, so a
// seed-relative copy would only add a rounding - and disks read from files come without seeds.
__global__ __launch_bounds__(DU_T) void disk_uniformity_kernel(const float* __restrict__ mapped, int N,
                                                               const long long* __restrict__ offsets,
                                                               const int* __restrict__ member, const int* __restrict__ level,
                                                               RD radii, int J, double* __restrict__ out_n,
                                                               double* __restrict__ out_dis) {
    __shared__ float4 sm[DU_TILE];               // x y z, level in the bits of w
    __shared__ double red[DU_T];
    __shared__ int wcnt[DU_W][DU_J];
    __shared__ int nj[DU_J];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row = offsets[s];
    const long long nl = offsets[s + 1] - row;
    const int n = nl < 0 ? 0 : (int)nl;
    const int* __restrict__ mem = member + row;
    const int* __restrict__ lev = level + row;

    // members per disk
    int cnt[DU_J];
#pragma unroll
    for (int j = 0; j < DU_J; ++j) cnt[j] = 0;
    for (int k0 = 0; k0 < n; k0 += DU_T) {
        const int k = k0 + tid;
        const int l = k < n ? lev[k] : DU_J;
#pragma unroll
        for (int j = 0; j < DU_J; ++j) cnt[j] += __popcll(__ballot(l <= j));
    }
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < DU_J; ++j) wcnt[wave][j] = cnt[j];
    __syncthreads();
    if (tid < DU_J) {
        int c = 0;
        for (int w = 0; w < DU_W; ++w) c += wcnt[w][tid];
        nj[tid] = c;
    }
    __syncthreads();
    double expect[DU_J];                          // d^_j = sqrt(2 (pi r_j^2 / n_j) / 1.732), the spacing of a hexagonal packing
#pragma unroll
    for (int j = 0; j < DU_J; ++j)
        expect[j] = j < J && nj[j] > 0 ? sqrt(2.0 * (3.14159265358979323846 * radii.v[j] * radii.v[j] / (double)nj[j]) / 1.732) : 0.0;

    double acc[DU_J];
#pragma unroll
    for (int j = 0; j < DU_J; ++j) acc[j] = 0.0;
    const int ntile = (n + DU_TILE - 1) / DU_TILE;
    for (int a0 = 0; a0 < n; a0 += DU_T) {       // uniform over the workgroup
        const int ka = a0 + tid;
        const bool live = ka < n;
        float ax = 0.f, ay = 0.f, az = 0.f;
        int la = DU_J;
        if (live) {
            const int ia = min(max(mem[ka], 0), N - 1);
            ax = mapped[(size_t)ia * 3]; ay = mapped[(size_t)ia * 3 + 1]; az = mapped[(size_t)ia * 3 + 2];
            la = lev[ka];
        }
        float best[DU_J];
#pragma unroll
        for (int j = 0; j < DU_J; ++j) best[j] = INFINITY;
        for (int t = 0; t < ntile; ++t) {
            if (ntile > 1 || a0 == 0) {           // a row that fits one tile is staged once
                __syncthreads();                  // the previous tile's reads are done
                for (int i = tid; i < min(DU_TILE, n - t * DU_TILE); i += DU_T) {
                    const int k = t * DU_TILE + i;
                    const int ib = min(max(mem[k], 0), N - 1);
                    sm[i] = make_float4(mapped[(size_t)ib * 3], mapped[(size_t)ib * 3 + 1], mapped[(size_t)ib * 3 + 2],
                                        __int_as_float(lev[k]));
                }
                __syncthreads();
            }
            const int cntb = min(DU_TILE, n - t * DU_TILE);
            const int self = ka - t * DU_TILE;    // this member's own place in the tile, if it is in it
            for (int i = 0; i < cntb; ++i) {
                const float4 b = sm[i];
                const float dx = ax - b.x, dy = ay - b.y, dz = az - b.z;
                const float d2 = i == self ? INFINITY : dx * dx + dy * dy + dz * dz;
                const int lb = __float_as_int(b.w);
#pragma unroll
                for (int j = 0; j < DU_J; ++j) best[j] = lb <= j ? fminf(best[j], d2) : best[j];
            }
        }
#pragma unroll
        for (int j = 0; j < DU_J; ++j)
            if (live && la <= j && j < J) {
                const double d = sqrt((double)best[j]) - expect[j];
                acc[j] += d * d / expect[j];
            }
    }
    // the threads' partial sums in a fixed tree, one disk at a time
    for (int j = 0; j < J; ++j) {
        double v = 0.0;
#pragma unroll
        for (int jj = 0; jj < DU_J; ++jj) v = jj == j ? acc[jj] : v;
        __syncthreads();
        red[tid] = v;
        __syncthreads();
        for (int w = DU_T / 2; w > 0; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        if (tid == 0) {
            const int c = nj[j];
            out_n[(size_t)s * J + j] = (double)c;
            out_dis[(size_t)s * J + j] = c >= 2 ? red[0] / (double)c : __builtin_nan("");   // one member has no neighbour
        }
    }
}

bool radii_ok(const double* radii, int J, R2* r2) {
    if (J <= 0 || J > DU_J) return false;
    for (int j = 0; j < J; ++j) {
        if (!(radii[j] > 0.0) || !(radii[j] < 1e18) || (j > 0 && radii[j] < radii[j - 1])) return false;
        if (r2) r2->v[j] = (float)(radii[j] * radii[j]);
    }
    if (r2)
        for (int j = J; j < DU_J; ++j) r2->v[j] = r2->v[J - 1];
    return true;
}

}  // namespace

extern "C" int pf_disk_tile() { return DU_TILE; }

extern "C" int pf_tri_closest_points(const float* pts, int P, const float* tris, int F, const int* face, float* out,
                                     void* stream) {
    if (!pts || !tris || !face || !out) return PF_ERR_NULL;
    if (P <= 0 || F <= 0 || P > (1 << 26) || F > (1 << 28)) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(closest_points_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, pts, P, tris, F, face,
                       out);
    return pf_last_launch_status();
}

extern "C" int pf_mesh_sample(const float* tris, int F, const double* cum_area, int S, unsigned long long seed, float* seeds,
                              int* face, float* uniforms, void* stream) {
    if (!tris || !cum_area || !seeds || !face || !uniforms) return PF_ERR_NULL;
    if (F <= 0 || S <= 0 || F > (1 << 28) || S > (1 << 24)) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(mesh_sample_kernel, dim3((S + 255) / 256), dim3(256), 0, (hipStream_t)stream, tris, F, cum_area, S,
                       (unsigned)seed, (unsigned)(seed >> 32), seeds, face, uniforms);
    return pf_last_launch_status();
}

extern "C" int pf_disk_count(const float* mapped, int N, const float* seeds, int S, const double* radii, int J, int* counts,
                             void* stream) {
    if (!mapped || !seeds || !radii || !counts) return PF_ERR_NULL;
    R2 r2;
    if (N <= 0 || S <= 0 || N > (1 << 26) || S > (1 << 24) || !radii_ok(radii, J, &r2)) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(disk_count_kernel<false>, dim3(S), dim3(DU_T), 0, (hipStream_t)stream, mapped, N, seeds, r2, J, counts,
                       PfReach{});
    return pf_last_launch_status();
}

extern "C" int pf_disk_count_reach(const float* mapped, int N, const float* seeds, int S, const double* radii, int J,
                                   const int* mapped_face, const long long* reach_offsets, const int* rface, const float* rb2,
                                   int* counts, void* stream) {
    if (!mapped || !seeds || !radii || !counts || !mapped_face || !reach_offsets || !rface || !rb2) return PF_ERR_NULL;
    R2 r2;
    if (N <= 0 || S <= 0 || N > (1 << 26) || S > (1 << 24) || !radii_ok(radii, J, &r2)) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(disk_count_kernel<true>, dim3(S), dim3(DU_T), 0, (hipStream_t)stream, mapped, N, seeds, r2, J, counts,
                       PfReach{mapped_face, reach_offsets, rface, rb2});
    return pf_last_launch_status();
}

extern "C" int pf_disk_fill(const float* mapped, int N, const float* seeds, int S, const double* radii, int J,
                            const long long* offsets, int* member, int* level, void* stream) {
    if (!mapped || !seeds || !radii || !offsets || !member || !level) return PF_ERR_NULL;
    R2 r2;
    if (N <= 0 || S <= 0 || N > (1 << 26) || S > (1 << 24) || !radii_ok(radii, J, &r2)) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(disk_fill_kernel<false>, dim3(S), dim3(DU_T), 0, (hipStream_t)stream, mapped, N, seeds, r2, J, offsets,
                       member, level, PfReach{});
    return pf_last_launch_status();
}

extern "C" int pf_disk_fill_reach(const float* mapped, int N, const float* seeds, int S, const double* radii, int J,
                                  const int* mapped_face, const long long* reach_offsets, const int* rface, const float* rb2,
                                  const long long* offsets, int* member, int* level, void* stream) {
    if (!mapped || !seeds || !radii || !offsets || !member || !level || !mapped_face || !reach_offsets || !rface || !rb2)
        return PF_ERR_NULL;
    R2 r2;
    if (N <= 0 || S <= 0 || N > (1 << 26) || S > (1 << 24) || !radii_ok(radii, J, &r2)) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(disk_fill_kernel<true>, dim3(S), dim3(DU_T), 0, (hipStream_t)stream, mapped, N, seeds, r2, J, offsets,
                       member, level, PfReach{mapped_face, reach_offsets, rface, rb2});
    return pf_last_launch_status();
}

extern "C" int pf_disk_uniformity(const float* mapped, int N, const long long* offsets, const int* member, const int* level,
                                  int S, const double* radii, int J, double* out_n, double* out_dis, void* stream) {
    if (!mapped || !offsets || !member || !level || !radii || !out_n || !out_dis) return PF_ERR_NULL;
    if (N <= 0 || S <= 0 || N > (1 << 26) || S > (1 << 24) || !radii_ok(radii, J, nullptr)) return PF_ERR_SHAPE;
    RD rd;
    for (int j = 0; j < DU_J; ++j) rd.v[j] = radii[j < J ? j : J - 1];
    hipLaunchKernelGGL(disk_uniformity_kernel, dim3(S), dim3(DU_T), 0, (hipStream_t)stream, mapped, N, offsets, member, level,
                       rd, J, out_n, out_dis);
    return pf_last_launch_status();
}
