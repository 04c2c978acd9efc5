// Training batches assembled and augmented on the device (include/puflow_hip.h: pf_patch_batch).  Replaces the host work of
// the reference's data path per batch (dataset/pu1k/fetcher.py:69-101, dataset/point_operation.py: nonuniform_sampling,
// jitter_perturbation_point_cloud, rotate_point_cloud_and_gt, random_scale_point_cloud_and_gt, shift_point_cloud_and_gt):
// one launch, one 1024-thread workgroup per patch, no grid barrier, no float atomics, no host synchronisation.
// The work is ~0.5 MB per batch: the launch is latency-bound, what it buys is the host work and the three copies it removes.
//
// Randomness is counter-based (Philox-4x32-10, pf_philox.h): every value is a pure function of (seed, global patch slot,
// stage, element), so a patch does not depend on the grid shape, on the rows a call produces or on the rank that produced them.
// Every fp32 operation that reaches an output is written as an explicit __f*_rn / fmaf call: -ffp-contract changes nothing.
#include <climits>
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"
#include "pf_philox.h"

namespace {

constexpr int PB_T = 1024;                       // threads per patch = candidates per round
constexpr int PB_ROUNDS = PF_PATCH_MAX_ROUNDS;
constexpr int PB_MAX_NIN = PF_PATCH_MAX_NIN;     // first-occurrence table (LDS)
constexpr int PB_MAX_N = PF_PATCH_MAX_N;         // selected indices (LDS)
constexpr unsigned PB_STREAM_PARAMS = 0, PB_STREAM_CAND = 1, PB_STREAM_JITTER = 2;
constexpr float PB_TWO_PI = 6.28318530717958647692f;

struct PbArgs {
    const float* inp; const float* gt; const float* radius; const int* order;
    int M, n_in, n_out, n, T, flags;
    long long pos;
    unsigned long long slot0, seed;
    float sigma, clip, scale_low, scale_high, shift_range;
    float* out_inp; float* out_gt; float* out_radius; float* params;
    int* idx; int* cand; int* status;
};

__device__ __forceinline__ U4 draw(const PbArgs& a, unsigned long long slot, unsigned stream, unsigned elem) {
    return philox(elem, stream, (unsigned)slot, (unsigned)(slot >> 32), (unsigned)a.seed, (unsigned)(a.seed >> 32));
}
// 2u - 1 of the same u, exact: an odd integer below 2^24 in magnitude times 2^-24 (a symmetric range has no cancellation then)
__device__ __forceinline__ float usym(unsigned x) {
    return __fmul_rn((float)((int)((x >> 8) << 1) + 1 - (1 << 24)), 0x1p-24f);
}
__device__ __forceinline__ float urange(float lo, float hi, float u) {
    return __fadd_rn(lo, __fmul_rn(__fsub_rn(hi, lo), u));
}
// Box-Muller on (x, y): which = 0 -> r cos(2 pi u1), 1 -> r sin(2 pi u1), r = sqrt(-2 ln u0); precise logf / sinf / cosf
__device__ __forceinline__ float normal(unsigned x, unsigned y, int which) {
    const float r = __fsqrt_rn(__fmul_rn(-2.f, logf(u01(x))));
    const float th = __fmul_rn(PB_TWO_PI, u01(y));
    return __fmul_rn(r, which ? sinf(th) : cosf(th));
}

// one point: [+ noise] -> row vector times R -> scale -> shift, a fixed operation order per coordinate
__device__ __forceinline__ void transform(float& x, float& y, float& z, const float* __restrict__ p, int flags) {
    if (flags & PF_PATCH_ROTATE) {
        const float rx = fmaf(z, p[6], fmaf(y, p[3], __fmul_rn(x, p[0])));
        const float ry = fmaf(z, p[7], fmaf(y, p[4], __fmul_rn(x, p[1])));
        const float rz = fmaf(z, p[8], fmaf(y, p[5], __fmul_rn(x, p[2])));
        x = rx; y = ry; z = rz;
    }
    if (flags & PF_PATCH_SCALE) { x = __fmul_rn(x, p[9]); y = __fmul_rn(y, p[9]); z = __fmul_rn(z, p[9]); }
    if (flags & PF_PATCH_SHIFT) { x = __fadd_rn(x, p[10]); y = __fadd_rn(y, p[11]); z = __fadd_rn(z, p[12]); }
}

__global__ __launch_bounds__(PB_T) void patch_batch_kernel(const PbArgs a) {
    __shared__ int first[PB_MAX_NIN];            // stream position of a value's first occurrence
    __shared__ int sel[PB_MAX_N];                // the first n distinct valid candidates, in stream order
    __shared__ int wsum[PB_T / 64];
    __shared__ float prm[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.x;
    const unsigned long long slot = a.slot0 + (unsigned long long)row;
    const int flags = a.flags;
    const bool sub = (flags & PF_PATCH_SUBSAMPLE) && a.n_in > a.n;

    int patch = a.order[(a.pos + row) % a.M];
    if ((unsigned)patch >= (unsigned)a.M) {      // a corrupt permutation must not become an out-of-bounds read
        if (tid == 0) atomicOr(a.status, PF_PATCH_ST_ORDER);
        patch = 0;
    }

    if (tid == 0) {                              // the patch's parameters, once
        const U4 q0 = draw(a, slot, PB_STREAM_PARAMS, 0), q1 = draw(a, slot, PB_STREAM_PARAMS, 1);
        float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
        if (flags & PF_PATCH_ROTATE) {
            const float ax = __fmul_rn(PB_TWO_PI, u01(q0.y)), ay = __fmul_rn(PB_TWO_PI, u01(q0.z)), az = __fmul_rn(PB_TWO_PI, u01(q0.w));
            const bool zo = flags & PF_PATCH_Z_ROTATED;
            const float cx = zo ? 1.f : cosf(ax), sx = zo ? 0.f : sinf(ax), cy = zo ? 1.f : cosf(ay), sy = zo ? 0.f : sinf(ay);
            const float cz = cosf(az), sz = sinf(az);
            const float czsy = __fmul_rn(cz, sy), szsy = __fmul_rn(sz, sy);
            R[0] = __fmul_rn(cz, cy); R[1] = __fsub_rn(__fmul_rn(czsy, sx), __fmul_rn(sz, cx)); R[2] = __fadd_rn(__fmul_rn(sz, sx), __fmul_rn(czsy, cx));
            R[3] = __fmul_rn(sz, cy); R[4] = __fadd_rn(__fmul_rn(cz, cx), __fmul_rn(szsy, sx)); R[5] = __fsub_rn(__fmul_rn(szsy, cx), __fmul_rn(cz, sx));
            R[6] = -sy;               R[7] = __fmul_rn(cy, sx);                                R[8] = __fmul_rn(cy, cx);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) prm[k] = R[k];
        prm[9] = (flags & PF_PATCH_SCALE) ? urange(a.scale_low, a.scale_high, u01(q1.x)) : 1.f;
        const bool sh = flags & PF_PATCH_SHIFT;
        prm[10] = sh ? __fmul_rn(a.shift_range, usym(q1.y)) : 0.f;
        prm[11] = sh ? __fmul_rn(a.shift_range, usym(q1.z)) : 0.f;
        prm[12] = sh ? __fmul_rn(a.shift_range, usym(q1.w)) : 0.f;
        prm[13] = sub ? urange(0.1f, 0.9f, u01(q0.x)) : 0.f;
        prm[14] = 0.f; prm[15] = 0.f;
    }
    if (sub)
        for (int i = tid; i < a.n_in; i += PB_T) first[i] = INT_MAX;
    __syncthreads();

    if (sub) {
        // The reference's rejection loop keeps the first n DISTINCT in-range candidates in stream order.  In parallel: a round
        // of 1024 candidates records every value's first stream position (integer LDS min), a candidate is kept when it IS that
        // first occurrence, and a prefix sum over stream positions (wave ballots + 16 wave totals) gives its rank.
        const float loc = prm[13], fn = (float)a.n_in;
        int base = 0, r = 0;                      // uniform over the workgroup
        for (; r < PB_ROUNDS && base < a.n; ++r) {
            const int p = r * PB_T + tid;
            const U4 q = draw(a, slot, PB_STREAM_CAND, (unsigned)(p >> 2));
            const float z = (p & 2) ? normal(q.z, q.w, p & 1) : normal(q.x, q.y, p & 1);
            const int c = (int)__fmul_rn(__fadd_rn(loc, __fmul_rn(0.3f, z)), fn);      // truncation, like int() / astype(int64)
            const bool valid = c >= 0 && c < a.n_in;
            if (a.cand && p < a.T) a.cand[(size_t)row * a.T + p] = c;
            if (valid) atomicMin(&first[c], p);
            __syncthreads();
            const bool isf = valid && first[c] == p;
            const unsigned long long m = __ballot(isf);
            if (lane == 0) wsum[wave] = __popcll(m);
            __syncthreads();
            int off = 0, tot = 0;
#pragma unroll
            for (int w = 0; w < PB_T / 64; ++w) { const int v = wsum[w]; off += w < wave ? v : 0; tot += v; }
            const int rank = base + off + __popcll(m & ((1ull << lane) - 1ull));
            if (isf && rank < a.n) sel[rank] = c;
            base += tot;
            __syncthreads();
        }
        if (base < a.n) {                         // still short after the last round: sticky status, pad with the last index
            if (tid == 0) atomicOr(a.status, PF_PATCH_ST_SHORT);
            const int last = base > 0 ? sel[base - 1] : 0;
            for (int i = base + tid; i < a.n; i += PB_T) sel[i] = last;
            __syncthreads();
        }
        if (tid == 0) prm[14] = (float)r;
    }
    __syncthreads();
    if (tid < 16) a.params[(size_t)row * 16 + tid] = prm[tid];
    if (tid == 0) {
        const float rad = a.radius[patch];
        a.out_radius[row] = (flags & PF_PATCH_SCALE) ? __fmul_rn(rad, prm[9]) : rad;
    }

    const float* __restrict__ src = a.inp + (size_t)patch * a.n_in * 3;
    float* __restrict__ dst = a.out_inp + (size_t)row * a.n * 3;
    for (int i = tid; i < a.n; i += PB_T) {
        const int s = sub ? sel[i] : i;
        if (a.idx) a.idx[(size_t)row * a.n + i] = s;
        float x = src[s * 3 + 0], y = src[s * 3 + 1], z = src[s * 3 + 2];
        if (flags & PF_PATCH_JITTER) {
            const U4 q = draw(a, slot, PB_STREAM_JITTER, (unsigned)i);
            const float r = __fsqrt_rn(__fmul_rn(-2.f, logf(u01(q.x))));
            const float th = __fmul_rn(PB_TWO_PI, u01(q.y));
            const float z0 = __fmul_rn(r, cosf(th)), z1 = __fmul_rn(r, sinf(th)), z2 = normal(q.z, q.w, 0);
            x = __fadd_rn(x, fminf(fmaxf(__fmul_rn(a.sigma, z0), -a.clip), a.clip));
            y = __fadd_rn(y, fminf(fmaxf(__fmul_rn(a.sigma, z1), -a.clip), a.clip));
            z = __fadd_rn(z, fminf(fmaxf(__fmul_rn(a.sigma, z2), -a.clip), a.clip));
        }
        transform(x, y, z, prm, flags);
        dst[i * 3 + 0] = x; dst[i * 3 + 1] = y; dst[i * 3 + 2] = z;
    }
    const float* __restrict__ gsrc = a.gt + (size_t)patch * a.n_out * 3;
    float* __restrict__ gdst = a.out_gt + (size_t)row * a.n_out * 3;
    for (int i = tid; i < a.n_out; i += PB_T) {
        float x = gsrc[i * 3 + 0], y = gsrc[i * 3 + 1], z = gsrc[i * 3 + 2];
        transform(x, y, z, prm, flags);
        gdst[i * 3 + 0] = x; gdst[i * 3 + 1] = y; gdst[i * 3 + 2] = z;
    }
}

}  // namespace

extern "C" int pf_patch_batch(const float* inp, const float* gt, const float* radius, const int* order, int M, int n_in,
                              int n_out, long long pos, int b, int n, unsigned long long slot0, unsigned long long seed,
                              int flags, float jitter_sigma, float jitter_clip, float scale_low, float scale_high,
                              float shift_range, float* out_inp, float* out_gt, float* out_radius, float* params, int* idx,
                              int* cand, int T, int* status, void* stream) {
    if (!inp || !gt || !radius || !order || !out_inp || !out_gt || !out_radius || !params || !status) return PF_ERR_NULL;
    if (M <= 0 || n_in <= 0 || n_out <= 0 || b <= 0 || n <= 0 || n > n_in || pos < 0) return PF_ERR_SHAPE;
    if ((long long)n_in * 3 > 0x7fffffffll || (long long)n_out * 3 > 0x7fffffffll) return PF_ERR_SHAPE;
    if (n_in > n && !(flags & PF_PATCH_SUBSAMPLE)) return PF_ERR_SHAPE;          // nothing else chooses n of n_in points
    if (cand && T <= 0) return PF_ERR_SHAPE;
    if (!(jitter_sigma >= 0.f) || !(jitter_clip >= 0.f) || !(scale_low <= scale_high) || !(shift_range >= 0.f)) return PF_ERR_SHAPE;
    if (flags & ~PF_PATCH_ALL) return PF_ERR_UNSUPPORTED;
    if (n_in > n && (n_in > PB_MAX_NIN || n > PB_MAX_N)) return PF_ERR_UNSUPPORTED;
    if (shift_range == 0.f) flags &= ~PF_PATCH_SHIFT;
    PbArgs a;
    a.inp = inp; a.gt = gt; a.radius = radius; a.order = order;
    a.M = M; a.n_in = n_in; a.n_out = n_out; a.n = n; a.T = cand ? T : 0; a.flags = flags;
    a.pos = pos % M; a.slot0 = slot0; a.seed = seed;
    a.sigma = jitter_sigma; a.clip = jitter_clip; a.scale_low = scale_low; a.scale_high = scale_high; a.shift_range = shift_range;
    a.out_inp = out_inp; a.out_gt = out_gt; a.out_radius = out_radius; a.params = params;
    a.idx = idx; a.cand = cand; a.status = status;
    hipLaunchKernelGGL(patch_batch_kernel, dim3(b), dim3(PB_T), 0, (hipStream_t)stream, a);
    return pf_last_launch_status();
}
