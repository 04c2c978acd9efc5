// Column statistics of the fused training kernels (BatchNorm sums without a second launch) and the small device helpers the
// EdgeConv unit (train_ec_fwd.hip, train_fused.hip) and the BatchNorm MLPs (train_bnmlp.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "pf_api_internal.h"
#include "pf_mfma.h"

// ---- column statistics without a second launch: every workgroup adds its column sums to 64 double accumulators, the
// workgroup that arrives last turns them into the layer's constants and clears them for the next user.
//   mode 1 (BatchNorm forward): sums of y, y^2 -> scale, shift, mean, 1/std (aff rows 0..3), running statistics
//   mode 2 (BatchNorm backward): sums of dz, dz xhat -> their means (coef rows 0, 1), dbeta, dgamma
struct StatFin {
    double* acc;                      // [STAT_COPIES][2][STAT_W] + a counter word behind them; all zero between uses
    int mode, g, col0, ld;
    float* aff; const float* gamma; const float* beta; float* run_mean; float* run_var; float eps, momentum;
    float* coef; float* dgamma; float* dbeta;
    double R;
    double* defer;                    // SyncBN: non-null = the last workgroup does NOT finish the layer; it leaves the LOCAL sums in
                                      // defer[0 .. ncol) / defer[STAT_W ..] and the local row count in defer[2 STAT_W] (mode 2: dbeta /
                                      // dgamma are written from the local sums, as torch.nn.SyncBatchNorm does); the host all-reduces
                                      // the 2 STAT_W + 1 doubles over the ranks and stat_finalize_kernel finishes with the global sums
    int det;                          // PF_TRAIN_DETERMINISTIC: the accumulators hold 64-bit FIXED-POINT sums (two words per value:
                                      // quanta 2^-28 and 2^-60) added with integer atomics - exact, so independent of the order in
                                      // which the workgroups arrive; the default (double atomics) rounds in arrival order once a sum
                                      // needs more than 53 bits
};

// SyncBN on the fused kernels: after a launch whose StatFin defers (the local sums sit in fin.defer), the caller's callback
// all-reduces them over the ranks (stream-ordered, e.g. torch.distributed.all_reduce on the tensor behind the pointer) and
// one small launch (stat_finalize_kernel, train_fused.hip) finishes the layer with the global sums.
typedef int (*PfSyncFn)(void* user, double* sums, int n, void* stream);
PF_INTERNAL int pf_stat_sync(const StatFin& fin, int ncol, PfSyncFn cb, void* user, hipStream_t s);

namespace {

#ifndef PF_EC_GRID
#define PF_EC_GRID 512
#endif
constexpr int EC_GRID = PF_EC_GRID;   // persistent workgroups of the per-edge kernels (2 per CU)

__device__ __forceinline__ float lrelu1(float v, float s) { return fmaxf(v, v * s); }
__device__ __forceinline__ f4 lrelu4(f4 z, float s) {
    f4 r;
    r.x = fmaxf(z.x, z.x * s); r.y = fmaxf(z.y, z.y * s); r.z = fmaxf(z.z, z.z * s); r.w = fmaxf(z.w, z.w * s);
    return r;
}
__device__ __forceinline__ f4 mfma4(f4 a, f4 b, f4 c) {
    c = pf_mfma(a.x, b.x, c); c = pf_mfma(a.y, b.y, c); c = pf_mfma(a.z, b.z, c); c = pf_mfma(a.w, b.w, c);
    return c;
}
// B operand that makes mfma4(a, ident, c) add the A-layout tile `a` (lane (row, q) holds channels 4q..4q+3 of its row) to the
// accumulator-layout tile c: the matrix pipe as a transposer for per-row gathered addends
__device__ __forceinline__ f4 ident_b(int row, int q) {
    f4 r;
    r.x = 4 * q + 0 == row ? 1.f : 0.f; r.y = 4 * q + 1 == row ? 1.f : 0.f;
    r.z = 4 * q + 2 == row ? 1.f : 0.f; r.w = 4 * q + 3 == row ? 1.f : 0.f;
    return r;
}

constexpr int STAT_COPIES = 16;       // workgroups spread their atomics over this many accumulator sets (same-address atomics serialise)
constexpr int STAT_W = 128;           // statistics columns per launch (EdgeConv layers use <= 32, the BatchNorm MLPs up to 128)
constexpr int STAT_DOUBLES = STAT_COPIES * 2 * STAT_W + 1;
// deterministic accumulation (StatFin::det): a workgroup's float partial v split into two 64-bit integers, hi = v rounded to a
// multiple of 2^-28 (|sum| < 3.4e10) and lo = the remainder as a multiple of 2^-60 (|lo| <= 2^31 per partial) - the sum is
// exact to ~4e-19 per partial, whatever the size of the sum (one coarse quantum alone put an absolute error of up to 1.9e-9 on
// every partial: BatchNorm gradients of 1e-5 missed float64 by 3.3e-3 to 1.0e-2, tests/test_gpu_deterministic.py case (b)).
// The same 8-byte accumulator words, zero in either reading: copies [0, STAT_DET_COPIES) hold hi, the copies behind them lo.
#define PF_DET(p) (((p)->flags & PF_TRAIN_DETERMINISTIC) ? 1 : 0)
constexpr int STAT_DET_COPIES = STAT_COPIES / 2;
constexpr double STAT_FIX = 268435456.0, STAT_FIX_INV = 1.0 / 268435456.0;                 // 2^28
constexpr double STAT_FIX_LO = 4294967296.0, STAT_FIX_LO_INV = 1.0 / (268435456.0 * 4294967296.0);   // 2^32 more
__device__ __forceinline__ void stat_add(double* acc, float v, int det) {
    if (det) {
        const double s = (double)v * STAT_FIX;                          // exact (a float times a power of two)
        const long long hi = __double2ll_rn(s);
        const long long lo = __double2ll_rn((s - (double)hi) * STAT_FIX_LO);   // s - hi exact: |s - hi| <= 1/2, hi within 2x of s
        atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)hi);
        atomicAdd(reinterpret_cast<unsigned long long*>(acc + STAT_DET_COPIES * 2 * STAT_W), (unsigned long long)lo);
    } else
        unsafeAtomicAdd(acc, (double)v);
}
__device__ __forceinline__ double stat_load(const double* acc) { return PF_LD(acc); }
__device__ __forceinline__ long long stat_load_fix(const double* acc) {
    return (long long)PF_LD(reinterpret_cast<const unsigned long long*>(acc));
}
// det: one column's sum from its hi / lo words - integer sums first (exact, any order), then one fixed conversion
__device__ __forceinline__ double stat_load_det(const double* acc) {
    long long hi = 0, lo = 0;
    for (int k = 0; k < STAT_DET_COPIES; ++k) {
        hi += stat_load_fix(acc + k * 2 * STAT_W);
        lo += stat_load_fix(acc + (k + STAT_DET_COPIES) * 2 * STAT_W);
    }
    return (double)hi * STAT_FIX_INV + (double)lo * STAT_FIX_LO_INV;
}

// sums of one column -> the layer's constants.  R: rows the sums run over (the GLOBAL count under SyncBN); param_grads: mode 2
// also writes dbeta / dgamma from these sums (not under SyncBN: there they are the LOCAL sums, written by stat_flush)
__device__ __forceinline__ void stat_finish_col(const StatFin& f, int c, double a0, double a1, double R, bool param_grads) {
    if (f.mode == 1) {
        // a0, a1 are sums of (y - pivot), (y - pivot)^2 with pivot = the running mean the kernels started from (read here
        // before it is updated below; 0 without running statistics)
        const double pv = f.run_mean ? (double)f.run_mean[c] : 0.0;
        const double dm = a0 / R;
        const double mean = pv + dm;
        double var = a1 / R - dm * dm;
        if (var < 0.0) var = 0.0;
        const float rstd = 1.0f / sqrtf((float)var + f.eps);
        const float sc = f.gamma[c] * rstd;
        f.aff[f.col0 + c] = sc;
        f.aff[f.ld + f.col0 + c] = f.beta[c] - (float)mean * sc;
        f.aff[2 * f.ld + f.col0 + c] = (float)mean;
        f.aff[3 * f.ld + f.col0 + c] = rstd;
        if (f.run_mean) {
            f.run_mean[c] = (1.f - f.momentum) * f.run_mean[c] + f.momentum * (float)mean;
            f.run_var[c] = (1.f - f.momentum) * f.run_var[c] + f.momentum * (float)(var * (R / (R - 1.0)));
        }
    } else {
        f.coef[f.col0 + c] = (float)(a0 / R);
        f.coef[f.ld + f.col0 + c] = (float)(a1 / R);
        if (param_grads) { f.dbeta[c] = (float)a0; f.dgamma[c] = (float)a1; }
    }
}

// s0 / s1: this lane's sums for column (lane & 15) of each 16-column tile; `first`: the column that maps to statistics
// column 0; ncol <= STAT_W.  red: 4 * 2 * STAT_W floats of LDS.
template <int NT>
__device__ __forceinline__ void stat_flush(float (&s0)[NT], float (&s1)[NT], int first, int ncol, const StatFin& f, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        s0[nt] += __shfl_xor(s0[nt], 16); s0[nt] += __shfl_xor(s0[nt], 32);       // written out: through pf_xor_sum the 25 kernels that
        s1[nt] += __shfl_xor(s1[nt], 16); s1[nt] += __shfl_xor(s1[nt], 32);       // end in stat_flush compile to other instruction streams
    }
    if (lane < 16) {                                                  // red[wave][2][STAT_W]
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int c = nt * 16 + lane - first;
            if (c >= 0 && c < ncol) { red[wave * 2 * STAT_W + c] = s0[nt]; red[wave * 2 * STAT_W + STAT_W + c] = s1[nt]; }
        }
    }
    __syncthreads();
    if ((threadIdx.x & (STAT_W - 1)) < ncol) {                        // 256 threads = 2 x STAT_W sums
        const int t = threadIdx.x;
        const float v = (red[t] + red[2 * STAT_W + t]) + (red[4 * STAT_W + t] + red[6 * STAT_W + t]);
        if (f.det) stat_add(f.acc + (blockIdx.x % STAT_DET_COPIES) * 2 * STAT_W + t, v, 1);
        else stat_add(f.acc + (blockIdx.x % STAT_COPIES) * 2 * STAT_W + t, v, 0);
    }
    // order the accumulator atomics before the arrival count WITHOUT a release fence: a device-scope fence writes the whole
    // L2 back on this multi-die part (tens of microseconds per launch); the atomics themselves are performed at the coherent
    // level, so waiting for their acknowledgement is enough
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned* counter = reinterpret_cast<unsigned*>(f.acc + STAT_COPIES * 2 * STAT_W);
    if (threadIdx.x == 0) red[0] = atomicAdd(counter, 1u) == gridDim.x - 1 ? 1.f : 0.f;
    __syncthreads();
    if (red[0] == 0.f) return;
    const int c = threadIdx.x;
    if (c < ncol) {
        double a0 = 0.0, a1 = 0.0;
        if (f.det) {
            a0 = stat_load_det(f.acc + c);
            a1 = stat_load_det(f.acc + STAT_W + c);
            for (int k = 0; k < STAT_COPIES; ++k) { f.acc[k * 2 * STAT_W + c] = 0.0; f.acc[k * 2 * STAT_W + STAT_W + c] = 0.0; }
        } else
            for (int k = 0; k < STAT_COPIES; ++k) {
                a0 += stat_load(f.acc + k * 2 * STAT_W + c);
                a1 += stat_load(f.acc + k * 2 * STAT_W + STAT_W + c);
                f.acc[k * 2 * STAT_W + c] = 0.0; f.acc[k * 2 * STAT_W + STAT_W + c] = 0.0;
            }
        if (f.defer) {                                                // SyncBN: local sums out, the layer is finished after the all-reduce
            f.defer[c] = a0;
            f.defer[STAT_W + c] = a1;
            if (f.mode == 2) { f.dbeta[c] = (float)a0; f.dgamma[c] = (float)a1; }
        } else
            stat_finish_col(f, c, a0, a1, f.R, true);
    }
    if (threadIdx.x == 0) {
        if (f.defer) f.defer[2 * STAT_W] = f.R;
        *counter = 0u;
    }
}

}  // namespace
