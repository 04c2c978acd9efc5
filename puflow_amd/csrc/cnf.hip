// Continuous (CNF) variant of the flow blocks: the ODE right-hand side and the Runge-Kutta
// bookkeeping of an adaptive Dormand-Prince solver.  Replaces ODEfunc.forward + ODEnet + ConcatSquashLinear
// (modules/continuous/odefunc.py:60-148, diffeq_layers.py:72-86) and the arithmetic of torchdiffeq's dopri5
// stages (called from modules/continuous/cnf.py:97-113).  The step-size CONTROL (a handful of scalars per step)
// runs on the device, for inference (cnf_ctl_update below) and for flow_block's tape (cnf_ctl_update_taped); on the host
// only under flow_block's controller="host" reference path (puflow_amd/cnf.py).
//
// State rows are [y0 y1 y2 logp]; one MFMA column tile = 16 rows.  A ConcatSquash layer is
//     out = (W x + b) * sigmoid(Wg [t; c] + bg) + Wb [t; c]
// and everything that depends on the context c only is precomputed per ORIGINAL point by a GEMM
// (ctx = Hc c + hb, 288 floats per point and block), so a right-hand-side evaluation is
//     3 -> 64 (VALU) -> tanh -> 64 -> 64 (split-fp16 MFMA) -> tanh -> 64 -> 3 (MFMA)
// plus the Hutchinson term  e^T (d f / d y) e  that the reference obtains with autograd (odefunc.py:9-31):
// here the vector-Jacobian product is written out (W3^T, tanh', W2^T as a second MFMA image, tanh', W1^T).
//
// The layouts of the weight record and of the context row: csrc/pf_cnf.h.
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"
#include "pf_mfma.h"
#include "pf_wave.h"
#include "pf_cnf.h"
#include "pf_cnf_eval.h"

namespace {

#ifndef PF_CNF_SPLIT_FWD
#define PF_CNF_SPLIT_FWD 1           // 0: A/B builds with the factored gates in the inverse pass only
#endif
#ifndef PF_CNF_NW
#define PF_CNF_NW 4
#endif
#ifndef PF_CNF_WPE
#define PF_CNF_WPE 2                      // waves per SIMD the step kernels are compiled for (register budget 512 / WPE)
#endif
constexpr int CNF_NW = PF_CNF_NW;         // waves per workgroup

constexpr int CTL_T = 0, CTL_DT = 1, CTL_T1 = 2, CTL_NTOT = 3, CTL_CUR = 4, CTL_DONE = 5, CTL_ACC = 6, CTL_REJ = 7, CTL_NFE = 8,
              CTL_STATUS = 9, CTL_REV = 10, CTL_H0 = 11, CTL_D1 = 12,    // device-side dopri5 state, see cnf_ctl_update
              CTL_ARRIVE = 13;                                           // (as a 32-bit word) workgroups of the running attempt that are done

struct CnfArgs {
    const float* y0;        // [rows,4] state at the start of the step
    const float* k;         // [7][rows][4] stage derivatives
    float coef[6];          // yi = y0 + h * sum_j coef[j] k[j], j < ncoef
    int ncoef;
    float h;
    float t;                // time the net sees
    float sgn;              // -1: reversed integration (returns -f)
    const float* ctx;       // [T, 288]
    const float* e;         // [T, 3]
    const float* rec;       // CNF_REC floats
    float* kout;            // [rows,4]
    float* yout;            // nullable: the stage state yi (the last stage's is the step's solution)
    int rows, R, ntiles;
    const double* ctl;      // nullable: take h = ctl[CTL_H0] and t = +-(ctl[CTL_T] + h) from the device (initial-step probe)
};

__global__ __launch_bounds__(CNF_NW * 64) void cnf_rhs_kernel(CnfArgs a) {
    __shared__ f4 wl[CNF_REC / 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4;
    const CnfW w = cnf_stage_weights(wl, a.rec, CNF_NW * 64, lane);
    const size_t kstride = (size_t)a.rows * 4;
    float h = a.h, t = a.t;
    if (a.ctl) {
        const double hd = a.ctl[CTL_H0], td = a.ctl[CTL_T] + hd;
        h = (float)hd;
        t = (float)(a.ctl[CTL_REV] != 0.0 ? -td : td);
    }
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const auto [row, pt, ok] = cnf_tile_row(tile, CNF_NW, wave, col, a.rows, a.R);
        f4 y = *reinterpret_cast<const f4*>(a.y0 + (size_t)row * 4);
        for (int j = 0; j < a.ncoef; ++j) {
            const f4 kj = *reinterpret_cast<const f4*>(a.k + j * kstride + (size_t)row * 4);
            y += kj * (h * a.coef[j]);
        }
        if (a.yout && ok && q == 0) *reinterpret_cast<f4*>(a.yout + (size_t)row * 4) = y;
        const float* cx = a.ctx + (size_t)pt * CNF_CTX;
        const f4 k = cnf_eval(w, q, y, t, a.sgn, cx, a.e[(size_t)pt * 3 + 0], a.e[(size_t)pt * 3 + 1],
                              a.e[(size_t)pt * 3 + 2]);
        if (ok && q == 0) *reinterpret_cast<f4*>(a.kout + (size_t)row * 4) = k;
    }
}

// ---- one whole Dormand-Prince step per launch: the six stage evaluations run back to back on register-held stage
// derivatives (the context rows are re-read from L1/L2, not HBM); outputs the step's solution, its FSAL derivative,
// optionally the dense-output mid-point, and this workgroup's share of the scaled error sum.
struct CnfStepArgs {
    const float* y0;        // [rows,4]
    const float* f0;        // [rows,4]  derivative at the start (FSAL)
    const float* ctx;
    const float* e;
    const float* rec;
    float* y1;              // [rows,4]
    float* f1;              // [rows,4]
    float* ymid;            // nullable
    double* partial;        // [gridDim.x]
    float t, h, sgn, tsign; // net time of stage s: tsign * (t + alpha_s h)
    float rtol, atol;
    int rows, R, ntiles;
};

__global__ __launch_bounds__(CNF_NW * 64) void cnf_step_kernel(CnfStepArgs a) {
    __shared__ f4 wl[CNF_REC / 4];
    __shared__ double red[CNF_NW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4;
    const CnfW w = cnf_stage_weights(wl, a.rec, CNF_NW * 64, lane);
    double acc = 0.0;
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const auto [row, pt, ok] = cnf_tile_row(tile, CNF_NW, wave, col, a.rows, a.R);
        const f4 y0 = *reinterpret_cast<const f4*>(a.y0 + (size_t)row * 4);
        const float* cx = a.ctx + (size_t)pt * CNF_CTX;
        const float e0 = a.e[(size_t)pt * 3 + 0], e1 = a.e[(size_t)pt * 3 + 1], e2 = a.e[(size_t)pt * 3 + 2];
        f4 k[7];
        k[0] = *reinterpret_cast<const f4*>(a.f0 + (size_t)row * 4);
        f4 yi = y0;
        const f4 err = cnf_dopri_stages<false, false, 0>(w, q, y0, k, yi, a.t, a.h, a.sgn, a.tsign, cx, e0, e1, e2, nullptr, cx);
        if (ok && q == 0) {
            *reinterpret_cast<f4*>(a.y1 + (size_t)row * 4) = yi;
            *reinterpret_cast<f4*>(a.f1 + (size_t)row * 4) = k[6];
            if (a.ymid) {
                *reinterpret_cast<f4*>(a.ymid + (size_t)row * 4) = y0 + cnf_comb7(k, CNF_CM) * a.h;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float r = err[c] / (a.atol + a.rtol * fmaxf(fabsf(y0[c]), fabsf(yi[c])));
                acc += (double)r * (double)r;
            }
        }
    }
    acc = pf_wave_sum(acc);                                          // workgroup sum in a fixed order: lanes -> wave -> workgroup
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < CNF_NW; ++i) t += red[i];
        a.partial[blockIdx.x] = t;
    }
}

// ---- adaptive step control on the device ------------------------------------------------------------
// The host-side dopri5 loop read the error norm after every step attempt (one device->host sync per attempt, ~60 per
// forward).  Here the controller state lives in device memory and a one-thread kernel takes torchdiffeq's decisions
// (accept / reject, next step size, end-time coverage: the same formulas as oracle/cnf_ref.py::dopri5 and the host loop in
// puflow_amd/cnf.py); the step kernel reads (t, dt, which buffer is current) from that state and is a no-op once the
// integration is done, so the host can enqueue a batch of attempts and look at the state once per batch.
//   ctl (doubles): [0] t  [1] dt  [2] t1  [3] n_tot  [4] cur (0/1)  [5] done  [6] accepted  [7] rejected  [8] nfe
//                  [9] status (0 ok, 1 non-finite error norm, 2 dt underflow, 3 tape full: taped variant only)  [10] reverse (0/1)
// The step that covers t1 writes the dense-output value at t1 (quartic through y0, y_mid, y1: torchdiffeq's interpolation)
// straight into `out`; if that attempt is rejected a later covering attempt overwrites it.

// The per-workgroup sums (<= 1024) added in a fixed order by a WHOLE workgroup: four independent loads per thread in flight at
// once, then wave shuffles and four LDS words.  (One wave walking the array in a dependent loop was 16 L2 round trips in a
// row: ~10 us at the tail of every step attempt, ~100 attempts per forward.)  Every thread returns the total.
__device__ __forceinline__ double cnf_partial_total(const double* partial, int nblocks, double* red4) {
    double v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = threadIdx.x + j * CNF_NW * 64;
        v[j] = i < nblocks ? PF_LD(partial + i) : 0.0;
    }
    static_assert(CNF_NW * 64 * 4 >= 1024, "a workgroup covers the largest grid in four loads per thread");
    double sum = ((v[0] + v[1]) + v[2]) + v[3];
    sum = pf_wave_sum(sum);
    __syncthreads();                                                         // red4 may still be read from an earlier total
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = sum;
    __syncthreads();
    double t = red4[0];
#pragma unroll
    for (int w = 1; w < CNF_NW; ++w) t += red4[w];
    return t;
}

// torchdiffeq's `_adaptive_step` decisions on the error norm of the attempt just made (thread 0 decides).  Called by the whole
// workgroup of cnf_step_dev_kernel that finishes LAST (every partial sum is in place by then).
__device__ __forceinline__ void cnf_ctl_update(double* ctl, const double* partial, int nblocks, double* red4) {
    const double sum = cnf_partial_total(partial, nblocks, red4);
    if (threadIdx.x != 0) return;
    const double ratio = sqrt(sum / ctl[CTL_NTOT]);
    const double t = ctl[CTL_T], dt = ctl[CTL_DT], t1 = ctl[CTL_T1];
    ctl[CTL_NFE] += 6.0;
    if (!(ratio == ratio) || ratio > 1.7e308) { ctl[CTL_STATUS] = 1.0; ctl[CTL_DONE] = 1.0; return; }
    if (!(t + dt > t)) { ctl[CTL_STATUS] = 2.0; ctl[CTL_DONE] = 1.0; return; }
    double tn = t;
    if (ratio <= 1.0) {
        ctl[CTL_ACC] += 1.0;
        tn = t + dt;
        ctl[CTL_T] = tn;
        ctl[CTL_CUR] = 1.0 - ctl[CTL_CUR];                       // accepted state; FSAL: f1 becomes the next f0
    } else {
        ctl[CTL_REJ] += 1.0;
    }
    double ndt;
    if (ratio == 0.0) ndt = dt * 10.0;
    else {
        const double dfac = ratio < 1.0 ? 1.0 : 0.2;
        double fac = 0.9 / pow(ratio, 1.0 / 5.0);
        fac = fac > dfac ? fac : dfac;
        fac = fac < 10.0 ? fac : 10.0;
        ndt = dt * fac;
    }
    ctl[CTL_DT] = ndt;
    if (!(t1 > tn)) ctl[CTL_DONE] = 1.0;
}

// The step size a taped attempt takes from the controller state: the step that would cover t1 is cut to end there.
__device__ __forceinline__ float cnf_taped_h(const double* ctl, bool& cover) {
    cover = ctl[CTL_T1] <= ctl[CTL_T] + ctl[CTL_DT];
    return (float)(cover ? ctl[CTL_T1] - ctl[CTL_T] : ctl[CTL_DT]);
}

// The same decisions for the TAPED integration (pf_cnf_steps_taped; puflow_amd/cnf.py tape_forward's rule): the covering step is
// cut, not interpolated, an accepted step is recorded as the fp32 pair (s, h) the kernel computed with, and the time advances in
// that fp32 arithmetic, s' = s + h, so that the recorded list is contiguous bit for bit; the last step lands on t1 itself.
// Status 3: the tape is full (cap steps recorded, t1 not reached).
__device__ __forceinline__ void cnf_ctl_update_taped(double* ctl, const double* partial, int nblocks, double* red4, float* steps, int cap) {
    const double sum = cnf_partial_total(partial, nblocks, red4);
    if (threadIdx.x != 0) return;
    const double ratio = sqrt(sum / ctl[CTL_NTOT]);
    const double t = ctl[CTL_T], t1 = ctl[CTL_T1];
    bool cover;
    const float hf = cnf_taped_h(ctl, cover);
    const float sf = (float)t;
    const double tn = cover ? t1 : (double)(sf + hf);
    ctl[CTL_NFE] += 6.0;
    if (!(ratio == ratio) || ratio > 1.7e308) { ctl[CTL_STATUS] = 1.0; ctl[CTL_DONE] = 1.0; return; }
    if (!(tn > t)) { ctl[CTL_STATUS] = 2.0; ctl[CTL_DONE] = 1.0; return; }
    if (ratio <= 1.0) {
        const int acc = (int)ctl[CTL_ACC];
        steps[2 * acc] = sf; steps[2 * acc + 1] = hf;
        ctl[CTL_ACC] = (double)(acc + 1);
        ctl[CTL_T] = tn;
        ctl[CTL_CUR] = 1.0 - ctl[CTL_CUR];                       // FSAL: f1 becomes the next f0 (the states go to the tape)
        if (cover) ctl[CTL_DONE] = 1.0;
        else if (acc + 1 >= cap) { ctl[CTL_STATUS] = 3.0; ctl[CTL_DONE] = 1.0; }
    } else {
        ctl[CTL_REJ] += 1.0;
    }
    const double h = (double)hf;
    double ndt;
    if (ratio == 0.0) ndt = h * 10.0;
    else {
        const double dfac = ratio < 1.0 ? 1.0 : 0.2;
        double fac = 0.9 / pow(ratio, 1.0 / 5.0);
        fac = fac > dfac ? fac : dfac;
        fac = fac < 10.0 ? fac : 10.0;
        ndt = h * fac;
    }
    ctl[CTL_DT] = ndt;
}

struct CnfDevArgs {
    double* ctl;
    float* yb[2];
    float* fb[2];
    const float* ctx; const float* e; const float* rec;
    float* out;              // [rows,4] dense output at t1
    double* partial;
    float rtol, atol;
    int rows, R, ntiles;
    float* states;           // TAPED: [cap + 1][rows][4], the state at the start of accepted step k in states[k]
    float* steps;            // TAPED: [cap][2] (s, h) of the accepted steps
    int cap;
};

// CTX_LDS (inverse direction, R >= 4 rows per original point): the context rows of the workgroup's 64 / R points are copied
// to LDS once per tile and all six stage evaluations read them there - each evaluation re-read 1 152 B per row from L2 before
// SPLIT (the caller's PF_CNF_SPLIT_GATES): see cnf_eval.  Without CTX_LDS (the forward pass, R = 1: 64 points per tile) only the
// 144 gate columns of a point go to LDS, in the compact layout (cnf_eval<.., COMPACT>); the bias columns stay in global memory.
// TAPED (pf_cnf_steps_taped, the forward a backward sweep replays): the states do not ping-pong, attempt number acc reads
// states[acc] and writes states[acc + 1] (acc = accepted steps so far; a rejected attempt's result is overwritten by the next),
// the covering step is cut to end at t1 and no dense output is written - the result is states[accepted].
template <bool CTX_LDS, bool SPLIT, bool TAPED = false>
__global__ __launch_bounds__(CNF_NW * 64, PF_CNF_WPE) void cnf_step_dev_kernel(CnfDevArgs a) {
    constexpr bool COMPACT = SPLIT && !CTX_LDS;
    constexpr int TW = COMPACT ? CNF_GATES : CNF_CTX;               // width of a stage's row of the factor table
    __shared__ f4 wl[CNF_REC / 4];
    __shared__ double red[CNF_NW];
    __shared__ f4 sctx[CTX_LDS ? CNF_NW * 4 * CNF_CTX / 4 : (COMPACT ? CNF_NW * 16 * CNF_GATES / 4 : 1)];
    __shared__ float stf[SPLIT ? 6 * TW : 1];                        // [stage][column]: 2^(gt tsign alpha_s h) of the gate columns
    if (a.ctl[CTL_DONE] != 0.0) return;                              // uniform over the grid
    const int cur = (int)a.ctl[CTL_CUR];
    const float t = (float)a.ctl[CTL_T];
    float h = (float)a.ctl[CTL_DT];
    const bool reverse = a.ctl[CTL_REV] != 0.0;
    const float sgn = reverse ? -1.f : 1.f, tsign = sgn;
    bool cover = a.ctl[CTL_T1] <= a.ctl[CTL_T] + a.ctl[CTL_DT];
    if constexpr (TAPED) h = cnf_taped_h(a.ctl, cover);
    float wd[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (!TAPED && cover) {                                                     // weights of (y0, y1, y_mid, dt f0, dt f1) at x = (t1 - t) / dt
        const double x = (a.ctl[CTL_T1] - a.ctl[CTL_T]) / a.ctl[CTL_DT], x2 = x * x, x3 = x2 * x, x4 = x2 * x2, dt = a.ctl[CTL_DT];
        wd[0] = (float)(-8 * x4 + 18 * x3 - 11 * x2 + 1); wd[1] = (float)(-8 * x4 + 14 * x3 - 5 * x2);
        wd[2] = (float)(16 * x4 - 32 * x3 + 16 * x2);
        wd[3] = (float)(dt * (-2 * x4 + 5 * x3 - 4 * x2 + x)); wd[4] = (float)(dt * (2 * x4 - 3 * x3 + x2));
    }
    const float* y0p = a.yb[cur];
    const float* f0p = a.fb[cur];
    float* y1p = a.yb[1 - cur];
    float* f1p = a.fb[1 - cur];
    if constexpr (TAPED) {
        const int acc = (int)a.ctl[CTL_ACC];
        if (acc >= a.cap) return;                                    // (the controller sets `done` before this can happen)
        y0p = a.states + (size_t)acc * a.rows * 4;
        y1p = a.states + (size_t)(acc + 1) * a.rows * 4;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4;
    const CnfW w = cnf_stage_weights(wl, a.rec, CNF_NW * 64, lane);
    if (SPLIT) {
        const float* tv = w.rec + CNF_TV;
        for (int i = threadIdx.x; i < 6 * TW; i += CNF_NW * 64) {
            const int s = i / TW, r = COMPACT ? cnf_gate_col(i % TW) : i % TW;
            stf[i] = cnf_gate_row(r) ? __builtin_amdgcn_exp2f(tv[r] * (tsign * CNF_AL[s] * h)) : 0.f;
        }                                                             // (visible after the tile loop's barriers)
    }
    double acc = 0.0;
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const auto [row, pt, ok] = cnf_tile_row(tile, CNF_NW, wave, col, a.rows, a.R);
        const f4 y0 = *reinterpret_cast<const f4*>(y0p + (size_t)row * 4);
        const float* cx = a.ctx + (size_t)pt * CNF_CTX;
        const float* cxb = cx;
        if (COMPACT) {
            // the gate columns of the tile's points (rows [64 tile, 64 tile + 63] -> points first .. last) as 2^(gt tsign t + gc)
            const long long npts = ((long long)a.rows + a.R - 1) / a.R;
            const long long r0 = (long long)tile * CNF_NW * 16;
            const long long p0 = r0 / a.R;
            long long pe = (r0 + CNF_NW * 16 - 1) / a.R;
            pe = pe < npts ? pe : npts - 1;
            const int np = (int)(pe - p0 + 1);                     // <= 64
            __syncthreads();                                       // every wave is done with the previous tile's columns
            const float tt = tsign * t;
            for (int i = threadIdx.x; i < np * (CNF_GATES / 4); i += CNF_NW * 64) {
                const int pp = i / (CNF_GATES / 4), c4 = (i % (CNF_GATES / 4)) * 4;
                const int r = cnf_gate_col(c4);
                const f4 v = *reinterpret_cast<const f4*>(a.ctx + (size_t)(p0 + pp) * CNF_CTX + r);
                const f4 g4 = *reinterpret_cast<const f4*>(w.rec + CNF_TV + r);
                f4 o;
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = __builtin_amdgcn_exp2f(fmaf(g4[k], tt, v[k]));
                sctx[i] = o;
            }
            __syncthreads();
            const long long pl = pt - p0;
            cx = reinterpret_cast<const float*>(sctx) + (size_t)(pl < 0 ? 0 : (pl >= np ? np - 1 : pl)) * CNF_GATES;
        }
        if (CTX_LDS) {
            const int ppw = CNF_NW * 16 / a.R;                     // points of this workgroup's tile (<= 16)
            const long long p0 = (long long)tile * ppw;
            const long long npts = ((long long)a.rows + a.R - 1) / a.R;
            __syncthreads();                                       // every wave is done with the previous tile's rows
            for (int i = threadIdx.x; i < ppw * (CNF_CTX / 4); i += CNF_NW * 64) {
                const long long pp = p0 + i / (CNF_CTX / 4);
                f4 v = reinterpret_cast<const f4*>(a.ctx)[(pp < npts ? pp : npts - 1) * (CNF_CTX / 4) + i % (CNF_CTX / 4)];
                if (SPLIT && cnf_gate_row(4 * (i % (CNF_CTX / 4)))) {  // the gate rows become 2^(gt tsign t + gc), once per point
                    const f4 g4 = *reinterpret_cast<const f4*>(w.rec + CNF_TV + 4 * (i % (CNF_CTX / 4)));
                    const float tt = tsign * t;
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = __builtin_amdgcn_exp2f(fmaf(g4[r], tt, v[r]));
                }
                sctx[i] = v;
            }
            __syncthreads();
            const long long pl = pt - p0;                            // a clamped out-of-range lane may point past the tile
            cx = reinterpret_cast<const float*>(sctx) + (size_t)(pl < 0 ? 0 : (pl >= ppw ? ppw - 1 : pl)) * CNF_CTX;
        }
        const float e0 = a.e[(size_t)pt * 3 + 0], e1 = a.e[(size_t)pt * 3 + 1], e2 = a.e[(size_t)pt * 3 + 2];
        f4 k[7];
        k[0] = *reinterpret_cast<const f4*>(f0p + (size_t)row * 4);
        f4 yi = y0;
        const f4 err = cnf_dopri_stages<SPLIT, COMPACT, SPLIT ? TW : 0>(w, q, y0, k, yi, t, h, sgn, tsign, cx, e0, e1, e2, stf, cxb);
        if (ok && q == 0) {
            *reinterpret_cast<f4*>(y1p + (size_t)row * 4) = yi;
            *reinterpret_cast<f4*>(f1p + (size_t)row * 4) = k[6];
            if (!TAPED && cover) {
                const f4 ymid = y0 + cnf_comb7(k, CNF_CM) * h;
                // the same term order as the host path's pf_lincomb: ((((w0 y0) + w1 y1) + w2 ymid) + w3 f0) + w4 f1, fused
                f4 o;
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    o[c] = fmaf(wd[4], k[6][c], fmaf(wd[3], k[0][c], fmaf(wd[2], ymid[c], fmaf(wd[1], yi[c], fmaf(wd[0], y0[c], 0.f)))));
                *reinterpret_cast<f4*>(a.out + (size_t)row * 4) = o;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float r = err[c] / (a.atol + a.rtol * fmaxf(fabsf(y0[c]), fabsf(yi[c])));
                acc += (double)r * (double)r;
            }
        }
    }
    acc = pf_wave_sum(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    // ---- this workgroup's share of the error sum; the workgroup that finishes LAST takes the controller's decision (it was a
    // one-wave launch of its own behind every attempt: ~100 launches of 5 - 7 us per forward).  Every workgroup has read the
    // controller state at its start, before the last one can have arrived here.
    __shared__ int last;
    if (threadIdx.x == 0) {
        double tt = 0.0;
        for (int i = 0; i < CNF_NW; ++i) tt += red[i];
        PF_ST(a.partial + blockIdx.x, tt);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned* counter = reinterpret_cast<unsigned*>(a.ctl + CTL_ARRIVE);
        last = atomicAdd(counter, 1u) == gridDim.x - 1 ? 1 : 0;
        if (last) *counter = 0u;
    }
    __syncthreads();
    if (last) {                                                                          // `last` is uniform over the workgroup
        if constexpr (TAPED) cnf_ctl_update_taped(a.ctl, a.partial, (int)gridDim.x, red, a.steps, a.cap);
        else cnf_ctl_update(a.ctl, a.partial, (int)gridDim.x, red);
    }
}

// torchdiffeq's `_select_initial_step` (oracle/cnf_ref.py::dopri5, first lines) around the probe evaluation
// f(t0 + h0, y0 + h0 f0): d0 = rms(y0 / scale), d1 = rms(f0 / scale), d2 = rms((f1 - f0) / scale) / h0.
// The same start in TWO launches (it was 13: reset, f0, two norms of two launches each, init_a, the probe, its norm, init_b -
// ~5 us of timeline apiece, twelve integrations per forward).  Launch A builds the state rows (x, 0) from the caller's points
// (row stride 3 or 4: the previous block's state is taken as it lies), evaluates f0 and sums |y0 / scale|^2 and |f0 / scale|^2;
// launch B evaluates the probe f(t0 + h0, y0 + h0 f0) and sums |(f1 - f0) / scale|^2 without storing f1.  In both, the
// workgroup that finishes last adds the per-workgroup sums in a fixed order and takes the one-thread decision.
struct CnfInitArgs {
    double* ctl;
    const float* x; int xs;   // A: points, row stride in floats
    float* y;                 // [rows,4]  A: written, B: read
    float* f0;                // [rows,4]  A: written, B: read
    const float* ctx; const float* e; const float* rec;
    double t0, t1, n_tot, extra_scale, reverse;
    const double* extra_d0;   // nullable device word: what the state rows outside y add to |y0 / scale|^2 (x extra_scale)
    float sgn, rtol, atol;
    int rows, R, ntiles;
    double* partial;          // [3][1024]
    const double* t_end;      // TDEV: the block's end time T on the device (pf_cnf_pack_blocks' meta row); [t0, t1] = [0, T] / [-T, 0]
};

// TDEV (pf_cnf_init_dev): t0 / t1 from the device word a.t_end instead of the arguments - nothing of the weights' pack is read
// on the host.  Only launch A reads the interval; launch B takes it from ctl.
template <bool PROBE, bool TDEV = false>
__global__ __launch_bounds__(CNF_NW * 64) void cnf_init_kernel(CnfInitArgs a) {
    __shared__ f4 wl[CNF_REC / 4];
    __shared__ double red[2][CNF_NW];
    __shared__ int last;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4;
    const CnfW w = cnf_stage_weights(wl, a.rec, CNF_NW * 64, lane);
    double t0 = a.t0, t1 = a.t1;
    if constexpr (TDEV) {
        const double T = a.t_end[0];
        t0 = a.reverse != 0.0 ? -T : 0.0;
        t1 = a.reverse != 0.0 ? 0.0 : T;
    }
    float h = 0.f, t = (float)(a.reverse != 0.0 ? -t0 : t0);
    if (PROBE) {
        const double hd = a.ctl[CTL_H0], td = a.ctl[CTL_T] + hd;
        h = (float)hd;
        t = (float)(a.ctl[CTL_REV] != 0.0 ? -td : td);
    }
    double acc0 = 0.0, acc1 = 0.0;
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const auto [row, pt, ok] = cnf_tile_row(tile, CNF_NW, wave, col, a.rows, a.R);
        f4 y0, f0 = pf_splat(0.f);
        if (PROBE) {
            y0 = *reinterpret_cast<const f4*>(a.y + (size_t)row * 4);
            f0 = *reinterpret_cast<const f4*>(a.f0 + (size_t)row * 4);
        } else {
            const float* xp = a.x + (size_t)row * a.xs;
            y0 = (f4){xp[0], xp[1], xp[2], 0.f};
            if (ok && q == 0) *reinterpret_cast<f4*>(a.y + (size_t)row * 4) = y0;
        }
        f4 y = y0;
        if (PROBE) y += f0 * (h * 1.f);
        const float* cx = a.ctx + (size_t)pt * CNF_CTX;
        const f4 k = cnf_eval(w, q, y, t, a.sgn, cx, a.e[(size_t)pt * 3 + 0], a.e[(size_t)pt * 3 + 1], a.e[(size_t)pt * 3 + 2]);
        if (ok && q == 0 && !PROBE) *reinterpret_cast<f4*>(a.f0 + (size_t)row * 4) = k;
        if (ok) {                                            // the four lanes of a column take one component each (same box:
                                                             // 12.96 -> 12.86 ms per forward against the q = 0 lanes doing all four)
            const float yc = q == 0 ? y0.x : (q == 1 ? y0.y : (q == 2 ? y0.z : y0.w));
            const float kc = q == 0 ? k.x : (q == 1 ? k.y : (q == 2 ? k.z : k.w));
            const float sc = a.atol + a.rtol * fabsf(yc);
            if (PROBE) {
                const float fc = q == 0 ? f0.x : (q == 1 ? f0.y : (q == 2 ? f0.z : f0.w));
                const float r = (kc - fc) / sc;
                acc0 += (double)r * (double)r;
            } else {
                const float r0 = yc / sc, r1 = kc / sc;
                acc0 += (double)r0 * (double)r0;
                acc1 += (double)r1 * (double)r1;
            }
        }
    }
    acc0 = pf_wave_sum(acc0); acc1 = pf_wave_sum(acc1);
    if (lane == 0) { red[0][wave] = acc0; red[1][wave] = acc1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s0 = 0.0, s1 = 0.0;
        for (int i = 0; i < CNF_NW; ++i) { s0 += red[0][i]; s1 += red[1][i]; }
        PF_ST(a.partial + (PROBE ? 2048 : 0) + blockIdx.x, s0);
        if (!PROBE) PF_ST(a.partial + 1024 + blockIdx.x, s1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned* counter = reinterpret_cast<unsigned*>(a.ctl + CTL_ARRIVE);
        last = atomicAdd(counter, 1u) == gridDim.x - 1 ? 1 : 0;
        if (last) *counter = 0u;
    }
    __syncthreads();
    if (!last) return;                                                                   // uniform over the workgroup
    double* ctl = a.ctl;
    if (PROBE) {
        const double r2 = cnf_partial_total(a.partial + 2048, (int)gridDim.x, red[0]);
        if (threadIdx.x != 0) return;
        const double h0 = ctl[CTL_H0], d1 = ctl[CTL_D1];
        const double d2 = sqrt(r2 / ctl[CTL_NTOT]) / h0;
        const double dm = d1 > d2 ? d1 : d2;
        const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? (1e-6 > h0 * 1e-3 ? 1e-6 : h0 * 1e-3) : pow(0.01 / dm, 1.0 / 5.0);
        ctl[CTL_DT] = 100.0 * h0 < h1 ? 100.0 * h0 : h1;
        ctl[CTL_NFE] = 2.0;
    } else {
        const double r0 = cnf_partial_total(a.partial, (int)gridDim.x, red[0]);
        const double r1 = cnf_partial_total(a.partial + 1024, (int)gridDim.x, red[0]);
        if (threadIdx.x != 0) return;
        for (int i = 0; i < 16; ++i)
            ctl[i] = i == CTL_T ? t0 : i == CTL_T1 ? t1 : i == CTL_NTOT ? a.n_tot : i == CTL_REV ? a.reverse : 0.0;
        const double extra = a.extra_d0 ? a.extra_d0[0] * a.extra_scale : 0.0;
        const double d0 = sqrt((r0 + extra) / a.n_tot), d1 = sqrt(r1 / a.n_tot);
        ctl[CTL_H0] = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        ctl[CTL_D1] = d1;
    }
}

// ---- Runge-Kutta bookkeeping -----------------------------------------------------------------------
struct LinArgs {
    const float* p[8];
    float w[8];
    int n_terms;
    float* out;
    long long n;
};

__global__ __launch_bounds__(256) void lincomb_kernel(LinArgs a) {                 // out = sum_j w[j] p[j]
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    float s = 0.f;
    for (int j = 0; j < a.n_terms; ++j) s = fmaf(a.w[j], a.p[j][i], s);
    a.out[i] = s;
}

// sum over elements of ((A - B) / (atol + rtol * max(|S0|, |S1|)))^2, two deterministic levels, double accumulation.
// A may be given as h * sum_j w[j] K_j (error estimate) by passing n_terms > 0.
struct SumsqArgs {
    const float* a;          // nullable when n_terms > 0
    const float* b;          // nullable
    const float* s0;         // scale state
    const float* s1;         // nullable (second state of the max)
    const float* k;          // [n_terms][n]
    float w[8];
    int n_terms;
    float h, rtol, atol;
    long long n;
    double* partial;         // [gridDim.x]
};

__global__ __launch_bounds__(256) void sumsq_kernel(SumsqArgs s) {
    __shared__ double sh[256];
    double acc = 0.0;
    // a - b against s0 (| s1) with 16-byte loads when the layout allows it (the context norms: 8 M elements per block, one
    // 4-byte load and one division per loop trip took 50 us = 0.66 TB/s); the per-thread order of the additions changes,
    // the double accumulation keeps the sum's low bits out of reach of the step-size heuristic it feeds
    const bool vec = s.n_terms == 0 && (s.n & 3) == 0 && ((reinterpret_cast<size_t>(s.a) | reinterpret_cast<size_t>(s.b) |
                     reinterpret_cast<size_t>(s.s0) | reinterpret_cast<size_t>(s.s1)) & 15) == 0;
    if (vec) {
        const long long n4 = s.n / 4;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
            f4 v = reinterpret_cast<const f4*>(s.a)[i];
            if (s.b) v -= reinterpret_cast<const f4*>(s.b)[i];
            const f4 m0 = reinterpret_cast<const f4*>(s.s0)[i];
            f4 m = {fabsf(m0.x), fabsf(m0.y), fabsf(m0.z), fabsf(m0.w)};
            if (s.s1) {
                const f4 m1 = reinterpret_cast<const f4*>(s.s1)[i];
                m = (f4){fmaxf(m.x, fabsf(m1.x)), fmaxf(m.y, fabsf(m1.y)), fmaxf(m.z, fabsf(m1.z)), fmaxf(m.w, fabsf(m1.w))};
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float r = v[k] / (s.atol + s.rtol * m[k]);
                acc += (double)r * (double)r;
            }
        }
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < s.n && !vec; i += (long long)gridDim.x * 256) {
        float v;
        if (s.n_terms > 0) {
            v = 0.f;
            for (int j = 0; j < s.n_terms; ++j) v = fmaf(s.w[j], s.k[(long long)j * s.n + i], v);
            v *= s.h;
        } else {
            v = s.a[i] - (s.b ? s.b[i] : 0.f);
        }
        float m = fabsf(s.s0[i]);
        if (s.s1) m = fmaxf(m, fabsf(s.s1[i]));
        const float r = v / (s.atol + s.rtol * m);
        acc += (double)r * (double)r;
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) s.partial[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(256) void sumsq_final_kernel(const double* __restrict__ partial, int np, double* __restrict__ out) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += 256) acc += partial[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0];
}

constexpr int SUMSQ_BLOCKS = 256;

// The end of a taped integration whose attempts were enqueued without a look at the controller (pf_cnf_tape_close): the result
// and the derivative at the end go to buffers of FIXED address, whatever the number of accepted steps turned out to be - or quiet
// NaNs when the integration is not clean (attempts ran out, an error status, tape full), so that whatever is computed from it is
// visibly void.  One lane keeps the books in `sticky` (ordinary stores; launches on one stream are ordered).
__global__ __launch_bounds__(256) void cnf_tape_close_kernel(const double* __restrict__ ctl, const float* __restrict__ states, int cap,
                                                             const float* __restrict__ fa, const float* __restrict__ fb, int rows,
                                                             float* __restrict__ y_out, float* __restrict__ f_end, int* sticky) {
    const double done = ctl[CTL_DONE], status = ctl[CTL_STATUS];
    const int n = (int)ctl[CTL_ACC];
    const bool clean = done != 0.0 && status == 0.0 && n >= 0 && n <= cap;      // (n <= cap always: the bound guards the read below)
    const f4 nan4 = pf_splat(__builtin_nanf(""));
    const f4* ys = reinterpret_cast<const f4*>(states) + (size_t)(clean ? n : 0) * rows;
    const f4* fs = reinterpret_cast<const f4*>(ctl[CTL_CUR] != 0.0 ? fb : fa);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < rows; i += gridDim.x * 256) {
        reinterpret_cast<f4*>(y_out)[i] = clean ? ys[i] : nan4;
        reinterpret_cast<f4*>(f_end)[i] = clean ? fs[i] : nan4;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sticky[0] += 1;
        if (!clean) {
            sticky[1] += 1;
            sticky[2] = done == 0.0 ? 4 : (status != 0.0 ? (int)status : 3);
        }
        const int took = (int)(ctl[CTL_ACC] + ctl[CTL_REJ]);
        if (took > sticky[3]) sticky[3] = took;
    }
}

}  // namespace

extern "C" int pf_cnf_rhs(const float* y0, const float* k, const float* coef, int ncoef, float h, float t, float sgn,
                          const float* ctx, const float* e, const float* rec, float* kout, float* yout, int rows, int R,
                          void* stream) {
    if (!y0 || !ctx || !e || !rec || !kout || (ncoef > 0 && (!k || !coef))) return PF_ERR_NULL;
    if (rows <= 0 || R <= 0 || ncoef < 0 || ncoef > 6) return PF_ERR_SHAPE;
    CnfArgs a{};
    a.y0 = y0; a.k = k; a.ncoef = ncoef; a.h = h; a.t = t; a.sgn = sgn; a.ctx = ctx; a.e = e; a.rec = rec;
    a.kout = kout; a.yout = yout; a.rows = rows; a.R = R;
    for (int j = 0; j < ncoef; ++j) a.coef[j] = coef[j];
    const int grid = cnf_grid(rows, CNF_NW * 16, &a.ntiles);
    hipLaunchKernelGGL(cnf_rhs_kernel, dim3(grid), dim3(CNF_NW * 64), 0, (hipStream_t)stream, a);
    return pf_last_launch_status();
}

// out[i] = sum_j w[j] * p[j][i], j < n_terms <= 8 (host arrays of device pointers / weights)
extern "C" int pf_lincomb(const float* const* ptrs, const float* w, int n_terms, float* out, long long n, void* stream) {
    if (!ptrs || !w || !out) return PF_ERR_NULL;
    if (n_terms <= 0 || n_terms > 8 || n <= 0) return PF_ERR_SHAPE;
    LinArgs a{};
    for (int j = 0; j < n_terms; ++j) {
        if (!ptrs[j]) return PF_ERR_NULL;
        a.p[j] = ptrs[j]; a.w[j] = w[j];
    }
    a.n_terms = n_terms; a.out = out; a.n = n;
    hipLaunchKernelGGL(lincomb_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return pf_last_launch_status();
}

// out[0] (double) = sum_i (v_i / (atol + rtol * max(|s0_i|, |s1_i|)))^2 with v = a - b, or v = h * sum_j w[j] k[j] when
// n_terms > 0 (k: [n_terms][n]).  ws: >= 256 doubles of scratch.  Deterministic (fixed two-level tree).
extern "C" int pf_scaled_sumsq(const float* a, const float* b, const float* s0, const float* s1, const float* k,
                               const float* w, int n_terms, float h, float rtol, float atol, long long n, double* ws,
                               double* out, void* stream) {
    if (!s0 || !ws || !out || (n_terms == 0 && !a) || (n_terms > 0 && (!k || !w))) return PF_ERR_NULL;
    if (n <= 0 || n_terms < 0 || n_terms > 8) return PF_ERR_SHAPE;
    SumsqArgs s{};
    s.a = a; s.b = b; s.s0 = s0; s.s1 = s1; s.k = k; s.n_terms = n_terms; s.h = h; s.rtol = rtol; s.atol = atol;
    s.n = n; s.partial = ws;
    for (int j = 0; j < n_terms; ++j) s.w[j] = w[j];
    hipLaunchKernelGGL(sumsq_kernel, dim3(SUMSQ_BLOCKS), dim3(256), 0, (hipStream_t)stream, s);
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, SUMSQ_BLOCKS, out);
    return pf_last_launch_status();
}

// One Dormand-Prince 5(4) step attempt: y1 = y0 + h sum b_j k_j (k_1 = f0 given, FSAL), f1 = k_7, optional dense-output
// mid-point, and out[0] (double) = sum_i (err_i / (atol + rtol max(|y0_i|, |y1_i|)))^2 of the embedded error estimate.
// t: start of the step in solver time; reverse != 0 integrates the way torchdiffeq does for decreasing times
// (net time = -solver time, derivative negated).  ws: >= 1024 doubles.
extern "C" int pf_cnf_step(const float* y0, const float* f0, float t, float h, int reverse, const float* ctx, const float* e,
                           const float* rec, float* y1, float* f1, float* ymid, float rtol, float atol, int rows, int R,
                           double* ws, double* out, void* stream) {
    if (!y0 || !f0 || !ctx || !e || !rec || !y1 || !f1 || !ws || !out) return PF_ERR_NULL;
    if (rows <= 0 || R <= 0) return PF_ERR_SHAPE;
    CnfStepArgs a{};
    a.y0 = y0; a.f0 = f0; a.ctx = ctx; a.e = e; a.rec = rec; a.y1 = y1; a.f1 = f1; a.ymid = ymid; a.partial = ws;
    a.t = t; a.h = h; a.sgn = reverse ? -1.f : 1.f; a.tsign = reverse ? -1.f : 1.f; a.rtol = rtol; a.atol = atol;
    a.rows = rows; a.R = R;
    const int grid = cnf_grid(rows, CNF_NW * 16, &a.ntiles);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cnf_step_kernel, dim3(grid), dim3(CNF_NW * 64), 0, s, a);
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, s, ws, grid, out);
    return pf_last_launch_status();
}

// `n_attempts` step attempts of the adaptive integration whose state is in `ctl` (layout above), enqueued back to back; the
// controller's decision is taken inside each attempt's launch by the workgroup that finishes last: no host synchronisation.  ya / yb and fa / fb: the two state and derivative buffers
// ([rows,4]; ctl's `cur` says which one holds the current state), out: the solution at t1 once ctl's `done` is set with
// status 0.  ws: >= 1024 doubles.
// flags: PF_CNF_SPLIT_GATES - the caller vouches that log2(e) max|gate time weight| |t1 - t0| <= 100 for this record
// (packing.cnf_split_ok); the gates' 2^x then factor into a per-point and a per-stage part without overflow (cnf_eval).
extern "C" int pf_cnf_steps(double* ctl, float* ya, float* yb, float* fa, float* fb, const float* ctx, const float* e,
                            const float* rec, float* out, float rtol, float atol, int rows, int R, int n_attempts, double* ws,
                            int flags, void* stream) {
    if (!ctl || !ya || !yb || !fa || !fb || !ctx || !e || !rec || !out || !ws) return PF_ERR_NULL;
    if (rows <= 0 || R <= 0 || n_attempts <= 0) return PF_ERR_SHAPE;
    CnfDevArgs a{};
    a.ctl = ctl; a.yb[0] = ya; a.yb[1] = yb; a.fb[0] = fa; a.fb[1] = fb; a.ctx = ctx; a.e = e; a.rec = rec; a.out = out;
    a.partial = ws; a.rtol = rtol; a.atol = atol; a.rows = rows; a.R = R;
    const int grid = cnf_grid(rows, CNF_NW * 16, &a.ntiles);
    hipStream_t s = (hipStream_t)stream;
    const bool lds = R >= 4 && (CNF_NW * 16) % R == 0;     // context rows through LDS when a tile's 64 rows belong to <= 16 whole points
    const bool split = (flags & PF_CNF_SPLIT_GATES) && (lds || PF_CNF_SPLIT_FWD);
    void (*kern)(CnfDevArgs) = lds ? (split ? cnf_step_dev_kernel<true, true> : cnf_step_dev_kernel<true, false>)
                                   : (split ? cnf_step_dev_kernel<false, true> : cnf_step_dev_kernel<false, false>);
    for (int i = 0; i < n_attempts; ++i) hipLaunchKernelGGL(kern, dim3(grid), dim3(CNF_NW * 64), 0, s, a);
    return pf_last_launch_status();
}

// pf_cnf_steps for an integration whose accepted steps a backward sweep replays (pf_cnf_tape_vjp): plain gates, the states on a
// tape instead of two buffers, the covering step cut to end at t1 (include/puflow_hip.h).
extern "C" int pf_cnf_steps_taped(double* ctl, float* states, float* steps, int cap, float* fa, float* fb, const float* ctx,
                                  const float* e, const float* rec, float rtol, float atol, int rows, int R, int n_attempts,
                                  double* ws, void* stream) {
    if (!ctl || !states || !steps || !fa || !fb || !ctx || !e || !rec || !ws) return PF_ERR_NULL;
    if (rows <= 0 || R <= 0 || n_attempts <= 0 || cap <= 0) return PF_ERR_SHAPE;
    CnfDevArgs a{};
    a.ctl = ctl; a.yb[0] = states; a.yb[1] = states; a.fb[0] = fa; a.fb[1] = fb; a.ctx = ctx; a.e = e; a.rec = rec; a.out = nullptr;
    a.partial = ws; a.rtol = rtol; a.atol = atol; a.rows = rows; a.R = R; a.states = states; a.steps = steps; a.cap = cap;
    const int grid = cnf_grid(rows, CNF_NW * 16, &a.ntiles);
    hipStream_t s = (hipStream_t)stream;
    const bool lds = R >= 4 && (CNF_NW * 16) % R == 0;
    void (*kern)(CnfDevArgs) = lds ? cnf_step_dev_kernel<true, false, true> : cnf_step_dev_kernel<false, false, true>;
    for (int i = 0; i < n_attempts; ++i) hipLaunchKernelGGL(kern, dim3(grid), dim3(CNF_NW * 64), 0, s, a);
    return pf_last_launch_status();
}

// The start of an adaptive integration over [t0, t1] (solver time; the network sees -t when reverse), all on the device, two
// launches (cnf_init_kernel): the state rows y = (x, 0) from the points x (row stride x_stride = 3 or 4 floats), f0 = f(t0, y),
// the controller state reset, torchdiffeq's initial step size into ctl[1].  n_tot: elements of the RMS norms (rows*4 + the
// context rows torchdiffeq integrates alongside), extra_d0 (a DEVICE double, nullable) x extra_scale: what those extra rows
// add to the squared norm of y0 (pf_scaled_sumsq of the context with itself as the scale; the host never reads it).
// ws: >= 3072 doubles.  ctl: 16 doubles, ALL ZERO before its first use (the arrival word at [13] is left zero by every launch).
// Both entry points launch from here: pf_cnf_init with (t0, t1) from the host, pf_cnf_init_dev with t_end, a device word.
namespace {
int cnf_init_launch(double* ctl, const float* x, int x_stride, float* y, float* f0, const float* ctx, const float* e,
                    const float* rec, double t0, double t1, const double* t_end, double n_tot, const double* extra_d0,
                    double extra_scale, int reverse, float rtol, float atol, int rows, int R, double* ws, void* stream) {
    if (!ctl || !x || !y || !f0 || !ctx || !e || !rec || !ws) return PF_ERR_NULL;
    if (rows <= 0 || R <= 0 || !(n_tot > 0.0) || (x_stride != 3 && x_stride != 4)) return PF_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    CnfInitArgs a{};
    a.ctl = ctl; a.x = x; a.xs = x_stride; a.y = y; a.f0 = f0; a.ctx = ctx; a.e = e; a.rec = rec;
    a.t0 = t0; a.t1 = t1; a.t_end = t_end; a.n_tot = n_tot; a.extra_d0 = extra_d0; a.extra_scale = extra_scale; a.reverse = reverse ? 1.0 : 0.0;
    a.sgn = reverse ? -1.f : 1.f; a.rtol = rtol; a.atol = atol; a.rows = rows; a.R = R; a.partial = ws;
    const int grid = cnf_grid(rows, CNF_NW * 16, &a.ntiles);
    if (t_end) hipLaunchKernelGGL((cnf_init_kernel<false, true>), dim3(grid), dim3(CNF_NW * 64), 0, s, a);
    else hipLaunchKernelGGL(cnf_init_kernel<false>, dim3(grid), dim3(CNF_NW * 64), 0, s, a);
    hipLaunchKernelGGL(cnf_init_kernel<true>, dim3(grid), dim3(CNF_NW * 64), 0, s, a);
    return pf_last_launch_status();
}
}  // namespace

extern "C" int pf_cnf_init(double* ctl, const float* x, int x_stride, float* y, float* f0, const float* ctx, const float* e,
                           const float* rec, double t0, double t1, double n_tot, const double* extra_d0, double extra_scale,
                           int reverse, float rtol, float atol, int rows, int R, double* ws, void* stream) {
    return cnf_init_launch(ctl, x, x_stride, y, f0, ctx, e, rec, t0, t1, nullptr, n_tot, extra_d0, extra_scale, reverse, rtol, atol,
                           rows, R, ws, stream);
}

// pf_cnf_init with the interval taken from the device: t_end[0] = T (a word of pf_cnf_pack_blocks' meta row), [t0, t1] = [0, T],
// reversed [-T, 0].  Nothing about the block's weights passes through the host.
extern "C" int pf_cnf_init_dev(double* ctl, const float* x, int x_stride, float* y, float* f0, const float* ctx, const float* e,
                               const float* rec, const double* t_end, double n_tot, const double* extra_d0, double extra_scale,
                               int reverse, float rtol, float atol, int rows, int R, double* ws, void* stream) {
    if (!t_end) return PF_ERR_NULL;
    return cnf_init_launch(ctl, x, x_stride, y, f0, ctx, e, rec, 0.0, 0.0, t_end, n_tot, extra_d0, extra_scale, reverse, rtol, atol,
                           rows, R, ws, stream);
}

// One launch behind a blind batch of pf_cnf_steps_taped attempts (include/puflow_hip.h).
extern "C" int pf_cnf_tape_close(const double* ctl, const float* states, int cap, const float* fa, const float* fb, int rows,
                                 float* y_out, float* f_end, int* sticky, void* stream) {
    if (!ctl || !states || !fa || !fb || !y_out || !f_end || !sticky) return PF_ERR_NULL;
    if (cap <= 0 || rows <= 0) return PF_ERR_SHAPE;
    const int grid = (rows + 255) / 256 < 256 ? (rows + 255) / 256 : 256;
    hipLaunchKernelGGL(cnf_tape_close_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, ctl, states, cap, fa, fb, rows, y_out,
                       f_end, sticky);
    return pf_last_launch_status();
}
