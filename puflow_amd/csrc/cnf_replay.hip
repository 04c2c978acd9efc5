// A continuous block integrated on a step list chosen IN ADVANCE (a frozen schedule): Dormand-Prince steps without a controller.
// On a fixed list nothing couples the rows - the error norm, a sum over all rows, decides nothing - so a lane carries its row
// through all steps in registers and a whole integration is ONE launch (+ one small launch when the caller asks for the
// per-step error sums).  The forward counterpart of pf_cnf_tape_vjp (csrc/cnf_bwd.hip): it writes the tape that sweep reads.
// The arithmetic is the taped adaptive path's (csrc/cnf.hip: cnf_init_kernel's f0, cnf_step_dev_kernel<.., false, true>), from
// the same functions (csrc/pf_cnf_eval.h, plain gates): replaying the steps that path recorded gives its bits.
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"
#include "pf_mfma.h"
#include "pf_wave.h"
#include "pf_cnf.h"
#include "pf_cnf_eval.h"

namespace {

constexpr int RP_NW = 4;                  // waves per workgroup: a tile is 64 rows, as in csrc/cnf.hip

struct CnfReplayArgs {
    const float* x; int xs;   // points, row stride in floats (3 or 4)
    const float* steps;       // [n_steps][2] (s, h), device
    int n_steps;
    const float* ctx; const float* e; const float* rec;
    float* states;            // nullable [n_steps + 1][rows][4]
    float* y_out;             // [rows][4]
    float* f_start;           // nullable [rows][4]
    float* f_end;             // nullable [rows][4]
    double* part;             // nullable [n_steps][gridDim.x * RP_NW]: each wave's share of each step's error sum
    float sgn, rtol, atol;
    int rows, R, ntiles;
};

// CTX_LDS (R >= 4 rows per original point, whole points per tile): the context rows of the tile's 64 / R points go to LDS once
// per tile and all 6 n_steps + 1 evaluations read them there.
template <bool CTX_LDS>
__global__ __launch_bounds__(RP_NW * 64, 2) void cnf_replay_kernel(CnfReplayArgs a) {
    __shared__ f4 wl[CNF_REC / 4];
    __shared__ f4 sctx[CTX_LDS ? RP_NW * 4 * CNF_CTX / 4 : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4;
    const CnfW w = cnf_stage_weights(wl, a.rec, RP_NW * 64, lane);
    const float sgn = a.sgn, tsign = a.sgn;
    const size_t plane = (size_t)a.rows * 4;
    const size_t nslots = (size_t)gridDim.x * RP_NW, slot = (size_t)blockIdx.x * RP_NW + wave;
    bool first = true;
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const auto [row, pt, ok] = cnf_tile_row(tile, RP_NW, wave, col, a.rows, a.R);
        const float* cx = a.ctx + (size_t)pt * CNF_CTX;
        if (CTX_LDS) {
            const int ppw = RP_NW * 16 / a.R;                      // points of this workgroup's tile (<= 16)
            const long long p0 = (long long)tile * ppw;
            const long long npts = ((long long)a.rows + a.R - 1) / a.R;
            __syncthreads();                                       // every wave is done with the previous tile's rows
            for (int i = threadIdx.x; i < ppw * (CNF_CTX / 4); i += RP_NW * 64) {
                const long long pp = p0 + i / (CNF_CTX / 4);
                sctx[i] = reinterpret_cast<const f4*>(a.ctx)[(pp < npts ? pp : npts - 1) * (CNF_CTX / 4) + i % (CNF_CTX / 4)];
            }
            __syncthreads();
            const long long pl = pt - p0;                          // a clamped out-of-range lane may point past the tile
            cx = reinterpret_cast<const float*>(sctx) + (size_t)(pl < 0 ? 0 : (pl >= ppw ? ppw - 1 : pl)) * CNF_CTX;
        }
        const float e0 = a.e[(size_t)pt * 3 + 0], e1 = a.e[(size_t)pt * 3 + 1], e2 = a.e[(size_t)pt * 3 + 2];
        const float* xp = a.x + (size_t)row * a.xs;
        f4 y = (f4){xp[0], xp[1], xp[2], 0.f};
        const bool st = ok && q == 0;
        f4 k[7];
        k[0] = cnf_eval(w, q, y, tsign * a.steps[0], sgn, cx, e0, e1, e2);
        if (st && a.f_start) *reinterpret_cast<f4*>(a.f_start + (size_t)row * 4) = k[0];
        for (int n = 0; n < a.n_steps; ++n) {
            const float s = a.steps[2 * n], h = a.steps[2 * n + 1];
            if (st && a.states) *reinterpret_cast<f4*>(a.states + n * plane + (size_t)row * 4) = y;
            f4 yi = y;
            const f4 err = cnf_dopri_stages<false, false, 0>(w, q, y, k, yi, s, h, sgn, tsign, cx, e0, e1, e2, nullptr, cx);
            if (a.part) {                                            // uniform over the grid
                double acc = 0.0;
                if (st) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float r = err[c] / (a.atol + a.rtol * fmaxf(fabsf(y[c]), fabsf(yi[c])));
                        acc += (double)r * (double)r;
                    }
                }
                acc = pf_wave_sum(acc);
                // this wave's slot of step n: its tiles one after the other, one lane, ordinary stores
                if (lane == 0) {
                    double* p = a.part + (size_t)n * nslots + slot;
                    *p = first ? acc : *p + acc;
                }
            }
            y = yi;
            k[0] = k[6];                                             // FSAL
        }
        if (st) {
            if (a.states) *reinterpret_cast<f4*>(a.states + a.n_steps * plane + (size_t)row * 4) = y;
            *reinterpret_cast<f4*>(a.y_out + (size_t)row * 4) = y;
            if (a.f_end) *reinterpret_cast<f4*>(a.f_end + (size_t)row * 4) = k[0];
        }
        first = false;
    }
}

// errsq[n] = the wave shares of step n added in a fixed order (one workgroup per step)
__global__ __launch_bounds__(256) void cnf_replay_errsq_kernel(const double* __restrict__ part, int nslots, double* __restrict__ errsq) {
    __shared__ double sh[256];
    const double* p = part + (size_t)blockIdx.x * nslots;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nslots; i += 256) acc += p[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) errsq[blockIdx.x] = sh[0];
}

}  // namespace

extern "C" long long pf_cnf_replay_workspace_bytes(int rows, int n_steps) {
    if (rows <= 0 || n_steps < 1) return PF_ERR_SHAPE;
    int ntiles;
    const int grid = cnf_grid(rows, RP_NW * 16, &ntiles);
    return (long long)grid * RP_NW * n_steps * (long long)sizeof(double);
}

extern "C" int pf_cnf_replay(const float* x, int x_stride, const float* steps, int n_steps, int reverse, const float* ctx,
                             const float* e, const float* rec, float* states, float* y_out, float* f_start, float* f_end,
                             double* errsq, float rtol, float atol, int rows, int R, void* ws, void* stream) {
    if (!x || !steps || !ctx || !e || !rec || !y_out || (errsq && !ws)) return PF_ERR_NULL;
    if (rows <= 0 || R < 1 || rows % R != 0 || n_steps < 1 || (x_stride != 3 && x_stride != 4)) return PF_ERR_SHAPE;
    CnfReplayArgs a{};
    a.x = x; a.xs = x_stride; a.steps = steps; a.n_steps = n_steps; a.ctx = ctx; a.e = e; a.rec = rec; a.states = states;
    a.y_out = y_out; a.f_start = f_start; a.f_end = f_end; a.part = errsq ? static_cast<double*>(ws) : nullptr;
    a.sgn = reverse ? -1.f : 1.f; a.rtol = rtol; a.atol = atol; a.rows = rows; a.R = R;
    const int grid = cnf_grid(rows, RP_NW * 16, &a.ntiles);
    hipStream_t s = (hipStream_t)stream;
    const bool lds = R >= 4 && (RP_NW * 16) % R == 0;      // a tile's 64 rows belong to <= 16 whole points
    if (lds) hipLaunchKernelGGL(cnf_replay_kernel<true>, dim3(grid), dim3(RP_NW * 64), 0, s, a);
    else hipLaunchKernelGGL(cnf_replay_kernel<false>, dim3(grid), dim3(RP_NW * 64), 0, s, a);
    if (errsq) hipLaunchKernelGGL(cnf_replay_errsq_kernel, dim3(n_steps), dim3(256), 0, s, a.part, grid * RP_NW, errsq);
    return pf_last_launch_status();
}
