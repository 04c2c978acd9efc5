// What the continuous (CNF) kernels share: the layouts of the weight record, the context row and the gradient record, the
// hardware-exp activations, the record's LDS staging, the Dormand-Prince tableau and the tile -> row mapping.  Included by
// csrc/cnf.hip, csrc/cnf_replay.hip, csrc/cnf_bwd.hip and csrc/cnf_pack.hip (which WRITES the record and the context matrices on the device, bit for
// bit what packing.py makes on the host); packing.py carries the same names with the same values (tests/test_cnf_layout.py).
// Device and host, everything inline.  All offsets in floats.
#pragma once
#include <hip/hip_runtime.h>
#include "pf_mfma.h"

// Weight record of one block (packing.pack_cnf_block), resident in LDS:
//   CNF_W2   f16x2 image of 2 log2e W2 [64][64]        CNF_W2T  f16x2 image of W2^T (plain)
//   CNF_W3   f16x2 image of W3 (its 3 rows replicated into every 4-row q group of a 16-row block)
//   CNF_W1B  2 log2e [W1 | b1]  [64][4]                CNF_W3T  W3^T [64][4] (3 used, 4th zero)
//   CNF_B1   b1 [64] (plain)    CNF_B2  2 log2e b2 [64]    CNF_B3  b3 [16] (replicated like W3)
//   CNF_TV   the time coefficients [288], in the context row's layout
constexpr int CNF_W2 = 0, CNF_W2T = 4096, CNF_W3 = 8192, CNF_W1B = 9216, CNF_W3T = 9472, CNF_B1 = 9728, CNF_B2 = 9792,
              CNF_B3 = 9856, CNF_TV = 9872, CNF_REC = 10160;
// Context row per original point and block (ctx = Hc c + hb: pf_cnf_context), also of the time coefficients and of ctxbar:
// gate1 [64] bias1 [64] gate2 [64] bias2 [64] gate3 [16] bias3 [16], layer 3 as 3 values replicated into four 4-float slots.
// Gate columns carry -log2e x their pre-activation, the bias columns of the two tanh layers 2 log2e x.
constexpr int CNF_CTX_G1 = 0, CNF_CTX_B1 = 64, CNF_CTX_G2 = 128, CNF_CTX_B2 = 192, CNF_CTX_G3 = 256, CNF_CTX_B3 = 272, CNF_CTX = 288;
// Compact gate row (cnf_step_dev_kernel<false, true>): the 144 gate columns alone, gate1 gate2 gate3 one after the other.
constexpr int CNF_GATE_G2 = 64, CNF_GATE_G3 = 128, CNF_GATES = 144;
// Gradient record of pf_cnf_rhs_vjp (include/puflow_hip.h states it for callers), in the units of the model's parameters:
// dW2 [64][64], dW1 [64][3], db1 [64], db2 [64], dW3 [3][64], db3 [3], one unused word (written as zero), then the gradients
// of the time coefficients [288] in the context row's layout (layer 3: the first slot only).
constexpr int CNF_GRAD_W2 = 0, CNF_GRAD_W1 = 4096, CNF_GRAD_B1 = 4288, CNF_GRAD_B2 = 4352, CNF_GRAD_W3 = 4416, CNF_GRAD_B3 = 4608,
              CNF_GRAD_UNUSED = 4611, CNF_GRAD_TV = 4612, CNF_GRAD = 4900;

// every region starts where the one before it ends (64 hidden channels; a [16][64] block's f16x2 image is 1024 floats)
static_assert(CNF_W2T == CNF_W2 + 4096 && CNF_W3 == CNF_W2T + 4096 && CNF_W1B == CNF_W3 + 1024 && CNF_W3T == CNF_W1B + 64 * 4 &&
              CNF_B1 == CNF_W3T + 64 * 4 && CNF_B2 == CNF_B1 + 64 && CNF_B3 == CNF_B2 + 64 && CNF_TV == CNF_B3 + 16 &&
              CNF_REC == CNF_TV + CNF_CTX && CNF_REC % 4 == 0, "weight record (staged as float4)");
static_assert(CNF_CTX_B1 == CNF_CTX_G1 + 64 && CNF_CTX_G2 == CNF_CTX_B1 + 64 && CNF_CTX_B2 == CNF_CTX_G2 + 64 && CNF_CTX_G3 == CNF_CTX_B2 + 64 &&
              CNF_CTX_B3 == CNF_CTX_G3 + 16 && CNF_CTX == CNF_CTX_B3 + 16 && CNF_GATE_G3 == CNF_GATE_G2 + 64 && CNF_GATES == CNF_GATE_G3 + 16,
              "context row, compact gate row");
static_assert(CNF_GRAD_W1 == CNF_GRAD_W2 + 64 * 64 && CNF_GRAD_B1 == CNF_GRAD_W1 + 64 * 3 && CNF_GRAD_B2 == CNF_GRAD_B1 + 64 &&
              CNF_GRAD_W3 == CNF_GRAD_B2 + 64 && CNF_GRAD_B3 == CNF_GRAD_W3 + 3 * 64 && CNF_GRAD_UNUSED == CNF_GRAD_B3 + 3 &&
              CNF_GRAD_TV == CNF_GRAD_UNUSED + 1 && CNF_GRAD == CNF_GRAD_TV + CNF_CTX, "gradient record");

// is column r of a context row a gate column / the context column of compact gate column c
__device__ __forceinline__ bool cnf_gate_row(int r) { return r < CNF_CTX_B1 || (r >= CNF_CTX_G2 && r < CNF_CTX_B2) || (r >= CNF_CTX_G3 && r < CNF_CTX_B3); }
__device__ __forceinline__ int cnf_gate_col(int c) {
    return c < CNF_GATE_G2 ? c : (c < CNF_GATE_G3 ? c + (CNF_CTX_G2 - CNF_GATE_G2) : c + (CNF_CTX_G3 - CNF_GATE_G3));
}

// sigmoid and tanh on the hardware exp / rcp (1 ulp each): absolute error ~2e-7, against ~25 instructions for tanhf and a
// full-precision division - the right-hand side is bound by these (32 tanh + 32 sigmoid per lane and evaluation), not by its
// 54 MFMAs.  tanh(x) = 1 - 2 / (e^{2x} + 1) saturates correctly (e -> inf: 1, e -> 0: -1).
// The arguments arrive PRESCALED by the host (packing.pack_cnf_block): gates carry -log2e x, the tanh layers' pre-activations
// 2 log2e x, so each function is v_exp_f32 + add + v_rcp_f32 (+ one fma): one multiply per gate and per tanh saved.
__device__ __forceinline__ float sigm(float xs) { return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(xs)); }          // xs = -log2e x
__device__ __forceinline__ float tanh_fast(float xs) { return fmaf(-2.f, __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(xs) + 1.f), 1.f); }   // xs = 2 log2e x
constexpr float CNF_INV_2LOG2E = 0.34657359027997264f;      // 1 / (2 log2e): takes the record's fold out of W1, W2, b2 products

struct CnfW {                  // the record in LDS and the three split-fp16 images inside it
    const float* rec;
    PfW2Lds w2, w2t, w3;
};

// the record from global memory into the workgroup's LDS array wl, behind a barrier -> its views
__device__ __forceinline__ CnfW cnf_stage_weights(f4* wl, const float* rec_g, int nthreads, int lane) {
    for (int i = threadIdx.x; i < CNF_REC / 4; i += nthreads) wl[i] = reinterpret_cast<const f4*>(rec_g)[i];
    __syncthreads();
    const float* rec = reinterpret_cast<const float*>(wl);
    return CnfW{rec, PfW2Lds{reinterpret_cast<const u4*>(rec + CNF_W2), lane}, PfW2Lds{reinterpret_cast<const u4*>(rec + CNF_W2T), lane},
                PfW2Lds{reinterpret_cast<const u4*>(rec + CNF_W3), lane}};
}

// Dormand-Prince 5(4): stage times, stage coefficients, embedded error estimate (b - b*), dense-output mid-point
constexpr float CNF_AL[6] = {1.f / 5, 3.f / 10, 4.f / 5, 8.f / 9, 1.f, 1.f};
constexpr float CNF_BE[6][6] = {
    {1.f / 5, 0, 0, 0, 0, 0},
    {3.f / 40, 9.f / 40, 0, 0, 0, 0},
    {44.f / 45, -56.f / 15, 32.f / 9, 0, 0, 0},
    {19372.f / 6561, -25360.f / 2187, 64448.f / 6561, -212.f / 729, 0, 0},
    {9017.f / 3168, -355.f / 33, 46732.f / 5247, 49.f / 176, -5103.f / 18656, 0},
    {35.f / 384, 0, 500.f / 1113, 125.f / 192, -2187.f / 6784, 11.f / 84}};
constexpr float CNF_CE[7] = {(float)(35. / 384 - 1951. / 21600), 0, (float)(500. / 1113 - 22642. / 50085),
                             (float)(125. / 192 - 451. / 720), (float)(-2187. / 6784 + 12231. / 42400),
                             (float)(11. / 84 - 649. / 6300), (float)(-1. / 60)};
constexpr float CNF_CM[7] = {(float)(6025192743. / 30085553152 / 2), 0, (float)(51252292925. / 65400821598 / 2),
                             (float)(-2691868925. / 45128329728 / 2), (float)(187940372067. / 1594534317056 / 2),
                             (float)(-1776094331. / 19743644256 / 2), (float)(11237099. / 235043384 / 2)};

// sum_j c[j] k[j] over the seven stage derivatives, in the order j = 0 .. 6 (error estimate, mid-point)
__device__ __forceinline__ f4 cnf_comb7(const f4 (&k)[7], const float (&c)[7]) {
    f4 s = k[0] * c[0];
#pragma unroll
    for (int j = 1; j < 7; ++j) s += k[j] * c[j];
    return s;
}

// A tile is `nw` waves x 16 rows; lane column `col` of wave `wave` takes row (tile nw + wave) 16 + col.  Lanes past the end
// re-read the last row (ok = false: they store nothing and add nothing).  pt: the row's original point.
struct CnfRow { int row, pt; bool ok; };
__device__ __forceinline__ CnfRow cnf_tile_row(int tile, int nw, int wave, int col, int rows, int R) {
    const int g = (tile * nw + wave) * 16 + col;
    const bool ok = g < rows;
    const int row = ok ? g : rows - 1;
    return CnfRow{row, row / R, ok};
}

inline int cnf_grid(int rows, int tile_rows, int* ntiles) {      // -> workgroups, at most 1024: the size of the partial-sum arrays
    *ntiles = (rows + tile_rows - 1) / tile_rows;
    return *ntiles < 1024 ? *ntiles : 1024;
}
