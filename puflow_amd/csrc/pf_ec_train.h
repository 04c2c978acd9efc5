// One FeatureExtractUnit (EdgeConv dense block) of the TRAINING step as a handful of launches.
//
// Reference: modules/discrete/interpflow.py:190-248 (FeatureExtractUnit.forward in train() mode: edge feature ->
// [Conv2d 1x1 + BatchNorm2d (batch statistics) + LeakyReLU(0.05), dense concatenation] x nconv -> conv_out -> max over the K
// neighbours) and the autograd backward PyTorch derives from it.  The un-fused path (train_ops.hip + train_ops.py) runs
// this as ~170 launches per unit and step (GEMM, two-pass statistics, apply, concatenations, gradient adds); at
// 32 x 256 points every one of those kernels is shorter than the gap between two launches, so the step was bound by the
// NUMBER of launches.  Here a unit is 7 launches forward and ~12 backward:
//
//   forward   fold        Wp = W1 - W3, Wq = W2 + W3 of all convs -> Wpq [2S, C]   (the edge feature [x_i; x_j; x_j - x_i]
//                         enters every conv only through P = Wp x_i (+ bias) and Q = Wq x_j: packing.fold_edgeconv)
//             gemm        PQ [T, 2S] = x Wpq^T + bias                              (train_ops.hip: pf_gemm)
//             layer t     Y[:, g t : g (t+1)] = P_t[i] + Q_t[j] + lrelu(bn(Y[:, :g t])) Wg_t^T   - the BatchNorm of the
//                         EARLIER layers is applied on load (scale / shift per channel), this layer's pre-activation
//                         output is stored and its column sums / sums of squares leave in the epilogue
//                         (the workgroup that finishes last turns the sums into scale / shift / running statistics)
//             out         conv_out on lrelu(bn(Y)) + P_out[i] + Q_out[j], max over the 16 edges of a point in the MFMA
//                         accumulator layout (the [E, odim] tensor is never written), argmax kept for the backward
//   backward  out         dA [E, GT] = dYout Wg_out, dYout generated from (dh, argmax) on load; epilogue: BatchNorm-backward
//                         sums of the last growth layer
//             layer t     (t = nconv-1 .. 1)  dy_t = BN-backward of dA[:, slice t] formed on load and stored in place;
//                         dA[:, :g t] += dy_t Wg_t; epilogue: sums for layer t-1
//             layer 0     dA[:, :g] -> dy_0 in place
//             pq          dP[i] = sum_k dy, dQ[j] += dy (atomics), conv_out part from (dh, argmax)
//             dw          all growth-weight gradients of the unit in ONE split-K launch: [S, GT] = dY^T lrelu(bn(Y))
//             gemm x2     dx = dPQ Wpq, dWpq = dPQ^T x
//             assemble    conv weight gradients [*, 3C + g t] from dWpq (un-folding) and the dw partial sums
//
// All matrix products are v_mfma_f32_16x16x4_f32 (exact fp32 fma chains).  Rows of every per-edge tensor are edges in
// point-major order (e = i K + k), so a 16-row MFMA tile is one point's 16 neighbours (K = 16) or two points (K = 8).
//
// Files: train_ec_fwd.hip (fold, per-layer and persistent forward), train_fused.hip (backward, weight gradients, assembly, the
// shape checks and workspace layout both directions use), train_csr.hip (the transposed neighbour lists of the dPQ gather);
// this header holds what the two EdgeConv files share.
#pragma once
#include "pf_train_stat.h"

extern "C" int pf_gemm(const float* A, long long sam, long long sak, const float* B, long long sbk, long long sbn, float* C,
                       long long ldc, const float* bias, int M, int N, int K, float* ws, long long ws_floats, void* stream);
extern "C" long long pf_gemm_ws_floats(int M, int N, int K);

// shapes of one unit (pf_ec_dims)
struct EcDims {
    int T, GT, S, nconvs;
    long long E;
    int ntiles, grid, grid_light, nchunk, chunk;
};
// the convs of a unit as the fold / assemble kernels take them (pf_ec_convs)
struct EcConvs {
    const float* W[9]; const float* bias[9];
    float* dW[9]; float* dbias[9];
    int rows[9], rowoff[10], width[9];      // conv t: [rows, width = 3C + g t]; rowoff: first row in the S-row stacking
    int nconvs, C, S, GT;
};

// defined in train_fused.hip
PF_INTERNAL int pf_ec_dims(const PfEcTrain* p, EcDims& d);
PF_INTERNAL EcConvs pf_ec_convs(const PfEcTrain* p, const EcDims& d);
PF_INTERNAL long long pf_ec_gemm_ws_max(const PfEcTrain* p, const EcDims& d);
PF_INTERNAL int pf_ecp_grid(const EcDims& d, int tpw);
// defined in train_ec_fwd.hip (it asks for the occupancy of ec_fwdp_kernel)
PF_INTERNAL bool pf_ec_persistent_ok(const PfEcTrain* p, const EcDims& d);

namespace {

// ---- the persistent kernels (ec_fwdp_kernel, ec_bwdp_kernel): geometry, DPP row reductions, grid barrier
constexpr int ECP_WAVES = 8, ECP_T = 64 * ECP_WAVES, ECP_TPW = 4;
// Tiles per wave of the narrow units (growth 8 / 16).  They wait 82 - 84 % of their cycles (PMC) with two waves per SIMD; at 2
// tiles per wave they need half the registers (86 - 120 VGPRs) and run as 512 workgroups, two per CU.  Measured (round 5): the
// unit's forward alone 78 -> 102 us (twice the arrivals per barrier, twice the weight staging), and inside the training step -
// where the side stream's kernels hold wave slots and a grid of exactly 2 x 256 workgroups has no slack - barrier time-outs.
// So 4, like the 128-channel units (which at 2 tiles per wave would need 143 - 176 registers: two workgroups do not fit a CU).
constexpr int ECP_TPW_SMALL = 4;
__host__ __device__ constexpr int ecp_tpw(int G) { return G <= 16 ? ECP_TPW_SMALL : ECP_TPW; }
constexpr int ECP_SPIN = 1 << 22;
// timing-only ablations of ec_fwdp_kernel (tools/time_ecunit.py with -DPF_ECP_DBG=mask builds; results are WRONG with any bit set):
// 1 no conv_out, 2 barriers pass at once, 4 no weight staging, 8 no Y stores, 16 no statistics atomics
#ifndef PF_ECP_DBG
#define PF_ECP_DBG 0
#endif

__device__ __forceinline__ float ecp_ald(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ecp_ast(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <int CTRL>
__device__ __forceinline__ float ecp_dppf(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float ecp_rowsum16(float v) {           // sum over the 16 lanes of a DPP row, in every lane
    v += ecp_dppf<0x128>(v); v += ecp_dppf<0x124>(v); v += ecp_dppf<0x122>(v); v += ecp_dppf<0x121>(v);
    return v;
}
__device__ __forceinline__ float ecp_rowmax16(float v) {
    v = fmaxf(v, ecp_dppf<0x128>(v)); v = fmaxf(v, ecp_dppf<0x124>(v)); v = fmaxf(v, ecp_dppf<0x122>(v)); v = fmaxf(v, ecp_dppf<0x121>(v));
    return v;
}
__device__ __forceinline__ int ecp_rowmin16(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false)); v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x124, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x122, 0xf, 0xf, false)); v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x121, 0xf, 0xf, false));
    return v;
}

// grid barrier number `gen` (1, 2, ...) of this launch (pf_grid.h); false when the spin gave up (uniform over the workgroup)
__device__ __forceinline__ bool ecp_barrier(unsigned* sync, unsigned gen, int* flag) {
    if (PF_ECP_DBG & 2) { __syncthreads(); return true; }
    return pf_grid_barrier<ECP_SPIN>(sync, gen, flag);
}

}  // namespace
