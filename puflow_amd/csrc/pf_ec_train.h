// One FeatureExtractUnit (EdgeConv dense block) of the TRAINING step as a handful of launches.
//
// Reference: modules/discrete/interpflow.py:190-248 (FeatureExtractUnit.forward in train() mode: edge feature ->
// [Conv2d 1x1 + BatchNorm2d (batch statistics) + LeakyReLU(0.05), dense concatenation] x nconv -> conv_out -> max over the K
// neighbours) and the autograd backward PyTorch derives from it.  The un-fused path (train_ops.hip, train_gemm.hip + train_perop.py) runs
// this as ~170 launches per unit and step (GEMM, two-pass statistics, apply, concatenations, gradient adds); at
// 32 x 256 points every one of those kernels is shorter than the gap between two launches, so the step was bound by the
// NUMBER of launches.  Here a unit is 7 launches forward and ~12 backward:
//
//   forward   fold        Wp = W1 - W3, Wq = W2 + W3 of all convs -> Wpq [2S, C]   (the edge feature [x_i; x_j; x_j - x_i]
//                         enters every conv only through P = Wp x_i (+ bias) and Q = Wq x_j: packing.fold_edgeconv)
//             gemm        PQ [T, 2S] = x Wpq^T + bias                              (train_gemm.hip: pf_gemm)
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

// sum over the 16 lanes of a DPP row, in every lane
__device__ __forceinline__ float ecp_rowsum16(float v) { return pf_row_reduce(v, PfSum{}); }

// grid barrier number `gen` (1, 2, ...) of this launch (pf_grid.h); false when the spin gave up (uniform over the workgroup)
__device__ __forceinline__ bool ecp_barrier(unsigned* sync, unsigned gen, int* flag) {
    if (PF_ECP_DBG & 2) { __syncthreads(); return true; }
    return pf_grid_barrier<ECP_SPIN>(sync, gen, flag);
}

// ---- the grid-wide column-statistic exchange of one BatchNorm layer, the same in both persistent kernels.  A layer has its own 32
// statistics columns 32 slot .. of the spread double accumulators `acc`, so nothing has to be cleared between two barriers of a
// launch.  The grid barrier between the two halves stays in the kernels (what a kernel does before it differs).
// Publish: lane (col, q) holds sums s0 / s1 over its edges for the channels 16 (b0 + nt) + 4 q + r, of which col0 .. col0 + G - 1
// are the layer's: DPP row sum -> LDS over the waves (red: ECP_WAVES x 64 floats) -> ONE double atomic per column and statistic.
template <int G, int NTG>
__device__ __forceinline__ void ecp_stat_publish(const f4 (&s0)[NTG], const f4 (&s1)[NTG], int b0, int col0, int slot, double* acc,
                                                 float* red, bool atomics) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, q = lane >> 4;
#pragma unroll
    for (int nt = 0; nt < NTG; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float a0 = ecp_rowsum16(s0[nt][r]), a1 = ecp_rowsum16(s1[nt][r]);
            const int c = 16 * (b0 + nt) + 4 * q + r - col0;
            if (col == 0 && c >= 0 && c < G) { red[wave * 64 + c] = a0; red[wave * 64 + 32 + c] = a1; }
        }
    __syncthreads();
    if (atomics && threadIdx.x < 64 && (threadIdx.x & 31) < G) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < ECP_WAVES; ++w) v += red[w * 64 + threadIdx.x];
        unsafeAtomicAdd(acc + (blockIdx.x % STAT_COPIES) * 2 * STAT_W + (threadIdx.x >> 5) * STAT_W + 32 * slot + (threadIdx.x & 31), (double)v);
    }
}
// Fetch (after the barrier): thread (pt = tid & 3, stat = (tid >> 2) & 1, column = tid >> 3) of the first 256 reads 4 of the 16
// copies of one sum (all loads of the workgroup in flight at once), the 4 parts meet through lane shuffles.  `part`: the sum over
// all 16 copies of the thread's statistic of its column, `other`: the other statistic of the same column - the threads with
// (tid & 7) == 0 hold (sum 0, sum 1) of column tid >> 3.
struct EcpSums { double part, other; };
__device__ __forceinline__ EcpSums ecp_stat_fetch(const double* acc, int slot) {
    double part = 0.0;
    if (threadIdx.x < 256) {
        const int pt = threadIdx.x & 3, stt = (threadIdx.x >> 2) & 1, c = threadIdx.x >> 3;
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = PF_LD(acc + (4 * pt + k) * 2 * STAT_W + stt * STAT_W + 32 * slot + c);
        part = pf_xor_sum<1, 2>((v[0] + v[1]) + (v[2] + v[3]));
    }
    return {part, __shfl_xor(part, 4)};
}
// End of the launch: the workgroup that leaves last clears the accumulator columns the `nlayers` layers used and puts the barrier
// words back to zero (every workgroup is past every barrier and has read every sum by then).  `flag`: one int of LDS.
__device__ __forceinline__ void ecp_exit_reset(double* acc, unsigned* sync, int nlayers, int* flag) {
    __syncthreads();
    if (threadIdx.x == 0) *flag = atomicAdd(sync + 2, 1u) == gridDim.x - 1 ? 1 : 0;
    __syncthreads();
    if (*flag == 1) {
        for (int i = threadIdx.x; i < STAT_COPIES * 2 * STAT_W; i += ECP_T)
            if ((i % STAT_W) < 32 * nlayers) PF_ST(acc + i, 0.0);
        if (threadIdx.x == 0) {
            PF_ST(sync + 0, 0u);
            PF_ST(sync + 1, 0u);
            PF_ST(sync + 2, 0u);
        }
    }
}

}  // namespace
