// The continuous blocks' ODE right-hand side and the six stages of a Dormand-Prince attempt, shared by the adaptive step
// kernels (csrc/cnf.hip) and the fixed-schedule replay (csrc/cnf_replay.hip): one definition, so both sources compile the same
// arithmetic.  Layouts, activations and tableau: csrc/pf_cnf.h.  Device only.
#pragma once
#include <hip/hip_runtime.h>
#include "pf_mfma.h"
#include "pf_cnf.h"

// SPLIT (cnf_step_dev_kernel, context rows in LDS): the gates depend on (point, channel, stage time) only, and
// 2^(gt (t + alpha h) + gc) = 2^(gt t + gc) x 2^(gt alpha h).  The first factor is computed ONCE per point and tile into the
// context rows' gate slots (shared by the point's R rows and the step's six evaluations), the second once per launch into a
// [stage][channel] table `tvg` points at: a gate is fma + v_rcp_f32, without the v_exp_f32 (36 of an evaluation's 135
// quarter-rate transcendentals, on a kernel the PMC counters show VALU-bound).
// COMPACT (the forward pass's step kernel, R = 1: 64 points per tile, whose full context rows would not fit in LDS): cx / tvg hold
// only the CNF_GATES gate columns, layer after layer (pf_cnf.h: compact gate row); the bias columns come from cxb (the
// row in global memory, the full 288-column layout).
// One evaluation for this lane's row: k = sgn * (f(t, y), -e^T (df/dy) e).  All four q groups of a column return the same f4.
template <bool SPLIT = false, bool COMPACT = false>
__device__ __forceinline__ f4 cnf_eval(const CnfW& w, int q, f4 y, float t, float sgn, const float* __restrict__ cx,
                                       float e0, float e1, float e2, const float* __restrict__ tvg = nullptr,
                                       const float* __restrict__ cxb = nullptr) {
    const float* rec = w.rec;
    const float* tv = rec + CNF_TV;
    if (!SPLIT) tvg = tv;
    if (!COMPACT) cxb = cx;
    constexpr int G1 = COMPACT ? 0 : CNF_CTX_G1, G2 = COMPACT ? CNF_GATE_G2 : CNF_CTX_G2, G3 = COMPACT ? CNF_GATE_G3 : CNF_CTX_G3;
    auto gatef = [](float gt, float tt, float gc) {
        return SPLIT ? __builtin_amdgcn_rcpf(fmaf(gc, gt, 1.f)) : sigm(fmaf(gt, tt, gc));
    };
    const int col = threadIdx.x & 15;
    // ---- layer 1 (3 -> 64): this lane's channels 16 cb + 4 q + r.  W1 y + b1 is ONE v_mfma_f32_16x16x4_f32 per 16 channels
    // ([W1 | b1] x [y; 1]: k = 3 carries the bias) instead of 16 x (an LDS row + 3 fmas) on a VALU that PMC shows ~90 % busy
    // (profiles/r4_cnf/: 50 M VALU wave-instructions per step launch on 1024 SIMDs)
    const float yb = q == 0 ? y.x : (q == 1 ? y.y : (q == 2 ? y.z : 1.f));
    f4 h1[1][4], g1[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        const int ch = cb * 16 + 4 * q;
        const f4 gc = *reinterpret_cast<const f4*>(cx + G1 + ch), bc = *reinterpret_cast<const f4*>(cxb + CNF_CTX_B1 + ch);
        const f4 gt = *reinterpret_cast<const f4*>(tvg + G1 + ch), bt = *reinterpret_cast<const f4*>(tv + CNF_CTX_B1 + ch);
        const f4 lin4 = pf_mfma(rec[CNF_W1B + (cb * 16 + col) * 4 + q], yb, pf_splat(0.f));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float lin = lin4[r];
            const float gate = gatef(gt[r], t, gc[r]);
            g1[cb][r] = gate;
            h1[0][cb][r] = tanh_fast(fmaf(lin, gate, fmaf(bt[r], t, bc[r])));
        }
    }
    // ---- layer 2 (64 -> 64)
    f4 h2[1][4], g2[4];
    {
        PfPair2 hp[1][2];
        hp[0][0] = pf_pair2(h1[0][0], h1[0][1]);
        hp[0][1] = pf_pair2(h1[0][2], h1[0][3]);
        f4 a2[1][4];
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) a2[0][ob] = pf_bias(rec + CNF_B2, ob, q);
        pf_mm2f<4, 2, 2>(w.w2, 0, hp, 0, a2, 0);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const int ch = cb * 16 + 4 * q;
            const f4 gc = *reinterpret_cast<const f4*>(cx + G2 + ch), bc = *reinterpret_cast<const f4*>(cxb + CNF_CTX_B2 + ch);
            const f4 gt = *reinterpret_cast<const f4*>(tvg + G2 + ch), bt = *reinterpret_cast<const f4*>(tv + CNF_CTX_B2 + ch);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float gate = gatef(gt[r], t, gc[r]);
                g2[cb][r] = gate;
                h2[0][cb][r] = tanh_fast(fmaf(a2[0][cb][r], gate, fmaf(bt[r], t, bc[r])));
            }
        }
    }
    // ---- layer 3 (64 -> 3; rows replicated: every q group holds channels 0..2 in .x .y .z)
    f4 dy, g3;
    {
        PfPair2 hp[1][2];
        hp[0][0] = pf_pair2(h2[0][0], h2[0][1]);
        hp[0][1] = pf_pair2(h2[0][2], h2[0][3]);
        f4 a3[1][1];
        a3[0][0] = *reinterpret_cast<const f4*>(rec + CNF_B3 + 4 * q);
        pf_mm2f<1, 2, 2>(w.w3, 0, hp, 0, a3, 0);
        const f4 gc = *reinterpret_cast<const f4*>(cx + G3 + 4 * q), bc = *reinterpret_cast<const f4*>(cxb + CNF_CTX_B3 + 4 * q);
        const f4 gt = *reinterpret_cast<const f4*>(tvg + G3 + 4 * q), bt = *reinterpret_cast<const f4*>(tv + CNF_CTX_B3 + 4 * q);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            g3[r] = gatef(gt[r], t, gc[r]);
            dy[r] = fmaf(a3[0][0][r], g3[r], fmaf(bt[r], t, bc[r]));
        }
    }
    // ---- Hutchinson term e^T J e by the vector-Jacobian product of e through the three layers
    const float v0 = e0 * g3.x, v1 = e1 * g3.y, v2 = e2 * g3.z;
    const float vb = q == 0 ? v0 : (q == 1 ? v1 : (q == 2 ? v2 : 0.f));       // W3^T v as one f32 MFMA per 16 channels, like layer 1
    f4 w2v[1][4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        const f4 u4 = pf_mfma(rec[CNF_W3T + (cb * 16 + col) * 4 + q], vb, pf_splat(0.f));               // W3[:, ch] (4th column zero)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float hh = h2[0][cb][r];
            w2v[0][cb][r] = u4[r] * (1.f - hh * hh) * g2[cb][r];
        }
    }
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
    {
        PfPair2 wp[1][2];
        wp[0][0] = pf_pair2(w2v[0][0], w2v[0][1]);
        wp[0][1] = pf_pair2(w2v[0][2], w2v[0][3]);
        f4 u1[1][4];
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) u1[0][ob] = pf_splat(0.f);
        pf_mm2f<4, 2, 2>(w.w2t, 0, wp, 0, u1, 0);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float hh = h1[0][cb][r];
                const float w1v = u1[0][cb][r] * (1.f - hh * hh) * g1[cb][r];
                const f4 wr = *reinterpret_cast<const f4*>(rec + CNF_W1B + (cb * 16 + 4 * q + r) * 4);  // W1[ch, :]
                r0 = fmaf(wr.x, w1v, r0); r1 = fmaf(wr.y, w1v, r1); r2 = fmaf(wr.z, w1v, r2);
            }
    }
    // sum over the 4 q groups of the column (lanes col, col+16, col+32, col+48)
    // (the three sums interleaved, written out: one after the other they cost the step kernels their instruction streams)
    r0 += __shfl_xor(r0, 16); r1 += __shfl_xor(r1, 16); r2 += __shfl_xor(r2, 16);
    r0 += __shfl_xor(r0, 32); r1 += __shfl_xor(r1, 32); r2 += __shfl_xor(r2, 32);
    // (the W1 rows of the record carry the forward's 2 log2e: taken out of the three sums here)
    const float div = fmaf(r2, e2, fmaf(r1, e1, r0 * e0)) * CNF_INV_2LOG2E;
    return (f4){sgn * dy.x, sgn * dy.y, sgn * dy.z, -sgn * div};
}

// The six stages of one Dormand-Prince attempt from y0 with k[0] = f0 given: fills k[1 .. 6], leaves the step's solution in yi
// and returns the embedded error estimate.  Net time of stage s: tsign * (t + alpha_s h); stf: [stage][TW] gate factors (SPLIT).
template <bool SPLIT, bool COMPACT, int TW>
__device__ __forceinline__ f4 cnf_dopri_stages(const CnfW& w, int q, f4 y0, f4 (&k)[7], f4& yi, float t, float h, float sgn, float tsign,
                                               const float* cx, float e0, float e1, float e2, const float* stf, const float* cxb) {
    pf_static_for<0, 6>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        f4 comb = k[0] * CNF_BE[s][0];
#pragma unroll
        for (int j = 1; j <= s; ++j) comb += k[j] * CNF_BE[s][j];
        yi = y0 + comb * h;
        k[s + 1] = cnf_eval<SPLIT, COMPACT>(w, q, yi, tsign * (t + CNF_AL[s] * h), sgn, cx, e0, e1, e2, stf + s * TW, cxb);
    });
    return cnf_comb7(k, CNF_CE) * h;
}
