// Vector-Jacobian product of the continuous blocks' ODE right-hand side (csrc/cnf.hip: cnf_eval), the kernel a
// differentiable flow block is built on (puflow_amd/cnf.py: flow_block).  The forward of one evaluation is
//     k = sgn * ( f(t, y), -e^T (df/dy) e )                                      (pf_cnf_rhs's kout)
// and for a cotangent kbar [rows,4] this file computes the gradient of S = sum_rows kbar . k with respect to y, to the
// per-point context terms and to the block's weights - oracle/cnf_ref.py::rhs_vjp with a_y = sgn kbar[:, :3] and
// a_l = sgn kbar[:, 3], which is the checker it is held to (tests/test_gpu_cnf_grad.py).
//
// One launch, per 64-row workgroup tile (four waves, 16 rows = one MFMA column tile each, channels on the MFMA rows):
//   forward   value AND tangent along e through the three ConcatSquash layers (cnf_eval's images: W2 and W3 once more each);
//   reverse   the two adjoint streams (pbar, pdbar of DESIGN 9a) through W3^T (f32 MFMA), W2^T (the split-fp16 image the
//             Hutchinson term already uses; each row's adjoints are scaled to O(1) by a power of two first, because a
//             cotangent has no natural magnitude and the fp16 split has a range) and W1^T;
//   weights   sums of outer products over rows: the factors of a layer are written to LDS row by row and read back as the
//             operands of v_mfma_f32_16x16x4_f32 with the ROWS on the reduction index, D += A^T B.  Every wave owns a
//             16-channel block of each product and keeps its accumulators in registers over ALL tiles of the workgroup
//             (grid-stride loop); the workgroup writes ONE partial slab at its end and a small second kernel adds the slabs
//             in a fixed order into the caller's gradient record (and multiplies the time-coefficient part by t).
// No float atomics anywhere: results are bit-reproducible from run to run.
// The same body also runs as the reverse sweep of a whole recorded integration in one launch (pf_cnf_tape_vjp: bw_sweep<true>).
//
// Rows of a point: rows pt R .. pt R + R - 1 are adjacent.  A wave tile holds floor(16 / R) WHOLE points ((16 / R) R of its
// 16 columns are used - 15 for R = 3), so a point never straddles tiles: its R rows are summed inside the 16-lane row by
// shuffles and the first lane of the point adds into ctxbar as the only writer of that row.  R <= 16.
// Clamped lanes (a partial tile re-reads row rows - 1) get a ZERO cotangent: every adjoint quantity is linear in it, so they
// add nothing to ctxbar, to the weight gradients or anywhere else.
//
// Units: the forward record carries folded constants (2 log2e in W1 | b1, W2, b2 and the tanh layers' bias rows, -log2e in
// the gate rows); everything this file OUTPUTS is in the units of the model's own parameters and pre-activations.
//   ctxbar [T,288]  += the gradients with respect to the hyper networks' outputs (gate pre-activation, bias); layer 3 uses the
//                      FIRST of its four replicated slots only, the other twelve + twelve columns are left alone.
//   grad [4900]     += the weight gradients, then t x this evaluation's column sums of the ctxbar contributions.
// The layouts of the record, the context row (ctxbar's too) and the gradient record: csrc/pf_cnf.h.
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"
#include "pf_mfma.h"
#include "pf_wave.h"
#include "pf_cnf.h"

namespace {

constexpr int BW_NW = 4;                  // waves per workgroup
constexpr int BW_MAX_GRID = 256;          // one workgroup per CU (LDS-bound); also the number of partial slabs
// Row strides of the staged matrices (floats).  bw_atb reads row 4 kk + q, column c0 + col per lane: with strides of 16 mod 64 the
// four q groups of a wave sit 16 banks apart and the 64 lanes of a read hit the 64 LDS banks once each.
constexpr int BW_ST = 80;                 // a staged 64-column stream
constexpr int BW_SS = 16;                 // the two 16-column side matrices

struct BwArgs {
    const float* y;         // [rows,4]
    const float* kbar;      // [rows,4]
    const float* ctx;       // [T,288]
    const float* e;         // [T,3]
    const float* rec;       // CNF_REC floats
    float* ybar;            // [rows,4]
    float* ctxbar;          // [T,288]
    float* slabs;           // [gridDim.x][CNF_GRAD]
    float t, sgn;
    int rows, R, rpt, ntiles;        // rpt: rows of a wave tile = (16 / R) R
};

struct BwTapeArgs {
    const float* states;    // [n_steps][rows][4] state at the start of each recorded step
    const float* steps;     // [n_steps][2] (s, h), solver time
    const float* ctx; const float* e; const float* rec;
    float* ybar;            // [rows,4]  in: cotangent of the final state, out: of states[0]
    float* ctxbar;          // [T,288]
    float* slabs;           // [gridDim.x][CNF_GRAD]
    float sgn;
    int n_steps, rows, R, rpt, ntiles;
};

// Row-local state of the tape sweep in LDS, one f4 per slot and staged row: the stage states Y_1 .. Y_6 (Y_1 = the step's start),
// their cotangents, the cotangent of the step's result.  A row's slots are touched by the four q lanes of its column only - one
// wave - so they need no workgroup barrier, only the wave's program order.
constexpr int BW_RS_Y = 0, BW_RS_YB = 6, BW_RS_Y1B = 12, BW_RS = 13;

// acc += A^T B over the workgroup's 64 staged rows: A [64][sa] columns a0 .. a0 + 15 -> D rows, B [64][sb] columns
// b0 .. b0 + 15 -> D columns.  Lane (col, q): acc[r] = D[4 q + r][col].
__device__ __forceinline__ f4 bw_atb(const float* __restrict__ A, int sa, int a0, const float* __restrict__ B, int sb, int b0,
                                     f4 acc, int col, int q) {
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        const int row = 4 * kk + q;
        acc = pf_mfma(A[row * sa + a0 + col], B[row * sb + b0 + col], acc);
    }
    return acc;
}

// this lane's 16 channels (4 blocks of 16 cb + 4 q .. + 3) of its row into a staged stream
__device__ __forceinline__ void bw_stage(float* __restrict__ S, int lrow, int q, const f4 (&v)[4]) {
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) *reinterpret_cast<f4*>(S + lrow * BW_ST + cb * 16 + 4 * q) = v[cb];
}

// sum over the R adjacent lanes of a point inside the 16-lane row; complete in the point's first lane (pos == 0)
__device__ __forceinline__ f4 bw_point_sum(f4 v, int pos, int R) {
    f4 s = v;
    for (int d = 1; d < R; ++d) {
        f4 o;
        o.x = __shfl_down(v.x, d, 16); o.y = __shfl_down(v.y, d, 16); o.z = __shfl_down(v.z, d, 16); o.w = __shfl_down(v.w, d, 16);
        if (pos + d < R) s += o;
    }
    return s;
}

// power-of-two scale that brings the largest magnitude of a row's adjoints to [1, 2): the split-fp16 product has fp16's range
__device__ __forceinline__ void bw_row_scale(const f4 (&a)[4], const f4 (&b)[4], float& sc, float& inv) {
    float m = 0.f;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmaxf(m, fmaxf(fabsf(a[cb][r]), fabsf(b[cb][r])));
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    int ex = (int)((__builtin_bit_cast(unsigned, m) >> 23) & 0xffu);
    ex = ex < 1 ? 1 : (ex > 253 ? 253 : ex);
    sc = __builtin_bit_cast(float, (unsigned)(254 - ex) << 23);
    inv = __builtin_bit_cast(float, (unsigned)ex << 23);
}

// The body of both kernels.  TAPE = false: one evaluation per tile, (y, kbar, t) from the caller (cnf_rhs_vjp_kernel).
// TAPE = true: per tile the whole recorded integration, last step to first (cnf_tape_vjp_kernel): per step the stage states are
// recomputed from the step's start (f alone: the Hutchinson term never enters a stage STATE's first three columns, and the
// fourth is read by nothing), then for j = 6 .. 1 the evaluation below runs on (Y_j, kbar_j = h b_j y1bar + h sum_{m > j} a_mj
// Ybar_m, sgn (s + alpha_j h)) and leaves Ybar_j in LDS, and y0bar = y1bar + sum_j Ybar_j seeds the step before.  The
// accumulators stay in registers over stages, steps and tiles.  The side matrix Bs carries the evaluation's net time in a column
// of its own, so the time-coefficient sums leave the MFMA already multiplied by THEIR t (the reduction's factor is 1).
template <bool TAPE, class Args>
__device__ __forceinline__ void bw_sweep(const Args& a) {
    __shared__ f4 wl[CNF_REC / 4];
    __shared__ f4 stg4[4 * 64 * BW_ST / 4];          // four staged 64-column streams of the workgroup's 64 rows
    __shared__ f4 side4[2 * 64 * BW_SS / 4];         // Bs = [y 1 | e 0 | t 0 .. (TAPE) | 0 ..] and P3 = [gl3 | gld3 | gate_pre3 | bias_pre3]
    __shared__ f4 rsl[TAPE ? BW_RS * 64 : 1];        // TAPE: the rows' stage states and cotangents
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4;
    // (cnf_stage_weights written out: through the function the views' LDS addresses fold differently and the kernel's stream moves)
    for (int i = threadIdx.x; i < CNF_REC / 4; i += BW_NW * 64) wl[i] = reinterpret_cast<const f4*>(a.rec)[i];
    __syncthreads();
    const float* rec = reinterpret_cast<const float*>(wl);
    const PfW2Lds w2{reinterpret_cast<const u4*>(rec + CNF_W2), lane}, w2t{reinterpret_cast<const u4*>(rec + CNF_W2T), lane},
                  w3{reinterpret_cast<const u4*>(rec + CNF_W3), lane};
    const float* tv = rec + CNF_TV;
    float* stg = reinterpret_cast<float*>(stg4);
    float* S0 = stg; float* S1 = stg + 64 * BW_ST; float* S2 = stg + 2 * 64 * BW_ST; float* S3 = stg + 3 * 64 * BW_ST;
    float* Bs = reinterpret_cast<float*>(side4);
    float* P3 = Bs + 64 * BW_SS;
    const int lrow = wave * 16 + col;                // this lane's row of the staged matrices
    constexpr int TC = TAPE ? 8 : 3;                 // the column of Bs the time-coefficient sums are taken from: t / 1

    // accumulators over all tiles of this workgroup; wave w owns output block w of every product
    f4 aW2[4], aB2 = pf_splat(0.f), aG2 = pf_splat(0.f), aH2 = pf_splat(0.f);       // dW2 rows 16 w .., db2, sum gate_pre2, sum bias_pre2
    f4 aW1a = pf_splat(0.f), aW1b = pf_splat(0.f), aG1 = pf_splat(0.f), aH1 = pf_splat(0.f);
    f4 aW3a = pf_splat(0.f), aW3b = pf_splat(0.f), aS3 = pf_splat(0.f);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) aW2[nb] = pf_splat(0.f);

    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const long long g = (long long)(tile * BW_NW + wave) * a.rpt + col;
        const bool ok = col < a.rpt && g < a.rows;
        const int row = ok ? (int)g : a.rows - 1;
        const int pt = row / a.R;
        const int pos = col % a.R;                                   // position of the row inside its point (ok lanes)
        const float* cx = a.ctx + (size_t)pt * CNF_CTX;
        const float e0 = a.e[(size_t)pt * 3 + 0], e1 = a.e[(size_t)pt * 3 + 1], e2 = a.e[(size_t)pt * 3 + 2];
        const float eb = q == 0 ? e0 : (q == 1 ? e1 : (q == 2 ? e2 : 0.f));

        // one evaluation on this lane's row: ybar -> global memory, or (TAPE) -> the row's slot of stage j
        auto eval = [&](const f4 y, f4 kb, const float t, const int j) __attribute__((always_inline)) {
            if (!ok) kb = pf_splat(0.f);
            const float yb = q == 0 ? y.x : (q == 1 ? y.y : (q == 2 ? y.z : 1.f));

            // ---- forward, layer 1 (3 -> 64): value and tangent.  [W1 | b1] carries 2 log2e.
            f4 h1[4], h1d[4], g1[4];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const int ch = cb * 16 + 4 * q;
                const f4 gc = *reinterpret_cast<const f4*>(cx + CNF_CTX_G1 + ch), bc = *reinterpret_cast<const f4*>(cx + CNF_CTX_B1 + ch);
                const f4 gt = *reinterpret_cast<const f4*>(tv + CNF_CTX_G1 + ch), bt = *reinterpret_cast<const f4*>(tv + CNF_CTX_B1 + ch);
                const float wa = rec[CNF_W1B + (cb * 16 + col) * 4 + q];
                const f4 lin = pf_mfma(wa, yb, pf_splat(0.f)), lind = pf_mfma(wa, eb, pf_splat(0.f));
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float gate = sigm(fmaf(gt[r], t, gc[r]));
                    const float h = tanh_fast(fmaf(lin[r], gate, fmaf(bt[r], t, bc[r])));
                    g1[cb][r] = gate;
                    h1[cb][r] = h;
                    h1d[cb][r] = (1.f - h * h) * (lind[r] * CNF_INV_2LOG2E) * gate;
                }
            }
            // ---- layer 2 (64 -> 64)
            f4 h2[4], h2d[4], g2[4], lin2[4], lind2[4];
            {
                PfPair2 hp[1][2], hpd[1][2];
                hp[0][0] = pf_pair2(h1[0], h1[1]); hp[0][1] = pf_pair2(h1[2], h1[3]);
                hpd[0][0] = pf_pair2(h1d[0], h1d[1]); hpd[0][1] = pf_pair2(h1d[2], h1d[3]);
                f4 a2[1][4], a2d[1][4];
#pragma unroll
                for (int ob = 0; ob < 4; ++ob) { a2[0][ob] = pf_bias(rec + CNF_B2, ob, q); a2d[0][ob] = pf_splat(0.f); }
                pf_mm2f<4, 2, 2>(w2, 0, hp, 0, a2, 0);
                pf_mm2f<4, 2, 2>(w2, 0, hpd, 0, a2d, 0);
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const int ch = cb * 16 + 4 * q;
                    const f4 gc = *reinterpret_cast<const f4*>(cx + CNF_CTX_G2 + ch), bc = *reinterpret_cast<const f4*>(cx + CNF_CTX_B2 + ch);
                    const f4 gt = *reinterpret_cast<const f4*>(tv + CNF_CTX_G2 + ch), bt = *reinterpret_cast<const f4*>(tv + CNF_CTX_B2 + ch);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float gate = sigm(fmaf(gt[r], t, gc[r]));
                        const float h = tanh_fast(fmaf(a2[0][cb][r], gate, fmaf(bt[r], t, bc[r])));
                        g2[cb][r] = gate;
                        h2[cb][r] = h;
                        lin2[cb][r] = a2[0][cb][r] * CNF_INV_2LOG2E;
                        lind2[cb][r] = a2d[0][cb][r] * CNF_INV_2LOG2E;
                        h2d[cb][r] = (1.f - h * h) * lind2[cb][r] * gate;
                    }
                }
            }
            // ---- layer 3 (64 -> 3; every q group holds channels 0..2 in .x .y .z, .w is a zero row)
            f4 g3, lin3, lind3;
            {
                PfPair2 hp[1][2], hpd[1][2];
                hp[0][0] = pf_pair2(h2[0], h2[1]); hp[0][1] = pf_pair2(h2[2], h2[3]);
                hpd[0][0] = pf_pair2(h2d[0], h2d[1]); hpd[0][1] = pf_pair2(h2d[2], h2d[3]);
                f4 a3[1][1], a3d[1][1];
                a3[0][0] = *reinterpret_cast<const f4*>(rec + CNF_B3 + 4 * q);
                a3d[0][0] = pf_splat(0.f);
                pf_mm2f<1, 2, 2>(w3, 0, hp, 0, a3, 0);
                pf_mm2f<1, 2, 2>(w3, 0, hpd, 0, a3d, 0);
                lin3 = a3[0][0]; lind3 = a3d[0][0];
                const f4 gc = *reinterpret_cast<const f4*>(cx + CNF_CTX_G3 + 4 * q), gt = *reinterpret_cast<const f4*>(tv + CNF_CTX_G3 + 4 * q);
#pragma unroll
                for (int r = 0; r < 4; ++r) g3[r] = sigm(fmaf(gt[r], t, gc[r]));
            }

            // ---- reverse, layer 3: seeds fbar = sgn kbar[:3], fdotbar = -sgn kbar[3] e
            const float al = -a.sgn * kb.w;
            const f4 pb3 = {a.sgn * kb.x, a.sgn * kb.y, a.sgn * kb.z, 0.f};
            const f4 pdb3 = {al * e0, al * e1, al * e2, 0.f};
            const f4 gl3 = pb3 * g3, gld3 = pdb3 * g3;
            const f4 gp3 = (pb3 * lin3 + pdb3 * lind3) * g3 * (pf_splat(1.f) - g3);
            f4 xb[4], xdb[4];                                             // adjoints of h2 / its tangent
            {
                const float vb = q == 0 ? gl3.x : (q == 1 ? gl3.y : (q == 2 ? gl3.z : 0.f));
                const float vdb = q == 0 ? gld3.x : (q == 1 ? gld3.y : (q == 2 ? gld3.z : 0.f));
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const float wa = rec[CNF_W3T + (cb * 16 + col) * 4 + q];                 // W3[:, ch] (4th column zero)
                    xb[cb] = pf_mfma(wa, vb, pf_splat(0.f));
                    xdb[cb] = pf_mfma(wa, vdb, pf_splat(0.f));
                }
            }
            // ---- reverse, layer 2
            f4 gl2[4], gld2[4], gp2[4], bp2[4];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float h = h2[cb][r], om = 1.f - h * h, gate = g2[cb][r];
                    const float pdb = om * xdb[cb][r];
                    const float pb = om * (xb[cb][r] - 2.f * h * (lind2[cb][r] * gate) * xdb[cb][r]);
                    bp2[cb][r] = pb;
                    gl2[cb][r] = pb * gate;
                    gld2[cb][r] = pdb * gate;
                    gp2[cb][r] = (pb * lin2[cb][r] + pdb * lind2[cb][r]) * gate * (1.f - gate);
                }

            // ---- weights, first part: dW3 and the layer-3 / layer-2 context sums.  S0 = h2, S1 = h2d, S2 = gate_pre2, S3 = bias_pre2
            __syncthreads();                                             // the previous tile's products are done with the staging
            bw_stage(S0, lrow, q, h2); bw_stage(S1, lrow, q, h2d); bw_stage(S2, lrow, q, gp2); bw_stage(S3, lrow, q, bp2);
            {
                const f4 bs = q == 0 ? (f4){y.x, y.y, y.z, 1.f} : (q == 1 ? (f4){e0, e1, e2, 0.f} : (TAPE && q == 2 ? (f4){t, 0.f, 0.f, 0.f} : pf_splat(0.f)));
                const f4 p3 = q == 0 ? gl3 : (q == 1 ? gld3 : (q == 2 ? gp3 : pb3));
                *reinterpret_cast<f4*>(Bs + lrow * BW_SS + 4 * q) = bs;
                *reinterpret_cast<f4*>(P3 + lrow * BW_SS + 4 * q) = p3;
            }
            __syncthreads();
            aW3a = bw_atb(P3, BW_SS, 0, S0, BW_ST, 16 * wave, aW3a, col, q);
            aW3b = bw_atb(P3, BW_SS, 0, S1, BW_ST, 16 * wave, aW3b, col, q);
            if (wave == 0) aS3 = bw_atb(P3, BW_SS, 0, Bs, BW_SS, 0, aS3, col, q);      // one copy is enough: it covers all 64 rows
            aG2 = bw_atb(S2, BW_ST, 16 * wave, Bs, BW_SS, 0, aG2, col, q);
            aH2 = bw_atb(S3, BW_ST, 16 * wave, Bs, BW_SS, 0, aH2, col, q);

            // ---- ctxbar of layers 2 and 3: sum over the point's rows, its first lane is the only writer
            {
                float* cb_ = a.ctxbar + (size_t)pt * CNF_CTX;
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const f4 sg = bw_point_sum(gp2[cb], pos, a.R), sb = bw_point_sum(bp2[cb], pos, a.R);
                    if (ok && pos == 0) {
                        f4* pg = reinterpret_cast<f4*>(cb_ + CNF_CTX_G2 + cb * 16 + 4 * q);
                        f4* pbias = reinterpret_cast<f4*>(cb_ + CNF_CTX_B2 + cb * 16 + 4 * q);
                        *pg += sg; *pbias += sb;
                    }
                }
                const f4 sg3 = bw_point_sum(gp3, pos, a.R), sb3 = bw_point_sum(pb3, pos, a.R);
                if (ok && pos == 0 && q == 0) {
                    cb_[CNF_CTX_G3] += sg3.x; cb_[CNF_CTX_G3 + 1] += sg3.y; cb_[CNF_CTX_G3 + 2] += sg3.z;
                    cb_[CNF_CTX_B3] += sb3.x; cb_[CNF_CTX_B3 + 1] += sb3.y; cb_[CNF_CTX_B3 + 2] += sb3.z;
                }
            }

            // ---- W2^T on both adjoint streams (rows scaled to O(1) for the fp16 split)
            f4 x1b[4], x1db[4];
            {
                float sc, inv;
                bw_row_scale(gl2, gld2, sc, inv);
                f4 s0[4], s1[4];
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) { s0[cb] = gl2[cb] * sc; s1[cb] = gld2[cb] * sc; }
                PfPair2 wp[1][2], wpd[1][2];
                wp[0][0] = pf_pair2(s0[0], s0[1]); wp[0][1] = pf_pair2(s0[2], s0[3]);
                wpd[0][0] = pf_pair2(s1[0], s1[1]); wpd[0][1] = pf_pair2(s1[2], s1[3]);
                f4 u1[1][4], u1d[1][4];
#pragma unroll
                for (int ob = 0; ob < 4; ++ob) { u1[0][ob] = pf_splat(0.f); u1d[0][ob] = pf_splat(0.f); }
                pf_mm2f<4, 2, 2>(w2t, 0, wp, 0, u1, 0);
                pf_mm2f<4, 2, 2>(w2t, 0, wpd, 0, u1d, 0);
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) { x1b[cb] = u1[0][cb] * inv; x1db[cb] = u1d[0][cb] * inv; }
            }

            // ---- weights, second part: dW2, db2.  S0 = gl2, S1 = gld2, S2 = h1, S3 = h1d
            __syncthreads();
            bw_stage(S0, lrow, q, gl2); bw_stage(S1, lrow, q, gld2); bw_stage(S2, lrow, q, h1); bw_stage(S3, lrow, q, h1d);
            __syncthreads();
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                aW2[nb] = bw_atb(S0, BW_ST, 16 * wave, S2, BW_ST, 16 * nb, aW2[nb], col, q);
                aW2[nb] = bw_atb(S1, BW_ST, 16 * wave, S3, BW_ST, 16 * nb, aW2[nb], col, q);
            }
            aB2 = bw_atb(S0, BW_ST, 16 * wave, Bs, BW_SS, 0, aB2, col, q);

            // ---- reverse, layer 1 (its linear parts recomputed: one f32 MFMA each)
            f4 gl1[4], gld1[4], gp1[4], bp1[4];
            float r0 = 0.f, r1 = 0.f, r2 = 0.f;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const float wa = rec[CNF_W1B + (cb * 16 + col) * 4 + q];
                const f4 lin = pf_mfma(wa, yb, pf_splat(0.f)) * CNF_INV_2LOG2E, lind = pf_mfma(wa, eb, pf_splat(0.f)) * CNF_INV_2LOG2E;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float h = h1[cb][r], om = 1.f - h * h, gate = g1[cb][r];
                    const float pdb = om * x1db[cb][r];
                    const float pb = om * (x1b[cb][r] - 2.f * h * (lind[r] * gate) * x1db[cb][r]);
                    bp1[cb][r] = pb;
                    gl1[cb][r] = pb * gate;
                    gld1[cb][r] = pdb * gate;
                    gp1[cb][r] = (pb * lin[r] + pdb * lind[r]) * gate * (1.f - gate);
                    const f4 wr = *reinterpret_cast<const f4*>(rec + CNF_W1B + (cb * 16 + 4 * q + r) * 4);      // 2 log2e W1[ch, :]
                    r0 = fmaf(wr.x, gl1[cb][r], r0); r1 = fmaf(wr.y, gl1[cb][r], r1); r2 = fmaf(wr.z, gl1[cb][r], r2);
                }
            }
            r0 += __shfl_xor(r0, 16); r1 += __shfl_xor(r1, 16); r2 += __shfl_xor(r2, 16);
            r0 += __shfl_xor(r0, 32); r1 += __shfl_xor(r1, 32); r2 += __shfl_xor(r2, 32);
            if constexpr (TAPE) {
                if (q == 0) rsl[(BW_RS_YB + j) * 64 + lrow] = (f4){r0 * CNF_INV_2LOG2E, r1 * CNF_INV_2LOG2E, r2 * CNF_INV_2LOG2E, 0.f};
            } else {
                if (ok && q == 0) *reinterpret_cast<f4*>(a.ybar + (size_t)row * 4) = (f4){r0 * CNF_INV_2LOG2E, r1 * CNF_INV_2LOG2E, r2 * CNF_INV_2LOG2E, 0.f};
            }

            // ---- weights, third part: dW1 | db1 and the layer-1 context sums.  S0 = gl1, S1 = gld1, S2 = gate_pre1, S3 = bias_pre1
            __syncthreads();
            bw_stage(S0, lrow, q, gl1); bw_stage(S1, lrow, q, gld1); bw_stage(S2, lrow, q, gp1); bw_stage(S3, lrow, q, bp1);
            __syncthreads();
            aW1a = bw_atb(S0, BW_ST, 16 * wave, Bs, BW_SS, 0, aW1a, col, q);
            aW1b = bw_atb(S1, BW_ST, 16 * wave, Bs, BW_SS, 0, aW1b, col, q);
            aG1 = bw_atb(S2, BW_ST, 16 * wave, Bs, BW_SS, 0, aG1, col, q);
            aH1 = bw_atb(S3, BW_ST, 16 * wave, Bs, BW_SS, 0, aH1, col, q);
            {
                float* cb_ = a.ctxbar + (size_t)pt * CNF_CTX;
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const f4 sg = bw_point_sum(gp1[cb], pos, a.R), sb = bw_point_sum(bp1[cb], pos, a.R);
                    if (ok && pos == 0) {
                        f4* pg = reinterpret_cast<f4*>(cb_ + CNF_CTX_G1 + cb * 16 + 4 * q);
                        f4* pbias = reinterpret_cast<f4*>(cb_ + CNF_CTX_B1 + cb * 16 + 4 * q);
                        *pg += sg; *pbias += sb;
                    }
                }
            }
        };  // eval

        if constexpr (!TAPE) {
            eval(*reinterpret_cast<const f4*>(a.y + (size_t)row * 4), *reinterpret_cast<const f4*>(a.kbar + (size_t)row * 4), a.t, 0);
        } else {
            // sgn f(t, y): the value path of the evaluation above (csrc/cnf.hip cnf_eval with its plain gates), for the stage states
            auto value = [&](const f4 y, const float t) __attribute__((always_inline)) {
                const float yb = q == 0 ? y.x : (q == 1 ? y.y : (q == 2 ? y.z : 1.f));
                f4 h1[4], h2[4];
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const int ch = cb * 16 + 4 * q;
                    const f4 gc = *reinterpret_cast<const f4*>(cx + CNF_CTX_G1 + ch), bc = *reinterpret_cast<const f4*>(cx + CNF_CTX_B1 + ch);
                    const f4 gt = *reinterpret_cast<const f4*>(tv + CNF_CTX_G1 + ch), bt = *reinterpret_cast<const f4*>(tv + CNF_CTX_B1 + ch);
                    const f4 lin = pf_mfma(rec[CNF_W1B + (cb * 16 + col) * 4 + q], yb, pf_splat(0.f));
#pragma unroll
                    for (int r = 0; r < 4; ++r) h1[cb][r] = tanh_fast(fmaf(lin[r], sigm(fmaf(gt[r], t, gc[r])), fmaf(bt[r], t, bc[r])));
                }
                PfPair2 hp[1][2];
                hp[0][0] = pf_pair2(h1[0], h1[1]); hp[0][1] = pf_pair2(h1[2], h1[3]);
                f4 a2[1][4];
#pragma unroll
                for (int ob = 0; ob < 4; ++ob) a2[0][ob] = pf_bias(rec + CNF_B2, ob, q);
                pf_mm2f<4, 2, 2>(w2, 0, hp, 0, a2, 0);
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const int ch = cb * 16 + 4 * q;
                    const f4 gc = *reinterpret_cast<const f4*>(cx + CNF_CTX_G2 + ch), bc = *reinterpret_cast<const f4*>(cx + CNF_CTX_B2 + ch);
                    const f4 gt = *reinterpret_cast<const f4*>(tv + CNF_CTX_G2 + ch), bt = *reinterpret_cast<const f4*>(tv + CNF_CTX_B2 + ch);
#pragma unroll
                    for (int r = 0; r < 4; ++r) h2[cb][r] = tanh_fast(fmaf(a2[0][cb][r], sigm(fmaf(gt[r], t, gc[r])), fmaf(bt[r], t, bc[r])));
                }
                hp[0][0] = pf_pair2(h2[0], h2[1]); hp[0][1] = pf_pair2(h2[2], h2[3]);
                f4 a3[1][1];
                a3[0][0] = *reinterpret_cast<const f4*>(rec + CNF_B3 + 4 * q);
                pf_mm2f<1, 2, 2>(w3, 0, hp, 0, a3, 0);
                const f4 gc = *reinterpret_cast<const f4*>(cx + CNF_CTX_G3 + 4 * q), bc = *reinterpret_cast<const f4*>(cx + CNF_CTX_B3 + 4 * q);
                const f4 gt = *reinterpret_cast<const f4*>(tv + CNF_CTX_G3 + 4 * q), bt = *reinterpret_cast<const f4*>(tv + CNF_CTX_B3 + 4 * q);
                f4 dy;
#pragma unroll
                for (int r = 0; r < 4; ++r) dy[r] = a.sgn * fmaf(a3[0][0][r], sigm(fmaf(gt[r], t, gc[r])), fmaf(bt[r], t, bc[r]));
                return dy;
            };
            f4* my = rsl + lrow;                                         // slot s of this lane's row: my[64 s]
            {
                f4 yb1 = *reinterpret_cast<const f4*>(a.ybar + (size_t)row * 4);
                if (!ok) yb1 = pf_splat(0.f);
                if (q == 0) my[64 * BW_RS_Y1B] = yb1;
            }
#pragma unroll 1
            for (int st = a.n_steps - 1; st >= 0; --st) {
                const float s = a.steps[2 * st], h = a.steps[2 * st + 1];
                const f4 y0 = *reinterpret_cast<const f4*>(a.states + ((size_t)st * a.rows + row) * 4);
                // ---- the stage states Y_1 .. Y_6, recomputed from y0 (k_1 too: FSAL is an ordinary dependence on y0)
                f4 k[5], yi = y0;
                pf_static_for<0, 5>([&](auto sc) {
                    constexpr int j = decltype(sc)::value;
                    if (q == 0) my[64 * (BW_RS_Y + j)] = yi;
                    k[j] = value(yi, a.sgn * (j == 0 ? s : s + CNF_AL[j > 0 ? j - 1 : 0] * h));
                    f4 comb = k[0] * CNF_BE[j][0];
#pragma unroll
                    for (int m = 1; m <= j; ++m) comb += k[m] * CNF_BE[j][m];
                    yi = y0 + comb * h;
                });
                if (q == 0) my[64 * (BW_RS_Y + 5)] = yi;
                // ---- stages 6 .. 1: kbar_j = sum_{m > j} (h a_mj) Z_m with Z_7 = y1bar (a_7j = b_j), Z_m = Ybar_m
#pragma unroll 1
                for (int j = 5; j >= 0; --j) {
                    __builtin_amdgcn_wave_barrier();
                    const f4 yj = my[64 * (BW_RS_Y + j)];
                    f4 kb = my[64 * BW_RS_Y1B] * (h * CNF_BE[5][j]);
#pragma unroll 1
                    for (int m = j + 1; m < 6; ++m) kb += my[64 * (BW_RS_YB + m)] * (h * CNF_BE[m - 1][j]);
                    eval(yj, kb, a.sgn * (s + (j == 0 ? 0.f : CNF_AL[j > 0 ? j - 1 : 0]) * h), j);
                }
                // ---- y0bar = y1bar + sum_j Ybar_j (column 3: Ybar's is zero, y1bar's passes through)
                __builtin_amdgcn_wave_barrier();
                f4 nb = my[64 * BW_RS_Y1B];
#pragma unroll
                for (int j = 0; j < 6; ++j) nb += my[64 * (BW_RS_YB + j)];
                __builtin_amdgcn_wave_barrier();
                if (q == 0) my[64 * BW_RS_Y1B] = nb;
                if (st == 0 && ok && q == 0) *reinterpret_cast<f4*>(a.ybar + (size_t)row * 4) = nb;
            }
        }
    }

    // ---- this workgroup's slab, in the gradient record's layout.  Lane (col, q) holds D[4 q + r][col] of its wave's blocks.
    float* sl = a.slabs + (size_t)blockIdx.x * CNF_GRAD;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = 16 * wave + 4 * q + r;                         // output channel of the layer-1 / layer-2 blocks
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) sl[CNF_GRAD_W2 + o * 64 + 16 * nb + col] = aW2[nb][r];
        // dW1[o][j] = (gl1^T y)[o][j] + (gld1^T e)[o][j]: columns j and 4 + j of the two products against Bs; column 3 of a
        // product against Bs is the plain column sum
        const float we = __shfl_down(aW1b[r], 4, 16);
        if (col < 3) sl[CNF_GRAD_W1 + o * 3 + col] = aW1a[r] + we;
        if (col == 3) {
            sl[CNF_GRAD_B1 + o] = aW1a[r];
            sl[CNF_GRAD_B2 + o] = aB2[r];
        }
        if (col == TC) {
            sl[CNF_GRAD_TV + CNF_CTX_G1 + o] = aG1[r]; sl[CNF_GRAD_TV + CNF_CTX_B1 + o] = aH1[r];
            sl[CNF_GRAD_TV + CNF_CTX_G2 + o] = aG2[r]; sl[CNF_GRAD_TV + CNF_CTX_B2 + o] = aH2[r];
        }
        // dW3[j][i] = (gl3^T h2)[j][i] + (gld3^T h2d)[j][i]: D rows j (q = 0) and 4 + j (q = 1) of the two products
        const float w3d = __shfl(aW3b[r], lane + 16);
        if (q == 0 && r < 3) sl[CNF_GRAD_W3 + r * 64 + 16 * wave + col] = aW3a[r] + w3d;
        if (wave == 0 && r < 3) {
            if (col == 3 && q == 0) sl[CNF_GRAD_B3 + r] = aS3[r];
            if (col == TC && q == 2) sl[CNF_GRAD_TV + CNF_CTX_G3 + r] = aS3[r];
            if (col == TC && q == 3) sl[CNF_GRAD_TV + CNF_CTX_B3 + r] = aS3[r];
        }
    }
    if (threadIdx.x < 27) {                  // the words nothing above writes: the unused one and the replicated layer-3 slots (13 + 13)
        const int i = threadIdx.x;                 // 1 .. 13 -> gate3 columns 3 .. 15, 14 .. 26 -> bias3 columns 3 .. 15
        sl[i == 0 ? CNF_GRAD_UNUSED : (i < 14 ? CNF_GRAD_TV + CNF_CTX_G3 + 2 + i : CNF_GRAD_TV + CNF_CTX_B3 - 11 + i)] = 0.f;
    }
}

__global__ __launch_bounds__(BW_NW * 64) void cnf_rhs_vjp_kernel(BwArgs a) { bw_sweep<false>(a); }
__global__ __launch_bounds__(BW_NW * 64) void cnf_tape_vjp_kernel(BwTapeArgs a) { bw_sweep<true>(a); }
// The same sweep with the number of recorded steps taken from the integration's controller row (csrc/cnf.hip: [5] done,
// [6] accepted, [9] status) - a kernel of its own, so that cnf_tape_vjp_kernel keeps its code.  Read once per workgroup and made
// provably wave-uniform: it bounds the step loop.  Not clean, or outside [1, cap]: zero steps - ybar passes through, the slab
// is still written (zeros) for the reduction.
__global__ __launch_bounds__(BW_NW * 64) void cnf_tape_vjp_dev_kernel(BwTapeArgs a, const double* __restrict__ ctl, int cap) {
    int n = (int)ctl[6];
    n = (ctl[5] != 0.0 && ctl[9] == 0.0 && n >= 1 && n <= cap) ? n : 0;
    BwTapeArgs b = a;
    b.n_steps = __builtin_amdgcn_readfirstlane(n);
    bw_sweep<true>(b);
}

// grad[i] += (i in the time-coefficient part ? t : 1) x sum of the slabs.  32 outputs per workgroup, eight threads per output take
// every eighth slab each (eight loads in flight per output instead of one thread walking all slabs), then the eight partial
// sums are added in a fixed order: the same bits from run to run.
__global__ __launch_bounds__(256) void cnf_rhs_vjp_reduce_kernel(const float* __restrict__ slabs, int n, float t, float* __restrict__ grad) {
    __shared__ float part[8][32];
    const int o = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + o;
    float s = 0.f;
    if (i < CNF_GRAD)
        for (int j = g; j < n; j += 8) s += slabs[(size_t)j * CNF_GRAD + i];
    part[g][o] = s;
    __syncthreads();
    if (g == 0 && i < CNF_GRAD) {
        float tot = part[0][o];
#pragma unroll
        for (int k = 1; k < 8; ++k) tot += part[k][o];
        grad[i] += i >= CNF_GRAD_TV ? t * tot : tot;
    }
}

inline int bw_grid(int rows, int R, int* rpt, int* ntiles) {
    *rpt = (16 / R) * R;
    const long long wt = ((long long)rows + *rpt - 1) / *rpt;        // wave tiles
    *ntiles = (int)((wt + BW_NW - 1) / BW_NW);
    return *ntiles < BW_MAX_GRID ? *ntiles : BW_MAX_GRID;
}

}  // namespace

extern "C" long long pf_cnf_rhs_vjp_workspace_bytes(int rows, int R) {
    if (rows <= 0 || R <= 0 || R > 16 || rows % R != 0) return PF_ERR_SHAPE;
    int rpt, ntiles;
    return (long long)bw_grid(rows, R, &rpt, &ntiles) * CNF_GRAD * (long long)sizeof(float);
}

extern "C" int pf_cnf_rhs_vjp(const float* y, const float* kbar, float t, float sgn, const float* ctx, const float* e,
                              const float* rec, float* ybar, float* ctxbar, float* grad, int rows, int R, void* ws,
                              void* stream) {
    if (!y || !kbar || !ctx || !e || !rec || !ybar || !ctxbar || !grad || !ws) return PF_ERR_NULL;
    if (rows <= 0 || R <= 0 || R > 16 || rows % R != 0) return PF_ERR_SHAPE;
    BwArgs a{};
    a.y = y; a.kbar = kbar; a.ctx = ctx; a.e = e; a.rec = rec; a.ybar = ybar; a.ctxbar = ctxbar; a.slabs = (float*)ws;
    a.t = t; a.sgn = sgn; a.rows = rows; a.R = R;
    const int grid = bw_grid(rows, R, &a.rpt, &a.ntiles);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cnf_rhs_vjp_kernel, dim3(grid), dim3(BW_NW * 64), 0, s, a);
    hipLaunchKernelGGL(cnf_rhs_vjp_reduce_kernel, dim3((CNF_GRAD + 31) / 32), dim3(256), 0, s, (const float*)ws, grid, t, grad);
    return pf_last_launch_status();
}

extern "C" long long pf_cnf_tape_vjp_workspace_bytes(int rows, int R) { return pf_cnf_rhs_vjp_workspace_bytes(rows, R); }

extern "C" int pf_cnf_tape_vjp(const float* states, const float* steps, int n_steps, float sgn, const float* ctx, const float* e,
                               const float* rec, float* ybar, float* ctxbar, float* grad, int rows, int R, void* ws, void* stream) {
    if (!states || !steps || !ctx || !e || !rec || !ybar || !ctxbar || !grad || !ws) return PF_ERR_NULL;
    if (rows <= 0 || R <= 0 || R > 16 || rows % R != 0 || n_steps <= 0) return PF_ERR_SHAPE;
    BwTapeArgs a{};
    a.states = states; a.steps = steps; a.ctx = ctx; a.e = e; a.rec = rec; a.ybar = ybar; a.ctxbar = ctxbar; a.slabs = (float*)ws;
    a.sgn = sgn; a.n_steps = n_steps; a.rows = rows; a.R = R;
    const int grid = bw_grid(rows, R, &a.rpt, &a.ntiles);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cnf_tape_vjp_kernel, dim3(grid), dim3(BW_NW * 64), 0, s, a);
    // every evaluation's time-coefficient share left the kernel multiplied by its own t: the reduction's factor is 1
    hipLaunchKernelGGL(cnf_rhs_vjp_reduce_kernel, dim3((CNF_GRAD + 31) / 32), dim3(256), 0, s, (const float*)ws, grid, 1.f, grad);
    return pf_last_launch_status();
}

// pf_cnf_tape_vjp for a tape recorded without a look at the controller: the step count is ctl[6] of the integration's controller
// row, read on the device; states / steps are the whole tape of `cap` steps (include/puflow_hip.h).
extern "C" int pf_cnf_tape_vjp_dev(const float* states, const float* steps, const double* ctl, int cap, float sgn, const float* ctx,
                                   const float* e, const float* rec, float* ybar, float* ctxbar, float* grad, int rows, int R,
                                   void* ws, void* stream) {
    if (!states || !steps || !ctl || !ctx || !e || !rec || !ybar || !ctxbar || !grad || !ws) return PF_ERR_NULL;
    if (rows <= 0 || R <= 0 || R > 16 || rows % R != 0 || cap <= 0) return PF_ERR_SHAPE;
    BwTapeArgs a{};
    a.states = states; a.steps = steps; a.ctx = ctx; a.e = e; a.rec = rec; a.ybar = ybar; a.ctxbar = ctxbar; a.slabs = (float*)ws;
    a.sgn = sgn; a.n_steps = 0; a.rows = rows; a.R = R;
    const int grid = bw_grid(rows, R, &a.rpt, &a.ntiles);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cnf_tape_vjp_dev_kernel, dim3(grid), dim3(BW_NW * 64), 0, s, a, ctl, cap);
    hipLaunchKernelGGL(cnf_rhs_vjp_reduce_kernel, dim3((CNF_GRAD + 31) / 32), dim3(256), 0, s, (const float*)ws, grid, 1.f, grad);
    return pf_last_launch_status();
}
