// =====================================================================================================================
// BatchNorm MLPs of the interpolation module in the training step: DistanceEncoder and WeightEstimationUnit
// (modules/discrete/interpflow.py:85-151: Conv2d 1x1 + BatchNorm2d + LeakyReLU(0.01), twice, then Conv2d 1x1) on the
// [B N K, C] edge rows.  Same construction as the EdgeConv unit (pf_ec_train.h), minus the neighbour gather: a layer's kernel applies
// the PREVIOUS layer's BatchNorm + LeakyReLU on load, stores its own pre-BatchNorm output and leaves the column sums in the
// epilogue (finalised by the last workgroup); the backward forms BatchNorm-backward on load.  The weight unit's input
// cat[d, feat] (256 wide) is never built: the first layer runs as two K-passes over the two tensors.
// =====================================================================================================================
#include "pf_train_stat.h"

namespace {

struct BnlFwdArgs {
    const float* addA; const float* addB;      // both non-NULL: no product at all - out = addA + addB ([rows, nout] each), statistics as usual
    const float* X; int ldx, kin;              // input rows [rows, ldx], kin <= 128 columns used
    const float* sc; const float* sh;          // BatchNorm scale / shift of the producing layer (nullable: raw input)
    float slope;
    const float* W; int ldw;                   // W[c * ldw + u], c < nout, u < kin (already offset to this K-slice)
    const float* bias;                         // nullable
    float* out; int nout;                      // [rows, nout]
    int accum;                                 // out += (second K-pass)
    int rows, ntiles;
    int want_stats;
    StatFin fin;
};

template <int NT, bool SUM2 = false>
__global__ __launch_bounds__(256) void bnl_fwd_kernel(BnlFwdArgs a) {
    extern __shared__ float lds[];
    __shared__ float red[8 * STAT_W];
    const int kin16 = (a.kin + 15) & ~15, kp = kin16 + 4, KS = kin16 / 16;
    float* Wl = lds;
    float* al = lds + NT * 16 * kp;
    float* bl = al + kin16;
    constexpr bool sum2 = SUM2;                                   // its own instantiation: out = addA + addB, no weights, no product
    for (int c = threadIdx.x >> 4; c < NT * 16 && !sum2; c += 16) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int u = (threadIdx.x & 15) + 16 * k;
            v[k] = (u < kin16 && c < a.nout && u < a.kin) ? a.W[(size_t)c * a.ldw + u] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int u = (threadIdx.x & 15) + 16 * k;
            if (u < kin16) Wl[c * kp + u] = v[k];
        }
    }
    for (int i = threadIdx.x; i < kin16; i += 256) {
        al[i] = i < a.kin ? (a.sc ? a.sc[i] : 1.f) : 0.f;
        bl[i] = (i < a.kin && a.sh) ? a.sh[i] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, q = lane >> 4;
    const bool vec = (a.kin & 3) == 0 && (a.ldx & 3) == 0;
    const float slope = a.sc ? a.slope : 1.f;                     // raw input: identity
    float s0[NT], s1[NT], bv[NT], piv[NT];                      // piv: centred statistics, see ec_fwd_kernel
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        s0[nt] = s1[nt] = 0.f;
        const int col = nt * 16 + row;
        bv[nt] = (a.bias && col < a.nout) ? a.bias[col] : 0.f;
        piv[nt] = (a.want_stats && a.fin.run_mean && col < a.nout) ? a.fin.run_mean[col] : 0.f;
    }
    // Not prefetched: the NEXT tile's rows in flight while this one is multiplied (a wave has ~2 tiles at the bench shape and
    // pays one memory latency for each) was MEASURED NEGATIVE (round 5, same box, whole step): 4.592 vs 4.557 ms - 32 more
    // registers take the 128-wide shape from 3 to 2 waves per SIMD, and the branch runs beside the main chain anyway
    auto loadx = [&](int tile, f4 (&xv_)[8]) {
        const int rr = min(tile * 16 + row, a.rows - 1);
        const float* xrow = a.X + (size_t)rr * a.ldx;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            xv_[ks] = pf_splat(0.f);
            const int u = ks * 16 + 4 * q;
            if (ks < KS && u < a.kin) {
                if (vec) xv_[ks] = *reinterpret_cast<const f4*>(xrow + u);
                else {
#pragma unroll
                    for (int w = 0; w < 4; ++w)
                        if (u + w < a.kin) xv_[ks][w] = xrow[u + w];
                }
            }
        }
    };
    const int tstep = gridDim.x * 4;
    for (int tile = blockIdx.x * 4 + wave; tile < a.ntiles; tile += tstep) {
        const int r0 = tile * 16;
        f4 xv[8];
        if (!sum2) loadx(tile, xv);
        f4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = pf_splat(0.f);
        if (sum2) {                                               // the accumulator layout read straight from the two tensors
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = nt * 16 + row;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rw = r0 + 4 * q + r;
                    if (col < a.nout && rw < a.rows) acc[nt][r] = a.addA[(size_t)rw * a.nout + col] + a.addB[(size_t)rw * a.nout + col];
                }
            }
        }
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            if (ks < KS && !sum2) {
                const int u = ks * 16 + 4 * q;
                const f4 av = lrelu4(xv[ks] * *reinterpret_cast<const f4*>(al + u) + *reinterpret_cast<const f4*>(bl + u), slope);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[nt] = mfma4(av, *reinterpret_cast<const f4*>(Wl + (nt * 16 + row) * kp + u), acc[nt]);
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = nt * 16 + row;
            if (col < a.nout) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rw = r0 + 4 * q + r;
                    if (rw < a.rows) {
                        float* op = a.out + (size_t)rw * a.nout + col;
                        float v = acc[nt][r] + bv[nt];
                        if (a.accum) v += *op;
                        *op = v;
                        const float vc = v - piv[nt];
                        s0[nt] += vc; s1[nt] = fmaf(vc, vc, s1[nt]);
                    }
                }
            }
        }
    }
    if (a.want_stats) stat_flush<NT>(s0, s1, 0, a.nout, a.fin, red);
}

// out = addA + addB ([rows, nout], nout = 16 NT) with the column statistics of the sum (PF_BNMLP_SUM_INPUTS): a streaming kernel -
// float4 per thread along the row, the column sums kept per thread over its rows, added over the workgroup's row groups through
// LDS and handed to stat_flush in the accumulator layout it expects (wave 0, the q = 0 lanes).  (The first version read the sum
// in the MFMA accumulator layout of bnl_fwd_kernel - 4-byte loads, 16 rows apart: 105 us for 100 MB.)
template <int NT>
__global__ __launch_bounds__(256) void bnl_sum_kernel(BnlFwdArgs a) {
    constexpr int C = 16 * NT, C4 = C / 4, RPP = 256 / C4;             // threads per row, rows per pass
    static_assert(256 % C4 == 0 && C4 <= 256, "shape");
    __shared__ float red[8 * STAT_W];
    __shared__ float part[2][RPP][C];
    const int c4 = threadIdx.x % C4, rr = threadIdx.x / C4;
    f4 piv = pf_splat(0.f);
    if (a.want_stats && a.fin.run_mean) piv = *reinterpret_cast<const f4*>(a.fin.run_mean + 4 * c4);
    f4 s0 = pf_splat(0.f), s1 = pf_splat(0.f);
    const long long step = (long long)gridDim.x * RPP;
    long long row = (long long)blockIdx.x * RPP + rr;
    for (; row + 3 * step < a.rows; row += 4 * step) {                     // eight loads in flight per thread
        f4 x[4], y[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            x[u] = *reinterpret_cast<const f4*>(a.addA + (row + u * step) * C + 4 * c4);
            y[u] = *reinterpret_cast<const f4*>(a.addB + (row + u * step) * C + 4 * c4);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const f4 v = x[u] + y[u];
            *reinterpret_cast<f4*>(a.out + (row + u * step) * C + 4 * c4) = v;
            const f4 vc = v - piv;
            s0 += vc; s1 += vc * vc;
        }
    }
    for (; row < a.rows; row += step) {
        const f4 v = *reinterpret_cast<const f4*>(a.addA + row * C + 4 * c4) + *reinterpret_cast<const f4*>(a.addB + row * C + 4 * c4);
        *reinterpret_cast<f4*>(a.out + row * C + 4 * c4) = v;
        const f4 vc = v - piv;
        s0 += vc; s1 += vc * vc;
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) { part[0][rr][4 * c4 + w] = s0[w]; part[1][rr][4 * c4 + w] = s1[w]; }
    __syncthreads();
    float t0[NT], t1[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        t0[nt] = t1[nt] = 0.f;
        if (threadIdx.x < 16) {                                           // wave 0, q = 0: column nt * 16 + lane
            const int c = nt * 16 + threadIdx.x;
            for (int g = 0; g < RPP; ++g) { t0[nt] += part[0][g][c]; t1[nt] += part[1][g][c]; }
        }
    }
    if (a.want_stats) stat_flush<NT>(t0, t1, 0, a.nout, a.fin, red);
}

// backward through one layer.  SRC 1: dy [rows, kin] dense (the last layer, or a later K-pass of an already converted buffer);
// SRC 2: dy = BatchNorm + LeakyReLU backward of dbuf (gradient wrt the layer's ACTIVATED output), formed on load and stored
// back in place.  dx [rows, nout] = dy W (nullable: conversion only); epilogue: BatchNorm-backward sums of the layer that
// produced this layer's input (pre-BN values xpre, constants aff_prev), when that layer has one.
struct BnlBwdArgs {
    const float* dy;
    float* dbuf; const float* ypre; const float* aff; const float* coef;
    int kin; float slope;
    const float* W; int ldw;                   // W[c * ldw + u], c < kin, u < nout
    float* dx; int nout;
    const float* xpre; const float* aff_prev; int want_stats;
    int rows, ntiles;
    StatFin fin;
};

template <int NT, int SRC>
__global__ __launch_bounds__(256) void bnl_bwd_kernel(BnlBwdArgs a) {
    extern __shared__ float lds[];
    __shared__ float red[8 * STAT_W];
    const int kin16 = (a.kin + 15) & ~15, kp = kin16 + 4, KS = kin16 / 16;
    float* Wt = lds;                                   // Wt[u][c]
    float* cf = lds + NT * 16 * kp;                    // SRC 2: [6][kin16]
    if (a.dx)
        for (int c = threadIdx.x >> 4; c < kin16; c += 16) {
            float v[NT];
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                const int u = (threadIdx.x & 15) + 16 * k;
                v[k] = (c < a.kin && u < a.nout) ? a.W[(size_t)c * a.ldw + u] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < NT; ++k) Wt[((threadIdx.x & 15) + 16 * k) * kp + c] = v[k];
        }
    if (SRC == 2) {
        for (int i = threadIdx.x; i < kin16; i += 256) {
            const bool ok = i < a.kin;
#pragma unroll
            for (int w = 0; w < 4; ++w) cf[w * kin16 + i] = ok ? a.aff[w * a.kin + i] : 0.f;
            cf[4 * kin16 + i] = ok ? a.coef[i] : 0.f;
            cf[5 * kin16 + i] = ok ? a.coef[a.kin + i] : 0.f;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, q = lane >> 4;
    float s0[NT], s1[NT], ssc[NT], ssh[NT], smu[NT], srs[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        s0[nt] = s1[nt] = 0.f;
        const int col = nt * 16 + row;
        const bool ok = a.want_stats && col < a.nout;
        ssc[nt] = ok ? a.aff_prev[col] : 0.f;
        ssh[nt] = ok ? a.aff_prev[a.nout + col] : 0.f;
        smu[nt] = ok ? a.aff_prev[2 * a.nout + col] : 0.f;
        srs[nt] = ok ? a.aff_prev[3 * a.nout + col] : 0.f;
    }
    for (int tile = blockIdx.x * 4 + wave; tile < a.ntiles; tile += gridDim.x * 4) {
        const int r0 = tile * 16;
        const int rr = min(r0 + row, a.rows - 1);
        const bool rok = r0 + row < a.rows;
        f4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = pf_splat(0.f);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            if (ks < KS) {
                const int c = ks * 16 + 4 * q;
                f4 av = pf_splat(0.f);
                if (c < a.kin && rok) {
                    if (SRC == 1) av = *reinterpret_cast<const f4*>(a.dy + (size_t)rr * a.kin + c);
                    else {
                        float* dp = a.dbuf + (size_t)rr * a.kin + c;
                        const f4 d = *reinterpret_cast<const f4*>(dp);
                        const f4 y = *reinterpret_cast<const f4*>(a.ypre + (size_t)rr * a.kin + c);
                        const f4 sc = *reinterpret_cast<const f4*>(cf + c), sh = *reinterpret_cast<const f4*>(cf + kin16 + c);
                        const f4 mu = *reinterpret_cast<const f4*>(cf + 2 * kin16 + c), rs = *reinterpret_cast<const f4*>(cf + 3 * kin16 + c);
                        const f4 m1 = *reinterpret_cast<const f4*>(cf + 4 * kin16 + c), m2 = *reinterpret_cast<const f4*>(cf + 5 * kin16 + c);
                        const f4 z = y * sc + sh;
                        const f4 xh = (y - mu) * rs;
#pragma unroll
                        for (int w = 0; w < 4; ++w) {
                            const float dz = d[w] * (z[w] > 0.f ? 1.f : a.slope);
                            av[w] = sc[w] * (dz - m1[w] - xh[w] * m2[w]);
                        }
                        *reinterpret_cast<f4*>(dp) = av;
                    }
                }
                if (a.dx)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[nt] = mfma4(av, *reinterpret_cast<const f4*>(Wt + (nt * 16 + row) * kp + c), acc[nt]);
            }
        }
        if (a.dx)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = nt * 16 + row;
                if (col < a.nout) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rw = r0 + 4 * q + r;
                        if (rw < a.rows) {
                            const float v = acc[nt][r];
                            a.dx[(size_t)rw * a.nout + col] = v;
                            if (a.want_stats) {
                                const float y = a.xpre[(size_t)rw * a.nout + col];
                                const float dz = v * (fmaf(y, ssc[nt], ssh[nt]) > 0.f ? 1.f : a.slope);
                                s0[nt] += dz;
                                s1[nt] = fmaf(dz, (y - smu[nt]) * srs[nt], s1[nt]);
                            }
                        }
                    }
                }
            }
    }
    if (a.want_stats) stat_flush<NT>(s0, s1, 0, a.nout, a.fin, red);
}

// part[chunk][c][u] = sum over the chunk's rows of dy[row, c] * act(X[row, u]) (c < RA, u < RB), bpart[chunk][c] = sum dy
constexpr int BNL_EB = 32;                          // rows per staged block of bnl_dw_kernel
struct BnlDwArgs {
    const float* dy; int RA;                   // [rows, RA]
    const float* X; int ldx, RB;               // [rows, ldx], RB columns used
    const float* sc; const float* sh; float slope;
    int rows, chunk;
    float* part; float* bpart;                 // [nchunk][RA16][RB16], [nchunk][RA16]
};
// one staged 32-row block for a wave that owns NS output tiles; SAME: consecutive row tiles of ONE column tile (one B read per
// k step).  Every operand read of a k step is issued before its MFMAs, through one LDS address per tile with the k step as an
// immediate offset (round 5: see mlp_dw_kernel in train_mlp.hip - with lane-dependent tile lists and run-time LDS strides hipcc
// kept an address register per (k step, tile) read and waited for one LDS read per MFMA)
constexpr int BNL_LD = 144;                         // LDS row stride of the staged blocks: >= 128 columns, = 16 (mod 32) floats
constexpr int BNL_DW_WAVES = 8, BNL_DW_T = 64 * BNL_DW_WAVES, BNL_DW_SLOTS = 8;     // <= 64 output tiles over 8 waves
template <int NS, bool SAME>
__device__ __forceinline__ void bnl_dw_block(const float* ar0, const float* br0, const int (&rts)[BNL_DW_SLOTS],
                                             const int (&cts)[BNL_DW_SLOTS], f4 (&acc)[BNL_DW_SLOTS]) {
    const float* ap[NS];
    const float* bp[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) { ap[s] = ar0 + rts[s] * 16; bp[s] = br0 + cts[SAME ? 0 : s] * 16; }
#pragma unroll
    for (int ks = 0; ks < BNL_EB / 4; ++ks) {
        float av[NS], bv[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            av[s] = ap[s][4 * ks * BNL_LD];
            bv[s] = (SAME && s > 0) ? bv[0] : bp[s][4 * ks * BNL_LD];
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[s] = pf_mfma(av[s], bv[s], acc[s]);
    }
}
__global__ __launch_bounds__(BNL_DW_T) void bnl_dw_kernel(BnlDwArgs a) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), row = lane & 15, q = lane >> 4;
    const int RA = (a.RA + 15) & ~15, RB = (a.RB + 15) & ~15;
    constexpr int lda = BNL_LD, ldb = BNL_LD;
    float* As = lds;
    float* Bs = lds + BNL_EB * lda;
    float* Sc = Bs + BNL_EB * ldb;                       // [2][128]: BatchNorm scale / shift of the input columns (1 / 0 without, 0 / 0 beyond RB)
    const int NT = RB / 16, NRT = RA / 16;
    // a wave's tiles: consecutive ids in column-major order (id = column tile x NRT + row tile)
    const int nper = (NRT * NT + BNL_DW_WAVES - 1) / BNL_DW_WAVES;
    const int ns = min(nper, max(0, NRT * NT - wave * nper));
    int rts[BNL_DW_SLOTS], cts[BNL_DW_SLOTS];
    bool same = true;
#pragma unroll
    for (int s = 0; s < BNL_DW_SLOTS; ++s) {
        const int id = wave * nper + s;
        const bool v = s < ns;
        cts[s] = v ? id / NRT : 0; rts[s] = v ? id - cts[s] * NRT : 0;
        if (v && cts[s] != cts[0]) same = false;
    }
    f4 acc[BNL_DW_SLOTS];
#pragma unroll
    for (int s = 0; s < BNL_DW_SLOTS; ++s) acc[s] = pf_splat(0.f);
    const int r_lo = blockIdx.x * a.chunk, r_hi = min(a.rows, r_lo + a.chunk);
    const int ra4 = RA / 4, rb4 = RB / 4;
    constexpr int UN = (BNL_EB * 32 + BNL_DW_T - 1) / BNL_DW_T;
    int elA[UN], cA[UN], elB[UN], cB[UN];
#pragma unroll
    for (int n = 0; n < UN; ++n) {
        const int k = threadIdx.x + BNL_DW_T * n;
        elA[n] = k / ra4; cA[n] = (k - elA[n] * ra4) * 4;
        elB[n] = k / rb4; cB[n] = (k - elB[n] * rb4) * 4;
    }
    const bool veca = (a.RA & 3) == 0, vecb = (a.RB & 3) == 0 && (a.ldx & 3) == 0;
    const float slope = a.sc ? a.slope : 1.f;
    for (int i = threadIdx.x; i < BNL_EB * (lda + ldb); i += BNL_DW_T) As[i] = 0.f;      // padding columns: never written again
    if (threadIdx.x < 128) {
        const int c = threadIdx.x;
        Sc[c] = c < a.RB ? (a.sc ? a.sc[c] : 1.f) : 0.f;
        Sc[128 + c] = (c < a.RB && a.sc) ? a.sh[c] : 0.f;
    }
    // every load is issued unconditionally through an address that is valid even when the unit is not (then replaced by zero)
    f4 ra[UN], rbx[UN];
    auto fetch = [&](int rb) {
#pragma unroll
        for (int n = 0; n < UN; ++n) {
            const int r = rb + elA[n], c = cA[n];
            const bool ok = elA[n] < BNL_EB && r < r_hi && c < a.RA;
            const float* ptr = ok ? a.dy + (size_t)r * a.RA + c : a.dy;
            f4 v;
            if (veca) v = *reinterpret_cast<const f4*>(ptr);
            else {
#pragma unroll
                for (int w = 0; w < 4; ++w) { const bool okw = ok && c + w < a.RA; const float x = ptr[okw ? w : 0]; v[w] = okw ? x : 0.f; }
            }
            ra[n] = ok ? v : pf_splat(0.f);
        }
#pragma unroll
        for (int n = 0; n < UN; ++n) {
            const int r = rb + elB[n], c = cB[n];
            const bool ok = elB[n] < BNL_EB && r < r_hi && c < a.RB;
            const float* ptr = ok ? a.X + (size_t)r * a.ldx + c : a.X;
            f4 v;
            if (vecb) v = *reinterpret_cast<const f4*>(ptr);
            else {
#pragma unroll
                for (int w = 0; w < 4; ++w) { const bool okw = ok && c + w < a.RB; const float x = ptr[okw ? w : 0]; v[w] = okw ? x : 0.f; }
            }
            rbx[n] = ok ? v : pf_splat(0.f);
        }
    };
    const bool bpow = (RA & (RA - 1)) == 0;              // RA = 16 .. 128: thread (column, row group) sums its rows of every block
    const int bcol = threadIdx.x & (RA - 1), bgrp = threadIdx.x / RA, brows = bpow ? BNL_EB / (BNL_DW_T / RA) : 0;
    float bsum = 0.f;
    fetch(r_lo);
    for (int rb = r_lo; rb < r_hi; rb += BNL_EB) {
        __syncthreads();
#pragma unroll
        for (int n = 0; n < UN; ++n) {
            if (elA[n] < BNL_EB) *reinterpret_cast<f4*>(As + elA[n] * lda + cA[n]) = ra[n];
            if (elB[n] < BNL_EB) {
                const f4 s1 = *reinterpret_cast<const f4*>(Sc + cB[n]), s2 = *reinterpret_cast<const f4*>(Sc + 128 + cB[n]);
                *reinterpret_cast<f4*>(Bs + elB[n] * ldb + cB[n]) = lrelu4(rbx[n] * s1 + s2, slope);
            }
        }
        __syncthreads();
        if (rb + BNL_EB < r_hi) fetch(rb + BNL_EB);
        if (bpow) {
            for (int e = 0; e < brows; ++e) bsum += As[(bgrp * brows + e) * lda + bcol];
        } else if ((int)threadIdx.x < RA) {
#pragma unroll 8
            for (int el = 0; el < BNL_EB; ++el) bsum += As[el * lda + threadIdx.x];
        }
        const float* ar0 = As + q * lda + row;
        const float* br0 = Bs + q * ldb + row;
        switch (same ? ns : -ns) {
#define PF_BNLB(NS)                                                                 \
            case NS: bnl_dw_block<NS, true>(ar0, br0, rts, cts, acc); break;        \
            case -NS: bnl_dw_block<NS, false>(ar0, br0, rts, cts, acc); break;
            PF_BNLB(1) PF_BNLB(2) PF_BNLB(3) PF_BNLB(4) PF_BNLB(5) PF_BNLB(6) PF_BNLB(7) PF_BNLB(8)
#undef PF_BNLB
            default: break;
        }
    }
    if (bpow) {                                          // the row groups' bias sums, added in group order
        __syncthreads();
        if (brows > 0) As[bgrp * lda + bcol] = bsum;
        __syncthreads();
        bsum = 0.f;
        if ((int)threadIdx.x < RA)
            for (int gI = 0; gI < BNL_DW_T / RA; ++gI) bsum += As[gI * lda + threadIdx.x];
    }
    if ((int)threadIdx.x < RA) a.bpart[(size_t)blockIdx.x * RA + threadIdx.x] = bsum;
    float* out = a.part + (size_t)blockIdx.x * RA * RB;
#pragma unroll
    for (int s = 0; s < BNL_DW_SLOTS; ++s)
        if (s < ns)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)(rts[s] * 16 + 4 * q + r) * RB + cts[s] * 16 + row] = acc[s][r];
}

// dW[c * ldw + coff + u] = sum_chunks part[k][c][u] (c < RA, u < RB); db[c] = sum_chunks bpart[k][c] (db nullable)
__global__ __launch_bounds__(256) void bnl_reduce_kernel(const float* part, const float* bpart, int nchunk, int RA, int RB, int RA16,
                                                         int RB16, float* dW, int ldw, int coff, float* db) {
    __shared__ double shr[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + tx;
    const int total = RA * (RB + 1);
    const bool ok = i < total;
    const int c = ok ? i / (RB + 1) : 0, u = ok ? i % (RB + 1) : 0;
    double s = 0.0;
    if (ok) {
        if (u == RB) { for (int k = ty; k < nchunk; k += 4) s += (double)bpart[(size_t)k * RA16 + c]; }
        else {
            int k = ty;
            for (; k + 12 < nchunk; k += 16) {                        // four loads in flight per thread
                const float v0 = part[((size_t)k * RA16 + c) * RB16 + u], v1 = part[((size_t)(k + 4) * RA16 + c) * RB16 + u];
                const float v2 = part[((size_t)(k + 8) * RA16 + c) * RB16 + u], v3 = part[((size_t)(k + 12) * RA16 + c) * RB16 + u];
                s += ((double)v0 + (double)v1) + ((double)v2 + (double)v3);
            }
            for (; k < nchunk; k += 4) s += (double)part[((size_t)k * RA16 + c) * RB16 + u];
        }
    }
    shr[ty][tx] = s;
    __syncthreads();
    if (ty != 0 || !ok) return;
    s = (shr[0][tx] + shr[1][tx]) + (shr[2][tx] + shr[3][tx]);
    if (u == RB) { if (db) db[c] = (float)s; }
    else dW[(size_t)c * ldw + coff + u] = (float)s;
}

#ifndef PF_BNL_CHUNK
#define PF_BNL_CHUNK 256
#endif
constexpr int BNL_CHUNK = PF_BNL_CHUNK;

int bnl_check(const PfBnMlpTrain* p) {
    if (!p) return PF_ERR_NULL;
    if (p->rows < 16 || (p->nl != 2 && p->nl != 3)) return PF_ERR_SHAPE;       // (rows >= 2 also keeps the unbiased-variance factor R / (R - 1) finite)
    if (p->kin0a < 1 || p->kin0a > 128 || p->kin0b < 0 || p->kin0b > 128) return PF_ERR_UNSUPPORTED;
    if (p->kin0b > 0 && (p->kin0a & 3)) return PF_ERR_UNSUPPORTED;
    for (int l = 0; l < p->nl; ++l)
        if (p->width[l] < 16 || p->width[l] > 128 || p->width[l] % 16 != 0) return PF_ERR_UNSUPPORTED;
    const bool sum_in = (p->flags & PF_BNMLP_SUM_INPUTS) != 0;
    if (sum_in && (p->nl < 2 || p->kin0a != p->width[0] || p->kin0b != p->width[0] || !p->xb)) return PF_ERR_SHAPE;
    for (int l = 0; l < p->nl; ++l)
        if ((!p->W[l] && !(sum_in && l == 0)) || !p->y[l]) return PF_ERR_NULL;
    for (int l = 0; l < p->nl - 1; ++l)
        if (!p->gamma[l] || !p->beta[l] || !p->aff[l]) return PF_ERR_NULL;
    if (!p->xa || (p->kin0b > 0 && !p->xb) || !p->stat) return PF_ERR_NULL;
    return PF_OK;
}
inline int bnl_nt(int w) { const int n = (w + 15) / 16; return n <= 1 ? 1 : (n <= 2 ? 2 : (n <= 4 ? 4 : 8)); }

template <int NT>
void bnl_fwd_launch(const BnlFwdArgs& a, int grid, hipStream_t s) {
    const int kin16 = (a.kin + 15) & ~15;
    const size_t lds = sizeof(float) * ((size_t)NT * 16 * (kin16 + 4) + 2 * kin16);
    if (a.addA) {
        if (a.nout == 16 * NT && NT >= 1) {                               // the streaming form (full 16-column blocks)
            hipLaunchKernelGGL(bnl_sum_kernel<NT>, dim3(grid), dim3(256), 0, s, a);
            return;
        }
        allow_lds((bnl_fwd_kernel<NT, true>), lds);
        hipLaunchKernelGGL((bnl_fwd_kernel<NT, true>), dim3(grid), dim3(256), lds, s, a);
        return;
    }
    allow_lds((bnl_fwd_kernel<NT, false>), lds);
    hipLaunchKernelGGL((bnl_fwd_kernel<NT, false>), dim3(grid), dim3(256), lds, s, a);
}
void bnl_fwd_dispatch(const BnlFwdArgs& a, int grid, hipStream_t s) {
    switch (bnl_nt(a.nout)) {
        case 1: bnl_fwd_launch<1>(a, grid, s); break;
        case 2: bnl_fwd_launch<2>(a, grid, s); break;
        case 4: bnl_fwd_launch<4>(a, grid, s); break;
        default: bnl_fwd_launch<8>(a, grid, s); break;
    }
}
template <int NT, int SRC>
void bnl_bwd_launch(const BnlBwdArgs& a, int grid, hipStream_t s) {
    const int kin16 = (a.kin + 15) & ~15;
    const size_t lds = sizeof(float) * ((size_t)NT * 16 * (kin16 + 4) + 6 * kin16);
    allow_lds(bnl_bwd_kernel<NT, SRC>, lds);
    hipLaunchKernelGGL((bnl_bwd_kernel<NT, SRC>), dim3(grid), dim3(256), lds, s, a);
}
void bnl_bwd_dispatch(const BnlBwdArgs& a, int src, int grid, hipStream_t s) {
    const int nt = a.dx ? bnl_nt(a.nout) : 1;
#define PF_BNLB(NT) do { if (src == 1) bnl_bwd_launch<NT, 1>(a, grid, s); else bnl_bwd_launch<NT, 2>(a, grid, s); } while (0)
    switch (nt) {
        case 1: PF_BNLB(1); break;
        case 2: PF_BNLB(2); break;
        case 4: PF_BNLB(4); break;
        default: PF_BNLB(8); break;
    }
#undef PF_BNLB
}

}  // namespace

extern "C" long long pf_bnmlp_train_ws_floats(const PfBnMlpTrain* p) {
    if (!p || p->rows < 16) return -1;
    const long long nchunk = (p->rows + BNL_CHUNK - 1) / BNL_CHUNK;
    return nchunk * (128ll * 128 + 128);
}

extern "C" int pf_bnmlp_train_fwd(const PfBnMlpTrain* p, void* stream) {
    int st = bnl_check(p);
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    const int ntiles = (p->rows + 15) / 16;
    const int grid = (ntiles + 3) / 4 < EC_GRID ? (ntiles + 3) / 4 : EC_GRID;
    const int in0 = p->kin0a + p->kin0b;
    for (int l = 0; l < p->nl; ++l) {
        const bool bn = l < p->nl - 1;
        BnlFwdArgs a{};
        a.slope = p->slope; a.out = p->y[l]; a.nout = p->width[l]; a.rows = p->rows; a.ntiles = ntiles;
        if (bn) a.fin = StatFin{p->stat, 1, p->width[l], 0, p->width[l], p->aff[l], p->gamma[l], p->beta[l], p->run_mean[l],
                                p->run_var[l], p->eps, p->momentum, nullptr, nullptr, nullptr, (double)p->rows, p->sync_sums};
        if (bn) a.fin.det = PF_DET(p);
        if (l == 0 && (p->flags & PF_BNMLP_SUM_INPUTS)) {
            // layer 0 is NOT a product: its pre-BatchNorm output is the sum of the two inputs (their producers' last linear layers
            // carry this layer's weights folded in - train_ops.py interp_weights): y[0] = xa + xb, statistics as usual
            a.addA = p->xa; a.addB = p->xb; a.X = p->xa; a.ldx = p->kin0a; a.kin = 16; a.W = nullptr; a.ldw = 0; a.bias = nullptr;
            a.want_stats = bn;
            bnl_fwd_dispatch(a, grid, s);
        } else if (l == 0) {
            a.X = p->xa; a.ldx = p->kin0a; a.kin = p->kin0a; a.W = p->W[0]; a.ldw = in0; a.bias = p->b[0];
            a.want_stats = bn && p->kin0b == 0;
            bnl_fwd_dispatch(a, grid, s);
            if (p->kin0b > 0) {
                a.X = p->xb; a.ldx = p->kin0b; a.kin = p->kin0b; a.W = p->W[0] + p->kin0a; a.bias = nullptr; a.accum = 1;
                a.want_stats = bn;
                bnl_fwd_dispatch(a, grid, s);
            }
        } else {
            a.X = p->y[l - 1]; a.ldx = p->width[l - 1]; a.kin = p->width[l - 1];
            a.sc = p->aff[l - 1]; a.sh = p->aff[l - 1] + p->width[l - 1];
            a.W = p->W[l]; a.ldw = p->width[l - 1]; a.bias = p->b[l]; a.want_stats = bn;
            bnl_fwd_dispatch(a, grid, s);
        }
        if (bn && (st = pf_stat_sync(a.fin, p->width[l], p->sync_cb, p->sync_user, s))) return st;   // SyncBN: global statistics
    }
    return pf_last_launch_status();
}

extern "C" int pf_bnmlp_train_bwd(const PfBnMlpTrain* p, void* stream) {
    int st = bnl_check(p);
    if (st) return st;
    if (!p->dout || !p->ws) return PF_ERR_NULL;
    for (int l = 0; l < p->nl; ++l)
        if (!p->dW[l] && !((p->flags & PF_BNMLP_SUM_INPUTS) && l == 0)) return PF_ERR_NULL;
    for (int l = 0; l < p->nl - 1; ++l)
        if (!p->d[l] || !p->coef[l] || !p->dgamma[l] || !p->dbeta[l]) return PF_ERR_NULL;
    if (p->ws_floats < pf_bnmlp_train_ws_floats(p)) return PF_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int ntiles = (p->rows + 15) / 16;
    const int grid = (ntiles + 3) / 4 < EC_GRID ? (ntiles + 3) / 4 : EC_GRID;
    const int nchunk = (p->rows + BNL_CHUNK - 1) / BNL_CHUNK;
    float* part = p->ws;
    float* bpart = p->ws + (size_t)nchunk * 128 * 128;
    const int in0 = p->kin0a + p->kin0b;
    auto dw = [&](const float* dy, int RA, const float* X, int ldx, int RB, const float* sc, const float* sh, float* dW, int ldw,
                  int coff, float* db) {
        const int RA16 = (RA + 15) & ~15, RB16 = (RB + 15) & ~15;
        BnlDwArgs a{dy, RA, X, ldx, RB, sc, sh, p->slope, p->rows, BNL_CHUNK, part, bpart};
        const size_t lds = sizeof(float) * ((size_t)BNL_EB * 2 * BNL_LD + 256);
        (void)RA16; (void)RB16;
        hipLaunchKernelGGL(bnl_dw_kernel, dim3(nchunk), dim3(BNL_DW_T), lds, s, a);
        const int total = RA * (RB + 1);
        hipLaunchKernelGGL(bnl_reduce_kernel, dim3((total + 63) / 64), dim3(256), 0, s, part, bpart, nchunk, RA, RB, RA16, RB16, dW,
                           ldw, coff, db);
    };
    for (int l = p->nl - 1; l >= 0; --l) {
        const bool bn = l < p->nl - 1;
        const float* dyl = bn ? p->d[l] : p->dout;          // after the kernel below: the gradient wrt this layer's pre-BN output
        BnlBwdArgs a{};
        a.kin = p->width[l]; a.slope = p->slope; a.rows = p->rows; a.ntiles = ntiles;
        if (bn) { a.dbuf = p->d[l]; a.ypre = p->y[l]; a.aff = p->aff[l]; a.coef = p->coef[l]; }
        else a.dy = p->dout;
        if (l > 0) {
            a.W = p->W[l]; a.ldw = p->width[l - 1]; a.dx = p->d[l - 1]; a.nout = p->width[l - 1];
            a.xpre = p->y[l - 1]; a.aff_prev = p->aff[l - 1]; a.want_stats = 1;
            a.fin = StatFin{p->stat, 2, p->width[l - 1], 0, p->width[l - 1], nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f,
                            p->coef[l - 1], p->dgamma[l - 1], p->dbeta[l - 1], (double)p->rows, p->sync_sums};
            a.fin.det = PF_DET(p);
            bnl_bwd_dispatch(a, bn ? 2 : 1, grid, s);
            if ((st = pf_stat_sync(a.fin, p->width[l - 1], p->sync_cb, p->sync_user, s))) return st;   // SyncBN: global sums of layer l - 1
            dw(dyl, p->width[l], p->y[l - 1], p->width[l - 1], p->width[l - 1], p->aff[l - 1], p->aff[l - 1] + p->width[l - 1],
               p->dW[l], p->width[l - 1], 0, p->db[l]);
        } else if (p->flags & PF_BNMLP_SUM_INPUTS) {
            // y[0] = xa + xb: the gradient of both inputs is d[0] after its BatchNorm backward (converted in place); no weights
            a.W = nullptr; a.ldw = 0; a.dx = nullptr; a.nout = 0;
            if (bn) bnl_bwd_dispatch(a, 2, grid, s);
        } else {
            // first layer: one pass per input tensor; the first pass also converts d[0] in place
            a.W = p->W[0]; a.ldw = in0; a.dx = p->dxa; a.nout = p->kin0a;
            if (bn || p->dxa) bnl_bwd_dispatch(a, bn ? 2 : 1, grid, s);
            if (p->kin0b > 0 && p->dxb) {
                BnlBwdArgs b2 = a;
                b2.dy = dyl; b2.dbuf = nullptr; b2.W = p->W[0] + p->kin0a; b2.dx = p->dxb; b2.nout = p->kin0b;
                bnl_bwd_dispatch(b2, 1, grid, s);
            }
            dw(dyl, p->width[0], p->xa, p->kin0a, p->kin0a, nullptr, nullptr, p->dW[0], in0, 0, p->db[0]);
            if (p->kin0b > 0) dw(dyl, p->width[0], p->xb, p->kin0b, p->kin0b, nullptr, nullptr, p->dW[0], in0, p->kin0a, nullptr);
        }
    }
    return pf_last_launch_status();
}
