// Forward of one FeatureExtractUnit of the training step (pf_ec_train.h describes the whole unit): weight fold, the per-layer
// kernels and the persistent one-launch form.
#include "pf_ec_train.h"
#include "pf_wave.h"

namespace {

// ------------------------------------------------------------------------------------------------ forward, one conv
// growth layer t (OUT = false): Y[:, col0 : col0 + g] = P_t[i] + Q_t[j] + lrelu(bn(Y[:, :kin])) W^T, statistics of the result
// conv_out (OUT = true): the same product on all GT growth channels, then max over the 16 edges of a point (POOL) or the
// per-edge rows
struct EcFwdArgs {
    float* Y; int ldy;               // [E, ldy] pre-BN outputs of the growth layers
    const float* aff;                // [4][ldy]: scale, shift, mean, rstd of the finished layers
    const float* W; int ldw;         // growth columns of this conv: W[c * ldw + u], c < nout, u < kin
    const float* pq; int ldpq;       // [T, ldpq] = P (+ bias) | Q
    int poff, qoff;                  // columns of this conv's P and Q
    const int* idx;                  // [E] batch-local neighbour index
    int N, K;
    int kin, col0, nout;
    int ntiles;                      // E / 16
    float slope;
    float* out; unsigned char* arg;  // conv_out only
    StatFin fin;                     // growth layers only
};

template <int NT, bool OUT, bool POOL>
__global__ __launch_bounds__(256) void ec_fwd_kernel(EcFwdArgs a) {
    extern __shared__ float lds[];
    __shared__ float red[8 * STAT_W];
    const int kin16 = (a.kin + 15) & ~15, kp = kin16 + 4, KS = kin16 / 16;
    float* Wl = lds;
    float* al = lds + NT * 16 * kp;
    float* bl = al + kin16;
    // 16 lanes along a weight row (coalesced, no division); a thread's <= 8 elements of a row are loaded together, then stored:
    // a load -> store loop pays a full memory latency per element
    for (int c = threadIdx.x >> 4; c < NT * 16; c += 16) {
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
        al[i] = i < a.kin ? a.aff[i] : 0.f;
        bl[i] = i < a.kin ? a.aff[a.ldy + i] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, q = lane >> 4;
    const f4 ident = ident_b(row, q);
    // column statistics are accumulated CENTRED on a pivot (the layer's running mean as every workgroup reads it at its
    // start - the last workgroup updates it only after all have arrived): sum (y - p), sum (y - p)^2.  E[y^2] - E[y]^2 on raw
    // fp32 partial sums loses |mean|^2 / var digits; the running mean tracks the batch mean, so the centred form does not
    float s0[NT], s1[NT], piv[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        s0[nt] = s1[nt] = 0.f;
        const int col = nt * 16 + row;
        piv[nt] = (!OUT && a.fin.run_mean && col < a.nout) ? a.fin.run_mean[col] : 0.f;
    }
    const int tile0 = blockIdx.x * 4 + wave;
    int jnext = tile0 < a.ntiles ? a.idx[(long long)tile0 * 16 + row] : 0;
    for (int tile = tile0; tile < a.ntiles; tile += gridDim.x * 4) {
        const long long e0 = (long long)tile * 16;
        // all loads of the tile first: the growth-feature row of this lane's edge and its P[i] + Q[j] addend (the neighbour
        // index was fetched during the previous tile: one dependent memory latency less per tile)
        const int er = (int)e0 + row;
        const int ir = er / a.K;
        const long long jr = (long long)(ir / a.N) * a.N + jnext;
        {
            const int tn = tile + gridDim.x * 4;
            if (tn < a.ntiles) jnext = a.idx[(long long)tn * 16 + row];
        }
        const float* yrow = a.Y + (size_t)er * a.ldy;
        f4 yv[8];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            yv[ks] = pf_splat(0.f);
            if (ks < KS && ks * 16 + 4 * q < a.kin) yv[ks] = *reinterpret_cast<const f4*>(yrow + ks * 16 + 4 * q);
        }
        f4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int c4 = nt * 16 + 4 * q;
            f4 ex = pf_splat(0.f);
            if (c4 < a.nout)
                ex = *reinterpret_cast<const f4*>(a.pq + (size_t)ir * a.ldpq + a.poff + c4) +
                     *reinterpret_cast<const f4*>(a.pq + (size_t)jr * a.ldpq + a.qoff + c4);
            acc[nt] = mfma4(ex, ident, pf_splat(0.f));
        }
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            if (ks < KS) {
                const int u = ks * 16 + 4 * q;
                f4 av = pf_splat(0.f);
                if (u < a.kin)
                    av = lrelu4(yv[ks] * *reinterpret_cast<const f4*>(al + u) + *reinterpret_cast<const f4*>(bl + u), a.slope);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[nt] = mfma4(av, *reinterpret_cast<const f4*>(Wl + (nt * 16 + row) * kp + u), acc[nt]);
            }
        }
        if (!OUT) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = nt * 16 + row;
                if (col < a.nout) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = acc[nt][r];
                        a.Y[(e0 + 4 * q + r) * a.ldy + a.col0 + col] = v;
                        const float vc = v - piv[nt];
                        s0[nt] += vc; s1[nt] = fmaf(vc, vc, s1[nt]);
                    }
                }
            }
        } else if (!POOL) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = nt * 16 + row;
                if (col < a.nout)
#pragma unroll
                    for (int r = 0; r < 4; ++r) a.out[(e0 + 4 * q + r) * a.nout + col] = acc[nt][r];
            }
        } else {                                                       // K = 16: the tile is point `tile`
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                float best = acc[nt][0];
                int bk = 4 * q;
#pragma unroll
                for (int r = 1; r < 4; ++r)
                    if (acc[nt][r] > best) { best = acc[nt][r]; bk = 4 * q + r; }
#pragma unroll
                for (int m = 16; m < 64; m <<= 1) {
                    const float ov = __shfl_xor(best, m);
                    const int ok = __shfl_xor(bk, m);
                    if (ov > best || (ov == best && ok < bk)) { best = ov; bk = ok; }
                }
                const int col = nt * 16 + row;
                if (q == 0 && col < a.nout) {
                    a.out[(long long)tile * a.nout + col] = best;
                    a.arg[(long long)tile * a.nout + col] = (unsigned char)bk;
                }
            }
        }
    }
    if (!OUT) stat_flush<NT>(s0, s1, 0, a.nout, a.fin, red);
}

// ------------------------------------------------------------------------------------------------ forward, conv_out on the fp16 pipe
// conv_out is the one forward kernel whose matrix work is not negligible (E x GT x odim products: 38 % pipe-busy on f32 MFMAs).
// Here its products run as split-fp16 (csrc/pf_mfma.h "f16x2": x = hi + lo' 2^-11, hi.hi in the main accumulator, hi.lo' + lo'.hi
// in a second one folded in as acc + accx 2^-11 - 22+ significant bits per operand; activations after BatchNorm + LeakyReLU and
// weights are far inside the fp16 range): three v_mfma_f32_16x16x32_f16 per 32 channels instead of eight f32 MFMAs.  Lane
// (row = edge, kg = l >> 4) holds the 8 channels 8 kg .. 8 kg + 7 of a 32-channel chunk of its edge's feature row; the weights
// are converted once per workgroup into ready fragments [tile][chunk][hi | lo'][lane][8 x f16]; the per-edge addend P[i] + Q[j]
// enters through an identity B operand, split the same way.  Accumulator layout, pooling and outputs as in ec_fwd_kernel.
template <int NT, bool POOL>
__global__ __launch_bounds__(256) void ec_fwd16_kernel(EcFwdArgs a) {
    extern __shared__ float lds[];
    const int nch = (a.kin + 31) / 32;
    uint4* Wf = reinterpret_cast<uint4*>(lds);                    // ((nt * nch + chunk) * 2 + hi|lo) * 64 + lane
    float* al = lds + (size_t)NT * nch * 2 * 64 * 4;
    float* bl = al + nch * 32;
    for (int unit = threadIdx.x; unit < NT * nch * 64; unit += 256) {
        const int frag = unit >> 6, ln = unit & 63, u = ln & 15, kg = ln >> 4, nt = frag / nch, ch = frag % nch;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = ch * 32 + 8 * kg + j, o = nt * 16 + u;
            v[j] = (c < a.kin && o < a.nout) ? a.W[(size_t)o * a.ldw + c] : 0.f;
        }
        const f4 v0 = {v[0], v[1], v[2], v[3]}, v1 = {v[4], v[5], v[6], v[7]};
        const PfPair2 f = pf_pair2(v0, v1);
        Wf[(frag * 2 + 0) * 64 + ln] = __builtin_bit_cast(uint4, f.h);
        Wf[(frag * 2 + 1) * 64 + ln] = __builtin_bit_cast(uint4, f.l);
    }
    for (int i = threadIdx.x; i < nch * 32; i += 256) {
        al[i] = i < a.kin ? a.aff[i] : 0.f;
        bl[i] = i < a.kin ? a.aff[a.ldy + i] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, q = lane >> 4;
    h8 identh;                                            // B[k][j] = (k == j) for k < 16, this lane: j = row, k = 8 q + jj
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) identh[jj] = (8 * q + jj == row) ? (_Float16)1.f : (_Float16)0.f;
    const int tile0 = blockIdx.x * 4 + wave;
    int jnext = tile0 < a.ntiles ? a.idx[(long long)tile0 * 16 + row] : 0;
    for (int tile = tile0; tile < a.ntiles; tile += gridDim.x * 4) {
        const long long e0 = (long long)tile * 16;
        const int er = (int)e0 + row;
        const int ir = er / a.K;
        const long long jr = (long long)(ir / a.N) * a.N + jnext;
        {
            const int tn = tile + gridDim.x * 4;
            if (tn < a.ntiles) jnext = a.idx[(long long)tn * 16 + row];
        }
        const float* yrow = a.Y + (size_t)er * a.ldy;
        f4 y0[4], y1[4];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            y0[ch] = y1[ch] = pf_splat(0.f);
            const int c = ch * 32 + 8 * q;
            if (ch < nch && c < a.kin) {                             // kin is a multiple of 8
                y0[ch] = *reinterpret_cast<const f4*>(yrow + c);
                y1[ch] = *reinterpret_cast<const f4*>(yrow + c + 4);
            }
        }
        f4 acc[NT], accx[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int c8 = nt * 16 + 8 * q;                          // the addend's channels: k = 8 q + jj < 16 of this tile
            f4 e0v = pf_splat(0.f), e1v = pf_splat(0.f);
            if (q < 2 && c8 < a.nout) {
                const float* pp = a.pq + (size_t)ir * a.ldpq + a.poff + c8;
                const float* qp = a.pq + (size_t)jr * a.ldpq + a.qoff + c8;
                e0v = *reinterpret_cast<const f4*>(pp) + *reinterpret_cast<const f4*>(qp);
                e1v = *reinterpret_cast<const f4*>(pp + 4) + *reinterpret_cast<const f4*>(qp + 4);
            }
            const PfPair2 E = pf_pair2(e0v, e1v);
            acc[nt] = pf_mfma_f16(E.h, identh, pf_splat(0.f));
            accx[nt] = pf_mfma_f16(E.l, identh, pf_splat(0.f));
        }
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            if (ch < nch) {
                const int c = ch * 32 + 8 * q;
                const f4 a0 = lrelu4(y0[ch] * *reinterpret_cast<const f4*>(al + c) + *reinterpret_cast<const f4*>(bl + c), a.slope);
                const f4 a1 = lrelu4(y1[ch] * *reinterpret_cast<const f4*>(al + c + 4) + *reinterpret_cast<const f4*>(bl + c + 4), a.slope);
                const PfPair2 A = pf_pair2(c < a.kin ? a0 : pf_splat(0.f), c < a.kin ? a1 : pf_splat(0.f));
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const h8 bh = __builtin_bit_cast(h8, Wf[((nt * nch + ch) * 2 + 0) * 64 + lane]);
                    const h8 blo = __builtin_bit_cast(h8, Wf[((nt * nch + ch) * 2 + 1) * 64 + lane]);
                    acc[nt] = pf_mfma_f16(A.h, bh, acc[nt]);
                    accx[nt] = pf_mfma_f16(A.h, blo, accx[nt]);
                    accx[nt] = pf_mfma_f16(A.l, bh, accx[nt]);
                }
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = acc[nt] + accx[nt] * PF_LO_INV;
        if (!POOL) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = nt * 16 + row;
                if (col < a.nout)
#pragma unroll
                    for (int r = 0; r < 4; ++r) a.out[(e0 + 4 * q + r) * a.nout + col] = acc[nt][r];
            }
        } else {                                                       // K = 16: the tile is point `tile`
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                float best = acc[nt][0];
                int bk = 4 * q;
#pragma unroll
                for (int r = 1; r < 4; ++r)
                    if (acc[nt][r] > best) { best = acc[nt][r]; bk = 4 * q + r; }
#pragma unroll
                for (int m = 16; m < 64; m <<= 1) {
                    const float ov = __shfl_xor(best, m);
                    const int ok = __shfl_xor(bk, m);
                    if (ov > best || (ov == best && ok < bk)) { best = ov; bk = ok; }
                }
                const int col = nt * 16 + row;
                if (q == 0 && col < a.nout) {
                    a.out[(long long)tile * a.nout + col] = best;
                    a.arg[(long long)tile * a.nout + col] = (unsigned char)bk;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ forward, the whole unit in ONE launch
// The per-layer kernels above pay, per unit, five launch ramps / drains and re-read every earlier layer's pre-BatchNorm output
// from memory (0 + 1 + 2 + 3 growth blocks for the growth layers, all four again for conv_out: ~170 MB per 128-channel unit next
// to the 67 MB it has to write for the backward).  BatchNorm's batch statistics are the only thing that couples two edges, so a
// PERSISTENT grid can keep an edge tile's features in registers through the whole dense block and meet at a grid barrier once
// per BatchNorm layer:
//   * one workgroup per CU (512 threads = 8 waves, 2 per SIMD, <= 256 VGPRs), a wave owns up to ECP_TPW tiles of 16 edges (= one
//     point and its K = 16 neighbours) for the whole launch;
//   * channel-major chain (pf_mfma.h): output channels on MFMA rows, the 16 edges on the columns - a layer's accumulator tile
//     IS the next layer's B operand, no transposition, no LDS round trip;
//   * layer t: y_t = P_t[i] + Q_t[j] + W_t f_{<t} (v_mfma_f32_16x16x4_f32, the k order of ec_fwd_kernel: the stored Y is bit
//     for bit the per-layer kernels'), Y stored once for the backward, column sums (centred on the running mean) -> 16 spread
//     double accumulators -> arrival counter; the workgroup that arrives last turns the sums into scale / shift / running
//     statistics (the StatFin arithmetic) and publishes the barrier's generation word; everyone applies BatchNorm + LeakyReLU to
//     the tile it still holds;
//   * conv_out on split-fp16 products (the f16x2 arithmetic of ec_fwd16_kernel, weights converted once per workgroup into A
//     fragments in LDS), max over the 16 edges = the 16 lanes of a DPP row, argmax = smallest k among the maxima.
// Barrier: agent-scope relaxed atomics only (arrive: s_waitcnt vmcnt(0) + atomic add; release: the last arriver's atomic stores
// of aff, s_waitcnt, then the generation word) - no release fence (a device-scope fence writes the L2 back: tens of us).
// Co-residency is the HOST's job (pf_ec_train_fwd: occupancy x CU count >= grid, and the caller's PF_EC_PERSISTENT flag says no
// other barrier kernel of this process can be in flight); the spin is bounded anyway: on timeout the status word sync[3] is
// set, the unit's output becomes NaN and the grid drains.
struct EcFwdPArgs {
    float* Y; int ldy;               // [E, GT]
    float* aff;                      // [4][GT]
    const float* Wg[8]; int ldwg[8]; // growth columns of conv t (pointer past the 3C edge-feature columns)
    const float* Wout; int ldwout;
    const float* pq; int ldpq; int S;
    const int* idx; int N;
    int ntiles;                      // = points (K = 16)
    float slope;
    float* out; unsigned char* arg;
    const float* gamma[8]; const float* beta[8]; float* run_mean[8]; float* run_var[8];
    float eps, momentum; double R;
    double* acc;                     // [STAT_COPIES][2][STAT_W] accumulators (zero between uses)
    unsigned* sync;                  // [0] arrivals [1] generation [2] exits [3] status (sticky: 1 = a barrier timed out)
};

template <int G, int NC, int ODIM>
__global__ __launch_bounds__(ECP_T) void ec_fwdp_kernel(EcFwdPArgs a) {
    constexpr int TPW = ecp_tpw(G);                   // tiles of 16 edges a wave owns for the whole launch
    constexpr int GT = G * NC, NB = GT / 16, NTG = (G + 15) / 16, NTO = ODIM / 16, NCP = NB / 2;
    constexpr int OCH = NB >= 8 ? 1 : 2;                       // conv_out blocks per accumulator chunk: 2 x 4 x ECP_TPW x OCH accumulator
                                                               // registers beside the wave's ECP_TPW x NB x 4 feature registers
    constexpr bool OWN = G % 16 == 0;                          // a layer's 16-channel blocks are its own (G = 8: two layers share one)
    static_assert(GT % 32 == 0 && ODIM % 16 == 0 && NTO % OCH == 0 && 32 * NC <= STAT_W && G <= 32, "shape");
    // no aligned(16) here: every kernel of a source shares ONE dynamic LDS symbol and it stayed 4-byte aligned while this kernel
    // asked for 16 below the per-layer kernels' plain declaration (the request never took effect; the fragments are read with
    // unaligned-capable LDS instructions).  Honouring it moves the buffer by 12 bytes and changes the code of every kernel that
    // uses `lds`: a change to measure on its own.
    extern __shared__ float lds[];
    __shared__ float red[ECP_WAVES * 2 * 32];
    __shared__ float scsh[2 * 32];
    __shared__ int flag;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, q = lane >> 4;

    // ---- this wave's tiles
    int tl[TPW], jr[TPW];
    bool ok[TPW];
#pragma unroll
    for (int s = 0; s < TPW; ++s) {
        tl[s] = blockIdx.x * ECP_WAVES + wave + s * gridDim.x * ECP_WAVES;
        ok[s] = tl[s] < a.ntiles;
        const int tt = ok[s] ? tl[s] : 0;
        jr[s] = (tt / a.N) * a.N + a.idx[(size_t)tt * 16 + col];
        tl[s] = tt;
    }
    f4 f[TPW][NB];
#pragma unroll
    for (int s = 0; s < TPW; ++s)
#pragma unroll
        for (int b = 0; b < NB; ++b) f[s][b] = pf_splat(0.f);
    // the addends P_t[i] + Q_t[j] of layer t for all the wave's tiles (independent gathers, all in flight together).  OWN layers
    // accumulate in the feature slots they are about to fill (free until then), so layer t + 1's addends can be fetched BEFORE
    // the barrier of layer t and their latency disappears behind it
    f4 accs[OWN ? 1 : TPW][NTG];
    auto addends = [&](auto tc) {
        constexpr int t = decltype(tc)::value;
        constexpr int col0 = G * t, b0 = col0 / 16;
#pragma unroll
        for (int s = 0; s < TPW; ++s)
#pragma unroll
            for (int nt = 0; nt < NTG; ++nt) {
                const int c4 = 16 * (b0 + nt) + 4 * q;
                f4 v = pf_splat(0.f);
                if (c4 >= col0 && c4 < col0 + G)
                    v = *reinterpret_cast<const f4*>(a.pq + (size_t)tl[s] * a.ldpq + c4) +
                        *reinterpret_cast<const f4*>(a.pq + (size_t)jr[s] * a.ldpq + a.S + c4);
                if constexpr (OWN) f[s][b0 + nt] = v;
                else accs[s][nt] = v;
            }
    };
    addends(std::integral_constant<int, 0>{});                // layer 0 needs no weights: its gathers fly while the weights are staged

    // ---- LDS images: growth weights of layers 1 .. NC-1 (fp32, row = channel inside the layer's first block, padded rows /
    // columns zero), then conv_out as split-fp16 A fragments [ob][cp][hi | lo'][lane]; first read after barrier 1
    int woff[NC];
    {
        int o = 0;
#pragma unroll
        for (int t = 1; t < NC; ++t) { woff[t] = o; o += NTG * 16 * (((G * t + 15) & ~15) + 4); }
        woff[0] = o;                                           // [0]: start of the conv_out fragments (a multiple of 64 floats)
    }
    // (all of a thread's loads of a matrix are in flight before its first LDS store: a load -> store loop pays one memory
    // latency per element)
    pf_static_for<1, NC>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        if (PF_ECP_DBG & 4) return;
        constexpr int kin = G * t, kin16 = (kin + 15) & ~15, kp = kin16 + 4, ro = (G * t) % 16, NE = NTG * 16 * kin16;
        constexpr int IT = (NE + ECP_T - 1) / ECP_T;
        float* Wl = lds + woff[t];
        float v[IT];
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int i = threadIdx.x + k * ECP_T, rw = i / kin16, u = i % kin16, c = rw - ro;      // tile row -> row of the conv
            v[k] = (i < NE && c >= 0 && c < G && u < kin) ? a.Wg[t][(size_t)c * a.ldwg[t] + u] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int i = threadIdx.x + k * ECP_T;
            if (i < NE) Wl[(i / kin16) * kp + i % kin16] = v[k];
        }
    });
    uint4* Wf = reinterpret_cast<uint4*>(lds + woff[0]);
    if (!(PF_ECP_DBG & 4)) {
        constexpr int NU = NTO * NCP * 64, IT = (NU + ECP_T - 1) / ECP_T;
        f4 w0[IT], w1[IT];
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int unit = threadIdx.x + k * ECP_T, uu = unit < NU ? unit : 0;
            const int frag = uu >> 6, ln = uu & 63, o = (frag / NCP) * 16 + (ln & 15), cp = frag % NCP, kq = ln >> 4;
            const float* wr = a.Wout + (size_t)o * a.ldwout + 32 * cp + 4 * kq;
            w0[k] = (f4){wr[0], wr[1], wr[2], wr[3]};
            w1[k] = (f4){wr[16], wr[17], wr[18], wr[19]};
        }
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int unit = threadIdx.x + k * ECP_T;
            if (unit < NU) {
                const PfPair2 fr = pf_pair2(w0[k], w1[k]);
                Wf[((unit >> 6) * 2 + 0) * 64 + (unit & 63)] = __builtin_bit_cast(uint4, fr.h);
                Wf[((unit >> 6) * 2 + 1) * 64 + (unit & 63)] = __builtin_bit_cast(uint4, fr.l);
            }
        }
    }

    bool alive = true;
    pf_static_for<0, NC>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        constexpr int col0 = G * t, b0 = col0 / 16, KS = (G * t + 15) / 16, kp = ((G * t + 15) & ~15) + 4;
        if (!alive) return;
        const float* Wl = lds + woff[t];
        auto A = [&](int s, int nt) -> f4& {
            if constexpr (OWN) return f[s][b0 + nt];
            else return accs[s][nt];
        };
        if constexpr (!OWN && t > 0) addends(tc);
        // this lane's channels of the layer: c4 = 16 (b0 + nt) + 4 q .. + 3
        bool cv[NTG];
        f4 piv[NTG], s0[NTG], s1[NTG], ycur[OWN ? 1 : TPW][NTG];
#pragma unroll
        for (int nt = 0; nt < NTG; ++nt) {
            const int c4 = 16 * (b0 + nt) + 4 * q;
            cv[nt] = c4 >= col0 && c4 < col0 + G;
            piv[nt] = pf_splat(0.f);
            if (cv[nt] && a.run_mean[t]) piv[nt] = *reinterpret_cast<const f4*>(a.run_mean[t] + (c4 - col0));
            s0[nt] = s1[nt] = pf_splat(0.f);
        }
        if constexpr (t > 0) {                                  // the tiles' MFMA chains, interleaved (independent accumulators)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int nt = 0; nt < NTG; ++nt) {
                    const f4 w = *reinterpret_cast<const f4*>(Wl + (nt * 16 + col) * kp + ks * 16 + 4 * q);
#pragma unroll
                    for (int s = 0; s < TPW; ++s) A(s, nt) = mfma4(w, f[s][ks], A(s, nt));
                }
        }
#pragma unroll
        for (int s = 0; s < TPW; ++s)
#pragma unroll
            for (int nt = 0; nt < NTG; ++nt) {
                const f4 v = A(s, nt);
                if constexpr (!OWN) ycur[s][nt] = v;
                if (cv[nt] && ok[s]) {
                    const f4 vc = v - piv[nt];
                    s0[nt] = s0[nt] + vc;
                    s1[nt] = s1[nt] + vc * vc;
                }
            }
        ecp_stat_publish<G>(s0, s1, b0, col0, t, a.acc, red, !(PF_ECP_DBG & 16));
        if constexpr (OWN && t + 1 < NC) addends(std::integral_constant<int, t + 1>{});      // next layer's gathers fly during the barrier
        // the pivot of the column this thread finalises below, read BEFORE the barrier: workgroup 0 updates the running mean right
        // after it (every workgroup has arrived, i.e. has read its pivots, by then)
        const int fc = threadIdx.x >> 3;
        const float fpv = (a.run_mean[t] && threadIdx.x < 256 && fc < G) ? a.run_mean[t][fc] : 0.f;
        alive = ecp_barrier(a.sync, (unsigned)(t + 1), &flag);
        if (!alive) return;
        // ---- every workgroup turns the sums into the layer's constants for itself (the StatFin mode-1 arithmetic); workgroup 0
        // also leaves them in `aff` for the backward and updates the running statistics
        const EcpSums sums = ecp_stat_fetch(a.acc, t);
        if (threadIdx.x < 256 && (threadIdx.x & 7) == 0 && (threadIdx.x >> 3) < G) {
            const int c = threadIdx.x >> 3;
            const double a0 = sums.part, a1 = sums.other;
            const double pv = (double)fpv;
            const double dm = a0 / a.R;
            const double mean = pv + dm;
            double var = a1 / a.R - dm * dm;
            if (var < 0.0) var = 0.0;
            const float rstd = 1.0f / sqrtf((float)var + a.eps);
            const float sc = a.gamma[t][c] * rstd, sh = a.beta[t][c] - (float)mean * sc;
            scsh[c] = sc;
            scsh[32 + c] = sh;
            if (blockIdx.x == 0) {
                a.aff[col0 + c] = sc;
                a.aff[a.ldy + col0 + c] = sh;
                a.aff[2 * a.ldy + col0 + c] = (float)mean;
                a.aff[3 * a.ldy + col0 + c] = rstd;
                if (a.run_mean[t]) {            // every workgroup read its pivot before it arrived at the barrier above
                    a.run_mean[t][c] = (1.f - a.momentum) * a.run_mean[t][c] + a.momentum * (float)mean;
                    a.run_var[t][c] = (1.f - a.momentum) * a.run_var[t][c] + a.momentum * (float)(var * (a.R / (a.R - 1.0)));
                }
            }
        }
        __syncthreads();
        // ---- BatchNorm + LeakyReLU on the tiles this wave still holds: they become f[.][b0 ..] (rows of other layers that share
        // the block stay as they are: scale = shift = 0 outside the layer gives lrelu(0) = 0)
#pragma unroll
        for (int nt = 0; nt < NTG; ++nt) {
            f4 sc = pf_splat(0.f), sh = pf_splat(0.f);
            if (cv[nt]) {
                const int cl = 16 * (b0 + nt) + 4 * q - col0;
                sc = *reinterpret_cast<const f4*>(scsh + cl);
                sh = *reinterpret_cast<const f4*>(scsh + 32 + cl);
            }
            // the raw tile goes to memory only now (the backward reads it): its stores are in flight during the next layer
            // instead of in front of this layer's barrier, whose s_waitcnt would have waited for them
#pragma unroll
            for (int s = 0; s < TPW; ++s) {
                f4 raw;
                if constexpr (OWN) raw = f[s][b0 + nt];
                else raw = ycur[s][nt];
                if (cv[nt] && ok[s] && !(PF_ECP_DBG & 8))
                    *reinterpret_cast<f4*>(a.Y + ((size_t)tl[s] * 16 + col) * a.ldy + 16 * (b0 + nt) + 4 * q) = raw;
                if constexpr (OWN) f[s][b0 + nt] = lrelu4(raw * sc + sh, a.slope);
                else f[s][b0 + nt] = f[s][b0 + nt] + lrelu4(raw * sc + sh, a.slope);
            }
        }
    });

    // ---- conv_out + max over the 16 edges of the point
    // Operands swapped against the growth layers: the feature pair registers are bit for bit also the A operand with the EDGES on
    // the MFMA rows, the weight fragments the B operand with the channels on the columns, so D[edge][channel] puts 4 edges of ONE
    // channel into a lane - the max over the 16 edges is 3 in-lane comparisons + 2 exchanges across the lane rows instead of a
    // 16-lane reduction per value.  The addend comes in the same layout: P_out[i][c] once, Q_out[j_k][c] for the lane's four
    // edges k = 4 q + r (4-byte gathers, 64 B per 16 lanes).
    // What bounded this phase (58 of 128 us, and the 60 us of ec_fwd16_kernel) is the LDS weight stream: every tile read all
    // 64 KiB of fragments.  Here the features are converted ONCE into split operand pairs - in place of the fp32 registers they
    // replace, same count - and every fragment read serves all of the wave's tiles: a quarter of the LDS bytes.
    if (alive && !(PF_ECP_DBG & 1)) {
        PfPair2 fp[TPW][NCP];
#pragma unroll
        for (int s = 0; s < TPW; ++s)
#pragma unroll
            for (int cp = 0; cp < NCP; ++cp) fp[s][cp] = pf_pair2(f[s][2 * cp], f[s][2 * cp + 1]);
        int jq[TPW][4];
#pragma unroll
        for (int s = 0; s < TPW; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r) jq[s][r] = __shfl(jr[s], 4 * q + r);
#pragma unroll
        for (int oc = 0; oc < NTO; oc += OCH) {
            f4 acc[TPW][OCH], accx[TPW][OCH];
#pragma unroll
            for (int s = 0; s < TPW; ++s)
#pragma unroll
                for (int o = 0; o < OCH; ++o) {
                    const int c = GT + 16 * (oc + o) + col;
                    const float pv = a.pq[(size_t)tl[s] * a.ldpq + c];
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[s][o][r] = pv + a.pq[(size_t)jq[s][r] * a.ldpq + a.S + c];
                    accx[s][o] = pf_splat(0.f);
                }
#pragma unroll
            for (int cp = 0; cp < NCP; ++cp)
#pragma unroll
                for (int o = 0; o < OCH; ++o) {
                    const h8 wh = __builtin_bit_cast(h8, Wf[(((oc + o) * NCP + cp) * 2 + 0) * 64 + lane]);
                    const h8 wl = __builtin_bit_cast(h8, Wf[(((oc + o) * NCP + cp) * 2 + 1) * 64 + lane]);
#pragma unroll
                    for (int s = 0; s < TPW; ++s) {
                        acc[s][o] = pf_mfma_f16(fp[s][cp].h, wh, acc[s][o]);
                        accx[s][o] = pf_mfma_f16(fp[s][cp].l, wh, accx[s][o]);
                        accx[s][o] = pf_mfma_f16(fp[s][cp].h, wl, accx[s][o]);
                    }
                }
#pragma unroll
            for (int s = 0; s < TPW; ++s)
#pragma unroll
                for (int o = 0; o < OCH; ++o) {
                    const f4 v = acc[s][o] + accx[s][o] * PF_LO_INV;
                    float best = v[0];
                    int bk = 4 * q;
#pragma unroll
                    for (int r = 1; r < 4; ++r)
                        if (v[r] > best) { best = v[r]; bk = 4 * q + r; }
                    pf_xor_argmax<16, 32>(best, bk);
                    if (q == 0 && ok[s]) {
                        const size_t o0 = (size_t)tl[s] * ODIM + 16 * (oc + o) + col;
                        a.out[o0] = best;
                        a.arg[o0] = (unsigned char)bk;
                    }
                }
        }
    } else {
#pragma unroll
        for (int s = 0; s < TPW; ++s)
            if (ok[s] && col == 0)
                for (int c = 4 * q; c < ODIM; c += 16)
                    *reinterpret_cast<f4*>(a.out + (size_t)tl[s] * ODIM + c) = pf_splat(__builtin_nanf(""));
    }
    ecp_exit_reset(a.acc, a.sync, NC, &flag);
}

// ------------------------------------------------------------------------------------------------ weight folding / un-folding
// Wpq [2S, C], bpq [2S] = (bias | 0)
__global__ __launch_bounds__(256) void ec_fold_kernel(EcConvs cv, float* Wpq, float* bpq) {
    const int total = cv.S * cv.C;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int srow = i / cv.C, col = i % cv.C;
        int t = 0;
        while (t + 1 < cv.nconvs && srow >= cv.rowoff[t + 1]) ++t;
        const float* w = cv.W[t] + (size_t)(srow - cv.rowoff[t]) * cv.width[t];
        Wpq[(size_t)srow * cv.C + col] = w[col] - w[2 * cv.C + col];
        Wpq[(size_t)(cv.S + srow) * cv.C + col] = w[cv.C + col] + w[2 * cv.C + col];
        if (col == 0) { bpq[srow] = cv.bias[t][srow - cv.rowoff[t]]; bpq[cv.S + srow] = 0.f; }
    }
}
// The same fold for several units in ONE launch (pf_ec_train_fold_batch): Wpq / bpq depend on parameters only, so a training step
// folds all of its units before the first one runs instead of paying a 5 us launch at the head of every unit's forward.
constexpr int EC_FOLD_MAX = 8;
struct EcFoldOne {
    const float* W[9]; const float* bias[9];
    float* Wpq; float* bpq;
    int rowoff[10], width[9];
    int nconvs, C, S, pad;
};
struct EcFoldBatch { EcFoldOne u[EC_FOLD_MAX]; };
static_assert(sizeof(EcFoldBatch) <= 4032, "kernel argument block");
__global__ __launch_bounds__(256) void ec_fold_batch_kernel(EcFoldBatch fb) {
    const EcFoldOne& cv = fb.u[blockIdx.y];
    const int total = cv.S * cv.C;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int srow = i / cv.C, col = i % cv.C;
        int t = 0;
        while (t + 1 < cv.nconvs && srow >= cv.rowoff[t + 1]) ++t;
        const float* w = cv.W[t] + (size_t)(srow - cv.rowoff[t]) * cv.width[t];
        cv.Wpq[(size_t)srow * cv.C + col] = w[col] - w[2 * cv.C + col];
        cv.Wpq[(size_t)(cv.S + srow) * cv.C + col] = w[cv.C + col] + w[2 * cv.C + col];
        if (col == 0) { cv.bpq[srow] = cv.bias[t][srow - cv.rowoff[t]]; cv.bpq[cv.S + srow] = 0.f; }
    }
}

// ---- the unit's forward as ONE persistent launch (ec_fwdp_kernel): shapes it is instantiated for, and whether all of its
// workgroups can be resident at once on this device (grid barriers).  The caller's PF_EC_PERSISTENT flag is the promise that no
// OTHER barrier kernel of this process runs beside it (two barrier kernels can starve each other; ordinary kernels only delay it).
template <int G, int ODIM>
size_t ecp_lds_bytes() {
    size_t fl = 0;
    for (int t = 1; t < 4; ++t) fl += (size_t)((G + 15) / 16) * 16 * (((G * t + 15) & ~15) + 4);
    return fl * sizeof(float) + (size_t)(ODIM / 16) * (G * 4 / 32) * 2 * 64 * 16;
}
template <int G, int ODIM>
int ecp_capacity() {
    int ncu = 0;
    const int per_cu = resident_per_cu(ec_fwdp_kernel<G, 4, ODIM>, ECP_T, ecp_lds_bytes<G, ODIM>(), &ncu);
    const int want = ECP_TPW / ecp_tpw(G);          // workgroups per CU the unit's grid needs resident (2 for the narrow units)
    return (per_cu < want ? per_cu : want) * ncu;
}

}  // namespace

bool pf_ec_persistent_ok(const PfEcTrain* p, const EcDims& d) {
    if (!(p->flags & PF_EC_PERSISTENT) || (p->flags & PF_TRAIN_DETERMINISTIC) || !p->sync || !p->pooling || p->K != 16 || p->nconv != 4 ||
        p->sync_sums)
        return false;
    int cap = 0;
    if (p->growth == 8 && p->odim == 32) cap = ecp_capacity<8, 32>();
    else if (p->growth == 16 && p->odim == 64) cap = ecp_capacity<16, 64>();
    else if (p->growth == 32 && p->odim == 128) cap = ecp_capacity<32, 128>();
    return cap > 0 && (long long)d.ntiles <= (long long)cap * ECP_WAVES * ecp_tpw(p->growth);
}

namespace {

int ec_fwd_persistent(const PfEcTrain* p, const EcDims& d, const EcConvs& cv, hipStream_t s) {
    EcFwdPArgs a{};
    a.Y = p->Y; a.ldy = d.GT; a.aff = p->aff; a.pq = p->PQ; a.ldpq = 2 * d.S; a.S = d.S; a.idx = p->idx; a.N = p->N;
    a.ntiles = d.ntiles; a.slope = p->slope; a.out = p->out; a.arg = p->arg;
    for (int t = 0; t < p->nconv; ++t) {
        a.Wg[t] = p->W[t] + 3 * p->C; a.ldwg[t] = cv.width[t];
        a.gamma[t] = p->gamma[t]; a.beta[t] = p->beta[t]; a.run_mean[t] = p->run_mean[t]; a.run_var[t] = p->run_var[t];
    }
    a.Wout = p->W[p->nconv] + 3 * p->C; a.ldwout = cv.width[p->nconv];
    a.eps = p->eps; a.momentum = p->momentum; a.R = (double)d.E; a.acc = p->stat; a.sync = p->sync;
    const int grid = pf_ecp_grid(d, ecp_tpw(p->growth));
    const size_t l8 = ecp_lds_bytes<8, 32>(), l16 = ecp_lds_bytes<16, 64>(), l32 = ecp_lds_bytes<32, 128>();
    if (p->growth == 8) hipLaunchKernelGGL((ec_fwdp_kernel<8, 4, 32>), dim3(grid), dim3(ECP_T), l8, s, a);
    else if (p->growth == 16) hipLaunchKernelGGL((ec_fwdp_kernel<16, 4, 64>), dim3(grid), dim3(ECP_T), l16, s, a);
    else hipLaunchKernelGGL((ec_fwdp_kernel<32, 4, 128>), dim3(grid), dim3(ECP_T), l32, s, a);
    return pf_last_launch_status();
}

}  // namespace

extern "C" int pf_ec_train_fold_batch(const PfEcTrain* descs, int n, void* stream) {
    if (!descs) return PF_ERR_NULL;
    if (n < 1 || n > EC_FOLD_MAX) return PF_ERR_SHAPE;
    EcFoldBatch fb{};
    int most = 0;
    for (int k = 0; k < n; ++k) {
        const PfEcTrain* p = descs + k;
        EcDims d;
        const int st = pf_ec_dims(p, d);
        if (st) return st;
        if (!p->Wpq || !p->bpq) return PF_ERR_NULL;
        const EcConvs cv = pf_ec_convs(p, d);
        EcFoldOne& u = fb.u[k];
        for (int t = 0; t < d.nconvs; ++t) {
            if (!p->W[t] || !p->bias[t]) return PF_ERR_NULL;
            u.W[t] = cv.W[t]; u.bias[t] = cv.bias[t]; u.width[t] = cv.width[t]; u.rowoff[t] = cv.rowoff[t];
        }
        u.rowoff[d.nconvs] = cv.rowoff[d.nconvs];
        u.Wpq = p->Wpq; u.bpq = p->bpq; u.nconvs = d.nconvs; u.C = p->C; u.S = d.S;
        most = d.S * p->C > most ? d.S * p->C : most;
    }
    hipLaunchKernelGGL(ec_fold_batch_kernel, dim3((most + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, fb);
    return pf_last_launch_status();
}

extern "C" int pf_ec_train_fwd(const PfEcTrain* p, void* stream) {
    EcDims d;
    int st = pf_ec_dims(p, d);
    if (st) return st;
    if (!p->x || !p->idx || !p->Wpq || !p->bpq || !p->PQ || !p->Y || !p->aff || !p->out || !p->ws || !p->stat) return PF_ERR_NULL;
    if (p->pooling && !p->arg) return PF_ERR_NULL;
    for (int t = 0; t < d.nconvs; ++t)
        if (!p->W[t] || !p->bias[t]) return PF_ERR_NULL;
    for (int t = 0; t < p->nconv; ++t)
        if (!p->gamma[t] || !p->beta[t]) return PF_ERR_NULL;
    if (p->ws_floats < pf_ec_train_ws_floats(p)) return PF_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const EcConvs cv = pf_ec_convs(p, d);
    float* gws = p->ws + (long long)d.nchunk * d.S * (d.GT + 1);
    if (!(p->flags & PF_EC_PREFOLDED))
        hipLaunchKernelGGL(ec_fold_kernel, dim3((d.S * p->C + 255) / 256), dim3(256), 0, s, cv, p->Wpq, p->bpq);
    st = pf_gemm(p->x, p->C, 1, p->Wpq, 1, p->C, p->PQ, 2 * d.S, p->bpq, d.T, 2 * d.S, p->C, gws,
                 pf_gemm_ws_floats(d.T, 2 * d.S, p->C), stream);
    if (st) return st;
    const int g = p->growth;
    if (pf_ec_persistent_ok(p, d)) return ec_fwd_persistent(p, d, cv, s);
    EcFwdArgs a{};
    a.Y = p->Y; a.ldy = d.GT; a.aff = p->aff; a.pq = p->PQ; a.ldpq = 2 * d.S; a.idx = p->idx; a.N = p->N; a.K = p->K;
    a.ntiles = d.ntiles; a.slope = p->slope;
    for (int t = 0; t < p->nconv; ++t) {
        a.W = p->W[t] + 3 * p->C; a.ldw = cv.width[t]; a.poff = g * t; a.qoff = d.S + g * t;
        a.kin = g * t; a.col0 = g * t; a.nout = g;
        a.fin = StatFin{p->stat, 1, g, g * t, d.GT, p->aff, p->gamma[t], p->beta[t], p->run_mean[t], p->run_var[t], p->eps,
                        p->momentum, nullptr, nullptr, nullptr, (double)d.E, p->sync_sums};
        a.fin.det = PF_DET(p);
        const int kin16 = (a.kin + 15) & ~15;
        const int nt = g > 16 ? 2 : 1;
        const size_t lds = sizeof(float) * ((size_t)nt * 16 * (kin16 + 4) + 2 * kin16);
        if (nt == 2) hipLaunchKernelGGL((ec_fwd_kernel<2, false, false>), dim3(d.grid_light), dim3(256), lds, s, a);
        else hipLaunchKernelGGL((ec_fwd_kernel<1, false, false>), dim3(d.grid_light), dim3(256), lds, s, a);
        if ((st = pf_stat_sync(a.fin, g, p->sync_cb, p->sync_user, s))) return st;     // SyncBN: global statistics before the next layer
    }
    a.W = p->W[p->nconv] + 3 * p->C; a.ldw = cv.width[p->nconv]; a.poff = d.GT; a.qoff = d.S + d.GT;
    a.kin = d.GT; a.col0 = 0; a.nout = p->odim; a.out = p->out; a.arg = p->arg; a.fin = StatFin{};
    const int nto = p->odim / 16;
#ifdef PF_EC_FWD_F32
    const size_t lds = sizeof(float) * ((size_t)(nto <= 2 ? 2 : (nto <= 4 ? 4 : 8)) * 16 * (d.GT + 4) + 2 * d.GT);
#define PF_ECO(NT)                                                                                                        \
    do {                                                                                                                  \
        if (p->pooling) { allow_lds(ec_fwd_kernel<NT, true, true>, lds);                                                  \
            hipLaunchKernelGGL((ec_fwd_kernel<NT, true, true>), dim3(d.grid), dim3(256), lds, s, a); }                    \
        else { allow_lds(ec_fwd_kernel<NT, true, false>, lds);                                                            \
            hipLaunchKernelGGL((ec_fwd_kernel<NT, true, false>), dim3(d.grid), dim3(256), lds, s, a); }                   \
    } while (0)
#else
    const int nchk = (d.GT + 31) / 32;
    const size_t lds = (size_t)(nto <= 2 ? 2 : (nto <= 4 ? 4 : 8)) * nchk * 2 * 64 * 16 + sizeof(float) * 2 * nchk * 32;
#define PF_ECO(NT)                                                                                                        \
    do {                                                                                                                  \
        if (p->pooling) { allow_lds(ec_fwd16_kernel<NT, true>, lds);                                                      \
            hipLaunchKernelGGL((ec_fwd16_kernel<NT, true>), dim3(d.grid), dim3(256), lds, s, a); }                        \
        else { allow_lds(ec_fwd16_kernel<NT, false>, lds);                                                                \
            hipLaunchKernelGGL((ec_fwd16_kernel<NT, false>), dim3(d.grid), dim3(256), lds, s, a); }                       \
    } while (0)
#endif
    if (nto <= 2) PF_ECO(2); else if (nto <= 4) PF_ECO(4); else PF_ECO(8);
#undef PF_ECO
    return pf_last_launch_status();
}
