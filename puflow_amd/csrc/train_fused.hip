// Backward of one FeatureExtractUnit of the training step (pf_ec_train.h describes the whole unit): gradient of the dense block
// (per-layer gather form and the persistent one-launch form), dPQ, weight gradients, assembly; the unit's shape checks and
// workspace layout; the SyncBN finish of the column statistics (pf_train_stat.h).
#include "pf_ec_train.h"

namespace {

// SyncBN: the layer's constants from the all-reduced sums (defer[] as stat_flush left it, summed over the ranks by the host)
__global__ __launch_bounds__(STAT_W) void stat_finalize_kernel(StatFin f, int ncol) {
    const int c = threadIdx.x;
    if (c < ncol) stat_finish_col(f, c, f.defer[c], f.defer[STAT_W + c], f.defer[2 * STAT_W], false);
}

// ------------------------------------------------------------------------------------------------ backward, gather form
// The scatter form (ec_bwd_kernel, last in commit a5c3510) walked the convs from last to first and ADDED each one's contribution
// into the gradient columns of all earlier layers: the [E, GT] gradient tensor was read and rewritten once per layer (452 MB per
// 128-channel unit, 2.5 - 2.8 TB/s in every one of those kernels).  Here layer s GATHERS its own g columns from everything that
// consumes them, once:
//     G_s = dYout Wout[:, cols_s] + sum_{t > s} dy_t W_t[:, cols_s]
// with dy_t = BatchNorm + LeakyReLU backward of G_t (formed on load for t = s + 1, whose sums the previous launch finalised, and
// stored back; already in place for t > s + 1).  Same products, 4 + 4 + ... launches replaced by one per layer, every gradient
// column written once raw and once transformed: ~230 MB per unit.  Epilogue: the BatchNorm-backward sums of layer s.
// SRC 0: pooled unit, dYout[e, c] = dh[i, c] if argmax[i, c] == k else 0, formed on load; SRC 1: no pooling, dYout [E, odim] dense
struct EcBwdgArgs {
    const float* dh; const unsigned char* arg; const float* dyout; int odim;
    float* dA; const float* Y; int ld;
    const float* aff; const float* coef;
    const float* Wout; int ldwout;       // Wout[c * ldwout + col]: conv_out row c, growth column col (pointer offset by 3C)
    const float* Wg[8]; int ldwg[8];     // growth conv t: Wg[t][c * ldwg[t] + col]
    int s, nc, g, ntiles;
    float slope;
    StatFin fin;
};

template <int NTG, int SRC>
__global__ __launch_bounds__(256) void ec_bwdg_kernel(EcBwdgArgs a) {
    extern __shared__ float lds[];
    __shared__ float red[8 * STAT_W];
    const int g = a.g, g16 = (g + 15) & ~15, od16 = (a.odim + 15) & ~15;
    const int kpo = od16 + 4, kpg = g16 + 4, KSo = od16 / 16, KSg = g16 / 16;
    const int c0 = g * a.s, nsrc = a.nc - 1 - a.s;
    float* Wo = lds;                                   // Wo[u][c] = Wout[c][c0 + u]
    float* Wgl = Wo + NTG * 16 * kpo;                  // per later layer t: [NTG * 16][kpg], Wg_t[u][c] = Wg[t][c][c0 + u]
    float* cf = Wgl + nsrc * NTG * 16 * kpg;           // [6][g16]: scale, shift, mean, rstd, m1, m2 of layer s + 1
    for (int c = threadIdx.x >> 4; c < od16; c += 16) {
        float v[NTG];
#pragma unroll
        for (int k = 0; k < NTG; ++k) {
            const int u = (threadIdx.x & 15) + 16 * k;
            v[k] = (c < a.odim && u < g) ? a.Wout[(size_t)c * a.ldwout + c0 + u] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < NTG; ++k) Wo[((threadIdx.x & 15) + 16 * k) * kpo + c] = v[k];
    }
    for (int n = 0; n < nsrc; ++n) {
        const int t = a.s + 1 + n;
        const float* W = a.Wg[t];
        const int ldw = a.ldwg[t];
        float* dst = Wgl + n * NTG * 16 * kpg;
        for (int c = threadIdx.x >> 4; c < g16; c += 16) {
#pragma unroll
            for (int k = 0; k < NTG; ++k) {
                const int u = (threadIdx.x & 15) + 16 * k;
                dst[u * kpg + c] = (c < g && u < g) ? W[(size_t)c * ldw + c0 + u] : 0.f;
            }
        }
    }
    if (nsrc > 0) {
        const int c1 = c0 + g;
        for (int i = threadIdx.x; i < g16; i += 256) {
            const bool ok = i < g;
#pragma unroll
            for (int w = 0; w < 4; ++w) cf[w * g16 + i] = ok ? a.aff[w * a.ld + c1 + i] : 0.f;
            cf[4 * g16 + i] = ok ? a.coef[c1 + i] : 0.f;
            cf[5 * g16 + i] = ok ? a.coef[a.ld + c1 + i] : 0.f;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, q = lane >> 4;
    float s0[NTG], s1[NTG], ssc[NTG], ssh[NTG], smu[NTG], srs[NTG];
#pragma unroll
    for (int nt = 0; nt < NTG; ++nt) {
        s0[nt] = s1[nt] = 0.f;
        const int cl = nt * 16 + row;
        const bool ok = cl < g;
        ssc[nt] = ok ? a.aff[c0 + cl] : 0.f;
        ssh[nt] = ok ? a.aff[a.ld + c0 + cl] : 0.f;
        smu[nt] = ok ? a.aff[2 * a.ld + c0 + cl] : 0.f;
        srs[nt] = ok ? a.aff[3 * a.ld + c0 + cl] : 0.f;
    }
    for (int tile = blockIdx.x * 4 + wave; tile < a.ntiles; tile += gridDim.x * 4) {
        const long long e0 = (long long)tile * 16;
        // the tile's loads first: conv_out's gradient rows, then the later layers' gradient columns of this lane's edge
        f4 src[8];
        unsigned ag[SRC == 0 ? 8 : 1];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const int c = ks * 16 + 4 * q;
            src[ks] = pf_splat(0.f);
            if (ks < KSo && c < a.odim) {
                if (SRC == 0) {
                    src[ks] = *reinterpret_cast<const f4*>(a.dh + (long long)tile * a.odim + c);
                    ag[ks] = *reinterpret_cast<const unsigned*>(a.arg + (long long)tile * a.odim + c);
                } else src[ks] = *reinterpret_cast<const f4*>(a.dyout + (e0 + row) * a.odim + c);
            }
        }
        float* drow = a.dA + (e0 + row) * a.ld;
        f4 gsrc[7][2];
        f4 ysrc[2];
#pragma unroll
        for (int n = 0; n < 7; ++n)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                gsrc[n][ks] = pf_splat(0.f);
                const int c = ks * 16 + 4 * q;
                if (n < nsrc && ks < KSg && c < g) gsrc[n][ks] = *reinterpret_cast<const f4*>(drow + c0 + g * (n + 1) + c);
            }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            ysrc[ks] = pf_splat(0.f);
            const int c = ks * 16 + 4 * q;
            if (nsrc > 0 && ks < KSg && c < g) ysrc[ks] = *reinterpret_cast<const f4*>(a.Y + (e0 + row) * a.ld + c0 + g + c);
        }
        f4 acc[NTG];
#pragma unroll
        for (int nt = 0; nt < NTG; ++nt) acc[nt] = pf_splat(0.f);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            if (ks < KSo) {
                const int c = ks * 16 + 4 * q;
                f4 av = src[ks];
                if (SRC == 0) {
                    const f4 dv = src[ks];
                    const unsigned g4 = ag[ks];
                    av.x = (int)(g4 & 255u) == row ? dv.x : 0.f; av.y = (int)((g4 >> 8) & 255u) == row ? dv.y : 0.f;
                    av.z = (int)((g4 >> 16) & 255u) == row ? dv.z : 0.f; av.w = (int)(g4 >> 24) == row ? dv.w : 0.f;
                    if (c >= a.odim) av = pf_splat(0.f);
                }
#pragma unroll
                for (int nt = 0; nt < NTG; ++nt)
                    acc[nt] = mfma4(av, *reinterpret_cast<const f4*>(Wo + (nt * 16 + row) * kpo + c), acc[nt]);
            }
        }
#pragma unroll
        for (int n = 0; n < 7; ++n) {
            if (n < nsrc) {
                const float* Wt = Wgl + n * NTG * 16 * kpg;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    if (ks < KSg) {
                        const int c = ks * 16 + 4 * q;
                        f4 av = gsrc[n][ks];
                        if (n == 0 && c < g) {                      // layer s + 1: raw gradient -> dy, stored back
                            const f4 d = gsrc[0][ks], y = ysrc[ks];
                            const f4 sc = *reinterpret_cast<const f4*>(cf + c), sh = *reinterpret_cast<const f4*>(cf + g16 + c);
                            const f4 mu = *reinterpret_cast<const f4*>(cf + 2 * g16 + c), rs = *reinterpret_cast<const f4*>(cf + 3 * g16 + c);
                            const f4 m1 = *reinterpret_cast<const f4*>(cf + 4 * g16 + c), m2 = *reinterpret_cast<const f4*>(cf + 5 * g16 + c);
                            const f4 z = y * sc + sh;
                            const f4 xh = (y - mu) * rs;
#pragma unroll
                            for (int w = 0; w < 4; ++w) {
                                const float dz = d[w] * (z[w] > 0.f ? 1.f : a.slope);
                                av[w] = sc[w] * (dz - m1[w] - xh[w] * m2[w]);
                            }
                            *reinterpret_cast<f4*>(drow + c0 + g + c) = av;
                        }
#pragma unroll
                        for (int nt = 0; nt < NTG; ++nt)
                            acc[nt] = mfma4(av, *reinterpret_cast<const f4*>(Wt + (nt * 16 + row) * kpg + c), acc[nt]);
                    }
                }
            }
        }
#pragma unroll
        for (int nt = 0; nt < NTG; ++nt) {
            const int cl = nt * 16 + row;
            if (cl < g) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long long e = e0 + 4 * q + r;
                    const float v = acc[nt][r];
                    a.dA[e * a.ld + c0 + cl] = v;
                    const float y = a.Y[e * a.ld + c0 + cl];
                    const float dz = v * (fmaf(y, ssc[nt], ssh[nt]) > 0.f ? 1.f : a.slope);
                    s0[nt] += dz;
                    s1[nt] = fmaf(dz, (y - smu[nt]) * srs[nt], s1[nt]);
                }
            }
        }
    }
    stat_flush<NTG>(s0, s1, 0, g, a.fin, red);
}

// The same gather on the bf16 matrix pipe (both operands split as in ec_dw3_kernel: x = hi + mid, fp32 exponent range, three
// v_mfma_f32_16x16x32_bf16 per 32 channels instead of eight f32 MFMAs): lane (row = edge, kg = l >> 4) holds the 8 channels
// 8 kg .. 8 kg + 7 of a 32-channel chunk of its edge's gradient row (two 16-byte loads), the weights sit in LDS as ready
// fragments [tile][chunk][hi | mid][lane][8 x bf16] written once per workgroup.  Accumulators, epilogue and statistics are those of
// the f32 kernel (the 16x16 accumulator layout does not depend on the input type).
typedef __bf16 gbf8 __attribute__((ext_vector_type(8)));
struct GBf2 { gbf8 hi, mid; };
// Two floats rounded to bf16 (nearest, ties to even: the hardware's packed conversion), a in the low half of the word.  Both
// parts of a split are ROUNDED: with hi and mid truncated (a mask and a shift) every product came out short by ~4e-5 of itself,
// always towards zero, and through the six chained units of the extractor that bias added up to 2.8e-4 of the first unit's
// gradients against float64 (tests/test_gpu_extract_train.py); rounded, x - hi has either sign, what is left after mid is at
// most 2^-16 of x with mean zero, and so is the dropped mid mid product.  One v_cvt_pk_bf16_f32 per pair and part replaces the
// masks, shifts and ors of the truncating form (integer rounding by hand, add 0x7fff + lsb and mask, cost 2 % of the step).
typedef float gf2v __attribute__((ext_vector_type(2)));
typedef __bf16 gb2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned bf16_pair(float a, float b) {
    const gf2v v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, gb2v));
}
__device__ __forceinline__ GBf2 g_split(const float (&x)[8]) {
    unsigned hw[4], mw[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        hw[p] = bf16_pair(x[2 * p], x[2 * p + 1]);
        mw[p] = bf16_pair(x[2 * p] - __uint_as_float(hw[p] << 16), x[2 * p + 1] - __uint_as_float(hw[p] & 0xffff0000u));
    }
    GBf2 r;
    r.hi = __builtin_bit_cast(gbf8, *reinterpret_cast<const uint4*>(hw));
    r.mid = __builtin_bit_cast(gbf8, *reinterpret_cast<const uint4*>(mw));
    return r;
}

template <int NTG, int SRC>
__global__ __launch_bounds__(256) void ec_bwdg16_kernel(EcBwdgArgs a) {
    extern __shared__ float lds[];
    __shared__ float red[8 * STAT_W];
    const int g = a.g, g16 = (g + 15) & ~15;
    const int nco = (a.odim + 31) / 32, ncg = (g + 31) / 32;       // 32-channel chunks of conv_out / of a growth layer
    const int c0 = g * a.s, nsrc = a.nc - 1 - a.s;
    uint4* Wf = reinterpret_cast<uint4*>(lds);                    // fragments: ((frag * 2 + hi|mid) * 64 + lane), 16 bytes each
    const int nfrag = NTG * (nco + nsrc * ncg);                   // frag = nt * nco + chunk | NTG * nco + (n * NTG + nt) * ncg + chunk
    float* cf = lds + (size_t)nfrag * 2 * 64 * 4;                 // [6][g16]: scale, shift, mean, rstd, m1, m2 of layer s + 1
    for (int unit = threadIdx.x; unit < nfrag * 64; unit += 256) {
        const int frag = unit >> 6, ln = unit & 63, u = ln & 15, kg = ln >> 4;
        const float* W;
        int ldw, kin, nt, chunk;
        if (frag < NTG * nco) { nt = frag / nco; chunk = frag % nco; W = a.Wout; ldw = a.ldwout; kin = a.odim; }
        else {
            const int f2 = frag - NTG * nco, n = f2 / (NTG * ncg), r2 = f2 % (NTG * ncg);
            nt = r2 / ncg; chunk = r2 % ncg; W = a.Wg[a.s + 1 + n]; ldw = a.ldwg[a.s + 1 + n]; kin = g;
        }
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = chunk * 32 + 8 * kg + j, uu = nt * 16 + u;
            v[j] = (c < kin && uu < g) ? W[(size_t)c * ldw + c0 + uu] : 0.f;
        }
        const GBf2 f = g_split(v);
        Wf[(frag * 2 + 0) * 64 + ln] = __builtin_bit_cast(uint4, f.hi);
        Wf[(frag * 2 + 1) * 64 + ln] = __builtin_bit_cast(uint4, f.mid);
    }
    if (nsrc > 0) {
        const int c1 = c0 + g;
        for (int i = threadIdx.x; i < g16; i += 256) {
            const bool ok = i < g;
#pragma unroll
            for (int w = 0; w < 4; ++w) cf[w * g16 + i] = ok ? a.aff[w * a.ld + c1 + i] : 0.f;
            cf[4 * g16 + i] = ok ? a.coef[c1 + i] : 0.f;
            cf[5 * g16 + i] = ok ? a.coef[a.ld + c1 + i] : 0.f;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, q = lane >> 4;
    float s0[NTG], s1[NTG], ssc[NTG], ssh[NTG], smu[NTG], srs[NTG];
#pragma unroll
    for (int nt = 0; nt < NTG; ++nt) {
        s0[nt] = s1[nt] = 0.f;
        const int cl = nt * 16 + row;
        const bool ok = cl < g;
        ssc[nt] = ok ? a.aff[c0 + cl] : 0.f;
        ssh[nt] = ok ? a.aff[a.ld + c0 + cl] : 0.f;
        smu[nt] = ok ? a.aff[2 * a.ld + c0 + cl] : 0.f;
        srs[nt] = ok ? a.aff[3 * a.ld + c0 + cl] : 0.f;
    }
    auto mma = [&](const GBf2& A, int frag, f4& acc) {
        const gbf8 bh = __builtin_bit_cast(gbf8, Wf[(frag * 2 + 0) * 64 + lane]);
        const gbf8 bm = __builtin_bit_cast(gbf8, Wf[(frag * 2 + 1) * 64 + lane]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A.mid, bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A.hi, bm, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A.hi, bh, acc, 0, 0, 0);
    };
    for (int tile = blockIdx.x * 4 + wave; tile < a.ntiles; tile += gridDim.x * 4) {
        const long long e0 = (long long)tile * 16;
        // the tile's loads first: 8 channels per 32-channel chunk of conv_out's gradient row and of the later layers' columns
        float csrc[4][8];
        unsigned ag[SRC == 0 ? 4 : 1][2];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const int c = ch * 32 + 8 * q;
#pragma unroll
            for (int j = 0; j < 8; ++j) csrc[ch][j] = 0.f;
            if (ch < nco && c < a.odim) {                            // odim is a multiple of 16: an 8-channel group is all in or all out
                const float* sp = SRC == 0 ? a.dh + (long long)tile * a.odim + c : a.dyout + (e0 + row) * a.odim + c;
                const f4 v0 = *reinterpret_cast<const f4*>(sp), v1 = *reinterpret_cast<const f4*>(sp + 4);
                csrc[ch][0] = v0.x; csrc[ch][1] = v0.y; csrc[ch][2] = v0.z; csrc[ch][3] = v0.w;
                csrc[ch][4] = v1.x; csrc[ch][5] = v1.y; csrc[ch][6] = v1.z; csrc[ch][7] = v1.w;
                if (SRC == 0) {
                    const unsigned* apw = reinterpret_cast<const unsigned*>(a.arg + (long long)tile * a.odim + c);
                    ag[ch][0] = apw[0]; ag[ch][1] = apw[1];
                }
            }
        }
        float* drow = a.dA + (e0 + row) * a.ld;
        float gsrc[7][8], ysrc[8];
        const int cq = 8 * q;                                      // g <= 32: one chunk per growth layer
#pragma unroll
        for (int n = 0; n < 7; ++n) {
#pragma unroll
            for (int j = 0; j < 8; ++j) gsrc[n][j] = 0.f;
            if (n < nsrc && cq < g) {                              // g is a multiple of 8
                const float* sp = drow + c0 + g * (n + 1) + cq;
                const f4 v0 = *reinterpret_cast<const f4*>(sp), v1 = *reinterpret_cast<const f4*>(sp + 4);
                gsrc[n][0] = v0.x; gsrc[n][1] = v0.y; gsrc[n][2] = v0.z; gsrc[n][3] = v0.w;
                gsrc[n][4] = v1.x; gsrc[n][5] = v1.y; gsrc[n][6] = v1.z; gsrc[n][7] = v1.w;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) ysrc[j] = 0.f;
        if (nsrc > 0 && cq < g) {
            const float* sp = a.Y + (e0 + row) * a.ld + c0 + g + cq;
            const f4 v0 = *reinterpret_cast<const f4*>(sp), v1 = *reinterpret_cast<const f4*>(sp + 4);
            ysrc[0] = v0.x; ysrc[1] = v0.y; ysrc[2] = v0.z; ysrc[3] = v0.w; ysrc[4] = v1.x; ysrc[5] = v1.y; ysrc[6] = v1.z; ysrc[7] = v1.w;
        }
        f4 acc[NTG];
#pragma unroll
        for (int nt = 0; nt < NTG; ++nt) acc[nt] = pf_splat(0.f);
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            if (ch < nco) {
                float av[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    av[j] = csrc[ch][j];
                    if (SRC == 0) {
                        const unsigned wv = ag[ch][j >> 2];
                        av[j] = (int)((wv >> (8 * (j & 3))) & 255u) == row ? csrc[ch][j] : 0.f;
                    }
                }
                const GBf2 A = g_split(av);
#pragma unroll
                for (int nt = 0; nt < NTG; ++nt) mma(A, nt * nco + ch, acc[nt]);
            }
        }
#pragma unroll
        for (int n = 0; n < 7; ++n) {
            if (n < nsrc) {
                float av[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) av[j] = gsrc[n][j];
                if (n == 0 && cq < g) {                            // layer s + 1: raw gradient -> dy, stored back
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int c = cq + j;
                        const float sc = cf[c], sh = cf[g16 + c], mu = cf[2 * g16 + c], rs = cf[3 * g16 + c];
                        const float m1 = cf[4 * g16 + c], m2 = cf[5 * g16 + c];
                        const float y = ysrc[j], z = fmaf(y, sc, sh), xh = (y - mu) * rs;
                        const float dz = gsrc[0][j] * (z > 0.f ? 1.f : a.slope);
                        av[j] = sc * (dz - m1 - xh * m2);
                    }
                    float* dp = drow + c0 + g + cq;
                    f4 o0 = {av[0], av[1], av[2], av[3]}, o1 = {av[4], av[5], av[6], av[7]};
                    *reinterpret_cast<f4*>(dp) = o0;
                    *reinterpret_cast<f4*>(dp + 4) = o1;
                }
                const GBf2 A = g_split(av);
#pragma unroll
                for (int nt = 0; nt < NTG; ++nt) mma(A, NTG * nco + (n * NTG + nt) * ncg, acc[nt]);
            }
        }
#pragma unroll
        for (int nt = 0; nt < NTG; ++nt) {
            const int cl = nt * 16 + row;
            if (cl < g) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long long e = e0 + 4 * q + r;
                    const float v = acc[nt][r];
                    a.dA[e * a.ld + c0 + cl] = v;
                    const float y = a.Y[e * a.ld + c0 + cl];
                    const float dz = v * (fmaf(y, ssc[nt], ssh[nt]) > 0.f ? 1.f : a.slope);
                    s0[nt] += dz;
                    s1[nt] = fmaf(dz, (y - smu[nt]) * srs[nt], s1[nt]);
                }
            }
        }
    }
    stat_flush<NTG>(s0, s1, 0, g, a.fin, red);
}

// ------------------------------------------------------------------------------------------------ backward of the dense block in ONE launch
// The gather-form backward above is one launch per growth layer (+ ec_bwd0_kernel): layer s reads conv_out's gradient and the dy
// of EVERY later layer from memory again, and each launch ends in the BatchNorm-backward sums of its layer.  Same construction
// as ec_fwdp_kernel: a persistent grid (one workgroup per CU, 8 waves, a wave owns up to ECP_TPW tiles for the whole launch) keeps
// the tile's dy of the layers done so far in registers and meets at a grid barrier once per layer:
//   layer s = NC-1 .. 0:  G_s = dYout Wout[:, cols_s] + sum_{t > s} dy_t W_t[:, cols_s]   (channel-major: the columns of layer s on
//                          the MFMA rows, edges on the columns - a dy tile is the B operand of every earlier layer as it stands;
//                          split-bf16 products like ec_bwdg16_kernel: x = hi + mid, three v_mfma_f32_16x16x32_bf16 per 32
//                          channels; the weights are split once per workgroup into A fragments in LDS; dYout is formed from
//                          (dh, argmax) on load)
//                        dz = G_s lrelu'(bn(y_s));  sums of dz and dz xhat -> barrier -> dy_s = scale (dz - m1 - xhat m2), kept in
//                          registers for the layers below and stored ONCE to dA (the weight-gradient and dPQ kernels read it).
// dA ends up exactly as ec_bwd0_kernel leaves it; coef / dgamma / dbeta are written by workgroup 0.
struct EcBwdPArgs {
    const float* dh; const unsigned char* arg;       // [T, ODIM]
    float* dA; const float* Y; int ld;               // [E, GT]
    const float* aff; float* coef;                   // [4][GT], [2][GT]
    const float* Wout; int ldwout;
    const float* Wg[8]; int ldwg[8];
    float* dgamma[8]; float* dbeta[8];
    int ntiles;
    float slope; double R;
    double* acc; unsigned* sync;
    float* dP; int ldp;                              // nullable: dPQ [T, ldp] - the P half's growth columns = sum of dA over a point's 16 edges
};

template <int G, int NC, int ODIM>
__global__ __launch_bounds__(ECP_T) void ec_bwdp_kernel(EcBwdPArgs a) {
    constexpr int TPW = ecp_tpw(G);
    constexpr int GT = G * NC, NB = GT / 16, NTG = (G + 15) / 16, NCO = ODIM / 32, NCP = GT / 32;
    constexpr bool OWN = G % 16 == 0;
    static_assert(GT % 32 == 0 && ODIM % 32 == 0 && 32 * NC <= STAT_W && G <= 32, "shape");
    // no aligned(16) here: every kernel of a source shares ONE dynamic LDS symbol and it stayed 4-byte aligned while this kernel
    // asked for 16 below the per-layer kernels' plain declaration (the request never took effect; the fragments are read with
    // unaligned-capable LDS instructions).  Honouring it moves the buffer by 12 bytes and changes the code of every kernel that
    // uses `lds`: a change to measure on its own.
    extern __shared__ float lds[];
    __shared__ float red[ECP_WAVES * 2 * 32];
    __shared__ float m12[2 * 32];
    __shared__ float bnc2[2][4 * 32];     // double-buffered by layer parity: a wave may enter the next layer while another still reads
    __shared__ int flag;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, q = lane >> 4;
    // ---- A fragments (split-bf16, [hi | mid][lane] x 16 B): first conv_out's, one per (16-column block b of the growth
    // channels, 32-channel chunk co of odim) - Wout[c][16 b + row] - then per layer s its dy chunks cp >= cpmin(s) (32 growth
    // channels each: rows of the LATER layers' convs, zero for channels of layers <= s): frag fbase(s) + nt * ndy(s) + (cp - cpmin(s))
    auto cpmin = [](int s) { return (G * (s + 1)) / 32; };
    auto ndy = [&](int s) { return NCP - cpmin(s); };
    int fbase[NC + 1];
    fbase[0] = NB * NCO;
#pragma unroll
    for (int s = 0; s < NC; ++s) fbase[s + 1] = fbase[s] + NTG * ndy(s);
#ifdef PF_EC_BWDG_F32
    // A/B build (bench.py grad_parity): the SAME kernel on plain f32 products - fp32 images [row][k] with row = growth column,
    // k = source channel: Wo [GT][ODIM + 4] (conv_out), Ms [NC][NTG * 16][GT + 4] (the later layers' rows, zero for layers <= s)
    constexpr int KPO = ODIM + 4, KPG = GT + 4;
    float* Wo = lds;
    float* Ms = lds + GT * KPO;
    for (int i = threadIdx.x; i < GT * ODIM; i += ECP_T) Wo[(i % GT) * KPO + i / GT] = a.Wout[(size_t)(i / GT) * a.ldwout + i % GT];
    for (int i = threadIdx.x; i < NC * NTG * 16 * GT; i += ECP_T) {
        const int s = i / (NTG * 16 * GT), rw = (i / GT) % (NTG * 16), c = i % GT, t = c / G;
        const int ug = 16 * ((G * s) / 16) + rw;
        Ms[(s * NTG * 16 + rw) * KPG + c] = (ug >= G * s && ug < G * (s + 1) && t > s) ? a.Wg[t][(size_t)(c - G * t) * a.ldwg[t] + ug] : 0.f;
    }
#else
    uint4* Wf = reinterpret_cast<uint4*>(lds);
    {
        const int nunit = fbase[NC] * 64;
        constexpr int MAXU = ((NB * NCO + NTG * NC * NCP) * 64 + ECP_T - 1) / ECP_T;
        float v[MAXU][8];
#pragma unroll
        for (int k = 0; k < MAXU; ++k) {
            const int unit = threadIdx.x + k * ECP_T, uu = unit < nunit ? unit : 0;
            const int frag = uu >> 6, ln = uu & 63, row = ln & 15, kq = ln >> 4;
            if (frag < NB * NCO) {
                const int b = frag / NCO, co = frag % NCO, ug = 16 * b + row;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    v[k][j] = a.Wout[(size_t)(32 * co + (j < 4 ? 0 : 16) + 4 * kq + (j & 3)) * a.ldwout + ug];
            } else {
                int s = 0;
#pragma unroll
                for (int t = 1; t < NC; ++t) s = frag >= fbase[t] ? t : s;
                const int fr = frag - fbase[s], nd = ndy(s) > 0 ? ndy(s) : 1, nt = fr / nd, cp = cpmin(s) + fr % nd;
                const int b0 = (G * s) / 16, ug = 16 * (b0 + nt) + row;             // growth column of this output row
                const bool rowok = ug >= G * s && ug < G * (s + 1);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = 32 * cp + (j < 4 ? 0 : 16) + 4 * kq + (j & 3), t = c / G;
                    v[k][j] = (rowok && t > s) ? a.Wg[t][(size_t)(c - G * t) * a.ldwg[t] + ug] : 0.f;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < MAXU; ++k) {
            const int unit = threadIdx.x + k * ECP_T;
            if (unit < nunit) {
                const GBf2 f2 = g_split(v[k]);
                Wf[((unit >> 6) * 2 + 0) * 64 + (unit & 63)] = __builtin_bit_cast(uint4, f2.hi);
                Wf[((unit >> 6) * 2 + 1) * 64 + (unit & 63)] = __builtin_bit_cast(uint4, f2.mid);
            }
        }
    }
#endif
    // ---- this wave's tiles
    int tl[TPW];
    bool ok[TPW];
#pragma unroll
    for (int s = 0; s < TPW; ++s) {
        tl[s] = blockIdx.x * ECP_WAVES + wave + s * gridDim.x * ECP_WAVES;
        ok[s] = tl[s] < a.ntiles;
        tl[s] = ok[s] ? tl[s] : 0;
    }
    f4 dy[TPW][NB];
#pragma unroll
    for (int s = 0; s < TPW; ++s)
#pragma unroll
        for (int b = 0; b < NB; ++b) dy[s][b] = pf_splat(0.f);
    __syncthreads();
#ifndef PF_EC_BWDG_F32
    auto mma = [&](int frag, const GBf2& B, f4& acc) {
        const gbf8 wh = __builtin_bit_cast(gbf8, Wf[(frag * 2 + 0) * 64 + lane]);
        const gbf8 wm = __builtin_bit_cast(gbf8, Wf[(frag * 2 + 1) * 64 + lane]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wm, B.hi, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, B.mid, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, B.hi, acc, 0, 0, 0);
    };
#endif

    // ---- conv_out's contribution to EVERY layer in one pass: dy[.][b] = Wout[:, 16 b ..]^T dYout, dYout formed from (dh, argmax)
    // and split once per (tile, chunk) - this lane's 8 channels of a 32-channel chunk, edge = col.  Layer s adds the later
    // layers' part into its own slots below.
#pragma unroll
    for (int co = 0; co < NCO; ++co) {
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const float* dp = a.dh + (size_t)tl[t] * ODIM + 32 * co + 4 * q;
            const unsigned char* ap = a.arg + (size_t)tl[t] * ODIM + 32 * co + 4 * q;
            const f4 d0 = *reinterpret_cast<const f4*>(dp), d1 = *reinterpret_cast<const f4*>(dp + 16);
            const unsigned g0 = *reinterpret_cast<const unsigned*>(ap), g1 = *reinterpret_cast<const unsigned*>(ap + 16);
            float x[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x[j] = (int)((g0 >> (8 * j)) & 255u) == col ? d0[j] : 0.f;
                x[4 + j] = (int)((g1 >> (8 * j)) & 255u) == col ? d1[j] : 0.f;
            }
#ifdef PF_EC_BWDG_F32
            const f4 x0 = {x[0], x[1], x[2], x[3]}, x1 = {x[4], x[5], x[6], x[7]};
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                dy[t][b] = mfma4(*reinterpret_cast<const f4*>(Wo + (16 * b + col) * KPO + 32 * co + 4 * q), x0, dy[t][b]);
                dy[t][b] = mfma4(*reinterpret_cast<const f4*>(Wo + (16 * b + col) * KPO + 32 * co + 16 + 4 * q), x1, dy[t][b]);
            }
#else
            const GBf2 B = g_split(x);
#pragma unroll
            for (int b = 0; b < NB; ++b) mma(b * NCO + co, B, dy[t][b]);
#endif
        }
    }

    bool alive = true;
    pf_static_for<0, NC>([&](auto sc_) {
        constexpr int s = NC - 1 - decltype(sc_)::value;             // layers last to first
        constexpr int col0 = G * s, b0 = col0 / 16, CP0 = (G * (s + 1)) / 32, NDY = NCP - CP0;
        if (!alive) return;
        const int fb = fbase[s];
        // the layer's BatchNorm constants (scale, shift, mean, 1/std) as f4 rows in LDS: read when needed, not held in registers
        float* bnc = bnc2[s & 1];
        if (threadIdx.x < 4 * 32) {
            const int w = threadIdx.x >> 5, c = threadIdx.x & 31;
            bnc[w * 32 + c] = c < G ? a.aff[w * a.ld + col0 + c] : 0.f;
        }
        bool cv[NTG];
        f4 yv[TPW][NTG], accs[OWN ? 1 : TPW][NTG];
        auto A = [&](int t, int nt) -> f4& {
            if constexpr (OWN) return dy[t][b0 + nt];                // the layer's own slots hold conv_out's part already
            else return accs[t][nt];
        };
#pragma unroll
        for (int nt = 0; nt < NTG; ++nt) {
            const int c4 = 16 * (b0 + nt) + 4 * q;
            cv[nt] = c4 >= col0 && c4 < col0 + G;
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                yv[t][nt] = pf_splat(0.f);
                if (cv[nt] && ok[t]) yv[t][nt] = *reinterpret_cast<const f4*>(a.Y + ((size_t)tl[t] * 16 + col) * a.ld + c4);
                if constexpr (!OWN) accs[t][nt] = cv[nt] ? dy[t][b0 + nt] : pf_splat(0.f);   // rows of the layer that shares the block: not ours
            }
        }
        // ---- the later layers' dy (registers)
#pragma unroll
        for (int cp = CP0; cp < NCP; ++cp) {
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
#ifdef PF_EC_BWDG_F32
#pragma unroll
                for (int nt = 0; nt < NTG; ++nt) {
                    const float* mrow = Ms + ((size_t)s * NTG * 16 + nt * 16 + col) * KPG + 32 * cp + 4 * q;
                    A(t, nt) = mfma4(*reinterpret_cast<const f4*>(mrow), dy[t][2 * cp], A(t, nt));
                    A(t, nt) = mfma4(*reinterpret_cast<const f4*>(mrow + 16), dy[t][2 * cp + 1], A(t, nt));
                }
#else
                float x[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) { x[j] = dy[t][2 * cp][j]; x[4 + j] = dy[t][2 * cp + 1][j]; }
                const GBf2 B = g_split(x);
#pragma unroll
                for (int nt = 0; nt < NTG; ++nt) mma(fb + nt * NDY + cp - CP0, B, A(t, nt));
#endif
            }
        }
        __syncthreads();                                              // bnc
        // ---- dz (it replaces the raw gradient), its sums; xhat stays for the transform behind the barrier
        f4 s0[NTG], s1[NTG], xh[TPW][NTG];
#pragma unroll
        for (int nt = 0; nt < NTG; ++nt) {
            s0[nt] = s1[nt] = pf_splat(0.f);
            const int cl = cv[nt] ? 16 * (b0 + nt) + 4 * q - col0 : 0;
            const f4 bsc = *reinterpret_cast<const f4*>(bnc + cl), bsh = *reinterpret_cast<const f4*>(bnc + 32 + cl);
            const f4 bmu = *reinterpret_cast<const f4*>(bnc + 64 + cl), brs = *reinterpret_cast<const f4*>(bnc + 96 + cl);
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                const f4 y = yv[t][nt], z = y * bsc + bsh;
                xh[t][nt] = (y - bmu) * brs;
                f4 dz;
#pragma unroll
                for (int r = 0; r < 4; ++r) dz[r] = A(t, nt)[r] * (z[r] > 0.f ? 1.f : a.slope);
                if (cv[nt]) {
                    A(t, nt) = dz;
                    if (ok[t]) { s0[nt] = s0[nt] + dz; s1[nt] = s1[nt] + dz * xh[t][nt]; }
                }
            }
        }
        ecp_stat_publish<G>(s0, s1, b0, col0, s, a.acc, red, true);
        alive = ecp_barrier(a.sync, (unsigned)(NC - s), &flag);
        if (!alive) return;
        const EcpSums sums = ecp_stat_fetch(a.acc, s);
        const double part = sums.part, other = sums.other;
        if (threadIdx.x < 256 && (threadIdx.x & 7) == 0 && (threadIdx.x >> 3) < G) {
            const int c = threadIdx.x >> 3;
            m12[c] = (float)(part / a.R);
            m12[32 + c] = (float)(other / a.R);
            if (blockIdx.x == 0) {                                    // the StatFin mode-2 outputs
                a.coef[col0 + c] = (float)(part / a.R);
                a.coef[a.ld + col0 + c] = (float)(other / a.R);
                a.dbeta[s][c] = (float)part;
                a.dgamma[s][c] = (float)other;
            }
        }
        __syncthreads();
#pragma unroll
        for (int nt = 0; nt < NTG; ++nt) {
            if (!cv[nt]) continue;
            const int cl = 16 * (b0 + nt) + 4 * q - col0;
            const f4 m1 = *reinterpret_cast<const f4*>(m12 + cl), m2 = *reinterpret_cast<const f4*>(m12 + 32 + cl);
            const f4 bsc = *reinterpret_cast<const f4*>(bnc + cl);
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                const f4 v = bsc * (A(t, nt) - m1 - xh[t][nt] * m2);
                if (ok[t]) *reinterpret_cast<f4*>(a.dA + ((size_t)tl[t] * 16 + col) * a.ld + 16 * (b0 + nt) + 4 * q) = v;
                dy[t][b0 + nt] = v;
                // a tile = the 16 edges of ONE point (K = 16), an edge = a lane of the 16-lane row: the sum over the row IS the point's
                // dP for these columns - the column sums ec_pq_bwd_csr_kernel otherwise reads all of dA again for (67 MB per 128-wide unit)
                if (a.dP) {
                    f4 ps;
#pragma unroll
                    for (int r = 0; r < 4; ++r) ps[r] = ecp_rowsum16(v[r]);
                    if (ok[t] && col == 0) *reinterpret_cast<f4*>(a.dP + (size_t)tl[t] * a.ldp + 16 * (b0 + nt) + 4 * q) = ps;
                }
            }
        }
    });
    if (!alive) {                                                     // loud: the layers that were not finished
#pragma unroll
        for (int t = 0; t < TPW; ++t)
            if (ok[t])
                for (int c = 4 * q; c < GT; c += 16)
                    *reinterpret_cast<f4*>(a.dA + ((size_t)tl[t] * 16 + col) * a.ld + c) = pf_splat(__builtin_nanf(""));
    }
    ecp_exit_reset(a.acc, a.sync, NC, &flag);
}

// growth layer 0 has no growth input: only dA[:, 0:g] -> dy in place
__global__ __launch_bounds__(256) void ec_bwd0_kernel(float* dA, const float* Y, int ld, const float* aff, const float* coef, int g,
                                                      long long E, float slope) {
    const int g4 = g / 4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < E * g4; i += (long long)gridDim.x * 256) {
        const long long e = i / g4;
        const int c = (int)(i % g4) * 4;
        float* dp = dA + e * ld + c;
        const f4 d = *reinterpret_cast<const f4*>(dp);
        const f4 y = *reinterpret_cast<const f4*>(Y + e * ld + c);
        f4 o;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float sc = aff[c + w], z = fmaf(y[w], sc, aff[ld + c + w]);
            const float xh = (y[w] - aff[2 * ld + c + w]) * aff[3 * ld + c + w];
            const float dz = d[w] * (z > 0.f ? 1.f : slope);
            o[w] = sc * (dz - coef[c + w] - xh * coef[ld + c + w]);
        }
        *reinterpret_cast<f4*>(dp) = o;
    }
}

// ------------------------------------------------------------------------------------------------ dPQ
// dPQ [T, 2S]: P half written (sum over the K edges of a point), Q half accumulated with atomics (zeroed by the caller).
// columns 0..GT-1: growth layers (dY = the in-place converted dA), GT..S-1: conv_out (pooled: from dh / argmax).
struct EcPqBwdArgs {
    const float* dY; int ld;         // [E, ld = GT]
    const float* dh; const unsigned char* arg; const float* dyout; int pooled;
    const int* idx;
    int N, K, GT, odim, S;
    long long T;
    float* dPQ;                      // [T, 2S]
};
__global__ __launch_bounds__(256) void ec_pq_bwd_kernel(EcPqBwdArgs a) {
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < a.T * a.S; t += (long long)gridDim.x * 256) {
        const long long i = t / a.S;
        const int c = (int)(t % a.S);
        const long long base = (i / a.N) * a.N;
        float* dq = a.dPQ + a.S + c;
        float sum = 0.f;
        if (c < a.GT) {
            for (int k = 0; k < a.K; ++k) {
                const long long e = i * a.K + k;
                const float v = a.dY[e * a.ld + c];
                sum += v;
                atomicAdd(dq + (base + a.idx[e]) * 2 * a.S, v);
            }
        } else if (a.pooled) {
            const int co = c - a.GT;
            sum = a.dh[i * a.odim + co];
            const long long e = i * a.K + a.arg[i * a.odim + co];
            atomicAdd(dq + (base + a.idx[e]) * 2 * a.S, sum);
        } else {
            const int co = c - a.GT;
            for (int k = 0; k < a.K; ++k) {
                const long long e = i * a.K + k;
                const float v = a.dyout[e * a.odim + co];
                sum += v;
                atomicAdd(dq + (base + a.idx[e]) * 2 * a.S, v);
            }
        }
        a.dPQ[i * 2 * a.S + c] = sum;
    }
}

// The same without atomics, given the transposed neighbour lists (built once per step, pf_knn_csr): in-edges of point j are
// csr_edge[csr_off[j] .. csr_off[j+1]).  dQ[j] = sum over them (plain loads, coalesced over the channels), dP as above; the
// caller need not clear dPQ.
struct EcPqCsrArgs {
    EcPqBwdArgs b;
    const int* off; const int* edge;
    int p_done;                                      // the P half's growth columns were written by ec_bwdp_kernel
};
__global__ __launch_bounds__(256) void ec_pq_bwd_csr_kernel(EcPqCsrArgs a) {
    // one thread per (point, 4 channels): float4 loads, four edges in flight per accumulation step (a scalar thread per channel
    // with one load per dependent add ran at 2.2 TB/s with 86 % of its wave cycles waiting)
    const EcPqBwdArgs& b = a.b;
    const int S4 = b.S / 4;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < b.T * S4; t += (long long)gridDim.x * 256) {
        const int i = (int)(t / S4);
        const int c = (int)(t % S4) * 4;
        const int lo = a.off[i], hi = a.off[i + 1];
        f4 sum = pf_splat(0.f), q = pf_splat(0.f);
        if (c < b.GT || !b.pooled) {
            const float* src = c < b.GT ? b.dY + c : b.dyout + (c - b.GT);
            const size_t ld = c < b.GT ? (size_t)b.ld : (size_t)b.odim;
            const float* own = src + (size_t)i * b.K * ld;
            f4 s1 = pf_splat(0.f), s2 = pf_splat(0.f), s3 = pf_splat(0.f);
            const bool have_p = a.p_done && c < b.GT;
            int k = have_p ? b.K : 0;
            for (; k + 3 < b.K; k += 4) {
                const f4 v0 = *reinterpret_cast<const f4*>(own + (size_t)k * ld), v1 = *reinterpret_cast<const f4*>(own + (size_t)(k + 1) * ld);
                const f4 v2 = *reinterpret_cast<const f4*>(own + (size_t)(k + 2) * ld), v3 = *reinterpret_cast<const f4*>(own + (size_t)(k + 3) * ld);
                sum += v0; s1 += v1; s2 += v2; s3 += v3;
            }
            for (; k < b.K; ++k) sum += *reinterpret_cast<const f4*>(own + (size_t)k * ld);
            sum = (sum + s1) + (s2 + s3);
            f4 q1 = pf_splat(0.f), q2 = pf_splat(0.f), q3 = pf_splat(0.f);
            int n = lo;
            for (; n + 3 < hi; n += 4) {
                const int e0 = a.edge[n], e1 = a.edge[n + 1], e2 = a.edge[n + 2], e3 = a.edge[n + 3];
                const f4 v0 = *reinterpret_cast<const f4*>(src + (size_t)e0 * ld), v1 = *reinterpret_cast<const f4*>(src + (size_t)e1 * ld);
                const f4 v2 = *reinterpret_cast<const f4*>(src + (size_t)e2 * ld), v3 = *reinterpret_cast<const f4*>(src + (size_t)e3 * ld);
                q += v0; q1 += v1; q2 += v2; q3 += v3;
            }
            for (; n < hi; ++n) q += *reinterpret_cast<const f4*>(src + (size_t)a.edge[n] * ld);
            q = (q + q1) + (q2 + q3);
        } else {
            const int co = c - b.GT;
            sum = *reinterpret_cast<const f4*>(b.dh + (size_t)i * b.odim + co);
            // the pooled gradient reaches this point through the edges whose argmax it is: four edges in flight (edge id -> its
            // point's argmax word and gradient row: two dependent loads per edge - one edge at a time was the kernel's longest chain)
            auto take = [&](int e, unsigned g4, const f4& dv) {
                const int k = e - (e / b.K) * b.K;
                if ((int)(g4 & 255u) == k) q.x += dv.x;
                if ((int)((g4 >> 8) & 255u) == k) q.y += dv.y;
                if ((int)((g4 >> 16) & 255u) == k) q.z += dv.z;
                if ((int)(g4 >> 24) == k) q.w += dv.w;
            };
            int n = lo;
            for (; n + 3 < hi; n += 4) {
                int e[4];
                unsigned g4[4];
                f4 dv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) e[u] = a.edge[n + u];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const size_t ii = (size_t)(e[u] / b.K);
                    g4[u] = *reinterpret_cast<const unsigned*>(b.arg + ii * b.odim + co);
                    dv[u] = *reinterpret_cast<const f4*>(b.dh + ii * b.odim + co);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) take(e[u], g4[u], dv[u]);                  // (in list order: the same sums as before)
            }
            for (; n < hi; ++n) {
                const int e = a.edge[n];
                const size_t ii = (size_t)(e / b.K);
                take(e, *reinterpret_cast<const unsigned*>(b.arg + ii * b.odim + co), *reinterpret_cast<const f4*>(b.dh + ii * b.odim + co));
            }
        }
        if (!(a.p_done && c < b.GT)) *reinterpret_cast<f4*>(b.dPQ + (size_t)i * 2 * b.S + c) = sum;
        *reinterpret_cast<f4*>(b.dPQ + (size_t)i * 2 * b.S + b.S + c) = q;
    }
}

// ------------------------------------------------------------------------------------------------ growth-weight gradients
// part[chunk][c][u] = sum over the chunk's edges of dYfull[e, c] * lrelu(bn(Y[e, u])), c < S (growth layers then conv_out),
// u < GT.  K dimension = edges: both operands are channel-fast in memory, so a block of 32 edges is staged through LDS
// (coalesced float4 loads, the activation / the pooled gradient formed once on the way) and the MFMA operands are read
// from there edge-major.  blockIdx.y = 0: the conv_out rows; 1: the growth rows, whose output is block lower triangular
// (layer t sees columns u < g t only) - structurally empty 16 x 16 tiles are skipped.
struct EcDwArgs {
    const float* dY; const float* Y; int ld;
    const float* aff;
    const float* dh; const unsigned char* arg; const float* dyout; int pooled;
    int g, GT, odim, S, K;
    long long E; int chunk;
    float slope;
    float* part;
    float* bpart;                    // [nchunk][S]: column sums of dYfull over the chunk (the conv bias gradients)
};
#ifndef PF_DW_EB
#define PF_DW_EB 32
#endif
constexpr int DW_EB = PF_DW_EB;                     // edges per staged block

// NWV waves per workgroup share one staged block: 8 waves (4 per SIMD with two workgroups per CU) keep the matrix pipe fed while
// other waves sit in the load -> LDS -> barrier phase (PMC at 4 waves: MFMA busy 24 %, 57 % of the wave cycles waiting)
template <int NWV>
__global__ __launch_bounds__(64 * NWV) void ec_dw_kernel(EcDwArgs a) {
    constexpr int NTH = 64 * NWV, SL = 32 / NWV;         // row-tile slots per wave: 8 at 4 waves, 4 at 8
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, q = lane >> 4;
    const bool outrows = blockIdx.y == 0;
    const int RA = outrows ? a.odim : a.GT;
    const int lda = RA + 16, ldb = a.GT + 16;
    float* As = lds;
    float* Bs = lds + DW_EB * lda;
    // tile (rt, ct) of the output block -> wave: WC = min(4, NT) waves side by side along the columns, 4 / WC groups of
    // them along the rows; a wave owns column tiles ct_j = w % WC + WC j (j < 2) and row tiles rt_s = w / WC + (4 / WC) s
    // (s < 8): per K-step it reads <= 2 B values and <= 8 A values from LDS for <= 16 MFMAs
    const int NT = a.GT / 16, NRT = RA / 16;
    const int WC = NT < 4 ? NT : 4, rstep = NWV / WC, rbase = wave / WC;
    int ctj[2];
    bool cval[2];
#pragma unroll
    for (int jc = 0; jc < 2; ++jc) { ctj[jc] = wave % WC + WC * jc; cval[jc] = ctj[jc] < NT; }
    bool val[SL][2];
#pragma unroll
    for (int s = 0; s < SL; ++s) {
        const int rt = rbase + rstep * s;
        int ntn = NT;
        if (!outrows) {
            const int last = rt * 16 + 15;
            ntn = ((last / a.g) * a.g + 15) / 16;                 // column tiles u < g * (layer of the tile's last row)
        }
#pragma unroll
        for (int jc = 0; jc < 2; ++jc) val[s][jc] = rt < NRT && cval[jc] && ctj[jc] < ntn;
    }
    f4 acc[SL][2];
#pragma unroll
    for (int s = 0; s < SL; ++s) { acc[s][0] = pf_splat(0.f); acc[s][1] = pf_splat(0.f); }
    const int e_lo = blockIdx.x * a.chunk, e_hi = min((int)a.E, e_lo + a.chunk);      // E < 2^30: 32-bit edge indices
    const int ra4 = RA / 4, gt4 = a.GT / 4;
    float bsum = 0.f;
    // float4 staging units, thread t owns units t, t + 256, ... (fixed (edge, column) per unit); the next block's units are
    // fetched into registers while the current block is multiplied
    constexpr int UN = DW_EB * 32 / NTH;                 // DW_EB * 128 / 4 / threads
    int elA[UN], cA[UN], elB[UN], cB[UN];
#pragma unroll
    for (int n = 0; n < UN; ++n) {
        const int k = threadIdx.x + NTH * n;
        elA[n] = k / ra4; cA[n] = (k - elA[n] * ra4) * 4;
        elB[n] = k / gt4; cB[n] = (k - elB[n] * gt4) * 4;
    }
    f4 ra[UN], rbv[UN];
    auto fetch = [&](int eb) {
#pragma unroll
        for (int n = 0; n < UN; ++n) {
            f4 v = pf_splat(0.f);
            const int e = eb + elA[n], c = cA[n];
            if (elA[n] < DW_EB && e < e_hi) {
                if (!outrows) v = *reinterpret_cast<const f4*>(a.dY + (size_t)e * a.ld + c);
                else if (a.pooled) {
                    const int ii = e >> 4, k = e & 15;                          // pooled units have K = 16
                    const f4 dv = *reinterpret_cast<const f4*>(a.dh + (size_t)ii * a.odim + c);
                    const unsigned g4 = *reinterpret_cast<const unsigned*>(a.arg + (size_t)ii * a.odim + c);
                    v.x = (int)(g4 & 255u) == k ? dv.x : 0.f; v.y = (int)((g4 >> 8) & 255u) == k ? dv.y : 0.f;
                    v.z = (int)((g4 >> 16) & 255u) == k ? dv.z : 0.f; v.w = (int)(g4 >> 24) == k ? dv.w : 0.f;
                } else v = *reinterpret_cast<const f4*>(a.dyout + (size_t)e * a.odim + c);
            }
            ra[n] = v;
        }
#pragma unroll
        for (int n = 0; n < UN; ++n) {
            f4 v = pf_splat(0.f);
            const int e = eb + elB[n], c = cB[n];
            if (elB[n] < DW_EB && e < e_hi)
                v = lrelu4(*reinterpret_cast<const f4*>(a.Y + (size_t)e * a.ld + c) * *reinterpret_cast<const f4*>(a.aff + c) +
                           *reinterpret_cast<const f4*>(a.aff + a.ld + c), a.slope);
            rbv[n] = v;
        }
    };
    fetch(e_lo);
    for (int eb = e_lo; eb < e_hi; eb += DW_EB) {
        __syncthreads();
#pragma unroll
        for (int n = 0; n < UN; ++n) {
            if (elA[n] < DW_EB) *reinterpret_cast<f4*>(As + elA[n] * lda + cA[n]) = ra[n];
            if (elB[n] < DW_EB) *reinterpret_cast<f4*>(Bs + elB[n] * ldb + cB[n]) = rbv[n];
        }
        __syncthreads();
        if (eb + DW_EB < e_hi) fetch(eb + DW_EB);
        if (threadIdx.x < RA)
#pragma unroll 8
            for (int el = 0; el < DW_EB; ++el) bsum += As[el * lda + threadIdx.x];
#pragma unroll
        for (int ks = 0; ks < DW_EB / 4; ++ks) {
            const float* ar = As + (4 * ks + q) * lda + row + rbase * 16;
            const float* br = Bs + (4 * ks + q) * ldb + row;
            const float b0 = cval[0] ? br[ctj[0] * 16] : 0.f, b1 = cval[1] ? br[ctj[1] * 16] : 0.f;
#pragma unroll
            for (int s = 0; s < SL; ++s) {
                if (val[s][0] || val[s][1]) {
                    const float av = ar[rstep * s * 16];
                    if (val[s][0]) acc[s][0] = pf_mfma(av, b0, acc[s][0]);
                    if (val[s][1]) acc[s][1] = pf_mfma(av, b1, acc[s][1]);
                }
            }
        }
    }
    if (threadIdx.x < RA) a.bpart[(size_t)blockIdx.x * a.S + (outrows ? a.GT : 0) + threadIdx.x] = bsum;
    float* out = a.part + ((size_t)blockIdx.x * a.S + (outrows ? a.GT : 0)) * a.GT;
#pragma unroll
    for (int s = 0; s < SL; ++s)
#pragma unroll
        for (int jc = 0; jc < 2; ++jc)
            if (val[s][jc])
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    out[(size_t)((rbase + rstep * s) * 16 + 4 * q + r) * a.GT + ctj[jc] * 16 + row] = acc[s][jc][r];
}

// ------------------------------------------------------------------------------------------------ growth-weight gradients, no LDS
// The same partial sums with the operands loaded straight into the 32x32x2 f32 MFMA layout: a K-step is two edges, lane l holds
// A[channel l & 31][edge l >> 5] and B[edge l >> 5][channel l & 31] - one 4-byte load each, 128 contiguous bytes per half wave.
// No LDS image, no barriers: every wave streams its own operands four K-steps ahead and owns a strip of <= 4 output tiles
// (64 accumulator registers).  Jobs (one wave each): conv_out row strips with all GT / 32 column tiles, growth row strips with
// the column tiles their layers can see.  The staged kernel above spent 54 % of its wave cycles waiting with the matrix pipe
// 30 % busy; it stays for shapes that are not multiples of 32.
struct EcDw2Job { int out, rt, nct; };
struct EcDw2Args {
    EcDwArgs d;
    EcDw2Job job[8];
    int njob;
};
typedef float f16v __attribute__((ext_vector_type(16)));
#ifndef PF_DW2_D
#define PF_DW2_D 8
#endif
constexpr int DW2_D = PF_DW2_D;                               // K-steps (of two edges) per software-pipeline stage

#ifdef PF_EC_DW_F32                                    // the f32-product form of the no-LDS kernel: A/B builds only
__global__ __launch_bounds__(512) void ec_dw2_kernel(EcDw2Args g2) {
    const EcDwArgs& a = g2.d;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
    if (wave >= g2.njob) return;
    const EcDw2Job jb = g2.job[wave];
    const int e_lo = blockIdx.x * a.chunk, e_hi = min((int)a.E, e_lo + a.chunk);      // multiples of 16
    const int crow = jb.rt * 32 + col;                  // this lane's A channel
    const bool outj = jb.out != 0;
    float sc[4], sh[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int c = t * 32 + col;
        sc[t] = t < jb.nct ? a.aff[c] : 0.f;
        sh[t] = t < jb.nct ? a.aff[a.ld + c] : 0.f;
    }
    f16v acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float asum = 0.f;
    // one stage = DW2_D K-steps = 8 edges (inside one point: K = 16 edges per point for pooled units)
    float an[DW2_D], bn[DW2_D][4];
    auto fetch = [&](int e0) {
        if (outj && a.pooled) {
            const int ii = e0 >> 4;
            const float dv = a.dh[(size_t)ii * a.odim + crow];
            const int kk = a.arg[(size_t)ii * a.odim + crow];
#pragma unroll
            for (int k = 0; k < DW2_D; ++k) an[k] = (((e0 + 2 * k + h) & 15) == kk) ? dv : 0.f;
        } else {
#pragma unroll
            for (int k = 0; k < DW2_D; ++k) {
                const size_t e = (size_t)(e0 + 2 * k + h);
                an[k] = outj ? a.dyout[e * a.odim + crow] : a.dY[e * a.ld + crow];
            }
        }
#pragma unroll
        for (int k = 0; k < DW2_D; ++k) {
            const float* yr = a.Y + (size_t)(e0 + 2 * k + h) * a.ld + col;
#pragma unroll
            for (int t = 0; t < 4; ++t) bn[k][t] = t < jb.nct ? yr[t * 32] : 0.f;
        }
    };
    if (e_lo < e_hi) fetch(e_lo);
    for (int e0 = e_lo; e0 < e_hi; e0 += 2 * DW2_D) {
        float ac[DW2_D], bc[DW2_D][4];
#pragma unroll
        for (int k = 0; k < DW2_D; ++k) {
            ac[k] = an[k];
#pragma unroll
            for (int t = 0; t < 4; ++t) bc[k][t] = bn[k][t];
        }
        if (e0 + 2 * DW2_D < e_hi) fetch(e0 + 2 * DW2_D);
#pragma unroll
        for (int k = 0; k < DW2_D; ++k) {
            asum += ac[k];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < jb.nct) {
                    const float z = fmaf(bc[k][t], sc[t], sh[t]);
                    const float bv = fmaxf(z, z * a.slope);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[k], bv, acc[t], 0, 0, 0);
                }
            }
        }
    }
    const int rowbase = outj ? a.GT : 0;
    asum += __shfl_xor(asum, 32);
    if (h == 0) a.bpart[(size_t)blockIdx.x * a.S + rowbase + crow] = asum;
    float* out = a.part + ((size_t)blockIdx.x * a.S + rowbase + jb.rt * 32) * a.GT;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (t < jb.nct)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ri = (r & 3) + 8 * (r >> 2) + 4 * h;
                out[(size_t)ri * a.GT + t * 32 + col] = acc[t][r];
            }
}
#endif

// The same jobs on the bf16 matrix pipe: x = hi + mid with hi = bf16(x) and mid = bf16(x - hi), both rounded to nearest (bf16_pair
// above; 16 significant bits together, fp32 exponent range - gradients of 1e-7 keep their digits, which fp16 halves would not), three
// v_mfma_f32_32x32x16_bf16 per tile and 16 edges (hi hi + hi mid + mid hi, fp32 accumulate) instead of eight f32 MFMAs: 96 against
// 512 matrix-pipe cycles.  Lane l holds its channel for the 8 edges 8 (l >> 5) + j of a 16-edge step.  In the no-LDS structure
// the f32 pipe WAS the limit (the busiest SIMD of a workgroup owns 7 of its 22 tiles: 448 cycles per two edges); in the staged
// kernel the same change bought nothing.
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
struct Bf2 { bf8 hi, mid; };
__device__ __forceinline__ Bf2 dw3_split(const float (&x)[8]) {
    unsigned hw[4], mw[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        hw[p] = bf16_pair(x[2 * p], x[2 * p + 1]);
        mw[p] = bf16_pair(x[2 * p] - __uint_as_float(hw[p] << 16), x[2 * p + 1] - __uint_as_float(hw[p] & 0xffff0000u));
    }
    Bf2 r;
    r.hi = __builtin_bit_cast(bf8, *reinterpret_cast<const uint4*>(hw));
    r.mid = __builtin_bit_cast(bf8, *reinterpret_cast<const uint4*>(mw));
    return r;
}

__global__ __launch_bounds__(512) void ec_dw3_kernel(EcDw2Args g2) {
    const EcDwArgs& a = g2.d;
    // the wave index through readfirstlane: its job (row strip, column tile count) is then wave-uniform to the compiler - scalar
    // loads of the job, scalar branches around the per-tile MFMAs instead of exec masks
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
    if (wave >= g2.njob) return;
    const EcDw2Job jb = g2.job[wave];
    const int e_lo = blockIdx.x * a.chunk, e_hi = min((int)a.E, e_lo + a.chunk);      // multiples of 16
    const int crow = jb.rt * 32 + col;
    const bool outj = jb.out != 0;
    float sc[4], sh[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int c = t * 32 + col;
        sc[t] = t < jb.nct ? a.aff[c] : 0.f;
        sh[t] = t < jb.nct ? a.aff[a.ld + c] : 0.f;
    }
    f16v acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float asum = 0.f;
    // DEPTH 16-edge steps' operands in flight.  Measured (round 5, same box, whole step): depth 1 4.566 ms, 2 4.571,
    // 3 4.58 - 4.79: the kernel does not wait for its loads.  (Kept in the any-depth form: with the [1] arrays and
    // one-trip loops collapsed by hand the compiler orders the instructions differently.)
    constexpr int DEPTH = 1;
    float an[DEPTH][8], bn[DEPTH][4][8];
    auto fetch = [&](int e0, float (&an_)[8], float (&bn_)[4][8]) {
        if (outj && a.pooled) {
            const int ii = e0 >> 4;
            const float dv = a.dh[(size_t)ii * a.odim + crow];
            const int kk = a.arg[(size_t)ii * a.odim + crow];
#pragma unroll
            for (int j = 0; j < 8; ++j) an_[j] = (8 * h + j == kk) ? dv : 0.f;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const size_t e = (size_t)(e0 + 8 * h + j);
                an_[j] = outj ? a.dyout[e * a.odim + crow] : a.dY[e * a.ld + crow];
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float* yr = a.Y + (size_t)(e0 + 8 * h + j) * a.ld + col;
#pragma unroll
            for (int t = 0; t < 4; ++t) bn_[t][j] = t < jb.nct ? yr[t * 32] : 0.f;
        }
    };
#pragma unroll
    for (int u = 0; u < DEPTH; ++u)
        if (e_lo + 16 * u < e_hi) fetch(e_lo + 16 * u, an[u], bn[u]);
    for (int e0 = e_lo; e0 < e_hi; e0 += 16 * DEPTH)
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
        if (e0 + 16 * u >= e_hi) break;
        float ac[8], bc[4][8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            ac[j] = an[u][j];
            asum += an[u][j];
#pragma unroll
            for (int t = 0; t < 4; ++t) bc[t][j] = bn[u][t][j];
        }
        if (e0 + 16 * (u + DEPTH) < e_hi) fetch(e0 + 16 * (u + DEPTH), an[u], bn[u]);
        const Bf2 A = dw3_split(ac);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t < jb.nct) {
                float bv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float z = fmaf(bc[t][j], sc[t], sh[t]);
                    bv[j] = fmaxf(z, z * a.slope);
                }
                const Bf2 B = dw3_split(bv);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.mid, B.hi, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.hi, B.mid, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.hi, B.hi, acc[t], 0, 0, 0);
            }
        }
    }
    const int rowbase = outj ? a.GT : 0;
    asum += __shfl_xor(asum, 32);
    if (h == 0) a.bpart[(size_t)blockIdx.x * a.S + rowbase + crow] = asum;
    float* out = a.part + ((size_t)blockIdx.x * a.S + rowbase + jb.rt * 32) * a.GT;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (t < jb.nct)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ri = (r & 3) + 8 * (r >> 2) + 4 * h;
                out[(size_t)ri * a.GT + t * 32 + col] = acc[t][r];
            }
}

// dWpq [R, C] = dPQ^T x for a unit whose input has C <= 4 channels (the first unit: the coordinates): one thread per output row
// r, a chunk of points per workgroup, partial sums as split-K slabs for the reduction kernel of the point GEMMs.  The general
// GEMM takes its scalar staging path for these shapes (C is not a multiple of 4): 69 us for 2.4 M products.
__global__ __launch_bounds__(256) void ec_dwpq_small_kernel(const float* __restrict__ dPQ, const float* __restrict__ x, int R, int C,
                                                           int T, int chunk, float* __restrict__ slabs) {
    const int r = blockIdx.y * 256 + threadIdx.x;
    const int t_lo = blockIdx.x * chunk, t_hi = min(T, t_lo + chunk);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (r < R) {
        int t = t_lo;
        for (; t + 7 < t_hi; t += 8) {                                // eight loads in flight per thread
            float g[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) g[k] = dPQ[(size_t)(t + k) * R + r];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float* xp = x + (size_t)(t + k) * C;            // wave-uniform: scalar loads
                a0 = fmaf(g[k], xp[0], a0);
                if (C > 1) a1 = fmaf(g[k], xp[1], a1);
                if (C > 2) a2 = fmaf(g[k], xp[2], a2);
                if (C > 3) a3 = fmaf(g[k], xp[3], a3);
            }
        }
        for (; t < t_hi; ++t) {
            const float g = dPQ[(size_t)t * R + r];
            const float* xp = x + (size_t)t * C;
            a0 = fmaf(g, xp[0], a0);
            if (C > 1) a1 = fmaf(g, xp[1], a1);
            if (C > 2) a2 = fmaf(g, xp[2], a2);
            if (C > 3) a3 = fmaf(g, xp[3], a3);
        }
    }
    if (r < R) {
        float* o = slabs + ((size_t)blockIdx.x * R + r) * C;
        o[0] = a0;
        if (C > 1) o[1] = a1;
        if (C > 2) o[2] = a2;
        if (C > 3) o[3] = a3;
    }
}

// dW_t[r, :] = [dWp | dWq | dWq - dWp | sum_chunks part[:, rowoff_t + r, :g t]],  dbias_t[r] = sum_chunks bpart[:, rowoff_t + r].
// 64 consecutive elements per workgroup, the chunk sum split four ways (threadIdx.y) and joined through LDS.
constexpr int ASM_G = 16;            // groups of 64 threads that share the chunk range of an output element
// dWpq arrives as `nslab` split-K slabs [nslab][2 S, C] of its point GEMM (nslab = 1: the finished product): their sum is taken here,
// by the same 16 lanes per element that add the growth partials - it was a launch of its own (gemm_reduce_kernel) in front of this
// one, seven per step, and a replayed step pays ~5 - 10 us per kernel boundary.
__global__ __launch_bounds__(64 * ASM_G) void ec_assemble_kernel(EcConvs cv, const float* dWpq, int nslab, const float* part, int nchunk,
                                                                const float* bpart, int total) {
    __shared__ double sh[ASM_G][64], shb[ASM_G][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + tx;
    int t = 0, r = 0, col = 0, srow = 0;
    bool ok = i < total, grow = false;
    if (ok) {
        int rem = i;
        while (rem >= cv.rows[t] * cv.width[t]) { rem -= cv.rows[t] * cv.width[t]; ++t; }
        r = rem / cv.width[t]; col = rem % cv.width[t];
        srow = cv.rowoff[t] + r;
        grow = col >= 3 * cv.C;
    }
    double s = 0.0, sb = 0.0;
    if (ok && grow) {
        const int u = col - 3 * cv.C;
        int k = ty;
        for (; k + 3 * ASM_G < nchunk; k += 4 * ASM_G) {              // four loads in flight per thread
            const float v0 = part[((size_t)k * cv.S + srow) * cv.GT + u], v1 = part[((size_t)(k + ASM_G) * cv.S + srow) * cv.GT + u];
            const float v2 = part[((size_t)(k + 2 * ASM_G) * cv.S + srow) * cv.GT + u];
            const float v3 = part[((size_t)(k + 3 * ASM_G) * cv.S + srow) * cv.GT + u];
            s += ((double)v0 + (double)v1) + ((double)v2 + (double)v3);
        }
        for (; k < nchunk; k += ASM_G) s += (double)part[((size_t)k * cv.S + srow) * cv.GT + u];
    }
    if (ok && !grow) {                                 // [dWp | dWq | dWq - dWp] from the slabs of dWpq = [dWp; dWq]
        const int kind = col / cv.C, cc = col - kind * cv.C;
        const size_t ip = (size_t)srow * cv.C + cc, iq = (size_t)(cv.S + srow) * cv.C + cc, stride = (size_t)2 * cv.S * cv.C;
        double sp = 0.0, sq = 0.0;
        for (int k = ty; k < nslab; k += ASM_G) {
            const float vp = dWpq[k * stride + (kind != 1 ? ip : iq)], vq = dWpq[k * stride + (kind != 0 ? iq : ip)];
            sp += (double)vp; sq += (double)vq;
        }
        s = kind == 0 ? sp : (kind == 1 ? sq : sq - sp);
    }
    if (ok && col == 0)
        for (int k = ty; k < nchunk; k += ASM_G) sb += (double)bpart[(size_t)k * cv.S + srow];
    sh[ty][tx] = s; shb[ty][tx] = sb;
    __syncthreads();
    if (ty != 0 || !ok) return;
    float v;
    {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < ASM_G; ++k) a += sh[k][tx];
        v = (float)a;
    }
    cv.dW[t][(size_t)r * cv.width[t] + col] = v;
    if (col == 0) {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < ASM_G; ++k) a += shb[k][tx];
        cv.dbias[t][r] = (float)a;
    }
}

__global__ __launch_bounds__(256) void ec_zero_kernel(f4* p, long long n4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) p[i] = pf_splat(0.f);
}

#ifndef PF_EC_DW_CHUNK
#define PF_EC_DW_CHUNK 512
#endif
constexpr int EC_DW_CHUNK = PF_EC_DW_CHUNK;
#ifndef PF_EC_DW_CHUNK_SCALE
#define PF_EC_DW_CHUNK_SCALE 1
#endif
#ifndef EC_DW_WAVES
#define EC_DW_WAVES 8
#endif

template <int G, int ODIM>
size_t ecpb_lds_bytes() {
#ifdef PF_EC_BWDG_F32
    return sizeof(float) * ((size_t)G * 4 * (ODIM + 4) + (size_t)4 * ((G + 15) / 16) * 16 * (G * 4 + 4));
#else
    int nf = (G * 4 / 16) * (ODIM / 32);
    for (int s = 0; s < 4; ++s) nf += ((G + 15) / 16) * (G * 4 / 32 - (G * (s + 1)) / 32);
    return (size_t)nf * 2 * 64 * 16;
#endif
}
template <int G, int ODIM>
bool ecpb_fits() {
    return resident_per_cu(ec_bwdp_kernel<G, 4, ODIM>, ECP_T, ecpb_lds_bytes<G, ODIM>(), nullptr) >= ECP_TPW / ecp_tpw(G);
}
bool ec_bwd_persistent_fits(const PfEcTrain* p) {
    return p->growth == 8 ? ecpb_fits<8, 32>() : (p->growth == 16 ? ecpb_fits<16, 64>() : ecpb_fits<32, 128>());
}

}  // namespace

int pf_stat_sync(const StatFin& fin, int ncol, PfSyncFn cb, void* user, hipStream_t s) {
    if (!fin.defer) return PF_OK;
    if (!cb) return PF_ERR_NULL;
    if (cb(user, fin.defer, 2 * STAT_W + 1, (void*)s) != 0) return PF_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(stat_finalize_kernel, dim3(1), dim3(STAT_W), 0, s, fin, ncol);
    return PF_OK;
}

int pf_ec_dims(const PfEcTrain* p, EcDims& d) {
    if (!p) return PF_ERR_NULL;
    if (p->B <= 0 || p->N <= 0 || p->K <= 0 || p->C <= 0 || p->nconv < 1 || p->nconv > 8) return PF_ERR_SHAPE;
    if (p->growth != 8 && p->growth != 16 && p->growth != 32) return PF_ERR_UNSUPPORTED;
    if (p->odim % 16 != 0 || p->odim > 128 || p->odim < 16) return PF_ERR_UNSUPPORTED;
    if (p->pooling && p->K != 16) return PF_ERR_UNSUPPORTED;
    d.T = p->B * p->N;
    d.GT = p->growth * p->nconv;
    if (d.GT != 32 && d.GT != 64 && d.GT != 128) return PF_ERR_UNSUPPORTED;
    d.S = d.GT + p->odim;
    d.nconvs = p->nconv + 1;
    d.E = (long long)d.T * p->K;
    if (d.E % 16 != 0 || d.E > (1ll << 30)) return PF_ERR_SHAPE;
    d.ntiles = (int)(d.E / 16);
    d.grid = (d.ntiles + 3) / 4 < EC_GRID ? (d.ntiles + 3) / 4 : EC_GRID;
    // growth-layer kernels: measured (layer with 96 input channels, 131 072 edges) 44 / 30 / 29 / 41 us at 128 / 256 / 512 / 2048
    // workgroups: beyond 2 per CU the fixed cost per workgroup (weight staging, 64 statistics atomics) outweighs the latency hiding
    d.grid_light = d.grid;
    // edges per split-K chunk of the weight-gradient launch: one workgroup per chunk with (odim + GT) / 32 waves - the narrow units
    // (GT = 32 / 64: 2 / 4 waves) get shorter chunks so that they, too, put two waves on every SIMD
    d.chunk = PF_EC_DW_CHUNK_SCALE ? (d.GT <= 32 ? EC_DW_CHUNK / 4 : (d.GT <= 64 ? EC_DW_CHUNK / 2 : EC_DW_CHUNK)) : EC_DW_CHUNK;
    d.nchunk = (int)((d.E + d.chunk - 1) / d.chunk);
    return PF_OK;
}
EcConvs pf_ec_convs(const PfEcTrain* p, const EcDims& d) {
    EcConvs cv{};
    cv.nconvs = d.nconvs; cv.C = p->C; cv.S = d.S; cv.GT = d.GT;
    int off = 0;
    for (int t = 0; t < d.nconvs; ++t) {
        cv.W[t] = p->W[t]; cv.bias[t] = p->bias[t]; cv.dW[t] = p->dW[t]; cv.dbias[t] = p->dbias[t];
        cv.rows[t] = t < p->nconv ? p->growth : p->odim;
        cv.width[t] = 3 * p->C + p->growth * t;
        cv.rowoff[t] = off;
        off += cv.rows[t];
    }
    cv.rowoff[d.nconvs] = off;
    return cv;
}
long long pf_ec_gemm_ws_max(const PfEcTrain* p, const EcDims& d) {
    long long g1 = pf_gemm_ws_floats(2 * d.S, p->C, d.T), g2 = pf_gemm_ws_floats(d.T, p->C, 2 * d.S),
              g3 = pf_gemm_ws_floats(d.T, 2 * d.S, p->C);
    long long gm = g1 > g2 ? g1 : g2;
    return gm > g3 ? gm : g3;
}

int pf_ecp_grid(const EcDims& d, int tpw) {
    const int wgs = (d.ntiles + ECP_WAVES * tpw - 1) / (ECP_WAVES * tpw);               // fewest workgroups that hold every tile ...
    int ncu = 0, dev = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    const int spread = (d.ntiles + ECP_WAVES - 1) / ECP_WAVES;                         // ... spread over the CUs when there are fewer tiles
    return spread < ncu ? (spread > wgs ? spread : wgs) : (wgs > ncu ? wgs : ncu);
}

namespace {

int ec_bwd_persistent(const PfEcTrain* p, const EcDims& d, const EcConvs& cv, hipStream_t s) {
    EcBwdPArgs a{};
    a.dh = p->dout; a.arg = p->arg; a.dA = p->dA; a.Y = p->Y; a.ld = d.GT; a.aff = p->aff; a.coef = p->coef;
    a.Wout = p->W[p->nconv] + 3 * p->C; a.ldwout = cv.width[p->nconv];
    for (int t = 0; t < p->nconv; ++t) {
        a.Wg[t] = p->W[t] + 3 * p->C; a.ldwg[t] = cv.width[t];
        a.dgamma[t] = p->dgamma[t]; a.dbeta[t] = p->dbeta[t];
    }
    a.ntiles = d.ntiles; a.slope = p->slope; a.R = (double)d.E; a.acc = p->stat; a.sync = p->sync;
    if (p->K == 16 && p->csr_off && p->csr_edge) { a.dP = p->dPQ; a.ldp = 2 * d.S; }       // (ec_pq_bwd_kernel zeroes and accumulates dPQ itself)
    const int grid = pf_ecp_grid(d, ecp_tpw(p->growth));
    const size_t l8 = ecpb_lds_bytes<8, 32>(), l16 = ecpb_lds_bytes<16, 64>(), l32 = ecpb_lds_bytes<32, 128>();
    if (p->growth == 8) hipLaunchKernelGGL((ec_bwdp_kernel<8, 4, 32>), dim3(grid), dim3(ECP_T), l8, s, a);
    else if (p->growth == 16) hipLaunchKernelGGL((ec_bwdp_kernel<16, 4, 64>), dim3(grid), dim3(ECP_T), l16, s, a);
    else hipLaunchKernelGGL((ec_bwdp_kernel<32, 4, 128>), dim3(grid), dim3(ECP_T), l32, s, a);
    return pf_last_launch_status();
}

}  // namespace

// floats of scratch for either direction: dw partials [nchunk][S][GT] + [nchunk][S] + split-K slabs of the point GEMMs
extern "C" long long pf_ec_train_ws_floats(const PfEcTrain* p) {
    EcDims d;
    if (pf_ec_dims(p, d) != PF_OK) return -1;
    return (long long)d.nchunk * d.S * (d.GT + 1) + pf_ec_gemm_ws_max(p, d);
}

extern "C" int pf_ec_train_bwd(const PfEcTrain* p, void* stream) {
    EcDims d;
    int st = pf_ec_dims(p, d);
    if (st) return st;
    if (!p->x || !p->idx || !p->Wpq || !p->PQ || !p->Y || !p->aff || !p->dout || !p->dA || !p->dPQ || !p->coef || !p->dWpq ||
        !p->ws || !p->stat)
        return PF_ERR_NULL;
    if (p->pooling && !p->arg) return PF_ERR_NULL;
    for (int t = 0; t < d.nconvs; ++t)
        if (!p->W[t] || !p->dW[t] || !p->dbias[t]) return PF_ERR_NULL;
    for (int t = 0; t < p->nconv; ++t)
        if (!p->dgamma[t] || !p->dbeta[t]) return PF_ERR_NULL;
    if (p->ws_floats < pf_ec_train_ws_floats(p)) return PF_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const EcConvs cv = pf_ec_convs(p, d);
    const int g = p->growth, nc = p->nconv;
    // weight gradients on their own stream (pf_train_set_dw_stream) take the second workspace: the partial slabs and the
    // scratch of the dWpq GEMM; the calling stream keeps p->ws for the dx GEMM
    const bool dw_side = pf_dw_stream_get() && pf_dw_stream_get() != stream && p->ws_dw && p->ws_dw_floats >= pf_ec_train_ws_floats(p);
    float* dwpart = dw_side ? p->ws_dw : p->ws;
    float* bpart = dwpart + (long long)d.nchunk * d.S * d.GT;
    float* gws_dw = bpart + (long long)d.nchunk * d.S;
    float* gws = p->ws + (long long)d.nchunk * d.S * (d.GT + 1);
    const bool csr = p->csr_off && p->csr_edge;
    // cleared by a kernel rather than hipMemsetAsync: see csrc/emd.hip (memset nodes inside a captured hipGraph)
    if (!csr)
        hipLaunchKernelGGL(ec_zero_kernel, dim3(512), dim3(256), 0, s, reinterpret_cast<f4*>(p->dPQ), (long long)d.T * 2 * d.S / 4);

    const bool persistent = pf_ec_persistent_ok(p, d) && ec_bwd_persistent_fits(p);
    if (persistent) {
        st = ec_bwd_persistent(p, d, cv, s);
        if (st) return st;
    }
    // ---- gather form: layer s = nc - 1 .. 0 collects its own gradient columns from conv_out and the later growth convs
    for (int sl = nc - 1; sl >= 0 && !persistent; --sl) {
        EcBwdgArgs a{};
        a.dh = p->dout; a.arg = p->arg; a.dyout = p->dout; a.odim = p->odim;
        a.dA = p->dA; a.Y = p->Y; a.ld = d.GT; a.aff = p->aff; a.coef = p->coef;
        a.Wout = p->W[nc] + 3 * p->C; a.ldwout = cv.width[nc];
        for (int t = 1; t < nc; ++t) { a.Wg[t] = p->W[t] + 3 * p->C; a.ldwg[t] = cv.width[t]; }
        a.s = sl; a.nc = nc; a.g = g; a.ntiles = d.ntiles; a.slope = p->slope;
        a.fin = StatFin{p->stat, 2, g, g * sl, d.GT, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, p->coef,
                        p->dgamma[sl], p->dbeta[sl], (double)d.E, p->sync_sums};
        a.fin.det = PF_DET(p);
        const int g16 = (g + 15) & ~15, od16 = (p->odim + 15) & ~15, ntg = g16 / 16;
#ifdef PF_EC_BWDG_F32
        const size_t lds = sizeof(float) * ((size_t)ntg * 16 * ((od16 + 4) + (size_t)(nc - 1 - sl) * (g16 + 4)) + 6 * g16);
#define PF_ECG(NTG, SRC)                                                                                                  \
    do { allow_lds(ec_bwdg_kernel<NTG, SRC>, lds);                                                                        \
         hipLaunchKernelGGL((ec_bwdg_kernel<NTG, SRC>), dim3(d.grid), dim3(256), lds, s, a); } while (0)
#else
        (void)od16;
        const size_t nfrag = (size_t)ntg * ((p->odim + 31) / 32 + (size_t)(nc - 1 - sl) * ((g + 31) / 32));
        const size_t lds = nfrag * 2 * 64 * 16 + sizeof(float) * 6 * g16;
#define PF_ECG(NTG, SRC)                                                                                                  \
    do { allow_lds(ec_bwdg16_kernel<NTG, SRC>, lds);                                                                      \
         hipLaunchKernelGGL((ec_bwdg16_kernel<NTG, SRC>), dim3(d.grid), dim3(256), lds, s, a); } while (0)
#endif
        if (p->pooling) { if (ntg == 1) PF_ECG(1, 0); else PF_ECG(2, 0); }
        else { if (ntg == 1) PF_ECG(1, 1); else PF_ECG(2, 1); }
#undef PF_ECG
        if ((st = pf_stat_sync(a.fin, g, p->sync_cb, p->sync_user, s))) return st;     // SyncBN: global sums before the transform of this layer
    }
    if (!persistent) {
        const long long n = d.E * (g / 4);
        hipLaunchKernelGGL(ec_bwd0_kernel, dim3((unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256)), dim3(256), 0, s,
                           p->dA, p->Y, d.GT, p->aff, p->coef, g, d.E, p->slope);
    }
    // ---- dPQ (+ bias column sums)
    {
        EcPqBwdArgs a{p->dA, d.GT, p->dout, p->arg, p->dout, p->pooling, p->idx, p->N, p->K, d.GT, p->odim, d.S, (long long)d.T,
                      p->dPQ};
        const long long n = (long long)d.T * d.S;
        const dim3 grid((unsigned)((n + 255) / 256 > 8192 ? 8192 : (n + 255) / 256));
        const dim3 grid4((unsigned)((n / 4 + 255) / 256 > 8192 ? 8192 : (n / 4 + 255) / 256));
        const int p_done = (persistent && p->K == 16) ? 1 : 0;
        if (csr) hipLaunchKernelGGL(ec_pq_bwd_csr_kernel, grid4, dim3(256), 0, s, EcPqCsrArgs{a, p->csr_off, p->csr_edge, p_done});
        else hipLaunchKernelGGL(ec_pq_bwd_kernel, grid, dim3(256), 0, s, a);
    }
    // ---- dx first: it is what the unit before this one waits for
    if (p->dx) {
        st = pf_gemm_addend(0, p->dPQ, 2 * d.S, 1, p->Wpq, p->C, 1, p->dx, p->C, nullptr, p->dx_add, d.T, p->C, 2 * d.S, gws,
                            pf_gemm_ws_floats(d.T, p->C, 2 * d.S), stream, nullptr);
        if (st) return st;
    }
    // ---- growth-weight gradients (partials), dWpq, assembly: nobody reads them before the optimizer
    hipStream_t sm = s;                                   // (the kernels below are written with `s` and `stream`)
    if (dw_side) { s = pf_dw_fork(sm); stream = (void*)s; }
    {
        EcDwArgs a{p->dA, p->Y, d.GT, p->aff, p->dout, p->arg, p->dout, p->pooling, g, d.GT, p->odim, d.S, p->K, d.E, d.chunk,
                   p->slope, dwpart, bpart};
        // jobs of the no-LDS kernel: conv_out strips, then growth strips (a strip's column tiles: what its LAST row's layer sees)
        EcDw2Args a2{};
        a2.d = a;
        int nj = 0;
        bool direct = d.GT % 32 == 0 && p->odim % 32 == 0 && d.GT <= 128 && (!p->pooling || p->K == 16) && d.chunk % 16 == 0;
        if (direct) {
            for (int rt = 0; rt < p->odim / 32 && nj < 8; ++rt) a2.job[nj++] = EcDw2Job{1, rt, d.GT / 32};
            for (int rt = d.GT / 32 - 1; rt >= 0; --rt) {
                const int see = ((rt * 32 + 31) / g) * g;                   // growth columns u < g * layer(last row)
                const int nct = (see + 31) / 32;                            // 0: the strip still owes its bias sums
                if (nj >= 8) { direct = false; break; }
                a2.job[nj++] = EcDw2Job{0, rt, nct};
            }
            a2.njob = nj;
        }
        if (direct) {
#ifdef PF_EC_DW_F32
            hipLaunchKernelGGL(ec_dw2_kernel, dim3(d.nchunk), dim3(64 * nj), 0, s, a2);
#else
            hipLaunchKernelGGL(ec_dw3_kernel, dim3(d.nchunk), dim3(64 * nj), 0, s, a2);
#endif
        } else {
            const int ramax = p->odim > d.GT ? p->odim : d.GT;
            const size_t lds = sizeof(float) * (size_t)DW_EB * ((ramax + 16) + (d.GT + 16));
            allow_lds(ec_dw_kernel<EC_DW_WAVES>, lds);
            hipLaunchKernelGGL(ec_dw_kernel<EC_DW_WAVES>, dim3(d.nchunk, 2), dim3(64 * EC_DW_WAVES), lds, s, a);
        }
    }
    // slabs of the small-C kernel: as many as the GEMM scratch of this unit holds, at most 128
    const long long dw_cap = pf_ec_gemm_ws_max(p, d) / ((long long)2 * d.S * p->C);
    const int dw_want = (int)(dw_cap < 128 ? dw_cap : 128);
    const int dw_chunk = dw_want > 0 ? (d.T + dw_want - 1) / dw_want : d.T, dw_slabs = (d.T + dw_chunk - 1) / dw_chunk;
    const float* asm_src = p->dWpq;
    int asm_slabs = 1;
    if (p->C <= 4 && dw_want >= 16) {
        hipLaunchKernelGGL(ec_dwpq_small_kernel, dim3(dw_slabs, (2 * d.S + 255) / 256), dim3(256), 0, s, p->dPQ, p->x, 2 * d.S, p->C,
                           d.T, dw_chunk, gws_dw);
        st = pf_last_launch_status();
        asm_src = gws_dw; asm_slabs = dw_slabs;
    } else {
        int nsl = 0;                                    // split-K slabs left in gws_dw (0: the product went straight into dWpq)
        st = pf_gemm_addend(0, p->dPQ, 1, 2 * d.S, p->x, p->C, 1, p->dWpq, p->C, nullptr, nullptr, 2 * d.S, p->C, d.T, gws_dw,
                            pf_gemm_ws_floats(2 * d.S, p->C, d.T), stream, &nsl);
        if (nsl > 0) { asm_src = gws_dw; asm_slabs = nsl; }
    }
    if (st) return st;
    int total = 0;
    for (int t = 0; t < d.nconvs; ++t) total += cv.rows[t] * cv.width[t];
    hipLaunchKernelGGL(ec_assemble_kernel, dim3((total + 63) / 64), dim3(64 * ASM_G), 0, s, cv, asm_src, asm_slabs, dwpart, d.nchunk, bpart,
                       total);
    return pf_last_launch_status();
}
