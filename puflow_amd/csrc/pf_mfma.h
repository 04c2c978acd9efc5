// Device helpers shared by the PU-Flow HIP kernels (gfx950 / CDNA4 only).
//
// Register data layout used by every MLP-shaped kernel here ("channel-major chain"):
//   v_mfma_f32_16x16x4_f32 computes D(16x16) = A(16x4) * B(4x16) + C with
//     A: lane l holds A[row = l&15][k = l>>4]          (one float)
//     B: lane l holds B[k = l>>4][col = l&15]          (one float)
//     C/D: lane l holds D[row = 4*(l>>4) + r][col = l&15], r = 0..3   (float4)
//   We put OUTPUT CHANNELS on rows and POINTS/EDGES on the 16 columns, so a 16-channel block of
//   activations for 16 columns is one float4 per lane:  lane (col = l&15, q = l>>4), register r
//   <-> channel 16*cb + 4*q + r.  That is exactly the B operand the NEXT layer needs if its
//   K-step "r" consumes channels {16*cb + 4*q + r | q = 0..3}: no LDS round trip, no shuffles
//   between layers.  The host packs each weight matrix accordingly (packing.frag_pack):
//   fragment (ob, cb) is 64 lanes x float4, lane l = W[16*ob + (l&15)][16*cb + 4*(l>>4) + r].
//   The f32 MFMA is an exact k-ordered fp32 fma chain (no reduced precision).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "pf_wave.h"

typedef float f4 __attribute__((ext_vector_type(4)));

#define PF_WAVE 64

__device__ __forceinline__ f4 pf_mfma(float a, float b, f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f4 pf_splat(float v) { f4 r = {v, v, v, v}; return r; }

// leaky ReLU for 0 <= slope <= 1 as max(x, slope * x): same bits as the select form (x >= 0 ? x : slope * x)
// for every finite x including -0, one packed multiply + one max per value instead of compare + multiply + select
__device__ __forceinline__ f4 pf_lrelu(f4 v, float slope) {
    const f4 s = v * slope;
    f4 r;
    r.x = fmaxf(v.x, s.x); r.y = fmaxf(v.y, s.y); r.z = fmaxf(v.z, s.z); r.w = fmaxf(v.w, s.w);
    return r;
}

// ---- hardware transcendentals of the inference kernels (flow f / g, the interpolation softmax) -------------------------------
// One instruction each (v_exp_f32 after one multiply, v_rcp_f32, v_sqrt_f32; 1 ulp) where expf, an IEEE division and sqrtf are
// sequences of 8 - 12 around the same instruction.  exp: x log2(e) is rounded once, an absolute error of half an ulp of the
// product, i.e. a relative error of ln2 ulp(x log2e) / 2 + |x| 2^-25 in the result: 3e-7 at |x| = 5.3 (the largest injector
// log-scale s of the pretrained checkpoint), 6e-8 at |x| < 1; for the softmax terms e^(x - max), whose error weighs |x| e^-|x|,
// below 3e-8 of the sum at any spread.  Results below 2^-126 flush to zero and there is no overflow handling: s and the logits
// are O(10).  v_sqrt_f32 / v_rcp_f32 treat subnormal inputs as zero (a neighbour closer than 1e-19, a softmax sum is >= 1).
__device__ __forceinline__ float pf_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }
__device__ __forceinline__ float pf_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float pf_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }

// ---- weight fragment sources -----------------------------------------------------------
// Every lane-address of a weight fragment is (wave-uniform base) + lane*16.  hipcc otherwise
// hoists one 64-bit VGPR address pair PER FRAGMENT out of the persistent tile loop (hundreds of
// VGPRs); the sources here keep it to ONE VGPR:
//   PfWLds             : fragments resident in LDS, ds_read_b128 with a 16-bit immediate offset
//   PfW2BufD (f16 path): fragments in global memory through a buffer descriptor (SGPRs), uniform soffset
struct PfWLds {
    const f4* base;     // LDS
    int lane;
    __device__ __forceinline__ f4 load(int frag) const { return base[frag * PF_WAVE + lane]; }
};

// acc[p][acc0+ob] += W[ob][cb] * in[p][in0+cb]  for ob < OB, cb < CB.
// Fragment (ob, cb) of this matrix is `frag0 + ob*WCB + cb` of the weight source
// (WCB = number of 16-channel input blocks of the packed matrix = its row stride).
// P independent column tiles share each weight fragment (and give independent MFMA chains).
// Software pipeline: D fragments are kept in flight; a sched_barrier after every fragment's MFMAs
// stops hipcc from hoisting ALL loads to the top of the kernel.
template <int OB, int CB, int WCB, int D = 3, class WS, int P, int NIN, int NACC>
__device__ __forceinline__ void pf_mm(const WS& ws, int frag0, const f4 (&in)[P][NIN], int in0,
                                      f4 (&acc)[P][NACC], int acc0) {
    constexpr int NFRAG = OB * CB;
    constexpr int DD = D < NFRAG ? D : NFRAG;
    f4 wb[DD];
#pragma unroll
    for (int i = 0; i < DD; ++i) wb[i] = ws.load(frag0 + (i / CB) * WCB + (i % CB));
#pragma unroll
    for (int i = 0; i < NFRAG; ++i) {
        const int ob = i / CB, cb = i % CB;
        const f4 wv = wb[i % DD];
        if (i + DD < NFRAG) wb[i % DD] = ws.load(frag0 + ((i + DD) / CB) * WCB + ((i + DD) % CB));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int p = 0; p < P; ++p)
                acc[p][acc0 + ob] = pf_mfma(wv[r], in[p][in0 + cb][r], acc[p][acc0 + ob]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

typedef unsigned int u4 __attribute__((ext_vector_type(4)));

// ---- split-fp16 ("f16x2") path: fp32 accuracy in THREE fp16 MFMAs per 32-channel step ---------------
// x = hi + lo' * 2^-11 with hi = rne_f16(x) and lo' = rne_f16((x - hi) * 2^11): x - hi is exact in fp32 and at most
// half an fp16 ulp of x, so lo' never exceeds |x| (no overflow from the scale), is a normal fp16 number whenever x
// is (precision independent of magnitude) and hi + lo' 2^-11 carries 22+ significant bits.  A product keeps
// hi.hi in the main accumulator and hi.lo' + lo'.hi in a second one that is folded in as  acc + accx * 2^-11;
// the dropped lo.lo term is < 2^-24 relative.  gfx950's fp16 MFMA honours subnormal operands (probed), so tiny
// values degrade gracefully.  Range: |x| must stay below 65504 (fp16 max) - activations of this network are O(1..100);
// beyond it the result is inf/NaN (loud).  Used by csrc/cnf.hip; the eval kernels of the discrete path moved to the natural-scale variant below.
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef unsigned int u2 __attribute__((ext_vector_type(2)));
constexpr float PF_LO_SCALE = 2048.f, PF_LO_INV = 1.f / 2048.f;

__device__ __forceinline__ u2 pf_split2_pair(float a, float b) {
    unsigned hb = __builtin_bit_cast(unsigned, (h2){(_Float16)a, (_Float16)b});
    asm("" : "+v"(hb));          // opaque: read hi back from the packed register instead of converting twice
    const h2 h = __builtin_bit_cast(h2, hb);
    const h2 l = {(_Float16)((a - (float)h.x) * PF_LO_SCALE), (_Float16)((b - (float)h.y) * PF_LO_SCALE)};
    return (u2){hb, __builtin_bit_cast(unsigned, l)};
}

struct PfPair2 { h8 h, l; };
__device__ __forceinline__ PfPair2 pf_pair2(f4 b0, f4 b1) {
    const u2 s0 = pf_split2_pair(b0.x, b0.y), s1 = pf_split2_pair(b0.z, b0.w);
    const u2 s2 = pf_split2_pair(b1.x, b1.y), s3 = pf_split2_pair(b1.z, b1.w);
    PfPair2 p;
    p.h = __builtin_bit_cast(h8, (u4){s0.x, s1.x, s2.x, s3.x});
    p.l = __builtin_bit_cast(h8, (u4){s0.y, s1.y, s2.y, s3.y});
    return p;
}

__device__ __forceinline__ f4 pf_mfma_f16(h8 a, h8 b, f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

#ifndef PF_W2LDS_DEPTH
#define PF_W2LDS_DEPTH 2
#endif
// weights: [frag][2 splits hi / lo'][64 lanes] x 16 B in LDS
struct PfW2Lds {
    static constexpr int DEPTH = PF_W2LDS_DEPTH;   // fragments in flight (pf_mm2f): LDS latency
    const u4* base;
    int lane;
    __device__ __forceinline__ h8 load(int frag, int split) const {
        return __builtin_bit_cast(h8, base[(frag * 2 + split) * PF_WAVE + lane]);
    }
};

template <int DEPTH_>
struct PfW2BufD {
    static constexpr int DEPTH = DEPTH_;
    __amdgpu_buffer_rsrc_t rsrc;
    int voff;           // lane * 16
    __device__ __forceinline__ PfW2BufD(const void* p, int lane)
        : rsrc(__builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000)), voff(lane * 16) {}
    __device__ __forceinline__ h8 load(int frag, int split) const {
        return __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, (frag * 2 + split) * (PF_WAVE * 16), 0));
    }
};

// acc[p][acc0+ob] += Wh xh ;  accx[p][acc0+ob] += Wh xl' + Wl' xh   over block PAIRS cp < CP.
// Caller folds:  value = acc + accx * PF_LO_INV.  D fragments (two 16-B reads each) are kept in flight: 2 is enough
// for LDS-resident weights, L2-resident weights behind buffer loads want ~500 cycles of cover (a deeper PfW2BufD).
template <int OB, int CP, int WCP, int D = 2, class WS2, int P, int NIN, int NACC>
__device__ __forceinline__ void pf_mm2(const WS2& ws, int frag0, const PfPair2 (&in)[P][NIN], int in0,
                                       f4 (&acc)[P][NACC], f4 (&accx)[P][NACC], int acc0) {
    constexpr int NFRAG = OB * CP;
    constexpr int DD = D < NFRAG ? D : NFRAG;
    h8 wb[DD][2];
#pragma unroll
    for (int i = 0; i < DD; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s) wb[i][s] = ws.load(frag0 + (i / CP) * WCP + (i % CP), s);
#pragma unroll
    for (int i = 0; i < NFRAG; ++i) {
        const int ob = i / CP, cp = i % CP;
        const h8 wh = wb[i % DD][0], wl = wb[i % DD][1];
        if (i + DD < NFRAG) {
            const int f = frag0 + ((i + DD) / CP) * WCP + ((i + DD) % CP);
#pragma unroll
            for (int s = 0; s < 2; ++s) wb[i % DD][s] = ws.load(f, s);
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            f4 x = accx[p][acc0 + ob];
            x = pf_mfma_f16(wh, in[p][in0 + cp].l, x);
            x = pf_mfma_f16(wl, in[p][in0 + cp].h, x);
            accx[p][acc0 + ob] = x;
            acc[p][acc0 + ob] = pf_mfma_f16(wh, in[p][in0 + cp].h, acc[p][acc0 + ob]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// acc[p][acc0+ob] += W[ob][cp] in[p][cp] with the cross accumulator folded in (complete split-fp16 product)
template <int OB, int CP, int WCP, class WS2, int P, int NIN, int NACC>
__device__ __forceinline__ void pf_mm2f(const WS2& ws, int frag0, const PfPair2 (&in)[P][NIN], int in0,
                                        f4 (&acc)[P][NACC], int acc0) {
    f4 accx[P][OB];
    f4 accm[P][OB];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int o = 0; o < OB; ++o) { accx[p][o] = pf_splat(0.f); accm[p][o] = acc[p][acc0 + o]; }
    pf_mm2<OB, CP, WCP, WS2::DEPTH>(ws, frag0, in, in0, accm, accx, 0);
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int o = 0; o < OB; ++o) acc[p][acc0 + o] = accm[p][o] + accx[p][o] * PF_LO_INV;
}

// ---- split-fp16 with a NATURAL-scale low half ("f16n"): one accumulator, no fold ----------------------------------
// x = hi + lo, hi = rne_f16(x), lo = rne_f16(x - hi) written straight into the packed operand by v_fma_mixlo/mixhi_f16
// (3 VALU per value pair instead of 9).  gfx950's fp16 MFMA honours subnormal operands, so a small lo keeps an ABSOLUTE
// precision of 2^-25 in the units the operand is stored in; hosts keep that floor far below fp32 rounding by storing the
// weights scaled by a power of two (packing.frag_pack_f16n: max |W'| in [2^13, 2^14)) and, where the range allows,
// the activations too.  All three product terms (hi.hi, hi.lo, lo.hi) go into ONE fp32 accumulator.
struct PfPairN { h8 h, l; };
__device__ __forceinline__ unsigned pf_pk_f16(float a, float b) {
    return __builtin_bit_cast(unsigned, (h2){(_Float16)a, (_Float16)b});          // v_cvt_pk_f16_f32 (RNE)
}
__device__ __forceinline__ PfPairN pf_pairn(f4 b0, f4 b1) {
    const unsigned h0 = pf_pk_f16(b0.x, b0.y), h1 = pf_pk_f16(b0.z, b0.w), h2_ = pf_pk_f16(b1.x, b1.y), h3 = pf_pk_f16(b1.z, b1.w);
    unsigned l0, l1, l2, l3;
    // lo = fp16(x - hi) as fma(hi, -1, x); the trailing s_nop covers VALU write -> MFMA operand read (hipcc pads nothing
    // for registers written inside an asm statement)
    asm("v_fma_mixlo_f16 %0, %4, -1.0, %8 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixlo_f16 %1, %5, -1.0, %10 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixlo_f16 %2, %6, -1.0, %12 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixlo_f16 %3, %7, -1.0, %14 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %0, %4, -1.0, %9 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %1, %5, -1.0, %11 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %2, %6, -1.0, %13 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %3, %7, -1.0, %15 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "s_nop 1"
        : "=&v"(l0), "=&v"(l1), "=&v"(l2), "=&v"(l3)
        : "v"(h0), "v"(h1), "v"(h2_), "v"(h3), "v"(b0.x), "v"(b0.y), "v"(b0.z), "v"(b0.w), "v"(b1.x), "v"(b1.y), "v"(b1.z), "v"(b1.w));
    PfPairN p;
    p.h = __builtin_bit_cast(h8, (u4){h0, h1, h2_, h3});
    p.l = __builtin_bit_cast(h8, (u4){l0, l1, l2, l3});
    return p;
}

// ---- layer epilogues of the fused inference kernels: rescale, LeakyReLU / ReLU and the hi / lo split, single-issue fp32 only ----
// pf_pairn(pf_lrelu(v * inv, slope), ..) is written with 4-vector expressions, which hipcc turns into v_pk_mul_f32 (and, through
// SLP, packs neighbouring scalar fp32 math as well).  Beside MFMAs a packed fp32 op is dearer than the two plain ones it
// replaces, so the epilogues below do the same arithmetic - v * inv, then max(v, v * slope), then the split of pf_pairn, bit for
// bit - one value at a time.  The multiplies and the max stay C++ on purpose: they are the first readers of MFMA results, and
// hipcc pads the MFMA -> VALU read hazard only for instructions it issues itself, never for registers read inside an asm
// statement.  pf_opaque() ends the SLP vectoriser's search at each activated value; the split is asm as in pf_pairn.
// The rescale stays a multiply of its own: folding `inv` into the conversions (hi = f16(m * inv), lo = f16(m * inv - hi) with
// m = max(v, slope * v)) saves one instruction per value pair but is not the same bits where v * inv underflows fp32 - the
// separate multiply rounds to (signed) zero there and the low half of a zero is +0, the fused form keeps the sign.
__device__ __forceinline__ float pf_opaque(float v) { asm("" : "+v"(v)); return v; }

enum { PF_ACT_LRELU = 0, PF_ACT_RELU = 1 };
template <bool SCALE, int ACT>
__device__ __forceinline__ float pf_act1n(float v, float inv, float slope) {
    if constexpr (SCALE) v = v * inv;
    if constexpr (ACT == PF_ACT_RELU) return pf_opaque(fmaxf(v, 0.f));
    else return pf_opaque(fmaxf(v, v * slope));
}

// hi / lo split of one 16-channel block (half a PfPairN operand): two packed-fp16 registers each
struct PfHalfN { u2 h, l; };
__device__ __forceinline__ PfHalfN pf_splitn4(float x0, float x1, float x2, float x3) {
    const unsigned h0 = pf_pk_f16(x0, x1), h1 = pf_pk_f16(x2, x3);
    unsigned l0, l1;
    asm("v_fma_mixlo_f16 %0, %2, -1.0, %4 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixlo_f16 %1, %3, -1.0, %6 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %0, %2, -1.0, %5 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %1, %3, -1.0, %7 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "s_nop 1"
        : "=&v"(l0), "=&v"(l1)
        : "v"(h0), "v"(h1), "v"(x0), "v"(x1), "v"(x2), "v"(x3));
    return PfHalfN{(u2){h0, h1}, (u2){l0, l1}};
}
// the same for two blocks at once (the asm of pf_pairn on scalar operands: no 4-vector is built on the way in)
__device__ __forceinline__ PfPairN pf_splitn8(float x0, float x1, float x2, float x3, float x4, float x5, float x6, float x7) {
    const unsigned h0 = pf_pk_f16(x0, x1), h1 = pf_pk_f16(x2, x3), h2_ = pf_pk_f16(x4, x5), h3 = pf_pk_f16(x6, x7);
    unsigned l0, l1, l2, l3;
    asm("v_fma_mixlo_f16 %0, %4, -1.0, %8 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixlo_f16 %1, %5, -1.0, %10 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixlo_f16 %2, %6, -1.0, %12 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixlo_f16 %3, %7, -1.0, %14 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %0, %4, -1.0, %9 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %1, %5, -1.0, %11 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %2, %6, -1.0, %13 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %3, %7, -1.0, %15 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "s_nop 1"
        : "=&v"(l0), "=&v"(l1), "=&v"(l2), "=&v"(l3)
        : "v"(h0), "v"(h1), "v"(h2_), "v"(h3), "v"(x0), "v"(x1), "v"(x2), "v"(x3), "v"(x4), "v"(x5), "v"(x6), "v"(x7));
    PfPairN p;
    p.h = __builtin_bit_cast(h8, (u4){h0, h1, h2_, h3});
    p.l = __builtin_bit_cast(h8, (u4){l0, l1, l2, l3});
    return p;
}

template <bool SCALE, int ACT>
__device__ __forceinline__ PfPairN pf_act_pairn_t(f4 b0, f4 b1, float inv, float slope) {
    return pf_splitn8(pf_act1n<SCALE, ACT>(b0.x, inv, slope), pf_act1n<SCALE, ACT>(b0.y, inv, slope),
                      pf_act1n<SCALE, ACT>(b0.z, inv, slope), pf_act1n<SCALE, ACT>(b0.w, inv, slope),
                      pf_act1n<SCALE, ACT>(b1.x, inv, slope), pf_act1n<SCALE, ACT>(b1.y, inv, slope),
                      pf_act1n<SCALE, ACT>(b1.z, inv, slope), pf_act1n<SCALE, ACT>(b1.w, inv, slope));
}
template <bool SCALE, int ACT>
__device__ __forceinline__ PfHalfN pf_act_halfn_t(f4 b, float inv, float slope) {
    return pf_splitn4(pf_act1n<SCALE, ACT>(b.x, inv, slope), pf_act1n<SCALE, ACT>(b.y, inv, slope),
                      pf_act1n<SCALE, ACT>(b.z, inv, slope), pf_act1n<SCALE, ACT>(b.w, inv, slope));
}
// == pf_pairn(pf_lrelu(b0 * inv, slope), pf_lrelu(b1 * inv, slope));  inv, slope: wave-uniform
__device__ __forceinline__ PfPairN pf_act_pairn(f4 b0, f4 b1, float inv, float slope) { return pf_act_pairn_t<true, PF_ACT_LRELU>(b0, b1, inv, slope); }
// inv == 1 (the EdgeConv kernels: the scale plan leaves nothing to undo)
__device__ __forceinline__ PfPairN pf_act_pairn(f4 b0, f4 b1, float slope) { return pf_act_pairn_t<false, PF_ACT_LRELU>(b0, b1, 1.f, slope); }
// == pf_pairn(max(b0 * inv, 0), max(b1 * inv, 0))
__device__ __forceinline__ PfPairN pf_relu_pairn(f4 b0, f4 b1, float inv) { return pf_act_pairn_t<true, PF_ACT_RELU>(b0, b1, inv, 0.f); }
// one block at a time, for the 16-channel layers whose blocks reach a pair one layer apart: the earlier block's half is kept
// and joined with the next one instead of being split a second time.  A missing block is PfHalfN{} (the split of zeros).
__device__ __forceinline__ PfHalfN pf_act_halfn(f4 b, float inv, float slope) { return pf_act_halfn_t<true, PF_ACT_LRELU>(b, inv, slope); }
__device__ __forceinline__ PfHalfN pf_act_halfn(f4 b, float slope) { return pf_act_halfn_t<false, PF_ACT_LRELU>(b, 1.f, slope); }
__device__ __forceinline__ PfHalfN pf_relu_halfn(f4 b, float inv) { return pf_act_halfn_t<true, PF_ACT_RELU>(b, inv, 0.f); }
__device__ __forceinline__ PfPairN pf_join_halfn(PfHalfN a, PfHalfN b) {
    PfPairN p;
    p.h = __builtin_bit_cast(h8, (u4){a.h.x, a.h.y, b.h.x, b.h.y});
    p.l = __builtin_bit_cast(h8, (u4){a.l.x, a.l.y, b.l.x, b.l.y});
    return p;
}

// reduce-scatter max steps: (a, b) -> lanes 0..31 get max over both halves of a, lanes 32..63 of b;  rows: the same
// between odd and even 16-lane rows.  Inline asm because the builtin's two results are mis-paired by hipcc 7.2 once they
// are bit-cast to float; the leading s_nop is the VALU write -> permlane read hazard.
__device__ __forceinline__ float pf_rsmax32(float a, float b) {
    unsigned x = __builtin_bit_cast(unsigned, a), y = __builtin_bit_cast(unsigned, b);
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y));
    return fmaxf(__builtin_bit_cast(float, x), __builtin_bit_cast(float, y));
}
__device__ __forceinline__ float pf_rsmax16(float a, float b) {
    unsigned x = __builtin_bit_cast(unsigned, a), y = __builtin_bit_cast(unsigned, b);
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x), "+v"(y));
    return fmaxf(__builtin_bit_cast(float, x), __builtin_bit_cast(float, y));
}

// acc[p][o] += W[o][cp] feat[p][cp] over CP block pairs, three fp16 MFMAs per pair into the one accumulator (small terms
// first).  SWAP = false: D[channel][edge] (weights are the A operand);  SWAP = true: D[edge][channel].  The fragment walk is
// ob-major (one accumulator's whole chain, then the next); s_setprio around the chain was measured and dropped,
// as was a cp-major walk.  The non-SWAP step is pf_pq.h pq_step spelled out (that header sits above this one; SWAP adds
// its two small terms in the other order, lo.hi first).
// Products per 32-channel step: 3 = split-fp16 with the natural-scale low half (hi*lo + lo*hi + hi*hi: fp32-grade results,
// the parity mode and the default); 1 = hi*hi only - plain fp16 operands, fp32 accumulation: the reduced-precision THROUGHPUT
// build (`libpuflow_hip_f16.so`, BASELINE configs[1] "bf16/fp16" line; judged by Chamfer distance, never the headline)
#ifndef PF_MMN_TERMS
#define PF_MMN_TERMS 3
#endif
template <bool SWAP, int OB, int CP, int WCP, bool FENCE = true, class WS, int P, int NIN, int NACC>
__device__ __forceinline__ void pf_mmn(const WS& ws, int frag0, const PfPairN (&feat)[P][NIN], f4 (&acc)[P][NACC], int in0 = 0, int acc0 = 0) {
    constexpr int D = WS::DEPTH;                  // fragments in flight: 2 from LDS, 8 behind buffer loads (L2 latency)
    constexpr int NFRAG = OB * CP;
    constexpr int DD = D < NFRAG ? D : NFRAG;
    auto OBI = [](int i) { return i / CP; };
    auto CPI = [](int i) { return i % CP; };
    h8 wb[DD][2];
#pragma unroll
    for (int i = 0; i < DD; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s) wb[i][s] = ws.load(frag0 + OBI(i) * WCP + CPI(i), s);
#pragma unroll
    for (int i = 0; i < NFRAG; ++i) {
        const int ob = OBI(i), cp = CPI(i);
        const h8 wh = wb[i % DD][0], wl = wb[i % DD][1];
        if (i + DD < NFRAG) {
            const int f = frag0 + OBI(i + DD) * WCP + CPI(i + DD);
#pragma unroll
            for (int s = 0; s < 2; ++s) wb[i % DD][s] = ws.load(f, s);
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            f4 x = acc[p][acc0 + ob];
            if constexpr (SWAP) {
                if constexpr (PF_MMN_TERMS == 3) {
                    x = pf_mfma_f16(feat[p][in0 + cp].l, wh, x);
                    x = pf_mfma_f16(feat[p][in0 + cp].h, wl, x);
                }
                x = pf_mfma_f16(feat[p][in0 + cp].h, wh, x);
            } else {
                if constexpr (PF_MMN_TERMS == 3) {
                    x = pf_mfma_f16(wh, feat[p][in0 + cp].l, x);
                    x = pf_mfma_f16(wl, feat[p][in0 + cp].h, x);
                }
                x = pf_mfma_f16(wh, feat[p][in0 + cp].h, x);
            }
            acc[p][acc0 + ob] = x;
        }
        if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);      // FENCE = false: the caller interleaves two streams itself
    }
}

// ---- edge-table products as ONE MFMA ------------------------------------------------------------------------------------
// Every affine function of an edge's raw inputs e (8 values: x_i, x_j, a norm or 0, 1) is a product with an 8-column table T.
// As a split product through pf_mmn it costs three MFMAs whose k-slots are three quarters zeros.  The same three terms fit
// one: the B operand carries e_hi | e_lo | e_hi | 0 in the k-slots of lanes q = 0..3, the A operand T_hi | T_hi | T_lo | 0
// (packing._etab_frag1: one 1-KiB fp16 fragment per 16 table rows), and the sum over k is T_hi e_hi + T_hi e_lo + T_lo e_hi.
// PF_MMN_TERMS == 1 (the reduced-precision build) keeps T_hi e_hi alone: the operand's q = 1, 2 groups are zero then.
struct PfW1Lds {                                    // weights: [frag][64 lanes] x 16 B in LDS
    const u4* base;
    int lane;
    __device__ __forceinline__ h8 load(int frag) const { return __builtin_bit_cast(h8, base[frag * PF_WAVE + lane]); }
};
// e0 | e1: the 8 raw inputs of this lane's edge column, the same in all four q lanes of the column
__device__ __forceinline__ h8 pf_edge_operand(f4 e0, f4 e1, int q) {
    const PfPairN s = pf_pairn(e0, e1);
    const u4 h = __builtin_bit_cast(u4, s.h), l = __builtin_bit_cast(u4, s.l), z = {0u, 0u, 0u, 0u};
    if constexpr (PF_MMN_TERMS == 3) return __builtin_bit_cast(h8, q == 1 ? l : (q == 3 ? z : h));
    else return __builtin_bit_cast(h8, q == 0 ? h : z);
}
// acc[p][acc0 + ob] += T[ob] e[p] for ob < OB, one MFMA per fragment.  SWAP = true: D[edge][channel] (e is the A operand).
template <bool SWAP, int OB, class WS, int P, int NACC>
__device__ __forceinline__ void pf_mm1(const WS& ws, int frag0, const h8 (&e)[P], f4 (&acc)[P][NACC], int acc0 = 0) {
    h8 w[OB];
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) w[ob] = ws.load(frag0 + ob);
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) {
#pragma unroll
        for (int p = 0; p < P; ++p) {
            if constexpr (SWAP) acc[p][acc0 + ob] = pf_mfma_f16(e[p], w[ob], acc[p][acc0 + ob]);
            else acc[p][acc0 + ob] = pf_mfma_f16(w[ob], e[p], acc[p][acc0 + ob]);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}

// cooperative global -> LDS copy of n 16-byte words by the whole workgroup (call before a __syncthreads).  D loads per thread
// are in flight before the first LDS store: a plain load -> store loop pays one full memory latency per iteration, and at
// 88 - 152 KiB of weights per workgroup (6 - 32 iterations) that was most of what a small-batch launch of these kernels cost.
template <int D = 8, class T4>
__device__ __forceinline__ void pf_stage_lds(T4* __restrict__ dst, const T4* __restrict__ src, int n) {
    const int nt = blockDim.x;
    for (int base = threadIdx.x; base < n; base += nt * D) {
        T4 v[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const int i = base + k * nt;
            v[k] = src[i < n ? i : n - 1];
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const int i = base + k * nt;
            if (i < n) dst[i] = v[k];
        }
    }
}

// compile-time loop: f(std::integral_constant<int, I>) for I in [I0, N)
template <int I, int N, class F>
__device__ __forceinline__ void pf_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        pf_static_for<I + 1, N>(f);
    }
}

// bias / per-channel vector as accumulator initialiser: channels 16*ob + 4*q .. +3
__device__ __forceinline__ f4 pf_bias(const float* __restrict__ b, int ob, int q) {
    return *reinterpret_cast<const f4*>(b + ob * 16 + 4 * q);
}

// max over the 16 lanes of a DPP row (= the 16 columns of one MFMA tile); every lane gets the max.
__device__ __forceinline__ float pf_rowmax16(float v) { return pf_row_reduce(v, PfMax{}); }

// XCD-aware tile order (guide T1): virtual id v -> logical tile so that the workgroups that
// share an XCD (equal blockIdx % 8 under round-robin dispatch) walk one contiguous chunk of
// tiles (= the same batch items -> their gather table stays in that XCD's L2).  Speed only.
__device__ __forceinline__ int pf_xcd_tile(int v, int chunk) { return (v & 7) * chunk + (v >> 3); }
