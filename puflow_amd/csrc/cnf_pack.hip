// pf_cnf_pack_blocks: what packing.pack_cnf_block / pack_cnf_context / cnf_hyper_matrix make on the host from a state dict, made
// on the device from the LIVE parameter tensors of up to six CNF blocks in one launch - the weight record, the folded and the
// plain hyper matrices, the f16n fragment image of the context GEMM and a meta row (end time, image scale, status).  Bit for bit
// the host packers' results (tests/test_gpu_cnf_pack.py): every value is produced by the same sequence of roundings -
//   * the 2 log2e folds of W2, [W1 | b1] and b2 in double, rounded to fp32 once;
//   * the -log2e / 2 log2e folds of the hyper rows as ONE fp32 product with the fp32 constant (a zero row keeps the sign that
//     product gives it: the images compare as bits);
//   * f16x2: hi = fp16(W), lo = fp16((W - hi) 2^11); f16n: lo = fp16(W - hi) at natural scale, of W 2^sw with
//     sw = clip(13 - floor(log2 max|W|), -24, 40), 1.0 for an all-zero or non-finite matrix (packing.f16n_scale).
// A plain kernel: grid (CNF_PACK_PARTS, nb), every workgroup of a block takes the block's max |Hc| itself (one wave-level and
// one LDS step, 36 864 L2-resident reads at most) and then its share of the outputs, consecutive lanes writing consecutive
// floats.  No grid barrier, no atomics, nothing has to be resident together.
#include "pf_api_internal.h"
#include "pf_cnf.h"
#include "pf_wave.h"

namespace {

constexpr int CNF_PACK_MAXB = 6, CNF_PACK_SLOTS = 16, CNF_PACK_PARTS = 8, CNF_PACK_THREADS = 256;
// slots of a block's parameter table: per layer l (0..2) at 5 l + ..., then the end time
constexpr int SLOT_W = 0, SLOT_B = 1, SLOT_GATE_W = 2, SLOT_GATE_B = 3, SLOT_BIAS_W = 4, SLOT_SQRT_T = 15;
constexpr double LOG2E_D = 1.4426950408889634;
constexpr double TWO_LOG2E_D = 2.0 * LOG2E_D;
constexpr float NEG_LOG2E_F = (float)(-LOG2E_D), TWO_LOG2E_F = (float)TWO_LOG2E_D;      // np.float32(f) of the hyper rows' folds
constexpr float F16_LIMIT = 65504.f, F16_LO_SCALE = 2048.f;

struct PackArgs {
    const float* p[CNF_PACK_MAXB][CNF_PACK_SLOTS];
    float* hc[CNF_PACK_MAXB];
    float* hplain[CNF_PACK_MAXB];
    float* image[CNF_PACK_MAXB];
    int cd[CNF_PACK_MAXB];
    float* rec;
    float* hb;
    double* meta;
};

// row r of the context layout: which hyper weight it comes from (slot), which of its rows (-1: a padding row of layer 3's
// 4-float slots) and the constant the forward folds into it
struct CtxSrc { int slot, srow; float f; bool gate; };
__device__ __forceinline__ CtxSrc ctx_src(int r) {
    int l, kind, srow;
    if (r < CNF_CTX_G3) { l = r >> 7; kind = (r >> 6) & 1; srow = r & 63; }
    else { l = 2; kind = (r - CNF_CTX_G3) >> 4; srow = (r & 3) < 3 ? (r & 3) : -1; }
    return CtxSrc{5 * l + (kind == 0 ? SLOT_GATE_W : SLOT_BIAS_W), srow, kind == 0 ? NEG_LOG2E_F : (l < 2 ? TWO_LOG2E_F : 1.f), kind == 0};
}

// max that keeps a NaN (numpy's max does; a NaN matrix then takes scale 1 and sets no status, like the host packers)
struct NanMax {
    __device__ __forceinline__ float operator()(float a, float b) const { return (b > a || b != b) ? b : a; }
};
__device__ __forceinline__ float block_max(float v, float* lds) {
    v = pf_wave_reduce(v, NanMax{});
    __syncthreads();                                      // lds may still be read from the reduction before
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return NanMax{}(NanMax{}(lds[0], lds[1]), NanMax{}(lds[2], lds[3]));
}

__device__ __forceinline__ unsigned f16_bits(float v) { return __builtin_bit_cast(unsigned short, (_Float16)v); }
// one half of a split-fp16 pair: si = 0 the high half, 1 the low half (natural scale, or x 2^11)
__device__ __forceinline__ unsigned split_half(float v, int si, bool natural) {
    const _Float16 hi = (_Float16)v;
    if (si == 0) return __builtin_bit_cast(unsigned short, hi);
    const float d = v - (float)hi;
    return f16_bits(natural ? d : d * F16_LO_SCALE);
}
// float k of the fragment image [OB][CP][hi / lo][64 lanes][8 fp16] of a matrix (packing.frag_pack_f16x2 / frag_pack_f16n):
// its two fp16 are columns col, col + 1 of one row; val(row, col) is the fp32 matrix entry
template <class Val>
__device__ __forceinline__ float frag_word(int k, int CP, bool natural, Val val) {
    const int h = 2 * k, j = h & 7, lane = (h >> 3) & 63, si = (h >> 9) & 1, blk = h >> 10;
    const int cp = blk % CP, ob = blk / CP, q = lane >> 4;
    const int row = ob * 16 + (lane & 15);
    const int col = 32 * cp + (j < 4 ? 4 * q + j : 16 + 4 * q + (j - 4));
    const unsigned lo16 = split_half(val(row, col), si, natural), hi16 = split_half(val(row, col + 1), si, natural);
    return __builtin_bit_cast(float, lo16 | (hi16 << 16));
}

__device__ __forceinline__ float fold2(float w) { return (float)((double)w * TWO_LOG2E_D); }

__global__ __launch_bounds__(CNF_PACK_THREADS) void cnf_pack_kernel(PackArgs a) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const int cd = a.cd[b], ld = cd + 1, nhc = CNF_CTX * cd;
    const float* const* p = a.p[b];
    const float *W1 = p[SLOT_W], *b1 = p[SLOT_B], *W2 = p[5 + SLOT_W], *b2 = p[5 + SLOT_B], *W3 = p[10 + SLOT_W], *b3 = p[10 + SLOT_B];
    const int gtid = blockIdx.x * CNF_PACK_THREADS + threadIdx.x, gstride = gridDim.x * CNF_PACK_THREADS;

    auto hc_val = [&](int r, int c) -> float {            // the folded hyper matrix (packing.pack_cnf_block's Hc)
        const CtxSrc s = ctx_src(r);
        return (s.srow < 0 ? 0.f : p[s.slot][s.srow * ld + 1 + c]) * s.f;
    };

    // ---- the image's power-of-two scale: every workgroup of the block takes the maximum itself
    float m = 0.f;
    for (int k = threadIdx.x; k < nhc; k += CNF_PACK_THREADS) m = NanMax{}(m, fabsf(hc_val(k / cd, k % cd)));
    m = block_max(m, red);
    double sc = 1.0;
    if (m != 0.f && m == m && m != INFINITY) {
        int sw = 13 - ilogbf(m);
        sw = sw < -24 ? -24 : (sw > 40 ? 40 : sw);
        sc = ldexp(1.0, sw);
    }

    // ---- meta row: end time, the image's 2^-sw, status (1: an f16x2 image of the record, 2: the f16n image out of fp16's range)
    if (blockIdx.x == 0) {
        float mr = 0.f;
        for (int k = threadIdx.x; k < 64 * 64; k += CNF_PACK_THREADS) mr = NanMax{}(mr, NanMax{}(fabsf(W2[k]), fabsf(fold2(W2[k]))));
        for (int k = threadIdx.x; k < 3 * 64; k += CNF_PACK_THREADS) mr = NanMax{}(mr, fabsf(W3[k]));
        mr = block_max(mr, red);
        if (threadIdx.x == 0) {
            const double s = (double)p[SLOT_SQRT_T][0];
            const int status = (mr >= F16_LIMIT ? 1 : 0) | (fabsf((float)((double)m * sc)) >= F16_LIMIT ? 2 : 0);
            double* mt = a.meta + 4 * b;
            mt[0] = s * s; mt[1] = 1.0 / sc; mt[2] = (double)status; mt[3] = 0.0;
        }
    }

    // ---- weight record
    float* rec = a.rec + (size_t)b * CNF_REC;
    for (int k = gtid; k < CNF_REC; k += gstride) {
        float v;
        if (k < CNF_W2T) v = frag_word(k - CNF_W2, 2, false, [&](int r, int c) { return fold2(W2[r * 64 + c]); });
        else if (k < CNF_W3) v = frag_word(k - CNF_W2T, 2, false, [&](int r, int c) { return W2[c * 64 + r]; });
        else if (k < CNF_W1B) v = frag_word(k - CNF_W3, 2, false, [&](int r, int c) { return (r & 3) < 3 ? W3[(r & 3) * 64 + c] : 0.f; });
        else if (k < CNF_W3T) { const int i = k - CNF_W1B, r = i >> 2, c = i & 3; v = fold2(c < 3 ? W1[r * 3 + c] : b1[r]); }
        else if (k < CNF_B1) { const int i = k - CNF_W3T, r = i >> 2, c = i & 3; v = c < 3 ? W3[c * 64 + r] : 0.f; }
        else if (k < CNF_B2) v = b1[k - CNF_B1];
        else if (k < CNF_B3) v = fold2(b2[k - CNF_B2]);
        else if (k < CNF_TV) { const int i = k - CNF_B3; v = (i & 3) < 3 ? b3[i & 3] : 0.f; }
        else { const CtxSrc s = ctx_src(k - CNF_TV); v = (s.srow < 0 ? 0.f : p[s.slot][s.srow * ld]) * s.f; }
        rec[k] = v;
    }

    // ---- context GEMM: bias, folded and plain matrix, fragment image of Hc 2^sw
    for (int r = gtid; r < CNF_CTX; r += gstride) {
        const CtxSrc s = ctx_src(r);
        a.hb[b * CNF_CTX + r] = ((s.gate && s.srow >= 0) ? p[s.slot + 1][s.srow] : 0.f) * s.f;
    }
    float *hc = a.hc[b], *hplain = a.hplain[b], *image = a.image[b];
    const int CP = cd >> 5;
    for (int k = gtid; k < nhc; k += gstride) {
        const int r = k / cd, c = k % cd;
        const CtxSrc s = ctx_src(r);
        const float w = s.srow < 0 ? 0.f : p[s.slot][s.srow * ld + 1 + c];
        hplain[k] = w;
        hc[k] = w * s.f;
        image[k] = frag_word(k, CP, true, [&](int rr, int cc) { return (float)((double)hc_val(rr, cc) * sc); });
    }
}

}  // namespace

extern "C" int pf_cnf_pack_blocks(const float* const* params, const int* cd, int nb, float* rec, float* hb, void* const* hc,
                                  void* const* hplain, void* const* image, double* meta, void* stream) {
    if (!params || !cd || !rec || !hb || !hc || !hplain || !image || !meta) return PF_ERR_NULL;
    if (nb < 1 || nb > CNF_PACK_MAXB) return PF_ERR_SHAPE;
    PackArgs a{};
    for (int b = 0; b < nb; ++b) {
        if (cd[b] != 32 && cd[b] != 64 && cd[b] != 128) return PF_ERR_UNSUPPORTED;
        if (!hc[b] || !hplain[b] || !image[b]) return PF_ERR_NULL;
        for (int s = 0; s < CNF_PACK_SLOTS; ++s) {
            if (!params[b * CNF_PACK_SLOTS + s]) return PF_ERR_NULL;
            a.p[b][s] = params[b * CNF_PACK_SLOTS + s];
        }
        a.hc[b] = static_cast<float*>(hc[b]); a.hplain[b] = static_cast<float*>(hplain[b]); a.image[b] = static_cast<float*>(image[b]);
        a.cd[b] = cd[b];
    }
    a.rec = rec; a.hb = hb; a.meta = meta;
    hipLaunchKernelGGL(cnf_pack_kernel, dim3(CNF_PACK_PARTS, nb), dim3(CNF_PACK_THREADS), 0, (hipStream_t)stream, a);
    return pf_last_launch_status();
}

namespace {
// What a training step that never reads `meta` on the host needs of it (pf_cnf_pack_status): the context GEMM's scale as the
// float word pf_cnf_context_dev reads, and a status that cannot be raised there made visible on the device - the block's
// record becomes NaN (every integration on it then ends with status 1) and the sticky row latches it.  One workgroup walks the
// blocks, so the row has one writer.
__global__ __launch_bounds__(256) void cnf_pack_status_kernel(const double* __restrict__ meta, int nb, float* __restrict__ rec,
                                                              float* __restrict__ scales, int* sticky) {
    for (int b = 0; b < nb; ++b) {
        const int status = (int)meta[4 * b + 2];
        if (threadIdx.x < 8) scales[8 * b + threadIdx.x] = threadIdx.x == 6 ? (float)meta[4 * b + 1] : 0.f;
        if (status != 0)
            for (int k = threadIdx.x; k < CNF_REC; k += 256) rec[(size_t)b * CNF_REC + k] = __builtin_nanf("");
        if (threadIdx.x == 0) {
            sticky[0] += 1;
            if (status != 0) { sticky[1] += 1; sticky[2] = status; sticky[3] = b; }
        }
    }
}
}  // namespace

// After pf_cnf_pack_blocks, for a caller that does not read meta: scales [nb, 8] floats, word 6 of a row = meta[b][1] (the layout
// of the P|Q scale rows, which pf_cnf_context_dev's kernel reads); a non-zero status turns block b's record into NaN and is
// latched in sticky [4] = (calls x blocks, blocks with a status, last status, its block).
extern "C" int pf_cnf_pack_status(const double* meta, int nb, float* rec, float* scales, int* sticky, void* stream) {
    if (!meta || !rec || !scales || !sticky) return PF_ERR_NULL;
    if (nb < 1 || nb > CNF_PACK_MAXB) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(cnf_pack_status_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, meta, nb, rec, scales, sticky);
    return pf_last_launch_status();
}
