// The generic GEMM of the training step: C[M,N] = A(M,K) B(K,N) (+ bias[N]) (+ addend) on fp32 tensors with any element strides.
// It serves every Conv2d(1x1) / nn.Linear forward, dX and dW of the per-op tier (puflow_amd/train_perop.py LinearFn), the point
// GEMMs of the fused EdgeConv units (csrc/train_ec_fwd.hip, csrc/train_fused.hip) and the CNF context rows (puflow_amd/cnf.py).
//
//   gemm2_kernel       the fast path: f32 MFMA 16x16x4, float4 loads (operands 4-aligned in extent, stride and base),
//                      conflict-free LDS images, the tile leaves through LDS as whole rows
//   gemm_kernel        the general path: the same products in the same order for ANY strides, scalar guarded loads
//   gemm_split_kernel  the same tiles on the fp16 / bf16 matrix pipe (operands split into 2 / 3 parts while they are staged)
//   gemm_reduce_kernel sum of the split-K slabs (+ bias, + addend), fixed combine order
//
// Host side: gemm_shape() picks a tile shape id from (M, N), GEMM_TILES says which kernel copy runs it, gemm_plan() adds the
// split-K layout, pf_gemm_addend() launches.  pf_gemm / pf_gemm_ex / pf_gemm_reduce / pf_gemm_ws_floats are the C ABI.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <utility>
#include "pf_api_internal.h"
#include "pf_mfma.h"

namespace {

struct GemmArgs {
    const float* A; long long sam, sak;      // A(m,k) = A[m*sam + k*sak]
    const float* B; long long sbk, sbn;      // B(k,n) = B[k*sbk + n*sbn]
    float* C; long long ldc;                 // C(m,n) = C[m*ldc + n]   (or slab z: C + z*M*ldc)
    const float* bias;                       // per column n, nullable (ignored when splitk > 1: added by the reduce)
    int M, N, K, kchunk;                     // kchunk = K range per blockIdx.z
    const float* add;                        // nullable: C(m,n) += add[m*ldc + n] (same layout as C; may BE C; ignored when splitk > 1:
};                                           //           added by the reduce) - a gradient that already holds another consumer's part

// ---- what the three kernels share ---------------------------------------------------------------------------------------
// Output tile BM x BN per 256-thread workgroup: WAVES_M x WAVES_N waves, each TM x TN MFMA tiles of 16x16.  The host picks
// the shape from (M, N): layer GEMMs here are very skinny (N = 8..128 forward, M = 8..128 for dW), so a square tile would
// waste most of its MFMAs.
//
// Only helpers that leave every kernel's instruction stream as it was are shared: the accumulator zeroing and the direct
// epilogue stay spelled out in gemm_kernel and gemm_split_kernel (as helpers, whether they take the accumulators by reference
// or fragment by fragment, hipcc schedules several copies differently and turns a v_or into a v_add in two).
struct TileAt { int wm, wn, m0, n0, k_lo, k_hi; };      // the wave's place in the tile, the tile's origin, the slab's K range

// tile prologue: where this workgroup and this wave work
template <int WAVES_N, int BM, int BN>
__device__ __forceinline__ TileAt tile_at(int wave, int K, int kchunk) {
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int k_lo = blockIdx.z * kchunk;
    const int k_hi = min(K, k_lo + kchunk);
    return {wm, wn, m0, n0, k_lo, k_hi};
}

// host: may p be read or written with float4 accesses
__forceinline__ bool al16(const void* p) { return (reinterpret_cast<unsigned long long>(p) & 15ull) == 0; }

// ---- the general path: any strides, scalar guarded loads ----------------------------------------------------------------
// Stages 16-deep K steps through As[BM][20] / Bs[16][BN + 4], zero outside the bounds, and multiplies k ascending through
// v_mfma_f32_16x16x4_f32.  It is also arithmetic mode 1, the bit-identity reference of gemm2_kernel.
template <int WAVES_M, int WAVES_N, int TM, int TN>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs g) {
    constexpr int BM = WAVES_M * TM * 16, BN = WAVES_N * TN * 16;
    __shared__ float As[BM][20];          // [m][k], row stride 20 floats: 16-B aligned rows
    __shared__ float Bs[16][BN + 4];      // [k][n]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const TileAt t = tile_at<WAVES_N, BM, BN>(wave, g.K, g.kchunk);
    const int wm = t.wm, wn = t.wn, m0 = t.m0, n0 = t.n0, k_lo = t.k_lo, k_hi = t.k_hi;
    const bool a_kfast = g.sak == 1, b_nfast = g.sbn == 1;
    f4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = pf_splat(0.f);
    for (int k0 = k_lo; k0 < k_hi; k0 += 16) {
        for (int v = tid; v < BM * 16; v += 256) {
            const int r = a_kfast ? (v >> 4) : (v % BM);
            const int k = a_kfast ? (v & 15) : (v / BM);
            const int gm = m0 + r, gk = k0 + k;
            As[r][k] = (gm < g.M && gk < k_hi) ? g.A[gm * g.sam + gk * g.sak] : 0.f;
        }
        for (int v = tid; v < BN * 16; v += 256) {
            const int n = b_nfast ? (v % BN) : (v >> 4);
            const int kb = b_nfast ? (v / BN) : (v & 15);
            const int gn = n0 + n, gkb = k0 + kb;
            Bs[kb][n] = (gn < g.N && gkb < k_hi) ? g.B[gkb * g.sbk + gn * g.sbn] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = As[(wm * TM + i) * 16 + (lane & 15)][kk * 4 + (lane >> 4)];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Bs[kk * 4 + (lane >> 4)][(wn * TN + j) * 16 + (lane & 15)];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = pf_mfma(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
    // direct epilogue: every lane writes the four rows of its accumulator column (+ bias + addend) to C or its split-K slab
    float* C = g.C + (long long)blockIdx.z * g.M * g.ldc;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + (wn * TN + j) * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + (wm * TM + i) * 16 + 4 * (lane >> 4) + r;
                if (m < g.M && n < g.N) C[m * g.ldc + n] = acc[i][j][r] + (g.bias ? g.bias[n] : 0.f) + (g.add ? g.add[m * g.ldc + n] : 0.f);
            }
        }
}

// ---- the fast path: the same MFMA chain per output element (bit-identical results) with conflict-free LDS images ---------
// gemm_kernel transposes an operand whose contiguous dimension is NOT k with scalar ds_write_b32 at a 20-float stride (8-way
// bank conflicts), its b32 fragment reads are 2-way (PMC: 54 - 86 % of the LDS cycles were conflict cycles), every 16-deep step
// pays two barriers and the epilogue stores 64-byte pieces.  Here, for operands that take float4 loads:
//   * an operand that is contiguous along k goes to LDS in FRAGMENT order [16-k group][tile][lane = q 16 + row][j]
//     (element j of lane (row, q) is k = 4 j + q: what MFMA step j of the group reads), written by four ds_write_b32 whose
//     32-lane groups cover 32 banks, read back as ONE ds_read_b128 per tile and group;
//   * an operand that is contiguous along its row index (m / n) keeps its memory order [k][rows + 16]: ds_write_b128 rows,
//     ds_read_b32 fragments whose two k rows of a 32-lane group sit 16 banks apart;
//   * 32-deep steps, two LDS buffers, ONE barrier per step, the next step's operands in registers during the MFMAs;
//   * the output tile leaves through LDS as whole rows (float4 per lane).
// The products and their order are those of gemm_kernel (k ascending through v_mfma_f32_16x16x4_f32, the same split-K chunks).
template <int WAVES_M, int WAVES_N, int TM, int TN>
__global__ __launch_bounds__(256) void gemm2_kernel(GemmArgs g, int cvec) {
    constexpr int BM = WAVES_M * TM * 16, BN = WAVES_N * TN * 16, BK = 32;
    constexpr int LDA = BM % 32 == 0 ? BM + 16 : BM + 32, LDB = BN % 32 == 0 ? BN + 16 : BN + 32;   // row stride = 16 mod 32 floats
    constexpr int ASZ = BK * LDA, BSZ = BK * LDB, LDC = BN + 4;
    extern __shared__ __attribute__((aligned(16))) float g2lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ml = lane & 15, q = lane >> 4;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;      // tile_at() spelled out: with the helper four copies differ
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int k_lo = blockIdx.z * g.kchunk;
    const int k_hi = min(g.K, k_lo + g.kchunk);
    const bool a_kfast = g.sak == 1, b_kfast = g.sbk == 1 && g.sbn != 1;
    f4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = pf_splat(0.f);
    constexpr int NA = (BM * 8 + 255) / 256, NB = (BN * 8 + 255) / 256;
    f4 ra[NA], rb[NB];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int v = tid + i * 256;
            f4 x = pf_splat(0.f);
            if (v < BM * 8) {
                if (a_kfast) {
                    const int gm = m0 + (v >> 3), gk = k0 + (v & 7) * 4;
                    if (gm < g.M && gk < k_hi) x = *reinterpret_cast<const f4*>(g.A + gm * g.sam + gk);
                } else {
                    const int gk = k0 + v / (BM / 4), gm = m0 + (v % (BM / 4)) * 4;
                    if (gm < g.M && gk < k_hi) x = *reinterpret_cast<const f4*>(g.A + gk * g.sak + gm);
                }
            }
            ra[i] = x;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int v = tid + i * 256;
            f4 x = pf_splat(0.f);
            if (v < BN * 8) {
                if (b_kfast) {
                    const int gn = n0 + (v >> 3), gk = k0 + (v & 7) * 4;
                    if (gn < g.N && gk < k_hi) x = *reinterpret_cast<const f4*>(g.B + gn * g.sbn + gk);
                } else {
                    const int gk = k0 + v / (BN / 4), gn = n0 + (v % (BN / 4)) * 4;
                    if (gn < g.N && gk < k_hi) x = *reinterpret_cast<const f4*>(g.B + gk * g.sbk + gn);
                }
            }
            rb[i] = x;
        }
    };
    auto stash = [&](float* As, float* Bs) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int v = tid + i * 256;
            if (v < BM * 8) {
                const f4 x = ra[i];
                if (a_kfast) {
                    const int r = v >> 3, c = v & 7;
                    float* p = As + (c >> 2) * (BM * 16) + ((r >> 4) * 64 + (r & 15)) * 4 + (c & 3);
                    p[0] = x.x; p[64] = x.y; p[128] = x.z; p[192] = x.w;
                } else {
                    *reinterpret_cast<f4*>(As + (v / (BM / 4)) * LDA + (v % (BM / 4)) * 4) = x;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int v = tid + i * 256;
            if (v < BN * 8) {
                const f4 x = rb[i];
                if (b_kfast) {
                    const int r = v >> 3, c = v & 7;
                    float* p = Bs + (c >> 2) * (BN * 16) + ((r >> 4) * 64 + (r & 15)) * 4 + (c & 3);
                    p[0] = x.x; p[64] = x.y; p[128] = x.z; p[192] = x.w;
                } else {
                    *reinterpret_cast<f4*>(Bs + (v / (BN / 4)) * LDB + (v % (BN / 4)) * 4) = x;
                }
            }
        }
    };
    fetch(k_lo);
    stash(g2lds, g2lds + ASZ);
    __syncthreads();
    int cur = 0;
    for (int k0 = k_lo; k0 < k_hi; k0 += BK) {
        const float* As = g2lds + cur * (ASZ + BSZ);
        const float* Bs = As + ASZ;
        const bool more = k0 + BK < k_hi;
        if (more) fetch(k0 + BK);
#pragma unroll
        for (int gq = 0; gq < 2; ++gq) {
            f4 a[TM], b[TN];
            if (a_kfast) {
#pragma unroll
                for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const f4*>(As + gq * (BM * 16) + ((wm * TM + i) * 64 + lane) * 4);
            } else {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) a[i][kk] = As[(gq * 16 + kk * 4 + q) * LDA + (wm * TM + i) * 16 + ml];
            }
            if (b_kfast) {
#pragma unroll
                for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const f4*>(Bs + gq * (BN * 16) + ((wn * TN + j) * 64 + lane) * 4);
            } else {
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) b[j][kk] = Bs[(gq * 16 + kk * 4 + q) * LDB + (wn * TN + j) * 16 + ml];
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = pf_mfma(a[i][kk], b[j][kk], acc[i][j]);
        }
        if (more) {
            float* An = g2lds + (cur ^ 1) * (ASZ + BSZ);
            stash(An, An + ASZ);
        }
        __syncthreads();
        cur ^= 1;
    }
    // ---- the tile through LDS: [BM][BN + 4] (a lane group's two 4-row blocks sit 16 banks apart), then whole rows out
    float* Cs = g2lds;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) Cs[((wm * TM + i) * 16 + 4 * q + r) * LDC + (wn * TN + j) * 16 + ml] = acc[i][j][r];
    __syncthreads();
    float* C = g.C + (long long)blockIdx.z * g.M * g.ldc;
    for (int v = tid; v < BM * (BN / 4); v += 256) {
        const int row = v / (BN / 4), c4 = (v % (BN / 4)) * 4;
        const int m = m0 + row, n = n0 + c4;
        if (m >= g.M || n >= g.N) continue;
        f4 x = *reinterpret_cast<const f4*>(Cs + row * LDC + c4);
        if (cvec && n + 3 < g.N) {
            if (g.bias) { const f4 bb = *reinterpret_cast<const f4*>(g.bias + n); x += bb; }
            if (g.add) { const f4 aa = *reinterpret_cast<const f4*>(g.add + m * g.ldc + n); x += aa; }
            *reinterpret_cast<f4*>(C + m * g.ldc + n) = x;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (n + e < g.N) C[m * g.ldc + n + e] = x[e] + (g.bias ? g.bias[n + e] : 0.f) + (g.add ? g.add[m * g.ldc + n + e] : 0.f);
        }
    }
}

// ---- split-precision GEMM: the same tiles on the fp16 / bf16 matrix pipe ------------------------------------------
// The f32 MFMA runs at 1/16 of the 16-bit rate; the big layer GEMMs above already sit near ITS roofline.  Here both
// operands are split while they are staged into LDS ([row][k] images, k contiguous: one 16-B read per MFMA operand):
//   NS = 2  x = hi + lo in fp16 (natural-scale low half, pf_mfma.h "f16n"): 3 MFMAs per 32-deep step - forward GEMMs
//           (activations and weights are O(1e-3 .. 1e2): inside the fp16 range)
//   NS = 3  x = hi + mid + lo in bf16: 6 MFMAs per step, fp32 exponent range - the GEMMs that take a gradient operand
//           (dX = dY W, dW = dY^T X: gradients reach 1e-8 and would underflow an fp16 split)
// Results are fp32-class (>= 22 significant bits per product, fp32 accumulation); 5.3x / 2.7x fewer MFMA cycles than f32.
// VEC: float4 loads of 4 consecutive elements along each operand's contiguous dimension (4-aligned strides and bases).
template <int NS> struct SplitT;
template <> struct SplitT<2> { typedef _Float16 T; };
template <> struct SplitT<3> { typedef __bf16 T; };

template <int NS, int WAVES_M, int WAVES_N, int TM, int TN, bool VEC>
__global__ __launch_bounds__(256) void gemm_split_kernel(GemmArgs g) {
    typedef typename SplitT<NS>::T T;
    typedef T T8 __attribute__((ext_vector_type(8)));
    constexpr int BM = WAVES_M * TM * 16, BN = WAVES_N * TN * 16, BK = 32, LDK = BK + 8;   // row stride 80 B: 16-B aligned
    __shared__ T As[NS][BM][LDK];
    __shared__ T Bs[NS][BN][LDK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const TileAt t = tile_at<WAVES_N, BM, BN>(wave, g.K, g.kchunk);
    const int wm = t.wm, wn = t.wn, m0 = t.m0, n0 = t.n0, k_lo = t.k_lo, k_hi = t.k_hi;
    const bool a_kfast = g.sak == 1, b_kfast = g.sbk == 1;
    f4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = pf_splat(0.f);
    // one element -> its NS parts
    auto split_store = [&](T* p0, long long part_stride, float x) {
        if constexpr (NS == 2) {
            const _Float16 h = (_Float16)x;
            p0[0] = h;
            p0[part_stride] = (_Float16)(x - (float)h);
        } else {
            const __bf16 h = (__bf16)x;
            const float r1 = x - (float)h;
            const __bf16 m = (__bf16)r1;
            p0[0] = h;
            p0[part_stride] = m;
            p0[2 * part_stride] = (__bf16)(r1 - (float)m);
        }
    };
    constexpr long long PSA = (long long)BM * LDK, PSB = (long long)BN * LDK;

    for (int k0 = k_lo; k0 < k_hi; k0 += BK) {
        // ---- stage A [BM][BK] and B^T [BN][BK], converting on the way
        for (int v = tid; v < BM * (BK / 4); v += 256) {
            int r, k;
            f4 x = pf_splat(0.f);
            if (a_kfast) {                                      // 4 consecutive k of one row
                r = v / (BK / 4); k = (v % (BK / 4)) * 4;
                const int gm = m0 + r, gk = k0 + k;
                if (gm < g.M) {
                    if (VEC && gk + 3 < k_hi) x = *reinterpret_cast<const f4*>(g.A + gm * g.sam + gk);
                    else
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (gk + e < k_hi) x[e] = g.A[gm * g.sam + (gk + e) * g.sak];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) split_store(&As[0][r][k + e], PSA, x[e]);
            } else {                                            // 4 consecutive rows of one k
                k = v / (BM / 4); r = (v % (BM / 4)) * 4;
                const int gm = m0 + r, gk = k0 + k;
                if (gk < k_hi) {
                    if (VEC && gm + 3 < g.M) x = *reinterpret_cast<const f4*>(g.A + gk * g.sak + gm * g.sam);
                    else
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (gm + e < g.M) x[e] = g.A[(gm + e) * g.sam + gk * g.sak];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) split_store(&As[0][r + e][k], PSA, x[e]);
            }
        }
        for (int v = tid; v < BN * (BK / 4); v += 256) {
            int n, k;
            f4 x = pf_splat(0.f);
            if (b_kfast) {                                      // 4 consecutive k of one column n
                n = v / (BK / 4); k = (v % (BK / 4)) * 4;
                const int gn = n0 + n, gk = k0 + k;
                if (gn < g.N) {
                    if (VEC && gk + 3 < k_hi) x = *reinterpret_cast<const f4*>(g.B + gn * g.sbn + gk);
                    else
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (gk + e < k_hi) x[e] = g.B[(gk + e) * g.sbk + gn * g.sbn];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) split_store(&Bs[0][n][k + e], PSB, x[e]);
            } else {                                            // 4 consecutive n of one k
                k = v / (BN / 4); n = (v % (BN / 4)) * 4;
                const int gn = n0 + n, gk = k0 + k;
                if (gk < k_hi) {
                    if (VEC && gn + 3 < g.N) x = *reinterpret_cast<const f4*>(g.B + gk * g.sbk + gn * g.sbn);
                    else
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (gn + e < g.N) x[e] = g.B[gk * g.sbk + (gn + e) * g.sbn];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) split_store(&Bs[0][n + e][k], PSB, x[e]);
            }
        }
        __syncthreads();
        T8 a[NS][TM], b[NS][TN];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int i = 0; i < TM; ++i) a[s][i] = *reinterpret_cast<const T8*>(&As[s][(wm * TM + i) * 16 + (lane & 15)][8 * (lane >> 4)]);
#pragma unroll
            for (int j = 0; j < TN; ++j) b[s][j] = *reinterpret_cast<const T8*>(&Bs[s][(wn * TN + j) * 16 + (lane & 15)][8 * (lane >> 4)]);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                f4 x = acc[i][j];
                if constexpr (NS == 2) {
                    x = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0][i], b[1][j], x, 0, 0, 0);
                    x = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[1][i], b[0][j], x, 0, 0, 0);
                    x = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0][i], b[0][j], x, 0, 0, 0);
                } else {
                    x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][i], b[2][j], x, 0, 0, 0);
                    x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2][i], b[0][j], x, 0, 0, 0);
                    x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][i], b[1][j], x, 0, 0, 0);
                    x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][i], b[1][j], x, 0, 0, 0);
                    x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][i], b[0][j], x, 0, 0, 0);
                    x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][i], b[0][j], x, 0, 0, 0);
                }
                acc[i][j] = x;
            }
        __syncthreads();
    }
    // direct epilogue, the text of gemm_kernel's
    float* C = g.C + (long long)blockIdx.z * g.M * g.ldc;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + (wn * TN + j) * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + (wm * TM + i) * 16 + 4 * (lane >> 4) + r;
                if (m < g.M && n < g.N) C[m * g.ldc + n] = acc[i][j][r] + (g.bias ? g.bias[n] : 0.f) + (g.add ? g.add[m * g.ldc + n] : 0.f);
            }
        }
}

// C = sum over split-K slabs (+ bias): 64 consecutive outputs x 4 slab lanes per workgroup, fixed combine order
__global__ __launch_bounds__(256) void gemm_reduce_kernel(const float* __restrict__ slabs, float* C,
                                                         const float* __restrict__ bias, int M, int N, long long ldc,
                                                         int nslab, const float* add) {
    __shared__ float sh[4][64];
    const int l = threadIdx.x & 63, part = threadIdx.x >> 6;
    const long long t = (long long)blockIdx.x * 64 + l;
    const long long MN = (long long)M * N;
    float s = 0.f;
    if (t < MN)
        for (int z = part; z < nslab; z += 4) s += slabs[(long long)z * MN + t];
    sh[part][l] = s;
    __syncthreads();
    if (part == 0 && t < MN) {
        const int m = (int)(t / N), n = (int)(t % N);
        C[m * ldc + n] = ((sh[0][l] + sh[1][l]) + (sh[2][l] + sh[3][l])) + (bias ? bias[n] : 0.f) + (add ? add[m * ldc + n] : 0.f);
    }
}

// ---- host: tile shapes ---------------------------------------------------------------------------------------------------
// One row per shape id: the <WAVES_M, WAVES_N, TM, TN> of the gemm2_kernel copy that runs it, and of the gemm_kernel /
// gemm_split_kernel copy.  Ids 8 and 9 exist as real tiles for gemm2_kernel only; the other two kernels run 64 x 64 there.
struct Tile {
    int waves_m, waves_n, tm, tn;
    constexpr int bm() const { return waves_m * tm * 16; }
    constexpr int bn() const { return waves_n * tn * 16; }
};
struct TileRow { Tile fast, general; };
constexpr int GEMM_SHAPES = 10;
constexpr TileRow GEMM_TILES[GEMM_SHAPES] = {
    {{2, 2, 4, 4}, {2, 2, 4, 4}},        // 0  128 x 128
    {{4, 1, 4, 1}, {4, 1, 4, 1}},        // 1  256 x 16   skinny N
    {{4, 1, 4, 2}, {4, 1, 4, 2}},        // 2  256 x 32
    {{4, 1, 4, 4}, {4, 1, 4, 4}},        // 3  256 x 64
    {{1, 4, 1, 4}, {1, 4, 1, 4}},        // 4  16 x 256   skinny M
    {{1, 4, 2, 4}, {1, 4, 2, 4}},        // 5  32 x 256
    {{1, 4, 4, 4}, {1, 4, 4, 4}},        // 6  64 x 256
    {{2, 2, 2, 2}, {2, 2, 2, 2}},        // 7  64 x 64
    {{2, 2, 1, 2}, {2, 2, 2, 2}},        // 8  32 x 64
    {{2, 2, 1, 1}, {2, 2, 2, 2}},        // 9  32 x 32
};

// calls f(std::integral_constant<int, shape>): the row of a run-time shape id as a compile-time constant.  False for an id
// outside the table.
template <class F, int... I>
bool with_shape(int shape, F&& f, std::integer_sequence<int, I...>) {
    return ((shape == I && (f(std::integral_constant<int, I>{}), true)) || ...);
}

// A skinny output that would leave the chip with one 4-wave workgroup per CU or less takes small tiles: 64 x 64 (shape 7), or -
// where even those are at most GEMM_SMALL_TILE_MAX (the [8192, 32..128] input gradients of the EdgeConv units: 128 / 256 tiles,
// every k-step's loads exposed) - 32 x 32 (9; 32 x 64 = 8 for N <= 32).  One MI355X, [8192, C] x K = 4 S: C = 32: 14.4 -> 10.6 us,
// 64: 24.9 -> 15.7, 128: 25.1 -> 21.9; training step 4.13 -> 4.08 ms
constexpr long long GEMM_SMALL_TILE_MAX = 256;
inline int gemm_small_tile(int M, int N) {
    const long long t64 = (long long)((M + 63) / 64) * ((N + 63) / 64);
    if (t64 <= GEMM_SMALL_TILE_MAX && M >= 32 && N > 32) return 9;
    if (t64 <= GEMM_SMALL_TILE_MAX && M >= 32) return 8;
    return 7;
}
// shape id for (M, N): 0 = 128x128, 1..3 = 256 x {16,32,64} (skinny N), 4..6 = {16,32,64} x 256 (skinny M), 7..9 small tiles
inline int gemm_shape(int M, int N) {
    // a skinny output whose 256-row tiles would not even give every second CU a workgroup (the [8192, 16..64] input-gradient
    // GEMMs of the training step: 32 tiles, 65 us for 0.27 G MAC) takes 64 x 64 tiles instead: 4 x the workgroups, no split-K
    // reduction, the wasted tile columns cost nothing at this size
    if (N <= 64 && M > 64 && (M + 255) / 256 < 128 && (M + 63) / 64 >= 64) return gemm_small_tile(M, N);
    if (N <= 16) return 1;
    if (N <= 32) return 2;
    if (N <= 64 && M > 64) return 3;
    if (M <= 16) return 4;
    if (M <= 32) return 5;
    if (M <= 64) return 6;
    // 128 x 128 tiles leave most CUs idle on the point-level GEMMs of the training step ([8192, 128..512] outputs: 64..256
    // tiles, one 1-wave-per-SIMD workgroup per CU): 64 x 64 tiles there
    if ((long long)((M + 127) / 128) * ((N + 127) / 128) < 1024) return gemm_small_tile(M, N);
    return 0;
}

// ---- host: the plan of one product ------------------------------------------------------------------------------------
struct GemmPlan {
    int shape;               // row of GEMM_TILES
    int split, kchunk;       // blockIdx.z = 0..split-1 multiplies K range [z kchunk, (z + 1) kchunk); kchunk is a multiple of 32
    long long ws_floats;     // the workspace the caller provides: 0 = no split-K, else room for the slabs [.][M, N]
};
GemmPlan gemm_plan(int M, int N, int K) {
    GemmPlan p{gemm_shape(M, N), 1, 0, 0};
    // The split count ALWAYS follows gemm2_kernel's tile of the shape, whichever kernel and arithmetic run it (the general and
    // split kernels cover ids 8 and 9 with fewer, larger tiles): equal K chunks are what makes arith 0 and arith 1 bit-identical.
    const Tile& t = GEMM_TILES[p.shape].fast;
    const long long tiles = (long long)((M + t.bm() - 1) / t.bm()) * ((N + t.bn() - 1) / t.bn());
    // split-K when the output has too few tiles to fill 256 CUs (dW GEMMs: tiny M x N, K = rows up to 131072):
    // aim at ~1024 workgroups, K chunks of at least 128, slabs capped at 16 M floats
    int split = 1;
    if (tiles < 512 && K >= 1024) {
        long long sp = (1024 + tiles - 1) / tiles;
        if (sp > K / 128) sp = K / 128;
        const long long cap = (16ll << 20) / ((long long)M * N);
        if (sp > cap) sp = cap;
        if (sp > 256) sp = 256;
        split = sp < 1 ? 1 : (int)sp;
    }
    p.ws_floats = split > 1 ? (long long)split * M * N : 0;
    p.kchunk = ((K + split - 1) / split + 31) / 32 * 32;      // whole 32-deep steps: fewer slabs than `split` may remain
    p.split = (K + p.kchunk - 1) / p.kchunk;
    return p;
}

// ---- host: launches ------------------------------------------------------------------------------------------------------
template <int BM, int BN>
dim3 gemm_grid(const GemmArgs& g, int split) { return dim3((g.N + BN - 1) / BN, (g.M + BM - 1) / BM, split); }

template <int WAVES_M, int WAVES_N, int TM, int TN>
void gemm2_launch(const GemmArgs& g, int split, hipStream_t s) {
    constexpr int BM = WAVES_M * TM * 16, BN = WAVES_N * TN * 16;
    constexpr int LDA = BM % 32 == 0 ? BM + 16 : BM + 32, LDB = BN % 32 == 0 ? BN + 16 : BN + 32;
    constexpr int loop_floats = 2 * 32 * (LDA + LDB), out_floats = BM * (BN + 4);
    constexpr size_t lds = sizeof(float) * (size_t)(loop_floats > out_floats ? loop_floats : out_floats);
    allow_lds(gemm2_kernel<WAVES_M, WAVES_N, TM, TN>, lds);
    const long long ldc = g.ldc;
    const int cvec = (ldc % 4 == 0) && al16(g.C) && (!g.bias || al16(g.bias)) && (!g.add || al16(g.add)) && (((long long)g.M * ldc) % 4 == 0);
    hipLaunchKernelGGL((gemm2_kernel<WAVES_M, WAVES_N, TM, TN>), (gemm_grid<BM, BN>(g, split)), dim3(256), lds, s, g, cvec);
}

template <int WAVES_M, int WAVES_N, int TM, int TN>
void gemm_launch(const GemmArgs& g, int split, hipStream_t s) {
    hipLaunchKernelGGL((gemm_kernel<WAVES_M, WAVES_N, TM, TN>), (gemm_grid<WAVES_M * TM * 16, WAVES_N * TN * 16>(g, split)), dim3(256), 0, s, g);
}

template <int NS, int WAVES_M, int WAVES_N, int TM, int TN>
void gemm_split_launch(const GemmArgs& g, int split, bool vec, hipStream_t s) {
    const dim3 grid = gemm_grid<WAVES_M * TM * 16, WAVES_N * TN * 16>(g, split);
    if (vec) hipLaunchKernelGGL((gemm_split_kernel<NS, WAVES_M, WAVES_N, TM, TN, true>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((gemm_split_kernel<NS, WAVES_M, WAVES_N, TM, TN, false>), grid, dim3(256), 0, s, g);
}

void gemm_reduce_launch(const float* slabs, float* C, const float* bias, int M, int N, long long ldc, int nslab, const float* add,
                        hipStream_t s) {
    hipLaunchKernelGGL(gemm_reduce_kernel, dim3((unsigned)(((long long)M * N + 63) / 64)), dim3(256), 0, s, slabs, C, bias, M, N, ldc,
                       nslab, add);
}

}  // namespace

// C[M,N] = A(M,K) B(K,N) (+ bias[N]); generic element strides.  ws: split-K slabs (>= pf_gemm_ws_floats).
extern "C" long long pf_gemm_ws_floats(int M, int N, int K) { return gemm_plan(M, N, K).ws_floats; }

// arith: 0 = f32 MFMA (bit-exact fp32 fma chain): gemm2_kernel when both operands take float4 loads, else gemm_kernel;
// 1 = gemm_kernel whatever the operands (the bit-identity reference of 0: tests/test_gpu_train_fused.py);
// 2 = split-fp16 (forward GEMMs), 3 = split-bf16 (gradient operands)
extern "C" int pf_gemm_ex(int arith, const float* A, long long sam, long long sak, const float* B, long long sbk, long long sbn,
                          float* C, long long ldc, const float* bias, int M, int N, int K, float* ws, long long ws_floats,
                          void* stream) {
    return pf_gemm_addend(arith, A, sam, sak, B, sbk, sbn, C, ldc, bias, nullptr, M, N, K, ws, ws_floats, stream, nullptr);
}
// (internal, pf_api_internal.h) the same with an addend: C = A B + bias + addend, addend [M, ldc] laid out like C (it may be C)
int pf_gemm_addend(int arith, const float* A, long long sam, long long sak, const float* B, long long sbk, long long sbn,
                   float* C, long long ldc, const float* bias, const float* addend, int M, int N, int K, float* ws,
                   long long ws_floats, void* stream, int* slabs_left) {
    if (slabs_left) *slabs_left = 0;
    if (arith != 0 && arith != 1 && arith != 2 && arith != 3) return PF_ERR_UNSUPPORTED;
    if (!A || !B || !C) return PF_ERR_NULL;
    if (M <= 0 || N <= 0 || K <= 0) return PF_ERR_SHAPE;
    const GemmPlan p = gemm_plan(M, N, K);
    const bool use_ws = p.ws_floats > 0;
    if (use_ws && (!ws || ws_floats < p.ws_floats)) return PF_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const GemmArgs g{A, sam, sak, B, sbk, sbn, use_ws ? ws : C, use_ws ? (long long)N : ldc, use_ws ? nullptr : bias, M, N, K, p.kchunk,
                     use_ws ? nullptr : addend};
    bool vec;
    if (arith < 2) {
        // gemm2_kernel's float4 loads: the contiguous dimension of each operand must be 4-aligned in extent, stride and base
        const bool va = (sak == 1) ? (K % 4 == 0 && sam % 4 == 0 && g.kchunk % 4 == 0) : (sam == 1 && M % 4 == 0 && sak % 4 == 0);
        const bool vb = (sbn == 1) ? (N % 4 == 0 && sbk % 4 == 0) : (sbk == 1 && K % 4 == 0 && sbn % 4 == 0);
        vec = arith == 0 && va && vb && al16(A) && al16(B);
    } else {
        // gemm_split_kernel's: 4 consecutive elements along each operand's contiguous dimension (it guards the extents itself)
        const bool va = (sak == 1) ? (sam % 4 == 0) : (sam == 1 && sak % 4 == 0);
        const bool vb = (sbk == 1) ? (sbn % 4 == 0) : (sbn == 1 && sbk % 4 == 0);
        vec = va && vb && al16(A) && al16(B);
    }
    const bool known = with_shape(p.shape, [&](auto id) {
        constexpr Tile f = GEMM_TILES[decltype(id)::value].fast, t = GEMM_TILES[decltype(id)::value].general;
        if (arith == 2) gemm_split_launch<2, t.waves_m, t.waves_n, t.tm, t.tn>(g, p.split, vec, s);
        else if (arith == 3) gemm_split_launch<3, t.waves_m, t.waves_n, t.tm, t.tn>(g, p.split, vec, s);
        else if (vec) gemm2_launch<f.waves_m, f.waves_n, f.tm, f.tn>(g, p.split, s);
        else gemm_launch<t.waves_m, t.waves_n, t.tm, t.tn>(g, p.split, s);
    }, std::make_integer_sequence<int, GEMM_SHAPES>{});
    if (!known) return PF_ERR_UNSUPPORTED;                                    // gemm_shape() returned an id without a row
    if (use_ws && slabs_left && !bias && !addend) *slabs_left = p.split;     // the caller sums the slabs itself
    else if (use_ws) gemm_reduce_launch(ws, C, bias, M, N, ldc, p.split, addend, s);
    return pf_last_launch_status();
}

// C [M, ldc] = sum of nslab split-K slabs [nslab][M * N] (fixed combine order): the reduction step of pf_gemm, for callers that
// produce their own slabs (csrc/train_fused.hip)
extern "C" int pf_gemm_reduce(const float* slabs, float* C, int M, int N, long long ldc, int nslab, void* stream) {
    if (!slabs || !C) return PF_ERR_NULL;
    if (M <= 0 || N <= 0 || nslab <= 0) return PF_ERR_SHAPE;
    gemm_reduce_launch(slabs, C, nullptr, M, N, ldc, nslab, nullptr, (hipStream_t)stream);
    return pf_last_launch_status();
}

extern "C" int pf_gemm(const float* A, long long sam, long long sak, const float* B, long long sbk, long long sbn, float* C,
                       long long ldc, const float* bias, int M, int N, int K, float* ws, long long ws_floats, void* stream) {
    return pf_gemm_ex(0, A, sam, sak, B, sbk, sbn, C, ldc, bias, M, N, K, ws, ws_floats, stream);
}
