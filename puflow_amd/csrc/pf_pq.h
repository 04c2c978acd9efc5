// The P|Q row-block product PQ' = Wpq h + bpq (and pf_cnf_context's ctx = Hc c + hb), written once: a split-fp16 ("f16n",
// pf_mfma.h) GEMM with the WEIGHTS as the A operand, 16 points per MFMA column tile.  Device only.  Used by
//   pointwise.hip  pq_gemm_kernel   two launches; weights resident for the launch, linear rounds of tiles
//   edgeconv.hip   pqf_gemm         inside the EdgeConv tile loop; weights from L2 per flush, the staged-tile list
//   edgeconv.hip   pq_tail          tail of the EdgeConv launch; weights resident for the tail, the XCD-aware walk
// which differ in the tile walk, in where the weights live and in how staging is split over the waves - nothing else: the
// products, their order, the rescale and the table layout below are these helpers', so the three forms write the same bits.
//
// Layouts (u4 = 16 B = 8 fp16):
//   weight image   [ROWS / 16 row blocks][CP][hi / lo][64 lanes] u4   (packing.frag_pack_f16n_scaled), CP = 32-channel pairs
//   staged tile    [CP][hi / lo][64 lanes] u4 in LDS: the B operands of 16 points; PQ_TILE_U4<CP> words, tiles back to back
//   B operand      channel ch of point column pt sits in lane 16 ((ch & 15) >> 2) + pt, element 4 ((ch >> 4) & 1) + (ch & 3)
//                  of pair ch >> 5 (lane (col, q) holds channels 4 q .. 4 q + 3 of both 16-channel blocks of the pair)
//   table          [T][ROWS] fp32; lane (col, q) writes rows 16 ob + 4 q .. + 3 of point col of the tile
// Per accumulator: cp ascending, hi.lo, lo.hi, hi.hi (small terms first), then fmaf(acc, inv, bias).
//
// The helpers take scalars, pointers and references to register arrays, never a kernel's argument struct: hipcc optimises
// a kernel before it inlines even an always-inline helper, so what a helper takes decides the instruction order afterwards
// (profiles/refactor_pq/README.md).
#pragma once
#include "pf_mfma.h"

template <int CP>
constexpr int PQ_TILE_U4 = CP * 2 * 64;                        // u4 words of one staged tile

__device__ __forceinline__ constexpr int pq_frag_u4(int cp, int split, int lane) { return (cp * 2 + split) * 64 + lane; }
__device__ __forceinline__ constexpr int pq_b_lane(int ch, int pt) { return 16 * ((ch & 15) >> 2) + pt; }
__device__ __forceinline__ constexpr int pq_b_elem(int ch) { return ((ch >> 4) & 1) * 4 + (ch & 3); }

// the three-term step of one 32-channel pair; the only reader of PF_MMN_TERMS in the P|Q code (1: hi.hi alone)
__device__ __forceinline__ f4 pq_step(h8 wh, h8 wl, h8 fh, h8 fl, f4 acc) {
    if constexpr (PF_MMN_TERMS == 3) {
        acc = pf_mfma_f16(wh, fl, acc);
        acc = pf_mfma_f16(wl, fh, acc);
    }
    return pf_mfma_f16(wh, fh, acc);
}

// the fragment pairs of row blocks blk0 .. blk0 + NB - 1 into registers (plain loads)
template <int NB, int CP>
__device__ __forceinline__ void pq_load_w(const u4* w, int blk0, int lane, h8 (&wh)[NB][CP], h8 (&wl)[NB][CP]) {
#pragma unroll
    for (int ob = 0; ob < NB; ++ob)
#pragma unroll
        for (int cp = 0; cp < CP; ++cp) {
            const u4* f = w + (size_t)pq_frag_u4((blk0 + ob) * CP + cp, 0, 0) + lane;
            wh[ob][cp] = __builtin_bit_cast(h8, f[0]);
            wl[ob][cp] = __builtin_bit_cast(h8, f[64]);
        }
}

// stage one (tile, 32-channel pair) unit: b0 | b1 = this lane's 4 channels of the pair's two 16-channel blocks (b1 = 0 past an
// odd block count), frag = the unit's hi fragment in LDS.  Second form: the two blocks read from the point's row, hr = its
// first block's 4 channels (a caller that stages a whole tile reads all its blocks first and uses the first form: one latency).
__device__ __forceinline__ void pq_stage_unit(u4* frag, f4 b0, f4 b1, int lane) {
    const PfPairN p = pf_pairn(b0, b1);
    frag[lane] = __builtin_bit_cast(u4, p.h);
    frag[64 + lane] = __builtin_bit_cast(u4, p.l);
}
__device__ __forceinline__ void pq_stage_unit(u4* frag, const float* hr, int lane) {
    pq_stage_unit(frag, *reinterpret_cast<const f4*>(hr), *reinterpret_cast<const f4*>(hr + 16), lane);
}

// acc[ob] = W[ob] x (staged tile) for the NB resident row blocks
template <int NB, int CP>
__device__ __forceinline__ void pq_tile_product(const u4* tile, int lane, const h8 (&wh)[NB][CP], const h8 (&wl)[NB][CP], f4 (&acc)[NB]) {
#pragma unroll
    for (int ob = 0; ob < NB; ++ob) acc[ob] = pf_splat(0.f);
#pragma unroll
    for (int cp = 0; cp < CP; ++cp) {
        const h8 fh = __builtin_bit_cast(h8, tile[pq_frag_u4(cp, 0, lane)]), fl = __builtin_bit_cast(h8, tile[pq_frag_u4(cp, 1, lane)]);
#pragma unroll
        for (int ob = 0; ob < NB; ++ob) acc[ob] = pq_step(wh[ob][cp], wl[ob][cp], fh, fl, acc[ob]);
    }
}

// rescale, bias and store of row blocks blk0 .. blk0 + NB - 1 of point pt: this lane's rows 16 ob + 4 q .. + 3.  The bias comes
// from registers (pq_gemm_kernel) or through bias = b + 16 blk0 + 4 q (the fused forms read it from L1 to stay at 128 VGPRs).
template <int ROWS, int NB>
__device__ __forceinline__ void pq_tile_store(float* table, int pt, int blk0, int q, const f4 (&acc)[NB], float inv, const f4 (&bias)[NB]) {
#pragma unroll
    for (int ob = 0; ob < NB; ++ob) {
        f4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = fmaf(acc[ob][r], inv, bias[ob][r]);
        *reinterpret_cast<f4*>(table + (size_t)pt * ROWS + (blk0 + ob) * 16 + 4 * q) = o;
    }
}
template <int ROWS, int NB>
__device__ __forceinline__ void pq_tile_store(float* table, int pt, int blk0, int q, const f4 (&acc)[NB], float inv, const float* bias) {
#pragma unroll
    for (int ob = 0; ob < NB; ++ob) {
        const f4 b = *reinterpret_cast<const f4*>(bias + ob * 16);
        f4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = fmaf(acc[ob][r], inv, b[r]);
        *reinterpret_cast<f4*>(table + (size_t)pt * ROWS + (blk0 + ob) * 16 + 4 * q) = o;
    }
}
