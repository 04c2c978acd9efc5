// Patch pipeline operators around the network: farthest point sampling and the
// large-K patch kNN.  Replace pointnet2_ops.furthest_point_sample (modules/utils/patch.py:102,156)
// and knn_cuda.KNN(k=256) (patch.py:33,107).  Both third-party packages are un-vendored and
// unpinned in the reference (docker/Dockerfile:47-49), so the semantics are defined here and in
// oracle/patch_ref.py:  FPS starts at index 0, squared distances are unfused fp32
// ((dx*dx)+(dy*dy))+(dz*dz), the farthest point is the FIRST maximum (smallest index);
// kNN is ordered by (distance, index) like pf_knn.
#include <cstdlib>
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"
#include "pf_wave.h"

namespace {

__device__ __forceinline__ float sqd(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)          // unfused, whatever -ffp-contract says
    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// ---- FPS: one 1024-thread workgroup per cloud; running min-distance in `mind` (global, L2-resident);
// sequential in npoint by nature: per step = one strided sweep + one workgroup arg-max.
constexpr int FPS_T = 1024;

// one cloud: p [N,3], md [N] scratch, o [npoint] (the dense and the ragged kernel differ only in where these come from).
// CTX (pf_fps_ragged_ctx): cx [nctx,3] are points already taken - with nctx > 0 every min-distance starts as the distance to
// the nearest of them and EVERY sample, the first included, is the arg-max; r2 (nullable) receives the min-distance the last
// sample had when it was taken.  CTX = false compiles to the kernel this was before the context existed.
template <bool CTX = false>
__device__ __forceinline__ void fps_body(const float* __restrict__ p, int N, int npoint, float* __restrict__ md,
                                         int* __restrict__ o, const float* __restrict__ cx = nullptr, int nctx = 0,
                                         float* __restrict__ r2 = nullptr) {
    __shared__ float sv[FPS_T / 64];
    __shared__ int si[FPS_T / 64];
    __shared__ int cur;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool seeded = CTX && nctx > 0;                    // uniform over the workgroup
    if (seeded) {
        for (int k = tid; k < N; k += FPS_T) {
            const float x = p[k * 3 + 0], y = p[k * 3 + 1], z = p[k * 3 + 2];
            float d = 1e10f;
            for (int c = 0; c < nctx; ++c) d = fminf(d, sqd(x, y, z, cx[c * 3 + 0], cx[c * 3 + 1], cx[c * 3 + 2]));
            md[k] = d;
        }
    } else {
        for (int k = tid; k < N; k += FPS_T) md[k] = 1e10f;
    }
    if (tid == 0 && !seeded) { cur = 0; o[0] = 0; }
    float lastd = 1e10f;                                    // thread 0: the min-distance of the sample taken last
    __syncthreads();
    for (int j = seeded ? 0 : 1; j < npoint; ++j) {
        const bool upd = !CTX || !seeded || j > 0;          // the first step after a context only looks for the arg-max
        const int last = upd ? cur : 0;
        const float lx = p[last * 3 + 0], ly = p[last * 3 + 1], lz = p[last * 3 + 2];
        float best = -1.f;
        int besti = 0;
        for (int k = tid; k < N; k += FPS_T) {
            float d = md[k];
            if (upd) {
                d = fminf(d, sqd(p[k * 3 + 0], p[k * 3 + 1], p[k * 3 + 2], lx, ly, lz));
                md[k] = d;
            }
            if (d > best) { best = d; besti = k; }          // increasing k: first maximum kept
        }
        pf_xor_argmax<1, 32>(best, besti);
        if (lane == 0) { sv[wave] = best; si[wave] = besti; }
        __syncthreads();
        if (tid == 0) {
            float bv = sv[0];
            int bi = si[0];
            for (int w = 1; w < FPS_T / 64; ++w)
                if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) { bv = sv[w]; bi = si[w]; }
            cur = bi;
            o[j] = bi;
            if (CTX) lastd = bv;
        }
        __syncthreads();
    }
    if (CTX && r2 && tid == 0) *r2 = lastd;
}

__global__ __launch_bounds__(FPS_T) void fps_kernel(const float* __restrict__ xyz, int N, int npoint,
                                                    float* __restrict__ mind, int* __restrict__ out) {
    const int b = blockIdx.x;
    fps_body(xyz + (size_t)b * N * 3, N, npoint, mind + (size_t)b * N, out + (size_t)b * npoint);
}

// ---- cooperative FPS: G workgroups per cloud, every point and its running min-distance live in REGISTERS ----
// The single-workgroup kernel above re-reads 16 B per point from L2 on every one of the npoint sequential steps
// (99 840 points -> 1.6 MB per step through ONE CU's 64 B/clk texture path: 19 us per step, 388 ms for the CLI's
// 99 840 -> 20 024 merge, 99.7 % of its per-cloud GPU time).  Here a cloud is split over G <= 32 workgroups
// (<= 32 points per thread), a step is: local arg-max in registers -> 64-bit candidates from every WAVE
// (distance bits << 32 | ~index, so an integer max is "farthest, then smallest index") published with an
// agent-scope atomic store into a 4-deep ring of G x 4 slots -> wave 0 of every workgroup polls the slots of the
// step (agent-scope atomic loads) and reduces them.  The 64-bit word IS the whole message (coordinates are re-read
// from the read-only input), so relaxed ordering suffices: no L2 write-back / invalidate per step, which is what an
// acquire / release pair costs at agent scope on this chip.  No read-modify-write atomics, no counters: a slot is
// "filled" when it carries the current step's 2-bit tag (the same slot held step j-4's word before): see the exchange below.
// Progress: blocks are dispatched in index order and a cloud's workgroups are contiguous, so the lowest
// unfinished cloud always has all its workgroups resident; a bounded spin + abort guarantees the grid drains
// even if that assumption were ever violated.  A cloud's status word is 0 only after all of its steps completed -
// pf_fps_scratch_layout tells the caller where that word is, puflow_amd.ops.furthest_point_sample checks it and raises.
#ifndef PF_FPSC_T
#define PF_FPSC_T 256
#endif
constexpr int FPSC_T = PF_FPSC_T;
constexpr int FPSC_GMAX = 32;
constexpr int FPSC_SLOTS = FPSC_GMAX * (FPSC_T / 64);    // one slot per wave of a cloud
static_assert(FPSC_SLOTS <= 128, "a lane of wave 0 polls two words per word a wave publishes");
// status word of a cloud (after its ring): 2 = not finished (set by fps_init_kernel), 1 = aborted, 0 = complete
constexpr unsigned long long FPSC_ST_DONE = 0ull, FPSC_ST_ABORT = PF_RING_ABORT, FPSC_ST_INIT = 2ull;
// wave-wide reductions without LDS traffic (pf_wave_reduce: DPP rotates inside the 16-lane rows, the four row results through SGPRs)
__device__ __forceinline__ int wave_max_i32(int v) { return pf_wave_reduce(v, PfMax{}); }
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) { return pf_wave_reduce(v, PfMax{}); }

// The exchange: every WAVE reduces its own points in registers (DPP) and publishes 64-bit words (distance bits << 32 | tag |
// ~index: an integer max is "farthest, then smallest index") into its slots of a 4-deep ring; wave 0 of every workgroup reads
// the slots of the round (pf_ring_poll), reduces them and hands the result to the other waves through LDS.  The 2-bit tag
// (r / 4) & 3 tells a word of THIS round from the one the same slot held four rounds ago, so a consumer can never take a stale
// candidate whatever order two relaxed stores to different addresses become visible in (no slot clearing, no release /
// acquire); within a round every word carries the same tag, so the integer max is unchanged.  The LDS words are
// double-buffered: wave 0 rewrites a round's half only after the NEXT round's barrier, which every wave reaches after it has
// read the half - ONE workgroup barrier per round.  Measured with one word per wave (the first cooperative kernel, up to
// commit b35a33c) on the CLI's merge (99 840 -> 20 024, 25 workgroups), per step:
//   one word per workgroup, shuffles through LDS, two barriers (round 2's first version)   2.86 us
//   one word per wave, every wave reads all slots itself (no barrier at all)               2.95-3.1 us  (100 readers of the
//                                                                          same lines: the reads get in each other's way)
//   one word per wave, wave 0 reads (the protocol kept)                                    2.2-2.3 us
//   the same with the workgroup's four words merged in LDS first (25 slots)                2.56 us
//   ... waiting for the OWN slots only (wrong results, timing experiment)                  1.65 us  = what the store -> load
//                                                                          round trip through the fabric leaves of a step
// Tried and dropped: all workgroups of a cloud on one XCD (8x oversubscribed grid, HW_REG_XCC_ID, claim counter) - agent-scope
// atomics bypass the XCD's L2 wherever the peers run (2.5 us), workgroup-scope loads are served by the CU's own L1 and never
// see the peers' stores, and an L1 invalidate (buffer_inv sc1) per read costs 6.3 us per step; two staggered reads in flight
// (2.37 us); s_sleep between reads (no change); touching the whole cloud once per XCD before the loop (-0.06 us).

// ---- two samples per exchange (rounds 2 - 4; the kernel is retired, the probe below still measures its exchange) ------------
// A step of the one-word kernel is ~0.4 us of arithmetic and ~1.8 us of waiting for the words to cross the fabric.  Here every wave
// publishes its TWO best points (keys K_a > K_b), so a round knows the global best c1 AND the best of the rest c2.  After c1
// has been added, every min-distance can only shrink, i.e. every key can only fall; points nobody published lie below their
// wave's K_b, which lies below K2 = key(c2).  So if c2 itself is not touched by c1 - d(c2, c1) >= md(c2), computed exactly as
// the update would - and md(c2) > 0, so that c2 also stays above c1's own new key (0, index of c1) - c2 is still the largest
// key after the update: it IS the next sample of the sequential algorithm (keys are distinct, so ties are decided exactly as
// there: farthest, then smallest index), and the round emits both.  Otherwise it
// emits c1 alone, as before.  Every workgroup takes the same decision from the same words.  Bit-identical output; on the CLI's
// merge (99 840 -> 20 024) 1.59 samples per round: 46.0 -> 30.4 ms per cloud.
constexpr int FPSC_SLOTS2 = 2 * FPSC_SLOTS;
constexpr int FPSC_RING2 = 4 * FPSC_SLOTS2;              // status word of the probe's ring

__device__ __forceinline__ unsigned long long fps_key(int vbits, unsigned idx, unsigned tag) {
    return vbits < 0 ? (unsigned long long)tag : (((unsigned long long)(unsigned)vbits << 32) | tag | ((~idx) & 0x1fffffffu));
}
__device__ __forceinline__ unsigned long long u64max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {       // two 32-bit passes: high word, then low
    const unsigned hi = (unsigned)(k >> 32), lo = (unsigned)k;
    const unsigned hmax = wave_max_u32(hi);
    const unsigned lmax = wave_max_u32(hi == hmax ? lo : 0u);
    return ((unsigned long long)hmax << 32) | lmax;
}

// ---- many samples per exchange --------------------------------------------------------------------------------------------
// A round of the two-sample kernel knows more than it uses.  Every wave publishes its KW best points; wave 0 of every workgroup
// holds ALL published candidates (keys and, after one gather, coordinates).  Let B = the largest of the waves' LAST published
// keys: every point nobody published lies below its own wave's last key, hence below B - and adding samples only lowers
// min-distances, i.e. keys.  So wave 0 can run the sequential algorithm on the published candidates alone: take the largest
// key c1 (always the true next sample); lower the candidates' keys by c1 exactly as the update will (min(md, sqd(cand, c1)),
// the same unfused arithmetic, same argument order); the largest updated key K' is the true next sample iff K' >= B (nothing
// unpublished can reach it) and its distance is > 0 (a zero distance would tie with the samples already taken, whose keys are
// (0, index): the sequential algorithm then picks by index among points this round does not know).  Repeat until the test
// fails or MS samples are out.  Unlike the two-sample rule a TOUCHED candidate may still be taken (its lowered key is exact),
// and so may the third, fourth, ... .  Every workgroup runs the same chain on the same words and reaches the same samples.
// CPU simulation of the CLI's merge shape (99 840 -> 20 024, 100 waves): KW = 2, MS = 8: 7.3 samples per round (cap reached
// in 76 % of the rounds); KW = 2, MS = 16: 11.3; KW = 4, MS = 16: 15.5 - against 1.6-1.7 of the two-sample kernel.
#ifndef PF_FPS_KW
#define PF_FPS_KW 4                                      // words (best points) a wave publishes per round: 2 or 4
#endif
#ifndef PF_FPS_MS
#define PF_FPS_MS 64                                     // samples a round may emit
#endif
constexpr int FPSM_KW = PF_FPS_KW, FPSM_MS = PF_FPS_MS;
#ifndef PF_FPS_NC
#define PF_FPS_NC 2                                      // candidates per lane the chain of wave 0 works on
#endif
static_assert(FPSM_KW >= 2 && 4 * FPSM_KW * FPSC_SLOTS + 2 <= 8192 / 2, "the ring must fit the scratch row of the smallest cooperative cloud (8192 points = 4096 words)");
constexpr int FPSM_NC = PF_FPS_NC;
constexpr int FPSC_SLOTSM = FPSM_KW * FPSC_SLOTS;
constexpr int FPSC_RINGM = 4 * FPSC_SLOTSM;              // status word of this kernel's ring
constexpr int FPSM_NT = FPSM_KW * 2;                     // words a lane of wave 0 polls (<= 128 waves per cloud)

template <int V> struct FpsInt { static constexpr int value = V; };
typedef float fps_f2 __attribute__((ext_vector_type(2)));
// two squared distances at once: the same unfused fp32 operations as sqd(), issued as packed v_pk_add / v_pk_mul
__device__ __forceinline__ fps_f2 sqd2(fps_f2 ax, fps_f2 ay, fps_f2 az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    const fps_f2 dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// Workgroup g of the G that share one cloud: p [N,3], ring [4][FPSC_SLOTSM], abort_w = the cloud's status word (+ 1: rounds),
// o [npoint].  fps_coopm_kernel (dense batch) and fps_coopm_ragged_kernel (clouds of different sizes) differ only in where
// these come from.
// CTX (pf_fps_ragged_ctx): cx [nctx,3] are points already taken.  With nctx > 0 a prologue lowers every min-distance to the
// distance to the nearest of them (64 context points at a time, culled by the round update's exact bounding-box test against
// the wave's current largest min-distance), and the rounds start with NOTHING emitted: round 0 only publishes, its chain takes
// sample 0.  Nothing else of a round changes - the chain's first sample is the arg-max whatever lowered the min-distances
// before, and a candidate a context point coincides with has distance 0 like one a sample coincides with.  r2 (nullable): the
// min-distance of the last sample when it was taken (the distance bits of its key).  A cloud with nctx = 0 runs the code of
// CTX = false, which in turn compiles to the kernel this was before the context existed.
template <int PPT, bool CTX = false>
__device__ __forceinline__ void fps_coopm_body(const float* __restrict__ p, int N, int npoint, int G, int g,
                                               unsigned long long* __restrict__ ring, unsigned long long* __restrict__ abort_w,
                                               int* __restrict__ o, const float* __restrict__ cx = nullptr, int nctx = 0,
                                               float* __restrict__ r2 = nullptr) {
    constexpr int NW = FPSC_T / 64, KW = FPSM_KW, MS = FPSM_MS, NT = FPSM_NT, PH = (PPT + 1) / 2, NC = FPSM_NC, CAP = 64 * NC;
    __shared__ unsigned long long s_ck[CAP];                            // wave 0: the round's compacted candidates
    __shared__ float s_l[2][3 * MS + 4];                                // samples of a round, [3 MS] = count, [3 MS + 1] = alive
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int SW = KW * G * NW;                                         // words per round

    // a thread holds PPT CONSECUTIVE points, a wave 64 PPT consecutive points: indices grow with k (first maximum = smallest
    // index), and when the input has any spatial order (the CLI's merge: 1024 consecutive candidates = one patch) a wave's
    // points share a small bounding box - see the culling test below
    const int base = ((g * NW + wave) * 64 + lane) * PPT;
    fps_f2 px[PH], py[PH], pz[PH], md[PH];                              // points 2h, 2h + 1 of this thread
    float lox = 3e38f, loy = 3e38f, loz = 3e38f, hix = -3e38f, hiy = -3e38f, hiz = -3e38f;
#pragma unroll
    for (int k = 0; k < 2 * PH; ++k) {
        const int i = base + k;
        const bool in = k < PPT && i < N;
        const int ic = in ? i : N - 1;
        const float x = p[ic * 3 + 0], y = p[ic * 3 + 1], z = p[ic * 3 + 2];
        px[k >> 1][k & 1] = x; py[k >> 1][k & 1] = y; pz[k >> 1][k & 1] = z;
        md[k >> 1][k & 1] = in ? 1e10f : -1.f;                          // padding can never be the farthest point
        if (in) { lox = fminf(lox, x); loy = fminf(loy, y); loz = fminf(loz, z); hix = fmaxf(hix, x); hiy = fmaxf(hiy, y); hiz = fmaxf(hiz, z); }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {                            // the wave's bounding box (once)
        lox = fminf(lox, __shfl_xor(lox, off)); loy = fminf(loy, __shfl_xor(loy, off)); loz = fminf(loz, __shfl_xor(loz, off));
        hix = fmaxf(hix, __shfl_xor(hix, off)); hiy = fmaxf(hiy, __shfl_xor(hiy, off)); hiz = fmaxf(hiz, __shfl_xor(hiz, off));
    }
    const bool seeded = CTX && nctx > 0;                                // uniform over the cloud's workgroups
    if (tid == 0) {
        if (!seeded) {
            if (g == 0) o[0] = 0;
            s_l[1][0] = p[0]; s_l[1][1] = p[1]; s_l[1][2] = p[2];       // "round -1" emitted point 0
            s_l[1][3 * MS] = 1.f; s_l[1][3 * MS + 1] = 1.f;
            if (CTX && r2 && g == 0) *r2 = 1e10f;                       // point 0's min-distance (stands when npoint = 1)
        } else {
            s_l[1][3 * MS] = 0.f; s_l[1][3 * MS + 1] = 1.f;             // "round -1" emitted nothing
        }
    }
    __syncthreads();
    float Dw = 1e10f;                                                   // >= every min-distance of this wave (its last published best)
    if (CTX && seeded) {
        // lane s looks at context point c0 + s; the skip is the round update's: sqd(nearest point of the box, c) >= Dw >= md
        for (int c0 = 0; c0 < nctx; c0 += 64) {
            const int ci = c0 + lane < nctx ? c0 + lane : nctx - 1;
            const float ccx = cx[ci * 3 + 0], ccy = cx[ci * 3 + 1], ccz = cx[ci * 3 + 2];
            const float bd = sqd(fminf(fmaxf(ccx, lox), hix), fminf(fmaxf(ccy, loy), hiy), fminf(fmaxf(ccz, loz), hiz), ccx, ccy, ccz);
            unsigned long long need = __ballot(c0 + lane < nctx && bd < Dw);
            if (need == 0ull) continue;                                 // uniform over the wave
            while (need) {
                const int s = __builtin_ctzll(need);
                need &= need - 1ull;
                auto rl = [](float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); };
                const float lx = rl(ccx, s), ly = rl(ccy, s), lz = rl(ccz, s);
#pragma unroll
                for (int h = 0; h < PH; ++h) {
                    const fps_f2 d = sqd2(px[h], py[h], pz[h], lx, ly, lz);
                    md[h][0] = fminf(md[h][0], d[0]); md[h][1] = fminf(md[h][1], d[1]);
                }
            }
            float mx = -1.f;                                            // the wave's largest min-distance bounds the next 64
#pragma unroll
            for (int h = 0; h < PH; ++h) mx = fmaxf(mx, fmaxf(md[h][0], md[h][1]));
            Dw = __int_as_float(wave_max_i32(__float_as_int(mx)));
        }
    }
    int pv[KW];                                                         // the wave's last published keys (distance bits, index)
    unsigned pidx[KW];
#pragma unroll
    for (int e = 0; e < KW; ++e) { pv[e] = -1; pidx[e] = 0u; }
    int j = seeded ? 0 : 1, rounds = 0;
    for (int r = 0; j < npoint; ++r) {
        // update with the samples of the previous round - those that can reach this wave.  Lane s looks at sample s: the
        // nearest point q of the wave's box to it is at least as close as every point of the wave, in fp32 as computed by
        // sqd() too (subtraction, multiplication and addition round monotonically), so sqd(q, c) >= Dw >= md means
        // fminf(md, sqd(p, c)) = md for the whole wave: the sample is skipped EXACTLY.  Late in a merge a sample reaches a
        // few per cent of the waves; a wave no sample reached publishes its previous keys again.
        bool touched = false;
        {
            const float* sp = s_l[(r + 1) & 1];
            const int m = (int)sp[3 * MS];
            const int ls = lane < MS ? lane : MS - 1;
            const float cx = sp[3 * ls], cy = sp[3 * ls + 1], cz = sp[3 * ls + 2];
            const float bd = sqd(fminf(fmaxf(cx, lox), hix), fminf(fmaxf(cy, loy), hiy), fminf(fmaxf(cz, loz), hiz), cx, cy, cz);
            unsigned long long need = __ballot(lane < m && bd < Dw);
            touched = need != 0ull || (CTX && seeded && r == 0);       // after the context prologue no key is published yet
            while (need) {
                const int s = __builtin_ctzll(need);
                need &= need - 1ull;
                auto rl = [](float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); };
                const float lx = rl(cx, s), ly = rl(cy, s), lz = rl(cz, s);
#pragma unroll
                for (int h = 0; h < PH; ++h) {
                    const fps_f2 d = sqd2(px[h], py[h], pz[h], lx, ly, lz);
                    md[h][0] = fminf(md[h][0], d[0]); md[h][1] = fminf(md[h][1], d[1]);
                }
            }
        }
        unsigned long long* slot = ring + (r & 3) * FPSC_SLOTSM;
        const unsigned tag = ((unsigned)(((r >> 2) & 3) << 1) | 1u) << 29;      // see the exchange above
        if (touched) {                                                  // uniform over the wave
            // per-lane best KW by (distance, then smaller index): indices grow with k, strict comparisons keep the smaller
            float bv[KW];
            int bk[KW];
#pragma unroll
            for (int q = 0; q < KW; ++q) { bv[q] = -1.f; bk[q] = 0; }
#pragma unroll
            for (int k = 0; k < 2 * PH; ++k) {
                const float d = md[k >> 1][k & 1];
                bool gt[KW];
#pragma unroll
                for (int q = 0; q < KW; ++q) gt[q] = d > bv[q];
#pragma unroll
                for (int q = KW - 1; q >= 0; --q) {
                    const bool up = q > 0 && gt[q > 0 ? q - 1 : 0];     // the element above moves down into q
                    bv[q] = gt[q] ? (up ? bv[q > 0 ? q - 1 : 0] : d) : bv[q];
                    bk[q] = gt[q] ? (up ? bk[q > 0 ? q - 1 : 0] : k) : bk[q];
                }
            }
            // the wave's best KW (distances are >= 0 or the -1 of padding: their bit patterns order like signed integers)
#pragma unroll
            for (int e = 0; e < KW; ++e) {
                const int vb = __float_as_int(bv[0]);
                const unsigned ib = (unsigned)(base + bk[0]);
                const int vmax = wave_max_i32(vb);
                const unsigned imin = ~wave_max_u32(vb == vmax ? ~ib : 0u);
                const bool mine = vb == vmax && ib == imin;             // the lane that holds this one pops it
                pv[e] = vmax; pidx[e] = imin;
#pragma unroll
                for (int q = 0; q + 1 < KW; ++q) { bv[q] = mine ? bv[q + 1] : bv[q]; bk[q] = mine ? bk[q + 1] : bk[q]; }
                bv[KW - 1] = mine ? -1.f : bv[KW - 1];
            }
            Dw = __int_as_float(pv[0]);
        }
        if (lane == 0) {
#pragma unroll
            for (int e = 0; e < KW; ++e) PF_ST(slot + KW * (g * NW + wave) + e, fps_key(pv[e], pidx[e], tag));
        }
        if (wave == 0) {
            unsigned long long kk[NT];
            const bool dead = !pf_ring_poll<NT>(slot, SW, tag, abort_w, kk);
            float* sl = s_l[r & 1];
            if (dead) {                                                     // uniform over the wave
                if (lane == 0) { PF_ST(abort_w, FPSC_ST_ABORT); sl[3 * MS + 1] = -1.f; }
            } else {
                // B: the largest LAST key of a wave (word w = KW * wave + e is a last key iff w mod KW == KW - 1)
                unsigned long long lastk = 0ull, f0 = 0ull;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    f0 = u64max(f0, kk[t]);
                    if ((lane + 64 * t) % KW == KW - 1) lastk = u64max(lastk, kk[t]);
                }
                const unsigned long long Bk = wave_max_u64(lastk);
                const unsigned long long K1 = wave_max_u64(f0);            // the round's first sample: the largest key of all
                // Only candidates with a key >= B (and a distance > 0) can follow it in this round - keys only fall: compact
                // them, NC per lane, through LDS (this wave only; the LDS operations of a wave execute in order) and chain on
                // those alone.  On the CLI's merge 12 (KW = 2), 34 (3) or 65 (4) candidates qualify on average, 144 at most; a
                // round with more than 64 NC emits its first sample only (still exact; KW = 4: 0.7 % of the rounds).
                unsigned long long rm[NT];
                int cnt = 0;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    rm[t] = __ballot(kk[t] == K1 || (kk[t] >= Bk && (unsigned)(kk[t] >> 32) != 0u));
                    cnt += __builtin_popcountll(rm[t]);
                }
                if (cnt > CAP) {                                            // uniform
                    cnt = 1;
#pragma unroll
                    for (int t = 0; t < NT; ++t) rm[t] = __ballot(kk[t] == K1);
                }
                {
                    int before = 0;
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const int pos = before + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(rm[t] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)rm[t], 0u));
                        if ((rm[t] >> lane) & 1ull) s_ck[pos] = kk[t];
                        before += __builtin_popcountll(rm[t]);
                    }
                }
                __builtin_amdgcn_wave_barrier();
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                // the chain on NCC candidates per lane: one when the round's candidates fit the wave (the usual case on the
                // pipeline's clouds: ~20 qualify), NC otherwise
                int m = 0;
                int kx = 0, ky = 0, kz = 0, ki = 0;
                unsigned kd = 0u;                                           // CTX: lane m keeps sample m's min-distance bits
                auto chain = [&](auto ncc_) {
                    constexpr int NCC = decltype(ncc_)::value;
                    unsigned long long ck[NCC];
                    float cx[NCC], cy[NCC], cz[NCC];
#pragma unroll
                    for (int c = 0; c < NCC; ++c) {
                        ck[c] = lane + 64 * c < cnt ? s_ck[lane + 64 * c] : 0ull;
                        const unsigned q = (~(unsigned)ck[c]) & 0x1fffffffu;
                        const unsigned qc = q < (unsigned)N ? q : 0u;           // the cloud is read-only: plain cached loads
                        cx[c] = p[qc * 3 + 0]; cy[c] = p[qc * 3 + 1]; cz[c] = p[qc * 3 + 2];
                    }
                    __builtin_amdgcn_wave_barrier();                            // s_ck is written again next round, after these reads
                    for (;;) {
                        // this lane's best, then the wave's
                        unsigned long long f = ck[0];
                        float fx = cx[0], fy = cy[0], fz = cz[0];
#pragma unroll
                        for (int c = 1; c < NCC; ++c) {
                            const bool gt = ck[c] > f;
                            f = gt ? ck[c] : f;
                            fx = gt ? cx[c] : fx; fy = gt ? cy[c] : fy; fz = gt ? cz[c] : fz;
                        }
                        const unsigned fh = (unsigned)(f >> 32), fl = (unsigned)f;
                        const unsigned hmax = wave_max_u32(fh);
                        unsigned long long own = __ballot(fh == hmax);
                        unsigned lmax;
                        if (__builtin_popcountll(own) == 1) {                  // the usual case: one lane holds the largest distance
                            lmax = (unsigned)__builtin_amdgcn_readlane((int)fl, __builtin_ctzll(own));
                        } else {
                            lmax = wave_max_u32(fh == hmax ? fl : 0u);
                            own = __ballot(fh == hmax && fl == lmax);
                        }
                        const unsigned long long K = ((unsigned long long)hmax << 32) | lmax;
                        if (m > 0 && !(K >= Bk && __uint_as_float(hmax) > 0.f)) break;
                        const int w = __builtin_ctzll(own);
                        auto rl = [](float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); };
                        const float sx = rl(fx, w), sy = rl(fy, w), sz = rl(fz, w);
                        const unsigned idx = (~lmax) & 0x1fffffffu;
                        // lane m keeps sample m (a select on the wave-uniform values): ONE LDS write and one index store per
                        // lane after the chain instead of an exec-masked write + store per sample
                        {
                            const bool me = lane == m;
                            kx = me ? __float_as_int(sx) : kx; ky = me ? __float_as_int(sy) : ky;
                            kz = me ? __float_as_int(sz) : kz; ki = me ? (int)idx : ki;
                            if (CTX) kd = me ? hmax : kd;
                        }
                        ++m;
                        if (m == MS || j + m >= npoint || idx >= (unsigned)N) break;
                        // lower the candidates' keys exactly as the update will (the sample itself falls to distance 0)
#pragma unroll
                        for (int c = 0; c < NCC; ++c) {
                            const float d = sqd(cx[c], cy[c], cz[c], sx, sy, sz);
                            const unsigned kh = (unsigned)(ck[c] >> 32);
                            if (d < __uint_as_float(kh)) ck[c] = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)ck[c];
                        }
                    }
                };
                if (cnt <= 64) chain(FpsInt<1>{}); else chain(FpsInt<NC>{});
                if (lane < m) {
                    sl[3 * lane] = __int_as_float(kx); sl[3 * lane + 1] = __int_as_float(ky); sl[3 * lane + 2] = __int_as_float(kz);
                    if (g == 0) o[j + lane] = ki;
                    if (CTX && r2 && g == 0 && lane == m - 1 && j + m >= npoint) *r2 = __uint_as_float(kd);
                }
                if (lane == 0) { sl[3 * MS] = (float)m; sl[3 * MS + 1] = 1.f; }
            }
        }
        // s_l is double-buffered (see the exchange above): one barrier per round
        __syncthreads();
        const float* sl = s_l[r & 1];
        if (sl[3 * MS + 1] < 0.f) return;                                 // uniform over the workgroup: aborted
        j += (int)sl[3 * MS];
        rounds = r + 1;
    }
    // the word after the status word: exchange rounds this cloud took (measurement only: bench.py --mode pugan reports
    // samples per round and the time per round next to the exchange floor of pf_fps_exchange_probe)
    if (g == 0 && tid == 0) { PF_ST(abort_w + 1, (unsigned long long)rounds); PF_ST(abort_w, FPSC_ST_DONE); }
}

template <int PPT>
__global__ __launch_bounds__(FPSC_T, (PPT <= 16 ? 4 : (PPT <= 24 ? 3 : 2))) void fps_coopm_kernel(const float* __restrict__ xyz, int N,
                                                                                 int npoint, int G,
                                                                                 unsigned long long* __restrict__ ringbuf,
                                                                                 long long ring_stride, int* __restrict__ out) {
    const int b = blockIdx.x / G, g = blockIdx.x % G;
    unsigned long long* ring = ringbuf + (size_t)b * ring_stride;       // [4][FPSC_SLOTSM] + status word
    fps_coopm_body<PPT>(xyz + (size_t)b * N * 3, N, npoint, G, g, ring, ring + FPSC_RINGM, out + (size_t)b * npoint);
}

// ---- ragged batches: clouds of different sizes stored back to back --------------------------------------------------------
// The per-cloud tables travel as kernel arguments (at most PF_RAGGED_MAXB clouds per launch; the entry points split longer
// lists): no device-side table to build, upload or keep alive, and the host validates every offset it hands out.
// Cooperative FPS with unequal G_i keeps the progress argument of the dense launch: workgroup ids are cloud-major and
// ascending (wg0 is a prefix sum), workgroups are dispatched in id order, so when a workgroup of cloud c is resident every
// workgroup of the clouds before c has been dispatched; the lowest unfinished cloud either has all of its G_c <= 32
// workgroups resident or is the only cloud still holding CUs, and one cloud always fits the chip.
constexpr int PF_RAGGED_MAXB = 64;
struct FpsRaggedTab {
    int off[PF_RAGGED_MAXB];          // first point of the cloud in xyz
    int n[PF_RAGGED_MAXB];            // its points
    int npoint[PF_RAGGED_MAXB];       // its samples
    int ooff[PF_RAGGED_MAXB];         // first sample in idx_out
    int cloud[PF_RAGGED_MAXB];        // its number in the batch (status word)
    int wg0[PF_RAGGED_MAXB + 1];      // cooperative launch: first workgroup of the cloud (prefix sum of G_i)
    long long soff[PF_RAGGED_MAXB];   // its scratch row, in floats (even: the ring is read as 64-bit words)
};

template <int PPT>
__global__ __launch_bounds__(FPSC_T, (PPT <= 16 ? 4 : (PPT <= 24 ? 3 : 2))) void fps_coopm_ragged_kernel(
    const float* __restrict__ xyz, const FpsRaggedTab t, int nc, float* __restrict__ scratch, unsigned long long* __restrict__ status,
    int* __restrict__ out) {
    int c = 0;
    while (c + 1 < nc && (int)blockIdx.x >= t.wg0[c + 1]) ++c;         // uniform: nc <= 64 table entries
    const int g = (int)blockIdx.x - t.wg0[c], G = t.wg0[c + 1] - t.wg0[c];
    unsigned long long* ring = reinterpret_cast<unsigned long long*>(scratch + t.soff[c]);
    fps_coopm_body<PPT>(xyz + (size_t)t.off[c] * 3, t.n[c], t.npoint[c], G, g, ring, status + 2 * t.cloud[c], out + t.ooff[c]);
}

// clouds below the cooperative threshold: fps_kernel's workgroup per cloud; the status word only says "ran to the end"
__global__ __launch_bounds__(FPS_T) void fps_ragged_kernel(const float* __restrict__ xyz, const FpsRaggedTab t,
                                                           float* __restrict__ scratch, unsigned long long* __restrict__ status,
                                                           int* __restrict__ out) {
    const int c = blockIdx.x;
    fps_body(xyz + (size_t)t.off[c] * 3, t.n[c], t.npoint[c], scratch + t.soff[c], out + t.ooff[c]);
    if (threadIdx.x == 0) PF_ST(status + 2 * t.cloud[c], FPSC_ST_DONE);
}

// ---- the same two launches with a fixed context per cloud (pf_fps_ragged_ctx) ---------------------------------------------
// Instantiations of their own: the context costs the kernels above neither an argument nor a register.  Both per-cloud
// tables of the context travel as kernel arguments next to FpsRaggedTab (2.6 KB of the 4 KB an argument block may have).
struct FpsCtxTab {
    int coff[PF_RAGGED_MAXB];         // first context point of the cloud in ctx
    int nctx[PF_RAGGED_MAXB];         // its context points (0: the cloud is sampled as by pf_fps_ragged)
};
static_assert(sizeof(FpsRaggedTab) + sizeof(FpsCtxTab) + 64 <= 4096, "the kernel argument block");

template <int PPT>
__global__ __launch_bounds__(FPSC_T, (PPT <= 16 ? 4 : (PPT <= 24 ? 3 : 2))) void fps_coopm_ragged_ctx_kernel(
    const float* __restrict__ xyz, const FpsRaggedTab t, const FpsCtxTab ct, int nc, const float* __restrict__ ctx,
    float* __restrict__ scratch, unsigned long long* __restrict__ status, int* __restrict__ out, float* __restrict__ r2_out) {
    int c = 0;
    while (c + 1 < nc && (int)blockIdx.x >= t.wg0[c + 1]) ++c;         // uniform: nc <= 64 table entries
    const int g = (int)blockIdx.x - t.wg0[c], G = t.wg0[c + 1] - t.wg0[c];
    unsigned long long* ring = reinterpret_cast<unsigned long long*>(scratch + t.soff[c]);
    fps_coopm_body<PPT, true>(xyz + (size_t)t.off[c] * 3, t.n[c], t.npoint[c], G, g, ring, status + 2 * t.cloud[c], out + t.ooff[c],
                              ctx + (size_t)ct.coff[c] * 3, ct.nctx[c], r2_out ? r2_out + t.cloud[c] : nullptr);
}

__global__ __launch_bounds__(FPS_T) void fps_ragged_ctx_kernel(const float* __restrict__ xyz, const FpsRaggedTab t,
                                                               const FpsCtxTab ct, const float* __restrict__ ctx,
                                                               float* __restrict__ scratch, unsigned long long* __restrict__ status,
                                                               int* __restrict__ out, float* __restrict__ r2_out) {
    const int c = blockIdx.x;
    fps_body<true>(xyz + (size_t)t.off[c] * 3, t.n[c], t.npoint[c], scratch + t.soff[c], out + t.ooff[c],
                   ctx + (size_t)ct.coff[c] * 3, ct.nctx[c], r2_out ? r2_out + t.cloud[c] : nullptr);
    if (threadIdx.x == 0) PF_ST(status + 2 * t.cloud[c], FPSC_ST_DONE);
}

// ---- the exchange alone: what a round of the two-sample kernel costs with NO points to update ------------------------------
// Same protocol, same ring, same shapes (G workgroups of FPSC_T threads, two words per wave, wave 0 polls 4 words per lane,
// reduces them and hands a result to the other waves through the double-buffered LDS words, one barrier per round) - only the
// per-point min-distance update and the candidate's coordinate fetch are missing.  Timed with HIP events it is the floor of a
// round: the store -> load round trip through the fabric plus waiting for the slowest of the G peers.
__global__ __launch_bounds__(FPSC_T) void fps_exchange_probe_kernel(int G, int rounds, unsigned long long* __restrict__ ring) {
    constexpr int NW = FPSC_T / 64;
    __shared__ float s_l[2][2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = blockIdx.x;
    unsigned long long* abort_w = ring + FPSC_RING2;
    const int S2 = 2 * G * NW;
    unsigned acc = (unsigned)(g * NW + wave) + 1u;
    for (int r = 0; r < rounds; ++r) {
        unsigned long long* slot = ring + (r & 3) * FPSC_SLOTS2;
        const unsigned tag = ((unsigned)(((r >> 2) & 3) << 1) | 1u) << 29;
        if (lane == 0) {
            PF_ST(slot + 2 * (g * NW + wave), ((unsigned long long)acc << 32) | tag | 1u);
            PF_ST(slot + 2 * (g * NW + wave) + 1, ((unsigned long long)(acc >> 1) << 32) | tag);
        }
        if (wave == 0) {
            unsigned long long k[4];
            const bool dead = !pf_ring_poll<4>(slot, S2, tag, abort_w, k);
            if (dead) {
                if (lane == 0) { PF_ST(abort_w, FPSC_ST_ABORT); s_l[r & 1][1] = -1.f; }
            } else {
                const unsigned long long K1 = wave_max_u64(u64max(u64max(k[0], k[1]), u64max(k[2], k[3])));
                if (lane == 0) { s_l[r & 1][0] = __uint_as_float((unsigned)(K1 >> 32) & 0xffffu); s_l[r & 1][1] = 1.f; }
            }
        }
        __syncthreads();
        if (s_l[r & 1][1] < 0.f) return;
        acc = acc * 1664525u + (unsigned)__float_as_uint(s_l[r & 1][0]) + 1013904223u;      // the next word depends on this round's result
        acc &= 0x7fffffffu;
    }
    if (g == 0 && tid == 0) PF_ST(abort_w, FPSC_ST_DONE);
}

// ---- large-K kNN: one workgroup per query; keys (dist bits << 32 | index) bitonic-sorted in LDS.
// N <= 16384: all N keys in one sort.  Larger clouds (knn_cuda.KNN takes any N, patch.py:33,107): the references are
// streamed in chunks; LDS holds the running best KP >= K keys in front of the chunk's keys, every pass sorts the
// NP = 16384 keys and keeps the front.  Keys are distinct (the index is part of the key), so the result is the exact
// (distance, index)-ordered top K whatever the chunking.
constexpr int KS_T = 1024;
constexpr int KS_NMAX = 16384;          // 128 KiB of 64-bit keys
constexpr int KS_KMAX = 8192;           // chunked path: at least half of the LDS keys are fresh references per pass

// one query qq [3] against its cloud r [N,3]; irow / drow: the query's K outputs
__device__ __forceinline__ void knn_sort_body(unsigned long long* keys, const float* __restrict__ r, const float* __restrict__ qq,
                                              int N, int K, int NP /*pow2: keys sorted per pass*/,
                                              int KP /*0: single pass; else pow2 >= K kept between passes*/,
                                              int* __restrict__ irow, float* __restrict__ drow) {
    const int tid = threadIdx.x;
    const float qx = qq[0], qy = qq[1], qz = qq[2];
    const int C = NP - KP;                                              // fresh references per pass
    for (int i = tid; i < KP; i += KS_T) keys[i] = ~0ull;
    for (int c0 = 0; c0 < N; c0 += C) {
        for (int i = tid; i < C; i += KS_T) {
            const int j = c0 + i;
            unsigned long long key = ~0ull;
            if (j < N) key = ((unsigned long long)__float_as_uint(sqd(qx, qy, qz, r[j * 3 + 0], r[j * 3 + 1], r[j * 3 + 2])) << 32) | (unsigned)j;
            keys[KP + i] = key;
        }
        __syncthreads();
        for (int k = 2; k <= NP; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < NP; i += KS_T) {
                    const int l = i ^ j;
                    if (l > i) {
                        const unsigned long long a = keys[i], c = keys[l];
                        const bool up = (i & k) == 0;
                        if ((a > c) == up) { keys[i] = c; keys[l] = a; }
                    }
                }
                __syncthreads();
            }
    }
    for (int i = tid; i < K; i += KS_T) {
        const unsigned long long key = keys[i];
        irow[i] = (int)(key & 0xffffffffu);
        if (drow) drow[i] = __uint_as_float((unsigned)(key >> 32));
    }
}

__global__ __launch_bounds__(KS_T) void knn_sort_kernel(const float* __restrict__ ref, const float* __restrict__ query,
                                                       int N, int M, int K, int NP, int KP,
                                                       int* __restrict__ idx_out, float* __restrict__ dist_out) {
    extern __shared__ unsigned long long keys[];
    const int b = blockIdx.y, q = blockIdx.x;
    const size_t row = ((size_t)b * M + q) * K;
    knn_sort_body(keys, ref + (size_t)b * N * 3, query + ((size_t)b * M + q) * 3, N, K, NP, KP, idx_out + row,
                  dist_out ? dist_out + row : nullptr);
}

// sort shape of a cloud of N references (the host's choice in pf_knn_large, per cloud here)
__host__ __device__ __forceinline__ void knn_sort_shape(int N, int K, int* np, int* kp) {
    int a = 1, k = 0;
    if (N <= KS_NMAX) {
        while (a < N) a <<= 1;
    } else {
        a = KS_NMAX;
        k = 1;
        while (k < K) k <<= 1;
    }
    *np = a; *kp = k;
}

struct KnnRaggedTab {
    int roff[PF_RAGGED_MAXB];         // first reference of the cloud
    int n[PF_RAGGED_MAXB];            // its references
    int q0[PF_RAGGED_MAXB + 1];       // its first query (queries of all clouds are stored back to back, as the outputs)
};
// one workgroup per query of the launch; every query looks up its own cloud
__global__ __launch_bounds__(KS_T) void knn_sort_ragged_kernel(const float* __restrict__ ref, const float* __restrict__ query,
                                                              const KnnRaggedTab t, int nc, int K, int* __restrict__ idx_out,
                                                              float* __restrict__ dist_out) {
    extern __shared__ unsigned long long keys[];
    const int q = t.q0[0] + (int)blockIdx.x;
    int c = 0;
    while (c + 1 < nc && q >= t.q0[c + 1]) ++c;                         // uniform
    int np, kp;
    knn_sort_shape(t.n[c], K, &np, &kp);
    const size_t row = (size_t)q * K;
    knn_sort_body(keys, ref + (size_t)t.roff[c] * 3, query + (size_t)q * 3, t.n[c], K, np, kp, idx_out + row,
                  dist_out ? dist_out + row : nullptr);
}

// ---- normalize_pc (modules/utils/patch.py:168-178): centroid = mean over the points, pc - centroid, divided by the largest
// norm.  One workgroup per cloud / patch with a FIXED summation order (thread t adds points t, t + 256, ... in order, then a
// binary tree over the 256 partial sums), so a cloud's result does not depend on how many clouds share the launch - torch's
// mean picks its reduction tree from the whole tensor shape.  All arithmetic unfused fp32, IEEE sqrt and division.
constexpr int NRM_T = 256;
// one cloud: p [N,3] -> o [N,3], cen [3], fdp [1]
__device__ __forceinline__ void normalize_pc_body(const float* p, int N, float* o, float* __restrict__ cen, float* __restrict__ fdp) {
#pragma clang fp contract(off)
    __shared__ float red[3][NRM_T];
    const int tid = threadIdx.x;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int i = tid; i < N; i += NRM_T) {
        sx = __fadd_rn(sx, p[i * 3 + 0]); sy = __fadd_rn(sy, p[i * 3 + 1]); sz = __fadd_rn(sz, p[i * 3 + 2]);
    }
    red[0][tid] = sx; red[1][tid] = sy; red[2][tid] = sz;
    __syncthreads();
    for (int s = NRM_T / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] = __fadd_rn(red[0][tid], red[0][tid + s]);
            red[1][tid] = __fadd_rn(red[1][tid], red[1][tid + s]);
            red[2][tid] = __fadd_rn(red[2][tid], red[2][tid + s]);
        }
        __syncthreads();
    }
    const float cx = __fdiv_rn(red[0][0], (float)N), cy = __fdiv_rn(red[1][0], (float)N), cz = __fdiv_rn(red[2][0], (float)N);
    __syncthreads();
    float m = 0.f;
    for (int i = tid; i < N; i += NRM_T) {
        const float dx = __fsub_rn(p[i * 3 + 0], cx), dy = __fsub_rn(p[i * 3 + 1], cy), dz = __fsub_rn(p[i * 3 + 2], cz);
        m = fmaxf(m, __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz))));
    }
    red[0][tid] = m;
    __syncthreads();
    for (int s = NRM_T / 2; s > 0; s >>= 1) {
        if (tid < s) red[0][tid] = fmaxf(red[0][tid], red[0][tid + s]);
        __syncthreads();
    }
    const float fd = red[0][0];
    for (int i = tid; i < N; i += NRM_T) {
        o[i * 3 + 0] = __fdiv_rn(__fsub_rn(p[i * 3 + 0], cx), fd);
        o[i * 3 + 1] = __fdiv_rn(__fsub_rn(p[i * 3 + 1], cy), fd);
        o[i * 3 + 2] = __fdiv_rn(__fsub_rn(p[i * 3 + 2], cz), fd);
    }
    if (tid == 0) {
        cen[0] = cx; cen[1] = cy; cen[2] = cz;
        fdp[0] = fd;
    }
}

__global__ __launch_bounds__(NRM_T) void normalize_pc_kernel(const float* __restrict__ x, int N, float* __restrict__ out,
                                                             float* __restrict__ centroid, float* __restrict__ fdist) {
    const int b = blockIdx.x;
    normalize_pc_body(x + (size_t)b * N * 3, N, out + (size_t)b * N * 3, centroid + b * 3, fdist + b);
}

struct NrmRaggedTab { int off[PF_RAGGED_MAXB + 1]; };                   // cloud c = points [off[c], off[c + 1])
// the same workgroup per cloud, the same summation order for the cloud's own N: a cloud's result depends on nothing else
__global__ __launch_bounds__(NRM_T) void normalize_pc_ragged_kernel(const float* __restrict__ x, const NrmRaggedTab t,
                                                                    float* __restrict__ out, float* __restrict__ centroid,
                                                                    float* __restrict__ fdist) {
    const int c = blockIdx.x;
    normalize_pc_body(x + (size_t)t.off[c] * 3, t.off[c + 1] - t.off[c], out + (size_t)t.off[c] * 3, centroid + c * 3, fdist + c);
}

}  // namespace

namespace {
// clears the scratch rows and sets every cloud's status word to "not finished"
__global__ __launch_bounds__(256) void fps_init_kernel(float* p, long long n, int B, long long stride_words, int status_word) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float v = 0.f;
        const long long w = i >> 1;                                       // 64-bit word index
        if ((i & 1) == 0 && stride_words > 0 && w % stride_words == status_word && w / stride_words < B)
            v = __uint_as_float((unsigned)FPSC_ST_INIT);                  // low half of the status word
        p[i] = v;
    }
}
}  // namespace

// 1 when pf_fps runs the cooperative kernel (fps_coopm_kernel) for clouds of N points (its scratch row then holds the candidate
// ring): stride_words = 64-bit words between the rings of consecutive clouds, abort_word = index of the status word in a ring
extern "C" int pf_fps_scratch_layout(int N, long long* stride_words, long long* abort_word) {
    if (stride_words) *stride_words = ((long long)N / 2) & ~1ll;
    if (abort_word) *abort_word = FPSC_RINGM;
    return N >= 8192 && N <= FPSC_GMAX * 1024 * 8 ? 1 : 0;
}

// xyz [B,N,3] -> idx [B,npoint] int32; mind: [B,N] float scratch
// points per thread of the cooperative kernel.  `group` > 0: the caller says that every `group` consecutive points are one
// spatial neighbourhood (the CLI's merge: 1280 candidates per patch); when a wave can hold exactly one group (64 x 12 / 20 / 24
// points) its bounding box is that neighbourhood's, which is what the culling of fps_coopm_kernel lives on.
static int fps_ppt(int N, int group) {
    if (group > 0 && group % 64 == 0) {
        const int p = group / 64;
        if ((p == 12 || p == 20 || p == 24) && (N + FPSC_T * p - 1) / (FPSC_T * p) <= FPSC_GMAX && N >= FPSC_T * p * 2) return p;
    }
    int ppt = N >= 16 * FPSC_T ? 4 : 1;                                               // fewer, fuller workgroups
    while ((N + FPSC_T * ppt - 1) / (FPSC_T * ppt) > FPSC_GMAX) ppt *= 2;              // -> 1, 4, 8 (16, 32) points per thread
    return ppt;
}

extern "C" int pf_fps(const float* xyz, int B, int N, int npoint, float* mind, int* idx_out, void* stream) {
    return pf_fps_grouped(xyz, B, N, npoint, 0, mind, idx_out, stream);
}

extern "C" int pf_fps_grouped(const float* xyz, int B, int N, int npoint, int group, float* mind, int* idx_out, void* stream) {
    if (!xyz || !mind || !idx_out) return PF_ERR_NULL;
    if (B <= 0 || N <= 0 || npoint <= 0 || npoint > N || group < 0) return PF_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    // cooperative kernel when the cloud is worth more than one CU; the candidate ring (4 x 32 + 1 64-bit words)
    // lives at the start of each cloud's N-float scratch row
    if (N >= 8192 && N <= FPSC_GMAX * 1024 * 8 && ((size_t)mind & 7) == 0) {
        const int ppt = fps_ppt(N, group);
        const int G = (N + FPSC_T * ppt - 1) / (FPSC_T * ppt);
        const long long stride = ((long long)N / 2) & ~1ll;                           // 64-bit words per cloud
        unsigned long long* ring = reinterpret_cast<unsigned long long*>(mind);
        // cleared by a kernel, not hipMemsetAsync: a memset node inside a captured hipGraph was observed to race with the
        // kernel node that follows it (csrc/emd.hip)
        hipLaunchKernelGGL(fps_init_kernel, dim3(256), dim3(256), 0, s, mind, (long long)B * N, B, stride, FPSC_RINGM);
        const dim3 grid(B * G), block(FPSC_T);
#define PF_FPS_LAUNCH(PPT) hipLaunchKernelGGL(fps_coopm_kernel<PPT>, grid, block, 0, s, xyz, N, npoint, G, ring, stride, idx_out)
        switch (ppt) {
            case 1: PF_FPS_LAUNCH(1); break;
            case 4: PF_FPS_LAUNCH(4); break;
            case 8: PF_FPS_LAUNCH(8); break;
            case 12: PF_FPS_LAUNCH(12); break;                                         // (group-aligned shapes)
            case 16: PF_FPS_LAUNCH(16); break;
            case 20: PF_FPS_LAUNCH(20); break;
            case 24: PF_FPS_LAUNCH(24); break;
            default: PF_FPS_LAUNCH(32); break;
        }
#undef PF_FPS_LAUNCH
        return pf_last_launch_status();
    }
    hipLaunchKernelGGL(fps_kernel, dim3(B), dim3(FPS_T), 0, s, xyz, N, npoint, mind, idx_out);
    return pf_last_launch_status();
}

// `rounds` exchange rounds of the cooperative FPS protocol between G workgroups (2 <= G <= 32) with no points to update: the
// floor of a round of the two-sample protocol.  ring: >= 1032 64-bit words of scratch (cleared here); its word 1024 is 0 afterwards
// when every round completed (1 = the bounded spin gave up).  Measurement aid of bench.py --mode pugan.
extern "C" int pf_fps_exchange_probe(int G, int rounds, unsigned long long* ring, void* stream) {
    if (!ring) return PF_ERR_NULL;
    if (G < 2 || G > FPSC_GMAX || rounds <= 0 || ((size_t)ring & 7) != 0) return PF_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fps_init_kernel, dim3(8), dim3(256), 0, s, reinterpret_cast<float*>(ring), 2ll * (FPSC_RING2 + 8), 1,
                       (long long)(FPSC_RING2 + 8), FPSC_RING2);
    hipLaunchKernelGGL(fps_exchange_probe_kernel, dim3(G), dim3(FPSC_T), 0, s, G, rounds, ring);
    return pf_last_launch_status();
}

// K nearest references of every query, K <= N (K <= 8192 when N > 16384): idx [B,M,K] int32, dist [B,M,K] squared L2 (nullable)
extern "C" int pf_knn_large(const float* ref, const float* query, int B, int N, int M, int K, int* idx_out,
                            float* dist_out, void* stream) {
    if (!ref || !query || !idx_out) return PF_ERR_NULL;
    if (B <= 0 || N <= 0 || M <= 0 || K <= 0 || K > N || B > 65535 || (long long)N * 3 > 0x7fffffffll) return PF_ERR_SHAPE;
    int np = 1, kp = 0;
    if (N <= KS_NMAX) {
        while (np < N) np <<= 1;
    } else {
        if (K > KS_KMAX) return PF_ERR_UNSUPPORTED;
        np = KS_NMAX;
        kp = 1;
        while (kp < K) kp <<= 1;
    }
    const size_t lds = (size_t)np * 8;
    allow_lds(knn_sort_kernel, lds);
    hipLaunchKernelGGL(knn_sort_kernel, dim3(M, B), dim3(KS_T), lds, (hipStream_t)stream, ref, query, N, M, K, np, kp,
                       idx_out, dist_out);
    return pf_last_launch_status();
}

// normalize_pc (patch.py:168-178) of B clouds / patches: x [B,N,3] -> out [B,N,3] (may alias x), centroid [B,3], fdist [B]
extern "C" int pf_normalize_pc(const float* x, int B, int N, float* out, float* centroid, float* fdist, void* stream) {
    if (!x || !out || !centroid || !fdist) return PF_ERR_NULL;
    if (B <= 0 || N <= 0 || (long long)N * 3 > 0x7fffffffll) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(normalize_pc_kernel, dim3(B), dim3(NRM_T), 0, (hipStream_t)stream, x, N, out, centroid, fdist);
    return pf_last_launch_status();
}

// ---- ragged entry points: B clouds of n[i] points stored back to back ([sum n, 3]); n / npoint / m are HOST arrays --------------
namespace {
bool fps_coop_size(int N) { return N >= 8192 && N <= FPSC_GMAX * 1024 * 8; }

// Shared by pf_fps_ragged_layout and pf_fps_ragged: the points per thread of the cooperative launch (0: no cooperative cloud)
// and the scratch rows.  One PPT per pass, chosen for the largest cooperative cloud (FPS is exact: the choice changes no index);
// a cloud that would need more than FPSC_GMAX workgroups at that PPT cannot occur, since G grows with N.
int fps_ragged_ppt(const int* n, int B, int group) {
    int nmax = 0;
    for (int i = 0; i < B; ++i)
        if (fps_coop_size(n[i]) && n[i] > nmax) nmax = n[i];
    return nmax ? fps_ppt(nmax, group) : 0;
}
long long fps_ragged_row(int n) { return ((long long)n + 1) & ~1ll; }      // floats: every row starts 64-bit aligned

__global__ __launch_bounds__(256) void fps_ragged_init_kernel(float* p, long long n, long long status_word) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long w = i >> 1;
        p[i] = ((i & 1) == 0 && w >= status_word && ((w - status_word) & 1) == 0) ? __uint_as_float((unsigned)FPSC_ST_INIT) : 0.f;
    }
}
}  // namespace

extern "C" int pf_fps_ragged_layout(const int* n, int B, int group, long long* scratch_off, int* wgs, long long* total_floats,
                                    long long* status_word, long long* status_stride) {
    if (!n) return PF_ERR_NULL;
    if (B <= 0 || group < 0) return PF_ERR_SHAPE;
    long long tot = 0;
    for (int i = 0; i < B; ++i) {
        if (n[i] <= 0) return PF_ERR_SHAPE;
        tot += n[i];
    }
    if (tot * 3 > 0x7fffffffll) return PF_ERR_SHAPE;
    const int ppt = fps_ragged_ppt(n, B, group);
    long long off = 0;
    for (int i = 0; i < B; ++i) {
        if (scratch_off) scratch_off[i] = off;
        if (wgs) wgs[i] = fps_coop_size(n[i]) ? (n[i] + FPSC_T * ppt - 1) / (FPSC_T * ppt) : 0;
        off += fps_ragged_row(n[i]);
    }
    if (total_floats) *total_floats = off + 4ll * B;                     // + {status, rounds} per cloud
    if (status_word) *status_word = off / 2;
    if (status_stride) *status_stride = 2;
    return ppt;
}

namespace {
// pf_fps_ragged (n_ctx = nullptr: the kernels without a context) and pf_fps_ragged_ctx (n_ctx: the context kernels, for every
// cloud of the pass - one with n_ctx[i] = 0 takes the other kernels' path inside them)
int fps_ragged_run(const float* xyz, const int* n, const int* npoint, const float* ctx, const int* n_ctx, int B, int group,
                   float* scratch, int* idx_out, float* r2_out, hipStream_t s) {
    long long total = 0, sw = 0;
    const int ppt = pf_fps_ragged_layout(n, B, group, nullptr, nullptr, &total, &sw, nullptr);
    if (ppt < 0) return ppt;
    if (((size_t)scratch & 7) != 0) return PF_ERR_SHAPE;
    for (int i = 0; i < B; ++i)
        if (npoint[i] <= 0 || npoint[i] > n[i]) return PF_ERR_SHAPE;
    if (n_ctx) {
        long long ctot = 0;
        for (int i = 0; i < B; ++i) {
            if (n_ctx[i] < 0) return PF_ERR_SHAPE;
            ctot += n_ctx[i];
        }
        if (ctot * 3 > 0x7fffffffll) return PF_ERR_SHAPE;
        if (ctot > 0 && !ctx) return PF_ERR_NULL;
    }
    unsigned long long* status = reinterpret_cast<unsigned long long*>(scratch) + sw;
    hipLaunchKernelGGL(fps_ragged_init_kernel, dim3(256), dim3(256), 0, s, scratch, total, sw);
    // two kernel families, each in launches of up to PF_RAGGED_MAXB clouds in batch order: cooperative, then single-workgroup
    for (int fam = 0; fam < 2; ++fam) {
        FpsRaggedTab t;
        FpsCtxTab ct;
        int nc = 0;
        long long poff = 0, ooff = 0, soff = 0, coff = 0;
        auto launch = [&]() {
            if (!nc) return;
            if (fam == 0) {
                const dim3 grid(t.wg0[nc]), block(FPSC_T);
#define PF_FPS_LAUNCH(PPT)                                                                                                        \
    do {                                                                                                                          \
        if (n_ctx) hipLaunchKernelGGL(fps_coopm_ragged_ctx_kernel<PPT>, grid, block, 0, s, xyz, t, ct, nc, ctx, scratch, status,  \
                                      idx_out, r2_out);                                                                           \
        else hipLaunchKernelGGL(fps_coopm_ragged_kernel<PPT>, grid, block, 0, s, xyz, t, nc, scratch, status, idx_out);           \
    } while (0)
                switch (ppt) {
                    case 1: PF_FPS_LAUNCH(1); break;
                    case 4: PF_FPS_LAUNCH(4); break;
                    case 8: PF_FPS_LAUNCH(8); break;
                    case 12: PF_FPS_LAUNCH(12); break;
                    case 16: PF_FPS_LAUNCH(16); break;
                    case 20: PF_FPS_LAUNCH(20); break;
                    case 24: PF_FPS_LAUNCH(24); break;
                    default: PF_FPS_LAUNCH(32); break;
                }
#undef PF_FPS_LAUNCH
            } else if (n_ctx) {
                hipLaunchKernelGGL(fps_ragged_ctx_kernel, dim3(nc), dim3(FPS_T), 0, s, xyz, t, ct, ctx, scratch, status, idx_out,
                                   r2_out);
            } else {
                hipLaunchKernelGGL(fps_ragged_kernel, dim3(nc), dim3(FPS_T), 0, s, xyz, t, scratch, status, idx_out);
            }
            nc = 0;
        };
        for (int i = 0; i < B; ++i) {
            // a cloud larger than the cooperative kernel's 32 workgroups x 8192 points runs on one workgroup, as in pf_fps
            if ((fps_coop_size(n[i]) ? 0 : 1) == fam) {
                if (nc == 0) t.wg0[0] = 0;
                t.off[nc] = (int)poff; t.n[nc] = n[i]; t.npoint[nc] = npoint[i]; t.ooff[nc] = (int)ooff; t.cloud[nc] = i;
                t.soff[nc] = soff;
                ct.coff[nc] = (int)coff; ct.nctx[nc] = n_ctx ? n_ctx[i] : 0;
                t.wg0[nc + 1] = t.wg0[nc] + (fam == 0 ? (n[i] + FPSC_T * ppt - 1) / (FPSC_T * ppt) : 1);
                if (++nc == PF_RAGGED_MAXB) launch();
            }
            poff += n[i]; ooff += npoint[i]; soff += fps_ragged_row(n[i]); coff += n_ctx ? n_ctx[i] : 0;
        }
        launch();
    }
    return pf_last_launch_status();
}
}  // namespace

extern "C" int pf_fps_ragged(const float* xyz, const int* n, const int* npoint, int B, int group, float* scratch, int* idx_out,
                             void* stream) {
    if (!xyz || !n || !npoint || !scratch || !idx_out) return PF_ERR_NULL;
    return fps_ragged_run(xyz, n, npoint, nullptr, nullptr, B, group, scratch, idx_out, nullptr, (hipStream_t)stream);
}

extern "C" int pf_fps_ragged_ctx(const float* xyz, const int* n, const int* npoint, const float* ctx, const int* n_ctx, int B,
                                 int group, float* scratch, int* idx_out, float* r2_out, void* stream) {
    if (!xyz || !n || !npoint || !n_ctx || !scratch || !idx_out) return PF_ERR_NULL;
    return fps_ragged_run(xyz, n, npoint, ctx, n_ctx, B, group, scratch, idx_out, r2_out, (hipStream_t)stream);
}

extern "C" int pf_knn_large_ragged(const float* ref, const float* query, const int* n, const int* m, int B, int K, int* idx_out,
                                   float* dist_out, void* stream) {
    if (!ref || !query || !n || !m || !idx_out) return PF_ERR_NULL;
    if (B <= 0 || K <= 0) return PF_ERR_SHAPE;
    long long nt = 0, mt = 0;
    int npmax = 1;
    for (int i = 0; i < B; ++i) {
        if (n[i] <= 0 || m[i] <= 0 || K > n[i]) return PF_ERR_SHAPE;
        if (n[i] > KS_NMAX && K > KS_KMAX) return PF_ERR_UNSUPPORTED;
        int np, kp;
        knn_sort_shape(n[i], K, &np, &kp);
        if (np > npmax) npmax = np;
        nt += n[i]; mt += m[i];
    }
    if (nt * 3 > 0x7fffffffll || mt * 3 > 0x7fffffffll) return PF_ERR_SHAPE;
    const size_t lds = (size_t)npmax * 8;
    allow_lds(knn_sort_ragged_kernel, lds);
    long long roff = 0, q = 0;
    for (int c0 = 0; c0 < B; c0 += PF_RAGGED_MAXB) {
        KnnRaggedTab t;
        const int nc = B - c0 < PF_RAGGED_MAXB ? B - c0 : PF_RAGGED_MAXB;
        t.q0[0] = (int)q;
        for (int c = 0; c < nc; ++c) {
            t.roff[c] = (int)roff; t.n[c] = n[c0 + c];
            roff += n[c0 + c]; q += m[c0 + c];
            t.q0[c + 1] = (int)q;
        }
        hipLaunchKernelGGL(knn_sort_ragged_kernel, dim3(t.q0[nc] - t.q0[0]), dim3(KS_T), lds, (hipStream_t)stream, ref, query, t, nc,
                           K, idx_out, dist_out);
    }
    return pf_last_launch_status();
}

extern "C" int pf_normalize_pc_ragged(const float* x, const int* n, int B, float* out, float* centroid, float* fdist, void* stream) {
    if (!x || !n || !out || !centroid || !fdist) return PF_ERR_NULL;
    if (B <= 0) return PF_ERR_SHAPE;
    long long tot = 0;
    for (int i = 0; i < B; ++i) {
        if (n[i] <= 0) return PF_ERR_SHAPE;
        tot += n[i];
    }
    if (tot * 3 > 0x7fffffffll) return PF_ERR_SHAPE;
    long long off = 0;
    for (int c0 = 0; c0 < B; c0 += PF_RAGGED_MAXB) {
        NrmRaggedTab t;
        const int nc = B - c0 < PF_RAGGED_MAXB ? B - c0 : PF_RAGGED_MAXB;
        for (int c = 0; c < nc; ++c) { t.off[c] = (int)off; off += n[c0 + c]; }
        t.off[nc] = (int)off;
        hipLaunchKernelGGL(normalize_pc_ragged_kernel, dim3(nc), dim3(NRM_T), 0, (hipStream_t)stream, x, t, out, centroid + c0 * 3,
                           fdist + c0);
    }
    return pf_last_launch_status();
}
