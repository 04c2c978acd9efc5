// Device idioms every kernel file shares: the relaxed agent-scope atomic load / store, DPP row and wave reductions, and the
// __shfl_xor butterflies.  Device code only, everything inlined.  The DPP control words and the atomics' constant arguments
// are spelled here and nowhere else.
//
// Operand order is part of the contract (float results depend on it): every step is op(v, <the other lane's v>), masks and
// rotates run in the order given, and the four rows of a wave combine as op(op(row 0, row 1), op(row 2, row 3)).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

// relaxed agent-scope atomic load / store: a word other workgroups of the launch write / read (never cached in the CU's L1);
// no ordering, i.e. no L2 write-back or invalidate.  Macros, not functions: a call inlined into a conditional arm or a poll loop
// leaves the compiler with another block order, and kernels that only load or store such words would no longer compile to the
// instruction streams they had (tools/cmp_isa.py).
#define PF_LD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define PF_ST(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// v of the lane a DPP control word names (row_ror:n = 0x120 + n: the lane n to the left within the 16-lane row, cyclic)
template <int CTRL, class T>
__device__ __forceinline__ T pf_dpp(T v) {
    static_assert(sizeof(T) == 4, "one 32-bit register");
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// v of lane `lane` (wave-uniform), through an SGPR
template <class T>
__device__ __forceinline__ T pf_lane(T v, int lane) {
    static_assert(sizeof(T) == 4, "one 32-bit register");
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// the reductions' operators (a lambda over T works too): max / min of floats are fmaxf / fminf, of integers max / min
struct PfSum {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct PfMax {
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
    __device__ __forceinline__ int operator()(int a, int b) const { return max(a, b); }
    __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return max(a, b); }
};
struct PfMin {
    __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
    __device__ __forceinline__ int operator()(int a, int b) const { return min(a, b); }
    __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return min(a, b); }
};

// reduction over the 16 lanes of a DPP row (= the 16 columns of one MFMA tile) by four rotates, the result in every lane of the row
template <class T, class Op>
__device__ __forceinline__ T pf_row_reduce(T v, Op op) {
    v = op(v, pf_dpp<0x128>(v)); v = op(v, pf_dpp<0x124>(v)); v = op(v, pf_dpp<0x122>(v)); v = op(v, pf_dpp<0x121>(v));
    return v;
}
// ... and over the wave: the four row results through SGPRs, no LDS traffic.  The result is wave-uniform.
template <class T, class Op>
__device__ __forceinline__ T pf_wave_reduce(T v, Op op) {
    v = pf_row_reduce(v, op);
    return op(op(pf_lane(v, 0), pf_lane(v, 16)), op(pf_lane(v, 32), pf_lane(v, 48)));
}

// __shfl_xor butterfly over the masks FIRST, 2 FIRST, .. LAST (FIRST > LAST: FIRST, FIRST / 2, .. LAST), fully unrolled; every
// lane of a group of 2 max(FIRST, LAST) lanes ends with the group's result
template <int FIRST, int LAST, class T, class Op>
__device__ __forceinline__ T pf_xor_reduce(T v, Op op) {
    if constexpr (FIRST <= LAST) {
#pragma unroll
        for (int m = FIRST; m <= LAST; m <<= 1) v = op(v, __shfl_xor(v, m));
    } else {
#pragma unroll
        for (int m = FIRST; m >= LAST; m >>= 1) v = op(v, __shfl_xor(v, m));
    }
    return v;
}
template <int FIRST, int LAST, class T>
__device__ __forceinline__ T pf_xor_sum(T v) { return pf_xor_reduce<FIRST, LAST>(v, PfSum{}); }
template <int FIRST, int LAST, class T>
__device__ __forceinline__ T pf_xor_max(T v) { return pf_xor_reduce<FIRST, LAST>(v, PfMax{}); }
template <int FIRST, int LAST, class T>
__device__ __forceinline__ T pf_xor_min(T v) { return pf_xor_reduce<FIRST, LAST>(v, PfMin{}); }
template <class T>
__device__ __forceinline__ T pf_wave_sum(T v) { return pf_xor_sum<1, 32>(v); }      // all 64 lanes, masks 1 .. 32

// arg-max butterfly over the masks FIRST, 2 FIRST, .. LAST: the largest value and, among equal values, the smallest index
template <int FIRST, int LAST>
__device__ __forceinline__ void pf_xor_argmax(float& best, int& idx) {
#pragma unroll
    for (int m = FIRST; m <= LAST; m <<= 1) {
        const float ov = __shfl_xor(best, m);
        const int oi = __shfl_xor(idx, m);
        if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
}
