// Philox-4x32-10 (Salmon et al. 2011; Random123's constants and round function) and the word-to-uniform mapping, shared by
// the kernels that draw counter-based random numbers (data_aug.hip: training batches; eval_uniform.hip: surface seeds).
// tests/philox_ref.py is the numpy restatement.
#pragma once
#include <hip/hip_runtime.h>

struct U4 { unsigned x, y, z, w; };

// counter (c0 c1 c2 c3), key (k0 k1)
__device__ __forceinline__ U4 philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        const unsigned n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return U4{c0, c1, c2, c3};
}
// u = (x >> 8) 2^-24 + 2^-25 rounded to fp32, kept below 1 (the largest 24-bit value would round to 1.0)
__device__ __forceinline__ float u01(unsigned x) {
    return fminf(fmaf((float)(x >> 8), 0x1p-24f, 0x1p-25f), 0x1.fffffep-1f);
}
