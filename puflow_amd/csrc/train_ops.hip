// The element-wise building blocks of the TRAINING step (train-mode forward with BatchNorm batch statistics, and the
// backward of every layer).  The reference trains with eager PyTorch ops on materialised
// [B,C,N,K] tensors (modules/discrete/interpflow.py:203-258, train_pu1k.py:53-74); here each of those
// ops is one hand-written kernel pair on channels-last [rows, C] fp32 tensors, wired into autograd
// by puflow_amd/train_perop.py.  This is the per-op reference tier of the fused training kernels; the matrix
// products of both tiers are csrc/train_gemm.hip.
//
//   colstat / bn    BatchNorm2d(train) + LeakyReLU forward / backward (two-pass mean / variance), whole and in stages
//   colsum          per-column sums (bias and flow-parameter gradients)
//   act             LeakyReLU / ReLU forward / backward
//   edge_feature    [x_i, x_j, x_j - x_i] gather forward, scatter-add backward   (interpflow.py:223-232)
//   maxpool_k       max over the K neighbours + argmax, backward                  (interpflow.py:245)
//   scatter_rows    backward of a row gather (z[idx], interpflow.py:183)
//   softmax_wsum    softmax over K of R logit channels, weighted sum of neighbour latents, backward (interpflow.py:180-185)
//   group_sum       backward of repeat_interleave(cs, R) (interpflow.py:319)
//   flow-block algebra on [R,3] rows (second part): ActNorm, coupling + injector, batch sums, distance features
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"
#include "pf_mfma.h"

namespace {

// ----------------------------------------------------------------------------- column statistics
// partial[chunk][which][c] over rows [chunk*rows_per, ...): MODE 0: sum x          (1 value)
//                                                             MODE 1: sum (x - mean[c])^2     (1)
//                                                             MODE 2: sum dz, sum dz*xhat     (2)  dz = dy * lrelu'(pre)
template <int MODE>
__global__ __launch_bounds__(256) void colstat_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                     const float* __restrict__ mean, const float* __restrict__ invstd,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float slope, long long R, int C, int rows_per,
                                                     float* __restrict__ partial) {
    __shared__ float s0[4][64], s1[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
    const long long r_lo = (long long)blockIdx.y * rows_per, r_hi = min(R, r_lo + rows_per);
    float a0 = 0.f, a1 = 0.f;
    if (c < C) {
        const float mu = MODE >= 1 ? mean[c] : 0.f;
        const float is = MODE == 2 ? invstd[c] : 0.f, ga = MODE == 2 ? gamma[c] : 0.f, be = MODE == 2 ? beta[c] : 0.f;
        for (long long r = r_lo + rl; r < r_hi; r += 4) {
            const float v = x[r * C + c];
            if (MODE == 0) a0 += v;
            else if (MODE == 1) { const float d = v - mu; a0 += d * d; }
            else {
                const float xh = (v - mu) * is;
                const float dz = dy[r * C + c] * ((xh * ga + be) > 0.f ? 1.f : slope);
                a0 += dz; a1 += dz * xh;
            }
        }
    }
    s0[rl][threadIdx.x & 63] = a0; s1[rl][threadIdx.x & 63] = a1;
    __syncthreads();
    if (rl == 0 && c < C) {
        const int l = threadIdx.x;
        partial[((long long)blockIdx.y * 2 + 0) * C + c] = (s0[0][l] + s0[1][l]) + (s0[2][l] + s0[3][l]);
        if (MODE == 2) partial[((long long)blockIdx.y * 2 + 1) * C + c] = (s1[0][l] + s1[1][l]) + (s1[2][l] + s1[3][l]);
    }
}

// float4 variant for C % 4 == 0: a thread owns 4 consecutive channels, `cgl` (power of two <= 64) channel lanes cover
// one row segment and 256 / cgl row lanes walk the rows, so every wave-instruction reads whole contiguous rows.
template <int MODE>
__global__ __launch_bounds__(256) void colstat4_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                      const float* __restrict__ mean, const float* __restrict__ invstd,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float slope, long long R, int C, int rows_per, int cgl,
                                                      float* __restrict__ partial) {
    __shared__ f4 s0[256], s1[256];
    const int cl = threadIdx.x % cgl, rl = threadIdx.x / cgl, nrl = 256 / cgl;
    const int c = (blockIdx.x * cgl + cl) * 4;
    const long long r_lo = (long long)blockIdx.y * rows_per, r_hi = min(R, r_lo + rows_per);
    f4 a0 = pf_splat(0.f), a1 = pf_splat(0.f);
    if (c < C) {
        f4 mu = pf_splat(0.f), is = pf_splat(0.f), ga = pf_splat(0.f), be = pf_splat(0.f);
        if (MODE >= 1) mu = *reinterpret_cast<const f4*>(mean + c);
        if (MODE == 2) {
            is = *reinterpret_cast<const f4*>(invstd + c);
            ga = *reinterpret_cast<const f4*>(gamma + c);
            be = *reinterpret_cast<const f4*>(beta + c);
        }
        for (long long r = r_lo + rl; r < r_hi; r += nrl) {
            const f4 v = *reinterpret_cast<const f4*>(x + r * C + c);
            if (MODE == 0) a0 += v;
            else if (MODE == 1) { const f4 d = v - mu; a0 += d * d; }
            else {
                const f4 g = *reinterpret_cast<const f4*>(dy + r * C + c);
                const f4 xh = (v - mu) * is;
                const f4 pre = xh * ga + be;
                f4 dz;
#pragma unroll
                for (int i = 0; i < 4; ++i) dz[i] = g[i] * (pre[i] > 0.f ? 1.f : slope);
                a0 += dz; a1 += dz * xh;
            }
        }
    }
    s0[threadIdx.x] = a0; s1[threadIdx.x] = a1;
    __syncthreads();
    for (int st = nrl >> 1; st > 0; st >>= 1) {                    // fixed tree over the row lanes
        if (rl < st) { s0[threadIdx.x] += s0[threadIdx.x + st * cgl]; s1[threadIdx.x] += s1[threadIdx.x + st * cgl]; }
        __syncthreads();
    }
    if (rl == 0 && c < C) {
        *reinterpret_cast<f4*>(partial + ((long long)blockIdx.y * 2 + 0) * C + c) = s0[cl];
        if (MODE == 2) *reinterpret_cast<f4*>(partial + ((long long)blockIdx.y * 2 + 1) * C + c) = s1[cl];
    }
}

template <int MODE>
void colstat_launch(const float* x, const float* dy, const float* mean, const float* invstd, const float* gamma,
                    const float* beta, float slope, long long R, int C, int nchunk, int rows_per, float* partial, hipStream_t s) {
    if (C % 4 == 0) {
        int cgl = 1;
        while (cgl < C / 4 && cgl < 64) cgl <<= 1;
        hipLaunchKernelGGL(colstat4_kernel<MODE>, dim3((C / 4 + cgl - 1) / cgl, nchunk), dim3(256), 0, s, x, dy, mean, invstd, gamma,
                           beta, slope, R, C, rows_per, cgl, partial);
    } else {
        hipLaunchKernelGGL(colstat_kernel<MODE>, dim3((C + 63) / 64, nchunk), dim3(256), 0, s, x, dy, mean, invstd, gamma, beta,
                           slope, R, C, rows_per, partial);
    }
}

// out[which][c] = scale * sum_chunks partial   (fixed order: 4 interleaved chunk lanes, then a fixed tree)
__global__ __launch_bounds__(256) void colstat_final_kernel(const float* __restrict__ partial, int nchunk, int C, int nwhich,
                                                           float scale, float* __restrict__ out) {
    __shared__ float sh[4][64];
    const int l = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + l;
    for (int w = 0; w < nwhich; ++w) {
        float s = 0.f;
        if (c < C)
            for (int k = part; k < nchunk; k += 4) s += partial[((long long)k * 2 + w) * C + c];
        sh[part][l] = s;
        __syncthreads();
        if (part == 0 && c < C) out[w * C + c] = ((sh[0][l] + sh[1][l]) + (sh[2][l] + sh[3][l])) * scale;
        __syncthreads();
    }
}

// BatchNorm backward: the two column sums once, written unscaled to (dbeta, dgamma) and scaled by 1/R to sums[2][C] - one
// launch, no device-to-device copy nodes (a copy node that reads `sums` right before a kernel node that overwrites it is a
// write-after-read across a memcpy -> kernel edge of a captured graph; the per-op path is captured whenever it is taken)
__global__ __launch_bounds__(256) void colstat_final_bwd_kernel(const float* __restrict__ partial, int nchunk, int C, float inv_r,
                                                               float* __restrict__ dbeta, float* __restrict__ dgamma,
                                                               float* __restrict__ sums) {
    __shared__ float sh[4][64];
    const int l = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + l;
    for (int w = 0; w < 2; ++w) {
        float s = 0.f;
        if (c < C)
            for (int k = part; k < nchunk; k += 4) s += partial[((long long)k * 2 + w) * C + c];
        sh[part][l] = s;
        __syncthreads();
        if (part == 0 && c < C) {
            const float t = (sh[0][l] + sh[1][l]) + (sh[2][l] + sh[3][l]);
            (w == 0 ? dbeta : dgamma)[c] = t * 1.0f;
            sums[w * C + c] = t * inv_r;
        }
        __syncthreads();
    }
}

// save[0..C) = mean (copied by the kernel: no copy node), save[C..2C) = 1/sqrt(var_b + eps); running statistics (nullable)
__global__ void bn_finish_kernel(const float* __restrict__ var_b, int C, float eps, float momentum, float unbias,
                                 const float* __restrict__ mean, float* __restrict__ invstd, float* __restrict__ run_mean,
                                 float* __restrict__ run_var, float* __restrict__ mean_out) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    invstd[c] = 1.0f / sqrtf(var_b[c] + eps);
    if (mean_out && mean_out != mean) mean_out[c] = mean[c];
    if (run_mean) {
        run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * mean[c];
        run_var[c] = (1.f - momentum) * run_var[c] + momentum * (var_b[c] * unbias);
    }
}

__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                      const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float slope, long long total, int C,
                                                      float* __restrict__ y) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const float v = (x[i] - mean[c]) * invstd[c] * gamma[c] + beta[c];
        y[i] = v > 0.f ? v : v * slope;
    }
}

// dx = gamma*invstd*(dz - s1/R - xhat*s2/R)
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                          const float* __restrict__ mean, const float* __restrict__ invstd,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const float* __restrict__ sums /*[2][C] already / R*/,
                                                          float slope, long long total, int C, float* __restrict__ dx) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const float xh = (x[i] - mean[c]) * invstd[c];
        const float dz = dy[i] * ((xh * gamma[c] + beta[c]) > 0.f ? 1.f : slope);
        dx[i] = gamma[c] * invstd[c] * (dz - sums[c] - xh * sums[C + c]);
    }
}

// y = x > 0 ? x : slope*x  ;  dx = dy * (y > 0 ? 1 : slope)
__global__ __launch_bounds__(256) void act_fwd_kernel(const float* __restrict__ x, float slope, long long total,
                                                     float* __restrict__ y) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const float v = x[i];
        y[i] = v > 0.f ? v : v * slope;
    }
}
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy, float slope,
                                                     long long total, float* __restrict__ dx) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256)
        dx[i] = dy[i] * (y[i] > 0.f ? 1.f : slope);
}

// ------------------------------------------------------------------------- edge features / pooling
// out[e][0:C] = x_i, [C:2C] = x_j, [2C:3C] = x_j - x_i ; e = t*K + k, j = (t / N)*N + idx[e]
__global__ __launch_bounds__(256) void edge_feature_fwd_kernel(const float* __restrict__ x, const int* __restrict__ idx,
                                                              int N, int K, int C, long long total /*E*C*/,
                                                              float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long e = i / C;
        const int c = (int)(i % C);
        const long long t = e / K;
        const long long j = (t / N) * N + idx[e];
        const float xi = x[t * C + c], xj = x[j * C + c];
        float* o = out + e * 3 * C;
        o[c] = xi; o[C + c] = xj; o[2 * C + c] = xj - xi;
    }
}
// dx[t] += g1 - g3 ; dx[j] += g2 + g3
__global__ __launch_bounds__(256) void edge_feature_bwd_kernel(const float* __restrict__ g, const int* __restrict__ idx,
                                                              int N, int K, int C, long long total,
                                                              float* __restrict__ dx) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long e = i / C;
        const int c = (int)(i % C);
        const long long t = e / K;
        const long long j = (t / N) * N + idx[e];
        const float* gg = g + e * 3 * C;
        atomicAdd(&dx[t * C + c], gg[c] - gg[2 * C + c]);
        atomicAdd(&dx[j * C + c], gg[C + c] + gg[2 * C + c]);
    }
}

__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ y, int K, int C, long long total /*T*C*/,
                                                         float* __restrict__ out, int* __restrict__ arg) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long t = i / C;
        const int c = (int)(i % C);
        float best = y[(t * K) * C + c];
        int bi = 0;
        for (int k = 1; k < K; ++k) {
            const float v = y[(t * K + k) * C + c];
            if (v > best) { best = v; bi = k; }
        }
        out[i] = best; arg[i] = bi;
    }
}
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dy, const int* __restrict__ arg, int K,
                                                         int C, long long total /*T*K*C*/, float* __restrict__ dx) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long e = i / C;
        const int c = (int)(i % C);
        const long long t = e / K;
        const int k = (int)(e % K);
        dx[i] = arg[t * C + c] == k ? dy[t * C + c] : 0.f;
    }
}

// out[row[e]] += g[e]   (rows given as batch-local idx: row = (t / N)*N + idx[e], t = e / K)
__global__ __launch_bounds__(256) void scatter_rows_kernel(const float* __restrict__ g, const int* __restrict__ idx, int N,
                                                          int K, int C, long long total, float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long e = i / C;
        const int c = (int)(i % C);
        const long long t = e / K;
        const long long j = (t / N) * N + idx[e];
        atomicAdd(&out[j * C + c], g[i]);
    }
}

// out[t][c] = sum_r g[t*R + r][c]
__global__ __launch_bounds__(256) void group_sum_kernel(const float* __restrict__ g, int R, int C, long long total /*T*C*/,
                                                       float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long t = i / C;
        const int c = (int)(i % C);
        float s = 0.f;
        for (int r = 0; r < R; ++r) s += g[(t * R + r) * C + c];
        out[i] = s;
    }
}

// ---- softmax over K of R logit channels + weighted latent sum; one thread per point (K = 8; R: any up-ratio the weight unit's
// 32 logit channels allow - the kernels loop over r and hold nothing sized by R; the g chain takes R = 16, and train_ops sends
// R > 8 here)
constexpr int SW_K = 8, SW_RMAX = 32;
__global__ __launch_bounds__(256) void softmax_wsum_fwd_kernel(const float* __restrict__ w /*[T,K,ldw] first R used*/,
                                                              int ldw, const float* __restrict__ zj /*[T,K,3]*/, int R,
                                                              long long T, float* __restrict__ a /*[T,K,R]*/,
                                                              float* __restrict__ fz /*[T,3,R]*/) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    for (int r = 0; r < R; ++r) {
        float m = -__builtin_inff();
        for (int k = 0; k < SW_K; ++k) m = fmaxf(m, w[(t * SW_K + k) * ldw + r]);
        float e[SW_K], s = 0.f;
        for (int k = 0; k < SW_K; ++k) { e[k] = expf(w[(t * SW_K + k) * ldw + r] - m); s += e[k]; }
        float o0 = 0.f, o1 = 0.f, o2 = 0.f;
        for (int k = 0; k < SW_K; ++k) {
            const float ak = e[k] / s;
            a[(t * SW_K + k) * R + r] = ak;
            const float* z = zj + (t * SW_K + k) * 3;
            o0 += ak * z[0]; o1 += ak * z[1]; o2 += ak * z[2];
        }
        fz[(t * 3 + 0) * R + r] = o0; fz[(t * 3 + 1) * R + r] = o1; fz[(t * 3 + 2) * R + r] = o2;
    }
}
// dzj[t,k,c] = sum_r a dfz ; dw[t,k,r] = a (da - sum_k a da), da[t,k,r] = sum_c dfz[t,c,r] zj[t,k,c]; dw beyond R = 0
__global__ __launch_bounds__(256) void softmax_wsum_bwd_kernel(const float* __restrict__ a, const float* __restrict__ zj,
                                                              const float* __restrict__ dfz, int R, int ldw, long long T,
                                                              float* __restrict__ dw, float* __restrict__ dzj) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    float dz[SW_K][3];
    for (int k = 0; k < SW_K; ++k) dz[k][0] = dz[k][1] = dz[k][2] = 0.f;
    for (int r = 0; r < R; ++r) {
        const float g0 = dfz[(t * 3 + 0) * R + r], g1 = dfz[(t * 3 + 1) * R + r], g2 = dfz[(t * 3 + 2) * R + r];
        float da[SW_K], dot = 0.f;
        for (int k = 0; k < SW_K; ++k) {
            const float* z = zj + (t * SW_K + k) * 3;
            const float ak = a[(t * SW_K + k) * R + r];
            da[k] = g0 * z[0] + g1 * z[1] + g2 * z[2];
            dot += ak * da[k];
            dz[k][0] += ak * g0; dz[k][1] += ak * g1; dz[k][2] += ak * g2;
        }
        for (int k = 0; k < SW_K; ++k) dw[(t * SW_K + k) * ldw + r] = a[(t * SW_K + k) * R + r] * (da[k] - dot);
    }
    for (int k = 0; k < SW_K; ++k) {
        for (int r = R; r < ldw; ++r) dw[(t * SW_K + k) * ldw + r] = 0.f;
        for (int c = 0; c < 3; ++c) dzj[(t * SW_K + k) * 3 + c] = dz[k][c];
    }
}

inline unsigned grid_for(long long total) {
    long long g = (total + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace

// BatchNorm(train) + LeakyReLU forward on x [R,C].  save [2][C] = mean, invstd (out); running stats updated in place
// (nullable); ws >= 2*nchunk*C + 2*C floats with nchunk = pf_bn_chunks(R).
extern "C" int pf_bn_chunks(long long R) { long long n = (R + 1023) / 1024; return (int)(n > 1024 ? 1024 : (n < 1 ? 1 : n)); }

extern "C" int pf_bn_lrelu_fwd(const float* x, long long R, int C, const float* gamma, const float* beta, float slope,
                               float eps, float momentum, float* run_mean, float* run_var, float* y, float* save, float* ws,
                               void* stream) {
    if (!x || !gamma || !beta || !y || !save || !ws) return PF_ERR_NULL;
    if (R <= 1 || C <= 0) return PF_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    const int nchunk = pf_bn_chunks(R);
    const int rows_per = (int)((R + nchunk - 1) / nchunk);
    float* partial = ws;
    float* var_b = ws + (long long)2 * nchunk * C;
    dim3 gc((C + 63) / 64);
    colstat_launch<0>(x, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, R, C, nchunk, rows_per, partial, s);
    hipLaunchKernelGGL(colstat_final_kernel, gc, dim3(256), 0, s, partial, nchunk, C, 1, 1.0f / (float)R, save);
    colstat_launch<1>(x, nullptr, save, nullptr, nullptr, nullptr, 0.f, R, C, nchunk, rows_per, partial, s);
    hipLaunchKernelGGL(colstat_final_kernel, gc, dim3(256), 0, s, partial, nchunk, C, 1, 1.0f / (float)R, var_b);
    hipLaunchKernelGGL(bn_finish_kernel, gc, dim3(64), 0, s, var_b, C, eps, momentum, (float)R / (float)(R - 1), save, save + C,
                       run_mean, run_var, (float*)nullptr);
    hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_for(R * C)), dim3(256), 0, s, x, save, save + C, gamma, beta, slope, R * C, C, y);
    return pf_last_launch_status();
}

// backward: dx [R,C], dgamma [C], dbeta [C]
extern "C" int pf_bn_lrelu_bwd(const float* x, const float* dy, long long R, int C, const float* gamma, const float* beta,
                               float slope, const float* save, float* dx, float* dgamma, float* dbeta, float* ws,
                               void* stream) {
    if (!x || !dy || !gamma || !beta || !save || !dx || !dgamma || !dbeta || !ws) return PF_ERR_NULL;
    if (R <= 1 || C <= 0) return PF_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    const int nchunk = pf_bn_chunks(R);
    const int rows_per = (int)((R + nchunk - 1) / nchunk);
    float* partial = ws;
    float* sums = ws + (long long)2 * nchunk * C;          // [2][C]: sum dz, sum dz*xhat
    dim3 gc((C + 63) / 64);
    colstat_launch<2>(x, dy, save, save + C, gamma, beta, slope, R, C, nchunk, rows_per, partial, s);
    hipLaunchKernelGGL(colstat_final_bwd_kernel, gc, dim3(256), 0, s, partial, nchunk, C, 1.0f / (float)R, dbeta, dgamma, sums);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for(R * C)), dim3(256), 0, s, x, dy, save, save + C, gamma, beta, sums, slope,
                       R * C, C, dx);
    return pf_last_launch_status();
}

// ---- the same BatchNorm in stages, so that the per-column sums can be all-reduced between them (SyncBN across ranks:
// puflow_amd/train_ops.py SyncBnLreluFn).  Statistics are UNSCALED sums here; the host divides by the global row count.
// out[c] = sum_r x[r,c]  (mean_in == NULL)  or  sum_r (x[r,c] - mean_in[c])^2.   ws >= 2*nchunk*C floats.
extern "C" int pf_bn_colstat(const float* x, long long R, int C, const float* mean_in, float* out, float* ws, void* stream) {
    if (!x || !out || !ws) return PF_ERR_NULL;
    if (R <= 0 || C <= 0) return PF_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    const int nchunk = pf_bn_chunks(R);
    const int rows_per = (int)((R + nchunk - 1) / nchunk);
    if (mean_in) colstat_launch<1>(x, nullptr, mean_in, nullptr, nullptr, nullptr, 0.f, R, C, nchunk, rows_per, ws, s);
    else colstat_launch<0>(x, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, R, C, nchunk, rows_per, ws, s);
    hipLaunchKernelGGL(colstat_final_kernel, dim3((C + 63) / 64), dim3(256), 0, s, ws, nchunk, C, 1, 1.0f, out);
    return pf_last_launch_status();
}

// y = lrelu(gamma (x - mean) / sqrt(var_b + eps) + beta) with GIVEN (global) mean / biased variance; save = [mean | invstd];
// running statistics updated with momentum and var_b * unbias (nullable).
extern "C" int pf_bn_apply_stats(const float* x, long long R, int C, const float* mean, const float* var_b, float unbias,
                                 const float* gamma, const float* beta, float slope, float eps, float momentum,
                                 float* run_mean, float* run_var, float* y, float* save, void* stream) {
    if (!x || !mean || !var_b || !gamma || !beta || !y || !save) return PF_ERR_NULL;
    if (R <= 0 || C <= 0) return PF_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_finish_kernel, dim3((C + 63) / 64), dim3(64), 0, s, var_b, C, eps, momentum, unbias, mean, save + C,
                       run_mean, run_var, save);
    hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_for(R * C)), dim3(256), 0, s, x, save, save + C, gamma, beta, slope, R * C, C, y);
    return pf_last_launch_status();
}

// backward, stage 1: sums[2][C] = (sum dz, sum dz * xhat) over THIS rank's rows (= dbeta, dgamma of the local loss)
extern "C" int pf_bn_bwd_sums(const float* x, const float* dy, long long R, int C, const float* gamma, const float* beta,
                              float slope, const float* save, float* sums, float* ws, void* stream) {
    if (!x || !dy || !gamma || !beta || !save || !sums || !ws) return PF_ERR_NULL;
    if (R <= 0 || C <= 0) return PF_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    const int nchunk = pf_bn_chunks(R);
    const int rows_per = (int)((R + nchunk - 1) / nchunk);
    colstat_launch<2>(x, dy, save, save + C, gamma, beta, slope, R, C, nchunk, rows_per, ws, s);
    hipLaunchKernelGGL(colstat_final_kernel, dim3((C + 63) / 64), dim3(256), 0, s, ws, nchunk, C, 2, 1.0f, sums);
    return pf_last_launch_status();
}

// backward, stage 2: dx from the GLOBAL means[2][C] = all-reduced sums / global row count
extern "C" int pf_bn_bwd_apply(const float* x, const float* dy, long long R, int C, const float* gamma, const float* beta,
                               float slope, const float* save, const float* means, float* dx, void* stream) {
    if (!x || !dy || !gamma || !beta || !save || !means || !dx) return PF_ERR_NULL;
    if (R <= 0 || C <= 0) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for(R * C)), dim3(256), 0, (hipStream_t)stream, x, dy, save, save + C, gamma,
                       beta, means, slope, R * C, C, dx);
    return pf_last_launch_status();
}

// column sums of g [R,C] -> out [C] (bias gradients).  ws >= 2*nchunk*C floats.
extern "C" int pf_colsum(const float* g, long long R, int C, float* out, float* ws, void* stream) {
    if (!g || !out || !ws) return PF_ERR_NULL;
    if (R <= 0 || C <= 0) return PF_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    const int nchunk = pf_bn_chunks(R);
    const int rows_per = (int)((R + nchunk - 1) / nchunk);
    colstat_launch<0>(g, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, R, C, nchunk, rows_per, ws, s);
    hipLaunchKernelGGL(colstat_final_kernel, dim3((C + 63) / 64), dim3(256), 0, s, ws, nchunk, C, 1, 1.0f, out);
    return pf_last_launch_status();
}

extern "C" int pf_act_fwd(const float* x, float slope, long long total, float* y, void* stream) {
    if (!x || !y) return PF_ERR_NULL;
    if (total <= 0) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(act_fwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, slope, total, y);
    return pf_last_launch_status();
}
extern "C" int pf_act_bwd(const float* y, const float* dy, float slope, long long total, float* dx, void* stream) {
    if (!y || !dy || !dx) return PF_ERR_NULL;
    if (total <= 0) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(act_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, y, dy, slope, total, dx);
    return pf_last_launch_status();
}

extern "C" int pf_edge_feature_fwd(const float* x, const int* idx, int B, int N, int K, int C, float* out, void* stream) {
    if (!x || !idx || !out) return PF_ERR_NULL;
    if (B <= 0 || N <= 0 || K <= 0 || C <= 0) return PF_ERR_SHAPE;
    const long long total = (long long)B * N * K * C;
    hipLaunchKernelGGL(edge_feature_fwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, idx, N, K, C, total, out);
    return pf_last_launch_status();
}
// dx [B*N, C] must be zero-filled by the caller (accumulates)
extern "C" int pf_edge_feature_bwd(const float* g, const int* idx, int B, int N, int K, int C, float* dx, void* stream) {
    if (!g || !idx || !dx) return PF_ERR_NULL;
    if (B <= 0 || N <= 0 || K <= 0 || C <= 0) return PF_ERR_SHAPE;
    const long long total = (long long)B * N * K * C;
    hipLaunchKernelGGL(edge_feature_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, g, idx, N, K, C, total, dx);
    return pf_last_launch_status();
}

extern "C" int pf_maxpool_k_fwd(const float* y, long long T, int K, int C, float* out, int* arg, void* stream) {
    if (!y || !out || !arg) return PF_ERR_NULL;
    if (T <= 0 || K <= 0 || C <= 0) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(grid_for(T * C)), dim3(256), 0, (hipStream_t)stream, y, K, C, T * C, out, arg);
    return pf_last_launch_status();
}
extern "C" int pf_maxpool_k_bwd(const float* dy, const int* arg, long long T, int K, int C, float* dx, void* stream) {
    if (!dy || !arg || !dx) return PF_ERR_NULL;
    if (T <= 0 || K <= 0 || C <= 0) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(grid_for(T * K * C)), dim3(256), 0, (hipStream_t)stream, dy, arg, K, C, T * K * C, dx);
    return pf_last_launch_status();
}

// out [B*N, C] += g [B*N*K, C] scattered by idx (out zero-filled by the caller)
extern "C" int pf_scatter_rows(const float* g, const int* idx, int B, int N, int K, int C, float* out, void* stream) {
    if (!g || !idx || !out) return PF_ERR_NULL;
    if (B <= 0 || N <= 0 || K <= 0 || C <= 0) return PF_ERR_SHAPE;
    const long long total = (long long)B * N * K * C;
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, g, idx, N, K, C, total, out);
    return pf_last_launch_status();
}

// the same sum as a gather over the transposed lists (pf_knn_csr of idx, lists sorted): one order, run after run - the
// deterministic form (PF_TRAIN_DETERMINISTIC) of the un-fused latent gather's backward.  Accumulated in double and rounded
// once: a hub row's list holds every edge of its cloud (100 in tests/test_gpu_deterministic.py), and the fp32 sum of such a
// list missed float64 by 1.2e-6 on one element, past that test's bar
static __global__ __launch_bounds__(256) void scatter_rows_det_kernel(const float* __restrict__ g, const int* __restrict__ off,
                                                                     const int* __restrict__ edge, int C, long long total,
                                                                     float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long long j = t / C;
    const int c = (int)(t - j * C);
    double s = 0.0;
    for (int q = off[j]; q < off[j + 1]; ++q) s += (double)g[(long long)edge[q] * C + c];
    out[t] = (float)s;
}
extern "C" int pf_scatter_rows_det(const float* g, const int* csr_off, const int* csr_edge, long long T, int C, float* out, void* stream) {
    if (!g || !csr_off || !csr_edge || !out) return PF_ERR_NULL;
    if (T <= 0 || C <= 0) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(scatter_rows_det_kernel, dim3((unsigned)((T * C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, csr_off, csr_edge, C, T * C, out);
    return pf_last_launch_status();
}

extern "C" int pf_group_sum(const float* g, long long T, int R, int C, float* out, void* stream) {
    if (!g || !out) return PF_ERR_NULL;
    if (T <= 0 || R <= 0 || C <= 0) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(group_sum_kernel, dim3(grid_for(T * C)), dim3(256), 0, (hipStream_t)stream, g, R, C, T * C, out);
    return pf_last_launch_status();
}

extern "C" int pf_softmax_wsum_fwd(const float* w, int ldw, const float* zj, int K, int R, long long T, float* a, float* fz,
                                   void* stream) {
    if (!w || !zj || !a || !fz) return PF_ERR_NULL;
    if (K != SW_K || R <= 0 || R > SW_RMAX || R > ldw || T <= 0) return PF_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(softmax_wsum_fwd_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, ldw, zj, R,
                       T, a, fz);
    return pf_last_launch_status();
}
extern "C" int pf_softmax_wsum_bwd(const float* a, const float* zj, const float* dfz, int K, int R, int ldw, long long T,
                                   float* dw, float* dzj, void* stream) {
    if (!a || !zj || !dfz || !dw || !dzj) return PF_ERR_NULL;
    if (K != SW_K || R <= 0 || R > SW_RMAX || R > ldw || T <= 0) return PF_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(softmax_wsum_bwd_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, zj, dfz, R,
                       ldw, T, dw, dzj);
    return pf_last_launch_status();
}

// ============================================================================================================
// Flow-block elementwise algebra on [R,3] rows (training path): ActNorm scale/shift, the additive coupling +
// channel reverse + conditional affine injector, and the Gaussian log-likelihood, each with its backward.
// Reference: modules/flows/normalize.py:30-43, coupling.py:55-58,82-85,114-118,132-151, permutate.py:75-80,
// modules/utils/probs.py:73-75.  One thread per row; parameter gradients are reduced with pf_colsum by the caller.
// ============================================================================================================
namespace {

// y = x*exp(logs)+bias (inv=0)   or   y = (x-bias)*exp(-logs) (inv=1)
__global__ __launch_bounds__(256) void actnorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ logs,
                                                         const float* __restrict__ bias, int inv, long long R,
                                                         float* __restrict__ y) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = x[r * 3 + c];
        y[r * 3 + c] = inv ? (v - bias[c]) * expf(-logs[c]) : v * expf(logs[c]) + bias[c];
    }
}
// dx, and per-row contributions glogs / gbias [R,3] (column-summed by the caller)
__global__ __launch_bounds__(256) void actnorm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                         const float* __restrict__ logs, const float* __restrict__ bias,
                                                         int inv, long long R, float* __restrict__ dx,
                                                         float* __restrict__ glogs, float* __restrict__ gbias) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float g = dy[r * 3 + c], v = x[r * 3 + c];
        if (inv) {
            const float e = expf(-logs[c]);
            dx[r * 3 + c] = g * e;
            gbias[r * 3 + c] = -g * e;
            glogs[r * 3 + c] = -g * (v - bias[c]) * e;
        } else {
            const float e = expf(logs[c]);
            dx[r * 3 + c] = g * e;
            gbias[r * 3 + c] = g;
            glogs[r * 3 + c] = g * v * e;
        }
    }
}

// forward direction: h2 = y[td:] - o ; v = reverse(cat[h1,h2]) ; out = (v - t) * exp(-s)
__global__ __launch_bounds__(256) void couple_inject_fwd_kernel(const float* __restrict__ y, const float* __restrict__ o,
                                                               const float* __restrict__ s, const float* __restrict__ t,
                                                               int td, long long R, float* __restrict__ out) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    float h[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) h[c] = y[r * 3 + c] - (c >= td ? o[r * (3 - td) + (c - td)] : 0.f);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[r * 3 + c] = (h[2 - c] - t[r * 3 + c]) * expf(-s[r * 3 + c]);
}
__global__ __launch_bounds__(256) void couple_inject_bwd_kernel(const float* __restrict__ out, const float* __restrict__ dout,
                                                               const float* __restrict__ s, int td, long long R,
                                                               float* __restrict__ dy, float* __restrict__ dobuf,
                                                               float* __restrict__ ds, float* __restrict__ dt) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    float dv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float g = dout[r * 3 + c];
        dv[c] = g * expf(-s[r * 3 + c]);
        ds[r * 3 + c] = -g * out[r * 3 + c];
        dt[r * 3 + c] = -dv[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float g = dv[2 - c];                       // un-reverse
        dy[r * 3 + c] = g;
        if (c >= td) dobuf[r * (3 - td) + (c - td)] = -g;
    }
}

// inverse direction, first half: v = reverse(u * exp(s) + t)
__global__ __launch_bounds__(256) void inject_inv_fwd_kernel(const float* __restrict__ u, const float* __restrict__ s,
                                                            const float* __restrict__ t, long long R, float* __restrict__ v) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[r * 3 + (2 - c)] = fmaf(u[r * 3 + c], expf(s[r * 3 + c]), t[r * 3 + c]);
}
__global__ __launch_bounds__(256) void inject_inv_bwd_kernel(const float* __restrict__ u, const float* __restrict__ s,
                                                            const float* __restrict__ dv, long long R, float* __restrict__ du,
                                                            float* __restrict__ ds, float* __restrict__ dt) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float g = dv[r * 3 + (2 - c)], e = expf(s[r * 3 + c]);
        du[r * 3 + c] = g * e;
        ds[r * 3 + c] = g * u[r * 3 + c] * e;
        dt[r * 3 + c] = g;
    }
}
// inverse direction, second half: out = cat[v[:td], v[td:] + o]   (backward: dv = dout, do = dout[td:])
__global__ __launch_bounds__(256) void couple_add_kernel(const float* __restrict__ v, const float* __restrict__ o, int td,
                                                        long long R, float* __restrict__ out) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[r * 3 + c] = v[r * 3 + c] + (c >= td ? o[r * (3 - td) + (c - td)] : 0.f);
}
__global__ __launch_bounds__(256) void slice_tail_kernel(const float* __restrict__ g, int td, long long R, float* __restrict__ o) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    for (int c = td; c < 3; ++c) o[r * (3 - td) + (c - td)] = g[r * 3 + c];
}

// per-batch sums over M consecutive values: out[b] = sum_m f(x[b*M + m]);  mode 0: x, mode 1: -0.5*(x^2 + log 2 pi)
__global__ __launch_bounds__(256) void batch_sum_kernel(const float* __restrict__ x, long long M, int mode, float* __restrict__ out) {
    __shared__ float sh[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    float acc = 0.f;
    for (long long m = tid; m < M; m += 256) {
        const float v = x[(long long)b * M + m];
        acc += mode == 0 ? v : -0.5f * (v * v + 1.8378770664093453f);
    }
    sh[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    if (tid == 0) out[b] = sh[0];
}
// dx[b*M + m] = g[b] * (mode 0: 1, mode 1: -x)
__global__ __launch_bounds__(256) void batch_sum_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, long long M,
                                                           int mode, long long total, float* __restrict__ dx) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const float gg = g[i / M];
        dx[i] = mode == 0 ? gg : -gg * x[i];
    }
}

inline unsigned rows_grid(long long R) { return (unsigned)((R + 255) / 256); }

}  // namespace

extern "C" int pf_actnorm_fwd(const float* x, const float* logs, const float* bias, int inv, long long R, float* y, void* stream) {
    if (!x || !logs || !bias || !y) return PF_ERR_NULL;
    if (R <= 0) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(actnorm_fwd_kernel, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, x, logs, bias, inv, R, y);
    return pf_last_launch_status();
}
extern "C" int pf_actnorm_bwd(const float* x, const float* dy, const float* logs, const float* bias, int inv, long long R,
                              float* dx, float* glogs_rows, float* gbias_rows, void* stream) {
    if (!x || !dy || !logs || !bias || !dx || !glogs_rows || !gbias_rows) return PF_ERR_NULL;
    if (R <= 0) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(actnorm_bwd_kernel, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, x, dy, logs, bias, inv, R, dx,
                       glogs_rows, gbias_rows);
    return pf_last_launch_status();
}
extern "C" int pf_couple_inject_fwd(const float* y, const float* o, const float* s, const float* t, int td, long long R,
                                    float* out, void* stream) {
    if (!y || !o || !s || !t || !out) return PF_ERR_NULL;
    if (R <= 0 || td < 1 || td > 2) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(couple_inject_fwd_kernel, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, y, o, s, t, td, R, out);
    return pf_last_launch_status();
}
extern "C" int pf_couple_inject_bwd(const float* out, const float* dout, const float* s, int td, long long R, float* dy,
                                    float* do_, float* ds, float* dt, void* stream) {
    if (!out || !dout || !s || !dy || !do_ || !ds || !dt) return PF_ERR_NULL;
    if (R <= 0 || td < 1 || td > 2) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(couple_inject_bwd_kernel, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, out, dout, s, td, R, dy,
                       do_, ds, dt);
    return pf_last_launch_status();
}
extern "C" int pf_inject_inv_fwd(const float* u, const float* s, const float* t, long long R, float* v, void* stream) {
    if (!u || !s || !t || !v) return PF_ERR_NULL;
    if (R <= 0) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(inject_inv_fwd_kernel, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, u, s, t, R, v);
    return pf_last_launch_status();
}
extern "C" int pf_inject_inv_bwd(const float* u, const float* s, const float* dv, long long R, float* du, float* ds, float* dt,
                                 void* stream) {
    if (!u || !s || !dv || !du || !ds || !dt) return PF_ERR_NULL;
    if (R <= 0) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(inject_inv_bwd_kernel, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, u, s, dv, R, du, ds, dt);
    return pf_last_launch_status();
}
extern "C" int pf_couple_add(const float* v, const float* o, int td, long long R, float* out, void* stream) {
    if (!v || !o || !out) return PF_ERR_NULL;
    if (R <= 0 || td < 1 || td > 2) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(couple_add_kernel, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, v, o, td, R, out);
    return pf_last_launch_status();
}
extern "C" int pf_slice_tail(const float* g, int td, long long R, float* o, void* stream) {
    if (!g || !o) return PF_ERR_NULL;
    if (R <= 0 || td < 1 || td > 2) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(slice_tail_kernel, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, g, td, R, o);
    return pf_last_launch_status();
}
extern "C" int pf_batch_sum_fwd(const float* x, int B, long long M, int mode, float* out, void* stream) {
    if (!x || !out) return PF_ERR_NULL;
    if (B <= 0 || M <= 0) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(batch_sum_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, M, mode, out);
    return pf_last_launch_status();
}
extern "C" int pf_batch_sum_bwd(const float* x, const float* g, int B, long long M, int mode, float* dx, void* stream) {
    if (!x || !g || !dx) return PF_ERR_NULL;
    if (B <= 0 || M <= 0) return PF_ERR_SHAPE;
    const long long total = (long long)B * M;
    hipLaunchKernelGGL(batch_sum_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, g, M, mode, total, dx);
    return pf_last_launch_status();
}

// DistanceEncoder.distance_vec (interpflow.py:100-115): out [B*N*K, 10] = [x_i, x_j, x_i - x_j, |x_i - x_j|] (inputs only: no backward)
namespace {
__global__ __launch_bounds__(256) void dist_feature_kernel(const float* __restrict__ xyz, const int* __restrict__ idx, int N, int K,
                                                          long long E, float* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const long long t = e / K;
    const long long j = (t / N) * N + idx[e];
    float* o = out + e * 10;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = xyz[t * 3 + c], b = xyz[j * 3 + c];
        o[c] = a; o[3 + c] = b; v[c] = __fsub_rn(a, b); o[6 + c] = v[c];
    }
    o[9] = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(v[0], v[0]), __fmul_rn(v[1], v[1])), __fmul_rn(v[2], v[2])));
}
}  // namespace

extern "C" int pf_dist_feature(const float* xyz, const int* idx, int B, int N, int K, float* out, void* stream) {
    if (!xyz || !idx || !out) return PF_ERR_NULL;
    if (B <= 0 || N <= 0 || K <= 0) return PF_ERR_SHAPE;
    const long long E = (long long)B * N * K;
    hipLaunchKernelGGL(dist_feature_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, (hipStream_t)stream, xyz, idx, N, K, E, out);
    return pf_last_launch_status();
}
