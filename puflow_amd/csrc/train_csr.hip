// Transposed neighbour lists of the kNN graph (in-edges per point): the dPQ gather of the EdgeConv backward (train_fused.hip),
// the glue kernels and the deterministic mode sum over them instead of scattering with atomics.
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"
#include "pf_mfma.h"

namespace {

__global__ __launch_bounds__(256) void ec_zero_kernel(f4* p, long long n4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) p[i] = pf_splat(0.f);
}

// transposed neighbour lists of idx [T, K] (batch-local indices, N points per sample): count -> scan -> fill
__global__ __launch_bounds__(256) void csr_count_kernel(const int* idx, int N, int K, long long E, int* cnt) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
        const long long i = e / K;
        atomicAdd(cnt + (i / N) * N + idx[e], 1);
    }
}
// exclusive scan of cnt[T] -> off[T+1] by ONE workgroup of 1024 threads (T <= a few 100 k); cnt is left as the running fill cursor
__global__ __launch_bounds__(1024) void csr_scan_kernel(int* cnt, int T, int* off) {
    __shared__ int part[1024];
    const int per = (T + 1023) / 1024;
    const int lo = threadIdx.x * per, hi = min(T, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += cnt[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int i = lo; i < hi; ++i) { const int c = cnt[i]; off[i] = run; cnt[i] = run; run += c; }
    if (threadIdx.x == 1023) off[T] = part[1023];
}
__global__ __launch_bounds__(256) void csr_fill_kernel(const int* idx, int N, int K, long long E, int* cursor, int* edge) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
        const long long i = e / K;
        edge[atomicAdd(cursor + (i / N) * N + idx[e], 1)] = (int)e;
    }
}
// Two lists from one pass over idx [T, K]: all K columns (cnt / edge ids i K + k) and the first K2 columns (cnt2 / edge ids
// i K2 + k: what pf_knn_csr gives for idx[:, :K2] stored contiguously) - the training step needs both (K = 16: feature units,
// K2 = 8: the interpolation unit), and each launch here is a few microseconds of work behind a launch of its own.
__global__ __launch_bounds__(256) void csr_count2_kernel(const int* idx, int N, int K, int K2, long long E, int* cnt, int* cnt2) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
        const long long i = e / K;
        const long long j = (i / N) * N + idx[e];
        atomicAdd(cnt + j, 1);
        if ((int)(e - i * K) < K2) atomicAdd(cnt2 + j, 1);
    }
}
__global__ __launch_bounds__(1024) void csr_scan2_kernel(int* cnt, int T, int Tpad, int* off, int* off2) {
    __shared__ int part[1024];
    if (blockIdx.x) { cnt += Tpad; off = off2; }
    const int per = (T + 1023) / 1024;
    const int lo = threadIdx.x * per, hi = min(T, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += cnt[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int i = lo; i < hi; ++i) { const int c = cnt[i]; off[i] = run; cnt[i] = run; run += c; }
    if (threadIdx.x == 1023) off[T] = part[1023];
}
__global__ __launch_bounds__(256) void csr_fill2_kernel(const int* idx, int N, int K, int K2, long long E, int* cursor, int* cursor2,
                                                        int* edge, int* edge2) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
        const long long i = e / K;
        const long long j = (i / N) * N + idx[e];
        const int k = (int)(e - i * K);
        edge[atomicAdd(cursor + j, 1)] = (int)e;
        if (k < K2) edge2[atomicAdd(cursor2 + j, 1)] = (int)(i * K2 + k);
    }
}
// the fill above hands out a list's slots in arrival order: sort every list (edge ids ascending) so that whatever is summed over it
// - the dQ gather of the EdgeConv backward, the latent's gradient, the Chamfer gradient - adds in ONE order, run after run
__global__ __launch_bounds__(256) void csr_sort_kernel(const int* __restrict__ off, int* __restrict__ edge, int T) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= T) return;
    const int lo = off[j], hi = off[j + 1];
    for (int a = lo + 1; a < hi; ++a) {
        const int v = edge[a];
        int b = a - 1;
        while (b >= lo && edge[b] > v) { edge[b + 1] = edge[b]; --b; }
        edge[b + 1] = v;
    }
}

}  // namespace

// transposed neighbour lists: off [T+1], edge [T*K] (edge ids e = i K + k grouped by the point they point AT), cnt [T] scratch.
// Built once per step and shared by every unit that uses the same idx (pf_ec_train_bwd: csr_off / csr_edge).
extern "C" int pf_knn_csr(const int* idx, int B, int N, int K, int* off, int* edge, int* cnt, void* stream) {
    if (!idx || !off || !edge || !cnt) return PF_ERR_NULL;
    if (B <= 0 || N <= 0 || K <= 0 || (long long)B * N > (1ll << 26)) return PF_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    const int T = B * N;
    const long long E = (long long)T * K;
    const unsigned g = (unsigned)((E + 255) / 256 > 2048 ? 2048 : (E + 255) / 256);
    hipLaunchKernelGGL(ec_zero_kernel, dim3(64), dim3(256), 0, s, reinterpret_cast<f4*>(cnt), (long long)(T + 3) / 4);
    hipLaunchKernelGGL(csr_count_kernel, dim3(g), dim3(256), 0, s, idx, N, K, E, cnt);
    hipLaunchKernelGGL(csr_scan_kernel, dim3(1), dim3(1024), 0, s, cnt, T, off);
    hipLaunchKernelGGL(csr_fill_kernel, dim3(g), dim3(256), 0, s, idx, N, K, E, cnt, edge);
    return pf_last_launch_status();
}

// pf_knn_csr for idx [B*N, K] AND for its first K2 columns (as if stored contiguously: edge ids i K2 + k) in the same four
// launches: off / edge as above, off2 [T+1], edge2 [T*K2]; cnt: 2 x ((T + 3) / 4 * 4) ints of scratch.
extern "C" int pf_knn_csr_pair(const int* idx, int B, int N, int K, int K2, int* off, int* edge, int* off2, int* edge2, int* cnt,
                               void* stream) {
    if (!idx || !off || !edge || !off2 || !edge2 || !cnt) return PF_ERR_NULL;
    if (B <= 0 || N <= 0 || K <= 0 || K2 <= 0 || K2 > K || (long long)B * N > (1ll << 26)) return PF_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    const int T = B * N, Tpad = (T + 3) / 4 * 4;
    const long long E = (long long)T * K;
    const unsigned g = (unsigned)((E + 255) / 256 > 2048 ? 2048 : (E + 255) / 256);
    hipLaunchKernelGGL(ec_zero_kernel, dim3(64), dim3(256), 0, s, reinterpret_cast<f4*>(cnt), (long long)(2 * Tpad) / 4);
    hipLaunchKernelGGL(csr_count2_kernel, dim3(g), dim3(256), 0, s, idx, N, K, K2, E, cnt, cnt + Tpad);
    hipLaunchKernelGGL(csr_scan2_kernel, dim3(2), dim3(1024), 0, s, cnt, T, Tpad, off, off2);
    hipLaunchKernelGGL(csr_fill2_kernel, dim3(g), dim3(256), 0, s, idx, N, K, K2, E, cnt, cnt + Tpad, edge, edge2);
    return pf_last_launch_status();
}

// Sorts every list of pf_knn_csr (edge ids ascending).  The fill hands out a list's slots in arrival order; whatever is summed over
// a sorted list adds in ONE order, run after run (PF_TRAIN_DETERMINISTIC: the gather-form gradients).  Not needed otherwise.
extern "C" int pf_knn_csr_sort(const int* off, int* edge, int T, void* stream) {
    if (!off || !edge) return PF_ERR_NULL;
    if (T <= 0) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(csr_sort_kernel, dim3((T + 255) / 256), dim3(256), 0, (hipStream_t)stream, off, edge, T);
    return pf_last_launch_status();
}
