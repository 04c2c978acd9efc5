// Tiled passes over large clouds (puflow_amd/tiles.py; the reference has no counterpart): the two geometric
// queries the orchestration needs on the device.
//   pf_box_count / _fill - the points inside axis-aligned boxes: counts, then a CSR of ascending point indices per box (the
//                          two-pass pattern of pf_disk_count / pf_disk_fill: order from wave ballots and prefix counts, no atomics).
//                          Used for a tile's halo (the cloud against the tiles' grown cells) and for a tile's context (the
//                          samples already selected against the same kind of box).
//   pf_kd_assign         - the leaf of every point in a complete k-d tree given as arrays, by descent.
// All stores are plain vector stores.
#include <hip/hip_runtime.h>
#include "pf_api_internal.h"

namespace {

constexpr int BX_T = 256, BX_W = BX_T / 64;

// lo <= p <= hi on every axis (faces included; +-inf faces never exclude; a NaN coordinate is in no box)
__device__ __forceinline__ bool in_box(const float* __restrict__ pts, int i, const float (&b)[6]) {
    const float x = pts[(size_t)i * 3], y = pts[(size_t)i * 3 + 1], z = pts[(size_t)i * 3 + 2];
    return x >= b[0] && y >= b[1] && z >= b[2] && x <= b[3] && y <= b[4] && z <= b[5];
}

__global__ __launch_bounds__(BX_T) void box_count_kernel(const float* __restrict__ pts, int M, const float* __restrict__ boxes,
                                                         int* __restrict__ counts) {
    __shared__ int wcnt[BX_W];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float b[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) b[c] = boxes[(size_t)t * 6 + c];
    int cnt = 0;
    for (int i0 = 0; i0 < M; i0 += BX_T) {       // uniform trip count: the ballots see whole waves
        const int i = i0 + tid;
        cnt += __popcll(__ballot(i < M && in_box(pts, i, b)));
    }
    if (lane == 0) wcnt[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
        int c = 0;
        for (int w = 0; w < BX_W; ++w) c += wcnt[w];
        counts[t] = c;
    }
}

__global__ __launch_bounds__(BX_T) void box_fill_kernel(const float* __restrict__ pts, int M, const float* __restrict__ boxes,
                                                        const long long* __restrict__ offsets, int* __restrict__ member) {
    __shared__ int wsum[BX_W];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float b[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) b[c] = boxes[(size_t)t * 6 + c];
    const long long row = offsets[t], cap = offsets[t + 1] - row;        // a row too short for its box is filled, not overrun
    long long base = 0;
    for (int i0 = 0; i0 < M; i0 += BX_T) {
        const int i = i0 + tid;
        const bool in = i < M && in_box(pts, i, b);
        const unsigned long long m = __ballot(in);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < BX_W; ++w) { const int v = wsum[w]; off += w < wave ? v : 0; tot += v; }
        const long long rank = base + off + __popcll(m & ((1ull << lane) - 1ull));
        if (in && rank < cap) member[row + rank] = i;
        base += tot;
        __syncthreads();
    }
}

// complete tree of depth L in heap order: inner node k has the children 2k + 1 (left) and 2k + 2 (right), the leaves are the
// nodes 2^L - 1 .. 2^(L+1) - 2; a point goes right iff p[axis] >= split
__global__ __launch_bounds__(256) void kd_assign_kernel(const float* __restrict__ pts, int M, const int* __restrict__ axis,
                                                        const float* __restrict__ split, int L, int* __restrict__ leaf) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const float p[3] = {pts[(size_t)i * 3], pts[(size_t)i * 3 + 1], pts[(size_t)i * 3 + 2]};
    int k = 0;
    for (int l = 0; l < L; ++l) {
        const int a = axis[k];
        const float v = a == 0 ? p[0] : (a == 1 ? p[1] : p[2]);          // an axis outside 0..2 reads z, never out of bounds
        k = 2 * k + 1 + (v >= split[k] ? 1 : 0);
    }
    leaf[i] = k - ((1 << L) - 1);
}

}  // namespace

extern "C" int pf_box_count(const float* pts, int M, const float* boxes, int T, int* counts, void* stream) {
    if (!pts || !boxes || !counts) return PF_ERR_NULL;
    if (M <= 0 || T <= 0 || (long long)M * 3 > 0x7fffffffll) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(box_count_kernel, dim3(T), dim3(BX_T), 0, (hipStream_t)stream, pts, M, boxes, counts);
    return pf_last_launch_status();
}

extern "C" int pf_box_fill(const float* pts, int M, const float* boxes, int T, const long long* offsets, int* member,
                           void* stream) {
    if (!pts || !boxes || !offsets || !member) return PF_ERR_NULL;
    if (M <= 0 || T <= 0 || (long long)M * 3 > 0x7fffffffll) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(box_fill_kernel, dim3(T), dim3(BX_T), 0, (hipStream_t)stream, pts, M, boxes, offsets, member);
    return pf_last_launch_status();
}

extern "C" int pf_kd_assign(const float* pts, int M, const int* axis, const float* split, int L, int* leaf, void* stream) {
    if (!pts || !leaf || (L > 0 && (!axis || !split))) return PF_ERR_NULL;
    if (M <= 0 || L < 0 || L > 24 || (long long)M * 3 > 0x7fffffffll) return PF_ERR_SHAPE;
    hipLaunchKernelGGL(kd_assign_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, pts, M, axis, split, L, leaf);
    return pf_last_launch_status();
}
