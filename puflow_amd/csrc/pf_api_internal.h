// Internal glue for the C-ABI entry points (error codes mirror include/puflow_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/puflow_hip.h"
#include "pf_grid.h"      // PF_INTERNAL: host helpers that cross source files without being part of the C ABI

static inline int pf_last_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? PF_OK : PF_ERR_LAUNCH;
}

// ---- weight gradients beside the backward chain (pf_train_set_dw_stream, csrc/api.hip) ------------------------------------
// A backward entry point produces two kinds of results: the gradient wrt its INPUT, which the layer before it waits for, and
// the gradients wrt its WEIGHTS, which nobody reads before the optimizer.  With a weight-gradient stream set (per host thread)
// the split-K weight-gradient kernels and their reductions are enqueued there, after an event that orders them behind what
// the calling stream holds at that point; the caller joins the stream once, before the optimizer (puflow_amd/train_ops.py does
// it at the end of the autograd pass).  Inside a hipGraph capture the event becomes an edge: a parallel branch of the graph.
PF_INTERNAL void* pf_dw_stream_get();
// the stream weight-gradient work of a call should go to: s itself when none is set (or it IS s), else the weight-gradient stream,
// made to wait for everything enqueued on s so far
PF_INTERNAL hipStream_t pf_dw_fork(hipStream_t s);
// pf_gemm_ex with an addend: C = A B + bias + addend (addend [M, ldc] laid out like C, nullable, may alias C) - csrc/train_gemm.hip
// slabs_left: nullable; when given and the product is split over K, the slabs stay in ws ([n][M, N], *slabs_left = n, no reduction
// launch: the caller sums them where it reads the result) - else *slabs_left = 0 and C holds the product
PF_INTERNAL int pf_gemm_addend(int arith, const float* A, long long sam, long long sak, const float* B, long long sbk, long long sbn,
                               float* C, long long ldc, const float* bias, const float* addend, int M, int N, int K, float* ws,
                               long long ws_floats, void* stream, int* slabs_left);
