#!/usr/bin/env python3
"""GPU box: what the generic GEMM (csrc/train_gemm.hip) computes, as SHA-256 of the output bytes: pf_gemm_ex with arithmetic 0
(f32 MFMA: gemm2_kernel, or gemm_kernel where an operand takes no float4 loads), 1 (gemm_kernel whatever the operands), 2 (split-fp16)
and 3 (split-bf16) on the 15 shapes of tests/test_gpu_train_fused.py - every tile shape, split-K slabs with the reduce, ragged
tiles, odd strides - with that test's operands (same seeds), the output prefilled with NaN.  One line per shape: the workspace
size pf_gemm_ws_floats asks for and the four hashes; columns 0 and 1 are equal.
C ABI only, so the same file runs against two trees: `gemm_fingerprint.py [DIR]`, DIR = the directory that holds the other
tree's `puflow_amd` (default: this repository).  Identical text = same bits."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from puflow_amd import _lib

SHAPES = [  # M, N, K, A contiguous along k, B contiguous along n, bias
    (8192, 512, 128, True, False, True), (8192, 128, 512, True, True, False), (512, 128, 8192, False, True, False),
    (8192, 128, 64, True, False, True), (8192, 64, 32, True, True, False), (8192, 16, 128, True, False, True),
    (8192, 32, 64, True, True, False), (16, 256, 8192, False, True, False), (64, 128, 8192, False, False, False),
    (1000, 72, 100, True, False, True), (260, 260, 36, False, True, True), (4096, 512, 512, True, False, False),
    (67, 33, 45, True, False, True), (33, 70, 50, True, True, True), (130, 20, 1030, False, True, False)]

lib = _lib.load()
for M, N, K, a_kfast, b_nfast, bias in SHAPES:
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K)
    A = torch.randn((M, K) if a_kfast else (K, M), generator=g).cuda()
    Bm = torch.randn((K, N) if b_nfast else (N, K), generator=g).cuda()
    b = torch.randn(N, generator=g).cuda() if bias else None
    sam, sak = (K, 1) if a_kfast else (1, M)
    sbk, sbn = (N, 1) if b_nfast else (1, K)
    need = lib.pf_gemm_ws_floats(M, N, K)
    ws = torch.empty(max(need, 1), device="cuda")
    row = f"[{M} x {N} x {K}] a_kfast {int(a_kfast)} b_nfast {int(b_nfast)} bias {int(bias)} ws_floats {need}"
    for arith in (0, 1, 2, 3):
        C = torch.full((M, N), float("nan"), device="cuda")
        _lib.check(lib.pf_gemm_ex(arith, A.data_ptr(), sam, sak, Bm.data_ptr(), sbk, sbn, C.data_ptr(), N, b.data_ptr() if bias else None,
                                  M, N, K, ws.data_ptr(), need, None), "pf_gemm_ex")
        torch.cuda.synchronize()
        row += f"\n  arith {arith} sha256 {hashlib.sha256(C.cpu().numpy().tobytes()).hexdigest()}"
    print(row, flush=True)
