"""The per-op reference tier of the training step: one kernel pair per eager op of the reference (csrc/train_ops.hip; the GEMM:
csrc/train_gemm.hip), wired into autograd.  The fused tiers (train_fusedfn) are tested against it; RepeatRowsFn, GatherRowsFn, SoftmaxWsumFn and BatchSumFn
also serve the default path.  Reads no switch of train_ops (PF_TRAIN_GEMM is its own).  Activations are channels-last [rows, C] fp32."""
from __future__ import annotations

import os

import torch
from torch import Tensor
from torch.autograd import Function

from . import _lib
from .train_state import _ptr, _stream, _sync_bn_active, _ws, deterministic


# Matrix-pipe arithmetic of the training GEMMs: "f32" (default) = every GEMM on the f32 MFMA (bit-exact fp32 fma chains);
# "split" = forward GEMMs as split-fp16 products (3 fp16 MFMAs per 32-deep step), GEMMs with a gradient operand as
# split-bf16 (6 bf16 MFMAs, fp32 exponent range) - csrc/train_gemm.hip gemm_split_kernel.  Measured at 32 x (256 -> 1024):
# the same step time (the layer GEMMs of this un-fused path are bound by staging and launch count, not by the MFMA rate:
# profiles/r2_train), so the exact arithmetic stays the default; the gradient tests pass in both modes.
_GEMM_MODE = os.environ.get("PF_TRAIN_GEMM", "f32")
ARITH_FWD, ARITH_BWD = (2, 3) if _GEMM_MODE == "split" else (0, 0)


def _gemm(A: Tensor, sam: int, sak: int, Bm: Tensor, sbk: int, sbn: int, C: Tensor, ldc: int, bias, M: int, N: int, K: int,
          arith: int = 0):
    lib = _lib.load()
    need = lib.pf_gemm_ws_floats(M, N, K)
    ws = _ws(C.device, need) if need else None
    _lib.check(lib.pf_gemm_ex(arith, A.data_ptr(), sam, sak, Bm.data_ptr(), sbk, sbn, C.data_ptr(), ldc, _ptr(bias), M, N, K,
                              _ptr(ws), need, _stream()), "pf_gemm")


class LinearFn(Function):
    """y[R,Cout] = x[R,Cin] W[Cout,Cin]^T + b   (nn.Linear / Conv2d 1x1 on channels-last rows)."""

    @staticmethod
    def forward(ctx, x, W, b):
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).contiguous()
        W = W.contiguous()
        R, Cin = x2.shape
        Cout = W.shape[0]
        y = torch.empty((R, Cout), dtype=torch.float32, device=x.device)
        _gemm(x2, Cin, 1, W, 1, Cin, y, Cout, b, R, Cout, Cin, ARITH_FWD)
        ctx.save_for_backward(x2, W)
        ctx.has_bias = b is not None
        ctx.shp = shp
        return y.view(*shp[:-1], Cout)

    @staticmethod
    def backward(ctx, dy):
        x2, W = ctx.saved_tensors
        R, Cin = x2.shape
        Cout = W.shape[0]
        dy2 = dy.reshape(R, Cout).contiguous()
        dx = dW = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x2)
            _gemm(dy2, Cout, 1, W, Cin, 1, dx, Cin, None, R, Cin, Cout, ARITH_BWD)
            dx = dx.view(ctx.shp)
        if ctx.needs_input_grad[1]:
            dW = torch.empty_like(W)
            _gemm(dy2, 1, Cout, x2, Cin, 1, dW, Cin, None, Cout, Cin, R, ARITH_BWD)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            lib = _lib.load()
            db = torch.empty((Cout,), dtype=torch.float32, device=dy.device)
            ws = _ws(dy.device, 2 * lib.pf_bn_chunks(R) * Cout)
            _lib.check(lib.pf_colsum(dy2.data_ptr(), R, Cout, db.data_ptr(), ws.data_ptr(), _stream()), "pf_colsum")
        return dx, dW, db


def linear(x: Tensor, W: Tensor, b=None) -> Tensor:
    return LinearFn.apply(x, W.reshape(W.shape[0], -1), b)


class BnLreluFn(Function):
    """BatchNorm(training, batch statistics over rows) + LeakyReLU; running stats updated in place."""

    @staticmethod
    def forward(ctx, x, gamma, beta, run_mean, run_var, slope, eps, momentum):
        lib = _lib.load()
        x = x.contiguous()
        R, C = x.shape
        y = torch.empty_like(x)
        save = torch.empty((2, C), dtype=torch.float32, device=x.device)
        ws = _ws(x.device, (2 * lib.pf_bn_chunks(R) + 2) * C)
        g, b = gamma.contiguous(), beta.contiguous()
        _lib.check(lib.pf_bn_lrelu_fwd(x.data_ptr(), R, C, g.data_ptr(), b.data_ptr(), slope, eps, momentum, _ptr(run_mean),
                                       _ptr(run_var), y.data_ptr(), save.data_ptr(), ws.data_ptr(), _stream()), "pf_bn_lrelu_fwd")
        ctx.save_for_backward(x, g, b, save)
        ctx.slope = slope
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, g, b, save = ctx.saved_tensors
        R, C = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dg = torch.empty((C,), dtype=torch.float32, device=x.device)
        db = torch.empty((C,), dtype=torch.float32, device=x.device)
        ws = _ws(x.device, (2 * lib.pf_bn_chunks(R) + 2) * C)
        _lib.check(lib.pf_bn_lrelu_bwd(x.data_ptr(), dy.data_ptr(), R, C, g.data_ptr(), b.data_ptr(), ctx.slope,
                                       save.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                       _stream()), "pf_bn_lrelu_bwd")
        return dx, dg, db, None, None, None, None, None


class SyncBnLreluFn(Function):
    """BnLreluFn with statistics over the GLOBAL batch (all ranks): the per-column sums are all-reduced between the
    kernel stages - 2 small all-reduces forward (mean, then centred variance: the same two-pass scheme as the local
    kernel), 1 backward.  dgamma / dbeta stay the LOCAL sums (the gradient bucket's mean over ranks then gives the
    gradient of the averaged loss, as with torch.nn.SyncBatchNorm under DDP); dx uses the global means."""

    @staticmethod
    def forward(ctx, x, gamma, beta, run_mean, run_var, slope, eps, momentum):
        import torch.distributed as dist
        lib = _lib.load()
        x = x.contiguous()
        R, C = x.shape
        dev = x.device
        ws = _ws(dev, 2 * lib.pf_bn_chunks(R) * C)
        g, b = gamma.contiguous(), beta.contiguous()
        stat = torch.empty((C + 1,), dtype=torch.float32, device=dev)
        _lib.check(lib.pf_bn_colstat(x.data_ptr(), R, C, None, stat.data_ptr(), ws.data_ptr(), _stream()), "pf_bn_colstat")
        stat[C] = float(R)
        dist.all_reduce(stat)
        Rg = float(stat[C].item())
        mean = (stat[:C] / Rg).contiguous()
        var = torch.empty((C,), dtype=torch.float32, device=dev)
        _lib.check(lib.pf_bn_colstat(x.data_ptr(), R, C, mean.data_ptr(), var.data_ptr(), ws.data_ptr(), _stream()), "pf_bn_colstat")
        dist.all_reduce(var)
        var = (var / Rg).contiguous()
        y = torch.empty_like(x)
        save = torch.empty((2, C), dtype=torch.float32, device=dev)
        _lib.check(lib.pf_bn_apply_stats(x.data_ptr(), R, C, mean.data_ptr(), var.data_ptr(), Rg / max(Rg - 1.0, 1.0),
                                         g.data_ptr(), b.data_ptr(), slope, eps, momentum, _ptr(run_mean), _ptr(run_var),
                                         y.data_ptr(), save.data_ptr(), _stream()), "pf_bn_apply_stats")
        ctx.save_for_backward(x, g, b, save)
        ctx.slope, ctx.Rg = slope, Rg
        return y

    @staticmethod
    def backward(ctx, dy):
        import torch.distributed as dist
        lib = _lib.load()
        x, g, b, save = ctx.saved_tensors
        R, C = x.shape
        dy = dy.contiguous()
        ws = _ws(x.device, 2 * lib.pf_bn_chunks(R) * C)
        sums = torch.empty((2, C), dtype=torch.float32, device=x.device)
        _lib.check(lib.pf_bn_bwd_sums(x.data_ptr(), dy.data_ptr(), R, C, g.data_ptr(), b.data_ptr(), ctx.slope, save.data_ptr(),
                                      sums.data_ptr(), ws.data_ptr(), _stream()), "pf_bn_bwd_sums")
        db, dg = sums[0].clone(), sums[1].clone()
        dist.all_reduce(sums)
        means = (sums / ctx.Rg).contiguous()
        dx = torch.empty_like(x)
        _lib.check(lib.pf_bn_bwd_apply(x.data_ptr(), dy.data_ptr(), R, C, g.data_ptr(), b.data_ptr(), ctx.slope, save.data_ptr(),
                                       means.data_ptr(), dx.data_ptr(), _stream()), "pf_bn_bwd_apply")
        return dx, dg, db, None, None, None, None, None


def bn_lrelu(x: Tensor, bn: torch.nn.BatchNorm2d, slope: float) -> Tensor:
    fn = SyncBnLreluFn if _sync_bn_active() else BnLreluFn
    y = fn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, slope, bn.eps, bn.momentum)
    with torch.no_grad():
        bn.num_batches_tracked += 1
    return y


class ActFn(Function):
    @staticmethod
    def forward(ctx, x, slope):
        lib = _lib.load()
        x = x.contiguous()
        y = torch.empty_like(x)
        _lib.check(lib.pf_act_fwd(x.data_ptr(), slope, x.numel(), y.data_ptr(), _stream()), "pf_act_fwd")
        ctx.save_for_backward(y)
        ctx.slope = slope
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(y)
        _lib.check(lib.pf_act_bwd(y.data_ptr(), dy.data_ptr(), ctx.slope, y.numel(), dx.data_ptr(), _stream()), "pf_act_bwd")
        return dx, None


class EdgeFeatureFn(Function):
    """x [B,N,C], idx int32 [B,N,K] -> [B*N*K, 3C] = [x_i, x_j, x_j - x_i]."""

    @staticmethod
    def forward(ctx, x, idx):
        lib = _lib.load()
        x = x.contiguous()
        B, N, C = x.shape
        K = idx.shape[-1]
        out = torch.empty((B * N * K, 3 * C), dtype=torch.float32, device=x.device)
        _lib.check(lib.pf_edge_feature_fwd(x.data_ptr(), idx.data_ptr(), B, N, K, C, out.data_ptr(), _stream()), "pf_edge_feature_fwd")
        ctx.save_for_backward(idx)
        ctx.dims = (B, N, K, C)
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        lib = _lib.load()
        (idx,) = ctx.saved_tensors
        B, N, K, C = ctx.dims
        g = g.contiguous()
        dx = torch.zeros((B, N, C), dtype=torch.float32, device=g.device)
        _lib.check(lib.pf_edge_feature_bwd(g.data_ptr(), idx.data_ptr(), B, N, K, C, dx.data_ptr(), _stream()), "pf_edge_feature_bwd")
        return dx, None


class MaxPoolKFn(Function):
    """y [T*K, C] -> max over the K rows of each point [T, C]."""

    @staticmethod
    def forward(ctx, y, K):
        lib = _lib.load()
        y = y.contiguous()
        C = y.shape[1]
        T = y.shape[0] // K
        out = torch.empty((T, C), dtype=torch.float32, device=y.device)
        arg = torch.empty((T, C), dtype=torch.int32, device=y.device)
        _lib.check(lib.pf_maxpool_k_fwd(y.data_ptr(), T, K, C, out.data_ptr(), arg.data_ptr(), _stream()), "pf_maxpool_k_fwd")
        ctx.save_for_backward(arg)
        ctx.dims = (T, K, C)
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (arg,) = ctx.saved_tensors
        T, K, C = ctx.dims
        dy = dy.contiguous()
        dx = torch.empty((T * K, C), dtype=torch.float32, device=dy.device)
        _lib.check(lib.pf_maxpool_k_bwd(dy.data_ptr(), arg.data_ptr(), T, K, C, dx.data_ptr(), _stream()), "pf_maxpool_k_bwd")
        return dx, None


def knn_csr(idx: Tensor):
    """Transposed neighbour lists of idx [B,N,K] int32 (batch-local): (off [T+1], edge [T*K]) - for every point the edges that
    point AT it.  Built once per step (4 small launches) and shared by all EdgeConv units on the same idx: their backward then
    gathers dQ instead of scatter-adding it with float atomics."""
    B, N, K = idx.shape
    T = B * N
    dev = idx.device
    off = torch.empty(T + 1, dtype=torch.int32, device=dev)
    edge = torch.empty(T * K, dtype=torch.int32, device=dev)
    cnt = torch.empty((T + 3) // 4 * 4, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().pf_knn_csr(idx.data_ptr(), B, N, K, off.data_ptr(), edge.data_ptr(), cnt.data_ptr(), _stream()),
               "pf_knn_csr")
    if deterministic():                                    # one summation order over every list, run after run
        _lib.check(_lib.load().pf_knn_csr_sort(off.data_ptr(), edge.data_ptr(), T, _stream()), "pf_knn_csr_sort")
    return off, edge


class GatherRowsFn(Function):
    """z [B,N,C], idx int32 [B,N,K] -> z[b, idx] as [B*N*K, C] (forward = indexing, backward = HIP scatter-add)."""

    @staticmethod
    def forward(ctx, z, idx):
        B, N, C = z.shape
        K = idx.shape[-1]
        out = z[torch.arange(B, device=z.device).view(B, 1, 1), idx.long()].reshape(B * N * K, C)
        ctx.save_for_backward(idx)
        ctx.dims = (B, N, K, C)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        (idx,) = ctx.saved_tensors
        B, N, K, C = ctx.dims
        g = g.contiguous()
        if deterministic():                                   # ordered gather over the sorted transposed lists: no float atomics
            off, edge = knn_csr(idx.contiguous())
            dz = torch.empty((B, N, C), dtype=torch.float32, device=g.device)
            _lib.check(lib.pf_scatter_rows_det(g.data_ptr(), off.data_ptr(), edge.data_ptr(), B * N, C, dz.data_ptr(), _stream()),
                       "pf_scatter_rows_det")
            return dz, None
        dz = torch.zeros((B, N, C), dtype=torch.float32, device=g.device)
        _lib.check(lib.pf_scatter_rows(g.data_ptr(), idx.data_ptr(), B, N, K, C, dz.data_ptr(), _stream()), "pf_scatter_rows")
        return dz, None


class RepeatRowsFn(Function):
    """repeat_interleave(c, R, dim=1): forward = data movement, backward = HIP group sum."""

    @staticmethod
    def forward(ctx, c, R):
        ctx.R = R
        ctx.shp = c.shape
        return torch.repeat_interleave(c, R, dim=1)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        B, N, C = ctx.shp
        g = g.contiguous()
        out = torch.empty((B, N, C), dtype=torch.float32, device=g.device)
        _lib.check(lib.pf_group_sum(g.data_ptr(), B * N, ctx.R, C, out.data_ptr(), _stream()), "pf_group_sum")
        return out, None


class SoftmaxWsumFn(Function):
    """w [T,K,ldw] logits (first R channels used), zj [T,K,3] -> fz [T,3,R]."""

    @staticmethod
    def forward(ctx, w, zj, R):
        lib = _lib.load()
        w, zj = w.contiguous(), zj.contiguous()
        T, K, ldw = w.shape
        a = torch.empty((T, K, R), dtype=torch.float32, device=w.device)
        fz = torch.empty((T, 3, R), dtype=torch.float32, device=w.device)
        _lib.check(lib.pf_softmax_wsum_fwd(w.data_ptr(), ldw, zj.data_ptr(), K, R, T, a.data_ptr(), fz.data_ptr(), _stream()),
                   "pf_softmax_wsum_fwd")
        ctx.save_for_backward(a, zj)
        ctx.dims = (T, K, R, ldw)
        return fz

    @staticmethod
    def backward(ctx, dfz):
        lib = _lib.load()
        a, zj = ctx.saved_tensors
        T, K, R, ldw = ctx.dims
        dfz = dfz.contiguous()
        dw = torch.empty((T, K, ldw), dtype=torch.float32, device=dfz.device)
        dzj = torch.empty((T, K, 3), dtype=torch.float32, device=dfz.device)
        _lib.check(lib.pf_softmax_wsum_bwd(a.data_ptr(), zj.data_ptr(), dfz.data_ptr(), K, R, ldw, T, dw.data_ptr(),
                                           dzj.data_ptr(), _stream()), "pf_softmax_wsum_bwd")
        return dw, dzj, None


def _det_inv3(W: Tensor):
    """(det, inverse) of a 3x3 matrix in closed form (cross products), differentiable.  torch.slogdet / torch.inverse go
    through a LAPACK-style solver that synchronises with the host, which a captured training step cannot do."""
    r0, r1, r2 = W[0], W[1], W[2]
    c0, c1, c2 = torch.linalg.cross(r1, r2), torch.linalg.cross(r2, r0), torch.linalg.cross(r0, r1)
    det = torch.dot(r0, c0)
    return det, torch.stack([c0, c1, c2], dim=1) / det


def _colsum3(rows: Tensor) -> Tensor:
    """[R,3] -> [3] column sums (HIP, deterministic)."""
    lib = _lib.load()
    R = rows.shape[0]
    out = torch.empty((3,), dtype=torch.float32, device=rows.device)
    ws = _ws(rows.device, 2 * lib.pf_bn_chunks(R) * 3)
    _lib.check(lib.pf_colsum(rows.data_ptr(), R, 3, out.data_ptr(), ws.data_ptr(), _stream()), "pf_colsum")
    return out


class ActNormFn(Function):
    """y = x exp(logs) + bias  (inv=0, normalize.py:34)   or   y = (x - bias) exp(-logs)  (inv=1, normalize.py:41)."""

    @staticmethod
    def forward(ctx, x, logs, bias, inv):
        lib = _lib.load()
        x = x.contiguous()
        lg, bs = logs.reshape(3).contiguous(), bias.reshape(3).contiguous()
        R = x.numel() // 3
        y = torch.empty_like(x)
        _lib.check(lib.pf_actnorm_fwd(x.data_ptr(), lg.data_ptr(), bs.data_ptr(), inv, R, y.data_ptr(), _stream()), "pf_actnorm_fwd")
        ctx.save_for_backward(x, lg, bs)
        ctx.inv, ctx.pshape = inv, logs.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, lg, bs = ctx.saved_tensors
        R = x.numel() // 3
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        gl = torch.empty((R, 3), dtype=torch.float32, device=x.device)
        gb = torch.empty((R, 3), dtype=torch.float32, device=x.device)
        _lib.check(lib.pf_actnorm_bwd(x.data_ptr(), dy.data_ptr(), lg.data_ptr(), bs.data_ptr(), ctx.inv, R, dx.data_ptr(),
                                      gl.data_ptr(), gb.data_ptr(), _stream()), "pf_actnorm_bwd")
        return dx, _colsum3(gl).view(ctx.pshape), _colsum3(gb).view(ctx.pshape), None


class CoupleInjectFn(Function):
    """h2 = y[td:] - o ; v = reverse(cat[h1,h2]) ; out = (v - t) exp(-s)   (coupling.py:55-58,114-118,132-137; permutate.py:77)."""

    @staticmethod
    def forward(ctx, y, o, s, t, td):
        lib = _lib.load()
        y, o, s, t = y.contiguous(), o.contiguous(), s.contiguous(), t.contiguous()
        R = y.numel() // 3
        out = torch.empty_like(y)
        _lib.check(lib.pf_couple_inject_fwd(y.data_ptr(), o.data_ptr(), s.data_ptr(), t.data_ptr(), td, R, out.data_ptr(), _stream()),
                   "pf_couple_inject_fwd")
        ctx.save_for_backward(out, s)
        ctx.td, ctx.oshape = td, o.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        out, s = ctx.saved_tensors
        R = out.numel() // 3
        dout = dout.contiguous()
        dy, ds, dt = torch.empty_like(out), torch.empty_like(out), torch.empty_like(out)
        do = torch.empty(ctx.oshape, dtype=torch.float32, device=out.device)
        _lib.check(lib.pf_couple_inject_bwd(out.data_ptr(), dout.data_ptr(), s.data_ptr(), ctx.td, R, dy.data_ptr(), do.data_ptr(),
                                            ds.data_ptr(), dt.data_ptr(), _stream()), "pf_couple_inject_bwd")
        return dy, do, ds, dt, None


class InjectInvFn(Function):
    """v = reverse(u exp(s) + t)   (coupling.py:147-149; permutate.py:79)."""

    @staticmethod
    def forward(ctx, u, s, t):
        lib = _lib.load()
        u, s, t = u.contiguous(), s.contiguous(), t.contiguous()
        R = u.numel() // 3
        v = torch.empty_like(u)
        _lib.check(lib.pf_inject_inv_fwd(u.data_ptr(), s.data_ptr(), t.data_ptr(), R, v.data_ptr(), _stream()), "pf_inject_inv_fwd")
        ctx.save_for_backward(u, s)
        return v

    @staticmethod
    def backward(ctx, dv):
        lib = _lib.load()
        u, s = ctx.saved_tensors
        R = u.numel() // 3
        dv = dv.contiguous()
        du, ds, dt = torch.empty_like(u), torch.empty_like(u), torch.empty_like(u)
        _lib.check(lib.pf_inject_inv_bwd(u.data_ptr(), s.data_ptr(), dv.data_ptr(), R, du.data_ptr(), ds.data_ptr(), dt.data_ptr(),
                                         _stream()), "pf_inject_inv_bwd")
        return du, ds, dt


class CoupleAddFn(Function):
    """out = cat[v[:td], v[td:] + o]   (coupling.py:82-85)."""

    @staticmethod
    def forward(ctx, v, o, td):
        lib = _lib.load()
        v, o = v.contiguous(), o.contiguous()
        R = v.numel() // 3
        out = torch.empty_like(v)
        _lib.check(lib.pf_couple_add(v.data_ptr(), o.data_ptr(), td, R, out.data_ptr(), _stream()), "pf_couple_add")
        ctx.td, ctx.oshape = td, o.shape
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        g = g.contiguous()
        R = g.numel() // 3
        do = torch.empty(ctx.oshape, dtype=torch.float32, device=g.device)
        _lib.check(lib.pf_slice_tail(g.data_ptr(), ctx.td, R, do.data_ptr(), _stream()), "pf_slice_tail")
        return g, do, None


class BatchSumFn(Function):
    """x [B, ...] -> [B]: mode 0 = sum, mode 1 = sum of -0.5 (x^2 + log 2 pi)  (probs.py:73-75,87-93)."""

    @staticmethod
    def forward(ctx, x, mode):
        lib = _lib.load()
        x = x.contiguous()
        B = x.shape[0]
        M = x.numel() // B
        out = torch.empty((B,), dtype=torch.float32, device=x.device)
        _lib.check(lib.pf_batch_sum_fwd(x.data_ptr(), B, M, mode, out.data_ptr(), _stream()), "pf_batch_sum_fwd")
        ctx.save_for_backward(x)
        ctx.mode = mode
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        (x,) = ctx.saved_tensors
        B = x.shape[0]
        M = x.numel() // B
        g = g.contiguous()
        dx = torch.empty_like(x)
        _lib.check(lib.pf_batch_sum_bwd(x.data_ptr(), g.data_ptr(), B, M, ctx.mode, dx.data_ptr(), _stream()), "pf_batch_sum_bwd")
        return dx, None


def edgeconv_perop(p, x: Tensor, idx: Tensor, pooling: bool = True) -> Tensor:
    """FeatureExtractUnit in train mode (interpflow.py:234-248), one kernel pair per op. x [B,N,C]; returns [B,N,odim] or
    [B*N*K, odim].  The reference of the fused unit (EdgeConvUnitFn) and the path of the shapes it does not take.

    Same algebra as the inference path's edge-feature fold (packing.fold_edgeconv): every conv of the dense block sees
    the edge feature [x_i; x_j; x_j - x_i] only through  (W1 - W3) x_i + (W2 + W3) x_j,  so that part of ALL five convs
    is one GEMM on the B*N points (instead of five on the B*N*K edges with 3C input channels) followed by a
    repeat / gather / add; only the growth-feature columns run per edge.  5.4x fewer MACs at C = 128 and the
    [B*N*K, 3C] edge tensor is never materialised.  Gradients reach W through the slices, x through the point GEMM
    and the gather's scatter-add - exact algebra, same results up to fp32 rounding."""
    B, N, C = x.shape
    K = idx.shape[-1]
    convs = [seq[0] for seq in p.convs] + [p.conv_out]
    Ws = [c.weight.reshape(c.weight.shape[0], -1) for c in convs]
    Wp = torch.cat([w[:, :C] - w[:, 2 * C:3 * C] for w in Ws], dim=0)            # acts on x_i
    Wq = torch.cat([w[:, C:2 * C] + w[:, 2 * C:3 * C] for w in Ws], dim=0)        # acts on x_j
    S = Wp.shape[0]
    bias = torch.cat([c.bias for c in convs] + [torch.zeros(S, dtype=torch.float32, device=x.device)])
    pq = linear(x.reshape(B * N, C), torch.cat([Wp, Wq], dim=0), bias)           # [B*N, 2S] = P (+ bias) | Q
    Pp, Qp = torch.split(pq, [S, S], dim=1)
    E = RepeatRowsFn.apply(Pp.reshape(B, N, S), K).reshape(B * N * K, S) \
        + GatherRowsFn.apply(Qp.reshape(B, N, S), idx)                            # P[i] + Q[j] per edge
    # split (not five slices): its backward is ONE concatenation instead of five zero-filled [B*N*K, S] tensors + adds
    Es = torch.split(E, [w.shape[0] for w in Ws], dim=1)
    feats = []
    for t, seq in enumerate(p.convs):
        y = Es[t]
        if feats:
            y = y + linear(feats[0] if len(feats) == 1 else torch.cat(feats, dim=1), Ws[t][:, 3 * C:])
        feats.append(bn_lrelu(y, seq[1], 0.05))
    y = Es[-1] + linear(torch.cat(feats, dim=1), Ws[-1][:, 3 * C:])
    if not pooling:
        return y.contiguous()
    return MaxPoolKFn.apply(y.contiguous(), K).view(B, N, -1)


def cond_net(net, h: Tensor) -> Tensor:
    """LinearA1D (interpflow.py:38-43)."""
    L = net.layers
    h = ActFn.apply(linear(h, L[0].weight), 0.01)
    h = ActFn.apply(linear(h, L[2].weight, L[2].bias), 0.01)
    return linear(h, L[4].weight, L[4].bias)


def cond_net_split(net, h1: Tensor, cpart: Tensor) -> Tensor:
    """LinearA1D on cat[h1, c] with the c-columns of the bias-free first layer already applied: W0 [h1; c] = W0[:, :td] h1 +
    cpart (interpflow.py:38-41).  cpart = W0[:, td:] c is per ORIGINAL point: f and the R replicas of g share one evaluation."""
    L = net.layers
    td = h1.shape[-1]
    h = ActFn.apply(linear(h1, L[0].weight[:, :td]) + cpart, 0.01)
    h = ActFn.apply(linear(h, L[2].weight, L[2].bias), 0.01)
    return linear(h, L[4].weight, L[4].bias)


def _mlp_bn(mlp, x: Tensor) -> Tensor:
    """Conv,BN,LReLU(.01),Conv,BN,LReLU,Conv on rows (DistanceEncoder / WeightEstimationUnit)."""
    x = bn_lrelu(linear(x, mlp[0].weight, mlp[0].bias), mlp[1], 0.01)
    x = bn_lrelu(linear(x, mlp[3].weight, mlp[3].bias), mlp[4], 0.01)
    return linear(x, mlp[6].weight, mlp[6].bias)
