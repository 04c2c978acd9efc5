"""The fused tiers of the training step: autograd nodes that each cover a unit, an MLP, a flow block piece or a whole flow
direction in a few launches (csrc/train_ec_fwd.hip, train_fused.hip, train_mlp.hip, train_bnmlp.hip, train_flow.hip,
train_flowchain.hip, train_glue.hip).  They read no switch: what train_ops decides reaches them as arguments (EcCfg.persistent)."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch
from torch import Tensor
from torch.autograd import Function

from . import _lib
from .train_state import (_DW_PASS, _FC_IMG, _FC_SCOPE, _attach_sync, _count_batches, _counter, _desc_buf, _dw_begin, _dw_call, _dw_ws,
                          _ptr, _stat, _stream, _sync_bn_active, _sync_words, _ws, deterministic)


class EcCfg(NamedTuple):                    # what EdgeConvUnitFn takes besides tensors with a gradient (edgeconv_train_fused)
    K: int
    growth: int
    nconv: int
    odim: int
    pooling: bool
    slope: float
    eps: float
    momentum: float
    run_means: list
    run_vars: list
    csr: Optional[tuple] = None       # (off, edge) of knn_csr(idx): dQ as a gather, no float atomics
    persistent: bool = False          # the forward / the dense block's backward as one persistent launch where the library can
    sync_bn: bool = False             # statistics over all ranks (fixed at forward time: the backward runs after the sync_bn() scope)
    dw_inline: bool = False           # conv_out's gradient is consumed INSIDE the pass (FoldWuFn): no weight-gradient stream
    prefold: Optional[tuple] = None   # (Wpq, bpq) folded by ec_prefold for this forward
    tap: bool = False                 # also return x, for x's other consumer (see forward)


class EdgeConvUnitFn(Function):
    """One FeatureExtractUnit in train mode as ~11 launches forward / ~20 backward (csrc/train_ec_fwd.hip, csrc/train_fused.hip: the folded edge
    feature, BatchNorm applied on load by the consumer of each layer, statistics in the GEMM epilogues, max-pool in the
    accumulator layout).  Same function and gradients as `edgeconv_train` (interpflow.py:190-248), which stays as the
    A/B reference (PF_TRAIN_FUSED=0) and as the SyncBN path."""

    @staticmethod
    def _desc(x, idx, cfg, Ws, bs, gammas, betas):
        B, N, C = x.shape
        d = _lib.PfEcTrain()
        d.B, d.N, d.K, d.C, d.growth, d.nconv, d.odim, d.pooling = B, N, cfg.K, C, cfg.growth, cfg.nconv, cfg.odim, int(cfg.pooling)
        d.slope, d.eps, d.momentum = cfg.slope, cfg.eps, cfg.momentum
        d.x, d.idx = x.data_ptr(), idx.data_ptr()
        for t in range(cfg.nconv + 1):
            d.W[t], d.bias[t] = Ws[t].data_ptr(), bs[t].data_ptr()
        for t in range(cfg.nconv):
            d.gamma[t], d.beta[t] = gammas[t].data_ptr(), betas[t].data_ptr()
            d.run_mean[t], d.run_var[t] = _ptr(cfg.run_means[t]), _ptr(cfg.run_vars[t])
        d.stat = _stat(x.device).data_ptr()
        if cfg.persistent and not deterministic():            # the forward / the dense block's backward as one persistent launch where
            d.flags, d.sync = _lib.PF_EC_PERSISTENT, _sync_words(x.device).data_ptr()        # the library can
        if deterministic():
            d.flags |= _lib.PF_TRAIN_DETERMINISTIC
        if cfg.sync_bn:
            _attach_sync(d, x.device)
        return d

    @staticmethod
    def forward(ctx, x, idx, cfg, *params):
        lib = _lib.load()
        K, g, nconv, odim, pooling = cfg.K, cfg.growth, cfg.nconv, cfg.odim, cfg.pooling
        nc1 = nconv + 1
        Ws = [w.contiguous() for w in params[:nc1]]
        bs = [b.contiguous() for b in params[nc1:2 * nc1]]
        gammas = [t.contiguous() for t in params[2 * nc1:2 * nc1 + nconv]]
        betas = [t.contiguous() for t in params[2 * nc1 + nconv:]]
        x_in = x
        x = x.contiguous()
        B, N, C = x.shape
        T, E, GT = B * N, B * N * K, g * nconv
        S = GT + odim
        dev = x.device
        f32 = dict(dtype=torch.float32, device=dev)
        pre = cfg.prefold
        if pre is not None and tuple(pre[0].shape) != (2 * S, C):
            raise ValueError("EdgeConvUnitFn: prefolded weights of another unit")
        Wpq, bpq = pre if pre is not None else (torch.empty((2 * S, C), **f32), torch.empty((2 * S,), **f32))
        PQ, Y, aff = torch.empty((T, 2 * S), **f32), torch.empty((E, GT), **f32), torch.empty((4, GT), **f32)
        out = torch.empty((T if pooling else E, odim), **f32)
        arg = torch.empty((T, odim), dtype=torch.uint8, device=dev) if pooling else None
        d = EdgeConvUnitFn._desc(x, idx, cfg, Ws, bs, gammas, betas)
        d.Wpq, d.bpq, d.PQ, d.Y, d.aff, d.out = (Wpq.data_ptr(), bpq.data_ptr(), PQ.data_ptr(), Y.data_ptr(), aff.data_ptr(),
                                                 out.data_ptr())
        d.arg = arg.data_ptr() if pooling else None
        need = lib.pf_ec_train_ws_floats(ctypes.byref(d))
        if need < 0:
            raise _lib.PuflowHipError(f"pf_ec_train: unsupported unit shape (K={K}, growth={g}, nconv={nconv}, odim={odim})")
        ws = _ws(dev, need)
        d.ws, d.ws_floats = ws.data_ptr(), ws.numel()
        if pre is not None:
            d.flags |= _lib.PF_EC_PREFOLDED
        _lib.check(lib.pf_ec_train_fwd(ctypes.byref(d), _stream()), "pf_ec_train_fwd")
        ctx.cfg = cfg
        ctx.has_arg = pooling
        ctx.save_for_backward(x, idx, Wpq, PQ, Y, aff, *(() if arg is None else (arg,)), *Ws, *gammas)
        res = out.view(B, N, odim) if pooling else out
        if cfg.tap:
            # tap: x again, as a second output for x's OTHER consumer - that consumer's gradient then arrives HERE (dtap) and is
            # added in the epilogue of the dx GEMM (PfEcTrain.dx_add) instead of by a launch of autograd's own
            return res, x_in.view_as(x_in)
        return res

    @staticmethod
    def backward(ctx, dout, dtap=None):
        lib = _lib.load()
        cfg = ctx.cfg
        K, g, nconv, odim = cfg.K, cfg.growth, cfg.nconv, cfg.odim
        nc1 = nconv + 1
        sv = list(ctx.saved_tensors)
        x, idx, Wpq, PQ, Y, aff = sv[:6]
        arg = sv[6] if ctx.has_arg else None
        rest = sv[7 if ctx.has_arg else 6:]
        Ws, gammas = rest[:nc1], rest[nc1:]
        B, N, C = x.shape
        T, E, GT = B * N, B * N * K, g * nconv
        S = GT + odim
        dev = x.device
        f32 = dict(dtype=torch.float32, device=dev)
        dout = dout.contiguous()
        d = EdgeConvUnitFn._desc(x, idx, cfg, Ws, Ws, gammas, gammas)      # biases / betas are not read by the backward
        d.Wpq, d.PQ, d.Y, d.aff = Wpq.data_ptr(), PQ.data_ptr(), Y.data_ptr(), aff.data_ptr()
        d.arg = arg.data_ptr() if arg is not None else None
        d.dout = dout.data_ptr()
        dA, dPQ = torch.empty((E, GT), **f32), torch.empty((T, 2 * S), **f32)
        coef, dWpq = torch.empty((2, GT), **f32), torch.empty((2 * S, C), **f32)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dWs = [torch.empty_like(w) for w in Ws]
        dbs = [torch.empty((w.shape[0],), **f32) for w in Ws]
        dgs = [torch.empty((g,), **f32) for _ in range(nconv)]
        dbe = [torch.empty((g,), **f32) for _ in range(nconv)]
        d.dA, d.dPQ, d.coef, d.dWpq = dA.data_ptr(), dPQ.data_ptr(), coef.data_ptr(), dWpq.data_ptr()
        d.dx = dx.data_ptr() if dx is not None else None
        if dtap is not None and dx is not None:
            dtap = dtap.contiguous()
            if dtap.shape != x.shape or dtap.dtype != torch.float32:
                raise ValueError("EdgeConvUnitFn: gradient of the tap has another shape than x")
            d.dx_add = dtap.data_ptr()
        for t in range(nc1):
            d.dW[t], d.dbias[t] = dWs[t].data_ptr(), dbs[t].data_ptr()
        for t in range(nconv):
            d.dgamma[t], d.dbeta[t] = dgs[t].data_ptr(), dbe[t].data_ptr()
        need = lib.pf_ec_train_ws_floats(ctypes.byref(d))
        ws = _ws(dev, need)
        d.ws, d.ws_floats = ws.data_ptr(), ws.numel()
        if cfg.csr is not None:                               # transposed neighbour lists: dQ as a gather, no float atomics
            d.csr_off, d.csr_edge = cfg.csr[0].data_ptr(), cfg.csr[1].data_ptr()
        dwst = None if cfg.dw_inline else _dw_begin(dev, sv, dout, dA, dPQ, coef, dWpq, ws)
        if dwst is not None:                                  # weight gradients on their own stream, with their own workspace
            ws2 = _dw_ws(dwst, dev, need)
            d.ws_dw, d.ws_dw_floats = ws2.data_ptr(), ws2.numel()
        with _dw_call(dwst):
            _lib.check(lib.pf_ec_train_bwd(ctypes.byref(d), _stream()), "pf_ec_train_bwd")
        return (dx, None, None, *dWs, *dbs, *dgs, *dbe)


class FlowParamsFn(Function):
    """W [3,3], logs [...,3] -> (W^-1 [3,3], ld [1] = (sum(logs) + log|det W|) n): the parameter-only scalars of a flow block
    (normalize.py:34-36, permutate.py:118-124) in one one-thread kernel instead of ~25 tiny torch launches."""

    @staticmethod
    def forward(ctx, W, logs, n):
        lib = _lib.load()
        W, lg = W.contiguous(), logs.reshape(3).contiguous()
        Winv = torch.empty_like(W)
        ld = torch.empty((1,), dtype=torch.float32, device=W.device)
        _lib.check(lib.pf_flow_params_fwd(W.data_ptr(), lg.data_ptr(), float(n), Winv.data_ptr(), ld.data_ptr(), _stream()),
                   "pf_flow_params_fwd")
        ctx.save_for_backward(Winv)
        ctx.n, ctx.lshape = float(n), logs.shape
        return Winv, ld

    @staticmethod
    def backward(ctx, dWinv, dld):
        lib = _lib.load()
        (Winv,) = ctx.saved_tensors
        dW = torch.empty_like(Winv)
        dlogs = torch.empty((3,), dtype=torch.float32, device=Winv.device)
        dWinv = dWinv.contiguous() if dWinv is not None else None
        dld = dld.contiguous() if dld is not None else None
        _lib.check(lib.pf_flow_params_bwd(Winv.data_ptr(), _ptr(dWinv), _ptr(dld), ctx.n, dW.data_ptr(), dlogs.data_ptr(),
                                          _stream()), "pf_flow_params_bwd")
        return dW, dlogs.view(ctx.lshape), None


class FlowAffineFn(Function):
    """inv=0: y = M (x e^logs + bias)  (ActNorm, then the 3x3 linear);  inv=1: y = (M [x_head, x_tail + o] - bias) e^-logs
    (coupling shift, inverse linear, inverse ActNorm).  One launch each way; the 15 parameter-gradient sums are reduced
    inside the backward kernel (csrc/train_flow.hip)."""

    @staticmethod
    def forward(ctx, x, o, td, logs, bias, M, inv):
        lib = _lib.load()
        x = x.contiguous()
        o = o.contiguous() if o is not None else None
        lg, bs, M = logs.reshape(3).contiguous(), bias.reshape(3).contiguous(), M.contiguous()
        R = x.numel() // 3
        y = torch.empty_like(x)
        _lib.check(lib.pf_flow_affine_fwd(x.data_ptr(), _ptr(o), td, lg.data_ptr(), bs.data_ptr(), M.data_ptr(), inv, R,
                                          y.data_ptr(), _stream()), "pf_flow_affine_fwd")
        ctx.save_for_backward(x, lg, bs, M, *(() if o is None else (o,)))
        ctx.cfg = (td, inv, logs.shape, o is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        td, inv, pshape, has_o = ctx.cfg
        sv = ctx.saved_tensors
        x, lg, bs, M = sv[:4]
        o = sv[4] if has_o else None
        R = x.numel() // 3
        dy = dy.contiguous()
        dev = x.device
        dx = torch.empty_like(x)
        do = torch.empty_like(o) if has_o else None
        dl, db = torch.empty((3,), dtype=torch.float32, device=dev), torch.empty((3,), dtype=torch.float32, device=dev)
        dM = torch.empty_like(M)
        ws = _ws(dev, 256 * 16)
        _lib.check(lib.pf_flow_affine_bwd(x.data_ptr(), _ptr(o), td, lg.data_ptr(), bs.data_ptr(), M.data_ptr(), inv, R,
                                          dy.data_ptr(), dx.data_ptr(), _ptr(do), dl.data_ptr(), db.data_ptr(), dM.data_ptr(),
                                          ws.data_ptr(), _counter(dev).data_ptr(), _stream()), "pf_flow_affine_bwd")
        return dx, do, None, dl.view(pshape), db.view(pshape), dM, None


class CoupleInject2Fn(Function):
    """CoupleInjectFn that also returns sum(s) (the injector's log-det term, coupling.py:137) from the same launch."""

    @staticmethod
    def forward(ctx, y, o, s, t, td):
        lib = _lib.load()
        y, o, s, t = y.contiguous(), o.contiguous(), s.contiguous(), t.contiguous()
        R = y.numel() // 3
        dev = y.device
        out = torch.empty_like(y)
        ssum = torch.empty((1,), dtype=torch.float32, device=dev)
        ws = _ws(dev, 256 * 16)
        _lib.check(lib.pf_couple_inject2_fwd(y.data_ptr(), o.data_ptr(), s.data_ptr(), t.data_ptr(), td, R, out.data_ptr(),
                                             ssum.data_ptr(), ws.data_ptr(), _counter(dev).data_ptr(), _stream()),
                   "pf_couple_inject2_fwd")
        ctx.save_for_backward(out, s)
        ctx.td, ctx.oshape = td, o.shape
        return out, ssum

    @staticmethod
    def backward(ctx, dout, dssum):
        lib = _lib.load()
        out, s = ctx.saved_tensors
        R = out.numel() // 3
        dout = dout.contiguous()
        dssum = dssum.contiguous() if dssum is not None else None
        dy, ds, dt = torch.empty_like(out), torch.empty_like(s), torch.empty_like(s)
        do = torch.empty(ctx.oshape, dtype=torch.float32, device=out.device)
        _lib.check(lib.pf_couple_inject2_bwd(out.data_ptr(), dout.data_ptr(), _ptr(dssum), s.data_ptr(), ctx.td, R, dy.data_ptr(),
                                             do.data_ptr(), ds.data_ptr(), dt.data_ptr(), _stream()), "pf_couple_inject2_bwd")
        return dy, do, ds, dt, None


class InjectInv2Fn(Function):
    """v = reverse(u e^s + t) with s, t [T,3] of the ORIGINAL points and u [T*R,3]: the repeat_interleave of the reference
    (interpflow.py:319) happens in the index, its backward (sum over the R rows) in the same kernel."""

    @staticmethod
    def forward(ctx, u, s, t, Rr):
        lib = _lib.load()
        u, s, t = u.contiguous(), s.contiguous(), t.contiguous()
        R = u.numel() // 3
        v = torch.empty_like(u)
        _lib.check(lib.pf_inject_inv2_fwd(u.data_ptr(), s.data_ptr(), t.data_ptr(), Rr, R, v.data_ptr(), _stream()),
                   "pf_inject_inv2_fwd")
        ctx.save_for_backward(u, s)
        ctx.Rr = Rr
        return v

    @staticmethod
    def backward(ctx, dv):
        lib = _lib.load()
        u, s = ctx.saved_tensors
        R = u.numel() // 3
        dv = dv.contiguous()
        du, ds, dt = torch.empty_like(u), torch.empty_like(s), torch.empty_like(s)
        _lib.check(lib.pf_inject_inv2_bwd(u.data_ptr(), s.data_ptr(), dv.data_ptr(), ctx.Rr, R, du.data_ptr(), ds.data_ptr(),
                                          dt.data_ptr(), _stream()), "pf_inject_inv2_bwd")
        return du, ds, dt, None


def _flat_grads(prm, f32):
    """One buffer for all parameter gradients of a node -> (the buffer, its slice per parameter)."""
    sizes = [int(p.numel()) for p in prm]
    flat = torch.empty((sum(sizes),), **f32)
    return flat, list(torch.split(flat, sizes))


class FlowChainFn(Function):
    """All flow blocks of one direction as ONE autograd node: two launches forward, four backward (csrc/train_flowchain.hip).
    apply(inv, R, n_ld, ccs, x, cflat, st, Bsz, *[logs, bias, W, w0, w2, b2, w4, b4] per block)
      ccs    conditioning channels per block; cflat = the blocks' conditioning features [T, cc_i], flattened and concatenated
             (ONE tensor: its three consumers cost two gradient additions instead of twelve)
      st     [2 nb, T, 3]: injector scale (2 i) and shift (2 i + 1) of block i per ORIGINAL point
      inv = 0 (PointInterpFlow.f, interpflow.py:302-310): x [B,N,3] -> (z, ssum [nb] = sum(s_i), ld [nb] = (sum(logs_i) + log|det W_i|) n_ld);
              with Bsz > 0 instead (z, logp [1]) - the log-likelihood -mean_b(log N(z_b) + sum_i (ld_i - sum(s_i)[b])) of
              interpflow.py:327-337 from the kernel's own epilogue, its backward folded into the chain kernel
      inv = 1 (PointInterpFlow.g, interpflow.py:312-321): u [B,N R,3] -> x, blocks in reverse order
    Replaces, per block, FlowParamsFn + FlowAffineFn + MlpFn + CoupleInject2Fn / InjectInv2Fn and the gradient-accumulation adds
    autograd inserted between them."""

    @staticmethod
    def _desc(inv, R, n_ld, ccs, x, cflat, st, prm):
        nb = len(ccs)
        d = _lib.PfFlowChain()
        d.nb, d.rows, d.R, d.inv, d.n_ld = nb, x.numel() // 3, R, inv, float(n_ld)
        d.x = x.data_ptr()
        T = d.rows // R
        off = 0
        for i in range(nb):
            lg, bi, W, w0, w2, b2, w4, b4 = prm[8 * i:8 * i + 8]
            d.cc[i] = ccs[i]
            d.td[i] = w0.shape[1] - ccs[i]
            d.c[i] = cflat.data_ptr() + 4 * off
            off += T * ccs[i]
            d.s[i], d.t[i] = st[2 * i].data_ptr(), st[2 * i + 1].data_ptr()
            d.logs[i], d.bias[i], d.W[i] = lg.data_ptr(), bi.data_ptr(), W.data_ptr()
            d.w0[i], d.w2[i], d.b2[i], d.w4[i], d.b4[i] = w0.data_ptr(), w2.data_ptr(), b2.data_ptr(), w4.data_ptr(), b4.data_ptr()
        if cflat.numel() != off or tuple(st.shape) != (2 * nb, T, 3):
            raise ValueError("FlowChainFn: conditioning tensors do not match the row count")
        return d

    @staticmethod
    def forward(ctx, inv, R, n_ld, ccs, x, cflat, st, Bsz, *prm):
        lib = _lib.load()
        x, cflat, st = x.contiguous(), cflat.contiguous(), st.contiguous()
        prm = [t.contiguous() for t in prm]
        nb = len(ccs)
        dev = x.device
        f32 = dict(dtype=torch.float32, device=dev)
        d = FlowChainFn._desc(inv, R, n_ld, ccs, x, cflat, st, prm)
        rows = d.rows
        keep = torch.empty((2, nb, rows, 3), **f32)                      # block inputs | y (f) / v (g)
        hh = torch.empty((2, nb, rows, 64), **f32)
        o = torch.empty((nb, rows, 2), **f32) if inv else None
        out = torch.empty_like(x)
        ssum, ld = torch.empty((nb,), **f32), torch.empty((nb,), **f32)   # sum(s) | log-det term, per block
        d.pin, d.mid, d.h1, d.h2, d.out = keep[0].data_ptr(), keep[1].data_ptr(), hh[0].data_ptr(), hh[1].data_ptr(), out.data_ptr()
        d.o = _ptr(o)
        d.ssum, d.ld = ssum.data_ptr(), ld.data_ptr()
        logp = None
        if Bsz and not inv:
            logp = torch.empty((1,), **f32)
            d.logp, d.Bsz = logp.data_ptr(), int(Bsz)
        d.part = _ws(dev, (nb + 1) * ((rows + 15) // 16)).data_ptr()
        d.counter = _counter(dev).data_ptr()
        # packed weights (the conditioner nets' LDS images), kept for the backward.  They do not depend on the direction: the g chain
        # of a forward takes the image the f chain packed from the same parameters on the same stream (one pack launch fewer)
        key = (_FC_SCOPE[0], tuple(int(c) for c in ccs), _stream(), tuple((t.data_ptr(), t._version) for t in prm))
        cached = _FC_IMG.get(dev) if _FC_SCOPE[0] else None      # only inside one forward_train call
        if cached is not None and cached[0] == key:
            img = cached[1]
            d.img_ready = 1
        else:
            img = torch.empty((lib.pf_flowchain_img_floats(ctypes.byref(d)),), **f32)
            _FC_IMG[dev] = (key, img)
        d.img = img.data_ptr()
        _lib.check(lib.pf_flowchain_fwd(ctypes.byref(d), _stream()), "pf_flowchain_fwd")
        ctx.cfg = (inv, R, float(n_ld), tuple(ccs), [t.shape for t in prm], int(Bsz) if logp is not None else 0)
        ctx.save_for_backward(x, out, keep, hh, img, cflat, st, *(() if o is None else (o,)), *prm)
        if inv:
            return out
        if logp is not None:
            return out, logp
        return out, ssum, ld

    @staticmethod
    def backward(ctx, dout, dssum=None, dld=None):
        lib = _lib.load()
        inv, R, n_ld, ccs, pshapes, Bsz = ctx.cfg
        dlogp = None
        if Bsz:                                            # outputs were (z, logp)
            dlogp, dssum = (dssum.contiguous().view(1) if dssum is not None else None), None
        nb = len(ccs)
        sv = list(ctx.saved_tensors)
        x, out, keep, hh, img, cflat, st = sv[:7]
        o, prm = (sv[7], sv[8:]) if inv else (None, sv[7:])
        dev = x.device
        f32 = dict(dtype=torch.float32, device=dev)
        d = FlowChainFn._desc(inv, R, n_ld, ccs, x, cflat, st, prm)
        rows = d.rows
        T = rows // R
        d.pin, d.mid, d.h1, d.h2, d.out = keep[0].data_ptr(), keep[1].data_ptr(), hh[0].data_ptr(), hh[1].data_ptr(), out.data_ptr()
        d.o = _ptr(o)
        d.img = img.data_ptr()
        dout = dout.contiguous() if dout is not None else None
        dssum = dssum.contiguous() if dssum is not None else None
        dld = dld.contiguous() if dld is not None else None
        if dout is None and dlogp is None:
            dout = torch.zeros_like(x)
        d.dout, d.dssum, d.dld, d.dlogp, d.Bsz = _ptr(dout), _ptr(dssum), _ptr(dld), _ptr(dlogp), Bsz
        dx = torch.empty_like(x) if ctx.needs_input_grad[4] else None
        d.dx = _ptr(dx)
        dcflat = torch.empty_like(cflat)
        dst = torch.empty_like(st)
        dz = torch.empty((2, nb, rows, 64), **f32)
        dob = torch.empty((nb, rows, 2), **f32)
        d.dz1, d.dz2, d.dob = dz[0].data_ptr(), dz[1].data_ptr(), dob.data_ptr()
        dzs = None
        if R > 1:
            # the first hidden layer's gradient summed over the R rows that share a conditioning row: the weight-gradient launch
            # then runs that layer's conditioning columns (cc of cc + td) over rows / R summed rows (PF_MLP_DW_DZSUM)
            dzs = torch.empty((nb, T, 64), **f32)
            d.dz1s = dzs.data_ptr()
        _, gp = _flat_grads(prm, f32)                                    # every parameter gradient of the chain, one buffer
        coff = 0
        for i in range(nb):
            d.dc[i] = dcflat.data_ptr() + 4 * coff
            coff += T * ccs[i]
            d.ds[i], d.dt[i] = dst[2 * i].data_ptr(), dst[2 * i + 1].data_ptr()
            for name, g in zip(("dlogs", "dbias", "dW", "dw0", "dw2", "db2", "dw4", "db4"), gp[8 * i:8 * i + 8]):
                getattr(d, name)[i] = g.data_ptr()
        npart = lib.pf_flowchain_part_floats(ctypes.byref(d))
        need = lib.pf_flowchain_ws_floats(ctypes.byref(d))
        if need < 0 or npart < 0:
            raise _lib.PuflowHipError("pf_flowchain: unsupported shape")
        ws = _ws(dev, npart + need)
        d.part = ws.data_ptr()
        d.ws, d.ws_floats = ws.data_ptr() + 4 * npart, need
        d.dev_descs = _desc_buf(dev).data_ptr()
        # (not on the weight-gradient stream: the f and the g chain share their parameters, so autograd ADDS the two chains'
        # gradients on this stream as soon as the second one returns - before any join)
        _lib.check(lib.pf_flowchain_bwd(ctypes.byref(d), _stream()), "pf_flowchain_bwd")
        grads = [g.view(shp) for g, shp in zip(gp, pshapes)]
        return (None, None, None, None, dx, dcflat, dst, None, *grads)


class FanoutFn(Function):
    """apply(n, x) -> n aliases of x, one per consumer; backward: the n gradients summed in ONE launch (pf_sum_n,
    ((g0 + g1) + g2) + ...) instead of autograd's n - 1 pairwise adds over the running sum."""

    @staticmethod
    def forward(ctx, n, x):
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        gs = [g.contiguous() for g in gs if g is not None]
        if not gs:
            return None, None
        if len(gs) == 1:
            return None, gs[0]
        g0 = gs[0]
        if (g0.numel() % 4 or len(gs) > 8 or not g0.is_cuda
                or any(g.dtype != torch.float32 or g.shape != g0.shape or g.data_ptr() % 16 for g in gs)):
            out = gs[0] + gs[1]
            for g in gs[2:]:
                out = out + g
            return None, out
        out = torch.empty_like(g0)
        ptrs = (ctypes.c_void_p * len(gs))(*[g.data_ptr() for g in gs])
        _lib.check(_lib.load().pf_sum_n(ptrs, len(gs), out.data_ptr(), g0.numel(), _stream()), "pf_sum_n")
        return None, out


class MlpFn(Function):
    """2- or 3-layer point-wise MLP (LinearA1D / FeatMergeUnit, interpflow.py:22-43, 251-258) on cat[y[:, :td], c[row // cdiv]]:
    one launch forward, three backward (csrc/train_mlp.hip).  wb = W0, b0, W1, b1[, W2, b2] (None for a missing bias)."""

    @staticmethod
    def _desc(y, c, td, cdiv, slopes, Ws, bs):
        d = _lib.PfMlpTrain()
        nl = len(Ws)
        cc = c.shape[-1]
        rows = c.numel() // cc * cdiv
        d.rows, d.nl, d.td, d.cc, d.cdiv = rows, nl, td, cc, cdiv
        d.ldy = y.shape[-1] if y is not None else 0
        for l in range(nl):
            d.width[l], d.W[l], d.b[l] = Ws[l].shape[0], Ws[l].data_ptr(), _ptr(bs[l])
        for l in range(nl - 1):
            d.slope[l] = slopes[l]
        d.y, d.c = _ptr(y), c.data_ptr()
        return d, rows

    @staticmethod
    def _cond_descs(cs, prm, chunk: int = 0):
        """One descriptor per LinearA1D conditioner that reads features only (first layer without bias, interpflow.py:22-43):
        net k = W0, W1, b1, W2, b2 = prm[5 k:5 k + 5] on cs[k].  The biases are for the forward to set; chunk: rows per split-K
        chunk of the weight gradients (0: the library's choice)."""
        descs = (_lib.PfMlpTrain * len(cs))()
        for k, c in enumerate(cs):
            d, _ = MlpFn._desc(None, c, 0, 1, (0.01, 0.01), [prm[5 * k], prm[5 * k + 1], prm[5 * k + 3]], [None] * 3)
            d.chunk = chunk
            descs[k] = d
        return descs

    @staticmethod
    def _batch_ws(descs, dev, dwst=None):
        """Weight-gradient scratch of a batched backward: one buffer (the weight-gradient stream's own under `dwst`), descriptor k
        takes its part of it."""
        lib = _lib.load()
        need = [lib.pf_mlp_train_ws_floats(ctypes.byref(d)) for d in descs]
        ws = _dw_ws(dwst, dev, sum(need))
        off = 0
        for d, n in zip(descs, need):
            d.ws, d.ws_floats = ws.data_ptr() + 4 * off, n
            off += n
        return ws

    @staticmethod
    def _bwd_ptrs(d, hs, dzs, dout, dy, dc, dWs, dbs) -> None:
        """The backward's tensors into descriptor d: hidden activations and their gradients per hidden layer, dW / db (None: no
        bias) per layer."""
        for l, (h, dz) in enumerate(zip(hs, dzs)):
            d.h[l], d.dz[l] = h.data_ptr(), dz.data_ptr()
        d.dout, d.dy, d.dc = dout.data_ptr(), _ptr(dy), _ptr(dc)
        for l, (dW, db) in enumerate(zip(dWs, dbs)):
            d.dW[l], d.db[l] = dW.data_ptr(), _ptr(db)

    @staticmethod
    def forward(ctx, y, c, td, cdiv, slopes, *wb):
        lib = _lib.load()
        Ws = [w.contiguous() for w in wb[0::2]]
        bs = [b.contiguous() if b is not None else None for b in wb[1::2]]
        y = y.contiguous() if (y is not None and td > 0) else None
        c = c.contiguous()
        d, rows = MlpFn._desc(y, c, td, cdiv, slopes, Ws, bs)
        f32 = dict(dtype=torch.float32, device=c.device)
        hs = [torch.empty((rows, Ws[l].shape[0]), **f32) for l in range(len(Ws) - 1)]
        out = torch.empty((rows, Ws[-1].shape[0]), **f32)
        for l, h in enumerate(hs):
            d.h[l] = h.data_ptr()
        d.out = out.data_ptr()
        _lib.check(lib.pf_mlp_train_fwd(ctypes.byref(d), _stream()), "pf_mlp_train_fwd")
        ctx.cfg = (td, cdiv, slopes, len(Ws), [b is not None for b in bs], y is not None)
        ctx.save_for_backward(c, *hs, *Ws, *(() if y is None else (y,)))
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        td, cdiv, slopes, nl, has_b, has_y = ctx.cfg
        sv = list(ctx.saved_tensors)
        c, hs, Ws = sv[0], sv[1:nl], sv[nl:2 * nl]
        y = sv[2 * nl] if has_y else None
        dout = dout.contiguous()
        d, rows = MlpFn._desc(y, c, td, cdiv, slopes, Ws, [None] * nl)
        f32 = dict(dtype=torch.float32, device=c.device)
        dzs = [torch.empty_like(h) for h in hs]
        dy = torch.empty_like(y) if (has_y and ctx.needs_input_grad[0]) else None
        dc = torch.empty_like(c) if ctx.needs_input_grad[1] else None
        dWs = [torch.empty_like(w) for w in Ws]
        dbs = [torch.empty((w.shape[0],), **f32) if has_b[l] else None for l, w in enumerate(Ws)]
        MlpFn._bwd_ptrs(d, hs, dzs, dout, dy, dc, dWs, dbs)
        need = lib.pf_mlp_train_ws_floats(ctypes.byref(d))
        if need < 0:
            raise _lib.PuflowHipError("pf_mlp_train: unsupported shape")
        dwst = _dw_begin(c.device, sv, dout, dzs, hs)
        ws = _dw_ws(dwst, c.device, need)                     # weight-gradient scratch only
        d.ws, d.ws_floats = ws.data_ptr(), ws.numel()
        with _dw_call(dwst):
            _lib.check(lib.pf_mlp_train_bwd(ctypes.byref(d), _stream()), "pf_mlp_train_bwd")
        return (dy, dc, None, None, None, *[g for pair in zip(dWs, dbs) for g in pair])


class CondNetStackFn(Function):
    """The injector scale / shift conditioners (LinearA1D, first layer without bias, interpflow.py:22-43) of ALL flow blocks on the
    flattened conditioning features: one launch forward, four backward (csrc/train_mlp.hip, batched entry points), ONE output
    tensor.  apply(ccs, T, cflat, cflat2, *[W0, W1, b1, W2, b2 per net]) -> st [n, T, 3]; net k reads block k // 2's features.
    cflat2: None, or a second alias of cflat (FanoutFn) - the gradient through the scale nets then goes to cflat and the one
    through the shift nets to cflat2, un-added (the fan-out sums them with the other consumers' in its one launch)."""

    @staticmethod
    def _descs(ccs, T, cflat, prm, n):
        offs = [0]
        for cc in ccs:
            offs.append(offs[-1] + T * cc)
        cs = [cflat.view(-1)[offs[k // 2]:offs[k // 2 + 1]].view(T, ccs[k // 2]) for k in range(n)]
        return MlpFn._cond_descs(cs, prm, chunk=256), offs      # n networks x 3 layers in one launch: long split-K chunks

    @staticmethod
    def forward(ctx, ccs, T, cflat, cflat2, *prm):
        lib = _lib.load()
        n = len(prm) // 5
        ctx.two = cflat2 is not None
        cflat = cflat.contiguous()
        prm = [w.contiguous() for w in prm]
        dev = cflat.device
        f32 = dict(dtype=torch.float32, device=dev)
        descs, _ = CondNetStackFn._descs(ccs, T, cflat, prm, n)
        hs = torch.empty((n, 2, T, 64), **f32)
        st = torch.empty((n, T, 3), **f32)
        for k in range(n):
            W0, W1, b1, W2, b2 = prm[5 * k:5 * k + 5]
            if W0.shape[0] != 64 or W1.shape[0] != 64 or W2.shape[0] != 3:
                raise ValueError("CondNetStackFn: unexpected conditioner shape")
            descs[k].b[1], descs[k].b[2] = b1.data_ptr(), b2.data_ptr()
            descs[k].h[0], descs[k].h[1], descs[k].out = hs[k, 0].data_ptr(), hs[k, 1].data_ptr(), st[k].data_ptr()
        _lib.check(lib.pf_mlp_train_fwd_batch(descs, n, _desc_buf(dev).data_ptr(), _stream()), "pf_mlp_train_fwd_batch")
        ctx.cfg = (tuple(ccs), T, n)
        ctx.save_for_backward(cflat, hs, *prm)
        return st

    @staticmethod
    def backward(ctx, dst):
        lib = _lib.load()
        ccs, T, n = ctx.cfg
        sv = list(ctx.saved_tensors)
        cflat, hs, prm = sv[0], sv[1], sv[2:]
        dev = cflat.device
        f32 = dict(dtype=torch.float32, device=dev)
        dst = dst.contiguous()
        descs, offs = CondNetStackFn._descs(ccs, T, cflat, prm, n)
        dz = torch.empty_like(hs)
        dc2 = torch.empty((2, cflat.numel()), **f32)                    # gradients through the scale nets | through the shift nets
        flat, gp = _flat_grads(prm, f32)
        dwst = _dw_begin(dev, sv, dst, dz, dc2, flat)
        MlpFn._batch_ws(descs, dev, dwst)
        ddesc = _desc_buf(dev)
        if dwst is not None:                                  # the side kernels read the descriptors: this call's own copy
            ddesc = torch.empty(16 * ctypes.sizeof(_lib.PfMlpTrain), dtype=torch.uint8, device=dev)
            _DW_PASS["keep"].append((ddesc,))
        for k, d in enumerate(descs):
            g = gp[5 * k:5 * k + 5]                             # W0, W1, b1, W2, b2
            MlpFn._bwd_ptrs(d, hs[k], dz[k], dst[k], None, dc2[k % 2, offs[k // 2]:], (g[0], g[1], g[3]), (None, g[2], g[4]))
        with _dw_call(dwst):
            _lib.check(lib.pf_mlp_train_bwd_batch(descs, n, ddesc.data_ptr(), _stream()), "pf_mlp_train_bwd_batch")
        grads = [g.view(p.shape) for g, p in zip(gp, prm)]
        if ctx.two:
            return (None, None, dc2[0], dc2[1], *grads)
        return (None, None, dc2[0] + dc2[1], None, *grads)


class CondNetBatchFn(Function):
    """Several LinearA1D conditioners (first layer without bias, interpflow.py:22-43) that only read conditioning features -
    the scale and shift nets of every flow block - in ONE launch forward and four backward (csrc/train_mlp.hip, batched
    entry points).  apply(cidx, *cs, *[W0, W1, b1, W2, b2 per net]) -> one [rows, dout] tensor per net; cidx[k] = which of
    the `cs` tensors net k reads."""

    @staticmethod
    def forward(ctx, cidx, *ts):
        lib = _lib.load()
        n = len(cidx)
        ncs = len(ts) - 5 * n
        cs = [c.contiguous() for c in ts[:ncs]]
        prm = [w.contiguous() for w in ts[ncs:]]
        descs = MlpFn._cond_descs([cs[i] for i in cidx], prm)
        outs, hs = [], []
        for k, d in enumerate(descs):
            W0, W1, b1, W2, b2 = prm[5 * k:5 * k + 5]
            f32 = dict(dtype=torch.float32, device=W0.device)
            h = [torch.empty((d.rows, W0.shape[0]), **f32), torch.empty((d.rows, W1.shape[0]), **f32)]
            out = torch.empty((d.rows, W2.shape[0]), **f32)
            d.b[1], d.b[2] = b1.data_ptr(), b2.data_ptr()
            d.h[0], d.h[1], d.out = h[0].data_ptr(), h[1].data_ptr(), out.data_ptr()
            outs.append(out)
            hs += h
        _lib.check(lib.pf_mlp_train_fwd_batch(descs, n, _desc_buf(cs[0].device).data_ptr(), _stream()), "pf_mlp_train_fwd_batch")
        ctx.cidx, ctx.ncs = cidx, ncs
        ctx.save_for_backward(*cs, *prm, *hs)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        lib = _lib.load()
        cidx, ncs = ctx.cidx, ctx.ncs
        n = len(cidx)
        sv = list(ctx.saved_tensors)
        cs, prm, hs = sv[:ncs], sv[ncs:ncs + 5 * n], sv[ncs + 5 * n:]
        dev = cs[0].device
        descs = MlpFn._cond_descs([cs[i] for i in cidx], prm)
        MlpFn._batch_ws(descs, dev)
        keep, grads, dcs = [], [], [[] for _ in range(ncs)]
        for k, d in enumerate(descs):
            W0, W1, b1, W2, b2 = prm[5 * k:5 * k + 5]
            dout = douts[k].contiguous() if douts[k] is not None else torch.zeros((d.rows, W2.shape[0]), dtype=torch.float32, device=dev)
            dz = [torch.empty_like(hs[2 * k]), torch.empty_like(hs[2 * k + 1])]
            dc = torch.empty_like(cs[cidx[k]])
            dW = [torch.empty_like(W0), torch.empty_like(W1), torch.empty_like(W2)]
            db = [torch.empty_like(b1), torch.empty_like(b2)]
            MlpFn._bwd_ptrs(d, hs[2 * k:2 * k + 2], dz, dout, None, dc, dW, (None, db[0], db[1]))
            keep += [dout, dz]
            dcs[cidx[k]].append(dc)
            grads += [dW[0], dW[1], db[0], dW[2], db[1]]
        _lib.check(lib.pf_mlp_train_bwd_batch(descs, n, _desc_buf(dev).data_ptr(), _stream()), "pf_mlp_train_bwd_batch")
        dc_out = []
        for lst in dcs:
            if len(lst) < 2:
                dc_out.append(lst[0] if lst else None)
            else:
                dc_out.append(torch.stack(lst).sum(0) if len(lst) > 2 else lst[0] + lst[1])
        return (None, *dc_out, *grads)


class MergeBatchFn(Function):
    """The FeatMergeUnits of all EdgeConv units (Linear + ReLU + Linear without bias, interpflow.py:251-258) in ONE launch forward
    and three backward (csrc/train_mlp.hip, batched entry points: one descriptor per unit, shapes may differ) instead of one /
    three per unit: their outputs are only read by the flow stage, so nothing waits for them before the last unit is done.
    apply(n, *hs, *[W1, b1, W2 per unit]) -> ONE flat tensor, the units' [rows, cdim] outputs one after the other (the layout the
    flow chains and the injector stack read: no concatenation afterwards).  Same kernels, same arithmetic as `mlp_fused`."""

    @staticmethod
    def _descs(hs, prm):
        descs = (_lib.PfMlpTrain * len(hs))()
        for k, h in enumerate(hs):                              # W1, b1, W2 = prm[3 k:3 k + 3]
            descs[k], rows = MlpFn._desc(None, h, 0, 1, (0.0,), [prm[3 * k], prm[3 * k + 2]], [prm[3 * k + 1], None])
        return descs, rows

    @staticmethod
    def forward(ctx, n, *ts):
        lib = _lib.load()
        hs = [h.contiguous() for h in ts[:n]]
        prm = [w.contiguous() for w in ts[n:]]
        descs, rows = MergeBatchFn._descs(hs, prm)
        f32 = dict(dtype=torch.float32, device=hs[0].device)
        mids = [torch.empty((rows, prm[3 * k].shape[0]), **f32) for k in range(n)]
        cds = [int(prm[3 * k + 2].shape[0]) for k in range(n)]
        flat = torch.empty((rows * sum(cds),), **f32)
        off = 0
        for k in range(n):
            descs[k].h[0], descs[k].out = mids[k].data_ptr(), flat.data_ptr() + 4 * off
            off += rows * cds[k]
        _lib.check(lib.pf_mlp_train_fwd_batch(descs, n, _desc_buf(hs[0].device).data_ptr(), _stream()), "pf_mlp_train_fwd_batch")
        ctx.n = n
        ctx.save_for_backward(*hs, *prm, *mids)
        return flat

    @staticmethod
    def backward(ctx, dflat):
        lib = _lib.load()
        n = ctx.n
        dflat = dflat.contiguous()
        sv = list(ctx.saved_tensors)
        hs, prm, mids = sv[:n], sv[n:4 * n], sv[4 * n:]
        dev = hs[0].device
        descs, rows = MergeBatchFn._descs(hs, prm)
        MlpFn._batch_ws(descs, dev)
        keep, dhs, grads, doff = [], [], [], 0
        for k, d in enumerate(descs):
            W1, b1, W2 = prm[3 * k:3 * k + 3]
            dout = dflat[doff:doff + rows * W2.shape[0]]
            doff += rows * W2.shape[0]
            dz, dh = torch.empty_like(mids[k]), torch.empty_like(hs[k])
            dW1, db1, dW2 = torch.empty_like(W1), torch.empty_like(b1), torch.empty_like(W2)
            MlpFn._bwd_ptrs(d, [mids[k]], [dz], dout, None, dh, (dW1, dW2), (db1, None))
            keep += [dout, dz]
            dhs.append(dh)
            grads += [dW1, db1, dW2]
        _lib.check(lib.pf_mlp_train_bwd_batch(descs, n, _desc_buf(dev).data_ptr(), _stream()), "pf_mlp_train_bwd_batch")
        return (None, *dhs, *grads)


def mlp_fused(y, c: Tensor, td: int, cdiv: int, slopes, layers) -> Tensor:
    """layers: nn.Linear modules.  -> [rows, out]"""
    wb = []
    for lin in layers:
        wb += [lin.weight, lin.bias]
    return MlpFn.apply(y, c, td, cdiv, tuple(slopes), *wb)


class FoldWuFn(Function):
    """(W0 [o, 2 o, 1, 1], b0, W6 [o, k6, 1, 1], b6, Wout [o, ko, 1, 1], bout) -> (W0a W6, W0a b6 + b0, W0b Wout, W0b bout) in the
    shapes of W6 / b6 / Wout / bout: WeightEstimationUnit's first conv folded into the last linear layers of its two producers
    (csrc/train_glue.hip pf_fold_wu_fwd / _bwd: fixed summation order, one launch per direction)."""

    @staticmethod
    def forward(ctx, W0, b0, W6, b6, Wout, bout):
        lib = _lib.load()
        W0, b0, W6, b6, Wout, bout = (t.contiguous() for t in (W0, b0, W6, b6, Wout, bout))
        o = W0.shape[0]
        k6, ko = W6.numel() // o, Wout.numel() // o
        assert W0.numel() == 2 * o * o and W6.shape[0] == o and Wout.shape[0] == o
        W6f, b6f, Wof, bof = torch.empty_like(W6), torch.empty_like(b6), torch.empty_like(Wout), torch.empty_like(bout)
        _lib.check(lib.pf_fold_wu_fwd(W0.data_ptr(), b0.data_ptr(), W6.data_ptr(), b6.data_ptr(), Wout.data_ptr(), bout.data_ptr(),
                                      o, k6, ko, W6f.data_ptr(), b6f.data_ptr(), Wof.data_ptr(), bof.data_ptr(), _stream()),
                   "pf_fold_wu_fwd")
        ctx.save_for_backward(W0, W6, b6, Wout, bout)
        return W6f, b6f, Wof, bof

    @staticmethod
    def backward(ctx, dW6f, db6f, dWof, dbof):
        lib = _lib.load()
        W0, W6, b6, Wout, bout = ctx.saved_tensors
        o = W0.shape[0]
        k6, ko = W6.numel() // o, Wout.numel() // o
        z = lambda g, like: torch.zeros_like(like) if g is None else g.contiguous()
        dW6f, db6f, dWof, dbof = z(dW6f, W6), z(db6f, b6), z(dWof, Wout), z(dbof, bout)
        dW0, db0 = torch.empty_like(W0), torch.empty_like(b6)
        dW6, db6, dWout, dbout = torch.empty_like(W6), torch.empty_like(b6), torch.empty_like(Wout), torch.empty_like(bout)
        _lib.check(lib.pf_fold_wu_bwd(W0.data_ptr(), W6.data_ptr(), b6.data_ptr(), Wout.data_ptr(), bout.data_ptr(), o, k6, ko,
                                      dW6f.data_ptr(), db6f.data_ptr(), dWof.data_ptr(), dbof.data_ptr(), dW0.data_ptr(),
                                      db0.data_ptr(), dW6.data_ptr(), db6.data_ptr(), dWout.data_ptr(), dbout.data_ptr(),
                                      _stream()), "pf_fold_wu_bwd")
        return dW0, db0, dW6, db6, dWout, dbout


class BnMlpCfg(NamedTuple):                 # what BnMlpFn takes besides tensors with a gradient (built by bnmlp_fused)
    slope: float
    eps: float
    momentum: float
    run_means: list
    run_vars: list
    sync_bn: bool = False
    sum_inputs: bool = False          # PF_BNMLP_SUM_INPUTS: y[0] = xa + xb


class BnMlpFn(Function):
    """[Conv2d 1x1 + BatchNorm2d(train) + LeakyReLU] x 2 + Conv2d 1x1 on rows (DistanceEncoder / WeightEstimationUnit,
    interpflow.py:85-151) on cat[xa, xb] without building it: 3-4 launches forward, ~10 backward (csrc/train_bnmlp.hip).
    apply(xa, xb | None, cfg, W0, b0, W1, b1, W2, b2, gamma0, beta0, gamma1, beta1)"""

    @staticmethod
    def _desc(xa, xb, cfg, Ws):
        d = _lib.PfBnMlpTrain()
        d.rows, d.nl = xa.shape[0], len(Ws)
        d.kin0a, d.kin0b = xa.shape[1], (xb.shape[1] if xb is not None else 0)
        for l, w in enumerate(Ws):
            d.width[l] = w.shape[0]
            d.W[l] = w.data_ptr()
        d.slope, d.eps, d.momentum = cfg.slope, cfg.eps, cfg.momentum
        d.xa, d.xb = xa.data_ptr(), _ptr(xb)
        d.stat = _stat(xa.device).data_ptr()
        d.flags = (_lib.PF_TRAIN_DETERMINISTIC if deterministic() else 0) | (_lib.PF_BNMLP_SUM_INPUTS if cfg.sum_inputs else 0)
        if cfg.sync_bn:
            _attach_sync(d, xa.device)
        return d

    @staticmethod
    def forward(ctx, xa, xb, cfg, *prm):
        lib = _lib.load()
        xa = xa.contiguous()
        xb = xb.contiguous() if xb is not None else None
        Ws = [w.contiguous() for w in prm[0:6:2]]
        bs = [b.contiguous() for b in prm[1:6:2]]
        gb = [g.contiguous() for g in prm[6:10]]
        dev = xa.device
        f32 = dict(dtype=torch.float32, device=dev)
        d = BnMlpFn._desc(xa, xb, cfg, Ws)
        ys = [torch.empty((xa.shape[0], w.shape[0]), **f32) for w in Ws]
        affs = [torch.empty((4, Ws[l].shape[0]), **f32) for l in range(2)]
        for l in range(3):
            d.b[l], d.y[l] = bs[l].data_ptr(), ys[l].data_ptr()
        for l in range(2):
            d.gamma[l], d.beta[l], d.aff[l] = gb[2 * l].data_ptr(), gb[2 * l + 1].data_ptr(), affs[l].data_ptr()
            d.run_mean[l], d.run_var[l] = _ptr(cfg.run_means[l]), _ptr(cfg.run_vars[l])
        _lib.check(lib.pf_bnmlp_train_fwd(ctypes.byref(d), _stream()), "pf_bnmlp_train_fwd")
        ctx.cfg, ctx.has_b = cfg, xb is not None
        ctx.save_for_backward(xa, *(() if xb is None else (xb,)), *Ws, *ys, *affs, gb[0], gb[2])
        return ys[2]

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        sv = list(ctx.saved_tensors)
        xa = sv[0]
        xb = sv[1] if ctx.has_b else None
        o = 2 if ctx.has_b else 1
        Ws, ys, affs, gam = sv[o:o + 3], sv[o + 3:o + 6], sv[o + 6:o + 8], sv[o + 8:o + 10]
        dev = xa.device
        f32 = dict(dtype=torch.float32, device=dev)
        dout = dout.contiguous()
        d = BnMlpFn._desc(xa, xb, ctx.cfg, Ws)
        ds = [torch.empty_like(ys[0]), torch.empty_like(ys[1])]
        coefs = [torch.empty((2, Ws[l].shape[0]), **f32) for l in range(2)]
        dxa = torch.empty_like(xa) if ctx.needs_input_grad[0] else None
        dxb = torch.empty_like(xb) if (xb is not None and ctx.needs_input_grad[1]) else None
        dWs = [torch.empty_like(w) for w in Ws]
        dbs = [torch.empty((w.shape[0],), **f32) for w in Ws]
        dgs = [torch.empty((Ws[l].shape[0],), **f32) for l in range(2)]
        dbe = [torch.empty((Ws[l].shape[0],), **f32) for l in range(2)]
        for l in range(3):
            d.y[l], d.dW[l], d.db[l] = ys[l].data_ptr(), dWs[l].data_ptr(), dbs[l].data_ptr()
        for l in range(2):
            d.gamma[l], d.beta[l] = gam[l].data_ptr(), gam[l].data_ptr()
            d.aff[l], d.d[l], d.coef[l] = affs[l].data_ptr(), ds[l].data_ptr(), coefs[l].data_ptr()
            d.dgamma[l], d.dbeta[l] = dgs[l].data_ptr(), dbe[l].data_ptr()
        d.dout, d.dxa, d.dxb = dout.data_ptr(), _ptr(dxa), _ptr(dxb)
        need = lib.pf_bnmlp_train_ws_floats(ctypes.byref(d))
        ws = _ws(dev, need)
        d.ws, d.ws_floats = ws.data_ptr(), ws.numel()
        _lib.check(lib.pf_bnmlp_train_bwd(ctypes.byref(d), _stream()), "pf_bnmlp_train_bwd")
        if ctx.cfg.sum_inputs:                                           # y[0] = xa + xb: both inputs take d[0]; layer 0 has no weights of its own
            return (ds[0], ds[0], None, None, None, dWs[1], dbs[1], dWs[2], dbs[2], dgs[0], dbe[0], dgs[1], dbe[1])
        return (dxa, dxb, None, dWs[0], dbs[0], dWs[1], dbs[1], dWs[2], dbs[2], dgs[0], dbe[0], dgs[1], dbe[1])


def bnmlp_fused(mlp, xa: Tensor, xb=None, last=None, sum_inputs: bool = False) -> Tensor:
    """last = (W, b): other tensors for the last (linear) layer - the next module's first layer folded in (interp_weights);
    sum_inputs: layer 0 = xa + xb (its weights live folded in the two producers' last layers)."""
    convs, bns = [mlp[0], mlp[3], mlp[6]], [mlp[1], mlp[4]]
    cfg = BnMlpCfg(slope=0.01, eps=float(bns[0].eps), momentum=float(bns[0].momentum), run_means=[bn.running_mean for bn in bns],
                   run_vars=[bn.running_var for bn in bns], sync_bn=_sync_bn_active(), sum_inputs=bool(sum_inputs))
    prm = []
    for i, c in enumerate(convs):
        if i == 2 and last is not None:
            prm += [last[0], last[1]]
            continue
        if i == 0 and sum_inputs:                               # shapes only: no gradient comes back for these two
            prm += [c.weight.detach(), c.bias.detach()]
            continue
        prm += [c.weight, c.bias]
    for bn in bns:
        prm += [bn.weight, bn.bias]
    out = BnMlpFn.apply(xa, xb, cfg, *prm)
    _count_batches(bns)
    return out


class InterpWsumFn(Function):
    """Interpolation of the latent (interpflow.py:153-186, 312-318): w [T,8,ldw] logits (first R channels), z [B,N,3], idx8 int32
    [B,N,16|8] -> u [B, N R, 3], the rows flow g reads.  One launch forward (gather + softmax + weighted sum + layout), two
    backward (csrc/train_glue.hip); replaces GatherRowsFn + SoftmaxWsumFn + a transposing copy."""

    @staticmethod
    def forward(ctx, w, z, idx8, R, csr=None):
        lib = _lib.load()
        ctx.csr = csr                                          # deterministic mode: (off, edge) of pf_knn_csr(idx8)
        w, z, idx8 = w.contiguous(), z.contiguous(), idx8.contiguous()
        B, N, _ = z.shape
        T, K, ldw = w.shape
        a = torch.empty((T, K, R), dtype=torch.float32, device=w.device)
        u = torch.empty((B, N * R, 3), dtype=torch.float32, device=w.device)
        _lib.check(lib.pf_interp_wsum_fwd(w.data_ptr(), ldw, z.data_ptr(), idx8.data_ptr(), N, K, R, T, a.data_ptr(), u.data_ptr(),
                                          _stream()), "pf_interp_wsum_fwd")
        ctx.save_for_backward(a, z, idx8)
        ctx.dims = (N, K, R, ldw, T)
        return u

    @staticmethod
    def backward(ctx, du):
        lib = _lib.load()
        a, z, idx8 = ctx.saved_tensors
        N, K, R, ldw, T = ctx.dims
        du = du.contiguous()
        dw = torch.empty((T, K, ldw), dtype=torch.float32, device=du.device)
        dz = torch.empty_like(z)
        csr = ctx.csr if deterministic() else None
        if csr is not None:                                   # dz as an ordered gather over the sorted transposed lists
            _lib.check(lib.pf_interp_wsum_bwd_det(a.data_ptr(), z.data_ptr(), idx8.data_ptr(), du.data_ptr(), N, K, R, ldw, T, dw.data_ptr(),
                                                  dz.data_ptr(), csr[0].data_ptr(), csr[1].data_ptr(), _stream()), "pf_interp_wsum_bwd_det")
        else:
            _lib.check(lib.pf_interp_wsum_bwd(a.data_ptr(), z.data_ptr(), idx8.data_ptr(), du.data_ptr(), N, K, R, ldw, T, dw.data_ptr(),
                                              dz.data_ptr(), _stream()), "pf_interp_wsum_bwd")
        return dw, dz, None, None, None


def knn_csr_pair(idx: Tensor, K2: int):
    """knn_csr(idx) and knn_csr(idx[..., :K2].contiguous()) from one pass over idx (pf_knn_csr_pair: 4 launches instead of 8)."""
    B, N, K = idx.shape
    T = B * N
    dev = idx.device
    i32 = dict(dtype=torch.int32, device=dev)
    off, edge = torch.empty(T + 1, **i32), torch.empty(T * K, **i32)
    off2, edge2 = torch.empty(T + 1, **i32), torch.empty(T * K2, **i32)
    cnt = torch.empty(2 * ((T + 3) // 4 * 4), **i32)
    lib = _lib.load()
    _lib.check(lib.pf_knn_csr_pair(idx.data_ptr(), B, N, K, K2, off.data_ptr(), edge.data_ptr(), off2.data_ptr(), edge2.data_ptr(),
                                   cnt.data_ptr(), _stream()), "pf_knn_csr_pair")
    if deterministic():
        _lib.check(lib.pf_knn_csr_sort(off.data_ptr(), edge.data_ptr(), T, _stream()), "pf_knn_csr_sort")
        _lib.check(lib.pf_knn_csr_sort(off2.data_ptr(), edge2.data_ptr(), T, _stream()), "pf_knn_csr_sort")
    return (off, edge), (off2, edge2)


class ParamFanFn(torch.autograd.Function):
    """Identity on parameters that are used several times in one forward: `uses[i]` aliases of params[i].  Autograd sums the
    gradients of a tensor's uses with one small add launch per extra use - 54 of them per step for the flow blocks'
    parameters (ActNorm, W, the coupling net: f and g share them).  Here the sums of ALL parameters are two multi-tensor
    launches in this node's backward."""

    @staticmethod
    def forward(ctx, uses, *params):
        ctx.uses = uses
        outs = []
        for p, u in zip(params, uses):
            outs += [p.view_as(p) for _ in range(u)]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        groups, k = [], 0
        for u in ctx.uses:
            groups.append([g for g in grads[k:k + u] if g is not None])
            k += u
        acc = [gs[0] if gs else None for gs in groups]
        for level in range(1, max(ctx.uses)):
            sel = [i for i, gs in enumerate(groups) if len(gs) > level]
            if sel:
                summed = torch._foreach_add([acc[i] for i in sel], [groups[i][level] for i in sel])
                for i, t in zip(sel, summed):
                    acc[i] = t
        return (None, *acc)


class _Lin:
    """weight / bias holder with the attribute names of nn.Linear (for mlp_fused on parameter aliases)."""
    __slots__ = ("weight", "bias")

    def __init__(self, weight, bias=None):
        self.weight, self.bias = weight, bias
