"""The training step: its switches and the train-mode forward of PointInterpFlow, assembled from the autograd nodes of the HIP
training kernels.  Four modules, each importing only the ones before it:
  train_state    per-(device, stream) caches, SyncBN callback, weight-gradient stream, per-call state; no autograd node
  train_perop    the per-op reference tier: one kernel pair per eager op (csrc/train_ops.hip, csrc/train_gemm.hip)
  train_fusedfn  the fused nodes (unit, MLP, flow block piece, flow chain); they read no switch
  train_ops      every switch and every function that reads one, forward_train and its stages; re-exports the names above
The tests assign to the switches on THIS module (train_ops._FUSED = False): a copy elsewhere would not see it.
HIP in training mode: every layer forward and backward, BatchNorm(train), ActNorm, the coupling / injector
algebra, kNN, the losses; torch: tensor re-layout and its autograd, parameter-only scalars, [B]-sized loss bookkeeping, Adam.
Activations are channels-last [rows, C] fp32 (rows = points or edges)."""
from __future__ import annotations

import os
from typing import List, Tuple

import torch
from torch import Tensor

from . import _lib
from .train_state import (_DW_PASS, _DW_STREAMS, _FC_IMG, _FC_SCOPE, _STAT, _SYNCW, _attach_sync, _count_batches, _dw_begin,  # noqa: F401
                          _multi_rank, _side_stream, _stream, _sync_bn_active, _sync_cb_impl, _sync_words, _zeros_kept, begin_forward,
                          check_persist_status, deterministic, end_forward, set_deterministic, sync_bn)
from .train_perop import (ARITH_BWD, ARITH_FWD, ActFn, ActNormFn, BatchSumFn, BnLreluFn, CoupleAddFn, CoupleInjectFn,  # noqa: F401
                          EdgeFeatureFn, GatherRowsFn, InjectInvFn, LinearFn, MaxPoolKFn, RepeatRowsFn, SoftmaxWsumFn, SyncBnLreluFn,
                          _det_inv3, _gemm, _mlp_bn, bn_lrelu, cond_net, cond_net_split, edgeconv_perop, knn_csr, linear)
from .train_fusedfn import (BnMlpCfg, BnMlpFn, CondNetBatchFn, CondNetStackFn, CoupleInject2Fn, EcCfg, EdgeConvUnitFn,  # noqa: F401
                            FanoutFn, FlowAffineFn, FlowChainFn, FlowParamsFn, FoldWuFn, InjectInv2Fn, InterpWsumFn, MergeBatchFn, MlpFn,
                            ParamFanFn, _Lin, bnmlp_fused, knn_csr_pair, mlp_fused)

_FUSED = os.environ.get("PF_TRAIN_FUSED", "1") != "0"
_FOLD_WU = os.environ.get("PF_TRAIN_FOLD_WU", "1") != "0"    # the weight unit's first conv folded into its producers (interp_weights); "0" = A/B reference
# persistent (grid-barrier) kernels of the training step (csrc/train_ec_fwd.hip: ec_fwdp_kernel, csrc/train_fused.hip: ec_bwdp_kernel): "1" = the main chain's EdgeConv
# units may use them (the default; the network attribute `train_persistent` and a device shared between processes switch them
# off per module), "0" = the per-layer kernels everywhere (the A/B reference).  Read once at import.
_PERSIST = os.environ.get("PF_TRAIN_PERSIST", "1") != "0"
# all flow blocks of a direction as one autograd node (FlowChainFn); "0" = one node per block piece (the A/B reference)
_CHAIN = os.environ.get("PF_TRAIN_CHAIN", "1") != "0"
# chains of one-element torch launches as fused kernels (csrc/train_glue.hip: interpolation of the latent, the log-likelihood
# inside the f chain, the loss head of loss.PuganLossFn); "0" = the torch expressions (the A/B reference)
_GLUE = os.environ.get("PF_TRAIN_GLUE", "1") != "0"
# References of three bit-for-bit / rounding-level comparisons in tests/test_gpu_train.py, which assigns False to them: not
# environment switches, and nothing else sets them
_PREFOLD = True      # the feature units' folded weights in one launch at the top of the forward (ec_prefold); False: one per unit
_TAP = True          # a unit's output gradient from its merge unit added inside the next unit's dx GEMM; False: autograd's add launch
_FANOUT = True       # the four gradients of the flattened conditioning features summed in one launch (FanoutFn); False: autograd's adds


def edgeconv_train(p, x: Tensor, idx: Tensor, pooling: bool = True, csr=None, persistent: bool = False, prefold=None,
                   tap: bool = False) -> Tensor:
    """FeatureExtractUnit in train mode (interpflow.py:234-248): the fused unit where its kernels take the shape, else per op."""
    if _FUSED and _ec_fused_supported(p, x, idx, pooling):
        return edgeconv_train_fused(p, x, idx, pooling, csr, persistent, prefold=prefold, tap=tap)   # tap: -> (out, x again)
    return edgeconv_perop(p, x, idx, pooling)


def _ec_fused_supported(p, x: Tensor, idx: Tensor, pooling: bool) -> bool:
    """Shapes the fused unit kernels are built for (csrc/train_fused.hip: pf_ec_dims); anything else takes the per-op path."""
    g, nconv, odim = p.convs[0][0].weight.shape[0], len(p.convs), p.conv_out.weight.shape[0]
    B, N, _ = x.shape
    K = idx.shape[-1]
    return (g in (8, 16, 32) and 1 <= nconv <= 8 and g * nconv in (32, 64, 128) and odim % 16 == 0 and 16 <= odim <= 128
            and (B * N * K) % 16 == 0 and (K == 16 or not pooling))


def ec_prefold(units, x0: Tensor, K: int):
    """Folded edge-feature weights (Wpq, bpq) of a CHAIN of pooled units (unit i + 1 reads unit i's output) in one launch
    (pf_ec_train_fold_batch) -> one pair per unit for `edgeconv_train_fused(..., prefold=)`, or None where the fused path
    does not apply.  Parameters only: valid until the next optimizer update."""
    if not (_FUSED and _PREFOLD) or not 1 <= len(units) <= 8:
        return None
    B, N, C = x0.shape
    if (B * N * K) % 16:
        return None
    dev = x0.device
    f32 = dict(dtype=torch.float32, device=dev)
    descs = (_lib.PfEcTrain * len(units))()
    outs = []
    for k, p in enumerate(units):
        convs = [seq[0] for seq in p.convs] + [p.conv_out]
        g, nconv, odim = convs[0].weight.shape[0], len(p.convs), p.conv_out.weight.shape[0]
        if g not in (8, 16, 32) or g * nconv not in (32, 64, 128) or odim % 16 or not 16 <= odim <= 128 or K != 16:
            return None
        if any(c.weight.dtype != torch.float32 or not c.weight.is_contiguous() or c.bias is None for c in convs):
            return None
        if convs[0].weight.reshape(g, -1).shape[1] != 3 * C:
            return None
        S = g * nconv + odim
        Wpq, bpq = torch.empty((2 * S, C), **f32), torch.empty((2 * S,), **f32)
        d = _lib.PfEcTrain()
        d.B, d.N, d.K, d.C, d.growth, d.nconv, d.odim, d.pooling = B, N, K, C, g, nconv, odim, 1
        for t, c in enumerate(convs):
            d.W[t], d.bias[t] = c.weight.data_ptr(), c.bias.data_ptr()
        d.Wpq, d.bpq = Wpq.data_ptr(), bpq.data_ptr()
        descs[k] = d
        outs.append((Wpq, bpq))
        C = odim
    _lib.check(_lib.load().pf_ec_train_fold_batch(descs, len(units), _stream()), "pf_ec_train_fold_batch")
    return outs


def edgeconv_train_fused(p, x: Tensor, idx: Tensor, pooling: bool = True, csr=None, persistent: bool = False, out=None,
                         prefold=None, tap: bool = False) -> Tensor:
    """out = (W, b): other tensors for conv_out (the next module's first layer folded in, interp_weights).
    prefold = (Wpq, bpq) from `ec_prefold`.  tap: return (result, x) - an alias of x for x's other consumer, whose gradient the
    unit's backward then adds inside its dx GEMM (EdgeConvUnitFn)."""
    convs = [seq[0] for seq in p.convs] + [p.conv_out]
    bns = [seq[1] for seq in p.convs]
    g, nconv, odim = convs[0].weight.shape[0], len(bns), p.conv_out.weight.shape[0]
    ws, bs = [c.weight for c in convs], [c.bias for c in convs]
    sync = _sync_bn_active()
    cfg = EcCfg(K=idx.shape[-1], growth=g, nconv=nconv, odim=odim, pooling=bool(pooling), slope=0.05, eps=float(bns[0].eps),
                momentum=float(bns[0].momentum), run_means=[bn.running_mean for bn in bns], run_vars=[bn.running_var for bn in bns],
                csr=csr, persistent=bool(persistent) and _PERSIST and not sync, sync_bn=sync)
    if out is not None:
        ws[-1], bs[-1] = out
        cfg = cfg._replace(dw_inline=True)
    else:
        cfg = cfg._replace(prefold=prefold, tap=bool(tap) and x.requires_grad)
    res = EdgeConvUnitFn.apply(x, idx, cfg, *ws, *bs, *[bn.weight for bn in bns], *[bn.bias for bn in bns])
    _count_batches(bns)
    return res


def cond_net_fused(net, y, c: Tensor, td: int, cdiv: int) -> Tensor:
    """LinearA1D on cat[y[..., :td], c[row // cdiv]] in one launch (csrc/train_mlp.hip); -> [rows, dout].
    net: the LinearA1D module, or its three linear layers (weight / bias holders) as a list."""
    L = net if isinstance(net, (list, tuple)) else [net.layers[0], net.layers[2], net.layers[4]]
    if cdiv not in (1, 2, 4, 8, 16):                   # the kernel shares a conditioning row between 2^k replicas only
        c, cdiv = RepeatRowsFn.apply(c, cdiv), 1
    return mlp_fused(y, c, td, cdiv, (0.01, 0.01), L)


def _block_params(net) -> List[Tensor]:
    """logs, bias, W, w0, w2, b2, w4, b4 of every flow block: the parameters f and g share."""
    plist = []
    for blk in net.flow_blocks:
        L = blk.coupling1.bias_net.layers
        plist += [blk.actnorm.logs, blk.actnorm.bias, blk.permutate1.permutater.W, L[0].weight, L[2].weight, L[2].bias,
                  L[4].weight, L[4].bias]
    return plist


def _flow_param_aliases(net):
    """Per flow block: aliases of the parameters f and g share (ParamFanFn) - dict of lists indexed by use."""
    plist = _block_params(net)
    flat = list(ParamFanFn.apply((3, 2, 2, 2, 2, 2, 2, 2) * len(net.flow_blocks), *plist))
    out, k = [], 0
    for _ in net.flow_blocks:
        a = {}
        for name, u in (("logs", 3), ("bias", 2), ("W", 2), ("w0", 2), ("w2", 2), ("b2", 2), ("w4", 2), ("b4", 2)):
            a[name] = flat[k:k + u]
            k += u
        a["net"] = [[_Lin(a["w0"][j]), _Lin(a["w2"][j], a["b2"][j]), _Lin(a["w4"][j], a["b4"][j])] for j in range(2)]
        out.append(a)
    return out


def _flow_chain_params(net):
    """The eight parameters of every flow block, twice (f and g share them): two alias lists for FlowChainFn."""
    plist = _block_params(net)
    flat = list(ParamFanFn.apply(tuple(2 for _ in plist), *plist))
    return flat[0::2], flat[1::2]


def forward_train(net, xyz: Tensor, upratio: int) -> Tuple[Tensor, Tensor]:
    """PointInterpFlow.forward in train() mode (interpflow.py:327-337) with gradients."""
    begin_forward(getattr(net, "deterministic", False), getattr(net, "train_dw_stream", False))
    try:
        with sync_bn(getattr(net, "sync_batchnorm", False)):
            return _forward_train(net, xyz, upratio)
    finally:
        end_forward()


def _forward_train(net, xyz: Tensor, upratio: int) -> Tuple[Tensor, Tensor]:
    from . import ops
    xyz = xyz.detach().contiguous().float()
    idx16, _ = ops.knn_idx32(xyz, xyz, 16)
    # ---- interpolation weights (interpflow.py:85-151): a function of xyz and the neighbour lists only, independent of the
    # feature extractor / flow f chain that follows.  At 32 x 256 points no kernel of the step fills the chip, so this branch
    # (two BatchNorm MLPs + one EdgeConv unit, forward and - autograd keeps the stream - backward) runs on a side stream
    # beside the main chain; inside a captured step it becomes a parallel branch of the graph.  Scratch buffers are per
    # (device, stream) (_ws / _stat), results are identical to the one-stream order (net.train_streams = False).
    # With a side stream the neighbour lists are made there too, off the chain knn -> fold -> first unit
    side = _side_stream(xyz.device) if getattr(net, "train_streams", True) and not _sync_bn_active() else None
    if side is None:
        idx8, csr16, csr8 = _neighbour_lists(idx16)
    # folded edge-feature weights of the six feature units: parameters only - one launch here instead of one per unit
    # (the fused kernels also run under SyncBN - they defer a layer's statistics to an all-reduce - but without the prefold)
    pre = ec_prefold(list(net.feat_convs), xyz, 16) if (_FUSED and not _sync_bn_active()) else None
    if side is not None:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            idx8, csr16, csr8 = _neighbour_lists(idx16)
            w = _interp_weights(net, xyz, idx8, csr8)
    else:
        w = _interp_weights(net, xyz, idx8, csr8)
    branch = (side, w, csr16, csr8, idx8)                       # the arguments of _join_side

    cs, cflat_m = _features(net, xyz, idx16, csr16, pre)
    R, nb = upratio, net.num_blocks
    chain = (_CHAIN and _FUSED and nb <= 8 and R in (1, 2, 4, 8, 16)
             and all(b.actnorm.is_inited for b in net.flow_blocks) and all(c.shape[-1] in (32, 64, 128) for c in cs)
             and all(b.coupling1.bias_net.layers[2].weight.shape == (64, 64) for b in net.flow_blocks))
    # ActNorm's data-dependent init needs each block's input on the host side of the chain: the first step takes the per-block path
    if chain:
        return _flow_chain(net, xyz, R, cs, cflat_m, branch)
    return (_flow_blocks if _FUSED else _flow_blocks_perop)(net, xyz, R, cs, branch)


def _neighbour_lists(idx16: Tensor):
    """-> (idx8, csr16, csr8) on the current stream.  idx8: the 8 nearest of the 16 - only the interpolation branch (and, after the
    join, the latent's interpolation) reads them.  csr*: the transposed neighbour lists (8 small launches, ~55 us) - only the
    BACKWARD of the fused EdgeConv units reads them."""
    idx8 = idx16[..., :8].contiguous()
    csr16, csr8 = knn_csr_pair(idx16, 8) if _FUSED else (None, None)
    return idx8, csr16, csr8


def _join_side(side, w, csr16, csr8, idx8) -> None:
    """The calling stream waits for the interpolation branch and takes over what was allocated on the side stream."""
    if side is None:
        return
    cur = torch.cuda.current_stream()
    cur.wait_stream(side)
    w.record_stream(cur)
    for t in (csr16 or ()) + (csr8 or ()) + (idx8,):
        t.record_stream(cur)


def _interp_weights(net, xyz: Tensor, idx8: Tensor, csr8) -> Tensor:
    """The interpolation logits [E8, 32] of net.interp (interpflow.py:85-151) on the current stream."""
    B, N, _ = xyz.shape
    ip = net.interp
    fd = torch.empty((B * N * 8, 10), dtype=torch.float32, device=xyz.device)        # inputs only: no gradient
    _lib.check(_lib.load().pf_dist_feature(xyz.data_ptr(), idx8.data_ptr(), B, N, 8, fd.data_ptr(), _stream()), "pf_dist_feature")
    de, wu, fc = ip.knn_context.distance_encoder.mlp, ip.weight_unit.mlp, ip.knn_context.feat_conv
    if (_FUSED and _FOLD_WU and _ec_fused_supported(fc, xyz, idx8, False)
            and wu[0].weight.shape[0] == de[6].weight.shape[0] == fc.conv_out.weight.shape[0] == wu[0].weight.shape[1] // 2):
        # The weight unit's first conv sees cat[d, feat] with NO nonlinearity after the producers' last (linear) layers
        # (interpflow.py:134,144-146), so W0 [d; feat] + b0 = (W0a W6) a2 + (W0b Wout) e + (W0a b6 + W0b bout + b0): the
        # producers' last layers run with the PRODUCT weights and emit the two halves of the pre-BatchNorm output directly;
        # the first layer of the weight unit is their sum (PF_BNMLP_SUM_INPUTS) - two [E8, 128] x [128, 128] products per
        # direction less, same function.  The products and their chain rule back to W0, W6, Wout and the three biases are one
        # small launch each (FoldWuFn; the same algebra as the eval path's packing.fold_state_dict).
        W6f, b6f, Wof, bof = FoldWuFn.apply(wu[0].weight, wu[0].bias, de[6].weight, de[6].bias, fc.conv_out.weight,
                                            fc.conv_out.bias)
        d = bnmlp_fused(de, fd, last=(W6f, b6f))
        feat = edgeconv_train_fused(fc, xyz, idx8, False, csr8, False, out=(Wof, bof))
        return bnmlp_fused(wu, d, feat, sum_inputs=True)
    d = bnmlp_fused(de, fd) if _FUSED else _mlp_bn(de, fd)
    feat = edgeconv_train(fc, xyz, idx8, pooling=False, csr=csr8)                            # d, feat: [E8,128]
    if _FUSED:
        return bnmlp_fused(wu, d, feat)                       # on cat[d, feat] (interpflow.py:146) without building it
    return _mlp_bn(wu, torch.cat([d, feat], dim=1))           # [E8,32]


def _features(net, xyz: Tensor, idx16: Tensor, csr16, pre):
    """The feature extractor: EdgeConv unit i on unit i - 1's output, a FeatMergeUnit on each unit's output.
    -> (cs: the conditioning features [B, N, cd_i] per block, cflat_m: the flat tensor they are views of | None)
    (the merge units on a second side stream beside EdgeConv unit i + 1 were tried: 7.65 -> 8.35 ms per captured step - six
    fork / join pairs of tiny kernels cost more in graph dependencies than their overlap returns)"""
    B, N, _ = xyz.shape
    # all merge units in one batched launch (MergeBatchFn) after the last unit; one launch per unit for more than 16 blocks
    batch_merge = _FUSED and net.num_blocks <= 16
    # the main chain's units may run as persistent grid-barrier launches: nothing else with a grid barrier runs beside them
    # (the side stream's interpolation unit keeps the per-layer kernels; the EMD auction starts after the forward)
    # An explicit opt-in: TrainerModule sets `network.train_persistent` from its configuration (on, unless the
    # device is shared: cfg.emd_workgroups == 1 / cfg.persistent_kernels = False); a bare PointInterpFlow.train() forward on a
    # GPU it may share with another process keeps the per-layer kernels - a grid barrier whose workgroups are not all resident
    # spins for seconds before its bounded time-out makes the output NaN.
    persistent = getattr(net, "train_persistent", False)
    cs: List[Tensor] = []
    hs_all: List[Tensor] = []
    h = xyz
    for i in range(net.num_blocks):
        h = edgeconv_train(net.feat_convs[i], h, idx16, csr=csr16, persistent=persistent,
                           prefold=pre[i] if pre is not None else None, tap=_TAP and batch_merge and i > 0)
        if isinstance(h, tuple):                                  # (output, the input again): the merge unit reads the alias, so
            h, hs_all[i - 1] = h                                  # its gradient reaches the previous unit through THIS unit's dx GEMM
        m = net.merge_convs[i]
        if batch_merge:
            hs_all.append(h)
        elif _FUSED:
            cs.append(mlp_fused(None, h, 0, 1, (0.0,), [m.conv1, m.conv2]).view(B, N, -1))
        else:
            cs.append(linear(ActFn.apply(linear(h, m.conv1.weight, m.conv1.bias), 0.0), m.conv2.weight))
    if not hs_all:
        return cs, None
    mp = []
    for m in net.merge_convs:
        mp += [m.conv1.weight, m.conv1.bias, m.conv2.weight]
    cflat_m = MergeBatchFn.apply(len(hs_all), *hs_all, *mp)
    off = 0
    for m in net.merge_convs:
        cd = m.conv2.weight.shape[0]
        cs.append(cflat_m[off:off + B * N * cd].view(B, N, cd))
        off += B * N * cd
    return cs, cflat_m


def _injector_params(net) -> List[Tensor]:
    """The injector nets (s, t) of every block: functions of cs[i] only - one batched launch (and shared by f and g)."""
    st_prm = []
    for blk in net.flow_blocks:
        for cn in (blk.coupling2.scale_net, blk.coupling2.bias_net):
            L = cn.layers
            st_prm += [L[0].weight, L[2].weight, L[2].bias, L[4].weight, L[4].bias]
    return st_prm


def _flow_chain(net, xyz: Tensor, R: int, cs, cflat_m, branch) -> Tuple[Tensor, Tensor]:
    """f, interpolation, g with every flow block of a direction in one autograd node (csrc/train_flowchain.hip): the default."""
    B, N, _ = xyz.shape
    _, w, _, csr8, idx8 = branch
    st_prm = _injector_params(net)
    pf, pg = _flow_chain_params(net)
    ccs = tuple(int(c.shape[-1]) for c in cs)
    cflat = cflat_m if cflat_m is not None else torch.cat([c.reshape(-1) for c in cs])       # one tensor for its consumers
    cflat_t = None
    cflat_f = cflat_g = cflat
    if _FANOUT:                                                   # their four gradients: one launch (FanoutFn)
        cflat, cflat_t, cflat_f, cflat_g = FanoutFn.apply(4, cflat)
    st = CondNetStackFn.apply(ccs, B * N, cflat, cflat_t, *st_prm)
    if _GLUE and net.num_blocks < 8:
        z, logp1 = FlowChainFn.apply(0, 1, float(N), ccs, xyz, cflat_f, st, B, *pf)     # log-likelihood from the kernel's epilogue
        logp = logp1.view(())
    else:
        z, ssum, ld = FlowChainFn.apply(0, 1, float(N), ccs, xyz, cflat_f, st, 0, *pf)
        logp = -(BatchSumFn.apply(z, 1).mean() + ld.sum() - ssum.sum() / B)
    if _GLUE and R <= 8:
        _join_side(*branch)
        u = InterpWsumFn.apply(w.view(B * N, 8, -1), z, idx8, R, csr8 if deterministic() else None)
    else:
        u = _interp_latent(branch, z, R)
    x = FlowChainFn.apply(1, R, float(N), ccs, u, cflat_g, st, 0, *pg)
    return x, logp


def _interp_latent(branch, z: Tensor, R: int) -> Tensor:
    """Join the interpolation branch (its weights w were started on the side stream before the feature extractor), then
    u [B, N R, 3] = the softmax(w)-weighted sums of z's 8 neighbours, per op."""
    B, N, _ = z.shape
    _, w, _, _, idx8 = branch
    _join_side(*branch)
    zj = GatherRowsFn.apply(z, idx8)                              # [E8,3]
    fz = SoftmaxWsumFn.apply(w.view(B * N, 8, -1), zj.view(B * N, 8, 3), R)      # [T,3,R]
    return fz.transpose(1, 2).reshape(B, N * R, 3)


def _actnorm_init(an, p: Tensor) -> None:
    """ActNorm's data-dependent init from its first input (normalize.py:45-54)."""
    if not an.is_inited:
        with torch.no_grad():
            an.bias.data.copy_(-torch.mean(p.detach(), dim=(0, 1), keepdim=True))
            an.logs.data.copy_(-torch.log(torch.std(p.detach(), dim=(0, 1), keepdim=True) + 1e-6))
            an.is_inited = True


def _flow_blocks(net, xyz: Tensor, R: int, cs, branch) -> Tuple[Tensor, Tensor]:
    """f, interpolation, g block by block, one fused node per block piece (csrc/train_flow.hip, train_mlp.hip): the first step
    (ActNorm's init), shapes the chain kernels do not take, and _CHAIN off."""
    B, N, _ = xyz.shape
    nb = net.num_blocks
    # injector (s, t) per block: functions of cs[i] only, one batched launch, shared by f and g
    st_all = CondNetBatchFn.apply(tuple(i for i in range(nb) for _ in range(2)), *cs, *_injector_params(net))
    # ---- f + log-likelihood
    p = xyz
    torch.zeros(B, device=xyz.device)     # ldj's zero-fill, read by the per-op path only: kept, the launch list is as it was
    st_nets, winvs, lds, ssums = [], [], [], []
    alias = _flow_param_aliases(net)                              # aliases share the parameters' storage (ActNorm init below)
    for i in range(nb):
        _actnorm_init(net.flow_blocks[i].actnorm, p)
        td = 1 if i % 2 == 0 else 2
        al = alias[i]
        Winv, ld = FlowParamsFn.apply(al["W"][0], al["logs"][0], float(N))    # W^-1 and (sum(logs) + log|det W|) N (permutate.py:119)
        winvs.append(Winv)
        lds.append(ld)
        y = FlowAffineFn.apply(p, None, 0, al["logs"][1], al["bias"][0], al["W"][1], 0)    # ActNorm + einsum 'ij,bnj->bni' (permutate.py:118)
        o = cond_net_fused(al["net"][0], y, cs[i], td, 1).view(B, N, -1)
        st_nets.append((st_all[2 * i].view(B, N, -1), st_all[2 * i + 1].view(B, N, -1)))
        p, ssum = CoupleInject2Fn.apply(y, o, *st_nets[i], td)
        ssums.append(ssum)
    # -mean_b(gauss_b + sum_i (ld_i - sum(s_i)[b])) with the batch mean taken once, over scalars: the same number as the
    # reference's per-sample bookkeeping (interpflow.py:327-337, probs.py:73-93)
    logp = -(BatchSumFn.apply(p, 1).mean() + torch.cat(lds).sum() - torch.cat(ssums).sum() / B)
    u = _interp_latent(branch, p, R)
    # ---- g (exact inverse); s, t of the original point: row // R
    for i in reversed(range(nb)):
        td = 1 if i % 2 == 0 else 2
        al = alias[i]
        v = InjectInv2Fn.apply(u, *st_nets[i], R)
        o = cond_net_fused(al["net"][1], v, cs[i], td, R).view(B, N * R, -1)
        u = FlowAffineFn.apply(v, o, td, al["logs"][2], al["bias"][1], winvs[i], 1)    # permutate.py:123-124
    return u, logp


def _flow_blocks_perop(net, xyz: Tensor, R: int, cs, branch) -> Tuple[Tensor, Tensor]:
    """_flow_blocks with one kernel pair per eager op (train_perop): _FUSED off, the reference of the fused tiers."""
    B, N, _ = xyz.shape
    # ---- f + log-likelihood
    p = xyz
    ldj = torch.zeros(B, device=xyz.device)
    st_nets: List[Tuple[Tensor, Tensor]] = []                      # injector (s, t) per block: functions of cs[i] only, shared by f and g
    cparts: List[Tensor] = []                                      # c-columns of coupling1's first layer, likewise
    for i in range(net.num_blocks):
        blk = net.flow_blocks[i]
        an = blk.actnorm
        _actnorm_init(an, p)
        W = blk.permutate1.permutater.W
        td = 1 if i % 2 == 0 else 2
        y = linear(ActNormFn.apply(p, an.logs, an.bias, 0), W)     # einsum 'ij,bnj->bni' (permutate.py:118)
        ld = (torch.sum(an.logs) + torch.log(torch.abs(_det_inv3(W)[0]))) * N        # parameter-only scalars (permutate.py:119)
        cparts.append(linear(cs[i], blk.coupling1.bias_net.layers[0].weight[:, td:]))
        o = cond_net_split(blk.coupling1.bias_net, y[..., :td], cparts[i])
        s = cond_net(blk.coupling2.scale_net, cs[i])
        t = cond_net(blk.coupling2.bias_net, cs[i])
        st_nets.append((s, t))
        p = CoupleInjectFn.apply(y, o, s, t, td)
        ldj = ldj + ld - BatchSumFn.apply(s, 0)
    logp = -torch.mean(BatchSumFn.apply(p, 1) + ldj)
    u = _interp_latent(branch, p, R)
    # ---- g (exact inverse); injector nets are evaluated per ORIGINAL point and replicated
    for i in reversed(range(net.num_blocks)):
        blk = net.flow_blocks[i]
        td = 1 if i % 2 == 0 else 2
        s = RepeatRowsFn.apply(st_nets[i][0], R)                   # same nets, same input as in f: evaluated once (autograd sums both uses)
        t = RepeatRowsFn.apply(st_nets[i][1], R)
        v = InjectInvFn.apply(u, s, t)
        o = cond_net_split(blk.coupling1.bias_net, v[..., :td], RepeatRowsFn.apply(cparts[i], R))
        u = linear(CoupleAddFn.apply(v, o, td), _det_inv3(blk.permutate1.permutater.W)[1])   # permutate.py:123-124 (3x3 inverse: parameter-only)
        u = ActNormFn.apply(u, blk.actnorm.logs, blk.actnorm.bias, 1)
    return u, logp
