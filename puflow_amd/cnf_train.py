"""The continuous model in train() mode: the three controllers of a taped integration as plans, the autograd nodes of
one block (`_FlowBlockFn`) and of the whole model (`_CnfPackFn`, `_CnfContextFn`, `_CnfIntegrateFn`), `flow_train`,
`forward_train` and the digest of the deferred controller's tables.  `cnf.py` holds the map of the four CNF modules."""
from __future__ import annotations

import functools
from typing import List, Optional

import torch
from torch import Tensor

from .cnf_engine import (_BlockTapeEngine, _deferred_steps_host, _DevicePack, _gauss_logp, _margin, _pack_keys, _pack_params,
                         _solver_error, _steps_host)
from .cnf_schedule import MAX_NUM_STEPS, PACK_ROW, _log_row, _row_key, schedule_step_lists
from .packing import CNF_CTX, CNF_GRAD, unpack_cnf_grads
from .train_perop import _gemm


# ---- the controllers of the train-mode forward -----------------------------------------------------------------------------------
class _EagerPlan:
    """The controller of a train-mode forward as an object: how the weights are packed (`pack`) and how one integration runs
    (`integrate` -> (state [rows,4], tape, what gives its (s, h) list on the host for `last_train_steps`)).  This one is the
    default: the taped device controller with a host read per batch of attempts (`tape_forward`), the pack's meta row read on
    the host; `net.tape_capacity` remembers how long a tape to allocate."""
    sticky_row: Optional[Tensor] = None                          # where the pack's status goes when it stays on the device
    read_meta = True                                             # end times and image scales as host floats: one read

    def __init__(self, net, dev: torch.device):
        self.caps = net.tape_capacity

    def pack(self, params, dev: torch.device, engs: list) -> None:
        """One pf_cnf_pack_blocks launch on the live parameters (sixteen per block); the blocks' engines are left in `engs`."""
        nb = len(params) // 16
        pack = _DevicePack([list(params[16 * j:16 * j + 16]) for j in range(nb)], dev, sticky=self.sticky_row, read_meta=self.read_meta)
        for j in range(nb):
            engs.append(_BlockTapeEngine(None, j, dev, pack=(pack, j), scratch=engs[0] if engs else None))
        self.bind(pack)

    def bind(self, pack: _DevicePack) -> None:
        pass

    def integrate(self, eng, i, R, reverse, x, c, e, ctx, d0c):
        y, tape = eng.tape_forward(i, x, c, e, R, reverse, self.caps.get((i, reverse), 32), ctx=ctx, d0c=d0c)
        steps = tape["steps"]
        self.caps[(i, reverse)] = _margin(len(steps))
        return y, tape, lambda: steps


class _DeferredPlan(_EagerPlan):
    """The deferred controller: the net's tape budgets, its log rows and sticky table.  An integration with a budget
    runs without a look at the controller - `check_train_logs` reads it later; one without goes through the host-read loop and
    learns its budget: attempts taken + a quarter + 2, steps + an eighth + 2.  The pack's status goes to the sticky table; its
    meta row is read only by a forward that still has such an integration to run, which needs the end times as host floats."""

    def __init__(self, net, dev: torch.device):
        self.logs, self.sticky = net._train_tables(dev)
        self.sticky_row = self.sticky[PACK_ROW]
        self.budget = net.tape_budget
        self.read_meta = any((i, r) not in self.budget for i in range(net.num_blocks) for r in (False, True))

    def integrate(self, eng, i, R, reverse, x, c, e, ctx, d0c):
        budget = self.budget.get((i, reverse))
        if budget is not None:
            k = _log_row(i, reverse)
            y, tape = eng.tape_forward_deferred(i, x, c, e, R, reverse, budget[0], budget[1], self.logs[k], self.sticky[k],
                                                ctx=ctx, d0c=d0c)
            return y, tape, functools.partial(_deferred_steps_host, tape)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"deferred CNF training: block {i} ({'g' if reverse else 'f'}) has no tape budget yet - run one "
                               "eager step before capturing (graphed_train_step's warm-up does)")
        y, tape = eng.tape_forward(i, x, c, e, R, reverse, 32, ctx=ctx, d0c=d0c)
        steps = tape["steps"]
        self.budget[(i, reverse)] = (tape["took"] + tape["took"] // 4 + 2, _margin(len(steps)))
        return y, tape, lambda: steps


class _SchedulePlan(_EagerPlan):
    """A frozen step schedule: the sticky table (the weight pack's status stays on the device, as under the deferred
    controller) and, once the weights are packed, the twelve step lists made on the device from the pack's end times.  ONE
    pf_cnf_replay launch per integration; no budgets, no log rows: a replay cannot fall short."""
    read_meta = False

    def __init__(self, net, dev: torch.device):
        self.sticky_row = net._train_tables(dev)[1][PACK_ROW]
        self.sdev = net._schedule_dev(dev)
        self.steps: Optional[Tensor] = None

    def bind(self, pack: _DevicePack) -> None:
        self.steps = self.sdev.lists(pack.meta[:, 0])

    def integrate(self, eng, i, R, reverse, x, c, e, ctx, d0c):
        k = _log_row(i, reverse)
        y, tape = eng.replay(i, x, self.steps[k, :self.sdev.n[k]], reverse, ctx, e, R, tape=True)
        return y, tape, functools.partial(_steps_host, tape["steps_dev"])


def _plan_of(net, dev: torch.device) -> _EagerPlan:
    if net.step_schedule is not None:
        return _SchedulePlan(net, dev)
    return _DeferredPlan(net, dev) if net.train_deferred else _EagerPlan(net, dev)


def digest_train_tables(logs: Tensor, sticky: Tensor, seen: Tensor, budget: dict):
    """What `PointInterpFlow.check_train_logs` makes of its one read.  logs [12, 16] float64 and sticky [13, 4] int32: the host
    copies of the controller rows and the sticky table (per row: runs, runs that were not clean, the last status, the most
    attempts / the pack's block); seen: the sticky table at the previous call; budget: `net.tape_budget`, updated in place.
    Since `seen`:
      * a weight pack with a status raises the host packers' ValueError;
      * an integration that ended with status 1 or 2 raises PuflowHipError, the eager path's messages - unless an integration
        BEFORE it in the forward fell short: its NaN output is what the later one choked on;
      * an integration that fell short - its attempts ran out (sticky status 4) or its tape filled (3) - gets that budget
        doubled (up to MAX_NUM_STEPS), if it has one.
    -> (how many integrations fell short, `last_skipped_steps`: the most new not-clean runs of any integration)."""
    new_bad = (sticky[:, 1] - seen[:, 1]).tolist()
    if new_bad[PACK_ROW]:
        _DevicePack.raise_status(int(sticky[PACK_ROW, 3]), int(sticky[PACK_ROW, 2]))
    short = 0
    for k in range(PACK_ROW):
        if not new_bad[k]:
            continue
        key, status = _row_key(k), int(sticky[k, 2])
        if status in (3, 4):
            short += 1
            a, c = budget.get(key, (0, 0))
            if status == 4:
                a = min(max(2 * a, 2), MAX_NUM_STEPS)
            else:
                c = min(max(2 * c, 2), MAX_NUM_STEPS)
                a = max(a, c)                                    # an accepted step is an attempt
            if key in budget:
                budget[key] = (a, c)
        elif not short:
            raise _solver_error(key[0], status, float(logs[k, 0]), float(logs[k, 1]))
    return short, max(new_bad[:PACK_ROW])


# ---- what the block backwards share ----------------------------------------------------------------------------------------------
def _ybar_of(gx: Optional[Tensor], gl: Optional[Tensor], rows: int, dev: torch.device) -> Tensor:
    """The cotangent of the state rows (x', delta logp) [rows,4] from the two outputs' cotangents."""
    ybar = torch.zeros((rows, 4), dtype=torch.float32, device=dev)
    if gx is not None:
        ybar[:, :3] = gx
    if gl is not None:
        ybar[:, 3] = gl
    return ybar


def _context_backward(ctxbar: Tensor, c: Tensor, Hplain: Tensor):
    """ctx = [1 | c] [hb | Hc]^T:  one GEMM for dc = ctxbar Hplain, one for d[hb | Hc] = ctxbar^T [1 | c] (column 0: the column
    sums).  -> (dc [T,cd], dH1 [288, 1 + cd])"""
    T, cd = c.shape
    c1 = torch.cat([torch.ones((T, 1), dtype=torch.float32, device=c.device), c], dim=1).contiguous()
    dH1 = torch.empty((CNF_CTX, cd + 1), dtype=torch.float32, device=c.device)
    _gemm(ctxbar, 1, CNF_CTX, c1, cd + 1, 1, dH1, cd + 1, None, CNF_CTX, cd + 1, T)
    dc = torch.empty((T, cd), dtype=torch.float32, device=c.device)
    _gemm(ctxbar, CNF_CTX, 1, Hplain, cd, 1, dc, cd, None, T, cd, CNF_CTX)
    return dc, dH1


def _dsqrt_end_time(ybar: Tensor, y0bar: Tensor, tape: dict, reverse: bool, sqrt_t: Tensor) -> Tensor:
    """sqrt_end_time's gradient.  End time T = sqrt_end_time^2 by the CONTINUOUS formula (not the derivative of the discrete
    scheme): the solution moves along the solver's derivative at the end whose time is T - the final state going forward, the
    start going backward."""
    dT = (ybar * tape["f_end"]).sum() if not reverse else (y0bar * tape["f_start"]).sum()
    return (dT * 2.0 * sqrt_t.detach()).reshape(sqrt_t.shape).to(sqrt_t.dtype)


class _FlowBlockFn(torch.autograd.Function):
    """(x, c, parameters of block i) -> (x', delta logp): `PointInterpFlow.flow_block`."""

    @staticmethod
    def forward(fctx, x, c, e, i, R, reverse, keys, record, opts, *params):
        on_device = opts["controller"] in ("deferred", "schedule")       # the pack's meta row stays on the device
        if on_device or opts["pack"] == "device":                # one launch on the live parameters (and one read of its meta row)
            by_key = dict(zip(keys, params))
            pack = _DevicePack([[by_key[k] for k in _pack_keys(i)]], x.device, sticky=opts["sticky"][PACK_ROW] if on_device else None,
                               read_meta=not on_device)
            eng = _BlockTapeEngine(None, i, x.device, pack=(pack, 0))
        else:                                                    # the numpy packers on a host copy: ~70 small uploads
            eng = _BlockTapeEngine({k: p.detach().cpu() for k, p in zip(keys, params)}, i, x.device)
        x32, c32, e32 = x.detach().float().contiguous(), c.detach().float().contiguous(), e.detach().float().contiguous()
        if opts["controller"] == "schedule":                     # one launch on a list made from the pack's end time, no read
            g = torch.tensor(opts["grid"], dtype=torch.float64)
            steps = schedule_step_lists((g[1:] - g[:-1])[None].to(x.device), torch.tensor([g.numel() - 2], device=x.device),
                                        torch.tensor([reverse], device=x.device), pack.meta[:1, 0])[0]
            y, tape = eng.replay(i, x32, steps, reverse, eng.context(i, c32), e32, R, tape=True)
            opts["tape"] = tape
        elif opts["controller"] == "deferred":
            k = _log_row(i, reverse)
            y, tape = eng.tape_forward_deferred(i, x32, c32, e32, R, reverse, opts["attempts"], opts["cap"], opts["logs"][k],
                                                opts["sticky"][k])
            opts["tape"] = tape
        elif opts["controller"] == "device":
            y, tape = eng.tape_forward(i, x32, c32, e32, R, reverse, opts["cap"])
        else:
            y, tape = eng.tape_forward_host(i, x32, c32, e32, R, reverse)
        fctx.eng, fctx.tape, fctx.args = eng, tape, (i, R, reverse, keys, x.dtype, c.dtype, opts["sweep"])
        fctx.save_for_backward(c32, e32, *params)
        record.extend(tape.get("steps", ()))                     # (a deferred tape's steps are on the device: `last_train_steps`)
        return y[:, :3].contiguous(), y[:, 3].contiguous()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, gx, gl):
        i, R, reverse, keys, xdt, cdt, sweep = fctx.args
        c, e, *params = fctx.saved_tensors
        eng, tape = fctx.eng, fctx.tape
        ybar = _ybar_of(gx, gl, tape["f_end"].shape[0], c.device)
        y0bar, grad, ctxbar = eng.tape_backward(i, tape, ybar, c, e, R, reverse, sweep)
        dc, dH1 = _context_backward(ctxbar, c, eng.Hplain)
        grads = unpack_cnf_grads(i, grad, dH1[:, 1:], dH1[:, 0])
        out = []
        for k, p in zip(keys, params):
            if k.endswith("sqrt_end_time"):
                out.append(_dsqrt_end_time(ybar, y0bar, tape, reverse, p))
            else:
                out.append(grads[k].reshape(p.shape).to(p.dtype))
        return (y0bar[:, :3].contiguous().to(xdt), dc.to(cdt), None, None, None, None, None, None, None, *out)


# ---- the train-mode forward: f, interpolation, g over all blocks ---------------------------------------------------
# Three kinds of autograd node.  `_CnfPackFn` stands between the parameters and everything that reads their packed form: per block
# it hands out two stand-in tensors whose GRADIENTS are what the kernels produce - the 4 900-float gradient record and
# d[hb | Hc] - and turns their sums over both directions into the parameters' gradients once.  `_CnfContextFn` is the context
# GEMM of a block, `_CnfIntegrateFn` one taped integration.  Autograd adds the two directions' ctxbar and records.
class _CnfPackFn(torch.autograd.Function):
    """(the sixteen parameters of every block) -> per block (grec [4900], h1 [288, 1 + cd]): stand-ins, their values are never
    read.  One pf_cnf_pack_blocks launch, as the plan packs (`_EagerPlan.pack`); the engines are left in `engs`."""

    @staticmethod
    def forward(fctx, engs, plan, *params):
        nb = len(params) // 16
        dev = params[0].device
        plan.pack(params, dev, engs)
        fctx.meta = [(p.shape, p.dtype) for p in params]
        fctx.set_materialize_grads(False)
        outs = [torch.empty(CNF_GRAD, dtype=torch.float32, device=dev) for _ in range(nb)]
        outs += [torch.empty((CNF_CTX, params[16 * j + 2].shape[1]), dtype=torch.float32, device=dev) for j in range(nb)]
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, *grads):
        nb = len(grads) // 2
        out = []
        for j in range(nb):
            grec, dH1 = grads[j], grads[nb + j]
            meta = fctx.meta[16 * j:16 * j + 16]
            if grec is None and dH1 is None:
                out += [None] * 16
                continue
            dev = (grec if grec is not None else dH1).device
            if grec is None:
                grec = torch.zeros(CNF_GRAD, dtype=torch.float32, device=dev)
            if dH1 is None:
                dH1 = torch.zeros((CNF_CTX, meta[2][0][1]), dtype=torch.float32, device=dev)
            g = unpack_cnf_grads(j, grec, dH1[:, 1:], dH1[:, 0])
            out += [g[k].reshape(s).to(dt) for k, (s, dt) in zip(_pack_keys(j)[:15], meta)] + [None]   # sqrt_end_time: _CnfIntegrateFn
        return (None, None, *out)


class _CnfContextFn(torch.autograd.Function):
    """ctx [T,288] = c Hc^T + hb of one block, once for f and g.  Backward, on the sum of both directions' ctxbar:
    `_context_backward`, d[hb | Hc] handed to `_CnfPackFn` through h1."""

    @staticmethod
    def forward(fctx, eng, i, c, h1):
        c32 = c.detach().float().contiguous()
        fctx.eng, fctx.cdt = eng, c.dtype
        fctx.save_for_backward(c32)
        return eng.context(i, c32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, ctxbar):
        (c,) = fctx.saved_tensors
        dc, dH1 = _context_backward(ctxbar.contiguous(), c, fctx.eng.Hplain)
        return None, None, dc.to(fctx.cdt), dH1


class _CnfIntegrateFn(torch.autograd.Function):
    """One taped integration of block i, run by the plan: (x [rows,3], ctx [T,288]) -> (x' [rows,3], delta logp [rows]).
    Backward: one launch sweeps the tape (`tape_backward`) -> xbar, this direction's ctxbar and gradient record (through grec to
    `_CnfPackFn`), and sqrt_end_time's gradient."""

    @staticmethod
    def forward(fctx, eng, i, R, reverse, plan, steps_out, c, d0c, e, x, ctx, grec, sqrt_t):
        y, tape, host_steps = plan.integrate(eng, i, R, reverse, x.detach().float().contiguous(), c, e, ctx.detach(), d0c)
        steps_out.append(host_steps)
        fctx.eng, fctx.tape, fctx.args = eng, tape, (i, R, reverse, x.dtype)
        fctx.save_for_backward(c, e, sqrt_t)
        return y[:, :3].contiguous(), y[:, 3].contiguous()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, gx, gl):
        i, R, reverse, xdt = fctx.args
        c, e, sqrt_t = fctx.saved_tensors
        tape = fctx.tape
        ybar = _ybar_of(gx, gl, tape["f_end"].shape[0], e.device)
        y0bar, grad, ctxbar = fctx.eng.tape_backward(i, tape, ybar, c, e, R, reverse, sweep="fused")
        return (None,) * 9 + (y0bar[:, :3].contiguous().to(xdt), ctxbar, grad, _dsqrt_end_time(ybar, y0bar, tape, reverse, sqrt_t))


def flow_train(net, xyz: Tensor, R: int, cs: List[Tensor], branch, noise: Optional[List[Tensor]] = None):
    """f over the blocks, the log-likelihood, the interpolation of the latent, g over the blocks in reverse: the flow part of the
    train-mode forward, differentiable in xyz, cs[i] [B,N,cd_i], the interpolation logits and the flow blocks' parameters.
    branch = (side stream | None, w [B N 8, >= R] logits, csr16, csr8, idx8): train_ops' interpolation branch.
    noise[i] [B,N,3]: block i's Hutchinson vector, used by f and g (default: torch.randn, drawn once per block).
    -> (x [B, N R, 3], logp); `net.last_train_steps`: the twelve recorded step lists, f's blocks 0 .. 5 then g's 5 .. 0."""
    from . import train_ops
    B, N, _ = xyz.shape
    T, nb = B * N, net.num_blocks
    dev = xyz.device
    if noise is None:
        noise = net.train_noise                                  # fixed vectors for every step (a reproducibility switch)
    if noise is None:
        noise = [torch.randn(B, N, 3, device=dev) for _ in range(nb)]
    es = [n.detach().reshape(T, 3).contiguous().float() for n in noise]
    engs: List[_BlockTapeEngine] = []
    params = [p for blk in net.flow_blocks for p in _pack_params(blk)]
    plan = _plan_of(net, dev)
    stand = _CnfPackFn.apply(engs, plan, *params)
    cflat, ctx, d0c = [], [], torch.empty(nb, dtype=torch.float64, device=dev)
    for i in range(nb):
        ci = cs[i].reshape(T, -1)
        cflat.append(ci.detach().float().contiguous())
        ctx.append(_CnfContextFn.apply(engs[i], i, ci, stand[nb + i]))
        if net.step_schedule is None:                            # (a replay takes no norm)
            engs[i].context_norm(cflat[i], d0c[i:i + 1])         # the context is a state of the reference's ODE: it enters the norms
    steps: list = []
    # ---- f + log-likelihood (oracle/cnf_ref.py::forward)
    p = xyz.reshape(T, 3)
    ldj = None
    for i in range(nb):
        p, dl = _CnfIntegrateFn.apply(engs[i], i, 1, False, plan, steps, cflat[i], d0c[i:i + 1], es[i], p, ctx[i], stand[i],
                                      net.flow_blocks[i].cnf.sqrt_end_time)
        ldj = dl if ldj is None else ldj + dl
    z = p.view(B, N, 3)
    logp = _gauss_logp(z, ldj.view(B, N).sum(dim=1))
    # ---- interpolation of the latent: the discrete training step's node
    _, w, _, csr8, idx8 = branch
    if train_ops._GLUE and R <= 8:
        train_ops._join_side(*branch)
        u = train_ops.InterpWsumFn.apply(w.view(T, 8, -1), z, idx8, R, csr8 if train_ops.deterministic() else None)
    else:
        u = train_ops._interp_latent(branch, z, R)
    # ---- g: the blocks in reverse, integrated backwards in time, the R rows of a point sharing its context row and vector
    u = u.reshape(T * R, 3)
    for i in reversed(range(nb)):
        u, _ = _CnfIntegrateFn.apply(engs[i], i, R, True, plan, steps, cflat[i], d0c[i:i + 1], es[i], u, ctx[i], stand[i],
                                     net.flow_blocks[i].cnf.sqrt_end_time)
    net._set_train_tapes(steps)
    return u.view(B, N * R, 3), logp


def forward_train(net, xyz: Tensor, upratio: int, noise: Optional[List[Tensor]] = None):
    """`PointInterpFlow.forward` in train() mode: kNN, the feature extractor and the interpolation weights exactly as the discrete
    model's training step runs them (train_ops._forward_train: side stream, prefold, `train_persistent`, `deterministic`,
    `train_dw_stream`), then `flow_train`.  Eager only - the taped integrations read their controllers - unless `net.train_deferred`
    is set and every integration has its budget (`tape_forward_deferred`): then nothing here reads the device."""
    from . import ops, train_ops
    train_ops.begin_forward(getattr(net, "deterministic", False), getattr(net, "train_dw_stream", False))
    try:
        with train_ops.sync_bn(getattr(net, "sync_batchnorm", False)):
            xyz = xyz.detach().contiguous().float()
            idx16, _ = ops.knn_idx32(xyz, xyz, 16)
            side = (train_ops._side_stream(xyz.device)
                    if getattr(net, "train_streams", True) and not train_ops._sync_bn_active() else None)
            if side is None:
                idx8, csr16, csr8 = train_ops._neighbour_lists(idx16)
            pre = (train_ops.ec_prefold(list(net.feat_convs), xyz, 16)
                   if (train_ops._FUSED and not train_ops._sync_bn_active()) else None)
            if side is not None:
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    idx8, csr16, csr8 = train_ops._neighbour_lists(idx16)
                    w = train_ops._interp_weights(net, xyz, idx8, csr8)
            else:
                w = train_ops._interp_weights(net, xyz, idx8, csr8)
            cs, _ = train_ops._features(net, xyz, idx16, csr16, pre)
            return flow_train(net, xyz, upratio, cs, (side, w, csr16, csr8, idx8), noise)
    finally:
        train_ops.end_forward()
