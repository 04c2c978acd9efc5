"""The continuous model's kernels and their drivers: the solver constants, the device weight packer (`_DevicePack`), the launch
wrappers of csrc/cnf.hip, cnf_replay.hip and cnf_bwd.hip with the look-per-batch controller loop (`_CnfKernels`), the inference
plan (`_CnfEngine`) and the taped engine of one block (`_BlockTapeEngine`).  `cnf.py` holds the map of the four CNF modules."""
from __future__ import annotations

import ctypes
import math
import os
from typing import Callable, List, Optional

import torch
from torch import Tensor

from . import _lib
from .cnf_schedule import MAX_NUM_STEPS
from .interpflow import NUM_BLOCKS, _Engine
from .packing import CNF_CTX, CNF_GRAD, CNF_REC, cnf_hyper_matrix, cnf_split_ok, pack_cnf_block, pack_cnf_context
from .train_perop import _gemm
from .weights import state_dict_spec

ATOL = RTOL = 1e-5                       # continuous/interpflow.py:28
SAFETY, IFACTOR, DFACTOR, ORDER = 0.9, 10.0, 0.2, 5
DP_ALPHA = [1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0]
DP_BETA = [
    [1 / 5],
    [3 / 40, 9 / 40],
    [44 / 45, -56 / 15, 32 / 9],
    [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
    [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
    [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84],
]


def _margin(n: int) -> int:
    """A budget from what a run took: that + an eighth + 2 (tape steps to allocate, attempts to enqueue blind)."""
    return n + n // 8 + 2


def _rows3(x: Tensor) -> Tensor:
    """x [rows, >= 3] as the kernels read it: fp32 rows 3 or 4 floats apart (a previous block's state is taken as it lies)."""
    if x.dtype != torch.float32 or x.stride(1) != 1 or x.stride(0) not in (3, 4):
        x = x.float().contiguous()[:, :3].contiguous()
    return x


def _steps_host(steps_dev: Tensor) -> list:
    """A device step list [n, 2] as host floats [(s, h)]: one read."""
    return [(float(s), float(h)) for s, h in steps_dev.cpu().tolist()]


def _deferred_steps_host(tape: dict) -> list:
    """The valid prefix of a deferred tape's step list (none of it when the run did not end cleanly): two reads."""
    ctl = tape["log"].cpu()
    n = int(ctl[6]) if (ctl[5] != 0 and ctl[9] == 0) else 0
    return _steps_host(tape["steps_dev"][:n])


def _gauss_logp(z: Tensor, ldj: Tensor) -> Tensor:
    """z [B,N,3] latent, ldj [B] = sum of delta logp per cloud -> the mean negative log-likelihood under N(0, I)."""
    return -torch.mean(torch.sum(-0.5 * (z ** 2 + math.log(2 * math.pi)), dim=(1, 2)) - ldj)


def _solver_error(block: int, status: int, t: float, dt: float) -> "_lib.PuflowHipError":
    """The controller's error states as the exception to raise: 1 = non-finite error norm, otherwise (2) dt underflow.
    torchdiffeq raises here too ('underflow in dt', NaN propagates into dt): without these guards a NaN error norm makes every
    comparison False - no step is ever accepted and dt grows tenfold per attempt, forever."""
    if status == 1:
        return _lib.PuflowHipError(f"dopri5: non-finite error norm in block {block} at t = {t:g} (NaN / inf in the input, "
                                   "the weights or the state)")
    return _lib.PuflowHipError(f"dopri5: underflow in dt ({dt:g}) at t = {t:g}, block {block}")


def _discrete_shell(sd) -> dict:
    """A discrete-model state dict around the shared extractor / interpolation weights: the discrete engine is reused
    for kNN, EdgeConv, merge (-> cs) and interpolation; its flow blocks get neutral parameters and are never run."""
    out = {}
    for key, shape, kind in state_dict_spec():
        if key in sd:
            out[key] = sd[key]
        elif kind == "inv1x1":
            out[key] = torch.eye(3)
        elif kind == "rev":
            out[key] = torch.tensor([2, 1, 0], dtype=torch.int64)
        elif kind == "nbt":
            out[key] = torch.tensor(0, dtype=torch.int64)
        else:
            out[key] = torch.zeros(shape)
    return out


_PACK_NAMES = ("_layer.weight", "_layer.bias", "_hyper_gate.weight", "_hyper_gate.bias", "_hyper_bias.weight")


def _pack_params(block: "_CNFBlockParams") -> List[Tensor]:
    """The sixteen tensors of a block in the order pf_cnf_pack_blocks (and `_CnfPackFn`) takes them: per layer the five of
    `_PACK_NAMES`, then sqrt_end_time."""
    out = []
    for layer in block.cnf.odefunc.diffeq.layers:
        out += [layer._layer.weight, layer._layer.bias, layer._hyper_gate.weight, layer._hyper_gate.bias, layer._hyper_bias.weight]
    return out + [block.cnf.sqrt_end_time]


def _pack_keys(i: int) -> List[str]:
    p = f"flow_blocks.{i}.cnf.odefunc.diffeq.layers"
    return [f"{p}.{l}.{n}" for l in range(3) for n in _PACK_NAMES] + [f"flow_blocks.{i}.cnf.sqrt_end_time"]


class _DevicePack:
    """pf_cnf_pack_blocks (csrc/cnf_pack.hip): the weight records, context matrices and fragment images of up to six blocks from
    their live parameter tensors in ONE launch, bit for bit what packing.pack_cnf_block / pack_cnf_context / cnf_hyper_matrix make
    on the host.  `blocks`: per block the sixteen tensors of `_pack_params`.  The meta rows (end time, image scale, status) are the
    one device -> host read; a status word raises the host packers' ValueError.
    sticky (the deferred training forward): an int32 [4] device row.  pf_cnf_pack_status then leaves the image scales
    as device floats (`scales` [nb, 8], word 6), turns a block with a status into NaN and latches the status in that row;
    read_meta=False skips the host read altogether - `T_end` / `inv_scale` are None and the kernels take both from the device."""

    def __init__(self, blocks: List[List[Tensor]], device: torch.device, sticky: Optional[Tensor] = None, read_meta: bool = True):
        nb = len(blocks)
        f32 = dict(dtype=torch.float32, device=device)
        keep = [[t.detach().to(**f32).contiguous() for t in blk] for blk in blocks]      # parameters as they are: no copy
        for blk in keep:
            if len(blk) != 16 or blk[2].dim() != 2 or blk[2].shape[1] - 1 not in (32, 64, 128):
                raise ValueError("pf_cnf_pack_blocks: sixteen tensors per block, context width 32, 64 or 128")
        cds = [int(blk[2].shape[1]) - 1 for blk in keep]
        self.rec = torch.empty((nb, CNF_REC), **f32)
        self.hb = torch.empty((nb, CNF_CTX), **f32)
        self.Hc = [torch.empty((CNF_CTX, cd), **f32) for cd in cds]
        self.Hplain = [torch.empty((CNF_CTX, cd), **f32) for cd in cds]
        self.image = [torch.empty(CNF_CTX * cd, **f32) for cd in cds]
        self.meta = torch.empty((nb, 4), dtype=torch.float64, device=device)
        ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        _lib.check(_lib.load().pf_cnf_pack_blocks(ptrs([t for blk in keep for t in blk]), _lib.counts(cds), nb, self.rec.data_ptr(),
                                                  self.hb.data_ptr(), ptrs(self.Hc), ptrs(self.Hplain), ptrs(self.image),
                                                  self.meta.data_ptr(), torch.cuda.current_stream().cuda_stream), "pf_cnf_pack_blocks")
        self.scales: Optional[Tensor] = None
        if sticky is not None:
            self.scales = torch.empty((nb, 8), **f32)
            _lib.check(_lib.load().pf_cnf_pack_status(self.meta.data_ptr(), nb, self.rec.data_ptr(), self.scales.data_ptr(),
                                                      sticky.data_ptr(), torch.cuda.current_stream().cuda_stream), "pf_cnf_pack_status")
        if not read_meta:
            if sticky is None:
                raise ValueError("_DevicePack: read_meta=False needs the sticky row that takes the status")
            self.T_end = self.inv_scale = [None] * nb
            return
        meta = self.meta.cpu()                                  # the one read: all blocks
        self.T_end = [float(v) for v in meta[:, 0]]
        self.inv_scale = [float(v) for v in meta[:, 1]]
        for j, st in enumerate(int(v) for v in meta[:, 2]):
            self.raise_status(j, st)

    @staticmethod
    def raise_status(j: int, st: int) -> None:
        """The messages of packing.frag_pack_f16x2 / frag_pack_f16n for block j's status word."""
        if st & 1:
            raise ValueError(f"block {j}: weight magnitude exceeds the fp16 range of the f16x2 path; use ec_mode='f32'")
        if st & 2:
            raise ValueError(f"block {j}: scaled weight magnitude exceeds the fp16 range of the f16n path; use ec_mode='f32'")


class _CnfKernels:
    """Launch wrappers of csrc/cnf.hip shared by the inference engine and the taped single-block engine.  What they read of
    `self` is set by `_init_kernels` (lib, device, the norm kernels' scratch `ws` / `ws1k` / `red`, the counter `nfe`) and by
    `_add_block`: per block index i the record `rec[i]`, the context GEMM's `Hc[i]`, `Hci[i]`, `hb[i]` and `T_end[i]`.
    `_cnf_init` / `_cnf_steps` also take the inference engine's `ws3k` and `split`."""

    def _init_kernels(self, device: torch.device, first_batch: int = 8, next_batch: int = 4) -> None:
        self.lib = _lib.load()
        self.device = device
        self.first_batch, self.next_batch = first_batch, next_batch   # step attempts enqueued before the first look / per later look
        self.rec, self.Hc, self.Hci, self.hb, self.T_end = {}, {}, {}, {}, {}
        self.T_dev, self.scales_dev = {}, {}                     # a device-side pack's end time / image scale ON the device
        self.ws =torch.empty(256, dtype=torch.float64, device=device)
        self.ws1k = torch.empty(1024, dtype=torch.float64, device=device)
        self.red = torch.empty(1, dtype=torch.float64, device=device)
        self.nfe = 0

    def _add_block(self, sd, i: int):
        """Pack block i of the state dict `sd` onto the device -> the host record (for `cnf_split_ok`)."""
        rec, Hc, hb, T_end = pack_cnf_block(sd, i)
        img, inv = pack_cnf_context(Hc)
        self.rec[i] = torch.from_numpy(rec).to(self.device)
        self.Hc[i] = torch.from_numpy(Hc).to(self.device)
        self.Hci[i] = (torch.from_numpy(img).to(self.device), float(inv))
        self.hb[i] = torch.from_numpy(hb).to(self.device)
        self.T_end[i] = T_end
        return rec

    def _add_packed(self, i: int, pack: "_DevicePack", j: int) -> None:
        """Block i = entry j of a device-side pack (pf_cnf_pack_blocks): views of its outputs, nothing is copied."""
        self.rec[i], self.Hc[i], self.hb[i] = pack.rec[j], pack.Hc[j], pack.hb[j]
        self.Hci[i] = (pack.image[j], pack.inv_scale[j])
        self.T_end[i] = pack.T_end[j]
        if pack.scales is not None:                              # pf_cnf_pack_status ran: the deferred kernels' arguments
            self.T_dev[i], self.scales_dev[i] = pack.meta[j], pack.scales[j]

    @staticmethod
    def _stream() -> int:
        return torch.cuda.current_stream().cuda_stream

    def _interval(self, i: int, reverse: bool):
        """(t0, t1) of block i's integration in solver time: [0, T] forward, [-T, 0] reversed."""
        T = self.T_end[i]
        return (0.0, T) if not reverse else (-T, 0.0)

    def _look_loop(self, i: int, ctl: Tensor, enqueue: Callable[[int], None]) -> Tensor:
        """The look-per-batch loop of block i on the controller row `ctl`: `enqueue(n)` launches n step attempts (those past
        the end are no-ops), the row is read once per batch until the integration is done (word 5).  -> the row's host copy;
        its counters are added to `nfe`, an error state raises."""
        attempts, batch = 0, self.first_batch
        while True:
            enqueue(batch)
            attempts += batch
            st = ctl.cpu()                                      # the one device->host read per batch of attempts
            if st[5] != 0:
                break
            if attempts > MAX_NUM_STEPS:
                raise _lib.PuflowHipError(f"dopri5: more than {MAX_NUM_STEPS} step attempts in block {i}")
            batch = self.next_batch
        self.nfe += int(st[8])
        if st[9] in (1, 2):
            raise _solver_error(i, int(st[9]), float(st[0]), float(st[1]))
        return st

    # ---- kernels ----------------------------------------------------------------------------------
    def context(self, i: int, c: Tensor) -> Tensor:
        """ctx [T,288] = c Hc^T + hb: everything a ConcatSquash layer takes from the context."""
        T, cd = c.shape
        ctx = torch.empty((T, CNF_CTX), dtype=torch.float32, device=c.device)
        if cd in (32, 64, 128) and c.is_contiguous():            # split-fp16 GEMM with register-resident weights (pf_pq_gemm's kernel)
            img, inv = self.Hci[i]
            if inv is None:                                      # packed without a host read: the scale is a device word
                _lib.check(self.lib.pf_cnf_context_dev(c.data_ptr(), cd, img.data_ptr(), self.hb[i].data_ptr(),
                                                       self.scales_dev[i].data_ptr(), ctx.data_ptr(), T, self._stream()),
                           "pf_cnf_context_dev")
                return ctx
            _lib.check(self.lib.pf_cnf_context(c.data_ptr(), cd, img.data_ptr(), self.hb[i].data_ptr(), inv, ctx.data_ptr(), T,
                                               self._stream()), "pf_cnf_context")
        else:
            _gemm(c, cd, 1, self.Hc[i], 1, cd, ctx, CNF_CTX, self.hb[i], T, CNF_CTX, cd)
        return ctx

    def _cnf_init_dev(self, i, ctl, x, y, f0, ctx, e, n_tot, extra_d0, extra_scale, reverse, rows, R) -> None:
        """pf_cnf_init_dev: `_cnf_init` over [0, T] / [-T, 0] with T read on the device (`T_dev[i]`, the pack's meta row)."""
        _lib.check(self.lib.pf_cnf_init_dev(ctl.data_ptr(), x.data_ptr(), int(x.stride(0)), y.data_ptr(), f0.data_ptr(),
                                            ctx.data_ptr(), e.data_ptr(), self.rec[i].data_ptr(), self.T_dev[i].data_ptr(),
                                            float(n_tot), extra_d0.data_ptr() if extra_d0 is not None else None,
                                            float(extra_scale), 1 if reverse else 0, RTOL, ATOL, rows, R, self.ws3k.data_ptr(),
                                            self._stream()), "pf_cnf_init_dev")

    def _rhs(self, i, y0, K, coef, h, t, sgn, ctx, e, kout, yout, rows, R):
        n = len(coef)
        arr = (ctypes.c_float * max(n, 1))(*[float(v) for v in coef])
        _lib.check(self.lib.pf_cnf_rhs(y0.data_ptr(), K.data_ptr() if n else None, arr, n, float(h), float(t), float(sgn),
                                       ctx.data_ptr(), e.data_ptr(), self.rec[i].data_ptr(), kout.data_ptr(),
                                       yout.data_ptr() if yout is not None else None, rows, R, self._stream()), "pf_cnf_rhs")
        self.nfe += 1

    def _lincomb(self, ptrs: List[Tensor], w: List[float], out: Tensor) -> None:
        n = len(ptrs)
        pa = (ctypes.c_void_p * n)(*[p.data_ptr() for p in ptrs])
        wa = (ctypes.c_float * n)(*[float(v) for v in w])
        _lib.check(self.lib.pf_lincomb(pa, wa, n, out.data_ptr(), out.numel(), self._stream()), "pf_lincomb")

    def _sumsq(self, a, b, s0, s1, K=None, w=None, h=0.0) -> float:
        n_terms = len(w) if w is not None else 0
        wa = (ctypes.c_float * max(n_terms, 1))(*([float(v) for v in w] if w is not None else [0.0]))
        _lib.check(self.lib.pf_scaled_sumsq(a.data_ptr() if a is not None else None, b.data_ptr() if b is not None else None,
                                            s0.data_ptr(), s1.data_ptr() if s1 is not None else None,
                                            K.data_ptr() if K is not None else None, wa, n_terms, float(h), RTOL, ATOL,
                                            s0.numel(), self.ws.data_ptr(), self.red.data_ptr(), self._stream()),
                   "pf_scaled_sumsq")
        return float(self.red.item())                       # the one device->host read per norm

    def _cnf_init(self, i, ctl, x, y, f0, ctx, e, t0, t1, n_tot, extra_d0, extra_scale, reverse, rows, R) -> None:
        """pf_cnf_init: the state rows (x, 0), f0 and torchdiffeq's initial step size, two launches; resets the controller `ctl`."""
        _lib.check(self.lib.pf_cnf_init(ctl.data_ptr(), x.data_ptr(), int(x.stride(0)), y.data_ptr(), f0.data_ptr(),
                                        ctx.data_ptr(), e.data_ptr(), self.rec[i].data_ptr(), t0, t1, float(n_tot),
                                        extra_d0.data_ptr() if extra_d0 is not None else None, float(extra_scale),
                                        1 if reverse else 0, RTOL, ATOL, rows, R, self.ws3k.data_ptr(), self._stream()),
                   "pf_cnf_init")

    def _cnf_steps(self, i, ctl, bufs, ctx, e, rows, R, attempts) -> None:
        """pf_cnf_steps: `attempts` step attempts enqueued back to back on bufs = (y, y1, f0, f1, out) [5, rows, 4]."""
        y, y1, f0, f1, out = bufs
        _lib.check(self.lib.pf_cnf_steps(ctl.data_ptr(), y.data_ptr(), y1.data_ptr(), f0.data_ptr(), f1.data_ptr(),
                                         ctx.data_ptr(), e.data_ptr(), self.rec[i].data_ptr(), out.data_ptr(), RTOL, ATOL,
                                         rows, R, int(attempts), self.ws1k.data_ptr(), self.split[i], self._stream()),
                   "pf_cnf_steps")

    def _cnf_steps_taped(self, i, ctl, states, steps, fbuf, ctx, e, rows, R, attempts) -> None:
        """pf_cnf_steps_taped: `attempts` attempts on the tape states [cap + 1, rows, 4] / steps [cap, 2], fbuf = (f0, f1) [2, rows, 4]."""
        _lib.check(self.lib.pf_cnf_steps_taped(ctl.data_ptr(), states.data_ptr(), steps.data_ptr(), int(steps.shape[0]),
                                               fbuf[0].data_ptr(), fbuf[1].data_ptr(), ctx.data_ptr(), e.data_ptr(),
                                               self.rec[i].data_ptr(), RTOL, ATOL, rows, R, int(attempts), self.ws1k.data_ptr(),
                                               self._stream()), "pf_cnf_steps_taped")

    def tape_forward(self, i: int, x: Tensor, c: Tensor, e: Tensor, R: int, reverse: bool, cap: int = 32, ctx: Optional[Tensor] = None,
                     d0c: Optional[Tensor] = None):
        """dopri5 on block i with the control on the DEVICE (pf_cnf_init, then batches of pf_cnf_steps_taped attempts with one read
        of the controller per batch, as `_CnfEngine.integrate`), the step that would cover the end time cut to END there: the
        result is the last accepted step's solution, so the forward is exactly the recorded steps.  cap: steps the tape is
        allocated for; a tape that fills up (status 3) is allocated anew at twice the size and the integration starts again.
        -> (state [rows,4], tape): (s, h) per accepted step on the device (`steps_dev` [n,2], the fp32 values the kernels
        computed with) and as host floats (`steps`, one read when done), the state at the start of each step (`states` [n,rows,4]),
        the context rows and the derivatives at both ends.
        ctx, d0c: block i's context rows and the context's norm word where the caller has them already (the train-mode forward
        computes both once per block for f and g)."""
        rows = x.shape[0]
        dev = x.device
        ctx, n_tot, d0c = self._tape_inputs(i, c, R, rows, ctx, d0c)
        fbuf =torch.empty((2, rows, 4), dtype=torch.float32, device=dev)
        cap = max(1, int(cap))
        while True:
            states = torch.empty((cap + 1, rows, 4), dtype=torch.float32, device=dev)
            steps = torch.empty((cap, 2), dtype=torch.float32, device=dev)
            self._cnf_init(i, self.ctl, x, states[0], fbuf[0], ctx, e, *self._interval(i, reverse), n_tot, d0c, float(R), reverse,
                           rows, R)
            f_start = fbuf[0].clone()                           # needed for dT when reversed; fbuf ping-pongs from here on
            st = self._look_loop(i, self.ctl, lambda n: self._cnf_steps_taped(i, self.ctl, states, steps, fbuf, ctx, e, rows, R, n))
            if st[9] != 3:
                break
            if cap > MAX_NUM_STEPS:
                raise _lib.PuflowHipError(f"dopri5: more than {MAX_NUM_STEPS} accepted steps in block {i}")
            cap *= 2
        n = int(st[6])
        return states[n], dict(steps=_steps_host(steps[:n]), steps_dev=steps[:n], states=states[:n], ctx=ctx, f_start=f_start,
                               f_end=fbuf[int(st[4])], took=int(st[6]) + int(st[7]))

    def _tape_inputs(self, i: int, c: Tensor, R: int, rows: int, ctx: Optional[Tensor], d0c: Optional[Tensor]):
        """What a taped integration takes from the context, computed here where the caller has not: -> (ctx [T,288], n_tot,
        d0c).  The context is a state of the reference's ODE: its elements count in the norms (n_tot) and d0c is its norm word."""
        if ctx is None:
            ctx = self.context(i, c)
        if d0c is None:
            d0c = torch.empty(1, dtype=torch.float64, device=c.device)
            self.context_norm(c, d0c)
        return ctx, float(rows * 4 + c.numel() * R), d0c

    def replay(self, i: int, x: Tensor, steps_dev: Tensor, reverse: bool, ctx: Tensor, e: Tensor, R: int, tape: bool = False,
               errsq: Optional[Tensor] = None):
        """pf_cnf_replay (csrc/cnf_replay.hip): block i integrated on the step list steps_dev [n, 2] (device floats (s, h)) in ONE
        launch, no controller.  x [rows, >= 3], row stride 3 or 4 floats.  tape: also write the states [n + 1, rows, 4] and the
        derivatives at both ends - the tape `tape_vjp` sweeps.  errsq [n] (device doubles): the per-step error sums.
        -> (state [rows,4], tape dict | None)"""
        rows, n = x.shape[0], int(steps_dev.shape[0])
        dev = x.device
        x = _rows3(x)
        if steps_dev.dtype != torch.float32 or not steps_dev.is_contiguous():
            steps_dev = steps_dev.float().contiguous()
        y = torch.empty((rows, 4), dtype=torch.float32, device=dev)
        states = torch.empty((n + 1, rows, 4), dtype=torch.float32, device=dev) if tape else None
        ends = torch.empty((2, rows, 4), dtype=torch.float32, device=dev) if tape else None
        ws = None
        if errsq is not None:
            need = self.lib.pf_cnf_replay_workspace_bytes(rows, n)
            if need < 0:
                raise _lib.PuflowHipError(f"pf_cnf_replay: rows = {rows}, n_steps = {n}")
            ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
        ptr = lambda t_: t_.data_ptr() if t_ is not None else None
        _lib.check(self.lib.pf_cnf_replay(x.data_ptr(), int(x.stride(0)), steps_dev.data_ptr(), n, 1 if reverse else 0,
                                          ctx.data_ptr(), e.data_ptr(), self.rec[i].data_ptr(), ptr(states), y.data_ptr(),
                                          ptr(ends[0]) if tape else None, ptr(ends[1]) if tape else None, ptr(errsq), RTOL, ATOL,
                                          rows, R, ptr(ws), self._stream()), "pf_cnf_replay")
        self.nfe += 1 + 6 * n
        if not tape:
            return y, None
        return y, dict(schedule=True, states=states, steps_dev=steps_dev, ctx=ctx, f_start=ends[0], f_end=ends[1])

    def context_norm(self, c: Tensor, out: Tensor) -> None:
        """out[0] (device double) = sum (c / (atol + rtol |c|))^2: the context's share of the solver's initial-step norm."""
        _lib.check(self.lib.pf_scaled_sumsq(c.data_ptr(), None, c.data_ptr(), None, None, (ctypes.c_float * 1)(0.0), 0, 0.0,
                                            RTOL, ATOL, c.numel(), self.ws.data_ptr(), out.data_ptr(), self._stream()),
                   "pf_scaled_sumsq")


class _CnfEngine(_CnfKernels):
    """Device-side plan of the continuous model + the dopri5 driver."""

    def __init__(self, sd, device: torch.device, upratio: int):
        self._init_kernels(device, int(os.environ.get("PF_CNF_FIRST_BATCH", "8")), int(os.environ.get("PF_CNF_NEXT_BATCH", "4")))
        self.R = upratio
        self.base = _Engine(_discrete_shell(sd), device)
        self.split = []
        for i in range(NUM_BLOCKS):
            rec = self._add_block(sd, i)
            # PF_CNF_SPLIT_GATES (include/puflow_hip.h): only where the factored 2^x cannot overflow; PF_CNF_SPLIT=0 keeps the plain kernel
            self.split.append(int(cnf_split_ok(rec, self.T_end[i]) and os.environ.get("PF_CNF_SPLIT", "1") != "0"))
        self.ws3k = torch.empty(3072, dtype=torch.float64, device=device)
        self.ctl = torch.zeros(16, dtype=torch.float64, device=device)       # dopri5 controller state (csrc/cnf.hip; zero before its first use)
        # attempts enqueued per integration when the whole forward runs WITHOUT reading the controller in between (attempts past
        # the end are ~4 us no-ops; an integration that needs more makes the forward fall back to the look-per-batch loop); 0 = off
        self.async_attempts = int(os.environ.get("PF_CNF_ASYNC_ATTEMPTS", "1"))             # 0 = never run blind
        self.logs = torch.zeros((2 * NUM_BLOCKS, 16), dtype=torch.float64, device=device)   # controller state after each integration
        # step attempts each of the twelve integrations took the last time (accepted + rejected): the blind run enqueues that
        # many + a margin (the trained model's blocks differ by 10x: 3 attempts for the short ones, 25 for the T = 36 block)
        self.hint: Optional[List[int]] = None
        self.accepted = 0
        self.rejected = 0
        self.last_attempts = 0                                   # attempts the last look-per-batch integration took
        self.sched_lists: Optional[tuple] = None                 # (a `_ScheduleDev`, its step lists at this plan's end times)

    def schedule_lists(self, sdev) -> Tensor:
        """The step lists [12, m, 2] of the schedule constants `sdev` at this plan's end times, which are fixed in eval mode:
        made once per plan and schedule."""
        if self.sched_lists is None or self.sched_lists[0] is not sdev:
            T_blocks = torch.tensor([self.T_end[i] for i in range(NUM_BLOCKS)], dtype=torch.float64).to(self.device)
            self.sched_lists = (sdev, sdev.lists(T_blocks))
        return self.sched_lists[1]

    def drop_schedule(self) -> None:
        self.sched_lists = None

    def integrate(self, i: int, x: Tensor, ctx: Tensor, e: Tensor, R: int, reverse: bool, extra_n: int,
                  extra_d0, log: Optional[Tensor] = None, blind: int = 0, extra_scale: float = 1.0) -> Tensor:
        """x [rows, >= 3] (row stride 3 or 4 floats: a previous block's state is taken as it lies) -> state [rows,4] =
        (x', delta logp) at the end time of block i.
        log (a [16] double device row, zero before its first use): do not look at the controller - `log` IS the controller
        state of this integration; enqueue `blind` attempts and return; the caller checks all rows once (`check_logs`).
        Otherwise the look-per-batch loop, which also leaves the number of attempts it took in `self.last_attempts`.
        extra_d0: a device double (or a python float / 0) x extra_scale - the context rows' share of |y0 / scale|^2."""
        rows = x.shape[0]
        dev = x.device
        n_tot = float(rows * 4 + extra_n)
        x = _rows3(x)
        bufs = torch.empty((5, rows, 4), dtype=torch.float32, device=dev)
        y, f0, out = bufs[0], bufs[2], bufs[4]
        # the state rows (x, 0), f0 and torchdiffeq's initial step size, on the device in two launches (csrc/cnf.hip:
        # pf_cnf_init); the controller state follows
        ctl = self.ctl if log is None else log
        if not isinstance(extra_d0, torch.Tensor):
            extra_d0 = torch.tensor([float(extra_d0)], dtype=torch.float64, device=dev) if extra_d0 else None
        self._cnf_init(i, ctl, x, y, f0, ctx, e, *self._interval(i, reverse), n_tot, extra_d0, extra_scale, reverse, rows, R)

        # ---- adaptive steps: ONE launch per attempt (six fused stage evaluations); the accept / reject / next-dt decisions are
        # taken on the device (csrc/cnf.hip: cnf_ctl_update, run by the workgroup of a step attempt that finishes last), the host
        # enqueues a batch of attempts and reads the controller state once per batch (attempts past the end are no-ops)
        if log is not None:
            self._cnf_steps(i, ctl, bufs, ctx, e, rows, R, blind)
            return out
        st = self._look_loop(i, ctl, lambda n: self._cnf_steps(i, ctl, bufs, ctx, e, rows, R, n))
        self.last_attempts = int(st[6]) + int(st[7])
        self.accepted += int(st[6])
        self.rejected += int(st[7])
        return out

    def time_step_attempts(self, i: int, x: Tensor, ctx: Tensor, e: Tensor, R: int, reverse: bool, extra_n: int, extra_d0,
                           attempts: int, extra_scale: float = 1.0):
        """bench.py's roofline leg: ONE integration of block i enqueued without a look at the controller, HIP events on the launch
        stream around the `attempts` step attempts alone (pf_cnf_steps: the kernel of the timed forward, cnf_step_dev_kernel) ->
        (milliseconds for all attempts, attempts the integration really took = accepted + rejected; the rest were no-ops)."""
        rows = x.shape[0]
        x = _rows3(x)
        bufs = torch.empty((5, rows, 4), dtype=torch.float32, device=x.device)
        ctl = torch.zeros(16, dtype=torch.float64, device=x.device)
        self._cnf_init(i, ctl, x, bufs[0], bufs[2], ctx, e, *self._interval(i, reverse), rows * 4 + extra_n, extra_d0, extra_scale,
                       reverse, rows, R)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self._cnf_steps(i, ctl, bufs, ctx, e, rows, R, attempts)
        b.record()
        torch.cuda.synchronize()
        st = ctl.cpu()
        return a.elapsed_time(b), int(st[6]) + int(st[7]), bool(st[5] != 0)

    def check_logs(self, n: int, took: List[int]) -> int:
        """The controller states of the first n deferred integrations, ONE device -> host read: how many of them, from the
        first on, finished cleanly inside their attempts.  Their counters are added to the statistics and their attempt counts
        written into `took`."""
        L = self.logs[:n].cpu()
        ok = ((L[:, 5] != 0) & (L[:, 9] == 0)).tolist()
        k = 0
        while k < n and ok[k]:
            k += 1
        for j in range(k):
            took[j] = int(L[j, 6] + L[j, 7])
        self.accepted += int(L[:k, 6].sum())
        self.rejected += int(L[:k, 7].sum())
        self.nfe += int(L[:k, 8].sum())
        return k


class _BlockTapeEngine(_CnfKernels):
    """The kernels of ONE block around weights packed from the live parameters: the taped integration of
    `PointInterpFlow.flow_block` and of the train-mode forward, and their backward.  sd_block: a host copy of the block's
    parameters for the numpy packers (the A/B reference), or None with pack = (a `_DevicePack`, the block's entry in it).
    scratch: another engine of the same device and stream whose controller, norm and slab workspaces this one shares (the six
    engines of a train-mode forward run one after the other)."""

    def __init__(self, sd_block, i: int, device: torch.device, pack=None, scratch: Optional["_BlockTapeEngine"] = None):
        self._init_kernels(device)
        if pack is None:
            self._add_block(sd_block, i)
            self.Hplain = torch.from_numpy(cnf_hyper_matrix(sd_block, i)[:, 1:].copy()).to(device)      # [288, cd], no folded constants
        else:
            self._add_packed(i, *pack)
            self.Hplain = pack[0].Hplain[pack[1]]
        self._vjp_wss: dict = {}
        if scratch is not None:
            self.ws, self.ws1k, self.red, self.ws3k, self.ctl, self._vjp_wss = (scratch.ws, scratch.ws1k, scratch.red, scratch.ws3k,
                                                                                 scratch.ctl, scratch._vjp_wss)
            return
        self.ws3k = torch.empty(3072, dtype=torch.float64, device=device)
        self.ctl = torch.zeros(16, dtype=torch.float64, device=device)       # dopri5 controller state of the device-side tape

    def step(self, i, y, f0, t, h, reverse, ctx, e, y1, f1, rows, R) -> float:
        """One Dormand-Prince attempt (pf_cnf_step) -> the scaled error sum, read back (one host read per attempt)."""
        _lib.check(self.lib.pf_cnf_step(y.data_ptr(), f0.data_ptr(), float(t), float(h), 1 if reverse else 0, ctx.data_ptr(),
                                        e.data_ptr(), self.rec[i].data_ptr(), y1.data_ptr(), f1.data_ptr(), None, RTOL, ATOL,
                                        rows, R, self.ws1k.data_ptr(), self.red.data_ptr(), self._stream()), "pf_cnf_step")
        self.nfe += 6
        return float(self.red.item())

    def tape_forward_deferred(self, i: int, x: Tensor, c: Tensor, e: Tensor, R: int, reverse: bool, attempts: int, cap: int,
                              log: Tensor, sticky: Tensor, ctx: Optional[Tensor] = None, d0c: Optional[Tensor] = None):
        """`tape_forward` WITHOUT a host read: pf_cnf_init(_dev) into `log` - a [16] double device row, zero before its first
        use, which IS this integration's controller, as in `_CnfEngine.integrate(log=...)` - then ONE pf_cnf_steps_taped call of
        `attempts` attempts (those past the end return at once) on a tape of `cap` steps, then pf_cnf_tape_close: the result and
        the derivative at the end at fixed addresses, NaN when the integration did not end cleanly inside (attempts, cap), and
        the run entered in `sticky` (int32 [4]).  -> (state [rows,4], tape): the WHOLE tape (`states` [cap + 1, rows, 4],
        `steps_dev` [cap, 2]; the valid prefix is log[6], known to the device alone), `log`, `cap`, `ctx`, `f_start`, `f_end`.
        The caller reads log rows and sticky table when it likes (`PointInterpFlow.check_train_logs`)."""
        rows = x.shape[0]
        dev = x.device
        attempts, cap = int(attempts), int(cap)
        if attempts < 1 or cap < 1:
            raise ValueError("tape_forward_deferred: attempts >= 1 and cap >= 1")
        ctx, n_tot, d0c = self._tape_inputs(i, c, R, rows, ctx, d0c)
        fbuf = torch.empty((2, rows, 4), dtype=torch.float32, device=dev)
        states = torch.empty((cap + 1, rows, 4), dtype=torch.float32, device=dev)
        steps = torch.empty((cap, 2), dtype=torch.float32, device=dev)
        if self.T_end[i] is None:
            self._cnf_init_dev(i, log, x, states[0], fbuf[0], ctx, e, n_tot, d0c, float(R), reverse, rows, R)
        else:
            self._cnf_init(i, log, x, states[0], fbuf[0], ctx, e, *self._interval(i, reverse), n_tot, d0c, float(R), reverse, rows, R)
        f_start = fbuf[0].clone()
        self._cnf_steps_taped(i, log, states, steps, fbuf, ctx, e, rows, R, attempts)
        end = torch.empty((2, rows, 4), dtype=torch.float32, device=dev)
        _lib.check(self.lib.pf_cnf_tape_close(log.data_ptr(), states.data_ptr(), cap, fbuf[0].data_ptr(), fbuf[1].data_ptr(), rows,
                                              end[0].data_ptr(), end[1].data_ptr(), sticky.data_ptr(), self._stream()),
                   "pf_cnf_tape_close")
        return end[0], dict(deferred=True, states=states, steps_dev=steps, log=log, cap=cap, ctx=ctx, f_start=f_start, f_end=end[1])

    def tape_forward_host(self, i: int, x: Tensor, c: Tensor, e: Tensor, R: int, reverse: bool):
        """The A/B reference of `tape_forward` (flow_block's controller="host"): ONE attempt per launch and the control on the host (oracle/cnf_ref.py::dopri5 restated), except
        that the step which would cover the end time is cut to END there: the result is the last accepted step's solution, not
        a dense-output value inside it, so the forward is exactly the recorded steps.
        -> (state [rows,4], tape): tape holds (s, h) per accepted step as host floats (the fp32 values the kernels were given),
        the state at the start of each step on the device, the context rows and the derivatives at both ends."""
        rows = x.shape[0]
        dev = x.device
        t0, t1 = self._interval(i, reverse)
        sgn = 1.0 if not reverse else -1.0
        f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
        ctx = self.context(i, c)
        n_tot = float(rows * 4 + c.numel() * R)                 # the context is a state of the reference's ODE: it enters the norms
        self.context_norm(c, self.red)
        d0c = float(self.red.item()) * R
        y = torch.zeros((rows, 4), dtype=torch.float32, device=dev)
        y[:, :3] = x
        f0, f1 = torch.empty_like(y), torch.empty_like(y)
        self._rhs(i, y, y, [], 0.0, sgn * t0, sgn, ctx, e, f0, None, rows, R)
        f_start = f0
        d0 = math.sqrt((self._sumsq(y, None, y, None) + d0c) / n_tot)
        d1 = math.sqrt(self._sumsq(f0, None, y, None) / n_tot)
        h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
        self._rhs(i, y, f0, [1.0], h0, sgn * (t0 + h0), sgn, ctx, e, f1, None, rows, R)
        d2 = math.sqrt(self._sumsq(f1, f0, y, None) / n_tot) / h0
        h1 = max(1e-6, h0 * 1e-3) if (d1 <= 1e-15 and d2 <= 1e-15) else (0.01 / max(d1, d2)) ** (1.0 / ORDER)
        dt = min(100 * h0, h1)
        t = t0
        steps, states = [], []
        for _ in range(MAX_NUM_STEPS):
            cover = t + dt >= t1
            ts, h = f32(t), f32(t1 - t if cover else dt)
            y1 = torch.empty_like(y)
            ratio = math.sqrt(self.step(i, y, f0, ts, h, reverse, ctx, e, y1, f1, rows, R) / n_tot)
            if not math.isfinite(ratio) or not (t + h > t):
                raise _solver_error(i, 2 if math.isfinite(ratio) else 1, t, h)
            if ratio <= 1.0:
                steps.append((ts, h)); states.append(y)
                y, f0, f1 = y1, f1, torch.empty_like(y)
                t = t + h
                if cover:
                    break
            dt = h * IFACTOR if ratio == 0 else h * min(IFACTOR, max(SAFETY / ratio ** (1.0 / ORDER), 1.0 if ratio < 1 else DFACTOR))
        else:
            raise _lib.PuflowHipError(f"dopri5: more than {MAX_NUM_STEPS} step attempts in block {i}")
        return y, dict(steps=steps, states=states, ctx=ctx, f_start=f_start, f_end=f0)

    def _vjp_workspace(self, rows, R, dev) -> Tensor:
        """The slab workspace of pf_cnf_rhs_vjp and pf_cnf_tape_vjp (the same size), kept per shape."""
        if (rows, R) not in self._vjp_wss:
            need = self.lib.pf_cnf_rhs_vjp_workspace_bytes(rows, R)
            if need < 0:
                raise _lib.PuflowHipError(f"pf_cnf_rhs_vjp: rows = {rows} must be a multiple of R = {R} <= 16")
            self._vjp_wss[(rows, R)] = torch.empty(need // 4, dtype=torch.float32, device=dev)
        return self._vjp_wss[(rows, R)]

    def tape_vjp(self, i, states, steps_dev, sgn, ctx, e, ybar, ctxbar, grad, rows, R) -> None:
        """pf_cnf_tape_vjp: the reverse sweep of the recorded steps in one launch; ybar [rows,4] in / out."""
        ws = self._vjp_workspace(rows, R, ybar.device)
        _lib.check(self.lib.pf_cnf_tape_vjp(states.data_ptr(), steps_dev.data_ptr(), int(steps_dev.shape[0]), float(sgn),
                                            ctx.data_ptr(), e.data_ptr(), self.rec[i].data_ptr(), ybar.data_ptr(),
                                            ctxbar.data_ptr(), grad.data_ptr(), rows, R, ws.data_ptr(), self._stream()),
                   "pf_cnf_tape_vjp")

    def tape_vjp_dev(self, i, tape, sgn, e, ybar, ctxbar, grad, rows, R) -> None:
        """pf_cnf_tape_vjp_dev on a tape of `tape_forward_deferred`: the step count is the controller row's, read on the device."""
        ws = self._vjp_workspace(rows, R, ybar.device)
        _lib.check(self.lib.pf_cnf_tape_vjp_dev(tape["states"].data_ptr(), tape["steps_dev"].data_ptr(), tape["log"].data_ptr(),
                                                int(tape["cap"]), float(sgn), tape["ctx"].data_ptr(), e.data_ptr(),
                                                self.rec[i].data_ptr(), ybar.data_ptr(), ctxbar.data_ptr(), grad.data_ptr(), rows, R,
                                                ws.data_ptr(), self._stream()), "pf_cnf_tape_vjp_dev")

    def vjp(self, i, y, kbar, t, sgn, ctx, e, ybar, ctxbar, grad, rows, R) -> None:
        ws = self._vjp_workspace(rows, R, y.device)
        _lib.check(self.lib.pf_cnf_rhs_vjp(y.data_ptr(), kbar.data_ptr(), float(t), float(sgn), ctx.data_ptr(), e.data_ptr(),
                                           self.rec[i].data_ptr(), ybar.data_ptr(), ctxbar.data_ptr(), grad.data_ptr(), rows, R,
                                           ws.data_ptr(), self._stream()), "pf_cnf_rhs_vjp")

    def tape_backward(self, i: int, tape: dict, ybar: Tensor, c: Tensor, e: Tensor, R: int, reverse: bool, sweep: str = "fused"):
        """The recorded steps in reverse, step sizes as constants.  sweep = "fused": one pf_cnf_tape_vjp launch for
        the whole tape.  sweep = "per_eval", its A/B reference, launch by launch: per step the stage states are recomputed
        (pf_cnf_rhs), then for j = 6 .. 1:  kbar_j = h b_j y1bar + h sum_{m > j} a_mj Ybar_m  (pf_lincomb),
        Ybar_j = VJP_F(Y_j, t_j; kbar_j)  (pf_cnf_rhs_vjp, which also adds the evaluation's weight / context gradients), and
        y0bar = y1bar + sum_j Ybar_j.  -> (y0bar [rows,4], grad record [4900], ctxbar [T,288])."""
        rows = ybar.shape[0]
        dev = ybar.device
        sgn = 1.0 if not reverse else -1.0
        ctx = tape["ctx"]
        grad = torch.zeros(CNF_GRAD, dtype=torch.float32, device=dev)
        ctxbar = torch.zeros((c.shape[0], CNF_CTX), dtype=torch.float32, device=dev)
        if tape.get("deferred"):
            if sweep != "fused":
                raise ValueError('a deferred tape is swept by pf_cnf_tape_vjp_dev: sweep="fused"')
            y0bar = ybar.clone()
            self.tape_vjp_dev(i, tape, sgn, e, y0bar, ctxbar, grad, rows, R)
            return y0bar, grad, ctxbar
        if sweep == "fused":
            states, steps_dev = tape["states"], tape.get("steps_dev")
            if not isinstance(states, Tensor):                                     # the host controller's tape: a list of states
                states = torch.stack(states)
            if steps_dev is None:
                steps_dev = torch.tensor(tape["steps"], dtype=torch.float32, device=dev).reshape(-1, 2)
            y0bar = ybar.clone()
            self.tape_vjp(i, states.contiguous(), steps_dev.contiguous(), sgn, ctx, e, y0bar, ctxbar, grad, rows, R)
            return y0bar, grad, ctxbar
        K = torch.empty((5, rows, 4), dtype=torch.float32, device=dev)             # k_1 .. k_5 of the step being swept
        Y = torch.empty((6, rows, 4), dtype=torch.float32, device=dev)
        Yb = torch.empty((6, rows, 4), dtype=torch.float32, device=dev)
        kb = torch.empty((rows, 4), dtype=torch.float32, device=dev)
        b = DP_BETA[5]
        alpha = [0.0] + DP_ALPHA[:5]
        for n in reversed(range(len(tape["steps"]))):
            (s, h), y0 = tape["steps"][n], tape["states"][n]
            self._rhs(i, y0, y0, [], 0.0, sgn * s, sgn, ctx, e, K[0], None, rows, R)
            for j in range(1, 5):
                self._rhs(i, y0, K, DP_BETA[j - 1], h, sgn * (s + alpha[j] * h), sgn, ctx, e, K[j], Y[j], rows, R)
            # the last stage's STATE only (its derivative k_6 is not needed: the sweep differentiates it, it does not use it)
            self._lincomb([y0] + [K[m] for m in range(5)], [1.0] + [h * a for a in DP_BETA[4]], Y[5])
            for j in reversed(range(6)):
                terms, w = [ybar], [h * b[j]]
                for m in range(j + 1, 6):
                    if DP_BETA[m - 1][j] != 0:
                        terms.append(Yb[m]); w.append(h * DP_BETA[m - 1][j])
                self._lincomb(terms, w, kb)
                self.vjp(i, y0 if j == 0 else Y[j], kb, sgn * (s + alpha[j] * h), sgn, ctx, e, Yb[j], ctxbar, grad, rows, R)
            nxt = torch.empty_like(ybar)
            self._lincomb([ybar] + [Yb[j] for j in range(6)], [1.0] * 7, nxt)
            ybar = nxt
        return ybar, grad, ctxbar
