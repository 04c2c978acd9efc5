"""Continuous (CNF) PU-Flow: `modules/continuous/interpflow.py` on the HIP library.

Same constructor, methods and the 390 state-dict keys of the reference's continuous `PointInterpFlow`
(`pretrain/puflow-x4-cnf-pu1k.pt` loads with `load_state_dict`).  eval(): the inference plan below.  train(): the forward with
gradients (`forward_train`: the discrete training step's extractor and interpolation branch, then `flow_train` - twelve taped
integrations, backward by `pf_cnf_tape_vjp`, csrc/cnf_bwd.hip, weights packed from the live parameters on the device by
`pf_cnf_pack_blocks`, csrc/cnf_pack.hip); `PointInterpFlow.flow_block` is ONE such block as an autograd function.  With
`net.train_deferred` (off by default) the taped integrations run against learnt budgets without a host read -
`pf_cnf_tape_close`, `pf_cnf_tape_vjp_dev`, `check_train_logs` - which is what a captured training step needs.  With
`net.step_schedule` (None by default) eval and train mode integrate on a FROZEN step schedule instead - per integration
a grid of step boundaries chosen in advance, e.g. the adaptive solver's own accepted steps on a calibration input
(`record_schedule`) - one `pf_cnf_replay` launch each (csrc/cnf_replay.hip), no controller at all.

What runs where:
  * kNN, the six EdgeConv units, the merge units and the interpolation module are the discrete model's kernels
    (the reference imports those modules from the discrete file too, continuous/interpflow.py:14);
  * the per-point context terms of every ConcatSquash layer: one split-fp16 GEMM per block (`pf_cnf_context`);
  * an integration of the forward: `pf_cnf_init`, then `pf_cnf_steps` - one fused launch per step attempt (six stage
    evaluations incl. the Hutchinson term, error norm) with dopri5's step-size CONTROL on the device (torchdiffeq semantics
    restated from its published algorithm, see oracle/cnf_ref.py header).  The controller states of the twelve integrations
    are read ONCE per forward; one that did not finish inside its attempts falls back to a read per batch of attempts;
  * `flow_block`: the same controller recording a tape (`pf_cnf_steps_taped`) and ONE launch that sweeps the tape in reverse
    (`pf_cnf_tape_vjp`, csrc/cnf_bwd.hip).  Its A/B references step from the host: one `pf_cnf_step` per attempt with the error
    norm read back, `pf_cnf_rhs`, `pf_lincomb`, `pf_scaled_sumsq` around it, and `pf_cnf_rhs_vjp` per evaluation in the backward.

Parity: the right-hand side is pinned to the reference's own ODEfunc (tests/golden/cnf_rhs.npz); the solver is UNPINNED
(torchdiffeq is not installed and not vendored) - the integrated path is tested against oracle/cnf_ref.py, a from-text
restatement of dopri5.  Tolerance of the integrated path is the solver's own (atol = rtol = 1e-5).
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import List, Optional

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib
from .interpflow import (COND_CHANNELS, FEAT_CHANNELS, GROWTH, NUM_BLOCKS, _EdgeConvParams, _Engine, _InterpParams,
                         _MergeParams)
from .packing import (CNF_CTX, CNF_GRAD, CNF_REC, cnf_hyper_matrix, cnf_split_ok, pack_cnf_block, pack_cnf_context,
                      unpack_cnf_grads)
from .train_perop import _gemm
from .weights import state_dict_spec

ATOL = RTOL = 1e-5                       # continuous/interpflow.py:28
SAFETY, IFACTOR, DFACTOR, ORDER = 0.9, 10.0, 0.2, 5
MAX_NUM_STEPS = 100000                   # step attempts per integration; a bound, never reached by a sane model
DP_ALPHA = [1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0]
DP_BETA = [
    [1 / 5],
    [3 / 40, 9 / 40],
    [44 / 45, -56 / 15, 32 / 9],
    [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
    [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
    [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84],
]
DP_C_ERR = [35 / 384 - 1951 / 21600, 0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720,
            -2187 / 6784 - -12231 / 42400, 11 / 84 - 649 / 6300, -1. / 60.]
DP_C_MID = [6025192743 / 30085553152 / 2, 0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
            187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2]


# ---- frozen step schedules: pure Python, no GPU ---------------------------------------------------------------
# A schedule is a dict: for each of the twelve integrations (block, reverse) a strictly increasing float64 grid of FRACTIONS of the
# integration's interval, from 0.0 to 1.0.  Step k of integration (i, r) spans [t0 + T g_k, t0 + T g_{k+1}] in solver time
# (T = the block's end time, t0 = 0 going forward and -T reversed).  A uniform grid is one special case; the usual source is the
# adaptive solver's own accepted steps on a calibration input (`PointInterpFlow.record_schedule`).
SCHEDULE_FORMAT = "puflow-cnf-step-schedule"


def schedule_keys(num_blocks: int = NUM_BLOCKS):
    """The integrations in the order they run: f's blocks 0 .. n - 1, then g's n - 1 .. 0."""
    return [(i, False) for i in range(num_blocks)] + [(i, True) for i in reversed(range(num_blocks))]


def validate_schedule(schedule, num_blocks: int = NUM_BLOCKS) -> dict:
    """-> the schedule as {(block, reverse): tuple of floats}; ValueError says what is wrong with it."""
    if not isinstance(schedule, dict):
        raise ValueError("a step schedule is a dict {(block, reverse): grid of fractions from 0.0 to 1.0}")
    keys = schedule_keys(num_blocks)
    extra = [k for k in schedule if k not in keys]
    if extra:
        raise ValueError(f"step schedule: unknown integration {extra[0]!r} (keys are (block 0..{num_blocks - 1}, reverse False/True))")
    out = {}
    for key in keys:
        if key not in schedule:
            raise ValueError(f"step schedule: no grid for integration (block {key[0]}, reverse {key[1]})")
        try:
            grid = tuple(float(v) for v in schedule[key])
        except (TypeError, ValueError):
            raise ValueError(f"step schedule {key}: the grid is a sequence of numbers") from None
        if len(grid) < 2:
            raise ValueError(f"step schedule {key}: a grid has at least the two ends 0.0 and 1.0")
        if len(grid) - 1 > MAX_NUM_STEPS:
            raise ValueError(f"step schedule {key}: more than {MAX_NUM_STEPS} steps")
        if any(not math.isfinite(v) for v in grid):
            raise ValueError(f"step schedule {key}: non-finite grid value")
        if grid[0] != 0.0 or grid[-1] != 1.0:
            raise ValueError(f"step schedule {key}: the grid starts at 0.0 and ends at 1.0 (got {grid[0]!r} .. {grid[-1]!r})")
        if any(not b > a for a, b in zip(grid, grid[1:])):
            raise ValueError(f"step schedule {key}: the grid must be strictly increasing")
        out[key] = grid
    return out


def uniform_schedule(k: int, num_blocks: int = NUM_BLOCKS) -> dict:
    """k equal steps for every integration."""
    if int(k) != k or k < 1:
        raise ValueError("uniform_schedule: k >= 1 steps")
    k = int(k)
    grid = tuple([j / k for j in range(k)] + [1.0])
    return {key: grid for key in schedule_keys(num_blocks)}


def refine_schedule(schedule, m: int) -> dict:
    """Every step cut into m equal parts (m = 1: the schedule itself, validated)."""
    if int(m) != m or m < 1:
        raise ValueError("refine_schedule: m >= 1")
    m = int(m)
    nb = 1 + max((k[0] for k in schedule if isinstance(k, tuple) and len(k) == 2 and isinstance(k[0], int)), default=NUM_BLOCKS - 1)
    out = {}
    for key, grid in validate_schedule(schedule, nb).items():
        fine = []
        for a, b in zip(grid, grid[1:]):
            fine += [a + (b - a) * (j / m) for j in range(m)]
        out[key] = tuple(fine + [1.0])
    return validate_schedule(out, nb)


def save_schedule(schedule, path) -> None:
    """JSON: {"format", "version", "integrations": [{"block", "reverse", "grid"}]}, in running order.  float64 round-trips."""
    import json
    nb = 1 + max(k[0] for k in schedule)
    sched = validate_schedule(schedule, nb)
    doc = dict(format=SCHEDULE_FORMAT, version=1,
               integrations=[dict(block=i, reverse=r, grid=list(sched[(i, r)])) for i, r in schedule_keys(nb)])
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


def load_schedule(path) -> dict:
    import json
    with open(path) as fh:
        try:
            doc = json.load(fh)
        except json.JSONDecodeError as err:
            raise ValueError(f"{path}: not a step-schedule file ({err})") from None
    if not isinstance(doc, dict) or doc.get("format") != SCHEDULE_FORMAT or not isinstance(doc.get("integrations"), list):
        raise ValueError(f"{path}: not a step-schedule file (format {SCHEDULE_FORMAT!r})")
    sched = {}
    for ent in doc["integrations"]:
        if not isinstance(ent, dict) or not {"block", "reverse", "grid"} <= set(ent):
            raise ValueError(f"{path}: an integration entry holds block, reverse and grid")
        key = (int(ent["block"]), bool(ent["reverse"]))
        if key in sched:
            raise ValueError(f"{path}: integration {key} is listed twice")
        sched[key] = ent["grid"]
    return validate_schedule(sched, 1 + max((k[0] for k in sched), default=0))


def schedule_from_steps(step_lists, T_ends) -> dict:
    """The grids of recorded (s, h) lists (`last_train_steps` order: `schedule_keys`) of integrations over T_ends[block]:
    g_k = (h_0 + .. + h_{k-1}) / T, the last one 1.0 - so that fl32(T (g_{k+1} - g_k)) gives back the fp32 h_k of every step but
    the last, which is cut to end on t1 (`schedule_step_lists`)."""
    nb = len(T_ends)
    out = {}
    for key, steps in zip(schedule_keys(nb), step_lists):
        T = float(T_ends[key[0]])
        if not steps:
            raise ValueError(f"schedule_from_steps: integration {key} recorded no step")
        grid, acc = [0.0], 0.0
        for _, h in steps[:-1]:
            acc += float(h)
            grid.append(acc / T)
        out[key] = tuple(grid + [1.0])
    return validate_schedule(out, nb)


def schedule_step_lists(deltas: Tensor, last: Tensor, rev: Tensor, T: Tensor) -> Tensor:
    """The (s, h) lists of n integrations from their grids, in fp32, by the contiguity rule of the taped controller
    (csrc/cnf.hip: cnf_ctl_update_taped): s_0 = t0, h_k = fl(T d_k), s_{k+1} = s_k + h_k in fp32, and the last step cut to end on
    t1: h = fl(t1 - s).  Works on any device, without a host read.
    deltas [n, m] float64: g_{k+1} - g_k per row, zero-padded; last [n] int64: index of each row's last step; rev [n] bool;
    T [n] float64: the end times.  -> [n, m, 2] float32; row j's list is its first last[j] + 1 entries."""
    n, m = deltas.shape
    t0 = torch.where(rev, -T, torch.zeros_like(T))
    t1 = torch.where(rev, torch.zeros_like(T), T)
    out = torch.empty((n, m, 2), dtype=torch.float32, device=deltas.device)
    S, H = out[:, :, 0], out[:, :, 1]
    H.copy_((T[:, None] * deltas).to(torch.float32))
    S[:, 0] = t0.to(torch.float32)
    for k in range(m - 1):                                   # a sequential fp32 sum: one add over all rows per step
        torch.add(S[:, k], H[:, k], out=S[:, k + 1])
    li = last[:, None]
    H.scatter_(1, li, (t1[:, None] - S.gather(1, li).to(torch.float64)).to(torch.float32))
    return out


class _ScheduleDev:
    """A schedule's constants on the device (made once, outside any capture): the grid differences of the twelve integrations in
    running order, padded to the longest, and what `schedule_step_lists` needs beside the end times."""

    def __init__(self, schedule: dict, device: torch.device, num_blocks: int = NUM_BLOCKS):
        self.schedule = schedule
        self.keys = schedule_keys(num_blocks)
        self.n = [len(schedule[k]) - 1 for k in self.keys]
        m = max(self.n)
        d = torch.zeros((len(self.keys), m), dtype=torch.float64)
        for j, k in enumerate(self.keys):
            g = torch.tensor(schedule[k], dtype=torch.float64)
            d[j, :self.n[j]] = g[1:] - g[:-1]
        self.deltas = d.to(device)
        self.last = torch.tensor([n - 1 for n in self.n], dtype=torch.int64).to(device)
        self.rev = torch.tensor([r for _, r in self.keys]).to(device)
        self.block = torch.tensor([i for i, _ in self.keys], dtype=torch.int64).to(device)
        self.device = device

    def lists(self, T_blocks: Tensor) -> Tensor:
        """T_blocks [num_blocks] float64 on the device -> steps [12, m, 2] float32."""
        return schedule_step_lists(self.deltas, self.last, self.rev, T_blocks.index_select(0, self.block))


# ---- parameter holders (key names of the reference) ------------------------------------------------
class _ConcatSquashParams(nn.Module):
    """diffeq_layers.py:72-86."""

    def __init__(self, din: int, dout: int, dc: int):
        super().__init__()
        self._layer = nn.Linear(din, dout)
        self._hyper_bias = nn.Linear(1 + dc, dout, bias=False)
        self._hyper_gate = nn.Linear(1 + dc, dout)


class _ODEnetParams(nn.Module):
    def __init__(self, dc: int):
        super().__init__()
        self.layers = nn.ModuleList([_ConcatSquashParams(3, 64, dc), _ConcatSquashParams(64, 64, dc),
                                     _ConcatSquashParams(64, 3, dc)])


class _ODEfuncParams(nn.Module):
    def __init__(self, dc: int):
        super().__init__()
        self.diffeq = _ODEnetParams(dc)
        self.register_buffer("_num_evals", torch.tensor(0.))


class _CNFParams(nn.Module):
    def __init__(self, dc: int):
        super().__init__()
        self.register_parameter("sqrt_end_time", nn.Parameter(torch.sqrt(torch.tensor(0.5))))     # cnf.py:41
        self.odefunc = _ODEfuncParams(dc)


class _CNFBlockParams(nn.Module):
    def __init__(self, dc: int):
        super().__init__()
        self.cnf = _CNFParams(dc)


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

    def _init_kernels(self, device: torch.device) -> None:
        self.lib = _lib.load()
        self.device = device
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
        T = self.T_end[i]
        t0, t1 = (0.0, T) if not reverse else (-T, 0.0)
        if ctx is None:
            ctx = self.context(i, c)
        n_tot = float(rows * 4 + c.numel() * R)                 # the context is a state of the reference's ODE: it enters the norms
        if d0c is None:
            d0c = torch.empty(1, dtype=torch.float64, device=dev)
            self.context_norm(c, d0c)
        fbuf =torch.empty((2, rows, 4), dtype=torch.float32, device=dev)
        cap = max(1, int(cap))
        while True:
            states = torch.empty((cap + 1, rows, 4), dtype=torch.float32, device=dev)
            steps = torch.empty((cap, 2), dtype=torch.float32, device=dev)
            self._cnf_init(i, self.ctl, x, states[0], fbuf[0], ctx, e, t0, t1, n_tot, d0c, float(R), reverse, rows, R)
            f_start = fbuf[0].clone()                           # needed for dT when reversed; fbuf ping-pongs from here on
            attempts, batch = 0, self.first_batch
            while True:
                self._cnf_steps_taped(i, self.ctl, states, steps, fbuf, ctx, e, rows, R, batch)
                attempts += batch
                st = self.ctl.cpu()                             # the one device->host read per batch of attempts
                if st[5] != 0:
                    break
                if attempts > MAX_NUM_STEPS:
                    raise _lib.PuflowHipError(f"dopri5: more than {MAX_NUM_STEPS} step attempts in block {i}")
                batch = self.next_batch
            self.nfe += int(st[8])
            if st[9] != 3:
                break
            if cap > MAX_NUM_STEPS:
                raise _lib.PuflowHipError(f"dopri5: more than {MAX_NUM_STEPS} accepted steps in block {i}")
            cap *= 2
        t, dt = float(st[0]), float(st[1])
        if st[9] == 1:
            raise _lib.PuflowHipError(f"dopri5: non-finite error norm in block {i} at t = {t:g}")
        if st[9] == 2:
            raise _lib.PuflowHipError(f"dopri5: underflow in dt ({dt:g}) at t = {t:g}, block {i}")
        n = int(st[6])
        host = [(float(s), float(h)) for s, h in steps[:n].cpu().tolist()]
        return states[n], dict(steps=host, steps_dev=steps[:n], states=states[:n], ctx=ctx, f_start=f_start, f_end=fbuf[int(st[4])],
                               took=int(st[6]) + int(st[7]))

    def replay(self, i: int, x: Tensor, steps_dev: Tensor, reverse: bool, ctx: Tensor, e: Tensor, R: int, tape: bool = False,
               errsq: Optional[Tensor] = None):
        """pf_cnf_replay (csrc/cnf_replay.hip): block i integrated on the step list steps_dev [n, 2] (device floats (s, h)) in ONE
        launch, no controller.  x [rows, >= 3], row stride 3 or 4 floats.  tape: also write the states [n + 1, rows, 4] and the
        derivatives at both ends - the tape `tape_vjp` sweeps.  errsq [n] (device doubles): the per-step error sums.
        -> (state [rows,4], tape dict | None)"""
        rows, n = x.shape[0], int(steps_dev.shape[0])
        dev = x.device
        if x.dtype != torch.float32 or x.stride(1) != 1 or x.stride(0) not in (3, 4):
            x = x.float().contiguous()[:, :3].contiguous()
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
        self._init_kernels(device)
        self.R = upratio
        self.base = _Engine(_discrete_shell(sd), device)
        self.split = []
        for i in range(NUM_BLOCKS):
            rec = self._add_block(sd, i)
            # PF_CNF_SPLIT_GATES (include/puflow_hip.h): only where the factored 2^x cannot overflow; PF_CNF_SPLIT=0 keeps the plain kernel
            self.split.append(int(cnf_split_ok(rec, self.T_end[i]) and os.environ.get("PF_CNF_SPLIT", "1") != "0"))
        self.ws3k = torch.empty(3072, dtype=torch.float64, device=device)
        self.ctl = torch.zeros(16, dtype=torch.float64, device=device)       # dopri5 controller state (csrc/cnf.hip; zero before its first use)
        self.first_batch = int(os.environ.get("PF_CNF_FIRST_BATCH", "8"))    # step attempts enqueued before the first look
        self.next_batch = int(os.environ.get("PF_CNF_NEXT_BATCH", "4"))
        # attempts enqueued per integration when the whole forward runs WITHOUT reading the controller in between (attempts past
        # the end are ~4 us no-ops; an integration that needs more makes the forward fall back to the look-per-batch loop); 0 = off
        self.async_attempts = int(os.environ.get("PF_CNF_ASYNC_ATTEMPTS", "1"))             # 0 = never run blind
        self.logs = torch.zeros((2 * NUM_BLOCKS, 16), dtype=torch.float64, device=device)   # controller state after each integration
        # step attempts each of the twelve integrations took the last time (accepted + rejected): the blind run enqueues that
        # many + a margin (the trained model's blocks differ by 10x: 3 attempts for the short ones, 25 for the T = 36 block)
        self.hint: Optional[List[int]] = None
        self.accepted = 0
        self.rejected = 0

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
        T = self.T_end[i]
        t0, t1 = (0.0, T) if not reverse else (-T, 0.0)
        n_tot = float(rows * 4 + extra_n)
        if x.dtype != torch.float32 or x.stride(1) != 1 or x.stride(0) not in (3, 4):
            x = x.float().contiguous()[:, :3].contiguous()
        bufs = torch.empty((5, rows, 4), dtype=torch.float32, device=dev)
        y, f0, out = bufs[0], bufs[2], bufs[4]
        # the state rows (x, 0), f0 and torchdiffeq's initial step size, on the device in two launches (csrc/cnf.hip:
        # pf_cnf_init); the controller state follows
        ctl = self.ctl if log is None else log
        if not isinstance(extra_d0, torch.Tensor):
            extra_d0 = torch.tensor([float(extra_d0)], dtype=torch.float64, device=dev) if extra_d0 else None
        self._cnf_init(i, ctl, x, y, f0, ctx, e, t0, t1, n_tot, extra_d0, extra_scale, reverse, rows, R)

        # ---- adaptive steps: ONE launch per attempt (six fused stage evaluations); the accept / reject / next-dt decisions are
        # taken on the device (csrc/cnf.hip: cnf_ctl_update, run by the workgroup of a step attempt that finishes last), the host
        # enqueues a batch of attempts and reads the controller state once per batch (attempts past the end are no-ops)
        if log is not None:
            self._cnf_steps(i, ctl, bufs, ctx, e, rows, R, blind)
            return out
        attempts = 0
        batch = self.first_batch
        while True:
            self._cnf_steps(i, ctl, bufs, ctx, e, rows, R, batch)
            attempts += batch
            st = ctl.cpu()                                      # the one device->host read per batch of attempts
            if st[5] != 0:
                break
            if attempts > MAX_NUM_STEPS:
                raise _lib.PuflowHipError(f"dopri5: more than {MAX_NUM_STEPS} step attempts in block {i}")
            batch = self.next_batch
        t, dt = float(st[0]), float(st[1])
        self.last_attempts = int(st[6]) + int(st[7])
        self.accepted += int(st[6])
        self.rejected += int(st[7])
        self.nfe += int(st[8])
        # torchdiffeq raises here too ('underflow in dt', NaN propagates into dt): without these guards a NaN error norm
        # makes every comparison False - no step is ever accepted and dt grows tenfold per attempt, forever
        if st[9] == 1:
            raise _lib.PuflowHipError(f"dopri5: non-finite error norm in block {i} at t = {t:g} (NaN / inf in the input, "
                                      "the weights or the state)")
        if st[9] == 2:
            raise _lib.PuflowHipError(f"dopri5: underflow in dt ({dt:g}) at t = {t:g}, block {i}")
        return out

    def time_step_attempts(self, i: int, x: Tensor, ctx: Tensor, e: Tensor, R: int, reverse: bool, extra_n: int, extra_d0,
                           attempts: int, extra_scale: float = 1.0):
        """bench.py's roofline leg: ONE integration of block i enqueued without a look at the controller, HIP events on the launch
        stream around the `attempts` step attempts alone (pf_cnf_steps: the kernel of the timed forward, cnf_step_dev_kernel) ->
        (milliseconds for all attempts, attempts the integration really took = accepted + rejected; the rest were no-ops)."""
        rows = x.shape[0]
        T = self.T_end[i]
        t0, t1 = (0.0, T) if not reverse else (-T, 0.0)
        x = x.float().contiguous()[:, :3].contiguous()
        bufs = torch.empty((5, rows, 4), dtype=torch.float32, device=x.device)
        ctl = torch.zeros(16, dtype=torch.float64, device=x.device)
        self._cnf_init(i, ctl, x, bufs[0], bufs[2], ctx, e, t0, t1, rows * 4 + extra_n, extra_d0, extra_scale, reverse, rows, R)
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
        self.first_batch, self.next_batch = 8, 4                             # step attempts enqueued per look at the controller
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
        if ctx is None:
            ctx = self.context(i, c)
        n_tot = float(rows * 4 + c.numel() * R)
        if d0c is None:
            d0c = torch.empty(1, dtype=torch.float64, device=dev)
            self.context_norm(c, d0c)
        fbuf = torch.empty((2, rows, 4), dtype=torch.float32, device=dev)
        states = torch.empty((cap + 1, rows, 4), dtype=torch.float32, device=dev)
        steps = torch.empty((cap, 2), dtype=torch.float32, device=dev)
        if self.T_end[i] is None:
            self._cnf_init_dev(i, log, x, states[0], fbuf[0], ctx, e, n_tot, d0c, float(R), reverse, rows, R)
        else:
            T = self.T_end[i]
            t0, t1 = (0.0, T) if not reverse else (-T, 0.0)
            self._cnf_init(i, log, x, states[0], fbuf[0], ctx, e, t0, t1, n_tot, d0c, float(R), reverse, rows, R)
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
        T = self.T_end[i]
        t0, t1 = (0.0, T) if not reverse else (-T, 0.0)
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
            if not math.isfinite(ratio):
                raise _lib.PuflowHipError(f"dopri5: non-finite error norm in block {i} at t = {t:g}")
            if not (t + h > t):
                raise _lib.PuflowHipError(f"dopri5: underflow in dt ({h:g}) at t = {t:g}, block {i}")
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


# ---- the deferred controller: twelve log rows + the sticky table, one read ------------------------------------------
PACK_ROW = 2 * NUM_BLOCKS                  # the sticky table's row of pf_cnf_pack_status, behind the twelve integrations'


def _log_row(i: int, reverse: bool) -> int:
    """Row of integration (block i, direction) in the log and sticky tables: the order they run in, f's 0 .. 5 then g's 5 .. 0."""
    return 2 * NUM_BLOCKS - 1 - i if reverse else i


def _row_key(k: int):
    return (k, False) if k < NUM_BLOCKS else (2 * NUM_BLOCKS - 1 - k, True)


class _DeferredPlan:
    """What a deferred train-mode forward hands its nodes: the net's tape budgets, its log rows and sticky table."""

    def __init__(self, net: "PointInterpFlow", dev: torch.device):
        self.logs, self.sticky = net._train_tables(dev)
        self.budget = net.tape_budget
        self.budget_cap0 = 32
        self.learning = any((i, r) not in self.budget for i in range(net.num_blocks) for r in (False, True))


class _SchedulePlan:
    """What a train-mode forward on a frozen step schedule hands its nodes: the sticky table (the weight pack's status
    stays on the device, as under the deferred controller) and, once the weights are packed, the twelve step lists made on the
    device from the pack's end times.  No budgets, no log rows: a replay cannot fall short."""
    learning = False                                             # `_CnfPackFn`: never read the pack's meta row

    def __init__(self, net: "PointInterpFlow", dev: torch.device):
        self.logs, self.sticky = net._train_tables(dev)
        self.sdev = net._schedule_dev(dev)
        self.steps: Optional[Tensor] = None

    def bind(self, pack: "_DevicePack") -> None:
        self.steps = self.sdev.lists(pack.meta[:, 0])

    def list_of(self, i: int, reverse: bool) -> Tensor:
        k = _log_row(i, reverse)
        return self.steps[k, :self.sdev.n[k]]


class _FlowBlockFn(torch.autograd.Function):
    """(x, c, parameters of block i) -> (x', delta logp): `PointInterpFlow.flow_block`."""

    @staticmethod
    def forward(fctx, x, c, e, i, R, reverse, keys, record, opts, *params):
        if opts["controller"] in ("deferred", "schedule"):       # the same launch, its meta row stays on the device
            by_key = dict(zip(keys, params))
            pack = _DevicePack([[by_key[k] for k in _pack_keys(i)]], x.device, sticky=opts["sticky"][PACK_ROW], read_meta=False)
            eng = _BlockTapeEngine(None, i, x.device, pack=(pack, 0))
        elif opts["pack"] == "device":                           # one launch on the live parameters, one read of its meta row
            by_key = dict(zip(keys, params))
            eng = _BlockTapeEngine(None, i, x.device, pack=(_DevicePack([[by_key[k] for k in _pack_keys(i)]], x.device), 0))
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
        rows = tape["f_end"].shape[0]
        ybar = torch.zeros((rows, 4), dtype=torch.float32, device=c.device)
        if gx is not None:
            ybar[:, :3] = gx
        if gl is not None:
            ybar[:, 3] = gl
        y0bar, grad, ctxbar = eng.tape_backward(i, tape, ybar, c, e, R, reverse, sweep)
        # ctx = [1 | c] [hb | Hc]^T:  one GEMM for d(hb | Hc) = ctxbar^T [1 | c] (column 0: the column sums), one for dc
        T, cd = c.shape
        c1 = torch.cat([torch.ones((T, 1), dtype=torch.float32, device=c.device), c], dim=1).contiguous()
        dH1 = torch.empty((CNF_CTX, cd + 1), dtype=torch.float32, device=c.device)
        _gemm(ctxbar, 1, CNF_CTX, c1, cd + 1, 1, dH1, cd + 1, None, CNF_CTX, cd + 1, T)
        dc = torch.empty((T, cd), dtype=torch.float32, device=c.device)
        _gemm(ctxbar, CNF_CTX, 1, eng.Hplain, cd, 1, dc, cd, None, T, cd, CNF_CTX)
        grads = unpack_cnf_grads(i, grad, dH1[:, 1:], dH1[:, 0])
        # end time T = sqrt_end_time^2 by the CONTINUOUS formula (not the derivative of the discrete scheme): the solution moves
        # along the solver's derivative at the end whose time is T - the final state going forward, the start going backward
        dT = (ybar * tape["f_end"]).sum() if not reverse else (y0bar * tape["f_start"]).sum()
        out = []
        for k, p in zip(keys, params):
            if k.endswith("sqrt_end_time"):
                out.append((dT * 2.0 * p.detach()).reshape(p.shape).to(p.dtype))
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
    read.  One pf_cnf_pack_blocks launch; the engines are left in `engs`."""

    @staticmethod
    def forward(fctx, engs, plan, *params):
        nb = len(params) // 16
        dev = params[0].device
        # plan (a deferred forward): the status goes to the sticky table; the meta row is read only by a forward that still has
        # an integration to run through the host-read loop (no budget yet), which needs the end times as host floats
        pack = (_DevicePack([list(params[16 * j:16 * j + 16]) for j in range(nb)], dev) if plan is None else
                _DevicePack([list(params[16 * j:16 * j + 16]) for j in range(nb)], dev, sticky=plan.sticky[PACK_ROW],
                            read_meta=plan.learning))
        for j in range(nb):
            engs.append(_BlockTapeEngine(None, j, dev, pack=(pack, j), scratch=engs[0] if engs else None))
        if isinstance(plan, _SchedulePlan):
            plan.bind(pack)
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
    d[hb | Hc] = ctxbar^T [1 | c] (one GEMM, handed to `_CnfPackFn` through h1) and dc = ctxbar Hplain (one GEMM)."""

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
        T, cd = c.shape
        ctxbar = ctxbar.contiguous()
        c1 = torch.cat([torch.ones((T, 1), dtype=torch.float32, device=c.device), c], dim=1).contiguous()
        dH1 = torch.empty((CNF_CTX, cd + 1), dtype=torch.float32, device=c.device)
        _gemm(ctxbar, 1, CNF_CTX, c1, cd + 1, 1, dH1, cd + 1, None, CNF_CTX, cd + 1, T)
        dc = torch.empty((T, cd), dtype=torch.float32, device=c.device)
        _gemm(ctxbar, CNF_CTX, 1, fctx.eng.Hplain, cd, 1, dc, cd, None, T, cd, CNF_CTX)
        return None, None, dc.to(fctx.cdt), dH1


class _CnfIntegrateFn(torch.autograd.Function):
    """One taped integration of block i: (x [rows,3], ctx [T,288]) -> (x' [rows,3], delta logp [rows]).  Backward: one
    pf_cnf_tape_vjp launch -> xbar, this direction's ctxbar and gradient record (through grec to `_CnfPackFn`), and
    sqrt_end_time's gradient by the continuous formula."""

    @staticmethod
    def forward(fctx, eng, i, R, reverse, caps, steps_out, c, d0c, e, x, ctx, grec, sqrt_t):
        x32 = x.detach().float().contiguous()
        plan = caps if isinstance(caps, _DeferredPlan) else None
        budget = plan.budget.get((i, reverse)) if plan is not None else None
        if isinstance(caps, _SchedulePlan):                      # a frozen schedule: ONE launch, nothing to look at
            y, tape = eng.replay(i, x32, caps.list_of(i, reverse), reverse, ctx.detach(), e, R, tape=True)
            steps_out.append(tape)
        elif budget is not None:                                   # no look at the controller: `check_train_logs` reads it later
            k = _log_row(i, reverse)
            y, tape = eng.tape_forward_deferred(i, x32, c, e, R, reverse, budget[0], budget[1], plan.logs[k], plan.sticky[k],
                                                ctx=ctx.detach(), d0c=d0c)
            steps_out.append(tape)
        else:
            if plan is not None and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"deferred CNF training: block {i} ({'g' if reverse else 'f'}) has no tape budget yet - run one "
                                   "eager step before capturing (graphed_train_step's warm-up does)")
            cap0 = plan.budget_cap0 if plan is not None else caps.get((i, reverse), 32)
            y, tape = eng.tape_forward(i, x32, c, e, R, reverse, cap0, ctx=ctx.detach(), d0c=d0c)
            n = len(tape["steps"])
            if plan is not None:                                 # learn: attempts taken + a quarter + 2, steps + an eighth + 2
                plan.budget[(i, reverse)] = (tape["took"] + tape["took"] // 4 + 2, n + n // 8 + 2)
            else:
                caps[(i, reverse)] = n + n // 8 + 2
            steps_out.append(tape["steps"])
        fctx.eng, fctx.tape, fctx.args = eng, tape, (i, R, reverse, x.dtype, c.shape[0])
        fctx.save_for_backward(e, sqrt_t)
        return y[:, :3].contiguous(), y[:, 3].contiguous()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, gx, gl):
        i, R, reverse, xdt, T = fctx.args
        e, sqrt_t = fctx.saved_tensors
        eng, tape = fctx.eng, fctx.tape
        rows = tape["f_end"].shape[0]
        dev = e.device
        ybar = torch.zeros((rows, 4), dtype=torch.float32, device=dev)
        if gx is not None:
            ybar[:, :3] = gx
        if gl is not None:
            ybar[:, 3] = gl
        y0bar = ybar.clone()
        grad = torch.zeros(CNF_GRAD, dtype=torch.float32, device=dev)
        ctxbar = torch.zeros((T, CNF_CTX), dtype=torch.float32, device=dev)
        if tape.get("deferred"):
            eng.tape_vjp_dev(i, tape, 1.0 if not reverse else -1.0, e, y0bar, ctxbar, grad, rows, R)
        else:
            eng.tape_vjp(i, tape["states"].contiguous(), tape["steps_dev"].contiguous(), 1.0 if not reverse else -1.0, tape["ctx"], e,
                         y0bar, ctxbar, grad, rows, R)
        dT = (ybar * tape["f_end"]).sum() if not reverse else (y0bar * tape["f_start"]).sum()      # as _FlowBlockFn
        dsq = (dT * 2.0 * sqrt_t.detach()).reshape(sqrt_t.shape).to(sqrt_t.dtype)
        return (None,) * 9 + (y0bar[:, :3].contiguous().to(xdt), ctxbar, grad, dsq)


def flow_train(net: "PointInterpFlow", xyz: Tensor, R: int, cs: List[Tensor], branch, noise: Optional[List[Tensor]] = None):
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
        noise = getattr(net, "train_noise", None)                # fixed vectors for every step (a reproducibility switch)
    if noise is None:
        noise = [torch.randn(B, N, 3, device=dev) for _ in range(nb)]
    es = [n.detach().reshape(T, 3).contiguous().float() for n in noise]
    engs: List[_BlockTapeEngine] = []
    params = [p for blk in net.flow_blocks for p in _pack_params(blk)]
    scheduled = getattr(net, "step_schedule", None) is not None
    plan = (_SchedulePlan(net, dev) if scheduled else _DeferredPlan(net, dev) if getattr(net, "train_deferred", False) else None)
    stand = _CnfPackFn.apply(engs, plan, *params)
    cflat, ctx, d0c = [], [], torch.empty(nb, dtype=torch.float64, device=dev)
    for i in range(nb):
        ci = cs[i].reshape(T, -1)
        cflat.append(ci.detach().float().contiguous())
        ctx.append(_CnfContextFn.apply(engs[i], i, ci, stand[nb + i]))
        if not scheduled:                                    # (a replay takes no norm)
            engs[i].context_norm(cflat[i], d0c[i:i + 1])         # the context is a state of the reference's ODE: it enters the norms
    steps: list = []
    caps = net.tape_capacity if plan is None else plan
    # ---- f + log-likelihood (oracle/cnf_ref.py::forward)
    p = xyz.reshape(T, 3)
    ldj = None
    for i in range(nb):
        p, dl = _CnfIntegrateFn.apply(engs[i], i, 1, False, caps, steps, cflat[i], d0c[i:i + 1], es[i], p, ctx[i], stand[i],
                                      net.flow_blocks[i].cnf.sqrt_end_time)
        ldj = dl if ldj is None else ldj + dl
    z = p.view(B, N, 3)
    logp = -torch.mean(torch.sum(-0.5 * (z ** 2 + math.log(2 * math.pi)), dim=(1, 2)) - ldj.view(B, N).sum(dim=1))
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
        u, _ = _CnfIntegrateFn.apply(engs[i], i, R, True, caps, steps, cflat[i], d0c[i:i + 1], es[i], u, ctx[i], stand[i],
                                     net.flow_blocks[i].cnf.sqrt_end_time)
    net.last_train_steps = steps
    return u.view(B, N * R, 3), logp


def forward_train(net: "PointInterpFlow", xyz: Tensor, upratio: int, noise: Optional[List[Tensor]] = None):
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


class PointInterpFlow(nn.Module):
    """Reference surface: modules/continuous/interpflow.py:53-139 (the continuous `PointInterpFlow`)."""

    def __init__(self, pc_channel: int = 3):
        super().__init__()
        if pc_channel != 3:
            raise ValueError("the HIP path is built for 3-D points (pc_channel=3)")
        self.num_blocks = NUM_BLOCKS
        self.num_neighbors = 16
        self.interp = _InterpParams()
        self.feat_convs = nn.ModuleList(
            [_EdgeConvParams(FEAT_CHANNELS[i], FEAT_CHANNELS[i + 1], GROWTH[i]) for i in range(NUM_BLOCKS)])
        self.merge_convs = nn.ModuleList(
            [_MergeParams(FEAT_CHANNELS[i + 1], COND_CHANNELS[i]) for i in range(NUM_BLOCKS)])
        self.flow_blocks = nn.ModuleList([_CNFBlockParams(COND_CHANNELS[i]) for i in range(NUM_BLOCKS)])
        self._engine_cache: Optional[_CnfEngine] = None
        self.last_stats: dict = {}
        # flow_block's device-side tape: steps to allocate it for, per (block, reverse) - what the last call took + an eighth + 2
        self.tape_capacity: dict = {}
        # ---- the deferred controller of the train-mode forward, off by default
        self.train_deferred = False               # no look at a controller inside the forward: `check_train_logs` reads them all, later
        self.tape_budget: dict = {}               # (block, reverse) -> (attempts to enqueue, tape capacity); learnt from a host-read run
        self.train_noise: Optional[List[Tensor]] = None       # fixed Hutchinson vectors for every training forward (default: drawn)
        self._train_tab: Optional[Tensor] = None  # the twelve log rows and the sticky table, one buffer = one read
        self._sticky_seen = None                  # the sticky table at the last `check_train_logs`
        self._logs_host = None
        self._last_steps = None
        self.last_skipped_steps = 0
        # ---- a frozen step schedule: None (the default) leaves every path on the adaptive solver
        self._step_schedule: Optional[dict] = None
        self._sched_dev: Optional[_ScheduleDev] = None
        self._sched_err = None                    # (errsq [12, m] device doubles, n_tot per integration) of the last scheduled eval forward
        self.last_record: dict = {}               # what `record_schedule` computed on the way: x, logp, the recorded step lists
        # (file, refine) | None: the first eval forward records its input's schedule, saves it there and switches it on
        self.record_first: Optional[tuple] = None

    # -- the frozen step schedule
    @property
    def step_schedule(self) -> Optional[dict]:
        """None: adaptive Dormand-Prince everywhere (the default).  A schedule (`uniform_schedule`, `record_schedule`,
        `load_schedule`): the eval forward and the train-mode forward integrate on its step grids, one `pf_cnf_replay` launch per
        integration, no controller.  Assigning validates (ValueError)."""
        return self._step_schedule

    @step_schedule.setter
    def step_schedule(self, schedule) -> None:
        self._step_schedule = None if schedule is None else validate_schedule(schedule, self.num_blocks)
        self._sched_dev = None
        self._sched_err = None
        if self._engine_cache is not None:
            self._engine_cache.sched_lists = None

    def _schedule_dev(self, dev: torch.device) -> _ScheduleDev:
        """The schedule's constants on the device, uploaded once per schedule (before any capture)."""
        if self._step_schedule is None:
            raise ValueError("no step schedule is set")
        if self._sched_dev is None or self._sched_dev.device != dev:
            self._sched_dev = _ScheduleDev(self._step_schedule, dev, self.num_blocks)
        return self._sched_dev

    def schedule_error_ratios(self) -> dict:
        """After an eval forward on a schedule: per integration (block, reverse) the embedded error estimate's ratio of every
        step, sqrt(errsq / n_tot) - the number the adaptive controller accepts a step on when it is <= 1 (n_tot counts the
        context's elements too, as there).  A schedule whose ratios are far above 1 is too coarse for this input:
        `refine_schedule`.  The one device -> host read of a scheduled forward, made here."""
        if self._sched_err is None:
            raise ValueError("schedule_error_ratios: no eval forward has run on the current step schedule")
        errsq, n_tot, keys, ns = self._sched_err
        host = errsq.cpu()
        return {k: [math.sqrt(float(v) / n_tot[j]) for v in host[j, :ns[j]]] for j, k in enumerate(keys)}

    @torch.no_grad()
    def record_schedule(self, xyz: Tensor, upratio: int = 4, noise: Optional[List[Tensor]] = None, refine: int = 1) -> dict:
        """The schedule of the adaptive solver's own accepted steps on the calibration input xyz [B,N,3]: the twelve integrations
        run with the taped device controller (`tape_forward`: the last step cut to end on the end time, so the result IS the
        recorded steps) on the eval plan's features, no gradients.  -> the schedule, every step cut into `refine` parts; with
        refine = 1 and the same input and noise, a scheduled eval forward replays these integrations bit for bit.
        `last_record`: x [B, N upratio, 3] and logp of this taped forward, the recorded (s, h) lists, accepted / rejected counts.
        Does not touch `step_schedule`: assign the result to switch it on."""
        if not xyz.is_cuda:
            raise _lib.PuflowHipError("input must be a GPU tensor (no CPU fallback)")
        if self.training:
            self.invalidate_plan()                               # the eval plan packs the weights as they are NOW
        xyz = xyz.detach().contiguous().float()
        B, N, _ = xyz.shape
        T = B * N
        eng = self._engine(upratio)
        base = eng.base
        idx16 = base.knn(xyz)
        cs, _, _ = base.features(xyz, idx16, want_cs=True, cs_only=True)
        if noise is None:
            noise = [torch.randn(B, N, 3, device=xyz.device) for _ in range(NUM_BLOCKS)]
        es = [n.reshape(T, 3).contiguous().float() for n in noise]
        cflat = [c.reshape(T, -1).contiguous() for c in cs]
        ctx = [eng.context(i, cflat[i]) for i in range(NUM_BLOCKS)]
        d0c = torch.empty(NUM_BLOCKS, dtype=torch.float64, device=xyz.device)
        for i in range(NUM_BLOCKS):
            eng.context_norm(cflat[i], d0c[i:i + 1])
        lists, took, outs = [], 0, []
        p = xyz.reshape(T, 3)
        for i in range(NUM_BLOCKS):
            p, tape = eng.tape_forward(i, p, cflat[i], es[i], 1, False, ctx=ctx[i], d0c=d0c[i:i + 1])
            outs.append(p)
            lists.append(tape["steps"]); took += tape["took"]
        ldj = torch.stack([s_[:, 3] for s_ in outs]).view(NUM_BLOCKS, B, N).sum(dim=(0, 2))
        z = outs[-1][:, :3].reshape(B, N, 3)
        logp = -torch.mean(torch.sum(-0.5 * (z ** 2 + math.log(2 * math.pi)), dim=(1, 2)) - ldj)
        u = base.interp(xyz, z.contiguous(), idx16, upratio).reshape(T * upratio, 3)
        for i in reversed(range(NUM_BLOCKS)):
            u, tape = eng.tape_forward(i, u, cflat[i], es[i], upratio, True, ctx=ctx[i], d0c=d0c[i:i + 1])
            lists.append(tape["steps"]); took += tape["took"]
        accepted = sum(len(s) for s in lists)
        self.last_record = dict(x=u[:, :3].contiguous().view(B, N * upratio, 3), logp=logp, steps=lists, accepted=accepted,
                                rejected=took - accepted)
        if self.training:
            self.invalidate_plan()
        return refine_schedule(schedule_from_steps(lists, [eng.T_end[i] for i in range(NUM_BLOCKS)]), refine)

    def _forward_eval_schedule(self, xyz: Tensor, upratio: int, noise: Optional[List[Tensor]], stages: bool):
        """The eval forward on `step_schedule`: twelve pf_cnf_replay launches, no controllers, no hints, no host read."""
        B, N, _ = xyz.shape
        T = B * N
        dev = xyz.device
        eng = self._engine(upratio)
        eng.nfe = eng.accepted = eng.rejected = 0
        base = eng.base
        sdev = self._schedule_dev(dev)
        if getattr(eng, "sched_lists", None) is None or eng.sched_lists[0] is not sdev:
            T_blocks = torch.tensor([eng.T_end[i] for i in range(NUM_BLOCKS)], dtype=torch.float64).to(dev)
            eng.sched_lists = (sdev, sdev.lists(T_blocks))       # the end times are fixed in eval mode: made once per plan
        steps = eng.sched_lists[1]
        idx16 = base.knn(xyz)
        cs, _, _ = base.features(xyz, idx16, want_cs=True, cs_only=True)
        if noise is None:
            noise = [torch.randn(B, N, 3, device=dev) for _ in range(NUM_BLOCKS)]
        es = [n.reshape(T, 3).contiguous().float() for n in noise]
        cflat = [c.reshape(T, -1).contiguous() for c in cs]
        ctx = [eng.context(i, cflat[i]) for i in range(NUM_BLOCKS)]
        errsq = torch.zeros((2 * NUM_BLOCKS, steps.shape[1]), dtype=torch.float64, device=dev)
        n_tot, outs = [], []
        p = xyz.reshape(T, 3)
        for k, (i, reverse) in enumerate(sdev.keys):
            R = upratio if reverse else 1
            if k == NUM_BLOCKS:
                ldj = torch.stack([s_[:, 3] for s_ in outs]).view(NUM_BLOCKS, B, N).sum(dim=(0, 2))
                z = p[:, :3].reshape(B, N, 3)
                logp = -torch.mean(torch.sum(-0.5 * (z ** 2 + math.log(2 * math.pi)), dim=(1, 2)) - ldj)
                p = base.interp(xyz, z.contiguous(), idx16, upratio).reshape(T * upratio, 3)
            n = sdev.n[k]
            p, _ = eng.replay(i, p, steps[k, :n], reverse, ctx[i], es[i], R, errsq=errsq[k, :n])
            outs.append(p)
            n_tot.append(float(p.shape[0] * 4 + cflat[i].numel() * R))
        x = p[:, :3].contiguous().view(B, N * upratio, 3)
        self._sched_err = (errsq, n_tot, list(sdev.keys), list(sdev.n))
        self.last_stats = dict(nfe=sum(1 + 6 * n for n in sdev.n), accepted=sum(sdev.n), rejected=0, schedule=True)
        if stages:
            return dict(idx16=idx16, cs=cs, z=z, ldj=ldj, logp=logp, x=x, **self.last_stats)
        return x, logp

    # -- the deferred controller's tables
    def _train_tables(self, dev: torch.device):
        """(logs [12, 16] float64, sticky [13, 4] int32): views of one zero-initialised buffer that outlives every hipGraph
        capture (train_state._zeros_kept: inside a capture it would be a memset node that clears the sticky counts per replay)."""
        nl = 2 * NUM_BLOCKS * 16 * 2                             # the log rows, in 32-bit words
        if self._train_tab is None or self._train_tab.device != dev:
            from .train_state import _zeros_kept
            self._train_tab = _zeros_kept(nl + (2 * NUM_BLOCKS + 1) * 4, torch.int32, dev)
            self._sticky_seen = torch.zeros((2 * NUM_BLOCKS + 1, 4), dtype=torch.int32)
        t = self._train_tab
        return t[:nl].view(torch.float64).view(2 * NUM_BLOCKS, 16), t[nl:].view(2 * NUM_BLOCKS + 1, 4)

    def check_train_logs(self) -> int:
        """The ONE device -> host read of a deferred training forward (or of the replays of a captured step since the last
        call): the twelve controller rows and the sticky table.  Since the last call:
          * a weight pack with a status raises the host packers' ValueError;
          * an integration that ended with status 1 or 2 raises PuflowHipError, the eager path's messages - unless an
            integration BEFORE it in the forward fell short: its NaN output is what the later one choked on;
          * an integration that fell short - its attempts ran out (sticky status 4) or its tape filled (3) - gets that budget
            doubled (up to MAX_NUM_STEPS); -> how many integrations fell short.  Their outputs were NaN: the step is void.
        `last_skipped_steps`: forwards since the last call with at least one integration that was not clean."""
        if self._train_tab is None:
            return 0
        host = self._train_tab.cpu()                             # the one read
        nl = 2 * NUM_BLOCKS * 16 * 2
        logs = host[:nl].view(torch.float64).view(2 * NUM_BLOCKS, 16)
        sticky = host[nl:].view(2 * NUM_BLOCKS + 1, 4)
        new_bad = (sticky[:, 1] - self._sticky_seen[:, 1]).tolist()
        self._sticky_seen = sticky.clone()
        self._logs_host = logs
        self.last_skipped_steps = max(new_bad[:PACK_ROW])
        if new_bad[PACK_ROW]:
            _DevicePack.raise_status(int(sticky[PACK_ROW, 3]), int(sticky[PACK_ROW, 2]))
        short = 0
        for k in range(PACK_ROW):
            if not new_bad[k]:
                continue
            i, reverse = _row_key(k)
            status = int(sticky[k, 2])
            if status in (3, 4):
                short += 1
                a, c = self.tape_budget.get((i, reverse), (0, 0))
                if status == 4:
                    a = min(max(2 * a, 2), MAX_NUM_STEPS)
                else:
                    c = min(max(2 * c, 2), MAX_NUM_STEPS)
                    a = max(a, c)                                # an accepted step is an attempt
                if (i, reverse) in self.tape_budget:
                    self.tape_budget[(i, reverse)] = (a, c)
            elif not short:
                t, dt = float(logs[k, 0]), float(logs[k, 1])
                if status == 1:
                    raise _lib.PuflowHipError(f"dopri5: non-finite error norm in block {i} at t = {t:g}")
                raise _lib.PuflowHipError(f"dopri5: underflow in dt ({dt:g}) at t = {t:g}, block {i}")
        return short

    def train_log_stats(self) -> dict:
        """From the tables as `check_train_logs` last read them: per integration, in running order, the attempts enqueued
        (budget), the most attempts any run took (the sticky table's max column) and the runs; `noop` = attempts enqueued per
        forward that returned at once because the integration was done (against the LARGEST count seen: a lower bound)."""
        if self._sticky_seen is None:
            return {}
        rows = []
        for k in range(PACK_ROW):
            a, c = self.tape_budget.get(_row_key(k), (0, 0))
            rows.append(dict(key=_row_key(k), attempts=a, cap=c, runs=int(self._sticky_seen[k, 0]), not_clean=int(self._sticky_seen[k, 1]),
                             max_took=int(self._sticky_seen[k, 3])))
        return dict(rows=rows, noop=sum(max(r["attempts"] - r["max_took"], 0) for r in rows if r["runs"]))

    @property
    def last_train_steps(self):
        """The twelve recorded step lists of the last train-mode forward, f's blocks 0 .. 5 then g's 5 .. 0.  After a deferred
        forward they are on the device: fetched on first access (one read per integration, and one of the log rows if
        `check_train_logs` has not run since)."""
        st = self._last_steps
        if st is not None and any(isinstance(t, dict) for t in st):
            out = []
            for t in st:
                if isinstance(t, dict) and t.get("schedule"):
                    t = [(float(s), float(h)) for s, h in t["steps_dev"].cpu().tolist()]
                elif isinstance(t, dict):
                    ctl = t["log"].cpu()
                    n = int(ctl[6]) if (ctl[5] != 0 and ctl[9] == 0) else 0
                    t = [(float(s), float(h)) for s, h in t["steps_dev"][:n].cpu().tolist()]
                out.append(t)
            st = self._last_steps = out
        return st

    @last_train_steps.setter
    def last_train_steps(self, steps) -> None:
        self._last_steps = steps

    def invalidate_plan(self) -> None:
        self._engine_cache = None

    def load_state_dict(self, *a, **kw):
        self.invalidate_plan()
        return super().load_state_dict(*a, **kw)

    def _apply(self, fn, *a, **kw):
        self.invalidate_plan()
        return super()._apply(fn, *a, **kw)

    def _engine(self, upratio: int) -> _CnfEngine:
        e = self._engine_cache
        dev = self.flow_blocks[0].cnf.sqrt_end_time.device
        if e is None or e.R != upratio or e.device != dev:
            if dev.type != "cuda":
                raise _lib.PuflowHipError("PointInterpFlow runs on the GPU only: move the module with .to('cuda')")
            e = _CnfEngine({k: v.detach().cpu() for k, v in self.state_dict().items()}, dev, upratio)
            self._engine_cache = e
        return e

    def set_to_initialized_state(self) -> None:      # continuous/interpflow.py:113-114: nothing to initialise
        pass

    def train(self, mode: bool = True):
        if bool(mode) != self.training:     # a switch: the eval plan holds packed copies of the weights - eval after an optimizer
            self.invalidate_plan()          # step packs anew (validation batches in a row, no switch between them, share one plan)
        return super().train(mode)

    def forward(self, xyz: Tensor, upratio: int = 4, noise: Optional[List[Tensor]] = None,
                stages: bool = False):
        """-> (x [B, N*upratio, 3], logp).  `noise[i]` [B,N,3]: block i's Hutchinson vector (default: torch.randn,
        like the reference, which draws it at the first right-hand-side call of f and re-uses it in g).
        In train() mode with gradients (`forward_train`: taped integrations, weights packed from the live parameters on the
        device); in eval() mode the inference plan, no autograd."""
        if not xyz.is_cuda:
            raise _lib.PuflowHipError("input must be a GPU tensor (no CPU fallback)")
        if self.training:
            if stages:
                raise ValueError("stages=True is an eval-mode option")
            return forward_train(self, xyz, upratio, noise)
        return self._forward_eval(xyz, upratio, noise, stages)

    @torch.no_grad()
    def _forward_eval(self, xyz: Tensor, upratio: int, noise: Optional[List[Tensor]], stages: bool):
        xyz = xyz.detach().contiguous().float()
        if self.record_first is not None:
            path, refine = self.record_first
            self.record_first = None
            if noise is None:                                    # one draw for the recording and the forward behind it
                noise = [torch.randn(xyz.shape[0], xyz.shape[1], 3, device=xyz.device) for _ in range(NUM_BLOCKS)]
            self.step_schedule = self.record_schedule(xyz, upratio, noise, refine)
            save_schedule(self.step_schedule, path)
        if self._step_schedule is not None:
            return self._forward_eval_schedule(xyz, upratio, noise, stages)
        B, N, _ = xyz.shape
        T = B * N
        eng = self._engine(upratio)
        eng.nfe = eng.accepted = eng.rejected = 0
        base = eng.base
        idx16 = base.knn(xyz)
        cs, _, _ = base.features(xyz, idx16, want_cs=True, cs_only=True)
        if noise is None:
            noise = [torch.randn(B, N, 3, device=xyz.device) for _ in range(NUM_BLOCKS)]
        es = [n.reshape(T, 3).contiguous().float() for n in noise]
        cflat = [c.reshape(T, -1).contiguous() for c in cs]
        ctx = [eng.context(i, cflat[i]) for i in range(NUM_BLOCKS)]
        # the context is a state of the reference's ODE (zero derivative): it only enters the solver's norms.  Six device words
        # (it was seven torch kernels per block and one host read in the middle of the forward)
        d0c = torch.empty(NUM_BLOCKS, dtype=torch.float64, device=xyz.device)
        for i in range(NUM_BLOCKS):
            eng.context_norm(cflat[i], d0c[i:i + 1])

        NI = 2 * NUM_BLOCKS

        def run(deferred: bool, k0: int = 0, outs=None):
            """f, interpolation, g = integrations 0 .. 11.  deferred: no look at a controller until all twelve are enqueued.
            k0 > 0: integrations < k0 are taken from `outs` (a blind run that got that far) and the rest is integrated."""
            outs = list(outs) if outs is not None else [None] * NI
            for i in range(NUM_BLOCKS):
                if i < k0:
                    continue
                p_in = xyz.reshape(T, 3) if i == 0 else outs[i - 1]        # [T,4]: a block reads the previous state's first three columns in place
                outs[i] = eng.integrate(i, p_in, ctx[i], es[i], 1, False, cflat[i].numel(), d0c[i:i + 1],
                                        eng.logs[i] if deferred else None, blind[i] if deferred else 0)
                took[i] = getattr(eng, "last_attempts", 0)
            # the six blocks' delta logp, summed per patch in one reduction (it was a reduce + an add per block)
            ldj = torch.stack([s_[:, 3] for s_ in outs[:NUM_BLOCKS]]).view(NUM_BLOCKS, B, N).sum(dim=(0, 2))
            z = outs[NUM_BLOCKS - 1][:, :3].reshape(B, N, 3)
            logp = -torch.mean(torch.sum(-0.5 * (z ** 2 + math.log(2 * math.pi)), dim=(1, 2)) - ldj)
            u0 = None
            for j, i in enumerate(reversed(range(NUM_BLOCKS))):
                k = NUM_BLOCKS + j
                if k < k0:
                    continue
                if j == 0:
                    u0 = base.interp(xyz, z.contiguous(), idx16, upratio).reshape(T * upratio, 3)        # row n*R + r
                outs[k] = eng.integrate(i, u0 if j == 0 else outs[k - 1], ctx[i], es[i], upratio, True, cflat[i].numel() * upratio,
                                        d0c[i:i + 1], eng.logs[k] if deferred else None, blind[k] if deferred else 0,
                                        extra_scale=float(upratio))
                took[k] = getattr(eng, "last_attempts", 0)
            return z, ldj, logp, outs[NI - 1][:, :3].contiguous(), outs

        # The host used to read the controller after every batch of attempts (~2 reads x 12 integrations, each a pipeline
        # bubble).  Now the whole forward is enqueued blind and the twelve final controller states are read ONCE.  An integration
        # that did not finish inside its attempts (or hit an error state) ends the blind part THERE: everything before it stands,
        # it and the integrations behind it go through the look-per-batch loop (which also raises the errors).  Same arithmetic
        # either way: attempts past the end of an integration are no-ops.
        # How many attempts to enqueue blind: what each integration took before + an eighth + 2; the counts decay by at most one
        # per forward, so an input stream whose counts flutter does not miss every other time (the first forward of an engine
        # takes the loop and leaves the counts).
        took: List[int] = [0] * NI
        k0, outs = 0, None
        ran_blind, enq = False, 0
        if eng.async_attempts > 0 and eng.hint is not None:
            blind = [h + h // 8 + 2 for h in eng.hint]
            ran_blind, enq = True, sum(blind)
            z, ldj, logp, u, outs = run(True)
            k0 = eng.check_logs(NI, took)
        if k0 < NI:
            blind = []
            z, ldj, logp, u, outs = run(False, k0, outs)
        old = eng.hint if eng.hint is not None else took
        eng.hint = [max(t, h - 1) for t, h in zip(took, old)]
        x = u.view(B, N * upratio, 3)
        # blind: was the forward enqueued without a look at a controller, how many step attempts were enqueued that way against the
        # attempts the twelve integrations took, and - when an integration did not finish inside its budget - from which
        # integration on the look-per-batch loop re-integrated (None: the blind forward stands)
        self.last_stats = dict(nfe=eng.nfe, accepted=eng.accepted, rejected=eng.rejected,
                               blind=dict(ran=ran_blind, attempts_enqueued=enq, attempts_taken=sum(took),
                                          fallback_from=(k0 if (ran_blind and k0 < NI) else None)))
        self.last_took = list(took)
        if stages:
            return dict(idx16=idx16, cs=cs, z=z, ldj=ldj, logp=logp, x=x, **self.last_stats)
        return x, logp

    def flow_block(self, i: int, x: Tensor, c: Tensor, e: Tensor, R: int = 1, reverse: bool = False, sweep: str = "fused",
                   controller: str = "device", pack: str = "device", attempts: Optional[int] = None, cap: Optional[int] = None,
                   schedule=None):
        """One CNF flow block, differentiable: x [rows,3] (rows = T R, the R rows of a point adjacent), c [T,cd] context,
        e [T,3] Hutchinson vector -> (x' [rows,3], delta logp [rows]).  An autograd function over x, c and the parameters of
        `self.flow_blocks[i]` (e gets no gradient), whatever `self.training` says; the weight record is packed from the live
        parameters on every call, so an optimizer step needs no `invalidate_plan`.
        Forward: adaptive Dormand-Prince steps, one attempt per launch, the last step cut to end at the end time.  Backward: the
        recorded steps in reverse, differentiating exactly what the forward computed with the step sizes as constants.
        controller = "device": the step-size control runs on the device and records the tape there (pf_cnf_steps_taped, one host
        read per batch of attempts; `self.tape_capacity` remembers how long a tape to allocate); "host": one host read per
        attempt (pf_cnf_step); "deferred" (DESIGN 9b): NO host read - `attempts` attempts are enqueued on a tape of `cap` steps
        (default: `self.tape_budget[(i, reverse)]`), the weights' pack status stays on the device too, the same tensors come back
        when the integration ends inside that budget and NaN when it does not; `self.check_train_logs()` reads what happened
        and `self.last_block_tape` holds the tape (the step list is on the device); "schedule" (DESIGN 9c): no controller at all -
        `schedule` is this integration's grid of fractions from 0.0 to 1.0, the (s, h) list is made on the device from the packed
        end time and ONE pf_cnf_replay launch writes the tape (`last_block_tape`: `steps_dev` [n, 2], `states` [n + 1, rows, 4]);
        no host read in the forward either.  sweep = "fused": the whole tape in one launch (pf_cnf_tape_vjp); "per_eval": pf_cnf_rhs_vjp per
        evaluation with pf_cnf_rhs / pf_lincomb between them.  "host" and "per_eval" are the in-library A/B references.
        pack = "device": the weight record is made from the live parameters on the device (pf_cnf_pack_blocks, one launch and one
        read of its meta row); "host", its A/B reference: the numpy packers on a host copy of the parameters.  The same bits.
        `sqrt_end_time` gets the CONTINUOUS formula dL/dT = sum(ybar(T) . k(T)) (reversed: -sum(xbar_in . k(T))
        at the start) x 2 sqrt_end_time - NOT the derivative of the discrete scheme, whose step sizes do not depend on T here.
        Under controller="schedule" the step sizes DO scale with T (h_k = T (g_{k+1} - g_k)); that dependence is ignored, as the
        adaptive controller's dependence on T is: the continuous formula stays.
        `self.last_block_steps`: the (s, h) of the accepted steps in solver time (s = -t when reversed)."""
        if not (x.is_cuda and c.is_cuda and e.is_cuda):
            raise _lib.PuflowHipError("inputs must be GPU tensors (no CPU fallback)")
        if x.dim() != 2 or x.shape[1] != 3 or c.dim() != 2 or e.shape != (c.shape[0], 3) or x.shape[0] != c.shape[0] * R:
            raise ValueError("flow_block: x [T R,3], c [T,cd], e [T,3]")
        if not 1 <= R <= 16:
            raise ValueError("flow_block: 1 <= R <= 16 (pf_cnf_rhs_vjp keeps a point's R rows inside one 16-row MFMA tile)")
        if sweep not in ("fused", "per_eval") or controller not in ("device", "host", "deferred", "schedule") or pack not in ("device", "host"):
            raise ValueError('flow_block: sweep is "fused" or "per_eval", controller "device", "host", "deferred" or "schedule", '
                             'pack "device" or "host"')
        if (schedule is not None) != (controller == "schedule"):
            raise ValueError('flow_block: `schedule` (a grid of fractions from 0.0 to 1.0) goes with controller="schedule"')
        pfx = f"flow_blocks.{i}."
        named = list(self.flow_blocks[i].named_parameters())
        keys = tuple(pfx + n for n, _ in named)
        steps: list = []
        opts = dict(sweep=sweep, controller=controller, pack=pack, cap=self.tape_capacity.get((int(i), bool(reverse)), 32))
        if controller == "schedule":
            if sweep != "fused" or pack != "device":
                raise ValueError('flow_block: controller="schedule" goes with sweep="fused" and pack="device"')
            key = (int(i), bool(reverse))
            full = {k: (0.0, 1.0) for k in schedule_keys(self.num_blocks)}     # (validated as one grid of a whole schedule)
            full[key] = schedule
            grid = validate_schedule(full, self.num_blocks)[key]
            logs, sticky = self._train_tables(x.device)
            opts.update(grid=grid, logs=logs, sticky=sticky)
        if controller == "deferred":
            if sweep != "fused" or pack != "device":
                raise ValueError('flow_block: controller="deferred" goes with sweep="fused" and pack="device"')
            known = self.tape_budget.get((int(i), bool(reverse)), (None, None))
            attempts, cap = attempts if attempts is not None else known[0], cap if cap is not None else known[1]
            if attempts is None or cap is None or int(attempts) < 1 or int(cap) < 1:
                raise ValueError('flow_block: controller="deferred" needs attempts >= 1 and cap >= 1 (or a learnt tape_budget entry)')
            self.tape_budget[(int(i), bool(reverse))] = (int(attempts), int(cap))
            logs, sticky = self._train_tables(x.device)
            opts.update(attempts=int(attempts), cap=int(cap), logs=logs, sticky=sticky)
        out = _FlowBlockFn.apply(x, c, e, int(i), int(R), bool(reverse), keys, steps, opts, *[p for _, p in named])
        if controller == "device":
            self.tape_capacity[(int(i), bool(reverse))] = len(steps) + len(steps) // 8 + 2
        self.last_block_steps = steps
        self.last_block_tape = opts.get("tape")
        return out

    def sample(self, sparse: Tensor, upratio: int = 4) -> Tensor:
        dense, _ = self(sparse, upratio)
        return dense
