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

Where it lives, by layer (each module imports only from those above it):
  * cnf_schedule.py - the order of the twelve integrations (`schedule_keys`, `_log_row`, `_row_key`, `PACK_ROW`), the frozen step
    schedules and their device constants (`_ScheduleDev`).  torch only: it loads without the library;
  * cnf_engine.py   - solver constants, `_DevicePack`, the launch wrappers with the look-per-batch loop (`_CnfKernels`), the
    inference plan `_CnfEngine`, the taped engine of one block `_BlockTapeEngine` and its backward;
  * cnf_train.py    - the controllers of a training forward as plans (eager, deferred, scheduled), the autograd nodes,
    `flow_train`, `forward_train`, the digest of the deferred controller's tables;
  * cnf.py (here)   - the parameter holders and `PointInterpFlow`: the eval forward on either controller, `record_schedule`,
    `flow_block`, `check_train_logs`.  Everything the rest of the tree imports from the other three is re-exported below.
"""
from __future__ import annotations

import math
from typing import List, Optional

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib
from .cnf_engine import ATOL, RTOL, _BlockTapeEngine, _CnfEngine, _DevicePack, _margin, _gauss_logp, _pack_keys  # noqa: F401
from .cnf_schedule import (PACK_ROW, _log_row, _row_key, _ScheduleDev, load_schedule, refine_schedule, save_schedule,  # noqa: F401
                           schedule_from_steps, schedule_keys, schedule_step_lists, uniform_schedule, validate_schedule)
from .cnf_train import _FlowBlockFn, digest_train_tables, flow_train, forward_train  # noqa: F401
from .interpflow import COND_CHANNELS, FEAT_CHANNELS, GROWTH, NUM_BLOCKS, _EdgeConvParams, _InterpParams, _MergeParams



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
        self.last_took: Optional[List[int]] = None    # step attempts of the twelve integrations of the last adaptive eval forward
        # flow_block's device-side tape: steps to allocate it for, per (block, reverse) - what the last call took + an eighth + 2
        self.tape_capacity: dict = {}
        self.last_block_steps: Optional[list] = None  # flow_block: the accepted steps' (s, h) as host floats
        self.last_block_tape: Optional[dict] = None   # flow_block under controller "deferred" / "schedule": the tape
        # ---- the deferred controller of the train-mode forward, off by default
        self.train_deferred = False               # no look at a controller inside the forward: `check_train_logs` reads them all, later
        self.tape_budget: dict = {}               # (block, reverse) -> (attempts to enqueue, tape capacity); learnt from a host-read run
        self.train_noise: Optional[List[Tensor]] = None       # fixed Hutchinson vectors for every training forward (default: drawn)
        self._train_tab: Optional[Tensor] = None  # the twelve log rows and the sticky table, one buffer = one read
        self._sticky_seen = None                  # the sticky table at the last `check_train_logs`
        self._last_steps = None                   # `last_train_steps` on the host, once fetched ...
        self._step_fetch = None                   # ... by these twelve calls, left by the last train-mode forward
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
            self._engine_cache.drop_schedule()

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
        eng, idx16, _, es, cflat, ctx, d0c = self._eval_prologue(xyz, upratio, noise)
        lists, took = [], []

        def step(k, i, reverse, R, p_in):
            y, tape = eng.tape_forward(i, p_in, cflat[i], es[i], R, reverse, ctx=ctx[i], d0c=d0c[i:i + 1])
            lists.append(tape["steps"]); took.append(tape["took"])
            return y

        _, _, logp, x, _ = self._walk(eng, xyz, upratio, idx16, step)
        accepted = sum(len(s) for s in lists)
        self.last_record = dict(x=x, logp=logp, steps=lists, accepted=accepted, rejected=sum(took) - accepted)
        if self.training:
            self.invalidate_plan()
        return refine_schedule(schedule_from_steps(lists, [eng.T_end[i] for i in range(NUM_BLOCKS)]), refine)

    def _eval_prologue(self, xyz: Tensor, upratio: int, noise: Optional[List[Tensor]], norms: bool = True):
        """What every eval-plan path runs before its integrations: kNN, the conditioning features, the Hutchinson vectors (drawn
        here when not given), the context rows of every block and - norms - the context's share of the solver's initial-step
        norm.  The context is a state of the reference's ODE (zero derivative): it only enters the solver's norms, six device
        words.  A replay takes none.  -> (engine, idx16, cs, es, cflat, ctx, d0c | None)"""
        B, N, _ = xyz.shape
        T = B * N
        eng = self._engine(upratio)
        idx16 = eng.base.knn(xyz)
        cs, _, _ = eng.base.features(xyz, idx16, want_cs=True, cs_only=True)
        if noise is None:
            noise = [torch.randn(B, N, 3, device=xyz.device) for _ in range(NUM_BLOCKS)]
        es = [n.reshape(T, 3).contiguous().float() for n in noise]
        cflat = [c.reshape(T, -1).contiguous() for c in cs]
        ctx = [eng.context(i, cflat[i]) for i in range(NUM_BLOCKS)]
        d0c = None
        if norms:
            d0c = torch.empty(NUM_BLOCKS, dtype=torch.float64, device=xyz.device)
            for i in range(NUM_BLOCKS):
                eng.context_norm(cflat[i], d0c[i:i + 1])
        return eng, idx16, cs, es, cflat, ctx, d0c

    @staticmethod
    def _walk(eng: _CnfEngine, xyz: Tensor, upratio: int, idx16: Tensor, step, k0: int = 0, outs=None):
        """f, the log-likelihood of the latent, its interpolation, g: the twelve integrations in running order, each run by
        step(k, i, reverse, R, p_in [rows, >= 3]) -> state [rows,4] (a block reads the previous state's first three columns in
        place).  k0 > 0: integrations < k0 are taken from `outs` and the rest is integrated.
        -> (z [B,N,3], ldj [B], logp, x [B, N upratio, 3], the twelve states)"""
        B, N, _ = xyz.shape
        T = B * N
        outs = list(outs) if outs is not None else [None] * (2 * NUM_BLOCKS)
        p = xyz.reshape(T, 3)
        for k, (i, reverse) in enumerate(schedule_keys()):
            if k == NUM_BLOCKS:
                # the six blocks' delta logp, summed per patch in one reduction (it was a reduce + an add per block)
                ldj = torch.stack([s_[:, 3] for s_ in outs[:NUM_BLOCKS]]).view(NUM_BLOCKS, B, N).sum(dim=(0, 2))
                z = p[:, :3].reshape(B, N, 3)
                logp = _gauss_logp(z, ldj)
                if k >= k0:
                    p = eng.base.interp(xyz, z.contiguous(), idx16, upratio).reshape(T * upratio, 3)        # row n*R + r
            if k >= k0:
                outs[k] = step(k, i, reverse, upratio if reverse else 1, p)
            p = outs[k]
        return z, ldj, logp, p[:, :3].contiguous().view(B, N * upratio, 3), outs

    def _forward_eval_schedule(self, xyz: Tensor, upratio: int, noise: Optional[List[Tensor]], stages: bool):
        """The eval forward on `step_schedule`: twelve pf_cnf_replay launches, no controllers, no hints, no host read."""
        sdev = self._schedule_dev(xyz.device)
        steps = self._engine(upratio).schedule_lists(sdev)
        eng, idx16, cs, es, cflat, ctx, _ = self._eval_prologue(xyz, upratio, noise, norms=False)
        eng.nfe = eng.accepted = eng.rejected = 0
        errsq = torch.zeros((2 * NUM_BLOCKS, steps.shape[1]), dtype=torch.float64, device=xyz.device)
        n_tot = []

        def step(k, i, reverse, R, p_in):
            n = sdev.n[k]
            y, _ = eng.replay(i, p_in, steps[k, :n], reverse, ctx[i], es[i], R, errsq=errsq[k, :n])
            n_tot.append(float(y.shape[0] * 4 + cflat[i].numel() * R))
            return y

        z, ldj, logp, x, _ = self._walk(eng, xyz, upratio, idx16, step)
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
        `last_skipped_steps`: forwards since the last call with at least one integration that was not clean.
        The reading is here, what it means in `cnf_train.digest_train_tables`."""
        if self._train_tab is None:
            return 0
        host = self._train_tab.cpu()                             # the one read
        nl = 2 * NUM_BLOCKS * 16 * 2
        sticky = host[nl:].view(2 * NUM_BLOCKS + 1, 4)
        seen, self._sticky_seen = self._sticky_seen, sticky.clone()
        short, self.last_skipped_steps = digest_train_tables(host[:nl].view(torch.float64).view(2 * NUM_BLOCKS, 16), sticky, seen,
                                                             self.tape_budget)
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
        if self._last_steps is None and self._step_fetch is not None:
            self._last_steps, self._step_fetch = [fetch() for fetch in self._step_fetch], None
        return self._last_steps

    @last_train_steps.setter
    def last_train_steps(self, steps) -> None:
        self._last_steps, self._step_fetch = steps, None

    def _set_train_tapes(self, fetch: list) -> None:
        """`flow_train` leaves what its plan handed out per integration: a call that gives the (s, h) list on the host."""
        self._last_steps, self._step_fetch = None, fetch

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
        eng, idx16, cs, es, cflat, ctx, d0c = self._eval_prologue(xyz, upratio, noise)
        eng.nfe = eng.accepted = eng.rejected = 0
        NI = 2 * NUM_BLOCKS

        def run(deferred: bool, k0: int = 0, outs=None):
            """Integrations k0 .. 11 (`_walk`).  deferred: no look at a controller until all twelve are enqueued; otherwise the
            look-per-batch loop, after a blind run that got as far as k0."""
            def step(k, i, reverse, R, p_in):
                out = eng.integrate(i, p_in, ctx[i], es[i], R, reverse, cflat[i].numel() * R, d0c[i:i + 1],
                                    eng.logs[k] if deferred else None, blind[k] if deferred else 0, extra_scale=float(R))
                took[k] = eng.last_attempts
                return out
            return self._walk(eng, xyz, upratio, idx16, step, k0, outs)

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
            blind = [_margin(h) for h in eng.hint]
            ran_blind, enq = True, sum(blind)
            z, ldj, logp, x, outs = run(True)
            k0 = eng.check_logs(NI, took)
        if k0 < NI:
            blind = []
            z, ldj, logp, x, outs = run(False, k0, outs)
        old = eng.hint if eng.hint is not None else took
        eng.hint = [max(t, h - 1) for t, h in zip(took, old)]
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
            self.tape_capacity[(int(i), bool(reverse))] = _margin(len(steps))
        self.last_block_steps = steps
        self.last_block_tape = opts.get("tape")
        return out

    def sample(self, sparse: Tensor, upratio: int = 4) -> Tensor:
        dense, _ = self(sparse, upratio)
        return dense
