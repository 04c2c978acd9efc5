"""The continuous model's integration order and its frozen step schedules: pure Python and torch, no GPU and no
library - this module loads where libpuflow_hip.so was never built.  `cnf.py` holds the map of the four CNF modules.

A schedule is a dict: for each of the twelve integrations (block, reverse) a strictly increasing float64 grid of FRACTIONS of the
integration's interval, from 0.0 to 1.0.  Step k of integration (i, r) spans [t0 + T g_k, t0 + T g_{k+1}] in solver time
(T = the block's end time, t0 = 0 going forward and -T reversed).  A uniform grid is one special case; the usual source is the
adaptive solver's own accepted steps on a calibration input (`PointInterpFlow.record_schedule`)."""
from __future__ import annotations

import math

import torch
from torch import Tensor

from .packing import NUM_BLOCKS

MAX_NUM_STEPS = 100000                   # step attempts per integration; a bound, never reached by a sane model
SCHEDULE_FORMAT = "puflow-cnf-step-schedule"


def schedule_keys(num_blocks: int = NUM_BLOCKS):
    """The integrations in the order they run: f's blocks 0 .. n - 1, then g's n - 1 .. 0."""
    return [(i, False) for i in range(num_blocks)] + [(i, True) for i in reversed(range(num_blocks))]


# The model's twelve integrations: entry k is the k-th to run, and row k of the deferred controller's log and sticky tables
# (DESIGN 9b), of a schedule's step lists and of `last_train_steps`.
_KEYS = tuple(schedule_keys())
_ROWS = {key: k for k, key in enumerate(_KEYS)}
PACK_ROW = len(_KEYS)                    # the sticky table's row of pf_cnf_pack_status, behind the twelve integrations'


def _log_row(i: int, reverse: bool) -> int:
    return _ROWS[(int(i), bool(reverse))]


def _row_key(k: int):
    return _KEYS[k]


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

