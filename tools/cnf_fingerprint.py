#!/usr/bin/env python3
"""GPU box: what the continuous (CNF) model computes, as SHA-256 of the bytes - every kernel of csrc/cnf.hip and csrc/cnf_bwd.hip
is launched at a shape with a partial tile.  Weights: synth_cnf_state_dict(2021) with the bench workload's dynamics and end times;
inputs, Hutchinson vectors and cotangents from fixed seeds.
  (a) the inference forward (stages=True) at 2 x 200 points = 400 rows = 6 1/4 tiles: x, logp, ldj, z, the solver's counters and
      which blocks take the factored gates.  upratio 4 (the inverse pass keeps the context rows in LDS) and 3 (64 % 3 != 0: it
      does not), each with PF_CNF_SPLIT=1 and =0: all four cnf_step_dev_kernel instantiations and both cnf_init_kernel.
  (b) flow_block, forward and backward of x'.sum() + dlogp.sum(): outputs, the accepted steps, the gradient of every parameter of
      the block, of x and of c.  (block 0, 200 points, R = 1, forward) and (block 3, 67 points, R = 3, reversed: 15 of a wave
      tile's 16 columns used, last tile partial): cnf_step_kernel, cnf_rhs_kernel, lincomb_kernel, the sumsq kernels,
      cnf_rhs_vjp_kernel and its reduction.
  (c) the eval forward on a frozen schedule (uniform, three steps; 2 x 200, upratio 4): x, logp, ldj, z and the error ratios.
  (d) record_schedule at upratio 3: the grids, its own x and logp, then x and logp of the forward that replays them.
  (e) flow_block on block 3 as in (b) under every controller: host (with sweep "per_eval" and pack "host", the A/B references),
      device (pack "host"), deferred (64 attempts, tape of 64; check_train_logs) and a four-step schedule.
  (f) the train-mode forward and backward of 0.5 logp + (x gx).sum() at (B, N, R) = (3, 50, 2), `deterministic` on, a fresh net
      per leg: eager, deferred (two steps: the first learns the budgets, the second reads nothing) and on a uniform schedule -
      x, logp, the twelve step lists, every parameter gradient, check_train_logs and last_skipped_steps.
In (e) and (f) the parameter gradients are hashed per group (`flow_blocks.3.*`, `feat_convs.0.*`, ...: one SHA-256 over every
tensor of the group); --each adds a line per tensor.
Public surface only, so the same file runs against two trees: `cnf_fingerprint.py [--each] [DIR]`, DIR = the directory that
holds the other tree's `puflow_amd` (default: this repository).  Identical text = same bits."""
import hashlib
import os
import sys

EACH = "--each" in sys.argv
ARGS = [a for a in sys.argv[1:] if a != "--each"]
sys.path.insert(0, os.path.abspath(ARGS[0]) if ARGS else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from puflow_amd.cnf import PointInterpFlow, schedule_keys, uniform_schedule
from puflow_amd.weights import CNF_PU1K_DYNAMICS, CNF_PU1K_END_TIMES, synth_cnf_state_dict, synth_patches

dev = "cuda:0"
B, N = 2, 200


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


sd = synth_cnf_state_dict(2021, dynamics=CNF_PU1K_DYNAMICS, end_times=CNF_PU1K_END_TIMES)
net = PointInterpFlow(3)
net.load_state_dict(sd, strict=True)
net = net.to(dev).eval()

xyz = synth_patches(B, N, seed=2021).to(dev)
g = torch.Generator().manual_seed(7)
noise = [torch.randn(B, N, 3, generator=g).to(dev) for _ in range(net.num_blocks)]
for upratio in (4, 3):
    for split in ("1", "0"):
        os.environ["PF_CNF_SPLIT"] = split
        net.invalidate_plan()                                  # the engine reads the switch when it is built
        out = net(xyz, upratio, noise=noise, stages=True)
        torch.cuda.synchronize()
        print(f"forward upratio {upratio} PF_CNF_SPLIT {split} split {net._engine(upratio).split} nfe {out['nfe']} "
              f"accepted {out['accepted']} rejected {out['rejected']}")
        for k in ("x", "logp", "ldj", "z"):
            print(f"  {k:5s} {tuple(out[k].shape)} sha256 {sha(out[k])}")
os.environ.pop("PF_CNF_SPLIT")

for block, T, R, reverse in ((0, 200, 1, False), (3, 67, 3, True)):
    cd = sd[f"flow_blocks.{block}.cnf.odefunc.diffeq.layers.0._hyper_gate.weight"].shape[1] - 1
    g = torch.Generator().manual_seed(100 + block)
    x = (torch.randn(T * R, 3, generator=g) * 0.8).to(dev).requires_grad_(True)
    c = (torch.randn(T, cd, generator=g) * 0.7).to(dev).requires_grad_(True)
    e = torch.randn(T, 3, generator=g).to(dev)
    net.zero_grad(set_to_none=True)
    ox, ol = net.flow_block(block, x, c, e, R, reverse)
    (ox.sum() + ol.sum()).backward()
    torch.cuda.synchronize()
    steps = torch.tensor(net.last_block_steps, dtype=torch.float64)
    print(f"flow_block {block} points {T} R {R} reversed {reverse} accepted steps {len(net.last_block_steps)}")
    print(f"  x'    sha256 {sha(ox)}\n  dlogp sha256 {sha(ol)}\n  steps sha256 {sha(steps)}")
    print(f"  dx    sha256 {sha(x.grad)}\n  dc    sha256 {sha(c.grad)}")
    for name, p in net.flow_blocks[block].named_parameters():
        print(f"  d {name} sha256 {sha(p.grad)}")


def fresh(train=False):
    n = PointInterpFlow(3)
    n.load_state_dict(sd, strict=True)
    n = n.to(dev)
    return n.train() if train else n.eval()


def print_grads(named):
    """One line per group of parameters (the name up to its index): SHA-256 over every gradient of the group, names included.
    With --each also one line per tensor, to find which one differs."""
    groups = {}
    for name, p in named:
        h = groups.setdefault(".".join(name.split(".")[:2]), hashlib.sha256())
        h.update(name.encode() + (b"none" if p.grad is None else p.grad.detach().cpu().contiguous().numpy().tobytes()))
        if EACH:
            print(f"    d {name} sha256 {sha(p.grad) if p.grad is not None else None}")
    for key, h in groups.items():
        print(f"  d {key}.* sha256 {h.hexdigest()}")


def sha_steps(lists):
    return sha(torch.tensor([v for steps in lists for sh in steps for v in sh] + [float(len(steps)) for steps in lists],
                            dtype=torch.float64))


# (c) the eval forward on a frozen schedule: pf_cnf_replay with the error sums
net = fresh()
net.step_schedule = uniform_schedule(3)
out = net(xyz, 4, noise=noise, stages=True)
torch.cuda.synchronize()
print(f"scheduled forward uniform 3 nfe {out['nfe']} accepted {out['accepted']} rejected {out['rejected']}")
for k in ("x", "logp", "ldj", "z"):
    print(f"  {k:5s} {tuple(out[k].shape)} sha256 {sha(out[k])}")
ratios = net.schedule_error_ratios()
print(f"  ratios sha256 {sha(torch.tensor([v for key in schedule_keys() for v in ratios[key]], dtype=torch.float64))}")

# (d) record_schedule (the taped device controller on the eval plan), then the forward on what it recorded
net = fresh()
sched = net.record_schedule(xyz, 3, noise=noise)
torch.cuda.synchronize()
rec = net.last_record
print(f"record_schedule upratio 3 steps {[len(sched[key]) - 1 for key in schedule_keys()]} accepted {rec['accepted']} "
      f"rejected {rec['rejected']}")
print(f"  grids sha256 {sha(torch.tensor([v for key in schedule_keys() for v in sched[key]], dtype=torch.float64))}")
print(f"  x     sha256 {sha(rec['x'])}\n  logp  sha256 {sha(rec['logp'])}")
net.step_schedule = sched
ox, ol = net(xyz, 3, noise=noise)
torch.cuda.synchronize()
print(f"  replayed x sha256 {sha(ox)}\n  replayed logp sha256 {sha(ol)}")

# (e) flow_block on block 3 (67 points, R = 3, reversed) under every controller, and the A/B references of sweep and pack
block, T, R, reverse = 3, 67, 3, True
cd = sd[f"flow_blocks.{block}.cnf.odefunc.diffeq.layers.0._hyper_gate.weight"].shape[1] - 1
for label, kw in (("host per_eval pack host", dict(controller="host", sweep="per_eval", pack="host")),
                  ("device pack host", dict(controller="device", pack="host")),
                  ("deferred 64 64", dict(controller="deferred", attempts=64, cap=64)),
                  ("schedule uniform 4", dict(controller="schedule", schedule=[0.0, 0.25, 0.5, 0.75, 1.0]))):
    net = fresh()
    g = torch.Generator().manual_seed(100 + block)
    x = (torch.randn(T * R, 3, generator=g) * 0.8).to(dev).requires_grad_(True)
    c = (torch.randn(T, cd, generator=g) * 0.7).to(dev).requires_grad_(True)
    e = torch.randn(T, 3, generator=g).to(dev)
    ox, ol = net.flow_block(block, x, c, e, R, reverse, **kw)
    (ox.sum() + ol.sum()).backward()
    torch.cuda.synchronize()
    line = f"flow_block {block} points {T} R {R} reversed {reverse} {label} accepted steps {len(net.last_block_steps)}"
    if kw["controller"] == "deferred":
        line += f" check_train_logs {net.check_train_logs()}"
    steps = torch.tensor(net.last_block_steps, dtype=torch.float64)
    tape = net.last_block_tape
    if tape is not None:                                       # the step list stayed on the device: its valid prefix
        steps = tape["steps_dev"][:int(tape["log"].cpu()[6]) if "log" in tape else None]
        line += f" tape steps {steps.shape[0]}"
    print(line)
    print(f"  x'    sha256 {sha(ox)}\n  dlogp sha256 {sha(ol)}\n  steps sha256 {sha(steps)}")
    print(f"  dx    sha256 {sha(x.grad)}\n  dc    sha256 {sha(c.grad)}")
    print_grads((f"flow_blocks.{block}.{name}", p) for name, p in net.flow_blocks[block].named_parameters())

# (f) the train-mode forward and backward at the tests' small shape: 150 f rows (a partial tile), 300 g rows
Bt, Nt, Rt = 3, 50, 2
xt = synth_patches(Bt, Nt, seed=61).to(dev)
g = torch.Generator().manual_seed(9)
nt = [torch.randn(Bt, Nt, 3, generator=g).to(dev) for _ in range(6)]
gxt = torch.randn(Bt, Nt * Rt, 3, generator=g).to(dev)
for label, steps_run in (("eager", 1), ("deferred", 2), ("scheduled", 1)):
    net = fresh(train=True)
    net.deterministic = True
    if label == "deferred":
        net.train_deferred = True
    if label == "scheduled":
        net.step_schedule = uniform_schedule(3)
    for it in range(steps_run):                                # deferred: the first step learns the budgets, the second reads nothing
        net.zero_grad(set_to_none=True)
        ox, ol = net(xt, Rt, noise=nt)
        (0.5 * ol + (ox * gxt).sum()).backward()
        torch.cuda.synchronize()
        line = f"train {Bt} x {Nt} x {Rt} {label} step {it}"
        if label != "eager":
            line += f" check_train_logs {net.check_train_logs()} skipped {net.last_skipped_steps}"
        lists = net.last_train_steps
        print(f"{line} steps {[len(s) for s in lists]}")
        print(f"  x     sha256 {sha(ox)}\n  logp  sha256 {sha(ol)}\n  steps sha256 {sha_steps(lists)}")
        print_grads(net.named_parameters())
    if label == "deferred":
        print(f"  budgets {sorted(net.tape_budget.items())}")
