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
Public surface only, so the same file runs against two trees: `cnf_fingerprint.py [DIR]`, DIR = the directory that holds the
other tree's `puflow_amd` (default: this repository).  Identical text = same bits."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from puflow_amd.cnf import PointInterpFlow
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
