#!/usr/bin/env python3
"""GPU box: the fingerprint of one default training step at batch 4 x (256 -> 1024) - what it launches and what it computes.
  (a) three warm-up steps (the first one initialises ActNorm on the per-block path)
  (b) one eager step under torch.profiler: every device activity's name with its count, sorted
  (c) three steps under cfg.deterministic from a fixed seed: SHA-256 of the loss and of every gradient's bytes, in parameter order
Run the same file against two trees of Python sources on ONE library (PF_LIB_PATH): `step_fingerprint.py [DIR]`, DIR = the
directory that holds the other tree's `puflow_amd` (default: this repository).  Identical text = same launches, same bits."""
import collections
import hashlib
import os
import sys

sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch.autograd import DeviceType
from torch.profiler import profile, ProfilerActivity
from puflow_amd.trainer import TrainerModule, default_cfg
from puflow_amd.weights import synth_patches, synth_state_dict

dev = "cuda:0"
dense = ((synth_patches(4, 1024, seed=2021) + 1) / 2).to(dev)
batch = (dense[:, ::4].contiguous(), dense, torch.ones(4, device=dev))


def module(**cfg):
    torch.manual_seed(0)
    tm = TrainerModule(default_cfg(learning_rate=1e-3, **cfg), loss_mix="pugan")
    tm.network.load_state_dict(synth_state_dict(2021))
    tm = tm.to(dev)
    return tm, tm.configure_optimizers()["optimizer"]


tm, opt = module()
for _ in range(3):
    tm.train_step(batch, opt)
torch.cuda.synchronize()
with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    tm.train_step(batch, opt)
    torch.cuda.synchronize()
counts = collections.Counter(e.name for e in prof.events() if e.device_type == DeviceType.CUDA)
print(f"launches {sum(counts.values())} distinct {len(counts)}")
for name, n in sorted(counts.items()):
    print(f"{n:5d}  {name}")

tm, opt = module(deterministic=True)
for step in range(3):
    loss = tm.train_step(batch, opt)
    torch.cuda.synchronize()
    h = hashlib.sha256(loss.cpu().numpy().tobytes())
    grads = 0
    for p in tm.parameters():
        if p.grad is not None:
            h.update(p.grad.detach().cpu().contiguous().numpy().tobytes())
            grads += 1
    print(f"step {step} loss {float(loss)!r} gradients {grads} sha256 {h.hexdigest()}")
