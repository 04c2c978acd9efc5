"""Wall time per training batch of `fit(graph=True)` by data path (GPU box):

  (a) PatchData            batches assembled and augmented on the host, three host-to-device copies per batch
  (b) DevicePatchData      one pf_patch_batch launch per batch into fresh tensors, copied into the captured step's inputs
  (c) DevicePatchData      bound: the launch writes the captured step's inputs directly

each with and without `use_random_input` (the non-uniform subsample of a 4x input), on synthetic patches, 32 x (256 -> 1024).
One warm-up epoch (capture, allocator, ActNorm init), then the steady state: wall time from the first batch request of an
epoch to the end of its last step (device synchronised), over >= 200 batches.  Also the launch-to-launch time of back-to-back
pf_patch_batch calls between two HIP events: an upper bound of the kernel's time (the host's launch rate when that is longer).

    python tools/time_data_pipeline.py [--batches 104] [--epochs 3] [--out profiles/data]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_data_pipeline.py --kernel_only     # the kernel's own duration
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


class Timed:
    """The data object with a stopwatch around every epoch; hide_bind: `fit` finds nothing to bind (case b)."""

    def __init__(self, inner, hide_bind=False):
        self._inner, self._hide, self.epochs = inner, hide_bind, []

    def __getattr__(self, name):
        if name == "bind" and self._hide:
            raise AttributeError(name)
        return getattr(self._inner, name)

    def __len__(self):
        return len(self._inner)

    def __iter__(self):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        yield from self._inner
        torch.cuda.synchronize()
        self.epochs.append((time.perf_counter() - t0) / len(self._inner))


def run_case(kind, random_input, a, dev):
    from puflow_amd.data import SyntheticDevicePatchData, SyntheticPatchData
    from puflow_amd.train import fit
    from puflow_amd.trainer import TrainerModule, default_cfg
    torch.manual_seed(a.seed)
    module = TrainerModule(default_cfg(seed=a.seed), loss_mix="pu1k").to(dev)
    cls = SyntheticPatchData if kind == "host" else SyntheticDevicePatchData
    data = Timed(cls(num_patches=8 * a.batch_size, up_ratio=4, batch_size=a.batch_size, num_point_patch=256, device=dev, seed=a.seed,
                     is_augment=True, jitter_sigma=0.01, jitter_max=0.03, use_random_input=random_input, num_batches=a.batches),
                 hide_bind=kind == "device")
    fit(module, data, None, a.epochs, log=None, graph=True)
    steady = data.epochs[1:]
    return {"ms_per_batch": 1e3 * sum(steady) / len(steady), "ms_per_batch_by_epoch": [1e3 * t for t in data.epochs],
            "batches_timed": len(steady) * a.batches}


def launch_to_launch_time(random_input, a, dev, launches=200):
    from puflow_amd.data import KEYS, SyntheticDevicePatchData
    d = SyntheticDevicePatchData(num_patches=8 * a.batch_size, up_ratio=4, batch_size=a.batch_size, num_point_patch=256, device=dev,
                                 seed=a.seed, is_augment=True, use_random_input=random_input, num_batches=launches + 20)
    d.bind({k: v.clone() for k, v in zip(KEYS, next(iter(d)).values())})
    it = iter(d)
    for _ in range(20):
        next(it)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        next(it)
    e1.record()
    torch.cuda.synchronize()
    assert d.status() == 0
    return 1e3 * e0.elapsed_time(e1) / launches         # back-to-back launches: the kernel or the launch rate, whichever is longer


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", type=int, default=104)
    p.add_argument("--epochs", type=int, default=3, help="the first is the warm-up")
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--seed", type=int, default=2021)
    p.add_argument("--out", default=os.path.join("profiles", "data"))
    p.add_argument("--kernel_only", action="store_true", help="only the back-to-back launches (to run under a kernel trace)")
    a = p.parse_args()
    from puflow_amd._host import limit_host_threads
    limit_host_threads()
    dev = "cuda:0"
    if a.kernel_only:
        for random_input in (False, True):
            print(f"launch to launch, random_input={random_input}: {launch_to_launch_time(random_input, a, dev):.1f} us", flush=True)
        return
    res = {"device": torch.cuda.get_device_name(0), "batch": [a.batch_size, 256, 1024], "batches_per_epoch": a.batches, "epochs": a.epochs,
           "cases": {}, "pf_patch_batch_launch_to_launch_us": {}}
    lines = [f"fit(graph=True), synthetic patches {a.batch_size} x (256 -> 1024), {a.epochs - 1} x {a.batches} steady-state batches, "
             f"{res['device']}", f"{'data path':<34}{'random_input':>14}{'ms / batch':>12}"]
    names = {"host": "(a) PatchData (host)", "device": "(b) DevicePatchData, unbound", "bound": "(c) DevicePatchData, bound"}
    for random_input in (False, True):
        for kind in ("host", "device", "bound"):
            r = run_case(kind, random_input, a, dev)
            res["cases"][f"{kind}{'_random_input' if random_input else ''}"] = r
            lines.append(f"{names[kind]:<34}{str(random_input):>14}{r['ms_per_batch']:>12.3f}")
            print(lines[-1], flush=True)
        us = launch_to_launch_time(random_input, a, dev)
        res["pf_patch_batch_launch_to_launch_us"]["random_input" if random_input else "plain"] = us
        lines.append(f"{'pf_patch_batch, launch to launch':<34}{str(random_input):>14}{us / 1e3:>12.4f}")
        print(lines[-1], flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "time_data_pipeline.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(a.out, "time_data_pipeline.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
