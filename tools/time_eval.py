"""Time the evaluation metrics on the GPU (csrc/eval_metrics.hip through puflow_amd.metrics, and the CLI):
  approx-match EMD at 2048 / 8192 / 20000 points, B = 1 and 16 (ms per launch sequence and per cloud pair);
  point-to-mesh distance of 8192 points to 1e4 / 1e5 / 1e6 faces (pruned and, up to 1e5 faces, brute force);
  the CLI's wall time over a synthetic PU1K-shaped directory (127 files of 8192 predicted / ground-truth points, meshes).

  python tools/time_eval.py [--quick] [--out profiles/eval/time_eval.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_ref as R  # noqa: E402
from puflow_amd import metrics  # noqa: E402


def gpu_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return float(np.median(times)), float(np.min(times))


def mesh_with_faces(F):
    """A bumpy torus with about F faces."""
    nu = int(round((F / 2 / 0.5) ** 0.5))
    v, f = R.torus(nu, max(3, nu // 2), bump=0.15)
    return v.astype(np.float32), f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cli_files", type=int, default=127)
    a = ap.parse_args()
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "emd": [], "p2f": []}
    g = torch.Generator().manual_seed(0)
    for n in (2048, 8192, 20000):
        for B in (1, 16):
            if a.quick and n * B > 8192 * 16:
                continue
            x = torch.randn(B, n, 3, generator=g).to(dev)
            y = torch.randn(B, n, 3, generator=g).to(dev)
            x, _, _ = metrics.normalize_point_cloud(x)
            y, _, _ = metrics.normalize_point_cloud(y)
            med, mn = gpu_ms(lambda: metrics.approx_match_emd(x, y), 3 if n * B > 100000 else 5)
            row = {"n": n, "B": B, "ms_median": med, "ms_min": mn, "ms_per_pair": med / B}
            res["emd"].append(row)
            print("emd", row, flush=True)
    rng = np.random.default_rng(1)
    for F in (10_000, 100_000, 1_000_000):
        v, f = mesh_with_faces(F)
        p = R.sample_surface(v, f, 8192, rng) + rng.normal(0, 0.01, (8192, 3))
        pt, vt, ft = torch.from_numpy(p.astype(np.float32)).to(dev), torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
        med, mn = gpu_ms(lambda: metrics.point_to_mesh_distance(pt, vt, ft), 5)
        row = {"points": 8192, "faces": int(len(f)), "ms_median": med, "ms_min": mn}
        if len(f) <= 200_000:
            row["brute_ms_median"] = gpu_ms(lambda: metrics.point_to_mesh_distance(pt, vt, ft, brute=True), 3)[0]
        res["p2f"].append(row)
        print("p2f", row, flush=True)
    # the CLI over a PU1K-shaped directory: 127 files of 8192 points, a 10^4-face mesh each (file reading, batching, writing)
    from puflow_amd import evaluate
    nfiles = 8 if a.quick else a.cli_files
    with tempfile.TemporaryDirectory() as td:
        v, f = mesh_with_faces(10_000)
        for d in ("pred", "gt", "mesh"):
            os.makedirs(os.path.join(td, d))
        R.write_off(os.path.join(td, "mesh", "m.off"), v, f)
        for i in range(nfiles):
            name = f"shape{i:03d}"
            for d in ("pred", "gt"):
                q = R.sample_surface(v, f, 8192, rng) + rng.normal(0, 0.003, (8192, 3))
                np.savetxt(os.path.join(td, d, name + ".xyz"), q.astype(np.float32), fmt="%.6f")
            os.link(os.path.join(td, "mesh", "m.off"), os.path.join(td, "mesh", name + ".off"))
        for label, extra in (("cli_s", []), ("cli_p2f_s", ["--mesh", os.path.join(td, "mesh"), "--write_p2m"])):
            t = time.perf_counter()
            evaluate.main(["--pred", os.path.join(td, "pred"), "--gt", os.path.join(td, "gt"), "--save_path",
                           os.path.join(td, "out")] + extra)
            torch.cuda.synchronize()
            res[label] = time.perf_counter() - t
            print(label, res[label], flush=True)
        res["cli_files"] = nfiles
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
