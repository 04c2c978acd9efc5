"""Time the uniformity columns (csrc/eval_uniform.hip through puflow_amd.metrics) and the reference's analyze_uniform.

  GPU side:  python tools/time_uniformity.py --out profiles/eval/time_uniformity.json [--keep DIR]
    per cloud of 8192 and 20000 points on a 10^4-face mesh, 1000 seeds: the whole sequence (closest face + mapped points +
    seeds + disks + statistic with its host finish) and each stage alone - a warm-up, then the median, minimum and maximum of
    the repeats.  --keep DIR writes every cloud's three disk files there.
  CPU side:  python tools/time_uniformity.py --reference DIR --out profiles/eval/time_uniformity.json
    wall time of the reference's analyze_uniform (evaluation/evaluate.py:116-165, its file reads included; the text is taken
    from the reference checkout at run time, as tools/make_golden_uniform.py does) on the files of DIR; the figures are merged
    into the JSON and the .txt beside it is rewritten.  Needs the reference checkout and sklearn, not a GPU.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SIZES = (8192, 20000)
SEEDS = 1000


def spread(times):
    return {"ms_median": float(np.median(times)), "ms_min": float(np.min(times)), "ms_max": float(np.max(times)), "repeats": len(times)}


def gpu_side(a):
    import torch
    import eval_ref as R
    from puflow_amd import metrics
    from time_eval import mesh_with_faces

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
        return spread(out)

    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "seeds": SEEDS, "clouds": []}
    v, f = mesh_with_faces(10_000)
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    radii, _ = metrics.mesh_area_radii(v, f)
    rng = np.random.default_rng(1)
    for n in SIZES:
        p = (R.sample_surface(v, f, n, rng) + rng.normal(0, 0.003, (n, 3))).astype(np.float32)
        pt = torch.from_numpy(p).to(dev)
        dist, face = metrics.point_to_mesh_distance(pt, vt, ft, return_face=True)
        mapped = metrics.mapped_points(pt, vt, ft, face=face)
        seeds, _, _ = metrics.sample_mesh(vt, ft, SEEDS, 0)
        counts, csr = metrics.disks(mapped, seeds, radii)

        def whole():
            _, fc = metrics.point_to_mesh_distance(pt, vt, ft, return_face=True)
            m = metrics.mapped_points(pt, vt, ft, face=fc)
            s, _, _ = metrics.sample_mesh(vt, ft, SEEDS, 0)
            _, c = metrics.disks(m, s, radii)
            return metrics.uniformity(m, c, radii)

        row = {"points": n, "faces": int(len(f)), "members": int(csr[1].shape[0]), "uniform": whole().tolist(),
               "whole": timed(whole, a.reps),
               "closest_face": timed(lambda: metrics.point_to_mesh_distance(pt, vt, ft, return_face=True), a.reps),
               "mapped_points": timed(lambda: metrics.mapped_points(pt, vt, ft, face=face), a.reps),
               "seeds": timed(lambda: metrics.sample_mesh(vt, ft, SEEDS, 0), a.reps),
               "disks": timed(lambda: metrics.disks(mapped, seeds, radii), a.reps),
               "statistic": timed(lambda: metrics.disk_statistics(mapped, csr, radii), a.reps)}
        res["clouds"].append(row)
        print(json.dumps(row), flush=True)
        if a.keep:
            os.makedirs(a.keep, exist_ok=True)
            metrics.write_disk_files(os.path.join(a.keep, f"cloud{n}"), pt, dist, mapped, csr, radii)
    return res


def reference_side(a, res):
    from make_golden_uniform import reference_functions
    analyze_uniform = reference_functions()
    for row in res["clouds"]:
        prefix = os.path.join(a.reference, f"cloud{row['points']}")
        times, val = [], None
        for _ in range(a.ref_reps + 1):                            # the first run is the warm-up (imports, file cache)
            t = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                val = analyze_uniform(prefix + "_disk_idx.txt", prefix + "_radius.txt", prefix + "_point2mesh_distance.txt")[:, 0]
            times.append((time.perf_counter() - t) * 1e3)
        row["reference_cpu"] = spread(times[1:])
        row["reference_uniform"] = val.tolist()
        row["reference_over_gpu"] = row["reference_cpu"]["ms_median"] / row["whole"]["ms_median"]
        print(row["points"], row["reference_cpu"], row["reference_over_gpu"], flush=True)
    res["reference_cpus"] = os.cpu_count()
    return res


def text(res):
    lines = [f"uniformity, {res['seeds']} seeds, 5 radii; {res['device']}; ms: median (min .. max) of the repeats after a warm-up"]
    for row in res["clouds"]:
        lines.append(f"{row['points']} points, {row['faces']} faces, {row['members']} members of the largest disks")
        for k in ("whole", "closest_face", "mapped_points", "seeds", "disks", "statistic", "reference_cpu"):
            if k in row:
                t = row[k]
                lines.append(f"  {k:14s} {t['ms_median']:10.3f} ({t['ms_min']:.3f} .. {t['ms_max']:.3f}) x{t['repeats']}")
        if "reference_over_gpu" in row:
            lines.append(f"  reference / GPU {row['reference_over_gpu']:.0f}x; largest relative difference of the five values "
                         f"{np.abs(np.array(row['uniform']) / np.array(row['reference_uniform']) - 1).max():.1e}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--keep", default=None)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ref_reps", type=int, default=3)
    a = ap.parse_args()
    if a.reference:
        with open(a.out) as fh:
            res = reference_side(a, json.load(fh))
    else:
        res = gpu_side(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.splitext(a.out)[0] + ".txt", "w") as fh:
        fh.write(text(res))


if __name__ == "__main__":
    main()
