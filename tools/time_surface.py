"""Time the surface-connected neighbourhoods (csrc/surface_reach.hip through puflow_amd.metrics / sampling) against the
Euclidean balls on the same tree.

  python tools/time_surface.py --out profiles/surface/time_surface.json
    uniformity disks: per cloud of 8192 and 20000 points on a 10^4-face mesh, 1000 seeds (the setting of
    tools/time_uniformity.py): the stages of --uniform_disks surface (face adjacency, reach count / fill / relax, disks with
    the reach) beside the ball's disks, the whole sequence both ways and their ratio, and the relaxation's sweeps per seed;
    the reach count pass alone on a 10^6-face mesh;
    patches: make_patches (50 patches, the defaults) with metric = ball and surface.
  A warm-up, then the median, minimum and maximum of the repeats.
"""
from __future__ import annotations

import argparse
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


def run(a):
    import torch
    import eval_ref as R
    from puflow_amd import metrics, sampling
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
        _, face = metrics.point_to_mesh_distance(pt, vt, ft, return_face=True)
        mapped = metrics.mapped_points(pt, vt, ft, face=face)
        seeds, sface, _ = metrics.sample_mesh(vt, ft, SEEDS, 0)
        adj = metrics.face_adjacency(vt, ft)
        reach, info = metrics.surface_reach(seeds, sface, vt, ft, float(radii[-1]), adj, return_info=True)
        cb, _ = metrics.disks(mapped, seeds, radii)
        cs, _ = metrics.disks(mapped, seeds, radii, reach=reach, mapped_face=face)

        def whole(surface):
            _, fc = metrics.point_to_mesh_distance(pt, vt, ft, return_face=True)
            m = metrics.mapped_points(pt, vt, ft, face=fc)
            s, sf, _ = metrics.sample_mesh(vt, ft, SEEDS, 0)
            if surface:
                _, c = metrics.disks(m, s, radii, reach=metrics.surface_reach(s, sf, vt, ft, float(radii[-1])), mapped_face=fc)
            else:
                _, c = metrics.disks(m, s, radii)
            return metrics.uniformity(m, c, radii)

        sw = info["sweeps"].cpu().numpy()
        row = {"points": n, "faces": int(len(f)), "candidate_faces": int(reach[1].shape[0]),
               "members_ball": int(cb[:, -1].sum()), "members_surface": int(cs[:, -1].sum()),
               "sweeps_min_median_max": [int(sw.min()), float(np.median(sw)), int(sw.max())],
               "uniform_ball": whole(False).tolist(), "uniform_surface": whole(True).tolist(),
               "whole_ball": timed(lambda: whole(False), a.reps), "whole_surface": timed(lambda: whole(True), a.reps),
               "face_adjacency": timed(lambda: metrics.face_adjacency(vt, ft), a.reps),
               "reach": timed(lambda: metrics.surface_reach(seeds, sface, vt, ft, float(radii[-1]), adj), a.reps),
               "disks_ball": timed(lambda: metrics.disks(mapped, seeds, radii), a.reps),
               "disks_surface": timed(lambda: metrics.disks(mapped, seeds, radii, reach=reach, mapped_face=face), a.reps)}
        row["surface_over_ball"] = row["whole_surface"]["ms_median"] / row["whole_ball"]["ms_median"]
        res["clouds"].append(row)
        print(json.dumps(row), flush=True)

    # the count pass where it is largest: seeds x faces closest-point tests, no spatial index
    vb, fb = mesh_with_faces(1_000_000)
    vbt, fbt = torch.from_numpy(vb).to(dev), torch.from_numpy(fb).to(dev)
    rb, _ = metrics.mesh_area_radii(vb, fb)
    sb, sfb, _ = metrics.sample_mesh(vbt, fbt, SEEDS, 0)
    adjb = metrics.face_adjacency(vbt, fbt)
    res["faces_1e6"] = {"faces": int(len(fb)), "face_adjacency": timed(lambda: metrics.face_adjacency(vbt, fbt), 3),
                        "reach": timed(lambda: metrics.surface_reach(sb, sfb, vbt, fbt, float(rb[-1]), adjb), 3)}
    print(json.dumps(res["faces_1e6"]), flush=True)

    res["patches"] = {m: timed(lambda m=m: sampling.make_patches(vt, ft, 50, metric=m), 3) for m in ("ball", "surface")}
    res["patches"]["surface_over_ball"] = res["patches"]["surface"]["ms_median"] / res["patches"]["ball"]["ms_median"]
    print(json.dumps(res["patches"]), flush=True)
    return res


def text(res):
    fmt = lambda t: f"{t['ms_median']:10.3f} ({t['ms_min']:.3f} .. {t['ms_max']:.3f}) x{t['repeats']}"      # noqa: E731
    lines = [f"surface disks against balls, {res['seeds']} seeds, 5 radii; {res['device']}; ms: median (min .. max) of the repeats "
             "after a warm-up, host glue included"]
    for row in res["clouds"]:
        lines.append(f"{row['points']} points, {row['faces']} faces: {row['candidate_faces']} candidate faces, members of the largest "
                     f"disks {row['members_ball']} (ball) / {row['members_surface']} (surface), sweeps per seed min / median / max "
                     f"{row['sweeps_min_median_max']}")
        for k in ("whole_ball", "whole_surface", "face_adjacency", "reach", "disks_ball", "disks_surface"):
            lines.append(f"  {k:15s} {fmt(row[k])}")
        lines.append(f"  surface / ball, whole sequence: {row['surface_over_ball']:.2f}x")
    big = res["faces_1e6"]
    lines.append(f"{big['faces']} faces, {res['seeds']} seeds: face_adjacency {fmt(big['face_adjacency'])}; reach (count + fill + relax) {fmt(big['reach'])}")
    pt = res["patches"]
    lines.append(f"make_patches, 50 patches: ball {fmt(pt['ball'])}; surface {fmt(pt['surface'])}; surface / ball {pt['surface_over_ball']:.2f}x")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    res = run(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.splitext(a.out)[0] + ".txt", "w") as fh:
        fh.write(text(res))


if __name__ == "__main__":
    main()
