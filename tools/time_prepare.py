"""Time the data preparation (puflow_amd.sampling / python -m puflow_amd.prepare, DESIGN "Poisson-disk sampling") on one GPU:

  python tools/time_prepare.py [--out profiles/prepare] [--patches 50] [--repeats 3]

Per mesh (a generated torus and the meshes of tests/golden/eval_uniform.npz): wall time of the clouds 2048 and 8192 and of
50 patches, phases / rounds / launches per pool of the elimination, and - for scale - the wall time of the sequential
restatement (tests/poisson_ref.py: numpy graph, heap-ordered greedy removal) on the pools small enough for it.  There is no
reference counterpart and no earlier implementation to compare with: the figures are a record, not a bar.
Writes time_prepare.json / time_prepare.txt under --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import poisson_ref as R  # noqa: E402
from puflow_amd import metrics, sampling  # noqa: E402

DEV = "cuda:0"


def torus(nu=96, nv=48, R0=1.0, r0=0.4):
    u, v = np.arange(nu) * (2.0 * np.pi / nu), np.arange(nv) * (2.0 * np.pi / nv)
    uu, vv = np.meshgrid(u, v, indexing="ij")
    verts = np.stack([(R0 + r0 * np.cos(vv)) * np.cos(uu), (R0 + r0 * np.cos(vv)) * np.sin(uu), r0 * np.sin(vv)], -1)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b = idx, np.roll(idx, -1, 0)
    c, d = np.roll(b, -1, 1), np.roll(idx, -1, 1)
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return verts.reshape(-1, 3).astype(np.float32), faces.astype(np.int64)


def wall(fn, repeats):
    """(best wall time in ms of `repeats` synchronised calls after one warm-up call, the last result)."""
    out = fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t) * 1e3)
    return best, out


def pool_record(pts, s, m, area, repeats, restate):
    ms, (keep, info) = wall(lambda: sampling.eliminate(pts, [s], [m], [area]), repeats)
    ms_graph, g = wall(lambda: sampling.neighbour_graph(pts, [s], [area], [m]), repeats)
    rec = {"s": s, "m": m, "path": info["paths"][0], "phases": int(info["phases"][0]), "rounds": int(info["rounds"][0]),
           "launches": info["launches"] + 2, "edges": int(g[1].numel()), "gpu_ms": round(ms, 3), "gpu_graph_ms": round(ms_graph, 3)}
    if restate:
        p = pts.cpu().numpy()
        t = time.perf_counter()
        graph = R.neighbour_graph(p, area, m)
        t1 = time.perf_counter()
        seq = R.eliminate_sequential(*graph, m)
        t2 = time.perf_counter()
        rec.update(cpu_graph_ms=round((t1 - t) * 1e3, 1), cpu_sequential_ms=round((t2 - t1) * 1e3, 1),
                   equal=bool(np.array_equal(seq, keep.cpu().numpy())))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prepare"))
    ap.add_argument("--patches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    meshes = {"torus_9216f": torus()}
    fx = np.load(os.path.join(ROOT, "tests", "golden", "eval_uniform.npz"))
    for c in range(int(fx["ncases"])):
        meshes[bytes(fx[f"c{c}_name"]).decode()] = (fx[f"c{c}_verts"].astype(np.float32), fx[f"c{c}_faces"].astype(np.int64))
    result = {"device": torch.cuda.get_device_name(0), "patches": a.patches, "repeats": a.repeats, "meshes": {}}
    lines = []
    for name, (v, f) in meshes.items():
        vt, ft = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
        area = float(metrics.mesh_area_radii(v, f)[1][-1])
        rec = {"faces": int(len(f)), "area": area, "pools": []}
        rec["clouds_2048_8192_ms"], _ = wall(lambda: [sampling.poisson_disk(vt, ft, n, 3 + i) for i, n in enumerate((2048, 8192))],
                                             a.repeats)
        rec["patches_ms"], (_, pools) = wall(lambda: sampling.make_patches(vt, ft, a.patches, return_pools=True), a.repeats)
        for n, sd, restate in ((2048, 3, True), (8192, 4, False)):
            pts = metrics.sample_mesh(vt, ft, 5 * n, sd)[0]
            rec["pools"].append(dict(pool_record(pts, 5 * n, n, area, a.repeats, restate), what=f"cloud {n}"))
        for key, n, n_set in (("input_pool", 256, 12500), ("gt_pool", 1024, 50000)):
            rec["pools"].append(dict(pool_record(pools[key][0].contiguous(), 5 * n, n, area * 5 * n / n_set, a.repeats, True),
                                     what=f"patch 0 {key}"))
        # all patch pools of the mesh in one call, as make_patches runs them
        P = a.patches
        pts = torch.cat([pools["input_pool"].reshape(-1, 3), pools["gt_pool"].reshape(-1, 3)])
        sizes, targets = [1280] * P + [5120] * P, [256] * P + [1024] * P
        areas = [area * 1280 / 12500] * P + [area * 5120 / 50000] * P
        ms, (_, info) = wall(lambda: sampling.eliminate(pts, sizes, targets, areas), a.repeats)
        rec["patch_pools_one_call"] = {"pools": 2 * P, "gpu_ms": round(ms, 3), "launches": info["launches"] + 2,
                                       "launches_per_pool": round((info["launches"] + 2) / (2 * P), 3),
                                       "phases_min_max": [int(info["phases"].min()), int(info["phases"].max())],
                                       "rounds_min_max": [int(info["rounds"].min()), int(info["rounds"].max())]}
        rec["clouds_2048_8192_ms"], rec["patches_ms"] = round(rec["clouds_2048_8192_ms"], 2), round(rec["patches_ms"], 2)
        result["meshes"][name] = rec
        lines.append(f"{name}: {len(f)} faces  clouds 2048 + 8192: {rec['clouds_2048_8192_ms']} ms   {P} patches: {rec['patches_ms']} ms")
        for r in rec["pools"]:
            cpu = (f"   CPU restatement: graph {r['cpu_graph_ms']} ms + sequential {r['cpu_sequential_ms']} ms, equal {r['equal']}"
                   if "equal" in r else "")
            lines.append(f"  {r['what']:>20}: {r['s']} -> {r['m']}  {r['path']:>9}  {r['phases']} phases {r['rounds']} rounds "
                         f"{r['launches']} launches  {r['edges']} edges  GPU {r['gpu_ms']} ms (graph alone {r['gpu_graph_ms']}){cpu}")
        o = rec["patch_pools_one_call"]
        lines.append(f"  {o['pools']} patch pools in one call: {o['gpu_ms']} ms, {o['launches']} launches ({o['launches_per_pool']} per "
                     f"pool), phases {o['phases_min_max']}, rounds {o['rounds_min_max']}")
        print("\n".join(lines[-(len(rec["pools"]) + 2):]), flush=True)
    with open(os.path.join(a.out, "time_prepare.json"), "w") as fh:
        json.dump(result, fh, indent=1)
    with open(os.path.join(a.out, "time_prepare.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
