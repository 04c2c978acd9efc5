#!/usr/bin/env python3
"""The two layouts of mesh_from_cloud side by side, by tools/time_reconstruct.py's method: device events per stage (the library's
own stages, through mesh_from_cloud's _stage hook), the median of --reps calls after one untimed call.  layout="dense" and
layout="sparse" legs alternate in FRESH processes over --rounds rounds; a leg's figure is the median over the rounds of its medians, its spread the largest minus the smallest of them.  By the
project's rule a difference counts only beyond three spreads of the dense leg.  Every leg also records its peak of allocated
device memory over one whole mesh_from_cloud call (torch.cuda.max_memory_allocated above what the cloud itself holds).
Shapes: the bumpy sheets of tools/time_reconstruct.py at 20 000, 262 144 and 1 048 576 points (normals from
estimate_normals(16, search="grid", orient="propagate")), and a closed unit sphere of 4 194 304 points with analytic normals,
whose box at the default cell the dense layout refuses.
  python tools/time_reconstruct_sparse.py [--out-dir profiles/reconstruct_sparse] [--commit ID] [--reps 5] [--rounds 3]"""
import json, os, socket, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

args = sys.argv[1:]
opt = lambda name, default: args[args.index(name) + 1] if name in args else default
out_dir = opt("--out-dir", os.path.join(ROOT, "profiles", "reconstruct_sparse"))
commit, reps, rounds = opt("--commit", "unknown"), int(opt("--reps", 5)), int(opt("--rounds", 3))
SHEETS = (20000, 262144, 1048576)
SPHERE = 4194304
K, SIGMA = 8, 1.0

from puflow_amd import _lib, reconstruct as P


STAGES = {"dense": ("cell-size search", "mark", "compaction", "K search", "IMLS", "count", "emit", "unique", "vertices"),
          "sparse": ("cell-size search", "block list", "mark", "compaction", "K search", "IMLS", "count", "emit", "unique", "vertices")}


def staged(points, normals, layout):
    """mesh_from_cloud with an event pair around every stage, through its _stage hook: ({stage: ms}, info)"""
    ms, active = {}, []

    def stage(name, thunk):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = thunk(); b.record(); torch.cuda.synchronize()
        ms[name] = a.elapsed_time(b)
        if name == "compaction":
            active.append(int(out.shape[0]))
        return out
    verts, faces, info = P.mesh_from_cloud(points, normals, k=K, sigma=SIGMA, layout=layout, _stage=stage)
    return ms, {"h": info["h"], "dims": info["dims"], "corners": int(np.prod([int(d) for d in info["dims"]])), "active_corners": active[0],
                "blocks": info["blocks"], "triangles": int(faces.shape[0]), "vertices": int(verts.shape[0])}


def leg(layout, cloud_dir, out_path):
    """one leg in this (fresh) process: every shape, the medians of `reps` staged calls after one untimed call"""
    torch.zeros(1, device="cuda"); torch.cuda.synchronize()
    rows = []
    for name in [str(n) for n in SHEETS] + ["sphere"]:
        rowsin = np.load(os.path.join(cloud_dir, name + ".npy"))
        points, normals = torch.from_numpy(rowsin[:, :3].copy()).cuda(), torch.from_numpy(rowsin[:, 3:].copy()).cuda()
        row = {"cloud": name, "points": int(points.shape[0])}
        try:
            staged(points, normals, layout); torch.cuda.synchronize()                  # untimed
        except _lib.PuflowHipError as e:
            row["refused"] = str(e)
            rows.append(row)
            continue
        runs = [staged(points, normals, layout) for _ in range(reps)]
        row.update(runs[0][1])
        row["stages"] = {s: sorted(r[0][s] for r in runs)[reps // 2] for s in STAGES[layout]}
        row["sum_ms"] = sorted(sum(r[0].values()) for r in runs)[reps // 2]
        del runs
        torch.cuda.empty_cache(); torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        a = P.mesh_from_cloud(points, normals, k=K, sigma=SIGMA, layout=layout)
        torch.cuda.synchronize()
        row["peak_bytes"] = int(torch.cuda.max_memory_allocated() - held)
        b = P.mesh_from_cloud(points, normals, k=K, sigma=SIGMA, layout=layout)
        row["same_bits_twice"] = bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]))
        row["open_edges"] = a[2]["open_edges"]
        row["mesh_crc"] = [int(a[0].view(torch.int32).to(torch.int64).sum()), int(a[1].to(torch.int64).sum())]      # legs must agree
        rows.append(row)
        del points, normals, a, b
        torch.cuda.empty_cache()
    with open(out_path, "w") as fh:
        json.dump(rows, fh)


if "--leg" in args:
    leg(opt("--leg", None), opt("--clouds", None), opt("--json", None))
    sys.exit(0)

# ---- the parent: make the clouds once, run the legs, write the report ---------------------------------------------------------
from puflow_amd import attributes as A
from puflow_amd.weights import synth_patches

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


torch.zeros(1, device="cuda"); torch.cuda.synchronize()
box = "%s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0))
legs = ("dense", "sparse")
results = {name: [] for name in legs}
with tempfile.TemporaryDirectory() as tmp:
    for n in SHEETS:
        points = synth_patches(1, n, seed=5, surface=True)[0].to("cuda:0")
        normals, _ = A.estimate_normals(points, 16, search="grid", orient="propagate")
        np.save(os.path.join(tmp, f"{n}.npy"), torch.cat([points, normals], dim=1).cpu().numpy())
        del points, normals
    v = torch.randn(SPHERE, 3, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    v = (v / v.norm(dim=1, keepdim=True)).to(torch.float32)
    np.save(os.path.join(tmp, "sphere.npy"), torch.cat([v, v], dim=1).numpy())
    del v
    torch.cuda.empty_cache()
    for r in range(rounds):
        for name in legs:
            path = os.path.join(tmp, "leg.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--clouds", tmp, "--json", path,
                            "--reps", str(reps)], check=True, timeout=600)
            with open(path) as fh:
                results[name].append(json.load(fh))

mid = lambda v: sorted(v)[len(v) // 2]
spread = lambda v: max(v) - min(v)
record = {"commit": commit, "k": K, "sigma": SIGMA, "reps": reps, "rounds": rounds, "box": box, "clouds": []}
ok = True
for c, cloud in enumerate([str(n) for n in SHEETS] + ["sphere"]):
    entry = {"cloud": cloud, "legs": {}}
    first = results["dense"][0][c]
    say(f"{'bumpy sheet' if cloud != 'sphere' else 'unit sphere, analytic normals'}, {first['points']} points")
    for name in legs:
        per_round = [results[name][r][c] for r in range(rounds)]
        if "refused" in per_round[0]:
            say(f"  {name}: refused - {per_round[0]['refused']}")
            entry["legs"][name] = {"refused": per_round[0]["refused"]}
            continue
        info = per_round[0]
        stages = STAGES[name]
        e = {k: info[k] for k in ("h", "dims", "corners", "active_corners", "blocks", "triangles", "vertices", "open_edges", "mesh_crc")}
        e["stages"] = {s: {"median_ms": mid([p["stages"][s] for p in per_round]), "spread_ms": spread([p["stages"][s] for p in per_round])}
                       for s in stages}
        e["sum_median_ms"], e["sum_spread_ms"] = mid([p["sum_ms"] for p in per_round]), spread([p["sum_ms"] for p in per_round])
        e["peak_bytes"] = max(p["peak_bytes"] for p in per_round)
        e["same_bits_twice"] = all(p["same_bits_twice"] for p in per_round)
        ok = ok and e["same_bits_twice"]
        entry["legs"][name] = e
        say(f"  {name}: h {info['h']:.6f}, grid {info['dims'][0]} x {info['dims'][1]} x {info['dims'][2]} = {info['corners']} corners, "
            f"{info['active_corners']} active, {info['blocks']} blocks, {info['triangles']} triangles, {info['vertices']} vertices")
        for s in stages:
            say(f"      {s:18s} {e['stages'][s]['median_ms']:10.3f} ms (spread {e['stages'][s]['spread_ms']:.3f})")
        say(f"      {'sum of the stages':18s} {e['sum_median_ms']:10.3f} ms (spread {e['sum_spread_ms']:.3f})")
        say(f"      peak of allocated device memory over one call {e['peak_bytes'] / 2 ** 20:10.1f} MiB; the same bits from two calls: "
            f"{e['same_bits_twice']}; open edges {info['open_edges']}")
    d, s = entry["legs"].get("dense", {}), entry["legs"].get("sparse", {})
    if "sum_median_ms" in d and "sum_median_ms" in s:
        same = d["mesh_crc"] == s["mesh_crc"] and d["triangles"] == s["triangles"] and d["vertices"] == s["vertices"]
        ok = ok and same
        diff = s["sum_median_ms"] - d["sum_median_ms"]
        entry["sparse_minus_dense_ms"], entry["counts"] = diff, bool(abs(diff) > 3 * d["sum_spread_ms"])
        say(f"  sparse - dense: {diff:+.3f} ms on the sum ({100 * diff / d['sum_median_ms']:+.1f} %), three spreads of the dense leg "
            f"{3 * d['sum_spread_ms']:.3f} ms: {'counts' if entry['counts'] else 'within the noise'}; peak memory x "
            f"{s['peak_bytes'] / max(d['peak_bytes'], 1):.2f}; the same mesh (checksums, counts): {same}")
    record["clouds"].append(entry)
say(f"medians over {rounds} rounds of fresh processes of the medians of {reps} calls after one untimed call, device events; "
    f"box: {box}   commit: {commit}")
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "time_reconstruct_sparse.txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
with open(os.path.join(out_dir, "time_reconstruct_sparse.json"), "w") as fh:
    json.dump(record, fh, indent=1)
sys.exit(0 if ok else 1)
