#!/usr/bin/env python3
"""pf_knn_grid against pf_knn_large, per query, by device events, at the shapes DESIGN.md 8e reports for the attribute search:
  N = 5000 input points, M = 20 000 output points, K = 8        (--attributes on a 5000-point file)
  self-search in 20 000 points, K = 16                          (--estimate_normals 16 on its output)
  N = 16 384, M = 65 536, K = 8  and  self-search in 65 536, K = 16
and, for the grid alone, the 262 144-point scan (K = 8 from its 1 048 576 output points, K = 16 among those).
The legs alternate (large, grid, large, grid, ...), --rounds each after one untimed call; a leg's figure is its median, its
spread max - min.  The grid's figure includes its build (box, histogram, scan, scatter), which is also timed alone as a call with
a single query.  `faster` is only said where the difference exceeds three spreads of the pf_knn_large leg.  Results are checked
equal on every shape where both run.
  python tools/time_knn_grid.py [--out-dir profiles/knn_grid] [--commit ID] [--rounds 5] [--skip-large-above N]"""
import json, os, socket, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from puflow_amd import ops
from puflow_amd.weights import synth_patches

args = sys.argv[1:]
out_dir = args[args.index("--out-dir") + 1] if "--out-dir" in args else os.path.join(ROOT, "profiles", "knn_grid")
commit = args[args.index("--commit") + 1] if "--commit" in args else "unknown"
rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 5
skip_above = int(args[args.index("--skip-large-above") + 1]) if "--skip-large-above" in args else 65536
DEV = "cuda:0"
lines, record = [], {"commit": commit, "rounds": rounds, "shapes": []}


def say(s):
    print(s, flush=True)
    lines.append(s)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record(); torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def stats(ms):
    s = sorted(ms)
    return s[len(s) // 2], s[-1] - s[0]


def shape(name, n, self_search, k):
    torch.manual_seed(n + k)
    cloud = synth_patches(1, n, seed=5, surface=True).to(DEV)                            # [1,n,3]
    if self_search:
        ref = query = cloud
    else:                                                                                # 4 output points about every input point
        ref, query = cloud, (cloud.repeat(1, 4, 1) + 0.002 * torch.randn((1, 4 * n, 3), device=DEV)).contiguous()
    m = query.shape[1]
    legs = {"grid": lambda: ops.knn_grid(ref, query, k), "build": lambda: ops.knn_grid(ref, query[:, :1].contiguous(), k)}
    if n <= skip_above:
        legs = {"large": lambda: ops.knn_large(ref, query, k), **legs}
    times, outs = {leg: [] for leg in legs}, {}
    for leg, fn in legs.items():
        outs[leg] = fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for leg, fn in legs.items():                                                     # alternated
            times[leg].append(event_ms(fn)[1])
    row = {"shape": name, "n": n, "m": m, "k": k}
    for leg in legs:
        med, spread = stats(times[leg])
        row[leg] = {"median_ms": med, "spread_ms": spread, "us_per_query": med * 1e3 / (1 if leg == "build" else m), "ms": times[leg]}
    text = f"{name:34s} N {n:7d} M {m:8d} K {k:2d}: grid {row['grid']['us_per_query']:8.4f} us/query ({row['grid']['median_ms']:9.3f} ms, spread " \
           f"{row['grid']['spread_ms']:.3f}; build alone {row['build']['median_ms']:.3f} ms, spread {row['build']['spread_ms']:.3f})"
    if "large" in legs:
        same = torch.equal(outs["large"][0], outs["grid"][0]) and torch.equal(outs["large"][1], outs["grid"][1])
        row["equal"] = bool(same)
        diff = row["large"]["median_ms"] - row["grid"]["median_ms"]
        bar = 3 * row["large"]["spread_ms"]
        row["verdict"] = "grid faster" if diff > bar else ("grid slower" if -diff > bar else "no difference beyond 3 spreads")
        text += f" | pf_knn_large {row['large']['us_per_query']:8.4f} us/query ({row['large']['median_ms']:9.3f} ms, spread " \
                f"{row['large']['spread_ms']:.3f}) | x{row['large']['median_ms'] / row['grid']['median_ms']:.1f}: {row['verdict']}; results equal: {same}"
    else:
        text += " | pf_knn_large not run at this size"
    record["shapes"].append(row)
    say(text)
    return row.get("equal", True)


ok = True
for spec in (("attributes, 5000-point file", 5000, False, 8), ("normals, its 20 000 outputs", 20000, True, 16),
             ("attributes, 16 384-point scan", 16384, False, 8), ("normals, its 65 536 outputs", 65536, True, 16),
             ("small cloud, 300 points", 300, False, 8), ("small cloud, 1200 self", 1200, True, 16),
             ("attributes, 262 144-point scan", 262144, False, 8), ("normals, its 1 048 576 outputs", 1048576, True, 16)):
    ok = shape(*spec) and ok
say(f"box: {socket.gethostname()} / {torch.cuda.get_device_name(0)}   commit: {commit}")
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "time_knn_grid.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
with open(os.path.join(out_dir, "time_knn_grid.json"), "w") as f:
    json.dump(record, f, indent=1)
sys.exit(0 if ok else 1)
