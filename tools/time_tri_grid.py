#!/usr/bin/env python3
"""point_to_mesh_distance(search="tiles") against search="grid", by device events, the Morton sort and (for the grid) the grid
build and its one host read included:
  P in {8192, 262 144} near-surface queries x F in {10^4, 10^5, 10^6} faces of the bumpy torus of tests/eval_ref.py,
  P in {8192, 262 144} x the mesh mesh_from_cloud makes from the 262 144-point sheet of tools/time_reconstruct.py,
  and one mesh_metrics.score of that mesh against the same sheet meshed at 1.5 cells (100 000 samples each way).
Every leg of every round is a FRESH process (this script started again with --child LEG) that runs all shapes: one untimed call,
then --reps timed ones, of which it reports the median.  The legs alternate (tiles, grid, tiles, grid, ...) over --rounds rounds; a
leg's figure is the median of its rounds, its spread max - min.  A difference is only called real beyond three spreads of the
tiles leg.  The legs' results are checked equal (a checksum of distances and faces).
  python tools/time_tri_grid.py [--out-dir profiles/tri_grid] [--commit ID] [--rounds 3] [--reps 3]"""
import json, os, socket, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

args = sys.argv[1:]
out_dir = args[args.index("--out-dir") + 1] if "--out-dir" in args else os.path.join(ROOT, "profiles", "tri_grid")
commit = args[args.index("--commit") + 1] if "--commit" in args else "unknown"
rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 3
reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 3
TORI = (("torus 10^4", 100, 50), ("torus 10^5", 316, 158), ("torus 10^6", 1000, 500))
QUERIES = (8192, 262144)


def child(leg):
    import numpy as np
    import torch
    import eval_ref as R
    from puflow_amd import attributes as A, mesh_metrics, metrics, reconstruct as P
    from puflow_amd.weights import synth_patches
    dev = "cuda:0"

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = fn(); b.record(); torch.cuda.synchronize()
        return out, a.elapsed_time(b)

    def timed(name, P_, F_, fn, check):
        out = fn()                                                                       # untimed
        torch.cuda.synchronize()
        ms = sorted(event_ms(fn)[1] for _ in range(reps))
        print(json.dumps({"shape": name, "P": P_, "F": F_, "leg": leg, "ms": ms[len(ms) // 2], "check": check(out)}), flush=True)

    def p2f(name, v, f, q):
        timed(name, q.shape[0], f.shape[0], lambda: metrics.point_to_mesh_distance(q, v, f, return_face=True, search=leg),
              lambda o: [float(o[0].double().sum()), int(o[1].sum())])

    for name, nu, nv in TORI:
        v, f = R.torus(nu, nv, bump=0.15)
        rng = np.random.default_rng(9)
        pts = R.sample_surface(v, f, QUERIES[-1], rng) + rng.normal(0, 0.01, (QUERIES[-1], 3))
        vd, fd = torch.from_numpy(v.astype(np.float32)).to(dev), torch.from_numpy(f).to(dev)
        qd = torch.from_numpy(pts.astype(np.float32)).to(dev)
        for n in QUERIES:
            p2f(name, vd, fd, qd[:n].contiguous())
    points = synth_patches(1, 262144, seed=5, surface=True)[0].to(dev)
    normals, _ = A.estimate_normals(points, 16, search="grid", orient="propagate")
    v, f, _ = P.mesh_from_cloud(points, normals)
    f = f.long()
    q, _, _ = metrics.sample_mesh(v, f, QUERIES[-1], 0)
    q = q + 0.002 * torch.randn(q.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    for n in QUERIES:
        p2f("reconstructed sheet", v, f, q[:n].contiguous())
    gv, gf, _ = P.mesh_from_cloud(points, normals, cell_scale=1.5)
    timed("mesh_metrics.score, sheet", 100000, f.shape[0],
          lambda: mesh_metrics.score(v, f, gv, gf.long(), samples=100000, seed=0, tau=0.01, search=leg),
          lambda s: [s[k] for k in mesh_metrics.COLUMNS[1:]])


if "--child" in args:
    child(args[args.index("--child") + 1])
    sys.exit(0)

lines, runs = [], {}


def say(s):
    print(s, flush=True)
    lines.append(s)


for r in range(rounds):
    for leg in ("tiles", "grid"):                                                        # alternated, a fresh process each
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--reps", str(reps)], check=True,
                             stdout=subprocess.PIPE, text=True, timeout=900).stdout
        for ln in out.splitlines():
            if ln.startswith("{"):
                row = json.loads(ln)
                runs.setdefault((row["shape"], row["P"], row["F"]), {}).setdefault(leg, []).append(row)
        print(f"round {r} leg {leg} done", flush=True)

import torch
record = {"commit": commit, "rounds": rounds, "reps": reps, "shapes": []}
ok = True
for (name, P_, F_), legs in runs.items():
    row = {"shape": name, "P": P_, "F": F_}
    for leg, rs in legs.items():
        ms = sorted(x["ms"] for x in rs)
        row[leg] = {"median_ms": ms[len(ms) // 2], "spread_ms": ms[-1] - ms[0], "ms": [x["ms"] for x in rs]}
    same = all(x["check"] == legs["tiles"][0]["check"] for rs in legs.values() for x in rs)
    ok = ok and same
    diff, bar = row["tiles"]["median_ms"] - row["grid"]["median_ms"], 3 * row["tiles"]["spread_ms"]
    row["equal"] = same
    row["verdict"] = "grid faster" if diff > bar else ("grid slower" if -diff > bar else "no difference beyond 3 spreads")
    record["shapes"].append(row)
    say(f"{name:28s} P {P_:7d} F {F_:8d}: tiles {row['tiles']['median_ms']:10.3f} ms (spread {row['tiles']['spread_ms']:.3f}) | grid "
        f"{row['grid']['median_ms']:10.3f} ms (spread {row['grid']['spread_ms']:.3f}) | x{row['tiles']['median_ms'] / row['grid']['median_ms']:.2f}: "
        f"{row['verdict']}; results equal: {same}")
say(f"box: {socket.gethostname()} / {torch.cuda.get_device_name(0)}   commit: {commit}")
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "time_tri_grid.txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
with open(os.path.join(out_dir, "time_tri_grid.json"), "w") as fh:
    json.dump(record, fh, indent=1)
sys.exit(0 if ok else 1)
