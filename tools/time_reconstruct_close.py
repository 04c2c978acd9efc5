#!/usr/bin/env python3
"""mesh_from_cloud(close_holes=R) at R = 0, 2 and 8 side by side, by tools/time_reconstruct_sparse.py's method: device events per
stage (the library's own stages, through mesh_from_cloud's _stage hook), the median of --reps calls after one untimed call; the legs alternate in FRESH processes over --rounds rounds; a leg's
figure is the median over the rounds of its medians, its spread the largest minus the smallest of them.  By the project's rule a
difference counts only beyond three spreads.  The growth stages are timed per round of growth and reported summed over the
rounds: the grow sweep (pf_recon_grow with its memset), the compaction (added & ~flags, nonzero), the K search and the IMLS
stage.  The exit count for info["grown_cells"], once after the rounds, is in no stage: it shows in the whole call only.
Shapes: the bumpy sheets of tools/time_reconstruct.py at 20 000, 262 144 and 1 048 576 points (normals from
estimate_normals(16, search="grid", orient="propagate")).  They are open, so every round grows.
--parent-root DIR adds a leg that runs the same hook on the package of another tree (a built checkout of a parent commit that
has the hook): R = 0 must stay within three spreads of it.
  python tools/time_reconstruct_close.py [--out-dir profiles/reconstruct_close] [--commit ID] [--reps 5] [--rounds 3]
                                         [--parent-root DIR]
  python tools/time_reconstruct_close.py --accuracy [--out-dir ...]     # accuracy.txt: what the rounds do to the meshes of the
      clouds with holes and to the x4 output of the 512-point torus by the trained weights, at R = 0, 1, 2, 4 and 8"""
import json, os, socket, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
opt = lambda name, default: args[args.index(name) + 1] if name in args else default
sys.path.insert(0, opt("--package-root", ROOT))
import numpy as np
import torch

out_dir = opt("--out-dir", os.path.join(ROOT, "profiles", "reconstruct_close"))
commit, reps, rounds = opt("--commit", "unknown"), int(opt("--reps", 5)), int(opt("--rounds", 3))
parent_root = opt("--parent-root", None)
SHEETS = (20000, 262144, 1048576)
K, SIGMA = 8, 1.0
BASE = ("cell-size search", "mark", "compaction", "K search", "IMLS")
GROW = ("grow sweep", "grow compaction", "grow K search", "grow IMLS")
TAIL = ("count", "emit", "unique", "vertices")

from puflow_amd import reconstruct as P


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record(); torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def staged(points, normals, R):
    """mesh_from_cloud(close_holes=R) with an event pair around every stage, through its _stage hook: ({stage: ms}, info).  From
    the first "grow" on, the stages up to the extraction belong to the rounds and are summed over them under GROW's names."""
    ms, sizes = {s: 0.0 for s in BASE + (GROW if R else ()) + TAIL}, []     # in the order they run
    in_rounds = {"grow": "grow sweep", "compaction": "grow compaction", "K search": "grow K search", "IMLS": "grow IMLS"}

    def stage(name, thunk):
        out, t = event_ms(thunk)
        if name == "compaction":
            sizes.append(int(out.shape[0]))
        stage.growing = (stage.growing or name == "grow") and name in in_rounds
        ms[in_rounds[name] if stage.growing else name] += t
        return out
    stage.growing = False
    verts, faces, info = P.mesh_from_cloud(points, normals, k=K, sigma=SIGMA, _stage=stage, **({"close_holes": R} if R else {}))
    return ms, {"h": info["h"], "dims": info["dims"], "corners": int(np.prod([int(d) for d in info["dims"]])), "active_corners": sizes[0],
                "new_corners": sum(sizes[1:]), "exits": info["grown_cells"], "triangles": int(faces.shape[0]),
                "vertices": int(verts.shape[0])}


def leg(R, cloud_dir, out_path):
    """one leg in this (fresh) process: every shape, the medians of `reps` staged calls after one untimed call"""
    torch.zeros(1, device="cuda"); torch.cuda.synchronize()
    kw = {"close_holes": R} if R else {}                                    # R = 0: the call as the parent commit has it
    rows = []
    for name in [str(n) for n in SHEETS]:
        rowsin = np.load(os.path.join(cloud_dir, name + ".npy"))
        points, normals = torch.from_numpy(rowsin[:, :3].copy()).cuda(), torch.from_numpy(rowsin[:, 3:].copy()).cuda()
        row = {"cloud": name, "points": int(points.shape[0])}
        staged(points, normals, R); torch.cuda.synchronize()                # untimed
        runs = [staged(points, normals, R) for _ in range(reps)]
        row.update(runs[0][1])
        row["stages"] = {s: sorted(r[0][s] for r in runs)[reps // 2] for s in runs[0][0]}
        row["sum_ms"] = sorted(sum(r[0].values()) for r in runs)[reps // 2]
        del runs
        P.mesh_from_cloud(points, normals, k=K, sigma=SIGMA, **kw); torch.cuda.synchronize()
        calls = [event_ms(lambda: P.mesh_from_cloud(points, normals, k=K, sigma=SIGMA, **kw)) for _ in range(reps)]
        row["call_ms"] = sorted(c[1] for c in calls)[reps // 2]             # the whole call, host reads included
        a, b = calls[0][0], calls[-1][0]
        row["same_bits_twice"] = bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]))
        row["open_edges"] = a[2]["open_edges"]
        row["grown_cells"] = a[2].get("grown_cells", [])
        row["mesh_crc"] = [int(a[0].view(torch.int32).to(torch.int64).sum()), int(a[1].to(torch.int64).sum())]
        rows.append(row)
        del points, normals, a, b, calls
        torch.cuda.empty_cache()
    with open(out_path, "w") as fh:
        json.dump(rows, fh)


if "--leg" in args:
    leg(int(opt("--leg", 0)), opt("--clouds", None), opt("--json", None))
    sys.exit(0)

# ---- the parent process: make the clouds once, run the legs, write the report ---------------------------------------------------
from puflow_amd import attributes as A
from puflow_amd.weights import synth_patches

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


torch.zeros(1, device="cuda"); torch.cuda.synchronize()
box = "%s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0))

if "--accuracy" in args:
    # accuracy.txt: what the rounds do to the meshes - the clouds with holes of the tests, then the project's open case, the x4
    # output of the 512-point torus by the trained weights (88 open edges at R = 0), reported as it falls
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import attr_ref as R
    import recon_grow_ref as G
    import recon_ref as M
    from puflow_amd import upsample as U

    def row(name, a, b, rounds, distance, exact):
        v, f, info = P.mesh_from_cloud(a, b, close_holes=rounds)
        v, f = v.cpu().numpy(), f.cpu().numpy()
        d = distance(v)
        say(f"{name:26s} R {rounds}: h {info['h']:.5f} dims {info['dims']} exits {info['grown_cells']} V {len(v)} F {len(f)} open edges "
            f"{info['open_edges']} V-E+F {M.euler(v, f)} volume {M.volume(v, f):.4f} (exact {exact:.4f}) | vertex distance mean "
            f"{d.mean():.5f}, max {d.max():.5f} = {d.max() / info['h']:.2f} h")

    say("mesh_from_cloud(close_holes=R) at the default cell size, K = 8, sigma = 1, analytic normals, on clouds with a hole cut out:")
    for name in ("sphere-512-0.7", "sphere-512-0.9", "sphere-2048-0.4", "sphere-2048-0.5", "sphere-2048-0.9", "torus"):
        pts, nrm = G.cloud(name)
        for rounds in (0, 8):
            row(f"{name} ({len(pts)} points)", torch.from_numpy(pts).cuda(), torch.from_numpy(nrm).cuda(), rounds,
                M.torus_distance if name == "torus" else M.sphere_distance, 2 * np.pi ** 2 * 0.35 ** 2 if name == "torus" else 4 / 3 * np.pi)
    g = np.load(os.path.join(ROOT, "tests", "golden", "pretrained_pu1k.npz"))
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}
    pts, _ = R.surface("torus", 0.0, 512)
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "in"))
        os.makedirs(os.path.join(tmp, "out"))
        np.savetxt(os.path.join(tmp, "in", "torus.xyz"), pts.astype(np.float64), fmt="%.6f")
        U.upsampling([os.path.join(tmp, "in", "torus.xyz")], os.path.join(tmp, "out"), None, up_ratio=4, num_outlier=24, num_patch=256,
                     seed=2021, state_dict=sd, estimate_normals=16, attr_search="grid", normals_orient="propagate")
        rows = U.load_xyz(os.path.join(tmp, "out", "torus.xyz"))
    say("")
    say("the x4 upsampling of a 512-point torus (R 1, r 0.35) by the trained weights of tests/golden/pretrained_pu1k.npz")
    say("(--estimate_normals 16 --normals_orient propagate), meshed with 0, 1, 2, 4 and 8 rounds:")
    up = torch.from_numpy(np.ascontiguousarray(rows[:, :3])).cuda()
    upn = torch.from_numpy(np.ascontiguousarray(rows[:, 3:6])).cuda()
    upn = upn / upn.norm(dim=1, keepdim=True).clamp_min(1e-30)
    for rounds in (0, 1, 2, 4, 8):
        row(f"x4 output, {len(rows)} points", up, upn, rounds, M.torus_distance, 2 * np.pi ** 2 * 0.35 ** 2)
    say(f"box: {box}   commit: {commit}")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "accuracy.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0)
legs = ([("parent", 0, parent_root)] if parent_root else []) + [("R = 0", 0, ROOT), ("R = 2", 2, ROOT), ("R = 8", 8, ROOT)]
results = {name: [] for name, _, _ in legs}
with tempfile.TemporaryDirectory() as tmp:
    for n in SHEETS:
        points = synth_patches(1, n, seed=5, surface=True)[0].to("cuda:0")
        normals, _ = A.estimate_normals(points, 16, search="grid", orient="propagate")
        np.save(os.path.join(tmp, f"{n}.npy"), torch.cat([points, normals], dim=1).cpu().numpy())
        del points, normals
    torch.cuda.empty_cache()
    for r in range(rounds):
        for name, R, root in legs:
            path = os.path.join(tmp, "leg.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", str(R), "--clouds", tmp, "--json", path, "--reps", str(reps),
                            "--package-root", root], check=True, timeout=600)
            with open(path) as fh:
                results[name].append(json.load(fh))

mid = lambda v: sorted(v)[len(v) // 2]
spread = lambda v: max(v) - min(v)
record = {"commit": commit, "k": K, "sigma": SIGMA, "reps": reps, "rounds": rounds, "box": box, "clouds": []}
ok = True
for c, cloud in enumerate([str(n) for n in SHEETS]):
    entry = {"cloud": cloud, "legs": {}}
    say(f"bumpy sheet, {results['R = 0'][0][c]['points']} points")
    for name, R, _ in legs:
        per_round = [results[name][r][c] for r in range(rounds)]
        info = per_round[0]
        stages = list(info["stages"])
        e = {k: info[k] for k in ("h", "dims", "corners", "active_corners", "new_corners", "exits", "triangles", "vertices", "open_edges",
                                  "grown_cells", "mesh_crc")}
        e["stages"] = {s: {"median_ms": mid([p["stages"][s] for p in per_round]), "spread_ms": spread([p["stages"][s] for p in per_round])}
                       for s in stages}
        e["sum_median_ms"], e["sum_spread_ms"] = mid([p["sum_ms"] for p in per_round]), spread([p["sum_ms"] for p in per_round])
        e["call_median_ms"], e["call_spread_ms"] = mid([p["call_ms"] for p in per_round]), spread([p["call_ms"] for p in per_round])
        e["same_bits_twice"] = all(p["same_bits_twice"] for p in per_round)
        ok = ok and e["same_bits_twice"] and info["exits"] == info["grown_cells"]
        entry["legs"][name] = e
        say(f"  {name}: h {info['h']:.6f}, grid {info['dims'][0]} x {info['dims'][1]} x {info['dims'][2]} = {info['corners']} corners, "
            f"{info['active_corners']} in the band + {info['new_corners']} grown, exits per round {info['exits']}, {info['triangles']} "
            f"triangles, {info['vertices']} vertices, open edges {info['open_edges']}")
        for s in stages:
            say(f"      {s:18s} {e['stages'][s]['median_ms']:10.3f} ms (spread {e['stages'][s]['spread_ms']:.3f})")
        say(f"      {'sum of the stages':18s} {e['sum_median_ms']:10.3f} ms (spread {e['sum_spread_ms']:.3f}); the whole call "
            f"{e['call_median_ms']:.3f} ms (spread {e['call_spread_ms']:.3f}); the same bits from two calls: {e['same_bits_twice']}")
    L = entry["legs"]
    if "parent" in L:
        diff, bar = L["R = 0"]["sum_median_ms"] - L["parent"]["sum_median_ms"], 3 * L["parent"]["sum_spread_ms"]
        same = L["R = 0"]["mesh_crc"] == L["parent"]["mesh_crc"]
        entry["r0_minus_parent_ms"], entry["r0_within_three_spreads"], entry["r0_same_mesh"] = diff, bool(abs(diff) <= bar), same
        ok = ok and same
        say(f"  R = 0 - parent: {diff:+.3f} ms on the sum, three spreads of the parent leg {bar:.3f} ms: "
            f"{'within' if abs(diff) <= bar else 'BEYOND'}; the same mesh (checksums): {same}")
    for name in ("R = 2", "R = 8"):
        diff = L[name]["sum_median_ms"] - L["R = 0"]["sum_median_ms"]
        n = max(len(L[name]["exits"]), 1)
        grow = sum(L[name]["stages"][s]["median_ms"] for s in GROW)
        say(f"  {name} - R = 0: {diff:+.3f} ms on the sum ({100 * diff / L['R = 0']['sum_median_ms']:+.1f} %); the rounds "
            f"{grow:.3f} ms = {grow / n:.3f} ms per round, of it the sweep {L[name]['stages']['grow sweep']['median_ms'] / n:.3f}")
    record["clouds"].append(entry)
say(f"medians over {rounds} rounds of fresh processes of the medians of {reps} calls after one untimed call, device events; "
    f"box: {box}   commit: {commit}")
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "time_reconstruct_close.txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
with open(os.path.join(out_dir, "time_reconstruct_close.json"), "w") as fh:
    json.dump(record, fh, indent=1)
sys.exit(0 if ok else 1)
