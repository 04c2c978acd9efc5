#!/usr/bin/env python3
"""What mesh_from_cloud costs, stage by stage, by device events: the median of --reps calls after one untimed call, with the
spread, on one cloud of 20 000, 262 144 and 1 048 576 points (the bumpy sheet of tools/time_normals_orient.py with normals from
estimate_normals(16, search="grid", orient="propagate"), K = 8, sigma = 1, the default cell size).  The stages are the library's
own, timed through mesh_from_cloud's _stage hook: the cell-size search (K = 7 self-search, median, box - up to the one host read),
mark, compaction (nonzero), the K search, IMLS, count (with the prefix sum), emit, unique, vertices.  What lies between the
stages (the corner-coordinate gathers, the scatter of the values) is in no stage.  Absolute times only.
  python tools/time_reconstruct.py [--out-dir profiles/reconstruct] [--commit ID] [--reps 5]
  python tools/time_reconstruct.py --accuracy [--out-dir ...]       # accuracy.txt: vertex distances on the analytic test surfaces
and the mesh of a 512-point torus against the mesh of its x4 upsampling with the trained weights of tests/golden"""
import json, os, socket, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

args = sys.argv[1:]
out_dir = args[args.index("--out-dir") + 1] if "--out-dir" in args else os.path.join(ROOT, "profiles", "reconstruct")
commit = args[args.index("--commit") + 1] if "--commit" in args else "unknown"
reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
SHAPES = (20000, 262144, 1048576)
K, SIGMA = 8, 1.0
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def write(name, record=None):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, name + ".txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    if record is not None:
        with open(os.path.join(out_dir, name + ".json"), "w") as f:
            json.dump(record, f, indent=1)


from puflow_amd import _lib, attributes as A, reconstruct as P
from puflow_amd.weights import synth_patches

torch.zeros(1, device="cuda"); torch.cuda.synchronize()
box = "%s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0))

if "--accuracy" in args:
    import attr_ref as R
    import recon_ref as M
    say("vertex distance to the analytic surface, mesh_from_cloud at the default cell size, K = 8, sigma = 1, analytic normals")
    for kind in ("sphere", "torus"):
        for n in (512, 2048):
            for noise in (0.0, 0.002):
                pts, nrm = R.surface(kind, noise, n)
                v, f, info = P.mesh_from_cloud(torch.from_numpy(pts).cuda(), torch.from_numpy(nrm.astype(np.float32)).cuda())
                v, f = v.cpu().numpy(), f.cpu().numpy()
                d = (M.sphere_distance if kind == "sphere" else M.torus_distance)(v)
                say(f"{kind:6s} n {n:5d} noise {noise:5.3f}: h {info['h']:.5f} dims {info['dims']} V {len(v)} F {len(f)} open edges "
                    f"{info['open_edges']} V-E+F {M.euler(v, f)} volume {M.volume(v, f):.4f} | vertex distance mean {d.mean() / info['h']:.4f} h, "
                    f"max {d.max() / info['h']:.4f} h (bound sqrt 3 = 1.7321 h)")
    # one quality figure: a 512-point torus meshed as it is, and after x4 upsampling with the trained weights
    from puflow_amd import upsample as U
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
    say("a 512-point torus (R 1, r 0.35) meshed with estimated, propagated normals (K = 16), and its x4 upsampling by the trained")
    say("weights of tests/golden/pretrained_pu1k.npz (--estimate_normals 16 --normals_orient propagate) meshed the same way:")
    p = torch.from_numpy(pts).cuda()
    nrm, _ = A.estimate_normals(p, 16, search="grid", orient="propagate")
    up = torch.from_numpy(np.ascontiguousarray(rows[:, :3])).cuda()
    upn = torch.from_numpy(np.ascontiguousarray(rows[:, 3:6])).cuda()
    upn = upn / upn.norm(dim=1, keepdim=True).clamp_min(1e-30)
    for name, a, b in (("input, 512 points", p, nrm), (f"x4 output, {len(rows)} points", up, upn)):
        v, f, info = P.mesh_from_cloud(a, b)
        v, f = v.cpu().numpy(), f.cpu().numpy()
        d = M.torus_distance(v)
        say(f"{name:24s}: h {info['h']:.5f} V {len(v)} F {len(f)} open edges {info['open_edges']} V-E+F {M.euler(v, f) if len(f) else 0} "
            f"volume {M.volume(v, f):.4f} (exact 2.4181) | vertex distance to the torus mean {d.mean():.5f}, max {d.max():.5f}; "
            f"the cloud's own points: mean {M.torus_distance(a.cpu().numpy()).mean():.5f}")
    say(f"box: {box}   commit: {commit}")
    write("accuracy")
    sys.exit(0)


STAGES = ("cell-size search", "mark", "compaction", "K search", "IMLS", "count", "emit", "unique", "vertices")


def staged(points, normals):
    """mesh_from_cloud with an event pair around every stage, through its _stage hook: ({stage: ms}, info)"""
    ms, active = {}, []

    def stage(name, thunk):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = thunk(); b.record(); torch.cuda.synchronize()
        ms[name] = a.elapsed_time(b)
        if name == "compaction":
            active.append(int(out.shape[0]))
        return out
    verts, faces, info = P.mesh_from_cloud(points, normals, k=K, sigma=SIGMA, _stage=stage)
    return ms, {"h": info["h"], "dims": info["dims"], "corners": int(np.prod(info["dims"])), "active_corners": active[0],
                "triangles": int(faces.shape[0]), "vertices": int(verts.shape[0])}


record = {"commit": commit, "k": K, "sigma": SIGMA, "reps": reps, "box": box, "rows": []}
ok = True
for n in SHAPES:
    points = synth_patches(1, n, seed=5, surface=True)[0].to("cuda:0")
    normals, _ = A.estimate_normals(points, 16, search="grid", orient="propagate")
    try:
        staged(points, normals); torch.cuda.synchronize()                          # untimed
    except _lib.PuflowHipError as e:
        say(f"{n:8d} points: refused - {e}")
        record["rows"].append({"points": n, "refused": str(e)})
        continue
    runs = [staged(points, normals) for _ in range(reps)]
    info = runs[0][1]
    row = {"points": n, **info, "stages": {}}
    say(f"{n:8d} points: h {info['h']:.6f}, box {info['dims'][0]} x {info['dims'][1]} x {info['dims'][2]} = {info['corners']} corners, "
        f"{info['active_corners']} active, {info['triangles']} triangles, {info['vertices']} vertices")
    whole = sorted(sum(r[0].values()) for r in runs)
    for s in STAGES:
        v = sorted(r[0][s] for r in runs)
        row["stages"][s] = {"median_ms": v[len(v) // 2], "spread_ms": v[-1] - v[0]}
        say(f"    {s:18s} {v[len(v) // 2]:10.3f} ms (spread {v[-1] - v[0]:.3f})")
    row["sum_median_ms"], row["sum_spread_ms"] = whole[len(whole) // 2], whole[-1] - whole[0]
    say(f"    {'sum of the stages':18s} {row['sum_median_ms']:10.3f} ms (spread {row['sum_spread_ms']:.3f})")
    a = P.mesh_from_cloud(points, normals, k=K, sigma=SIGMA)
    b = P.mesh_from_cloud(points, normals, k=K, sigma=SIGMA)
    row["same_bits_twice"] = bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]))
    row["open_edges"] = a[2]["open_edges"]
    ok = ok and row["same_bits_twice"]
    say(f"    the same bits from two calls: {row['same_bits_twice']}; open edges {row['open_edges']} (an open sheet: its rim, and its "
        "jitter against a cell of the sampling spacing)")
    record["rows"].append(row)
    del points, normals, runs, a, b
    torch.cuda.empty_cache()
say(f"medians of {reps} calls after one untimed call, device events; box: {box}   commit: {commit}")
write("time_reconstruct", record)
sys.exit(0 if ok else 1)
