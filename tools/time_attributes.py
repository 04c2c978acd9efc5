#!/usr/bin/env python3
"""What --attributes and --estimate_normals add to the .xyz CLI, in one call on one box:
  dense:  32 files of 5000 points (tools/time_cli_ragged.py's setting), default cloud_batch
  tiled:  one scan of --tiled-points points (default 262 144) with --tile_points 4096
each as three legs - no flags | --attributes normal,lin3 | --estimate_normals 16 - alternated, two rounds, every leg in a FRESH
process under its own time limit.  A leg calls upsampling() twice; the second call (weights planned, allocator warm) is the
figure.  The comparison leg is the same tree without the flags (on the files' x y z columns).
  share:  where the added time goes, per output point, for clouds of 5000 and --tiled-points input points: the neighbour search
          (pf_knn_large, an existing kernel) against the new kernels (pf_attr_blend, pf_normals_pca), timed with events on
          --sample output points (the search's cost per query does not depend on how many queries there are).
--attr_search grid runs the attribute and normal legs with the uniform-grid search (pf_knn_grid) instead of pf_knn_large and
writes time_attributes_grid.txt / .json; `share` times pf_knn_large and is left out then (tools/time_knn_grid.py compares the
two searches).  --skip-dense / --skip-share leave those parts out.
A leg that fails or runs out of time ends the run: nothing else is started on the GPU after it.
  python tools/time_attributes.py [--out-dir profiles/attributes] [--commit ID] [--tiled-points N] [--sample Q] [--skip-tiled]
                                  [--attr_search brute|grid] [--skip-dense] [--skip-share]"""
import json, os, socket, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FLAGS = {"none": {}, "attributes": {"attributes": "normal,lin3"}, "normals": {"estimate_normals": 16}}

if len(sys.argv) > 1 and sys.argv[1] == "--child":
    src, dst, leg, tile_points, search = sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]), sys.argv[6]
    import torch
    from puflow_amd import upsample as U
    from puflow_amd.weights import synth_state_dict
    sd = synth_state_dict(2021)
    torch.zeros(1, device="cuda"); torch.cuda.synchronize()           # GPU context
    paths = sorted(os.path.join(src, f) for f in os.listdir(src))
    for tag in ("FIRST", "ELAPSED"):
        t0 = time.perf_counter()
        U.upsampling(paths, dst, None, up_ratio=4, num_outlier=24, num_patch=256, seed=2021, state_dict=sd,
                     tile_points=tile_points or None, **FLAGS[leg], **({} if leg == "none" else {"attr_search": search}))
        print("%s %.6f" % (tag, time.perf_counter() - t0), flush=True)
    print("BOX %s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0)), flush=True)
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "--share":
    n, q = int(sys.argv[2]), int(sys.argv[3])
    import torch
    from puflow_amd import _lib, ops
    from puflow_amd.weights import synth_patches
    cloud = synth_patches(1, n, seed=5, surface=True).to("cuda:0")                       # [1,n,3]
    m = 4 * n
    pred = (cloud.repeat(1, 4, 1) + 0.002 * torch.randn((1, m, 3), device="cuda:0")).contiguous()
    q = min(q, m)
    sample = pred[:, torch.randperm(m, device="cuda:0")[:q]].contiguous()
    attr = torch.randn((1, n, 6), device="cuda:0")
    plan = [(_lib.PF_ATTR_UNIT, 3), (_lib.PF_ATTR_LIN, 3)]

    def timed(fn, reps=3):
        fn(); torch.cuda.synchronize()
        best = None
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); out = fn(); b.record(); torch.cuda.synchronize()
            best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
        return out, best * 1e3 / q                                                       # microseconds per output point

    (idx, d2), s_attr = timed(lambda: ops.knn_large(cloud, sample, 8))
    _, k_attr = timed(lambda: ops.attr_blend(idx, d2, attr, plan))
    (idx16, _), s_nrm = timed(lambda: ops.knn_large(pred, sample, 16))                   # the output cloud's own neighbourhoods
    sub = torch.randint(0, q, (1, q, 16), dtype=torch.int32, device="cuda:0")            # the kernel's cost: K gathers per point
    _, k_nrm = timed(lambda: ops.normals_pca(sample, sub))
    print("RESULT " + json.dumps({"n": n, "outputs": m, "sample": q, "us_per_point": {
        "attributes_search": s_attr, "attributes_blend": k_attr, "normals_search": s_nrm, "normals_pca": k_nrm}}), flush=True)
    sys.exit(0)

import numpy as np
from puflow_amd.weights import synth_patches

args = sys.argv[1:]
out_dir = args[args.index("--out-dir") + 1] if "--out-dir" in args else os.path.join(ROOT, "profiles", "attributes")
commit = args[args.index("--commit") + 1] if "--commit" in args else "unknown"
tiled_points = int(args[args.index("--tiled-points") + 1]) if "--tiled-points" in args else 262144
sample = int(args[args.index("--sample") + 1]) if "--sample" in args else 4096
attr_search = args[args.index("--attr_search") + 1] if "--attr_search" in args else "brute"
if attr_search not in ("brute", "grid"):
    sys.exit("--attr_search: brute or grid")
stem = "time_attributes" if attr_search == "brute" else "time_attributes_" + attr_search
lines, record = [], {"commit": commit, "attr_search": attr_search, "legs": [], "share": []}


def say(s):
    print(s, flush=True)
    lines.append(s)


def finish(ok):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, stem + ".txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(out_dir, stem + ".json"), "w") as f:
        json.dump(record, f, indent=1)
    sys.exit(0 if ok else 1)


def write_scans(folder, sizes):
    """x y z | a unit direction | three smooth values: 9 columns, and the x y z columns alone beside them"""
    for sub in ("xyz9", "xyz3"):
        os.makedirs(os.path.join(folder, sub))
    for k, n in enumerate(sizes):
        p = synth_patches(1, n, seed=100 + k, surface=True)[0].numpy().astype(np.float64)
        d = p - p.mean(axis=0)
        rows = np.concatenate([p, d / np.linalg.norm(d, axis=1, keepdims=True), np.abs(p)], axis=1)
        np.savetxt(os.path.join(folder, "xyz9", f"cloud{k:03d}.xyz"), rows, fmt="%.6f")
        np.savetxt(os.path.join(folder, "xyz3", f"cloud{k:03d}.xyz"), p, fmt="%.6f")


box = "?"
with tempfile.TemporaryDirectory() as tmp:
    settings = [("dense", [5000] * 32, 0, 240)] if "--skip-dense" not in args else []
    if "--skip-tiled" not in args:
        settings.append(("tiled", [tiled_points], 4096, 900))
    for name, sizes, tile_points, limit in settings:
        write_scans(os.path.join(tmp, name), sizes)
        times = {leg: [] for leg in FLAGS}
        for rnd in range(2):
            for leg in FLAGS:                                      # alternated: none, attributes, normals, none, ...
                dst = os.path.join(tmp, f"out_{name}_{leg}_{rnd}")
                os.makedirs(dst)
                src = os.path.join(tmp, name, "xyz9" if leg == "attributes" else "xyz3")
                try:
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", src, dst, leg, str(tile_points), attr_search],
                                         capture_output=True, text=True, timeout=limit)
                except subprocess.TimeoutExpired:
                    say(f"{name} / {leg}: TIMED OUT after {limit} s - stopping")
                    finish(False)
                got = {l.split()[0]: l.split(None, 1)[1] for l in out.stdout.splitlines()
                       if l.split() and l.split()[0] in ("FIRST", "ELAPSED", "BOX")}
                if out.returncode != 0 or "ELAPSED" not in got:
                    say(f"{name} / {leg}: FAILED (exit {out.returncode}) - stopping\n{out.stderr[-800:]}")
                    finish(False)
                box = got.get("BOX", box)
                times[leg].append(float(got["ELAPSED"]))
                record["legs"].append({"setting": name, "leg": leg, "round": rnd, "seconds": float(got["ELAPSED"]),
                                       "first_call_seconds": float(got["FIRST"]), "files": len(sizes), "points": sizes[0]})
                say(f"{name:5s} round {rnd} {leg:10s}: {float(got['ELAPSED']):8.3f} s = {float(got['ELAPSED']) / len(sizes) * 1e3:9.2f} ms "
                    f"per cloud (first call of the process {float(got['FIRST']):.3f} s)")
        base = min(times["none"])
        for leg in ("attributes", "normals"):
            say(f"{name:5s} {leg:10s} adds {(min(times[leg]) - base) / len(sizes) * 1e3:9.2f} ms per cloud to {base / len(sizes) * 1e3:.2f} "
                f"(best of two rounds each; {len(sizes)} clouds of {sizes[0]} points)")
    for n in (5000, tiled_points) if attr_search == "brute" and "--skip-share" not in args else ():
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--share", str(n), str(sample)], capture_output=True,
                                 text=True, timeout=600)
        except subprocess.TimeoutExpired:
            say(f"share, {n} points: TIMED OUT - stopping")
            finish(False)
        got = [l[7:] for l in out.stdout.splitlines() if l.startswith("RESULT ")]
        if out.returncode != 0 or not got:
            say(f"share, {n} points: FAILED (exit {out.returncode}) - stopping\n{out.stderr[-800:]}")
            finish(False)
        r = json.loads(got[0])
        record["share"].append(r)
        u = r["us_per_point"]
        say(f"share, cloud of {n} points ({r['outputs']} outputs, timed on {r['sample']}): per output point, attributes = search "
            f"{u['attributes_search']:.2f} us + blend {u['attributes_blend']:.4f} us (search {u['attributes_search'] / (u['attributes_search'] + u['attributes_blend']):.2%}); "
            f"normals = search {u['normals_search']:.2f} us + PCA {u['normals_pca']:.4f} us "
            f"(search {u['normals_search'] / (u['normals_search'] + u['normals_pca']):.2%}); whole cloud at these rates: attributes "
            f"{(u['attributes_search'] + u['attributes_blend']) * r['outputs'] * 1e-6:.2f} s, normals {(u['normals_search'] + u['normals_pca']) * r['outputs'] * 1e-6:.2f} s")
    say(f"box: {box}   commit: {commit}   attr_search: {attr_search}")
finish(True)
