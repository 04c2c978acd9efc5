#!/usr/bin/env python3
"""What orient="propagate" adds to estimate_normals(search="grid") at K = 16, by device events, at the shapes DESIGN.md 8e reports:
  32 clouds of 20 000 points (one dense call)   |   one cloud of 16 384   |   of 65 536   |   of 262 144 points
and what --normals_orient propagate adds to the .xyz CLI beside --estimate_normals 16 --attr_search grid (32 files of 5000 points,
tools/time_attributes.py's dense setting; second upsampling() call of the process).
The two legs - orient="point" and orient="propagate" - alternate, --rounds rounds, every leg in a FRESH process under its own time
limit; inside a process each shape is called --reps times after one untimed call and its figure is the median.  The propagate
leg also times pf_normals_orient alone on the lists the PCA used, and checks on every shape that scrambled input signs give the
same bits.  A leg that fails or runs out of time ends the run: nothing else is started on the GPU after it.
  python tools/time_normals_orient.py [--out-dir profiles/normals_orient] [--commit ID] [--rounds 3] [--reps 5] [--skip-cli]"""
import json, os, socket, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = (("32 clouds of 20 000", 32, 20000), ("one cloud of 16 384", 1, 16384), ("one cloud of 65 536", 1, 65536),
          ("one cloud of 262 144", 1, 262144))
K = 16

if len(sys.argv) > 1 and sys.argv[1] == "--child":
    leg, reps = sys.argv[2], int(sys.argv[3])
    import torch
    from puflow_amd import attributes as A, ops
    from puflow_amd.weights import synth_patches

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = fn(); b.record(); torch.cuda.synchronize()
        return out, a.elapsed_time(b)

    def median(fn):
        fn(); torch.cuda.synchronize()
        ms = sorted(event_ms(fn)[1] for _ in range(reps))
        return ms[len(ms) // 2], ms[-1] - ms[0]

    torch.zeros(1, device="cuda"); torch.cuda.synchronize()
    for name, b, n in SHAPES:
        pts = synth_patches(b, n, seed=5, surface=True).to("cuda:0")                     # [b,n,3]
        row = {"shape": name, "clouds": b, "points": n, "leg": leg}
        row["median_ms"], row["spread_ms"] = median(lambda: A.estimate_normals(pts, K, search="grid", orient=leg))
        if leg == "propagate":
            idx, _ = ops.knn_grid(pts, pts, K)
            normal, _ = ops.normals_pca(pts, idx)
            row["orient_alone_ms"], row["orient_alone_spread_ms"] = median(lambda: ops.normals_orient(pts, normal, idx))
            out, comp = ops.normals_orient(pts, normal, idx)
            sign = torch.randint(0, 2, normal.shape[:2], device="cuda:0").float()[..., None] * 2 - 1
            again, comp2 = ops.normals_orient(pts, normal * sign, idx)
            row["sign_independent"] = bool(torch.equal(out.view(torch.int32), again.view(torch.int32)) and torch.equal(comp, comp2))
            row["components_per_cloud"] = sum(int(torch.unique(c).numel()) for c in comp) / b
            row["rows_the_point_rule_has_opposed"] = int(((out * normal).sum(dim=-1) < 0).sum())
        print("ROW " + json.dumps(row), flush=True)
    print("BOX %s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0)), flush=True)
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "--cli-child":
    src, dst, leg = sys.argv[2], sys.argv[3], sys.argv[4]
    import torch
    from puflow_amd import upsample as U
    from puflow_amd.weights import synth_state_dict
    sd = synth_state_dict(2021)
    torch.zeros(1, device="cuda"); torch.cuda.synchronize()
    paths = sorted(os.path.join(src, f) for f in os.listdir(src))
    for tag in ("FIRST", "ELAPSED"):
        t0 = time.perf_counter()
        U.upsampling(paths, dst, None, up_ratio=4, num_outlier=24, num_patch=256, seed=2021, state_dict=sd, estimate_normals=K,
                     attr_search="grid", normals_orient=leg)
        print("%s %.6f" % (tag, time.perf_counter() - t0), flush=True)
    sys.exit(0)

args = sys.argv[1:]
out_dir = args[args.index("--out-dir") + 1] if "--out-dir" in args else os.path.join(ROOT, "profiles", "normals_orient")
commit = args[args.index("--commit") + 1] if "--commit" in args else "unknown"
rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 3
reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
lines, record = [], {"commit": commit, "k": K, "rounds": rounds, "reps": reps, "rows": [], "cli": []}
LEGS = ("point", "propagate")


def say(s):
    print(s, flush=True)
    lines.append(s)


def finish(ok):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "time_normals_orient.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(out_dir, "time_normals_orient.json"), "w") as f:
        json.dump(record, f, indent=1)
    sys.exit(0 if ok else 1)


def child(argv, limit, what):
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        say(f"{what}: TIMED OUT after {limit} s - stopping")
        finish(False)
    if out.returncode != 0:
        say(f"{what}: FAILED (exit {out.returncode}) - stopping\n{out.stderr[-800:]}")
        finish(False)
    return out.stdout.splitlines()


box, ok = "?", True
for rnd in range(rounds):
    for leg in LEGS:                                                   # alternated: point, propagate, point, ...
        for line in child(["--child", leg, str(reps)], 300, f"round {rnd} / {leg}"):
            if line.startswith("ROW "):
                row = dict(json.loads(line[4:]), round=rnd)
                record["rows"].append(row)
                text = f"round {rnd} {leg:9s} {row['shape']:22s}: {row['median_ms']:9.3f} ms (spread {row['spread_ms']:.3f})"
                if leg == "propagate":
                    ok = ok and row["sign_independent"]
                    text += f" | pf_normals_orient alone {row['orient_alone_ms']:.3f} ms (spread {row['orient_alone_spread_ms']:.3f}); " \
                            f"{row['components_per_cloud']:.1f} components per cloud; rows the point rule had the other way " \
                            f"{row['rows_the_point_rule_has_opposed']}; same bits from scrambled signs: {row['sign_independent']}"
                say(text)
            elif line.startswith("BOX "):
                box = line[4:]
for name, _, _ in SHAPES:
    med = {leg: sorted(r["median_ms"] for r in record["rows"] if r["shape"] == name and r["leg"] == leg) for leg in LEGS}
    p, q = med["point"][len(med["point"]) // 2], med["propagate"][len(med["propagate"]) // 2]
    spread = max(med["point"][-1] - med["point"][0], med["propagate"][-1] - med["propagate"][0])
    say(f"{name:22s}: search + PCA {p:9.3f} ms, with propagation {q:9.3f} ms: +{q - p:.3f} ms = x{q / p:.2f} (medians of {rounds} "
        f"processes; largest spread between processes {spread:.3f} ms)")
if "--skip-cli" not in args:
    import numpy as np
    from puflow_amd.weights import synth_patches
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "in"))
        for k in range(32):
            np.savetxt(os.path.join(tmp, "in", f"cloud{k:03d}.xyz"), synth_patches(1, 5000, seed=100 + k, surface=True)[0].numpy().astype(np.float64), fmt="%.6f")
        times = {leg: [] for leg in LEGS}
        for rnd in range(2):
            for leg in LEGS:
                dst = os.path.join(tmp, f"out_{leg}_{rnd}")
                os.makedirs(dst)
                got = {l.split()[0]: float(l.split()[1]) for l in child(["--cli-child", os.path.join(tmp, "in"), dst, leg], 240, f"cli round {rnd} / {leg}")
                       if l.split() and l.split()[0] in ("FIRST", "ELAPSED")}
                times[leg].append(got["ELAPSED"])
                record["cli"].append({"leg": leg, "round": rnd, "seconds": got["ELAPSED"], "first_call_seconds": got["FIRST"], "files": 32, "points": 5000})
                say(f"cli round {rnd} --estimate_normals 16 --attr_search grid --normals_orient {leg:9s}: {got['ELAPSED'] / 32 * 1e3:8.2f} ms per cloud "
                    f"(first call of the process {got['FIRST']:.3f} s)")
        say(f"cli: --normals_orient propagate adds {(min(times['propagate']) - min(times['point'])) / 32 * 1e3:.2f} ms per cloud to "
            f"{min(times['point']) / 32 * 1e3:.2f} (best of two rounds each; 32 files of 5000 points)")
say(f"box: {box}   commit: {commit}")
finish(ok)
