#!/usr/bin/env python3
"""Wall time of PatchHelper.upsample_tiled on synthetic surface clouds, per stage, in one call on one box:
  16 384 points: tile_points = 4096 against the untiled pipeline (whose FPS merge of 327 680 candidates leaves the cooperative
                 kernel: the cliff) - legs alternated tiled / untiled / tiled, the untiled one measured ONCE under a generous limit
  65 536 and 262 144 points: tiled only
Every leg runs in a FRESH process under its own time limit; a tiled leg runs the cloud twice and reports the second run (weights
planned, allocator warm) with its stages (synchronised at every stage boundary: their sum is a little above the unsynchronised
total printed beside it).  A leg that fails ends the run: nothing else is started on the GPU after it.
  python tools/time_tiled.py [--out-dir profiles/tiled] [--commit ID]"""
import json, os, socket, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if len(sys.argv) > 1 and sys.argv[1] == "--child":
    n, tile_points = int(sys.argv[2]), int(sys.argv[3])
    import torch
    from puflow_amd.interpflow import PointInterpFlow
    from puflow_amd.patch import PatchHelper
    from puflow_amd.weights import synth_patches, synth_state_dict
    net = PointInterpFlow(3)
    net.load_state_dict(synth_state_dict(2021))
    net.set_to_initialized_state()
    net = net.to("cuda:0").eval()
    pc = synth_patches(1, n, seed=5, surface=True)[0].to("cuda:0")
    helper, npoint = PatchHelper(256, 4), 4 * n + 24
    res = {"n": n, "tile_points": tile_points, "box": "%s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0))}
    with torch.no_grad():
        helper.upsample(net, pc[None, :2048].contiguous(), 8216, upratio=4)           # library load, weight plan
        torch.cuda.synchronize()
        if tile_points == 0:                                                            # untiled: once
            t0 = time.perf_counter()
            out = helper.upsample(net, pc[None], npoint, upratio=4)[0]
            torch.cuda.synchronize()
            res["total_s"] = time.perf_counter() - t0
        else:
            for run in ("first", "second"):
                t0 = time.perf_counter()
                out = helper.upsample_tiled(net, pc, npoint, upratio=4, tile_points=tile_points, tiles_per_pass=16)
                torch.cuda.synchronize()
                res["total_s" if run == "second" else "first_s"] = time.perf_counter() - t0
            stages, last = {}, [time.perf_counter()]

            def stage(name):
                torch.cuda.synchronize()
                now = time.perf_counter()
                stages[name] = stages.get(name, 0.0) + now - last[0]
                last[0] = now

            torch.cuda.synchronize()
            last[0] = time.perf_counter()
            out, st = helper.upsample_tiled(net, pc, npoint, upratio=4, tile_points=tile_points, tiles_per_pass=16,
                                            return_stats=True, _stage=stage)
            res.update(stages=stages, tiles=st["tiles"], colours=st["colours"], h=st["h"], overhead=sum(st["working"]) / n,
                       min_r2=float(st["r2"].min()), candidates_max=max(st["candidates"]), context_max=max(st["context"]))
        assert tuple(out.shape) == (npoint, 3) and bool(torch.isfinite(out).all())
    print("RESULT " + json.dumps(res), flush=True)
    sys.exit(0)

args = sys.argv[1:]
out_dir = args[args.index("--out-dir") + 1] if "--out-dir" in args else os.path.join(ROOT, "profiles", "tiled")
commit = args[args.index("--commit") + 1] if "--commit" in args else "unknown"
lines, results = [], []


def say(s):
    print(s, flush=True)
    lines.append(s)


LEGS = [(16384, 4096, 300), (16384, 0, 360), (16384, 4096, 300), (65536, 4096, 400), (262144, 4096, 600)]
ok = True
for n, tp, limit in LEGS:
    what = f"{n} points, " + (f"tile_points {tp}" if tp else "untiled (measured once)")
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(tp)], capture_output=True, text=True,
                             timeout=limit)
    except subprocess.TimeoutExpired:
        say(f"{what}: TIMED OUT after {limit} s - stopping")
        ok = False
        break
    got = [l[7:] for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    if out.returncode != 0 or not got:
        say(f"{what}: FAILED (exit {out.returncode}) - stopping\n{out.stderr[-1500:]}")
        ok = False
        break
    r = json.loads(got[0])
    results.append(r)
    if tp:
        say(f"{what}: {r['total_s']:.3f} s (first run of the process {r['first_s']:.3f} s); {r['tiles']} tiles, {r['colours']} colours, "
            f"h {r['h']:.4f}, network overhead sum|working set| / N = {r['overhead']:.2f}, largest tile {r['candidates_max']} "
            f"candidates, largest context {r['context_max']}, min r2 {r['min_r2']:.3e}")
        say("    stages (synchronised): " + ", ".join(f"{k} {v * 1e3:.1f} ms" for k, v in r["stages"].items()))
    else:
        say(f"{what}: {r['total_s']:.3f} s")
if results:
    say(f"box: {results[-1]['box']}   commit: {commit}")
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "time_tiled.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
with open(os.path.join(out_dir, "time_tiled.json"), "w") as f:
    json.dump({"commit": commit, "legs": results}, f, indent=1)
sys.exit(0 if ok else 1)
