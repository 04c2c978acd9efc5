#!/usr/bin/env python3
"""Wall time of the .xyz CLI per cloud when the files of a directory differ in size, in one call on one box:
  (a) 32 files of 5000 points, default cloud_batch                (dense batched passes: the figure the README quotes)
  (b) 32 files of 4000 ... 6000 points, the same total, default   (ragged passes)
  (c) the directory of (b) with --cloud_batch 1                   (one file per pass: what a size change forced before ragged
                                                                   passes existed)
Every configuration runs in a FRESH process under its own time limit and calls upsampling() twice; the second call (weights
planned, allocator warm) is the figure, the first is printed beside it.  A configuration that fails ends the run: nothing
else is started on the GPU after it.  (b) and (c) must write the same bytes.
  python tools/time_cli_ragged.py [--out FILE] [--commit ID]"""
import filecmp, os, socket, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if len(sys.argv) > 1 and sys.argv[1] == "--child":
    src, dst, cb = sys.argv[2], sys.argv[3], (None if sys.argv[4] == "default" else int(sys.argv[4]))
    import torch
    from puflow_amd import upsample as U
    from puflow_amd.weights import synth_state_dict
    sd = synth_state_dict(2021)
    torch.zeros(1, device="cuda"); torch.cuda.synchronize()           # GPU context
    paths = sorted(os.path.join(src, f) for f in os.listdir(src))
    for tag in ("FIRST", "ELAPSED"):
        t0 = time.perf_counter()
        U.upsampling(paths, dst, None, up_ratio=4, num_outlier=24, num_patch=256, seed=2021, state_dict=sd, cloud_batch=cb)
        print("%s %.6f" % (tag, time.perf_counter() - t0), flush=True)
    print("BOX %s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0)), flush=True)
    sys.exit(0)

import numpy as np
from puflow_amd.weights import synth_patches

args = sys.argv[1:]
out_path = args[args.index("--out") + 1] if "--out" in args else None
commit = args[args.index("--commit") + 1] if "--commit" in args else "unknown"
F = 32
mixed = [4000 + 500 * (k % 5) for k in range(F - 2)] + [4750, 5250]
assert sum(mixed) == 5000 * F
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


with tempfile.TemporaryDirectory() as tmp:
    for tag, sizes in (("equal", [5000] * F), ("mixed", mixed)):
        os.makedirs(os.path.join(tmp, tag))
        for k, n in enumerate(sizes):
            np.savetxt(os.path.join(tmp, tag, f"cloud{k:03d}.xyz"), synth_patches(1, n, seed=100 + k)[0].numpy(), fmt="%.6f")
    res, box = {}, "?"
    for key, tag, cb, what in (("a", "equal", "default", "32 files of 5000 points, default cloud_batch (dense passes)"),
                               ("b", "mixed", "default", "32 files of 4000..6000 points, same total, default cloud_batch (ragged passes)"),
                               ("c", "mixed", "1", "the same mixed directory, --cloud_batch 1 (one file per pass)")):
        dst = os.path.join(tmp, "out_" + key)
        os.makedirs(dst)
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.join(tmp, tag), dst, cb],
                                 capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired:
            say(f"({key}) TIMED OUT - stopping")
            break
        got = {l.split()[0]: l.split(None, 1)[1] for l in out.stdout.splitlines() if l.split() and l.split()[0] in ("FIRST", "ELAPSED", "BOX")}
        if out.returncode != 0 or "ELAPSED" not in got:
            say(f"({key}) FAILED (exit {out.returncode}) - stopping\n{out.stderr[-800:]}")
            break
        box = got.get("BOX", box)
        res[key] = float(got["ELAPSED"])
        say(f"({key}) {what}: {res[key]:6.3f} s = {res[key] / F * 1e3:6.2f} ms per cloud (first call of the process: {float(got['FIRST']) / F * 1e3:6.2f})")
    if len(res) == 3:
        names = sorted(os.listdir(os.path.join(tmp, "mixed")))
        match, mismatch, errors = filecmp.cmpfiles(os.path.join(tmp, "out_b"), os.path.join(tmp, "out_c"), names, shallow=False)
        say(f"(b) and (c) wrote the same bytes for {len(match)} of {len(names)} files")
        say(f"(b) / (c) = {res['b'] / res['c']:.3f}   (b) / (a) = {res['b'] / res['a']:.3f}")
    say(f"box: {box}   commit: {commit}")
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if len(res) == 3 else 1)
