"""Time one differentiable CNF flow block (PointInterpFlow.flow_block: taped forward, backward, pf_cnf_rhs_vjp alone) beside the
inference integration of the same block and shape, for both reverse sweeps (one pf_cnf_tape_vjp launch / pf_cnf_rhs_vjp per
evaluation) and both step-size controllers (device / host).

  python tools/time_cnf_block_grad.py --out profiles/cnf_grad/time_cnf_block_grad.json [--parent PARENT.json --parent-commit HASH]

--parent: the result file the PARENT commit's copy of this tool wrote on the same box in the same session; it is embedded and the
text file sets the default path's forward + backward beside it.

Block 5 of the bench workload's weights (weights.CNF_PU1K_DYNAMICS / CNF_PU1K_END_TIMES: the block with the longest integration) at
the training shape, 32 patches x 256 points: forward direction at R = 1 (8 192 rows) and reversed at R = 4 (32 768 rows).  Every
shape is warmed up; host clock around work that ends in a device synchronise, median (min .. max) of the repeats; the kernel
alone between HIP events around a batch of launches.  Recorded, not gated: no threshold.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCK, B, N = 5, 32, 256
CASES = (("forward_R1", 1, False), ("reversed_R4", 4, True))
CONFIGS = (("fused", "device"), ("per_eval", "device"), ("fused", "host"), ("per_eval", "host"))      # the first: flow_block's default


def spread(times):
    return {"ms_median": float(np.median(times)), "ms_min": float(np.min(times)), "ms_max": float(np.max(times)), "repeats": len(times)}


def run(a):
    import torch
    from puflow_amd.cnf import PointInterpFlow, _BlockTapeEngine
    from puflow_amd.packing import CNF_CTX, CNF_GRAD
    from puflow_amd.weights import CNF_PU1K_DYNAMICS, CNF_PU1K_END_TIMES, synth_cnf_state_dict

    dev = "cuda:0"
    sd = synth_cnf_state_dict(2021, dynamics=CNF_PU1K_DYNAMICS, end_times=CNF_PU1K_END_TIMES)
    net = PointInterpFlow(3)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    cd = sd[f"flow_blocks.{BLOCK}.cnf.odefunc.diffeq.layers.0._hyper_gate.weight"].shape[1] - 1
    T = B * N

    def timed(fn, reps):
        fn()                                                          # warm-up of this shape
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
        return spread(out)

    res = {"device": torch.cuda.get_device_name(0), "block": BLOCK, "points": T, "cases": []}
    for name, R, reverse in CASES:
        g = torch.Generator().manual_seed(R)
        rows = T * R
        x = (torch.randn(rows, 3, generator=g) * 0.8).to(dev)
        c = (torch.randn(T, cd, generator=g) * 0.7).to(dev)
        e = torch.randn(T, 3, generator=g).to(dev)
        gx = torch.randn(rows, 3, generator=g).to(dev)
        state = {}
        paths = {}
        for sweep, controller in CONFIGS:
            def forward():
                xr, cr = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
                ox, ol = net.flow_block(BLOCK, xr, cr, e, R, reverse, sweep=sweep, controller=controller)
                state["loss"] = (ox * gx).sum() + ol.sum()

            def forward_backward():
                forward()
                state["loss"].backward()

            f = timed(forward, a.reps)
            n = len(net.last_block_steps)
            fb = timed(forward_backward, a.reps)
            paths[f"{sweep}/{controller}"] = {"sweep": sweep, "controller": controller, "accepted_steps": n, "taped_forward": f,
                                              "forward_plus_backward": fb, "backward_ms_median": fb["ms_median"] - f["ms_median"]}
        default = paths["/".join(CONFIGS[0])]
        fwd, both, steps = default["taped_forward"], default["forward_plus_backward"], default["accepted_steps"]
        # the inference integration of the same block and shape (device-side controller, dense output at the end time)
        eng = net._engine(4)
        ctx = eng.context(BLOCK, c)
        d0c = torch.empty(1, dtype=torch.float64, device=dev)
        eng.context_norm(c, d0c)
        infer = timed(lambda: eng.integrate(BLOCK, x, ctx, e, R, reverse, c.numel() * R, d0c, extra_scale=float(R)), a.reps)
        attempts = int(eng.last_attempts)
        # the VJP kernel (+ its slab reduction) alone
        te = _BlockTapeEngine({k: v for k, v in sd.items() if k.startswith(f"flow_blocks.{BLOCK}.")}, BLOCK, torch.device(dev))
        y = torch.cat([x, torch.zeros(rows, 1, device=dev)], dim=1).contiguous()
        kbar = torch.randn(rows, 4, device=dev)
        ybar, ctxbar, grad = torch.empty_like(y), torch.zeros(T, CNF_CTX, device=dev), torch.zeros(CNF_GRAD, device=dev)
        kout = torch.empty_like(y)
        sgn = -1.0 if reverse else 1.0

        def batch(fn):
            fn()
            torch.cuda.synchronize()
            times = []
            for _ in range(a.reps):
                s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s0.record()
                for _ in range(a.launches):
                    fn()
                s1.record()
                torch.cuda.synchronize()
                times.append(s0.elapsed_time(s1) / a.launches)
            return spread(times)

        vjp = batch(lambda: te.vjp(BLOCK, y, kbar, 0.3, sgn, ctx, e, ybar, ctxbar, grad, rows, R))
        rhs = batch(lambda: te._rhs(BLOCK, y, y, [], 0.0, 0.3, sgn, ctx, e, kout, None, rows, R))
        row = {"case": name, "rows": rows, "R": R, "reverse": reverse, "accepted_steps": steps, "taped_forward": fwd,
               "forward_plus_backward": both, "backward_ms_median": both["ms_median"] - fwd["ms_median"],
               "inference_integrate": infer, "inference_attempts": attempts, "vjp_launch": vjp, "rhs_launch": rhs,
               "launches_per_batch": a.launches, "paths": paths}
        res["cases"].append(row)
        print(json.dumps(row), flush=True)
    return res


def text(res):
    lines = [f"CNF block {res['block']} gradient, {res['points']} points; {res['device']}; ms: median (min .. max) of the repeats after a warm-up"]
    for r in res["cases"]:
        lines.append(f"{r['case']}: {r['rows']} rows, {r['accepted_steps']} accepted steps (inference integration: {r['inference_attempts']} attempts)")
        for k in ("taped_forward", "forward_plus_backward", "inference_integrate", "vjp_launch", "rhs_launch"):
            t = r[k]
            lines.append(f"  {k:22s} {t['ms_median']:10.3f} ({t['ms_min']:.3f} .. {t['ms_max']:.3f}) x{t['repeats']}")
        lines.append(f"  {'backward (difference)':22s} {r['backward_ms_median']:10.3f}")
        for name, p in r.get("paths", {}).items():
            f, fb = p["taped_forward"], p["forward_plus_backward"]
            lines.append(f"  sweep/controller {name:16s} {p['accepted_steps']:3d} steps  forward {f['ms_median']:8.3f} ({f['ms_min']:.3f} .. {f['ms_max']:.3f})"
                         f"  forward+backward {fb['ms_median']:8.3f} ({fb['ms_min']:.3f} .. {fb['ms_max']:.3f})  backward {p['backward_ms_median']:8.3f}")
    par = res.get("parent")
    if par:
        lines.append(f"parent commit {par['commit']} (its own copy of this tool, same box, same session):")
        for r, q in zip(res["cases"], par["cases"]):
            n, o = r["forward_plus_backward"], q["forward_plus_backward"]
            spread = max(n["ms_max"] - n["ms_min"], o["ms_max"] - o["ms_min"])
            lines.append(f"  {r['case']}: forward+backward parent {o['ms_median']:.3f} ({o['ms_min']:.3f} .. {o['ms_max']:.3f}), "
                         f"{q['accepted_steps']} steps -> default path {n['ms_median']:.3f} ({n['ms_min']:.3f} .. {n['ms_max']:.3f}), "
                         f"{r['accepted_steps']} steps: gain {o['ms_median'] - n['ms_median']:.3f} ms against a spread of {spread:.3f} ms; "
                         f"taped forward {q['taped_forward']['ms_median']:.3f} -> {r['taped_forward']['ms_median']:.3f}, "
                         f"vjp_launch {q['vjp_launch']['ms_median']:.3f} -> {r['vjp_launch']['ms_median']:.3f}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--parent", help="result file of the parent commit's run of this tool")
    ap.add_argument("--parent-commit", default="?")
    a = ap.parse_args()
    res = run(a)
    if a.parent:
        with open(a.parent) as fh:
            res["parent"] = {"commit": a.parent_commit, "cases": json.load(fh)["cases"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.splitext(a.out)[0] + ".txt", "w") as fh:
        fh.write(text(res))


if __name__ == "__main__":
    main()
