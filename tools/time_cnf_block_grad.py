"""Time one differentiable CNF flow block (PointInterpFlow.flow_block: taped forward, backward, pf_cnf_rhs_vjp alone) beside the
inference integration of the same block and shape.

  python tools/time_cnf_block_grad.py --out profiles/cnf_grad/time_cnf_block_grad.json

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

        def forward():
            xr, cr = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
            ox, ol = net.flow_block(BLOCK, xr, cr, e, R, reverse)
            state["loss"] = (ox * gx).sum() + ol.sum()

        def backward():
            state["loss"].backward()

        def forward_backward():
            forward()
            backward()

        fwd = timed(forward, a.reps)
        steps = len(net.last_block_steps)
        both = timed(forward_backward, a.reps)
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
               "launches_per_batch": a.launches}
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
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    res = run(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.splitext(a.out)[0] + ".txt", "w") as fh:
        fh.write(text(res))


if __name__ == "__main__":
    main()
