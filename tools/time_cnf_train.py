"""Time the continuous model's training step (cnf.PointInterpFlow in train() mode) at the training shape, 32 patches x 256 -> 1024
points, with the bench workload's weights (weights.CNF_PU1K_DYNAMICS / CNF_PU1K_END_TIMES):

  (a) the eager training step: TrainerModule.train_step (forward, loss with EMD, backward, clip + Adam);
  (b) its flow part alone: cnf.flow_train on fixed conditioning features / logits, forward + backward;
  (c) the same twelve integrations as twelve `flow_block(..., pack="host")` calls, forward + backward: the path the code had
      before the device-side packer and the whole-model forward (every call packs on the host and runs its own context GEMM);
  (d) one taped forward of a block with pack="device" against pack="host" (block 5 at R = 1 and reversed at R = 4).

  python tools/time_cnf_train.py --out profiles/cnf_train/time_cnf_train.json

--legs: the deferred controller and the captured step against that eager step, three legs on one box, alternated:
  (a) the eager step as above (thirteen host reads per step), (b) the eager step with cfg.cnf_deferred (one read), (c) the captured
  step (TrainerModule.graphed_train_step with cfg.cnf_deferred: one replay, a read every CHECK_EVERY replays).
Five rounds a, b, c, a, b, c, ...; a run is --steps steps, each timed by the host clock around the step and a device synchronise;
per run the median step time and the spread (max - min) of its steps; the three modules start from the same weights and take the
same number of optimisation steps (--lr 0, the default, holds the weights: the step then costs the same in every run).  Between
the runs the captured step is checked and, when stale, captured anew, as train.fit does (untimed, counted).  For (b) and (c) also the step attempts enqueued per step that returned at once because their
integration was done (budget - the largest count of attempts the sticky table saw; cnf.PointInterpFlow.train_log_stats).

  python tools/time_cnf_train.py --legs --out profiles/cnf_graph/legs.json

Every case is warmed up; host clock around work that ends in a device synchronise; median (min .. max) of the repeats.  The
trainer runs with emd_workgroups = 1 (no grid-barrier kernels: safe on a device other processes use).  Recorded, not gated."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, N, R = 32, 256, 4
CDS = [32, 64, 128, 128, 128, 128]


def spread(times):
    return {"ms_median": float(np.median(times)), "ms_min": float(np.min(times)), "ms_max": float(np.max(times)), "repeats": len(times)}


def run(a):
    import torch
    from puflow_amd import cnf, ops, train_ops
    from puflow_amd.trainer import TrainerModule, default_cfg
    from puflow_amd.weights import CNF_PU1K_DYNAMICS, CNF_PU1K_END_TIMES, synth_cnf_state_dict, synth_patches

    dev = "cuda:0"
    sd = synth_cnf_state_dict(2021, dynamics=CNF_PU1K_DYNAMICS, end_times=CNF_PU1K_END_TIMES)
    T = B * N

    def timed(fn, reps):
        fn()                                                          # warm-up of this case
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
        return spread(out)

    res = {"device": torch.cuda.get_device_name(0), "shape": [B, N, R]}
    dense = synth_patches(B, N * R, seed=2021).to(dev)
    sparse = dense[:, ::R].contiguous()
    g = torch.Generator().manual_seed(1)
    noise = [torch.randn(B, N, 3, generator=g).to(dev) for _ in range(6)]

    # ---- (a) the eager step
    torch.manual_seed(0)
    m = TrainerModule(default_cfg(model="continuous", emd_workgroups=1))
    m.network.load_state_dict(sd, strict=True)
    m = m.to(dev)
    opt = m.configure_optimizers()["optimizer"]
    res["a_train_step"] = timed(lambda: m.train_step((sparse, dense), opt), a.reps)
    res["a_steps_per_integration"] = [len(s) for s in m.network.last_train_steps]

    # ---- (b) the flow part alone, (c) twelve flow_block calls on the same inputs
    net = cnf.PointInterpFlow(3)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()
    cs = [(torch.randn(B, N, cd, generator=g) * 0.7).to(dev) for cd in CDS]
    w = torch.randn(T * 8, 32, generator=g).to(dev)
    gx = torch.randn(B, N * R, 3, generator=g).to(dev)
    idx16, _ = ops.knn_idx32(sparse, sparse, 16)
    idx8 = idx16[..., :8].contiguous()
    train_ops.set_deterministic(False)

    def leaves():
        return [c.clone().requires_grad_(True) for c in cs], w.clone().requires_grad_(True)

    def flow_part():
        csl, wl = leaves()
        x, logp = cnf.flow_train(net, sparse, R, csl, (None, wl, None, None, idx8), noise)
        (0.5 * logp + (x * gx).sum()).backward()

    def twelve_calls(pack):
        csl, wl = leaves()
        p, ldj = sparse.reshape(T, 3), 0.0
        for i in range(6):
            p, dl = net.flow_block(i, p, csl[i].reshape(T, -1), noise[i].reshape(T, 3), 1, False, pack=pack)
            ldj = ldj + dl.sum()
        z = p.view(B, N, 3)
        u = train_ops.InterpWsumFn.apply(wl.view(T, 8, -1), z, idx8, R, None).reshape(T * R, 3)
        for i in reversed(range(6)):
            u, _ = net.flow_block(i, u, csl[i].reshape(T, -1), noise[i].reshape(T, 3), R, True, pack=pack)
        ((u.view(B, N * R, 3) * gx).sum() + 0.5 * ldj + (z ** 2).sum()).backward()

    res["b_flow_part"] = timed(flow_part, a.reps)
    res["b_steps_per_integration"] = [len(s) for s in net.last_train_steps]
    res["c_twelve_flow_block_calls_pack_host"] = timed(lambda: twelve_calls("host"), a.reps)
    res["c_twelve_flow_block_calls_pack_device"] = timed(lambda: twelve_calls("device"), a.reps)

    # ---- (d) one taped forward, device against host packing
    res["d_taped_forward"] = []
    for name, Rr, reverse in (("forward_R1", 1, False), ("reversed_R4", 4, True)):
        x = (torch.randn(T * Rr, 3, generator=g) * 0.8).to(dev)
        c, e = cs[5].reshape(T, -1), noise[5].reshape(T, 3)
        row = {"case": name, "block": 5, "rows": T * Rr}
        for pack in ("device", "host"):
            def fwd():
                with torch.no_grad():
                    net.flow_block(5, x, c, e, Rr, reverse, pack=pack)
            row[pack] = timed(fwd, a.reps)
        row["accepted_steps"] = len(net.last_block_steps)
        res["d_taped_forward"].append(row)
    return res


def run_legs(a):
    import torch
    from puflow_amd.trainer import TrainerModule, default_cfg
    from puflow_amd.weights import CNF_PU1K_DYNAMICS, CNF_PU1K_END_TIMES, synth_cnf_state_dict, synth_patches

    dev = "cuda:0"
    sd = synth_cnf_state_dict(2021, dynamics=CNF_PU1K_DYNAMICS, end_times=CNF_PU1K_END_TIMES)
    dense = synth_patches(B, N * R, seed=2021).to(dev)
    sparse = dense[:, ::R].contiguous()
    batch = (sparse, dense)

    def module(deferred):
        torch.manual_seed(0)
        m = TrainerModule(default_cfg(model="continuous", emd_workgroups=1, cnf_deferred=deferred, learning_rate=a.lr))
        m.network.load_state_dict(sd, strict=True)
        m = m.to(dev)
        return m, m.configure_optimizers()["optimizer"]

    ma, oa = module(False)
    mb, ob = module(True)
    mc, oc = module(True)
    for _ in range(2):                                                # the warm-up steps the capture takes, for all three
        ma.train_step(batch, oa)
        mb.train_step(batch, ob)
    graph = mc.graphed_train_step(batch, oc, warmup=2)
    cap = {"graph": graph, "captures": 1, "void": 0, "nan": 0}
    legs = {"a_eager": lambda: ma.train_step(batch, oa), "b_eager_deferred": lambda: mb.train_step(batch, ob),
            "c_captured": lambda: cap["graph"](batch)}
    res = {"device": torch.cuda.get_device_name(0), "shape": [B, N, R], "steps_per_run": a.steps, "rounds": 5, "learning_rate": a.lr,
           "runs": {k: [] for k in legs}}
    for _ in range(5):
        for name, fn in legs.items():
            if name == "c_captured":                                  # between runs, untimed: what train.fit does with a stale graph
                nan, void = cap["graph"].check()
                cap["nan"] += nan
                cap["void"] += void
                if cap["graph"].stale:
                    cap["graph"] = mc.graphed_train_step(batch, oc, warmup=1)
                    cap["captures"] += 1
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.steps):
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t) * 1e3)
            res["runs"][name].append({"ms_median": float(np.median(ts)), "ms_spread": float(np.max(ts) - np.min(ts))})
    nan, void = cap["graph"].check()
    mb.network.check_train_logs()
    res["c_nan_losses"], res["c_void_replays"], res["c_captures"] = int(cap["nan"] + nan), int(cap["void"] + void), cap["captures"]
    for name, m in (("b_eager_deferred", mb), ("c_captured", mc)):
        st = m.network.train_log_stats()
        res[name + "_attempts"] = {"enqueued_per_step": sum(r["attempts"] for r in st["rows"]),
                                   "largest_taken_per_step": sum(r["max_took"] for r in st["rows"]),
                                   "noop_launches_per_step": st["noop"], "not_clean_runs": sum(r["not_clean"] for r in st["rows"]),
                                   "budgets": [[r["attempts"], r["cap"]] for r in st["rows"]]}
    res["a_steps_per_integration"] = [len(s) for s in ma.network.last_train_steps]
    return res


def text_legs(res):
    B_, N_, R_ = res["shape"]
    lines = [f"continuous training step, {B_} x {N_} -> {N_ * R_} points; {res['device']}; three legs alternated on one box, {res['rounds']} rounds of "
             f"{res['steps_per_run']} steps each; per run: median step ms (spread = max - min of its steps)"]
    med = {}
    for name, runs in res["runs"].items():
        lines.append(f"{name:18s} " + "   ".join(f"{r['ms_median']:.3f} ({r['ms_spread']:.3f})" for r in runs))
        ms = [r["ms_median"] for r in runs]
        med[name] = (float(np.median(ms)), float(np.max(ms) - np.min(ms)))
    for name, (m, sp) in med.items():
        lines.append(f"{name:18s} median of the run medians {m:.3f} ms, spread of the run medians {sp:.3f} ms")
    a_m, a_sp = med["a_eager"]
    for name in ("b_eager_deferred", "c_captured"):
        d = med[name][0] - a_m
        lines.append(f"{name} - a_eager = {d:+.3f} ms ({100 * d / a_m:+.1f} %) against a_eager's spread of {a_sp:.3f} ms: "
                     f"{'more' if abs(d) >= 3 * a_sp else 'LESS'} than three spreads")
        at = res[name + "_attempts"]
        lines.append(f"   attempts enqueued per step {at['enqueued_per_step']}, largest taken {at['largest_taken_per_step']}, no-op attempt launches "
                     f"per step {at['noop_launches_per_step']}, runs not clean {at['not_clean_runs']}")
    lines.append(f"learning rate {res['learning_rate']:g}; captured leg: NaN losses {res['c_nan_losses']}, void replays {res['c_void_replays']} "
                 f"(an integration outgrew its captured budget; checked between the runs), captures {res['c_captures']}; accepted steps per "
                 f"integration (leg a, last step) {res['a_steps_per_integration']}")
    return "\n".join(lines) + "\n"


def text(res):
    f = lambda t: f"{t['ms_median']:10.3f} ({t['ms_min']:.3f} .. {t['ms_max']:.3f}) x{t['repeats']}"
    B_, N_, R_ = res["shape"]
    lines = [f"continuous training step, {B_} x {N_} -> {N_ * R_} points; {res['device']}; ms: median (min .. max) of the repeats after a warm-up",
             f"(a) eager train_step (emd_workgroups = 1)          {f(res['a_train_step'])}   accepted steps per integration {res['a_steps_per_integration']}",
             f"(b) flow part alone, forward + backward            {f(res['b_flow_part'])}   accepted steps per integration {res['b_steps_per_integration']}",
             f"(c) twelve flow_block calls, pack=\"host\"            {f(res['c_twelve_flow_block_calls_pack_host'])}   <- the yardstick: the path before this change",
             f"    twelve flow_block calls, pack=\"device\"          {f(res['c_twelve_flow_block_calls_pack_device'])}"]
    for r in res["d_taped_forward"]:
        d, h = r["device"], r["host"]
        sp = max(d["ms_max"] - d["ms_min"], h["ms_max"] - h["ms_min"])
        lines.append(f"(d) taped forward, block {r['block']} {r['case']} ({r['rows']} rows, {r['accepted_steps']} steps): pack=\"device\" {f(d)}   "
                     f"pack=\"host\" {f(h)}   gain {h['ms_median'] - d['ms_median']:.3f} ms against a spread of {sp:.3f} ms")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", action="store_true", help="eager / eager deferred / captured, alternated (DESIGN 9b)")
    ap.add_argument("--steps", type=int, default=20, help="--legs: steps per run")
    ap.add_argument("--lr", type=float, default=0.0, help="--legs: learning rate.  0 (default) holds the weights, so that every run of "
                    "every leg does the same work; with a real rate the integrations' step counts drift from run to run and a captured "
                    "step's budgets are outgrown (void replays until the next check, then a new capture)")
    a = ap.parse_args()
    if a.legs:
        res = run_legs(a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
        with open(os.path.splitext(a.out)[0] + ".txt", "w") as fh:
            fh.write(text_legs(res))
        print(text_legs(res))
        return
    res = run(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.splitext(a.out)[0] + ".txt", "w") as fh:
        fh.write(text(res))
    print(text(res))


if __name__ == "__main__":
    main()
