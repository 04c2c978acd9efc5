"""Time the continuous model on a frozen step schedule (one pf_cnf_replay launch per integration) against the adaptive
paths it stands beside, with the bench workload's weights (weights.CNF_PU1K_DYNAMICS / CNF_PU1K_END_TIMES).  All legs of a table
run in ONE process on one box, alternated round by round; a run is --steps forwards / steps, each timed by the host clock around
the call and a device synchronise; per run the median and the spread (max - min) of its steps.  The project's rule for "pays": a
leg differs from its reference leg when the medians of the run medians are more than three spreads of the reference leg's run
medians apart.  Recorded, not gated; no default depends on it.

  (a) eval forward, 32 x 2048 -> 8192, bench.py --mode cnf's four rotating input sets:
        a_adaptive      the default forward (blind attempt budgets, controller on the device)          <- the reference leg
        b_replay_r1     `step_schedule` = the schedule recorded on input set 0, refine 1
        c_replay_r2     the same schedule, every step halved
      with the evaluations, accepted / rejected steps and step launches per forward, and for the replays the worst per-step
      error ratio on each input set (the schedule was recorded on set 0 alone), the distance of x to the adaptive forward's and,
      for all three, to the same schedule with every step cut in four (the most accurate of them: the yardstick of x);
  (b) training step, 32 x 256 -> 1024 (TrainerModule, emd_workgroups = 1, learning rate 0: every run does the same work):
        a_eager         host-read controllers                                                         <- the reference leg
        b_eager_deferred, c_captured_deferred    cfg.cnf_deferred, eager and as one graph replay
        d_eager_schedule, e_captured_schedule    cfg.cnf_schedule = the schedule recorded on this batch, eager and captured

  python tools/time_cnf_schedule.py --out profiles/cnf_schedule/time_cnf_schedule.json [--only eval|train]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS = 5


def _legs(legs, steps, between=None):
    import torch
    runs = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for name, fn in legs.items():
            if between is not None:
                between(name)
            torch.cuda.synchronize()
            ts = []
            for s in range(steps):
                t = time.perf_counter()
                fn(s)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t) * 1e3)
            runs[name].append({"ms_median": float(np.median(ts)), "ms_spread": float(np.max(ts) - np.min(ts))})
    return runs


def _verdicts(runs, ref):
    med = {k: (float(np.median([r["ms_median"] for r in v])), float(np.ptp([r["ms_median"] for r in v]))) for k, v in runs.items()}
    out = {}
    for k, (m, _) in med.items():
        d = m - med[ref][0]
        out[k] = {"ms": m, "spread_of_run_medians": med[k][1], "delta_ms": d, "delta_pct": 100 * d / med[ref][0],
                  "more_than_three_spreads": bool(abs(d) > 3 * med[ref][1]) if k != ref else None}
    return out


def run_eval(a):
    import torch
    from puflow_amd import cnf
    from puflow_amd.weights import CNF_PU1K_DYNAMICS, CNF_PU1K_END_TIMES, synth_cnf_state_dict, synth_patches
    dev = "cuda:0"
    B, N, R, NSETS = a.batch, 2048, 4, 4
    sd = synth_cnf_state_dict(2021, dynamics=CNF_PU1K_DYNAMICS, end_times=CNF_PU1K_END_TIMES)
    net = cnf.PointInterpFlow(3)
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    sets = []
    for k in range(NSETS):                                              # bench.py --mode cnf's input sets
        g = torch.Generator().manual_seed(1000 * k)
        sets.append((synth_patches(B, N, seed=2021 + 101 * k).to(dev), [torch.randn(B, N, 3, generator=g).to(dev) for _ in range(6)]))
    sched1 = net.record_schedule(sets[0][0], R, noise=sets[0][1])
    rec = {k: net.last_record[k] for k in ("accepted", "rejected")}
    scheds = {"a_adaptive": None, "b_replay_r1": sched1, "c_replay_r2": cnf.refine_schedule(sched1, 2)}
    res = {"device": torch.cuda.get_device_name(0), "shape": [B, N, R], "steps_per_run": a.steps, "rounds": ROUNDS,
           "recorded_on_set_0": rec, "steps_per_integration": [len(sched1[k]) - 1 for k in cnf.schedule_keys()], "work": {}}
    net.step_schedule = cnf.refine_schedule(sched1, 4)                  # the yardstick of x: the same grids, every step in four
    fine_x, res["refine4_worst_error_ratio"] = [], []
    for x, ns in sets:
        fine_x.append(net(x, R, noise=ns)[0])
        res["refine4_worst_error_ratio"].append(max(max(v) for v in net.schedule_error_ratios().values()))
    ref_x = []
    for name, s in scheds.items():                                      # work counts, error ratios and warm-up of every leg
        net.step_schedule = s
        rows = []
        for k, (x, ns) in enumerate(sets):
            out, _ = net(x, R, noise=ns)
            st = net.last_stats
            row = {"nfe": st["nfe"], "accepted": st["accepted"], "rejected": st["rejected"],
                   "max_abs_x_minus_refine4": float((out - fine_x[k]).abs().max())}
            if s is None:
                net(x, R, noise=ns)                                     # the second forward on a set runs blind: its launch count
                bl = net.last_stats["blind"]
                row["step_launches"] = bl["attempts_enqueued"] if bl["ran"] else bl["attempts_taken"]
                row["launches"] = row["step_launches"] + 2 * 12         # + pf_cnf_init's two per integration
                row["noop_step_launches"] = max(bl["attempts_enqueued"] - bl["attempts_taken"], 0) if bl["ran"] else 0
                ref_x.append(out)
            else:
                ratios = net.schedule_error_ratios()
                row["launches"] = 2 * 12                                # pf_cnf_replay + the error sums' reduction
                row["worst_error_ratio"] = max(max(v) for v in ratios.values())
                row["worst_by_integration"] = [max(ratios[key]) for key in cnf.schedule_keys()]
                row["max_abs_x_minus_adaptive"] = float((out - ref_x[k]).abs().max())
            rows.append(row)
        res["work"][name] = rows

    def forward(s):
        x, ns = sets[s % NSETS]
        net(x, R, noise=ns)

    def between(name):                                                  # switch the leg and warm it up, untimed
        net.step_schedule = scheds[name]
        for x, ns in sets:
            net(x, R, noise=ns)
    res["runs"] = _legs({k: forward for k in scheds}, a.steps, between)
    res["verdict"] = _verdicts(res["runs"], "a_adaptive")
    return res


def run_train(a):
    import torch
    from puflow_amd.trainer import TrainerModule, default_cfg
    from puflow_amd.weights import CNF_PU1K_DYNAMICS, CNF_PU1K_END_TIMES, synth_cnf_state_dict, synth_patches
    dev = "cuda:0"
    B, N, R = a.batch, 256, 4
    sd = synth_cnf_state_dict(2021, dynamics=CNF_PU1K_DYNAMICS, end_times=CNF_PU1K_END_TIMES)
    dense = synth_patches(B, N * R, seed=2021).to(dev)
    batch = (dense[:, ::R].contiguous(), dense)

    def module(**kw):
        torch.manual_seed(0)
        m = TrainerModule(default_cfg(model="continuous", emd_workgroups=1, learning_rate=0.0, **kw))
        m.network.load_state_dict(sd, strict=True)
        m = m.to(dev)
        return m, m.configure_optimizers()["optimizer"]

    ma, oa = module()
    mb, ob = module(cnf_deferred=True)
    mc, oc = module(cnf_deferred=True)
    md, od = module()
    me, oe = module()
    sched = md.record_schedule(batch)                                   # the adaptive solver's steps on this batch, weights as loaded
    me.network.step_schedule = sched
    for _ in range(2):                                                  # the warm-up steps the captures take, for all
        for m, o in ((ma, oa), (mb, ob), (md, od)):
            m.train_step(batch, o)
    cap = {"c": mc.graphed_train_step(batch, oc, warmup=2), "e": me.graphed_train_step(batch, oe, warmup=2), "captures_c": 1, "void": 0}
    legs = {"a_eager": lambda s: ma.train_step(batch, oa), "b_eager_deferred": lambda s: mb.train_step(batch, ob),
            "c_captured_deferred": lambda s: cap["c"](batch), "d_eager_schedule": lambda s: md.train_step(batch, od),
            "e_captured_schedule": lambda s: cap["e"](batch)}

    def between(name):                                                  # what train.fit does with a stale graph, untimed
        if name == "c_captured_deferred":
            _, void = cap["c"].check()
            cap["void"] += void
            if cap["c"].stale:
                cap["c"] = mc.graphed_train_step(batch, oc, warmup=1)
                cap["captures_c"] += 1
        if name == "e_captured_schedule":
            cap["e"].check()
    res = {"device": torch.cuda.get_device_name(0), "shape": [B, N, R], "steps_per_run": a.steps, "rounds": ROUNDS,
           "runs": _legs(legs, a.steps, between)}
    res["verdict"] = _verdicts(res["runs"], "a_eager")
    mb.network.check_train_logs()
    cap["c"].check()
    for name, m in (("b_eager_deferred", mb), ("c_captured_deferred", mc)):
        st = m.network.train_log_stats()
        res[name + "_attempts"] = {"enqueued_per_step": sum(r["attempts"] for r in st["rows"]),
                                   "largest_taken_per_step": sum(r["max_took"] for r in st["rows"]), "noop_launches_per_step": st["noop"]}
    res["c_void_replays"], res["c_captures"], res["e_recaptures"] = cap["void"], cap["captures_c"], cap["e"].recaptures
    res["a_steps_per_integration"] = [len(s) for s in ma.network.last_train_steps]
    res["schedule_steps_per_integration"] = [len(s) for s in md.network.last_train_steps]
    res["integration_launches_per_step"] = {"adaptive_eager": "2 (init) + attempts per integration, a read per batch of attempts",
                                            "schedule": 12}
    return res


def text(res):
    lines = []
    for part, ref in (("eval", "a_adaptive"), ("train", "a_eager")):
        r = res.get(part)
        if r is None:
            continue
        B_, N_, R_ = r["shape"]
        what = "eval forward" if part == "eval" else "training step"
        lines.append(f"continuous model, {what}, {B_} x {N_} -> {N_ * R_} points; {r['device']}; legs alternated on one box in one process, "
                     f"{r['rounds']} rounds of {r['steps_per_run']} each; per run: median ms (spread = max - min of its steps)")
        for name, runs in r["runs"].items():
            lines.append(f"  {name:22s} " + "   ".join(f"{x['ms_median']:.3f} ({x['ms_spread']:.3f})" for x in runs))
        for name, v in r["verdict"].items():
            if name == ref:
                lines.append(f"  {name:22s} median of the run medians {v['ms']:.3f} ms, spread of the run medians {v['spread_of_run_medians']:.3f} ms"
                             "   <- the reference leg")
            else:
                lines.append(f"  {name:22s} median of the run medians {v['ms']:.3f} ms, {v['delta_ms']:+.3f} ms ({v['delta_pct']:+.1f} %) against "
                             f"{ref}: {'MORE' if v['more_than_three_spreads'] else 'less'} than three of its spreads")
        if part == "eval":
            lines.append(f"  schedule recorded on input set 0: {r['recorded_on_set_0']['accepted']} accepted / {r['recorded_on_set_0']['rejected']} rejected, "
                         f"steps per integration {r['steps_per_integration']}")
            for name, rows in r["work"].items():
                for k, w in enumerate(rows):
                    extra = (f"step launches {w['step_launches']} ({w['noop_step_launches']} no-ops), launches {w['launches']}" if "step_launches" in w else
                             f"launches {w['launches']}, worst error ratio {w['worst_error_ratio']:.2f}, max|x - adaptive x| {w['max_abs_x_minus_adaptive']:.2e}")
                    lines.append(f"  {name:14s} set {k}: nfe {w['nfe']}, accepted {w['accepted']}, rejected {w['rejected']}, {extra}, "
                                 f"max|x - refine-4 x| {w['max_abs_x_minus_refine4']:.2e}")
            lines.append(f"  refine 4 (the yardstick of x, not timed): worst error ratio per set {[round(v, 4) for v in r['refine4_worst_error_ratio']]}")
        else:
            for name in ("b_eager_deferred", "c_captured_deferred"):
                at = r[name + "_attempts"]
                lines.append(f"  {name}: attempts enqueued per step {at['enqueued_per_step']}, largest taken {at['largest_taken_per_step']}, "
                             f"no-op launches {at['noop_launches_per_step']}")
            lines.append(f"  captured deferred: void replays {r['c_void_replays']}, captures {r['c_captures']}; captured schedule: recaptures "
                         f"{r['e_recaptures']}; steps per integration adaptive {r['a_steps_per_integration']}, schedule {r['schedule_steps_per_integration']}")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", choices=["eval", "train"], default=None)
    ap.add_argument("--steps", type=int, default=12, help="forwards / steps per run")
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    res = {}
    if a.only != "train":
        res["eval"] = run_eval(a)
    if a.only != "eval":
        res["train"] = run_train(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.splitext(a.out)[0] + ".txt", "w") as fh:
        fh.write(text(res))
    print(text(res))


if __name__ == "__main__":
    main()
