"""GPU: `bench.py --mode train` in a FRESH process (one child, a few steps).  The graphed training step once faulted only
there - a memset node inside the captured hipGraph raced with the multi-workgroup EMD auction that follows it - while every
in-process test passed, so this path gets its own test."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("graph", ["1", "0"])
def test_bench_train_fresh_process(graph):
    env = dict(os.environ, PF_BENCH_GRAPH=graph)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--mode", "train", "--steps", "4", "--warmup", "2", "--cpu-seconds", "2"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["unit"] == "patches/s" and rec["value"] > 0 and rec["steps"] == 4
    assert rec["loss"] == rec["loss"] and abs(rec["loss"]) < 1e3          # finite, sane
    assert "capture failed" not in out.stderr
    # the measurement contract of the line: roofline of the dominant launch group (live HIP events) and the CPU oracle's step
    roof, cpu = rec["roofline"], rec["cpu_baseline"]
    assert roof["bound"] == "mfma" and roof["unit"] == "TFLOP/s" and 0 < roof["frac"] < 1 and roof["avg_launch_ms"] > 0
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-9
    assert cpu["kind"] == "port" and cpu["unit"] == "patches/s" and cpu["value"] > 0 and cpu["cores"] >= 1
    assert rec["value"] > 10 * cpu["value"]
    # the line says what it computes in, and how far the split-product gradients are from the f32-product build
    assert "split-bf16" in rec["dtype"] and "BACKWARD" in rec["dtype"]
    gp = rec["grad_parity"]
    for tag in ("backward_only", "all"):
        assert gp[tag]["n_parameters"] > 150 and gp[tag]["max"] == gp[tag]["max"], gp
        print("grad_parity", tag, {k: gp[tag][k] for k in ("max", "worst_parameter", "p95", "median", "run_to_run_noise_default_build",
                                                          "flat_gradient_rel_l2", "zero_gradient_tensors")})
    # the backward kernels' split-bf16 products alone (identical forward): 16 mantissa bits per operand -> ~2e-5 of the flat
    # gradient, 1e-4 of the worst tensor (measured: 2.4e-5 / 1.2e-4); the run-to-run noise of the float atomics is below 1e-5
    bo = gp["backward_only"]
    assert bo["flat_gradient_rel_l2"] < 1e-4 and bo["max"] < 5e-4 and bo["run_to_run_noise_default_build"]["max"] < 5e-5, bo
    assert gp["all"]["flat_gradient_rel_l2"] < 5e-3


def test_bench_reduced_precision_line():
    """`python bench.py`: the headline stays the fp32-parity arithmetic; the secondary single-term fp16 line (a child process on
    libpuflow_hip_f16.so) is present, faster, bit-exact in kNN and within Chamfer-distance noise of the fp32 oracle."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "20", "--warmup", "3", "--cpu-seconds", "2"],
                         cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["dtype"].startswith("f32") and rec["parity"]["max_abs_dx_vs_oracle"] < 1e-5
    red = rec["reduced_precision"]
    assert "value" in red, red
    assert red["dtype"].startswith("f16") and red["knn_idx_exact_match_rate"] == 1.0
    assert red["max_abs_dx_vs_fp32_oracle"] < 5e-3 and red["cd_build_vs_fp32_oracle"] < 1e-6
    assert red["value"] > 0.9 * rec["value"]
    # secondary two-steps-in-flight figure: part of the line only when it beats the headline on this box
    pl = rec.get("pipelined")
    assert pl is None or (pl["steps_in_flight"] == 2 and pl["value"] > rec["value"])
    # the launch mode of the timed region is the faster of the two probed ones, and the line says which and by how much
    lp = rec["launch_probe"]
    assert lp["chosen"] in ("graph", "eager") and lp["graph_replay_ms_per_step"] > 0 and lp["eager_ms_per_step"] > 0
    assert (lp["chosen"] == "graph") == (lp["graph_replay_ms_per_step"] <= lp["eager_ms_per_step"])
    assert rec["config"]["launch"].startswith("hipGraph replay" if lp["chosen"] == "graph" else "eager")
    assert rec["zero_copy_input"]["value"] > 0


def test_bench_pipeline_option_small_batch():
    """`--pipeline 3 --scaling strong --total-batch 4`: three captured graphs on three streams; the JSON line keeps the contract
    (steps, unit) and the results of every graph are the ones of the single-graph run (parity block)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--scaling", "strong", "--total-batch", "4", "--pipeline", "3",
                          "--steps", "30", "--warmup", "3", "--cpu-seconds", "1", "--no-reduced"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["steps"] == 30 and rec["unit"] == "patches/s" and rec["scaling"] == "strong" and rec["value"] > 0
    assert "3 steps in flight" in rec["config"]["launch"] and "pipelined" not in rec
    assert rec["parity"]["max_abs_dx_vs_oracle"] < 1e-5 and rec["parity"]["knn_idx_exact_match_rate"] == 1.0


def test_bench_gpus_n_starts_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it (WORLD_SIZE unset) must run TWO ranks - fresh child processes
    under torch.distributed.run, started before the parent touches the GPU - and report n_gpus = 2, not a silent one-rank
    run.  Rehearsal knobs of the one-GPU box: both ranks on cuda:0, gloo instead of RCCL."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(PF_BENCH_SINGLE_DEVICE="1", PF_BENCH_BACKEND="gloo")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--batch", "4", "--steps", "10", "--warmup", "2",
                          "--no-pipelined"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                    # rank 0 only
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["scaling"] == "weak" and rec["config"]["total_batch"] == 8 and rec["value"] > 0
    assert rec["cpu_baseline"] is None                        # N = 1 only
    assert "launching" in out.stderr
    # the same invocation also carries the strong-scaling figures and the communicator's own account (2 ranks over gloo)
    assert rec["strong"]["32"]["patches_per_rank"] == [16, 16] and rec["strong"]["256"]["patches_per_rank"] == [128, 128]
    assert all(v["value"] > 0 for v in rec["strong"].values())
    assert all(v["launch"] in ("graph", "eager") and v["ms_per_step"] == min(v["ms_per_step_graph_replay"], v["ms_per_step_eager"])
               for v in rec["strong"].values())
    col = rec["config"]["collectives"]
    assert col["world_size"] == 2 and col["communicator_ranks_seen_by_first_all_reduce"] == 2 and col["gradient_bucket_all_reduce"]["median_us"] > 0
    # a launcher environment that disagrees with --gpus is an error, not a mislabeled run
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"], cwd=ROOT,
                         env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "WORLD_SIZE" in bad.stderr


def test_bench_cnf_line():
    """`bench.py --mode cnf` (BASELINE configs[4]) on a small batch: the contract fields, the solver's work on the scaled
    synthetic ODE (rejected steps included) and the same evaluation / accept / reject counts as the CPU oracle's dopri5."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--mode", "cnf", "--batch", "2", "--npoint", "256", "--steps", "2",
                          "--warmup", "1", "--cpu-seconds", "1"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["unit"] == "patches/s" and rec["value"] > 0 and rec["steps"] == 2 and "configs[4]" in rec["config"]["workload"]
    work = rec["config"]["solver_work"]
    per = work["per_input_set"]                                    # the timed loop rotates four input sets
    assert min(per["nfe"]) >= 300 and min(per["rejected"]) >= 1    # not the trivial 168-evaluation ODE of random-init weights
    bl = work["blind"]
    assert bl["forwards"] == 2 and bl["attempts_taken"] > 0 and bl["fell_back"] <= bl["ran_blind"] <= bl["forwards"]
    assert rec["roofline"]["attempts_timed"]["real"] > 0 and "pf_cnf_steps" in rec["roofline"]["kernel"]
    roof, cpu, par = rec["roofline"], rec["cpu_baseline"], rec["parity"]
    assert roof["bound"] == "mfma" and 0 < roof["frac"] < 1 and cpu["kind"] == "port" and cpu["value"] > 0
    assert par["nfe"][0] == par["nfe"][1] and par["accepted"][0] == par["accepted"][1] and par["rejected"][0] == par["rejected"][1]
    # the bound comes from the line's own float64 anchor: the synthetic map expands in g, the fp32 CPU oracle itself sits
    # ~2e-3 from the float64 evaluation; the HIP path may be no further from fp64 than 4x that
    anc = par["fp64_anchor"]
    for k in ("x", "z", "ldj"):
        assert anc[k]["hip_vs_f64"] <= 4.0 * anc[k]["oracle_f32_vs_f64"] + 1e-4, (k, anc[k])
    assert par["max_abs_dx_vs_oracle"] <= 5.0 * anc["x"]["oracle_f32_vs_f64"] + 1e-4


def test_bench_train_two_ranks_self_launched():
    """`bench.py --gpus 2 --mode train` (rehearsal knobs: both ranks on cuda:0, gloo): the per-rank steps, the call profile's
    eager steps (they contain the gradient all-reduce, so EVERY rank must run them) and the report on rank 0."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(PF_BENCH_SINGLE_DEVICE="1", PF_BENCH_BACKEND="gloo")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--mode", "train", "--batch", "4", "--steps", "3",
                          "--warmup", "1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["n_gpus"] == 2 and rec["value"] > 0 and rec["loss"] == rec["loss"]
    assert rec["roofline"]["avg_launch_ms"] > 0 and rec["cpu_baseline"] is None


def test_bench_pugan_line():
    """`bench.py --mode pugan` (BASELINE configs[3]: clouds of 5000 -> 20000 points through the patch pipeline) on two clouds:
    contract fields, the FPS merge's latency roofline (rounds counted by the kernel, exchange floor probed live) and coverage
    parity with the CPU oracle pipeline."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--mode", "pugan", "--batch", "2", "--steps", "2", "--warmup", "1"],
                         cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["unit"] == "patches/s" and rec["value"] > 0 and "configs[3]" in rec["config"]["workload"]
    assert rec["config"]["patches_per_cloud"] == 78 and rec["config"]["candidates_per_cloud"] == 99840
    assert abs(rec["value"] - rec["clouds_per_s"] * 78) < 1e-6 * rec["value"]
    roof, lat = rec["roofline"], rec["roofline"]["latency"]
    assert roof["bound"] == "latency" and abs(roof["frac"] - roof["peak"] / roof["achieved"]) < 1e-12 and "fps_coopm_kernel" in roof["kernel"]
    assert abs(roof["hbm"]["frac"] - roof["hbm"]["achieved"] / roof["hbm"]["peak"]) < 1e-12
    assert lat["samples_per_cloud"] == 20024 and 313 <= lat["rounds_per_cloud"] <= 5000          # up to 64 samples per exchange round
    assert 0.5 < lat["exchange_floor_us_per_round"] < lat["us_per_round_one_cloud"] < 40.0
    cpu, par = rec["cpu_baseline"], rec["parity"]
    assert cpu["kind"] == "port" and cpu["value"] > 0 and rec["value"] > 10 * cpu["value"]
    assert par["rel_diff"] < 0.02


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """`python bench.py` without --full: the headline line alone (no secondary legs), and --dump-outputs writes what the timed
    path returned in its last step - the same x / logp as a forward of the benchmark's seeded batch in this process."""
    import numpy as np
    import torch
    from puflow_amd.interpflow import PointInterpFlow
    from puflow_amd.weights import synth_patches, synth_state_dict
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path)],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["steps"] == 7 and rec["unit"] == "patches/s" and rec["higher_is_better"] is True and rec["dtype"].startswith("f32")
    assert abs(rec["value"] - 32 / (rec["ms_per_step"] * 1e-3)) < 1e-6 * rec["value"]
    assert rec["roofline"] is None and rec["cpu_baseline"] is None
    assert not {"parity", "reduced_precision", "zero_copy_input", "pipelined", "stage_ms", "strong"} & set(rec)
    x, logp = np.load(tmp_path / "x.npy"), np.load(tmp_path / "logp.npy")
    assert x.dtype == np.float32 and x.shape == (32, 4 * 2048, 3) and logp.dtype == np.float32
    net = PointInterpFlow(3)
    net.load_state_dict(synth_state_dict(2021))
    net.set_to_initialized_state()
    net = net.to("cuda:0").eval()
    xr, lr = net(synth_patches(32, 2048, seed=2021).to("cuda:0"), 4)
    assert np.abs(x - xr.cpu().numpy()).max() < 1e-5
    assert abs(float(logp) - float(lr)) <= 1e-5 * abs(float(lr))
