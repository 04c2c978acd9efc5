#!/usr/bin/env python3
"""Headline benchmark: patches/sec, discrete PU-Flow x4, 2048 -> 8192 points per patch
(BASELINE.json metric; workload = configs[1]: batch of 32 x 2048-point patches per GPU, eval).

  python bench.py --gpus 1 --steps 20 --warmup 5
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

One process per GPU.  Patches are independent, so the batch is sharded over ranks with NO
data-path collective (weak scaling: 32 patches per GPU); the only collectives are the timing
barrier and the MAX over ranks of the elapsed time.  A step = one PointInterpFlow.forward over
the rank's 32 patches, inputs resident in HBM.  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times exactly --steps steps and prints the line; --full adds every secondary
measurement and check (roofline, CPU baseline and oracle parity, reduced precision, ...).  --dump-outputs DIR
writes what the timed path returned in its last step as .npy files (inputs are seeded: same arguments, same inputs).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
FP32_MFMA_PEAK_TF = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 / 32x32x2 peak
BF16_MFMA_PEAK_TF = 2500.0     # MI355X_MICROARCH.md: dense bf16 MFMA (~2.5 PF; the 5 PF headline includes 2:1 sparsity)


def edgeconv_ref_flops(T, C, g, nconv, odim, K=16):
    """Algorithmic FLOPs of one EdgeConv unit in the REFERENCE's dense formulation
    (2 x MACs of the 1x1 convs on [3C + g t] channels over T*K edges)."""
    macs = sum((3 * C + g * t) * g for t in range(nconv)) + (3 * C + g * nconv) * odim
    return 2.0 * T * K * macs


def model_ref_flops_per_patch():
    return 36.70e9               # 18.351 GMAC per 2048-pt patch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32, help="patches per GPU (weak scaling)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak: --batch patches per GPU; strong: --total-batch patches split over the ranks")
    ap.add_argument("--total-batch", type=int, default=256,
                    help="patches of the whole job under --scaling strong (default 8 x 32: 32 per GPU at 8 GPUs - SURVEY 8e's threshold for "
                         "the >= 6x claim is >= 8 patches per GPU, i.e. a total of >= 64; one 32-patch batch over 8 GPUs predicts 4.7x, "
                         "DESIGN section 6)")
    ap.add_argument("--npoint", type=int, default=2048)
    ap.add_argument("--mode", choices=["infer", "train", "cnf", "pugan"], default="infer",
                    help="infer = headline metric (BASELINE configs[1]); train = configs[2] training step (CD+EMD, RCCL all-reduce); "
                         "cnf = configs[4] continuous (CNF) x4 inference, dopri5 on the device; pugan = configs[3] PU-GAN clouds of 5000 -> "
                         "20000 points through the patch pipeline (--batch clouds per GPU and step)")
    ap.add_argument("--cloud-points", type=int, default=5000, help="--mode pugan: points per input cloud")
    ap.add_argument("--dump-grads", type=str, default=None,
                    help="--mode train, internal (the `grad_parity` leg): run ONE forward + loss + backward of the benchmark step from the "
                         "benchmark's initial state and save every parameter gradient to this file, then exit")
    ap.add_argument("--no-grad-parity", action="store_true", help="--mode train: skip the gradient comparison with the f32-product build")
    ap.add_argument("--pipeline", type=int, default=1,
                    help="steps in flight: P > 1 replays P captured graphs round-robin on P streams (independent batches overlap; "
                         "pays off when one batch cannot fill the chip, e.g. --scaling strong at 4 patches per GPU)")
    ap.add_argument("--no-pipelined", action="store_true", help="skip the secondary two-steps-in-flight measurement")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-reduced", action="store_true",
                    help="skip the secondary reduced-precision line (a child process on libpuflow_hip_f16.so)")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="budget for the CPU baseline sample")
    ap.add_argument("--cnf-dynamics", type=float, default=None,
                    help="--mode cnf: scale of the synthetic ODE nets (1 = random init; default weights.CNF_PU1K_DYNAMICS = 1.7, which "
                         "together with --cnf-end-times pu1k makes dopri5 work like on the reference's pretrained checkpoint)")
    ap.add_argument("--cnf-end-times", choices=["pu1k", "init"], default="pu1k",
                    help="--mode cnf: integration end times of the six blocks - pu1k = those of the reference's trained checkpoint "
                         "(weights.CNF_PU1K_END_TIMES), init = 0.5 everywhere (cnf.py:41)")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary measurement and check after the timed steps (roofline / per-stage timings, CPU "
                         "baseline and parity with the oracle, reduced-precision line, pipelined and zero-copy figures, strong scaling "
                         "and collectives under --gpus N, gradient parity in --mode train); without it a run sets up, warms up, times "
                         "--steps steps and prints the line")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy (float32 / "
                         "float64, at most 64 MB in all: a larger array is replaced by a fixed seeded sample of its elements); rank 0 only")
    args = ap.parse_args()
    # torch's CPU ops default to one OpenMP thread per VISIBLE CPU (128 on the MI355X boxes); a container owns far fewer CPUs' worth of
    # quota, and a pool of spinning threads exhausts it within ms - the whole process, the thread waiting for the GPU included, is
    # then throttled until the next 100 ms period.  Keep the host side within the CPUs the bench uses.
    torch.set_num_threads(max(1, min(torch.get_num_threads(), _ncpu())))

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves.  This process has made no GPU call
        # yet (importing torch does not initialise the device) and makes none: it only waits for the children.
        return self_launch(args.gpus)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with `python -m torch.distributed.run --nnodes=1 "
                         f"--nproc-per-node {args.gpus} --master-addr 127.0.0.1 --master-port P bench.py --gpus {args.gpus} ...` "
                         f"(or leave WORLD_SIZE unset and bench.py starts the ranks itself)")
    if args.scaling == "strong":                     # fixed total work: the rank's contiguous shard of --total-batch patches
        from puflow_amd.dist import shard_bounds
        lo, hi = shard_bounds(args.total_batch, rank, world)
        if hi - lo < 1:
            raise SystemExit(f"--total-batch {args.total_batch} leaves rank {rank} of {world} without a patch")
        args.batch = hi - lo
    # rehearsal knobs (one-GPU box): PF_BENCH_SINGLE_DEVICE=1 maps every rank to cuda:0 and PF_BENCH_BACKEND=gloo
    # replaces RCCL (two ranks cannot share one device under RCCL); the driver's multi-GPU runs use neither.
    if os.environ.get("PF_BENCH_SINGLE_DEVICE") == "1":
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    import torch.distributed as dist
    # PF_BENCH_FORCE_DIST=1: initialise the process group and run every collective of the multi-rank path even with ONE
    # rank (RCCL smoke on a one-GPU box: backend load, eager all-reduce between graph replays, clean teardown)
    use_dist = args.use_dist = world > 1 or os.environ.get("PF_BENCH_FORCE_DIST") == "1"
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:               # only without a launcher (one forced rank): any free port
            import socket
            sk = socket.socket(); sk.bind(("127.0.0.1", 0)); os.environ["MASTER_PORT"] = str(sk.getsockname()[1]); sk.close()
        if world == 1:
            from puflow_amd.dist import force_collectives
            force_collectives(True)
        backend = os.environ.get("PF_BENCH_BACKEND", "nccl")
        rccl_log = None
        if backend == "nccl" and os.environ.get("PF_BENCH_RCCL_DEBUG", "1") == "1" and args.mode == "infer" and args.full:
            # what RCCL says about itself goes to a per-rank file (NCCL_DEBUG_FILE), parsed after the first collective: the line
            # then carries the transport the rings really use (P2P over xGMI / SHM / NET) instead of an assumption
            import tempfile
            rccl_log = os.path.join(tempfile.gettempdir(), f"pf_bench_rccl_{os.environ.get('MASTER_PORT', '0')}_r{rank}.log")
            os.environ.setdefault("NCCL_DEBUG", "INFO")
            os.environ.setdefault("NCCL_DEBUG_SUBSYS", "INIT,GRAPH")
            os.environ.setdefault("NCCL_DEBUG_FILE", rccl_log)
        try:
            if backend == "nccl":
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
            else:
                dist.init_process_group(backend, rank=rank, world_size=world)
            probe = torch.ones(1, device=dev)
            dist.all_reduce(probe)                            # the first collective: creates the communicator, may fail on IPC set-up
            torch.cuda.synchronize()
        except Exception as ex:
            # a fresh child, nothing to retry here: say what to look at and leave (HSA_ENABLE_IPC_MODE_LEGACY=0 is what this
            # pool's host driver needs for cross-process device-memory sharing; self_launch exports it)
            print(f"[bench] rank {rank}: process group / first collective failed: {type(ex).__name__}: {str(ex)[:500]}\n"
                  f"[bench] environment: HSA_ENABLE_IPC_MODE_LEGACY={os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY')} "
                  f"NCCL_DEBUG_FILE={os.environ.get('NCCL_DEBUG_FILE')} backend={backend} world={world} "
                  "(hipIpcGetMemHandle: invalid argument => the dmabuf IPC mode is not set in THIS process's environment)",
                  file=sys.stderr, flush=True)
            raise SystemExit(4)
        seen = int(round(float(probe.item())))               # ranks that took part in the sum = the communicator's size
        if seen != args.gpus or dist.get_world_size() != args.gpus:
            print(f"[bench] the communicator has {seen} rank(s) (torch says {dist.get_world_size()}), --gpus says {args.gpus}", file=sys.stderr)
            raise SystemExit(3)
        args.collectives = {"backend": dist.get_backend(), "world_size": world, "forced_one_rank_group": world == 1}
        args.rccl_log = rccl_log
    else:
        args.collectives = None

    from puflow_amd.interpflow import PointInterpFlow
    from puflow_amd.weights import synth_patches, synth_state_dict

    if args.mode == "train":
        return bench_train(args, world, rank, dev, dist)
    if args.mode == "cnf":
        return bench_cnf(args, world, rank, dev, dist)
    if args.mode == "pugan":
        return bench_pugan(args, world, rank, dev, dist)

    sd = synth_state_dict(2021)
    net = PointInterpFlow(3)
    net.load_state_dict(sd)
    net.set_to_initialized_state()
    net = net.to(dev).eval()
    xyz_cpu = synth_patches(args.batch, args.npoint, seed=2021 + rank)     # each rank its own shard
    xyz = xyz_cpu.to(dev)

    def barrier():
        if use_dist:
            dist.barrier()

    # One step = the whole hot path on one batch.  The launches of a step (16 at 32 patches, 11 at small batches) can be replayed as ONE hipGraph
    # (PointInterpFlow.graphed: same kernels, same order, bit-identical results - tests/test_gpu_parity.py); the input is
    # copied into the graph's static buffer inside the timed step.  PF_BENCH_GRAPH=0 times the eager path.
    # PF_BENCH_GRAPH=auto (default): both launch modes - same kernels, same bits - are probed after the capture and the faster
    # one carries the timed region (the line's `launch_probe` holds both figures; the kernels and their durations are the same -
    # on a quiet host the eager stream saves the input copy and the ~9 us between two graph launches, under host jitter the
    # graph wins); =1 / =0 force one.
    gmode = os.environ.get("PF_BENCH_GRAPH", "auto")
    use_graph = gmode != "0"
    eager_step = lambda inp: net(inp, 4)
    step = eager_step
    if use_graph:
        try:
            step = net.graphed(args.batch, args.npoint, 4)
        except Exception as ex:                                  # capture unsupported on this stack: time the eager path
            print(f"[bench] hipGraph capture failed ({type(ex).__name__}: {ex}); timing the eager path", file=sys.stderr)
            use_graph = False
    pipe = max(int(args.pipeline), 1) if use_graph else 1
    # PF_BENCH_ZERO_COPY=1: the batch sits in the graph's own input buffer (PointInterpFlow.graphed's run.input - what a producer
    # kernel would write into) before the timed region starts, so a step is the replay alone; the default copies it in every step
    zero_copy = use_graph and os.environ.get("PF_BENCH_ZERO_COPY", "0") == "1"

    def feed(fn, zc):
        if not zc:
            return xyz
        fn.input.copy_(xyz)
        return fn.input

    def make_runner(p, zc=zero_copy, graph=None):
        """p steps in flight: p independent captures (own static buffers), replayed round-robin on p streams."""
        graph = use_graph if graph is None else (graph and use_graph)
        if p <= 1:
            fn1 = step if graph else eager_step
            inp = feed(step, zc) if graph else xyz

            def run_steps(n):
                out = None
                for _ in range(n):
                    out = fn1(inp)
                return out
            return run_steps
        lanes = [(step, torch.cuda.Stream(device=dev))] + [(net.graphed(args.batch, args.npoint, 4), torch.cuda.Stream(device=dev))
                                                           for _ in range(p - 1)]
        feeds = [feed(fn, zc) for fn, _ in lanes]

        def run_steps(n):
            cur = torch.cuda.current_stream(dev)
            for _, st in lanes:
                st.wait_stream(cur)
            out = None
            for k in range(n):
                fn, st = lanes[k % p]
                with torch.cuda.stream(st):
                    out = fn(feeds[k % p])
            for _, st in lanes:
                cur.wait_stream(st)
            return out
        return run_steps

    def timed(run_steps):
        run_steps(args.warmup)
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run_steps(args.steps)
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    headline_graph, launch_probe = use_graph, None
    if use_graph and gmode == "auto" and pipe == 1 and not zero_copy:
        n_probe = min(max(args.steps, 50), 200)                  # bounded: the probe's cost must not grow with --steps

        def probe_pass(g):
            r = make_runner(1, False, g)
            r(max(args.warmup, 5))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r(n_probe)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n_probe
        tg, te = probe_pass(True), probe_pass(False)
        tg, te = min(tg, probe_pass(True)), min(te, probe_pass(False))
        tt = torch.tensor([tg, te], dtype=torch.float64, device=dev)
        if use_dist:
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)          # every rank takes the same decision
        tg, te = float(tt[0].item()), float(tt[1].item())
        headline_graph = tg <= te
        launch_probe = {"graph_replay_ms_per_step": tg * 1e3, "eager_ms_per_step": te * 1e3, "steps_per_pass": n_probe,
                        "chosen": "graph" if headline_graph else "eager",
                        "note": "untimed probe before the timed region, best of two passes per mode, max over ranks; PF_BENCH_GRAPH=1 / 0 force a mode"}
    runner = make_runner(pipe, zero_copy, headline_graph)
    # the timed region is exactly --steps steps (the caller sizes it from ms_per_step)
    el, (x, logp) = timed(runner)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"x": x, "logp": logp})
    # per-stage HIP-event times (the roofline's live kernel duration) straight after the timed region, before the secondary legs
    # add another few seconds of load: 5 iterations are sensitive to what ran before them (0.131 vs 0.136 ms for the dominant
    # kernel with the secondary legs in front)
    prof_stages = net._engine(4).profile_stages(xyz, iters=5) if rank == 0 and args.full else None
    # secondary figure (never `value`): the same K steps with two of them in flight on two streams - independent batches
    # overlap; what a serving loop with more than one batch queued gets
    el_pipe = None
    if use_graph and pipe == 1 and not args.no_pipelined and args.full:
        el_pipe, _ = timed(make_runner(2))
        tp = torch.tensor([el_pipe], dtype=torch.float64, device=dev)
        if use_dist:
            dist.all_reduce(tp, op=dist.ReduceOp.MAX)
        el_pipe = float(tp.item())
    # secondary figure (never `value`): the batch already in the graph's own input buffer (run.input), no copy in front of the replay
    el_zc = None
    if use_graph and pipe == 1 and not zero_copy and not args.no_pipelined and args.full:
        el_zc, _ = timed(make_runner(1, True))
        tz = torch.tensor([el_zc], dtype=torch.float64, device=dev)
        if use_dist:
            dist.all_reduce(tz, op=dist.ReduceOp.MAX)
        el_zc = float(tz.item())
    t = torch.tensor([el], dtype=torch.float64, device=dev)
    if use_dist:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    el = float(t.item())
    patches = (args.total_batch if args.scaling == "strong" else world * args.batch) * args.steps
    value = patches / el

    strong = coll = None
    if use_dist and args.scaling == "weak" and args.full:
        # one invocation, both scalings: the weak-scaling figure above is `value`; the same ranks are re-timed
        # on a fixed total of 32 patches (the metric's own batch) and 256 (32 per GPU at 8 GPUs)
        strong = strong_block(args, world, rank, dev, dist, net)
        coll = collectives_probe(args, world, rank, dev, dist)
    out = None
    if rank == 0:
        eng = net._engine(4)
        roof = None
        extra = {"model_algorithmic_tflops": model_ref_flops_per_patch() * value / world / 1e12}
        if args.full:
            # ---- dominant kernel: EdgeConv (units 2..5 share one kernel); live HIP-event timing on the launch stream
            prof = prof_stages
            T = args.batch * args.npoint
            ec_ms = prof["edgeconv5"]                       # C=128 unit (the last one: never fused with a P|Q GEMM): avg ms per launch
            ec_fl = edgeconv_ref_flops(T, 128, 32, 4, 128)
            knn_ms = prof["knn"]
            knn_bytes = T * (3 * 4 + 16 * 4)               # 155 648 B per 2048-pt patch
            # (kernel, pipe peak, MFMAs executed per point, flops per MFMA, MFMAs per point that are not split overhead)
            KERNELS = {
                "f16n": ("edgeconv4_kernel<P=1,NW=16> (units 2-5, split-fp16 natural-scale low half, v_mfma_f32_16x16x32_f16)",
                         "edgeconv4_kernel", BF16_MFMA_PEAK_TF, 132, 16384.0, 44),
                "f32": ("edgeconv_kernel<GB=2,NCONV=4,ODIM=128> (units 2-5, v_mfma_f32_16x16x4_f32)",
                        "edgeconv_kernel<2, 4, 128", FP32_MFMA_PEAK_TF, 352, 2048.0, 352),
            }
            kname, kprefix, peak, n_mfma, fl_mfma, n_useful = KERNELS[eng.ec_mode]
            ec_exec = T * n_mfma * fl_mfma                  # MFMA flops actually issued per launch
            # roofline.frac = EXECUTED matrix flops / dense peak of the pipe the kernel runs on (= MFMA utilisation at the
            # nominal 2.4 GHz; rocprof's SQ_VALU_MFMA_BUSY_CYCLES / GRBM_GUI_ACTIVE gives the same ratio at the clock held).
            # The reference-formulation figure (2 x 16 x 120 832 MAC per point, 5.4x what the P/Q fold leaves to
            # execute) is kept as algorithmic_vs_fp16_peak; useful_frac discounts the split overhead as well (one of the
            # three fp16 MFMAs of a product is "the" product, the other two buy fp32 accuracy).
            roof = {"bound": "mfma", "kernel": kname,
                    "achieved": ec_exec / (ec_ms * 1e-3) / 1e12, "peak": peak, "unit": "TFLOP/s",
                    "frac": ec_exec / (ec_ms * 1e-3) / 1e12 / peak, "traffic": None,
                    "flops_basis": f"executed: {n_mfma} MFMAs x {int(fl_mfma)} flop per point x {T} points per launch; live HIP-event "
                                   "duration on the launch stream",
                    "useful_frac": ec_exec / (ec_ms * 1e-3) / 1e12 / peak * n_useful / n_mfma,
                    "algorithmic_tflops": ec_fl / (ec_ms * 1e-3) / 1e12,
                    "algorithmic_vs_fp16_peak": ec_fl / (ec_ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TF,
                    "avg_launch_ms": ec_ms}
            # HBM traffic and the profiler's own duration of the dominant kernel: PMC counters are collected offline with
            # rocprofv3 (bench.py cannot run under --pmc and time itself); the committed summary of the same command is read
            # back here so that every number of this object can be recomputed from profiles/ alone.
            try:
                with open(os.path.join(ROOT, "profiles", "pmc_latest.json")) as f:
                    pmc = json.load(f)["kernels"]
                key = [k for k in pmc if k.startswith(kprefix)][0]
                roof["traffic"] = pmc[key].get("hbm_bytes_per_launch")
                roof["profile"] = {"file": "profiles/pmc_latest.json", "kernel": key, "avg_launch_ms": pmc[key].get("avg_us", 0.0) / 1e3,
                                   "mfma_util_pct": pmc[key].get("mfma_util_pct"), "shader_clock_ghz": pmc[key].get("shader_clock_ghz")}
                alg_bytes = T * (512 * 4 + 16 * 4 + 128 * 4)                     # P|Q row + 16 indices + the 128-channel output row, per point
                if roof["traffic"]:
                    roof["traffic_vs_algorithmic"] = roof["traffic"] / alg_bytes
                roof["traffic_note"] = ("bytes per launch at 32 x 2048 (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, gfx950 correction); "
                                        "algorithmic HBM bytes per launch = PQ 134.2 MB + idx 4.2 MB + out 33.6 MB; the measured figure is an UPPER bound: the x2 "
                                        "is calibrated for 16-B-per-lane loads only and half of this kernel's gathers are 4-B loads, and Infinity-"
                                        "Cache hits (the 134 MB table was written by the kernel before) are counted as traffic")
            except Exception:
                pass
            # kNN: north_star asks for HBM GB/s; the kernel is ALU/selection-bound by construction (216 flop/B), so the ALU fraction
            # is the meaningful roofline.  knn5_kernel (csrc/knn.hip) runs its two sweeps as v_mfma_f32_16x16x4_f32 - 256 pairs per
            # instruction at 32 cycles per SIMD, i.e. the rate of the vector FMA lanes (64 FLOP / clk / SIMD: the f32 MFMA does not
            # add throughput over VALU, it replaces 6 operations per pair by 2 lane-slots) - plus 0.5 (v_min3, sweep A) and 1
            # (v_alignbit, sweep B) VALU lane-slots per pair: 5.5 executed lane-slots per pair against 1024 SIMDs x 16 lanes x 2.4 GHz
            # = 39.3 T lane-ops/s.  The appends and the exact ranking of the ~22 survivors per query are not counted: the fraction
            # is sweep arithmetic over the whole kernel time (knn4_kernel, the VALU form it replaced at this shape: 13 per pair).
            pair_evals = float(args.batch) * args.npoint * args.npoint
            knn5 = args.batch * ((args.npoint + 63) // 64) >= 1024 and args.npoint <= 4096
            slots = 5.5 if knn5 else 13.0
            roof_knn = {"kernel": "knn5_kernel<16> (f32-MFMA filter sweeps + exact ranking)" if knn5 else "knn4_kernel<16>", "bound": "valu",
                        "avg_launch_ms": knn_ms,
                        "hbm": {"achieved": knn_bytes / (knn_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                "frac": knn_bytes / (knn_ms * 1e-3) / 1e9 / HBM_PEAK_GBS},
                        "valu": {"pair_evals": pair_evals, "lane_slots_per_pair": slots, "achieved": pair_evals * slots / (knn_ms * 1e-3) / 1e12,
                                 "peak": 39.3, "unit": "T lane-ops/s", "frac": pair_evals * slots / (knn_ms * 1e-3) / 1e12 / 39.3}}
            extra.update({"stage_ms": prof, "roofline_knn": roof_knn})
        if el_pipe and patches / el_pipe > value:           # reported only when two steps in flight actually beat the headline on this box
            extra["pipelined"] = {"steps_in_flight": 2, "value": patches / el_pipe, "unit": "patches/s",
                                  "ms_per_step": el_pipe / args.steps * 1e3,
                                  "note": "secondary, never `value`: the same K steps replayed from two captured graphs on two "
                                          "streams, so consecutive (independent) batches overlap on the device"}
        if launch_probe:
            extra["launch_probe"] = launch_probe
        if el_zc:
            extra["zero_copy_input"] = {"value": patches / el_zc, "unit": "patches/s", "ms_per_step": el_zc / args.steps * 1e3,
                                        "note": "secondary, never `value`: one K-step pass with the batch written into the graph's own "
                                                "input buffer beforehand (PointInterpFlow.graphed: run.input), i.e. without the device-to-device "
                                                "copy that `value`'s step carries in front of every replay"}
        cpu = None
        if world == 1 and not args.no_cpu_baseline and args.full:
            from oracle import ref_cpu as O
            # cores this process may actually use (the GPU box exposes 256 logical CPUs but a one-GPU
            # job owns a 16-core share; oversubscribing torch's pool makes the baseline meaninglessly slow)
            try:
                ncpu = len(os.sched_getaffinity(0))
            except AttributeError:
                ncpu = os.cpu_count() or 1
            ncpu = max(1, min(ncpu, int(os.environ.get("PF_CPU_THREADS", "16"))))
            torch.set_num_threads(ncpu)
            bs = 2
            xs = xyz_cpu[:bs]
            O.forward(sd, xs, 4)                        # warm-up
            n, t1 = 0, time.perf_counter()
            while True:
                xr, lr = O.forward(sd, xs, 4)
                n += 1
                if time.perf_counter() - t1 > args.cpu_seconds:
                    break
            cel = time.perf_counter() - t1
            cpu = {"value": bs * n / cel, "unit": "patches/s", "cores": ncpu, "kind": "port",
                   "sample": f"{n} forwards of {bs} x {args.npoint}-pt patches, fp32 torch-CPU oracle (oracle/ref_cpu.py)"}
            # SURVEY 8(d) parity report, on the same sample the CPU baseline just computed (checker use of the oracle)
            from puflow_amd import ops
            err = (x[:bs].cpu() - xr).abs().max().item()
            _, i_ref = O.knn_canonical(xs, xs, 16)
            knn_match = (eng.knn(xyz[:bs]).cpu().long() == i_ref).float().mean().item()
            st_b = net.forward_stages(xyz[:bs], 4)
            st_o = O.forward(sd, xs, 4, stages=True)
            ld_rel = ((st_b["ldj"].cpu() - st_o["ldj"]).abs() / st_o["ldj"].abs()).max().item()
            xr_d = xr.to(dev)
            cd_bo = ops.history_chamfer_distance(x[:bs].contiguous(), xr_d).max().item()     # CD(build, oracle)
            gt = synth_patches(bs, 4 * args.npoint, seed=7, surface=True).to(dev)            # a common target cloud
            cd_diff = (ops.history_chamfer_distance(x[:bs].contiguous(), gt)
                       - ops.history_chamfer_distance(xr_d, gt)).abs().max().item()
            extra["parity"] = {"max_abs_dx_vs_oracle": err, "knn_idx_exact_match_rate": knn_match,
                               "max_rel_err_log_det": ld_rel, "cd_build_vs_oracle": cd_bo,
                               "abs_cd_diff_vs_common_target": cd_diff,
                               "logp_note": "logp is a batch mean; compared in tests on equal batches"}
        reduced_lib = os.environ.get("PF_LIB_PATH", "").endswith("_f16.so")
        if world == 1 and not args.no_cpu_baseline and not args.no_reduced and not reduced_lib and args.full:
            extra["reduced_precision"] = reduced_precision_line(args)
        out = {"metric": "patches/sec x4 2048->8192 (PU1K discrete, eval)", "value": value, "unit": "patches/s",
               "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": el / args.steps * 1e3,
               "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
               # the arithmetic the path computes in: fp32 values, each product as 2-term split-fp16 on the fp16 MFMA
               # with fp32 accumulation (PF_EC_MODE=f32: plain f32 MFMA in the 128-channel EdgeConv units)
               "dtype": "f16 operands (ONE fp16 MFMA product per step, fp32 accumulate): reduced-precision throughput build" if reduced_lib else
                        "f32 (split-fp16 MFMA products, fp32 accumulate)" if eng.ec_mode == "f16n" else
                        "f32 (f32 MFMA EdgeConv, split-fp16 elsewhere)",
               "data": "synthetic",
               "config": {"workload": "BASELINE configs[1]: PU1K discrete x4 inference, 32 x 2048-pt patches per GPU "
                                      "(fp32-parity mode)", "arithmetic": "fp32 inputs, accumulators and results; the dense layers run as 2-term split-fp16 "
                          "products on the fp16 MFMA pipe (hi.hi + hi.lo + lo.hi, fp32-class accuracy: parity tests hold the "
                          "same 1e-5 bar; PF_EC_MODE=f32 selects the bit-exact f32-MFMA EdgeConv kernels)", "launch": ("hipGraph replay (one launch per step" + (", batch resident in the graph's input buffer: PF_BENCH_ZERO_COPY=1)" if zero_copy else ", behind a device-to-device copy of the batch into the graph's input buffer)") + (f", {pipe} steps in flight on {pipe} streams" if pipe > 1 else "")) if headline_graph else "eager (one stream, one launch per kernel - the graph's kernels in the graph's order - the caller's tensor read in place)",
                          "patches_per_gpu": args.batch, "total_batch": args.total_batch if args.scaling == "strong" else world * args.batch,
                          "npoint": args.npoint,
                          "upratio": 4, "sharding": f"patch batch over {world} rank(s), no data-path collective",
                          "collectives": args.collectives},
               "roofline": roof, "cpu_baseline": cpu}
        out.update(extra)
        if strong is not None:
            out["strong"] = strong
        if coll is not None and out["config"].get("collectives") is not None:
            out["config"]["collectives"] = dict(out["config"]["collectives"], **coll)
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.destroy_process_group()


def collectives_probe(args, world, rank, dev, dist):
    """What the first multi-GPU run should say about itself: the size of the communicator as the first
    all-reduce saw it (checked at start-up), the latency of the training step's ONE collective - an all-reduce of the flat
    806 103-float gradient bucket, 10 timed calls - and, for RCCL, the transports its rings use, parsed from rank 0's
    NCCL_DEBUG=INFO log.  Every rank runs this (the all-reduces are collective); rank 0 returns the dict."""
    n = 806103
    buf = torch.ones(n, dtype=torch.float32, device=dev)
    for _ in range(3):
        dist.all_reduce(buf)
    torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
    ts = []
    for _ in range(10):
        t0 = time.perf_counter()
        dist.all_reduce(buf)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    t = torch.tensor([sorted(ts)[len(ts) // 2], max(ts)], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    info = {"communicator_ranks_seen_by_first_all_reduce": args.gpus,
            "gradient_bucket_all_reduce": {"floats": n, "bytes": 4 * n, "median_us": float(t[0]) * 1e6, "max_us": float(t[1]) * 1e6,
                                           "calls": 10, "note": "host wall time per call incl. synchronisation, max over ranks"}}
    log = getattr(args, "rccl_log", None)
    if rank == 0 and log:
        tr = {"P2P": 0, "SHM": 0, "NET": 0}
        other = []
        try:
            import glob
            for fn in glob.glob(log + "*"):
                for line in open(fn, errors="replace"):
                    if " via " in line:
                        for k in tr:
                            if f"via {k}" in line:
                                tr[k] += 1
                    if ("xGMI" in line or "XGMI" in line or "Rings" in line or "nChannels" in line or "RCCL version" in line or
                            "NCCL version" in line) and len(other) < 6:
                        other.append(line.strip()[-160:])
            info["rccl"] = {"channel_connections_by_transport": tr, "log_excerpt": other,
                            "source": "NCCL_DEBUG=INFO (INIT, GRAPH) of rank 0, NCCL_DEBUG_FILE; P2P = direct peer access (xGMI inside a node)"}
        except Exception as ex:
            info["rccl"] = {"failed": f"{type(ex).__name__}: {ex}"[:200]}
    return info


def strong_block(args, world, rank, dev, dist, net, totals=(32, 256)):
    """The SAME ranks re-timed with a fixed TOTAL batch split over them (contiguous shards, no collective on the data path):
    one `--gpus N` invocation then yields the weak figure (`value`) and the strong ones.  A rank whose shard is empty only
    joins the barriers.  Returns {total: {...}} on rank 0."""
    from puflow_amd.dist import shard_bounds
    from puflow_amd.weights import synth_patches
    out = {}
    for total in totals:
        lo, hi = shard_bounds(total, rank, world)
        bs = hi - lo
        run = xyz_s = None
        if bs > 0:
            xyz_s = synth_patches(bs, args.npoint, seed=4000 + total + rank).to(dev)
            try:
                run = net.graphed(bs, args.npoint, 4)
            except Exception:
                run = lambda inp: net(inp, 4)
        steps, warm = max(args.steps, 20), max(min(args.warmup, 10), 3)

        def one_pass(fn):
            for _ in range(warm):
                if fn is not None:
                    fn(xyz_s)
            torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                if fn is not None:
                    fn(xyz_s)
            torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
            t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())
        # both launch modes (same kernels, same bits), each a full barrier-bracketed pass with the max over ranks; the faster one is
        # the figure, both are in the line (small shards: an eager step has no input copy and no gap between two graph launches)
        el_g = one_pass(run)
        el_e = one_pass(None if run is None else (lambda inp: net(inp, 4)))
        el = min(el_g, el_e)
        out[str(total)] = {"total_batch": total, "patches_per_rank": [shard_bounds(total, r, world)[1] - shard_bounds(total, r, world)[0] for r in range(world)],
                           "value": total * steps / el, "unit": "patches/s", "ms_per_step": el / steps * 1e3, "steps": steps,
                           "launch": "graph" if el_g <= el_e else "eager",
                           "ms_per_step_graph_replay": el_g / steps * 1e3, "ms_per_step_eager": el_e / steps * 1e3,
                           "scaling": "strong"}
        del run, xyz_s
    return out


def self_launch(n: int) -> int:
    """`python bench.py --gpus N` with no launcher around it: run the same command line under torch.distributed.run as N
    FRESH child processes (one rank per GPU, RCCL), started before this process has touched the GPU - no exec of a process
    that initialised the device, no fork after it.  Rank 0's JSON line passes through on stdout; the exit code is the
    launcher's."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")        # dmabuf IPC: RCCL across processes needs it on this host driver
    env.setdefault("OMP_NUM_THREADS", "4")
    print("[bench] --gpus %d without WORLD_SIZE: launching %s" % (n, " ".join(cmd)), file=sys.stderr, flush=True)
    rc = subprocess.call(cmd, env=env)
    if rc != 0:
        raise SystemExit(rc)
    return 0


def reduced_precision_line(args):
    """BASELINE configs[1] also names a bf16 / fp16 run: the same workload on `libpuflow_hip_f16.so` (one fp16 MFMA product
    per 32-channel step instead of the three of the fp32-parity arithmetic; operands rounded to fp16, fp32 accumulation),
    measured in a CHILD process (the library is chosen at load time) and judged by Chamfer distance against the CPU oracle.
    A secondary line - never `value`."""
    import subprocess
    from puflow_amd.build import LIB_F16
    if not os.path.exists(LIB_F16):
        return {"skipped": "libpuflow_hip_f16.so not built (python -m puflow_amd.build)"}
    env = dict(os.environ, PF_LIB_PATH=LIB_F16)
    cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(min(args.steps, 100)), "--warmup", str(min(args.warmup, 10)),
           "--batch", str(args.batch), "--npoint", str(args.npoint), "--cpu-seconds", "3", "--no-reduced", "--full"]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        d = json.loads(line)
    except Exception as ex:                                                  # the headline must not depend on this leg
        return {"failed": f"{type(ex).__name__}: {ex}"[:200]}
    par = d.get("parity", {})
    return {"value": d["value"], "unit": d["unit"], "ms_per_step": d["ms_per_step"], "dtype": d["dtype"],
            "library": "puflow_amd/libpuflow_hip_f16.so (-DPF_MMN_TERMS=1)",
            "max_abs_dx_vs_fp32_oracle": par.get("max_abs_dx_vs_oracle"),
            "cd_build_vs_fp32_oracle": par.get("cd_build_vs_oracle"),
            "abs_cd_diff_vs_common_target": par.get("abs_cd_diff_vs_common_target"),
            "knn_idx_exact_match_rate": par.get("knn_idx_exact_match_rate"),
            "note": "same kernels, launches and weights as the headline; only the number of fp16 products per step differs"}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, arrays):
    """--dump-outputs: one DIR/<name>.npy per array the timed path returned in its last step, float64 kept, everything else as
    float32.  If the arrays exceed DUMP_LIMIT_BYTES together, each one over its equal share of the limit is replaced by the
    elements at a fixed, seeded, sorted sample of its flat indices (the same for the same shape), so that two builds run with
    the same arguments can still be compared element for element."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    arrs = {}
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        arrs[name] = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
    if sum(a.nbytes for a in arrs.values()) > DUMP_LIMIT_BYTES:
        share = DUMP_LIMIT_BYTES // len(arrs)
        for name, a in arrs.items():
            if a.nbytes > share:
                keep = share // a.itemsize
                idx = np.sort(np.random.default_rng(2021).choice(a.size, size=keep, replace=False))
                arrs[name] = a.reshape(-1)[idx]
    for name, a in arrs.items():
        np.save(os.path.join(dirname, name + ".npy"), a)
    return arrs


def _ncpu():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, int(os.environ.get("PF_CPU_THREADS", "16"))))


# executed MACs per EDGE of one 128-channel EdgeConv unit's backward (pf_ec_train_bwd, C = 128, g = 32, 4 growth layers,
# odim 128; csrc/train_fused.hip): conv_out dA 128 x 128, growth dA 32 x (32 + 64 + 96), all weight gradients
# [S, GT] = 6144 + 128 x 128, and the two P|Q GEMMs (dx, dWpq: 2 x 512 x 128 per POINT = / 16 per edge)
EC_BWD_MAC_PER_EDGE = 128 * 128 + 32 * (32 + 64 + 96) + (32 * (32 + 64 + 96) + 128 * 128) + 2 * 512 * 128 // 16


def bench_train(args, world, rank, dev, dist):
    """BASELINE configs[2]: training step on 32 x (256 -> 1024) patches per GPU, loss 1e-4 logp + 5e-2 EMD(eps .005,
    50 it) + 1e-1 CD (train_pugan.py:59-61), grad all-reduce (one 3.2 MB RCCL bucket), clip 1e-2, Adam 1e-3."""
    use_dist = args.use_dist
    from puflow_amd.trainer import TrainerModule, default_cfg
    from puflow_amd.weights import synth_patches, synth_state_dict
    from puflow_amd.dist import broadcast_module
    # rehearsal on one GPU (several ranks share the device): one EMD workgroup per sample - the multi-workgroup auction's grid
    # barriers assume this process's workgroups are co-resident (csrc/emd.hip)
    shared = os.environ.get("PF_BENCH_SINGLE_DEVICE") == "1" and world > 1
    syncbn = os.environ.get("PF_BENCH_SYNCBN") == "1"      # BatchNorm statistics over all ranks (cfg.sync_batchnorm) on the fused kernels
    det_env = os.environ.get("PF_BENCH_DETERMINISTIC") == "1"   # cfg.deterministic: bit-reproducible steps (tests; slower)

    def fresh_module(det=None):
        m = TrainerModule(default_cfg(learning_rate=1e-3, emd_workgroups=1 if shared else 0, sync_batchnorm=syncbn,
                                      deterministic=det_env if det is None else det), loss_mix="pugan")
        m.network.load_state_dict(synth_state_dict(2021))
        if os.environ.get("PF_BENCH_ACTNORM_INITED") == "1":
            # tests only: skip ActNorm's data-dependent first-batch init (the multi-rank path runs it as an extra forward + a
            # broadcast, the one-process path inside the first step: different kernels, different rounding) so that a forced
            # one-rank group and the plain path take literally the same steps
            m.network.set_to_initialized_state()
        return m.to(dev)
    sd = synth_state_dict(2021)
    dense_cpu = (synth_patches(args.batch, 1024, seed=2021 + rank) + 1) / 2                # [0,1] for the EMD
    dense = dense_cpu.to(dev)
    sparse = dense[:, ::4].contiguous()
    batch = (sparse, dense, torch.ones(args.batch, device=dev))

    def step_grads(det=None, full_loss=False):
        """Gradients of ONE benchmark step (train-mode forward, loss, backward; no update) from the benchmark's initial state.
        The loss is the step's WITHOUT the EMD term (1e-4 logp + 1e-1 CD): the auction's assignment is a discrete, chaotic
        function of the prediction - a 1e-6 change of x re-assigns points and moves the EMD gradient by percents, which would
        bury what this leg measures (the arithmetic of the backward kernels); the EMD backward itself is 2 g (x - y), no
        matrix product."""
        from puflow_amd import ops
        m = fresh_module(det)
        m.train()
        if full_loss:                                        # the step's own loss, EMD term included (TrainerModule.training_step)
            loss = m.training_step(batch, 0)
        else:
            x, logp = m(sparse, upratio=4)
            cd, _ = ops.chamfer_distance(x, dense)
            loss = logp * 1e-4 + cd * 1e-1
        loss.backward()
        torch.cuda.synchronize()
        return {k: (p.grad.detach().cpu().clone() if p.grad is not None else torch.zeros_like(p).cpu()) for k, p in m.named_parameters()}, float(loss)

    if args.dump_grads:
        g, l = step_grads()
        torch.save({"grads": g, "loss": l}, args.dump_grads)
        return
    tm = fresh_module()
    broadcast_module(tm)
    opt = tm.configure_optimizers()["optimizer"]

    def barrier():
        if use_dist:
            dist.barrier()

    # the step is replayed from hipGraphs by default (forward + loss + backward [+ all-reduce between two graphs] + clip + Adam:
    # same kernels, same order; PF_BENCH_GRAPH=0 times the eager launches)
    step = lambda b: tm.train_step(b, opt)
    graphed = False
    if os.environ.get("PF_BENCH_GRAPH", "1") == "1":
        try:
            step = tm.graphed_train_step(batch, opt)
            graphed = True
        except Exception as ex:
            print(f"[bench] training-step capture failed ({type(ex).__name__}: {ex}); timing the eager step", file=sys.stderr)
    for _ in range(args.warmup):
        step(batch)
    torch.cuda.synchronize(); barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step(batch)
    torch.cuda.synchronize(); barrier(); torch.cuda.synchronize()
    el = time.perf_counter() - t0
    grad_norm_last = float(opt.coef[1]) if hasattr(opt, "coef") else None      # of the last TIMED step (the call profile below runs more)
    tm.check_device_status()                      # EMD barrier time-outs raise, NaN substitutions of the captured steps are printed
    if args.dump_outputs and rank == 0:           # the last timed step's loss and the parameters it left (flat, in named_parameters order)
        dump_outputs(args.dump_outputs, {"loss": loss, "parameters": torch.cat([p.detach().reshape(-1).float() for p in tm.parameters()])})
    t = torch.tensor([el], dtype=torch.float64, device=dev)
    if use_dist:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    el = float(t.item())
    roof = cpu = grad_parity = None
    # ---- dominant launch group, timed live: HIP events around every C-ABI call of three EAGER steps (the same kernels
    # the graph replays).  The step is ~440 launches of 5 - 100 us; the largest share belongs to the backward of the
    # 128-channel EdgeConv units (pf_ec_train_bwd: conv_out / growth dA, one split-K launch for all weight gradients, the
    # neighbour scatter, two P|Q GEMMs), priced against the fp32 matrix pipe it runs on (v_mfma_f32_16x16x4_f32).
    # Every rank runs these steps (they contain the gradient all-reduce); rank 0 reports.
    if args.full:
        from puflow_amd._prof import profile_calls
        with profile_calls() as prof:
            for _ in range(3):
                tm.train_step(batch, opt)
            torch.cuda.synchronize()
        barrier()
        if rank == 0:
            tab = prof.table()
            calls_ms = {k: v[1] / 3 for k, v in sorted(tab.items(), key=lambda kv: -kv[1][1])[:8]}
            evs = prof.events.get("pf_ec_train_bwd", [])
            ms = sorted(a.elapsed_time(b) for a, b in evs)
            if ms:
                big = ms[len(ms) // 2:]                                        # 7 units per step: the upper half are the four 128-channel ones
                ec_ms = sum(big) / len(big)
                E = args.batch * 256 * 16
                flops = 2.0 * EC_BWD_MAC_PER_EDGE * E
                persist = getattr(tm.network, "train_persistent", False) and os.environ.get("PF_TRAIN_PERSIST", "1") != "0"
                roof = {"bound": "mfma", "kernel": "pf_ec_train_bwd of a 128-channel EdgeConv unit (csrc/train_fused.hip: " +
                                                 ("ec_bwdp_kernel - the dense block's backward as one persistent launch with a grid barrier per "
                                                  "BatchNorm layer - " if persist else "ec_bwdg16_kernel x4, ec_bwd0_kernel, ") +
                                                 "ec_pq_bwd_csr_kernel, ec_dw3_kernel, two gemm2_kernel, ec_assemble_kernel)",
                        "achieved": flops / (ec_ms * 1e-3) / 1e12, "peak": FP32_MFMA_PEAK_TF, "unit": "TFLOP/s",
                        "frac": flops / (ec_ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TF, "traffic": None, "avg_launch_ms": ec_ms,
                        "flops_basis": f"algorithmic: {EC_BWD_MAC_PER_EDGE} MAC per edge x {E} edges per call, each product once (split-bf16 "
                                       "products: three v_mfma_f32_16x16x32_bf16 / 32x32x16_bf16 each; the two point GEMMs on v_mfma_f32_16x16x4_f32); live HIP-event duration of the call's launches on the launch stream",
                        "calls_ms_per_step": calls_ms}
                # HBM bytes of the same call from the committed PMC summary of the training kernels (collected offline over eager
                # steps: tools/pmc_cmd.sh + tools/train_eager_steps.py): the launches of one 128-channel unit's backward
                try:
                    with open(os.path.join(ROOT, "profiles", "pmc_train_latest.json")) as f:
                        pk = json.load(f)
                    pk = pk.get("kernels", pk)
                    if "gemm2_kernel<2, 2, 1, 1>" in pk:                      # both point GEMMs of the call on 32 x 32 tiles (end of round 5)
                        gemms = {"gemm2_kernel<2, 2, 1, 1>": 2}
                    elif "gemm2_kernel<2, 2, 2, 2>" in pk:
                        gemms = {"gemm2_kernel<2, 2, 2, 2>": 2}
                    else:
                        gemms = {"gemm_kernel<2, 2, 2, 2, true>": 2}          # before round 5
                    group = {"ec_pq_bwd_csr_kernel": 1, "ec_dw3_kernel": 1, **gemms, "ec_assemble_kernel": 1}
                    if "gemm_reduce_kernel" in pk:                            # (until ec_assemble_kernel took over dWpq's slab sums)
                        group["gemm_reduce_kernel"] = 1
                    group.update({"ec_bwdp_kernel<32, 4, 128>": 1} if persist else {"ec_bwdg16_kernel<2, 0>": 4, "ec_bwd0_kernel": 1})
                    tot, us = 0.0, 0.0
                    for k, n in group.items():
                        tot += n * pk[k]["hbm_bytes_per_launch"]
                        us += n * pk[k]["avg_us"]
                    alg = E * 128 * 4 * (1 + 1 + 1) + 8192 * (256 + 512 + 128) * 4      # Y, dA read once, dA written once; dh, dPQ, dx
                    roof["traffic"] = tot
                    roof["traffic_vs_algorithmic"] = tot / alg
                    roof["profile"] = {"file": "profiles/pmc_train_latest.json", "kernels": group, "sum_avg_us": us,
                                       "note": "FETCH_SIZE x2 + WRITE_SIZE per launch (gfx950 correction), summed over the call's launches; "
                                               "algorithmic bytes = the [E, 128] growth outputs and their gradient read once and the "
                                               "gradient written once + the per-point tensors; layer s of the dense block reads the gradient columns of every later layer (gather form), "
                                               "ec_dw and the dPQ sums read the whole tensor again"}
                except Exception:
                    pass
            if world == 1 and not args.no_cpu_baseline:
                cpu = train_cpu_baseline(sd, dense_cpu, args.cpu_seconds)
            if world == 1 and not args.no_grad_parity:
                grad_parity = train_grad_parity(args, step_grads)
    if use_dist:
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"metric": "training patches/sec (256->1024 patches, CD+EMD loss, grad all-reduce)",
                          "value": world * args.batch * args.steps / el, "unit": "patches/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": el / args.steps * 1e3,
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                          # what the step computes in, said in full: fp32 values everywhere; the matrix products of the dominant
                          # kernels are NOT plain fp32 products
                          "dtype": "f32 values and accumulators; forward products f32 MFMA (growth layers, MLPs, flow chains) and split-fp16 "
                                   "(EdgeConv conv_out: hi + lo*2^-11, 22+ mantissa bits); BACKWARD products of the EdgeConv units split-bf16 "
                                   "(hi + mid: 16 mantissa bits per operand, fp32 exponent range, three bf16 MFMAs per product, fp32 "
                                   "accumulate), all other backward products f32 MFMA - narrower than the reference's fp32 in the EdgeConv "
                                   "backward; measured against the f32-product build in `grad_parity`",
                          "grad_parity": grad_parity,
                          "data": "synthetic", "loss": float(loss),
                          # global gradient norm (before clipping) of the last step, as the fused optimizer's norm kernel saw it:
                          # after the gradient all-reduce when ranks > 1 (or the forced one-rank path)
                          "grad_norm_last_step": grad_norm_last,
                          "config": {"workload": "BASELINE configs[2]: discrete x4 training step, 32 x (256->1024) patches per GPU",
                                     "loss": "1e-4 logp + 5e-2 EMD(eps .005, 50 it) + 1e-1 CD", "optimizer": "Adam 1e-3, clip 1e-2",
                                     "deterministic": bool(det_env),
                                     "launch": ("hipGraph replay (graph A: forward + loss + backward + gradient packing; eager all-reduce of the flat "
                                                "gradient bucket; graph B: clip + Adam)" if use_dist else "hipGraph replay") if graphed else "eager",
                                     "collectives": args.collectives, "sync_batchnorm": syncbn,
                                     "patches_per_gpu": args.batch, "sharding": f"patch batch over {world} rank(s); one RCCL "
                                     "all-reduce of the flat 806 103-float gradient per step"},
                          "roofline": roof, "cpu_baseline": cpu}), flush=True)


def train_grad_parity(args, step_grads):
    """How far the default build's gradients (split-bf16 / split-fp16 products in the EdgeConv units' kernels) are from the SAME
    kernels on plain f32 MFMA products, loaded in child processes (the library is chosen at load time):
      backward_only : libpuflow_hip_bwdf32.so  = -DPF_EC_BWDG_F32 -DPF_EC_DW_F32 (the persistent dense-block backward, the per-layer
                      one of the interpolation unit and the weight-gradient kernel on f32 products; the forward is bit for bit the
                      default build's: what differs is the arithmetic of the backward kernels alone)
      all           : libpuflow_hip_gradf32.so = the above + -DPF_EC_FWD_F32 (conv_out forward on f32 products too: the forward
                      then differs by ~1e-6, which ill-conditioned gradients - max-pool routes, the flow's conditioning -
                      amplify; the difference to `backward_only` is that amplification, not backward arithmetic)
    One benchmark step's forward + loss + backward from the benchmark's initial state in each, every parameter gradient compared
    as max|g - g_ref| / max|g_ref| over its elements.  The step is not bit-reproducible from run to run (float atomics), so the
    same figure between two runs of the DEFAULT build is reported as the noise floor."""
    import subprocess
    import tempfile
    from puflow_amd.build import LIB_BWDF32, LIB_GRADF32
    ga, la = step_grads()
    gb, _ = step_grads()

    def child(lib):
        if not os.path.exists(lib):
            return None, f"{os.path.basename(lib)} not built (python -m puflow_amd.build)"
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "g.pt")
            cmd = [sys.executable, os.path.abspath(__file__), "--mode", "train", "--batch", str(args.batch), "--dump-grads", path]
            try:
                subprocess.run(cmd, env=dict(os.environ, PF_LIB_PATH=lib), capture_output=True, text=True, timeout=600)
                return torch.load(path), None
            except Exception as ex:
                return None, f"{type(ex).__name__}: {ex}"[:300]

    def compare(ref, tag):
        gr, lr = ref["grads"], ref["loss"]
        # a convolution bias in front of a BatchNorm layer has a mathematically ZERO gradient (the batch mean removes it): what
        # the kernels leave there is rounding residue, reported as an absolute figure; every other tensor relatively
        scale = {k: float(v.abs().max()) for k, v in gr.items()}
        gmax = max(scale.values())
        live = [k for k in gr if scale[k] > 1e-5 * gmax]
        dead = [k for k in gr if k not in live]
        ab = {k: float((ga[k] - gr[k]).abs().max()) / scale[k] for k in live}
        noise = {k: float((ga[k] - gb[k]).abs().max()) / scale[k] for k in live}
        worst = max(ab, key=ab.get)
        v, nv = sorted(ab.values()), sorted(noise.values())
        tot = float(torch.sqrt(sum((t.double() ** 2).sum() for t in gr.values())))
        dif = float(torch.sqrt(sum(((ga[k] - gr[k]).double() ** 2).sum() for k in gr)))
        dump = os.environ.get("PF_BENCH_GRAD_TABLE")
        if dump:
            with open(dump + "." + tag, "w") as fh:
                for k in gr:
                    fh.write(f"{k:70s} max|g_ref| {scale[k]:.3e}  ab {float((ga[k] - gr[k]).abs().max()):.3e}  noise {float((ga[k] - gb[k]).abs().max()):.3e}\n")
        return {"n_parameters": len(ab), "max": v[-1], "worst_parameter": worst, "p95": v[int(0.95 * (len(v) - 1))], "median": v[len(v) // 2],
                "flat_gradient_rel_l2": dif / tot,
                "run_to_run_noise_default_build": {"max": nv[-1], "p95": nv[int(0.95 * (len(nv) - 1))], "median": nv[len(nv) // 2]},
                "zero_gradient_tensors": {"n": len(dead), "max_abs_value_default": max([float(ga[k].abs().max()) for k in dead], default=0.0),
                                          "max_abs_value_reference": max([scale[k] for k in dead], default=0.0), "largest_gradient": gmax},
                "loss_values": [la, lr]}
    # ---- cfg.deterministic: two runs of the step's OWN loss (EMD term included) from the same state must agree to the bit, in
    # the loss and in every gradient element; next to it the same two runs of the default build (float / double atomics in
    # arrival order: a 1e-7 difference in x flips auction assignments and max-pool routes)
    def two_runs(det):
        g1, l1 = step_grads(det=det, full_loss=True)
        g2, l2 = step_grads(det=det, full_loss=True)
        gm = max(float(v.abs().max()) for v in g1.values())
        return {"loss": [l1, l2], "loss_bit_identical": l1 == l2, "gradients_bit_identical": all(torch.equal(g1[k], g2[k]) for k in g1),
                "max_abs_gradient_difference_over_largest_gradient": max(float((g1[k] - g2[k]).abs().max()) for k in g1) / gm}
    determinism = {"loss": "the step's loss 1e-4 logp + 5e-2 EMD / radius + 1e-1 CD, forward + backward, two runs from the same state",
                   "cfg.deterministic=True": two_runs(True), "default": two_runs(False)}
    out = {"determinism": determinism,
           "loss": "1e-4 logp + 1e-1 CD of the benchmark batch (the step's loss without the EMD term: the comparison is ACROSS BUILDS whose "
                   "forward differs by ~1e-6, and the auction's assignment is a discrete, chaotic function of x - that is not noise and "
                   "cfg.deterministic does not remove it)",
           "metric": "per parameter tensor: max|g - g_ref| / max|g_ref| over the tensor's elements; tensors whose reference gradient is <= 1e-5 of "
                     "the largest one (conv biases in front of BatchNorm: mathematically zero) are listed as absolute residue",
           "patches": args.batch}
    for tag, lib, what in (("backward_only", LIB_BWDF32, "-DPF_EC_BWDG_F32 -DPF_EC_DW_F32: f32 MFMA products in the EdgeConv backward and weight-gradient "
                                                         "kernels, forward identical to the default build"),
                           ("all", LIB_GRADF32, "-DPF_EC_BWDG_F32 -DPF_EC_DW_F32 -DPF_EC_FWD_F32: conv_out's forward on f32 products as well")):
        ref, err = child(lib)
        out[tag] = {"failed": err} if ref is None else dict(compare(ref, tag), reference=f"puflow_amd/{os.path.basename(lib)} ({what}), child process")
    return out


def train_cpu_baseline(sd, dense_cpu, seconds):
    """The training step of the CPU oracle (oracle/ref_cpu.py::forward_train under autograd + Chamfer + the numpy auction of
    oracle/emd_ref.py with the assignment frozen, loss and backward; no optimizer update) on 2 patches, repeated for about
    `seconds`."""
    import numpy as np
    from oracle import emd_ref, ref_cpu as O
    ncpu = _ncpu()
    torch.set_num_threads(ncpu)
    bs = 2
    dense = dense_cpu[:bs].contiguous()
    sparse = dense[:, ::4].contiguous()

    def one():
        sdr = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.clone()) for k, v in sd.items()}
        x, logp, _ = O.forward_train(sdr, sparse, 4, actnorm_init=False)
        d1, _, d2, _ = O.chamfer_nn(x, dense)
        cd = d1.mean(1).mean() + d2.mean(1).mean()
        _, assign = emd_ref.emd_forward(x.detach().numpy(), dense.numpy(), 0.005, 50)
        tgt = torch.gather(dense, 1, torch.from_numpy(np.asarray(assign)).long().clamp_min(0).unsqueeze(-1).expand(-1, -1, 3))
        emd = ((x - tgt) ** 2).sum()
        loss = logp * 1e-4 + emd * 5e-2 + cd * 1e-1
        loss.backward()
        return float(loss)

    one()
    n, t1 = 0, time.perf_counter()
    while True:
        one()
        n += 1
        if time.perf_counter() - t1 > seconds:
            break
    cel = time.perf_counter() - t1
    return {"value": bs * n / cel, "unit": "patches/s", "cores": ncpu, "kind": "port",
            "sample": f"{n} training steps (forward + CD + EMD + backward, no optimizer update) of {bs} x (256 -> 1024)-pt patches, "
                      "fp32 torch-CPU oracle (oracle/ref_cpu.py::forward_train, oracle/emd_ref.py)"}


# MFMAs per 16-row tile and right-hand-side evaluation of the continuous model (csrc/cnf.hip: 64 -> 64 forward, its transpose
# for the Hutchinson vector-Jacobian product, 64 -> 3): 24 + 24 + 6 split-fp16 products
CNF_MFMA_PER_EVAL = 54


def bench_cnf(args, world, rank, dev, dist):
    """BASELINE configs[4]: continuous (CNF) x4 inference, 32 x 2048-pt patches per GPU; every flow block is an ODE
    integrated by dopri5 (atol = rtol = 1e-5) with the step-size controller on the device.  Random-init weights make a
    trivial ODE (168 evaluations, no rejected step); the default synthetic workload takes the six integration end times of the
    reference's trained checkpoint and scales the ODE nets (`weights.CNF_PU1K_*`) so that the solver works as hard as on that
    checkpoint (462 evaluations, 62 accepted / 11 rejected steps) on a map that is as well-conditioned as the
    trained one - the evaluation / accept / reject counts of the timed forward and the float64 anchor are part of the line."""
    use_dist = args.use_dist
    from puflow_amd.cnf import PointInterpFlow as CnfFlow
    from puflow_amd.weights import CNF_PU1K_DYNAMICS, CNF_PU1K_END_TIMES, synth_cnf_state_dict, synth_patches
    from puflow_amd import _lib
    if args.cnf_dynamics is None:
        args.cnf_dynamics = CNF_PU1K_DYNAMICS
    end_times = CNF_PU1K_END_TIMES if args.cnf_end_times == "pu1k" else None
    sd = synth_cnf_state_dict(2021, dynamics=args.cnf_dynamics, end_times=end_times)
    net = CnfFlow(3)
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    B, N = args.batch, args.npoint
    # FOUR different input batches with their own Hutchinson vectors rotate through the timed loop: the forward is
    # enqueued without a look at a controller, with per-integration attempt budgets taken from the PREVIOUS forward - on one
    # repeated input those budgets are always exact and the fallback (discard the blind work behind the first integration that
    # ran out, re-integrate through the look-per-batch loop) never runs.  The line reports how often it did.
    NSETS = 4
    sets = []
    for k in range(NSETS):
        xc = synth_patches(B, N, seed=2021 + rank + 101 * k)
        g = torch.Generator().manual_seed(1000 * k + rank)
        nc = [torch.randn(B, N, 3, generator=g) for _ in range(6)]
        sets.append((xc, nc, xc.to(dev), [n.to(dev) for n in nc]))
    xyz_cpu, noise_cpu, xyz, noise = sets[0]

    def barrier():
        if use_dist:
            dist.barrier()

    for w in range(max(args.warmup, 1)):
        net(sets[w % NSETS][2], 4, noise=sets[w % NSETS][3])
    torch.cuda.synchronize(); barrier(); torch.cuda.synchronize()
    blind = {"forwards": 0, "ran_blind": 0, "fell_back": 0, "attempts_enqueued": 0, "attempts_taken": 0, "fallback_from": []}
    work = {"nfe": [], "accepted": [], "rejected": []}
    t0 = time.perf_counter()
    for st_i in range(args.steps):
        k = st_i % NSETS
        x, logp = net(sets[k][2], 4, noise=sets[k][3])
        bs_ = net.last_stats.get("blind", {})
        blind["forwards"] += 1
        blind["ran_blind"] += int(bool(bs_.get("ran")))
        blind["attempts_enqueued"] += int(bs_.get("attempts_enqueued", 0))
        blind["attempts_taken"] += int(bs_.get("attempts_taken", 0))
        if bs_.get("fallback_from") is not None:
            blind["fell_back"] += 1
            blind["fallback_from"].append(int(bs_["fallback_from"]))
        if st_i < NSETS:                                     # the solver's work on each of the input sets
            for kk in work:
                work[kk].append(int(net.last_stats[kk]))
    torch.cuda.synchronize(); barrier(); torch.cuda.synchronize()
    el = time.perf_counter() - t0
    stats = dict(per_input_set=work, blind=blind,
                 note="nfe / accepted / rejected of one forward on each of the 4 rotating input sets (a fallback counts the discarded "
                      "blind attempts' evaluations too); blind: forwards enqueued without a look at a controller, how many fell back "
                      "to the look-per-batch loop (and from which of the 12 integrations), step attempts enqueued vs taken")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"x": x, "logp": logp})
    t = torch.tensor([el], dtype=torch.float64, device=dev)
    if use_dist:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    el = float(t.item())
    roof = cpu = None
    extra = {}
    if rank == 0 and args.full:
        # ---- dominant kernel: one dopri5 step attempt (six fused right-hand-side evaluations) on the R-times replicated rows of
        # the inverse pass, timed THROUGH pf_cnf_steps - the entry point and kernel of the timed forward (cnf_step_dev_kernel with
        # the controller on the device; the round-4 line timed pf_cnf_step's host-stepped kernel instead): the block with the
        # longest integration, 12 attempts enqueued without a look, HIP events on the launch stream around them
        eng = net._engine(4)
        rows = B * N * 4
        got0 = net(xyz, 4, noise=noise, stages=True)
        ib = max(range(6), key=lambda i_: eng.T_end[i_])
        cflat = got0["cs"][ib].reshape(B * N, -1).contiguous()
        ctx = eng.context(ib, cflat)
        e = noise[ib].reshape(B * N, 3).contiguous().float()
        u0 = (got0["z"].reshape(B * N, 1, 3).expand(B * N, 4, 3).reshape(rows, 3) * 1.0).contiguous()
        ATT = 12
        eng.time_step_attempts(ib, u0, ctx, e, 4, True, 0, None, ATT, 4.0)
        tot_ms, real, finished = 0.0, 0, False
        for _ in range(3):
            ms_, real_, fin_ = eng.time_step_attempts(ib, u0, ctx, e, 4, True, 0, None, ATT, 4.0)
            tot_ms += ms_; real += real_; finished = finished or fin_
        st_ms = tot_ms / max(real, 1)
        flops = rows / 16 * 6 * CNF_MFMA_PER_EVAL * 16384.0
        traffic = None
        try:                                                 # committed PMC summary of the step kernels (tools/pmc_cmd.sh over tools/time_cnf.py)
            pm = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "pmc_cnf_latest.json")))
            ent = [v for k_, v in pm.get("kernels", {}).items() if "cnf_step_dev_kernel" in k_ and "hbm_bytes_per_launch" in v]
            if ent:
                ent = max(ent, key=lambda v: v.get("pct", 0.0))
                traffic = {"bytes_per_launch": ent["hbm_bytes_per_launch"], "profiled_avg_us": ent.get("avg_us"),
                           "source": "profiles/pmc_cnf_latest.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, FETCH_SIZE doubled per the "
                                     "gfx950 note; mean over the step kernel's launches of two forwards, no-op attempts included)"}
        except Exception:
            traffic = None
        roof = {"bound": "mfma", "kernel": "cnf_step_dev_kernel through pf_cnf_steps (csrc/cnf.hip: one Dormand-Prince step attempt = six fused "
                                         "right-hand-side evaluations incl. the Hutchinson vector-Jacobian product + the controller), inverse "
                                         f"pass of block {ib} (T = {eng.T_end[ib]:.3g}), rows = 4 B N",
                "achieved": flops / (st_ms * 1e-3) / 1e12, "peak": BF16_MFMA_PEAK_TF, "unit": "TFLOP/s",
                "frac": flops / (st_ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TF, "traffic": traffic, "avg_launch_ms": st_ms,
                "attempts_timed": {"enqueued": 3 * ATT, "real": real, "integration_finished": finished},
                "flops_basis": f"executed: 6 evaluations x {CNF_MFMA_PER_EVAL} fp16 MFMAs x 16384 flop per 16-row tile, {rows} rows per launch; "
                               "live HIP-event duration on the launch stream",
                "note": "the evaluation is bound by its 32 tanh + 32 sigmoid per lane on the transcendental unit, not by the matrix pipe "
                        "(DESIGN section 9): the MFMA fraction is reported because the contract asks for one of hbm | mfma"}
        if world == 1 and not args.no_cpu_baseline:
            from oracle import cnf_ref
            ncpu = _ncpu()
            torch.set_num_threads(ncpu)
            bs = 1
            xs, ns = xyz_cpu[:bs], [n[:bs] for n in noise_cpu]
            n_run, t1 = 0, time.perf_counter()
            while True:
                ref = cnf_ref.forward(sd, xs, 4, noise=ns, stages=True)
                n_run += 1
                if time.perf_counter() - t1 > args.cpu_seconds:
                    break
            cel = time.perf_counter() - t1
            cpu = {"value": bs * n_run / cel, "unit": "patches/s", "cores": ncpu, "kind": "port",
                   "sample": f"{n_run} forwards of {bs} x {N}-pt patch, fp32 torch-CPU oracle (oracle/cnf_ref.py: from-text dopri5)"}
            got = net(xyz[:bs], 4, noise=[n[:bs] for n in noise], stages=True)
            # the float64 anchor: the same oracle with every operation of the network and the solver in double.  The flow g
            # expands (|x| up to ~7 here): plain fp32 arithmetic already sits ~2e-3 from the fp64 result on this workload (the
            # trained checkpoint: 6e-4 on |x| < 0.8), so the HIP path is judged by its distance to fp64 next to the fp32 oracle's own
            r64 = cnf_ref.forward(sd, xs, 4, noise=ns, stages=True, dtype=torch.float64)
            anchor = {}
            for k in ("x", "z", "ldj"):
                sc = 1.0 if k != "ldj" else float(r64[k].abs().max())
                anchor[k] = {"hip_vs_f64": float((got[k].cpu().double() - r64[k]).abs().max()) / sc,
                             "oracle_f32_vs_f64": float((ref[k].double() - r64[k]).abs().max()) / sc}
            extra["parity"] = {"max_abs_dx_vs_oracle": float((got["x"].cpu() - ref["x"]).abs().max()),
                               "nfe": [int(got["nfe"]), int(ref["nfe"])], "accepted": [int(got["accepted"]), int(ref["accepted"])],
                               "rejected": [int(got["rejected"]), int(ref["rejected"])],
                               "fp64_anchor": dict(anchor, nfe_f64=int(r64["nfe"]), rejected_f64=int(r64["rejected"]),
                                                   note="max abs error against oracle/cnf_ref.py evaluated in float64 (ldj relative to "
                                                        "its largest value): HIP path next to the fp32 CPU oracle - both are the same "
                                                        "distance from fp64, i.e. the gap between them is the map's conditioning, "
                                                        "not the split-fp16 right-hand side"),
                               "note": "HIP vs oracle on the same patch and Hutchinson vectors; the solver's own tolerance is 1e-5 per "
                                       "integration, 12 chained integrations"}
    if use_dist:
        dist.destroy_process_group()
    if rank == 0:
        out = {"metric": "patches/sec x4 2048->8192 (PU1K continuous CNF, eval)", "value": world * B * args.steps / el, "unit": "patches/s",
               "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": el / args.steps * 1e3,
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "f32 (split-fp16 MFMA products, fp32 accumulate; solver state fp32, norms f64)", "data": "synthetic",
               "config": {"workload": "BASELINE configs[4]: continuous CNF x4 inference, 32 x 2048-pt patches per GPU",
                          "solver": "dopri5, atol = rtol = 1e-5, controller on the device", "ode_dynamics_scale": args.cnf_dynamics,
                          "ode_end_times": list(end_times) if end_times else [0.5] * 6,
                          "solver_work": stats, "patches_per_gpu": B, "npoint": N},
               "roofline": roof, "cpu_baseline": cpu}
        out.update(extra)
        print(json.dumps(out), flush=True)


def bench_pugan(args, world, rank, dev, dist):
    """BASELINE configs[3]: PU-GAN inference, clouds of 5000 points -> 20000 through the reference's patch pipeline
    (modules/utils/patch.py:35-110,142-165 + discrete/upsample.py:42-56): normalise -> FPS seeds (78) -> K = 256 kNN patches ->
    the network on 78 x 256-pt patches per cloud (x4) -> 99 840 candidates -> FPS merge 20 024 -> de-normalise -> drop 24
    outliers.  A step = `--batch` clouds per GPU through `PatchHelper.upsample` + `remove_outliers`, device-resident in and out;
    clouds are independent and sharded over ranks with no collective (the CLI shards files the same way)."""
    use_dist = args.use_dist
    import ctypes
    from puflow_amd import _lib, ops
    from puflow_amd.interpflow import PointInterpFlow
    from puflow_amd.patch import PatchHelper
    from puflow_amd.weights import synth_patches, synth_state_dict
    sd = synth_state_dict(2021)
    net = PointInterpFlow(3)
    net.load_state_dict(sd)
    net.set_to_initialized_state()
    net = net.to(dev).eval()
    B, N = args.batch, args.cloud_points
    NPATCH, UP, NOUT = 256, 4, 24
    n_patch = int(N / NPATCH * 4)
    npoint = N * UP + NOUT
    # clouds in world coordinates (scaled and shifted: the pipeline's own normalisation is part of the step)
    pc_cpu = synth_patches(B, N, seed=2021 + rank) * 2.0 + 0.7
    pc = pc_cpu.to(dev)
    ph = PatchHelper(NPATCH, 4)

    def barrier():
        if use_dist:
            dist.barrier()

    @torch.no_grad()
    def step():
        pred = ph.upsample(net, pc, npoint=npoint, upratio=UP, jitter=False)
        return PatchHelper.remove_outliers(pred, pc, NOUT)

    for _ in range(max(args.warmup, 1)):
        out = step()
    torch.cuda.synchronize(); barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    torch.cuda.synchronize(); barrier(); torch.cuda.synchronize()
    el = time.perf_counter() - t0
    t = torch.tensor([el], dtype=torch.float64, device=dev)
    if use_dist:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    el = float(t.item())
    assert tuple(out.shape) == (B, N * UP, 3)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"points": out})
    roof = cpu = None
    extra = {}
    if rank == 0 and args.full:
        lib = _lib.load()

        def ev_ms(fn, iters=3):
            fn(); torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                r = fn()
            b.record(); torch.cuda.synchronize()
            return a.elapsed_time(b) / iters, r
        # ---- stages (HIP events on the launch stream, whole batch)
        with torch.no_grad():
            pcn, gc, gfd = PatchHelper.normalize_pc(pc)
            st = {}
            st["fps_seeds"], _ = ev_ms(lambda: ops.furthest_point_sample(pcn, n_patch))
            st["knn256_patches"], patches = ev_ms(lambda: PatchHelper.extract_knn_patch(pcn, ph.knn, NPATCH, 4))
            st["network"], cand = ev_ms(lambda: PatchHelper.upsampling_patches(net, patches, UP))
            M = cand.shape[1] * cand.shape[2]
            flat = cand.reshape(B, M, 3).contiguous()
            GRP = cand.shape[2]                                                        # candidates per patch: the merge's layout hint
            st["fps_merge"], _ = ev_ms(lambda: ops.furthest_point_sample(flat, npoint, group=GRP))
            den = PatchHelper.merge_patches(cand, npoint).transpose(1, 2).contiguous()
            st["remove_outliers"], _ = ev_ms(lambda: PatchHelper.remove_outliers(den, pc, NOUT))
            # ---- dominant kernel: the cooperative FPS merge (fps_coopm_kernel).  One launch = B clouds x G workgroups; a cloud's
            # samples are sequential BY DEFINITION (sample j+1 needs the min-distances after sample j), so a launch is bound by
            # the latency of one dependent exchange round x the rounds of one cloud, not by bytes or flops: the whole cloud
            # lives in registers and the algorithmic HBM traffic is one read of the candidates + one write of the indices.
            mind = torch.empty((1, M), dtype=torch.float32, device=dev)
            idx1 = torch.zeros((1, npoint), dtype=torch.int32, device=dev)
            one = flat[:1].contiguous()
            s = torch.cuda.current_stream().cuda_stream
            one_ms, _ = ev_ms(lambda: _lib.check(lib.pf_fps_grouped(one.data_ptr(), 1, M, npoint, GRP, mind.data_ptr(), idx1.data_ptr(), s), "pf_fps"))
            stride, word = ctypes.c_longlong(0), ctypes.c_longlong(0)
            coop = bool(lib.pf_fps_scratch_layout(M, ctypes.byref(stride), ctypes.byref(word)))
            rounds = int(mind.view(-1)[: M // 2 * 2].view(torch.int64)[word.value + 1].item()) if coop else npoint
            ppt = 4 if M >= 16 * 256 else 1                                           # pf_fps's choice of points per thread and
            while -(-M // (256 * ppt)) > 32:                                            # workgroups per cloud (csrc/patch_ops.hip)
                ppt *= 2
            if GRP % 64 == 0 and GRP // 64 in (12, 20, 24) and -(-M // (256 * (GRP // 64))) <= 32:
                ppt = GRP // 64                                                          # one patch per wave (pf_fps_grouped)
            G = -(-M // (256 * ppt))
            ring = torch.zeros(2048, dtype=torch.int64, device=dev)
            PROBE_ROUNDS = 20000
            probe_ms, _ = ev_ms(lambda: _lib.check(lib.pf_fps_exchange_probe(min(max(G, 2), 32), PROBE_ROUNDS, ring.data_ptr(), s), "probe"))
            assert int(ring[1024].item()) == 0, "exchange probe did not complete"
        alg_bytes = B * (M * 12 + npoint * 4)
        merge_ms = st["fps_merge"]
        # HBM bytes of one launch from the committed PMC pass (tools/pmc_cmd.sh over tools/time_fps.py 99840 20024 32 patch)
        traffic = None
        try:
            pm = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "pmc_pugan_latest.json")))
            ent = [v for k_, v in pm.get("kernels", {}).items() if "fps_coopm_kernel" in k_ and "hbm_bytes_per_launch" in v]
            if ent:
                ent = max(ent, key=lambda v: v.get("pct", 0.0))
                traffic = {"bytes_per_launch": ent["hbm_bytes_per_launch"], "profiled_avg_us": ent.get("avg_us"),
                           "valu_insts_per_launch": ent.get("SQ_INSTS_VALU_mean"),
                           "source": "profiles/pmc_pugan_latest.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over 32 patch-ordered clouds, "
                                     "FETCH_SIZE doubled per the gfx950 note): almost all of it is the polled exchange words, which are agent-scope "
                                     "atomic loads that bypass the L2 - the cloud itself is read once (1.2 MB per cloud)"}
        except Exception:
            traffic = None
        us_round_one = one_ms * 1e3 / max(rounds, 1)
        floor_us = probe_ms * 1e3 / PROBE_ROUNDS
        roof = {"bound": "latency", "kernel": f"fps_coopm_kernel<{ppt}> (csrc/patch_ops.hip): FPS merge {M} -> {npoint} per cloud, "
                                              f"{B} clouds x {G} cooperating workgroups per launch",
                "achieved": us_round_one, "peak": floor_us, "unit": "us per exchange round (one cloud alone; lower is better)",
                "frac": floor_us / us_round_one, "traffic": traffic, "avg_launch_ms": merge_ms,
                "bound_note": "the contract's two bounds do not describe this kernel: FPS is sequential in its output count (sample j+1 needs the "
                              "min-distances after sample j), every point and its running min-distance live in registers for the whole launch and "
                              "the algorithmic HBM traffic is ~1.3 MB per cloud.  What bounds a cloud is the number of DEPENDENT exchange rounds x "
                              "the time of a round; `peak` is the measured floor of a round (pf_fps_exchange_probe: the same ring protocol between "
                              "the same number of workgroups with no points), `achieved` the time of a round of one cloud alone - which now also "
                              "holds the chain that takes up to 64 samples out of one exchange (~0.25 us per sample, serial in one wave)",
                "latency": {"samples_per_cloud": npoint, "rounds_per_cloud": rounds, "samples_per_round": npoint / max(rounds, 1),
                            "one_cloud_ms": one_ms, "us_per_round_one_cloud": us_round_one,
                            "us_per_sample_one_cloud": one_ms * 1e3 / npoint,
                            "exchange_floor_us_per_round": floor_us,
                            "floor_ms_per_cloud": floor_us * rounds * 1e-3,
                            "batch_ms": merge_ms, "us_per_sample_in_batch": merge_ms * 1e3 / (B * npoint),
                            "note": "in a batch the clouds' rounds overlap (independent rings): batch_ms / one_cloud_ms clouds' worth of time for "
                                    f"{B} clouds"},
                "hbm": {"achieved": alg_bytes / (merge_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": alg_bytes / (merge_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                        "bytes_basis": f"algorithmic: {M} candidates x 12 B read once + {npoint} indices x 4 B written, per cloud, {B} clouds per "
                                       "launch; live HIP-event duration on the launch stream"}}
        extra["stage_ms"] = st
        if world == 1 and not args.no_cpu_baseline:
            from oracle import patch_ref as P, ref_cpu as O
            ncpu = _ncpu()
            torch.set_num_threads(ncpu)
            t1 = time.perf_counter()
            c1 = pc_cpu[:1]
            pn1, gc1, gf1 = P.normalize_pc(c1)
            pt = P.extract_knn_patch(pn1, NPATCH, 4)
            pnn, pcen, pfd = P.normalize_pc(pt.reshape(n_patch, NPATCH, 3))
            pred_ref, _ = O.forward(sd, pnn, UP)
            cand_ref = (torch.cat([pred_ref, pnn], 1) * pfd + pcen).reshape(1, n_patch, -1, 3)
            merged = P.merge_patches(cand_ref, npoint) * gf1 + gc1
            ref_out = P.remove_outliers(merged, c1, NOUT)
            cel = time.perf_counter() - t1
            cpu = {"value": n_patch / cel, "unit": "patches/s", "clouds_per_s": 1.0 / cel, "cores": ncpu, "kind": "port",
                   "sample": f"1 cloud of {N} points ({n_patch} patches) through the CPU oracle pipeline (oracle/patch_ref.py + oracle/ref_cpu.py: "
                             "numpy FPS, torch-CPU network), once"}
            # parity on the same cloud: the GPU pipeline stage by stage is bit-exact / within 1e-5 in tests/test_gpu_patch.py; the FPS
            # merge is chaotic in its input, so end to end the clouds are compared as coverage (Chamfer distance to the input)
            cd_gpu = float(O.chamfer_distance_mean(out[:1].cpu(), c1))
            cd_ref = float(O.chamfer_distance_mean(ref_out, c1))
            extra["parity"] = {"cd_to_input_gpu": cd_gpu, "cd_to_input_oracle": cd_ref, "rel_diff": abs(cd_gpu - cd_ref) / cd_ref,
                               "note": "coverage of the same input cloud by the HIP pipeline's and the CPU oracle pipeline's 20 000 points"}
    if use_dist:
        dist.destroy_process_group()
    if rank == 0:
        clouds = world * B * args.steps
        rec = {"metric": "patches/sec x4 (PU-GAN 5000->20000 clouds, 78 x 256-pt patches per cloud, whole patch pipeline)",
               "value": clouds * n_patch / el, "unit": "patches/s", "clouds_per_s": clouds / el, "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": el / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "f32 (split-fp16 MFMA products in the network, fp32 accumulate; FPS / kNN / outlier distances exact unfused fp32)",
               "data": "synthetic",
               "config": {"workload": f"BASELINE configs[3]: PU-GAN {N} -> {N * UP} inference, {B} clouds per GPU and step "
                                      f"({B * n_patch} patches of 256 points)", "clouds_per_gpu": B, "points_per_cloud": N,
                          "patches_per_cloud": n_patch, "candidates_per_cloud": n_patch * NPATCH * (UP + 1), "outliers_removed": NOUT,
                          "collectives": args.collectives,
                          "sharding": f"clouds over {world} rank(s), no data-path collective"},
               "roofline": roof, "cpu_baseline": cpu}
        rec.update(extra)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
