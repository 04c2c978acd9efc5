"""The continuous model on a frozen step schedule on the GPU: `record_schedule`, the scheduled eval forward and its error
ratios, the scheduled train-mode forward / backward, the captured step and the entries (puflow_amd/cnf.py, trainer, train_graph,
train, upsample_cnf).  Weights: synth_cnf_state_dict(7); shapes (B, N, R) = (2, 128, 4), those of tests/test_gpu_cnf_deferred.py."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import cnf_grad_ref as G
import cnf_train_ref as TR
from puflow_amd.weights import synth_cnf_state_dict, synth_patches

DEV = "cuda:0"
B, N, R = 2, 128, 4


@functools.lru_cache(maxsize=None)
def _sd():
    return synth_cnf_state_dict(7)


def _net(train=False, deterministic=False):
    from puflow_amd.cnf import PointInterpFlow
    net = PointInterpFlow(3)
    net.load_state_dict(_sd(), strict=True)
    net = net.to(DEV)
    net.deterministic = deterministic
    return net.train() if train else net.eval()


def _flow_keys():
    return [k for i in range(6) for k in G.block_keys(i) + [G.end_key(i)]]


# ---- 1. record, then replay ----------------------------------------------------------------------------------------------------------
def test_recorded_schedule_replays_the_taped_adaptive_forward_bit_for_bit():
    """`record_schedule` runs the twelve integrations with the taped device controller (the covering step cut); an eval forward on
    the recorded schedule, same input and noise, is the same steps: x and logp as bits, no rejected step, every error ratio <= 1
    (they are the ratios the controller accepted these steps on)."""
    from puflow_amd import cnf
    g = torch.Generator().manual_seed(3)
    xyz = synth_patches(B, N, seed=9).to(DEV)
    noise = [torch.randn(B, N, 3, generator=g).to(DEV) for _ in range(6)]
    net = _net()
    x_adaptive, _ = net(xyz, R, noise=noise)                 # the default path, untouched by what follows
    assert "schedule" not in net.last_stats
    sched = net.record_schedule(xyz, R, noise=noise)
    assert net.step_schedule is None and sorted(sched) == sorted(cnf.schedule_keys())
    rec = net.last_record
    ns = [len(s) for s in rec["steps"]]
    assert [len(sched[k]) - 1 for k in cnf.schedule_keys()] == ns and min(ns) >= 1
    net.step_schedule = sched
    x, logp = net(xyz, R, noise=noise)
    assert torch.equal(x, rec["x"]) and torch.equal(logp, rec["logp"])
    assert net.last_stats == dict(nfe=sum(1 + 6 * n for n in ns), accepted=sum(ns), rejected=0, schedule=True)
    ratios = net.schedule_error_ratios()
    assert sorted(ratios) == sorted(sched) and [len(ratios[k]) for k in cnf.schedule_keys()] == ns
    worst = max(max(v) for v in ratios.values())
    print(f"\nsteps per integration {ns}; worst error ratio {worst:.3f}; |x - adaptive (dense output)| "
          f"{float((x - x_adaptive).abs().max()):.2e}")
    assert 0 < worst <= 1.0
    assert float((x - x_adaptive).abs().max()) < 1e-3        # the same solution to the solver's tolerance, not the same bits
    # refined by two: twice the evaluations, a different grid, the same solution
    net.step_schedule = cnf.refine_schedule(sched, 2)
    x2, _ = net(xyz, R, noise=noise)
    assert net.last_stats["accepted"] == 2 * sum(ns) and float((x2 - x).abs().max()) < 1e-3 and not torch.equal(x2, x)
    assert max(max(v) for v in net.schedule_error_ratios().values()) < worst
    net.step_schedule = None
    x3, _ = net(xyz, R, noise=noise)
    assert torch.equal(x3, x_adaptive) and "schedule" not in net.last_stats


# ---- 2. train-mode forward / backward ------------------------------------------------------------------------------------------------
class _HostReads:
    """Counts the calls that bring a GPU tensor's value to the host (tests/test_gpu_cnf_deferred.py)."""
    NAMES = ("cpu", "item", "tolist", "numpy", "__bool__", "__float__", "__int__", "__index__")

    def __init__(self, monkeypatch):
        self.n = 0
        for name in self.NAMES:
            orig = getattr(torch.Tensor, name)

            def counted(t, *a, _orig=orig, **kw):
                if t.is_cuda:
                    self.n += 1
                return _orig(t, *a, **kw)
            monkeypatch.setattr(torch.Tensor, name, counted)


@functools.lru_cache(maxsize=None)
def _wiring_case():
    """tests/test_gpu_cnf_train.py::_flow_case under a schedule of two uniform steps (block 3's grid hand-made)."""
    from puflow_amd import cnf, ops, train_ops
    CDS = [32, 64, 128, 128, 128, 128]
    g = torch.Generator().manual_seed(1000 * B + N)
    xyz = synth_patches(B, N, seed=11 + N)
    cs = [torch.randn(B, N, cd, generator=g) * 0.7 for cd in CDS]
    w = torch.randn(B * N * 8, 32, generator=g)
    noise = [torch.randn(B, N, 3, generator=g) for _ in range(6)]
    gx = torch.randn(B, N * R, 3, generator=g)
    loss = lambda x, logp: 0.5 * logp + (x * gx.to(x)).sum()
    net = _net(train=True)
    sched = cnf.uniform_schedule(2)
    sched[(3, False)] = (0.0, 0.1, 0.45, 1.0)
    sched[(3, True)] = (0.0, 0.7, 1.0)
    net.step_schedule = sched
    xd = xyz.to(DEV).requires_grad_(True)
    csd = [c.to(DEV).requires_grad_(True) for c in cs]
    wd = w.to(DEV).requires_grad_(True)
    idx16, _ = ops.knn_idx32(xyz.to(DEV), xyz.to(DEV), 16)
    idx8 = idx16[..., :8].contiguous()
    train_ops.set_deterministic(False)
    x, logp = cnf.flow_train(net, xd, R, csd, (None, wd, None, None, idx8), [n.to(DEV) for n in noise])
    loss(x, logp).backward()
    steps = [list(s) for s in net.last_train_steps]
    params = dict(net.named_parameters())
    got = {"x": x.detach().cpu(), "logp": logp.detach().cpu(), "xyz": xd.grad.cpu().reshape(B * N, 3), "w": wd.grad.cpu()}
    got.update({f"cs.{i}": c.grad.cpu() for i, c in enumerate(csd)})
    got.update({k: params[k].grad.detach().cpu() for k in _flow_keys()})
    ref = {}
    for dt in (torch.float64, torch.float32):
        r = TR.run(_sd(), xyz, R, steps, noise, dt, cs=cs, w=w, idx8=idx8.cpu(), xyz_leaf=True)
        gr = TR.gradients(r, loss)
        gr["x"], gr["logp"] = r.x.detach(), r.logp.detach()
        ref[dt] = gr
    keys = ["x", "logp", "xyz", "w"] + [f"cs.{i}" for i in range(6)] + _flow_keys()
    err = {k: G.rel_err(got[k], ref[torch.float64][k].reshape(got[k].shape)) for k in keys}
    err32 = {k: G.rel_err(ref[torch.float32][k], ref[torch.float64][k]) for k in keys}
    print(f"\nscheduled flow wiring {B} x {N} x {R}: steps per integration {[len(s) for s in steps]}")
    for k in keys:
        print(f"  {k:66s} err32 {err32[k]:.2e}  gpu {err[k]:.2e}  max|ref| {float(ref[torch.float64][k].abs().max()):.2e}")
    return dict(keys=keys, err=err, err32=err32, ref=ref[torch.float64], steps=steps, sched=sched)


def test_scheduled_train_forward_backward_matches_float64_on_its_step_lists():
    """x, logp and the gradients of every cs[i], the logits, xyz and all 16 x 6 flow-block tensors against tests/cnf_train_ref.py
    in float64 on the step lists the device made, the bound of tests/test_gpu_cnf_train.py: max(2e-5, 4 x err32), err32 <= 1e-4."""
    from puflow_amd import cnf
    r = _wiring_case()
    assert [len(s) for s in r["steps"]] == [len(r["sched"][k]) - 1 for k in cnf.schedule_keys()]
    T_end = 0.5                                              # synth_cnf_state_dict(7): every block's end time
    for (i, reverse), steps in zip(cnf.schedule_keys(), r["steps"]):
        assert abs(steps[0][0] - (-T_end if reverse else 0.0)) < 1e-6
        assert abs(steps[-1][0] + steps[-1][1] - (0.0 if reverse else T_end)) < 1e-6
    for k in r["keys"]:
        if k not in ("x", "logp"):
            assert float(r["ref"][k].abs().max()) > 0, k
        assert r["err32"][k] <= 1e-4, ("the float32 yardstick is too coarse for this seed", k, r["err32"][k])
        assert r["err"][k] <= max(2e-5, 4 * r["err32"][k]), (k, r["err"][k], r["err32"][k])


def test_scheduled_train_step_reads_nothing_in_the_forward(monkeypatch):
    from puflow_amd import cnf
    g = torch.Generator().manual_seed(3)
    xyz = synth_patches(B, N, seed=9).to(DEV)
    noise = [torch.randn(B, N, 3, generator=g).to(DEV) for _ in range(6)]
    gx = torch.randn(B, N * R, 3, generator=g).to(DEV)
    net = _net(train=True, deterministic=True)
    net.step_schedule = cnf.uniform_schedule(2)

    def run():
        net.zero_grad(set_to_none=True)
        x, logp = net(xyz, R, noise=noise)
        (0.5 * logp + (x * gx).sum()).backward()
        return x.detach()

    run()                                                    # library loads, workspaces, the schedule's upload
    torch.cuda.synchronize()
    reads = _HostReads(monkeypatch)
    x = run()
    assert reads.n == 0, "the scheduled forward + backward read the device"
    assert net.check_train_logs() == 0 and net.last_skipped_steps == 0
    assert reads.n == 1, "check_train_logs is ONE read"
    steps = net.last_train_steps                             # read when asked
    monkeypatch.undo()
    assert [len(s) for s in steps] == [2] * 12
    assert bool(torch.isfinite(x).all()) and all(p.grad is not None for p in net.parameters())


# ---- 3. captured step ----------------------------------------------------------------------------------------------------------------
def _trainer(schedule):
    from puflow_amd.trainer import TrainerModule, default_cfg
    m = TrainerModule(default_cfg(model="continuous", cnf_schedule=schedule, emd_workgroups=1, deterministic=True))
    m.network.load_state_dict(_sd(), strict=True)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(17)
    m.network.train_noise = [torch.randn(2, 64, 3, generator=g).to(DEV) for _ in range(6)]
    return m


def test_graphed_train_step_replays_the_eager_schedule_steps_and_recaptures_on_a_new_schedule():
    """One warm-up step and three replays against four eager steps on the same schedule: losses and every parameter as bits, no
    void step.  Then a refined schedule is assigned: the next call captures anew and goes on matching the eager steps."""
    from puflow_amd import cnf
    dense = synth_patches(2, 256, seed=21).to(DEV)
    batch = (dense[:, ::4].contiguous(), dense)
    eager = _trainer(2)
    assert eager.network.step_schedule == cnf.uniform_schedule(2) and eager.capturable()
    opt_e = eager.configure_optimizers()["optimizer"]
    losses_e = [eager.train_step(batch, opt_e) for _ in range(4)]
    m = _trainer(2)
    opt = m.configure_optimizers()["optimizer"]
    step = m.graphed_train_step(batch, opt, warmup=1)
    losses = [step.warmup_loss.clone()] + [step(batch).clone() for _ in range(3)]
    assert step.check() == (0, 0) and step.stale is False and step.recaptures == 0 and not m.network.tape_budget
    print("\nlosses eager", [float(v) for v in losses_e], "captured", [float(v) for v in losses])
    assert all(bool(torch.isfinite(v)) for v in losses) and all(torch.equal(a, b) for a, b in zip(losses_e, losses))
    pe, pg = dict(eager.network.named_parameters()), dict(m.network.named_parameters())
    diff = [k for k in pe if not torch.equal(pe[k].detach(), pg[k].detach())]
    assert not diff, (len(diff), diff[:5])
    fine = cnf.refine_schedule(m.network.step_schedule, 2)
    eager.network.step_schedule = fine
    m.network.step_schedule = fine
    le = eager.train_step(batch, opt_e)
    lg = step(batch).clone()
    assert step.recaptures == 1 and [len(s) for s in m.network.last_train_steps] == [4] * 12
    assert torch.equal(le, lg)
    diff = [k for k in pe if not torch.equal(pe[k].detach(), pg[k].detach())]
    assert not diff, (len(diff), diff[:5])
    assert step(batch) is not None and step.recaptures == 1 and step.check() == (0, 0)


# ---- 4. entries ----------------------------------------------------------------------------------------------------------------------
def test_train_entry_captures_the_continuous_model_on_a_schedule(tmp_path):
    from puflow_amd import cnf, train
    argv = ["--model", "continuous", "--cnf_schedule", "4", "--graph", "--synthetic", "--batch_size", "2", "--max_epochs", "1",
            "--seed", "3", "--checkpoint_path", str(tmp_path / "cnf.ckpt")]
    module, hist = train.main(argv)
    assert hist["epochs"] == 1 and len(hist["CD"]) == 1 and hist["loss"][0] == hist["loss"][0]
    assert module.network.step_schedule == cnf.uniform_schedule(4) and not module.network.tape_budget
    assert [len(s) for s in module.network.last_train_steps] == [4] * 12
    path = tmp_path / "sched.json"
    cnf.save_schedule(cnf.uniform_schedule(3), path)
    from puflow_amd.trainer import TrainerModule, default_cfg
    assert TrainerModule(default_cfg(model="continuous", cnf_schedule=str(path))).network.step_schedule == cnf.uniform_schedule(3)
    batch = (synth_patches(2, 64, seed=4).to(DEV), synth_patches(2, 256, seed=4).to(DEV))
    sched = module.record_schedule(batch)                    # a run refreshes its schedule between steps
    assert module.network.step_schedule is sched or module.network.step_schedule == sched
    assert all(len(g) >= 2 for g in sched.values())


def test_upsample_entry_records_and_loads_a_schedule(tmp_path):
    import numpy as np
    from puflow_amd import cnf, upsample_cnf
    src, out1, out2 = tmp_path / "in", tmp_path / "out1", tmp_path / "out2"
    src.mkdir()
    pts = synth_patches(1, 512, seed=6)[0].numpy()
    np.savetxt(src / "cloud.xyz", pts, fmt="%.6f")
    torch.save(_sd(), tmp_path / "cnf.pt")
    sched = tmp_path / "sched.json"
    common = ["--source", str(src), "--checkpoint", str(tmp_path / "cnf.pt"), "--up_ratio", "4", "--num_patch", "128"]
    upsample_cnf.main(common + ["--target", str(out1), "--record_schedule", str(sched), "--schedule_refine", "2"])
    loaded = cnf.load_schedule(sched)
    assert sorted(loaded) == sorted(cnf.schedule_keys()) and all((len(g) - 1) % 2 == 0 for g in loaded.values())
    upsample_cnf.main(common + ["--target", str(out2), "--schedule", str(sched)])
    a, b = np.loadtxt(out1 / "cloud.xyz"), np.loadtxt(out2 / "cloud.xyz")
    assert a.shape == b.shape == (2048, 3) and np.isfinite(a).all() and np.isfinite(b).all()
    assert np.array_equal(a, b)                              # the same seed, the same schedule: the same cloud
