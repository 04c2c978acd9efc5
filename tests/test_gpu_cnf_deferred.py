"""The continuous model's deferred step-size controller on the GPU: taped integrations that nobody looks at while they
run (csrc/cnf.hip: pf_cnf_tape_close, pf_cnf_init_dev; csrc/cnf_bwd.hip: pf_cnf_tape_vjp_dev; puflow_amd/cnf.py:
tape_forward_deferred, check_train_logs), the eager step built on them and the captured one (trainer / train_graph / train).

Everything here is a comparison of BITS against the host-read path that exists already (torch.equal): the deferred path runs the
same kernels on the same numbers, it only stops asking the device how far it got.  Weights: synth_cnf_state_dict(7), two accepted
steps per integration.  Shapes: (B, N, R) = (2, 128, 4) - sixteen full 64-row tiles in g - and (3, 50, 2): a partial tile, 8 points
per 16-row MFMA tile."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from puflow_amd.weights import synth_cnf_state_dict, synth_patches

DEV = "cuda:0"
SHAPES = [(2, 128, 4), (3, 50, 2)]
BLOCK_OF = {(2, 128, 4): 5, (3, 50, 2): 1}                  # context widths 128 and 64


@functools.lru_cache(maxsize=None)
def _sd():
    return synth_cnf_state_dict(7)


def _net(deterministic=False, deferred=False):
    from puflow_amd.cnf import PointInterpFlow
    net = PointInterpFlow(3)
    net.load_state_dict(_sd(), strict=True)
    net = net.to(DEV).train()
    net.deterministic = deterministic
    net.train_deferred = deferred
    return net


def _block_inputs(block, T, R, seed):
    g = torch.Generator().manual_seed(seed)
    cd = _sd()[f"flow_blocks.{block}.cnf.odefunc.diffeq.layers.0._hyper_gate.weight"].shape[1] - 1
    c = (torch.randn(T, cd, generator=g) * 0.7).to(DEV)
    e = torch.randn(T, 3, generator=g).to(DEV)
    x = (torch.randn(T * R, 3, generator=g) * 0.8).to(DEV)
    gx = torch.randn(T * R, 3, generator=g).to(DEV)
    gl = torch.randn(T * R, generator=g).to(DEV)
    return x, c, e, gx, gl


# ---- 1. kernel bits -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("B,N,R", SHAPES)
def test_tape_vjp_dev_is_tape_vjp_with_the_count_on_the_device(B, N, R, reverse):
    """pf_cnf_tape_vjp_dev with the recorded controller row against pf_cnf_tape_vjp with the host n: ybar, ctxbar, grad as bits, for
    a tape of exactly n steps, one with five more, and one whose rows past n are NaN (they are never read).  A controller row that
    is not clean sweeps nothing: ybar passes through, ctxbar and grad stay zero."""
    from puflow_amd.cnf import _BlockTapeEngine
    from puflow_amd.packing import CNF_CTX, CNF_GRAD
    block, T = BLOCK_OF[(B, N, R)], B * N
    Rr = R if reverse else 1
    rows = T * Rr
    x, c, e, gx, gl = _block_inputs(block, T, Rr, 31 + N)
    eng = _BlockTapeEngine({k: v for k, v in _sd().items() if k.startswith(f"flow_blocks.{block}.")}, block, torch.device(DEV))
    y, tape = eng.tape_forward(block, x, c, e, Rr, reverse)
    n = len(tape["steps"])
    assert n >= 1
    ctl = eng.ctl.clone()                                   # the controller row as the integration left it: done, n accepted, status 0
    assert int(ctl[5]) == 1 and int(ctl[6]) == n and int(ctl[9]) == 0
    sgn = -1.0 if reverse else 1.0
    ybar_in = torch.cat([gx, gl[:, None]], dim=1).contiguous()

    def fresh():
        return ybar_in.clone(), torch.zeros(T, CNF_CTX, device=DEV), torch.zeros(CNF_GRAD, device=DEV)

    ref = fresh()
    eng.tape_vjp(block, tape["states"].contiguous(), tape["steps_dev"].contiguous(), sgn, tape["ctx"], e, *ref, rows, Rr)

    def dev_sweep(cap, pad, row=ctl):
        states = torch.full((cap + 1, rows, 4), pad, device=DEV)
        steps = torch.full((cap, 2), pad, device=DEV)
        states[:n], steps[:n] = tape["states"], tape["steps_dev"]
        out = fresh()
        eng.tape_vjp_dev(block, dict(states=states, steps_dev=steps, log=row, cap=cap, ctx=tape["ctx"]), sgn, e, *out, rows, Rr)
        return out

    for what, got in (("cap == n", dev_sweep(n, 0.25)), ("cap == n + 5", dev_sweep(n + 5, 0.25)),
                      ("NaN past n", dev_sweep(n + 5, float("nan")))):
        for name, a, b in zip(("ybar", "ctxbar", "grad"), got, ref):
            assert torch.equal(a, b), (what, name)
    assert float(ref[2].abs().max()) > 0 and not torch.equal(ref[0], ybar_in)
    for what, edit in (("not done", (5, 0.0)), ("status 3", (9, 3.0)), ("n > cap", (6, float(n + 9))), ("n = 0", (6, 0.0))):
        row = ctl.clone()
        row[edit[0]] = edit[1]
        yb, cb, gr = dev_sweep(n + 5, float("nan"), row)
        assert torch.equal(yb, ybar_in) and not bool(cb.any()) and not bool(gr.any()), what


# ---- 2. / 3. block bits, shortfalls -------------------------------------------------------------------------------------------------
BLOCK_CASES = {"b0_f_R1": (0, 2 * 128, 1, False), "b5_g_R4": (5, 2 * 128, 4, True), "b1_g_R2": (1, 3 * 50, 2, True)}
# tensors whose two controller="device" runs do not agree as bits (none: the block's backward has no float atomics)
UNSTABLE = ()


def _block_run(net, name, **kw):
    block, T, R, reverse = BLOCK_CASES[name]
    x, c, e, gx, gl = _block_inputs(block, T, R, 53 + T)
    x, c = x.requires_grad_(True), c.requires_grad_(True)
    net.zero_grad(set_to_none=True)
    x1, dl = net.flow_block(block, x, c, e, R, reverse, **kw)
    ((x1 * gx).sum() + (dl * gl).sum()).backward()
    out = {"x'": x1.detach(), "dlogp": dl.detach(), "xbar": x.grad, "cbar": c.grad}
    out.update({k: p.grad for k, p in net.flow_blocks[block].named_parameters()})
    return out


@functools.lru_cache(maxsize=None)
def _block_ref(name):
    net = _net()
    a, b = _block_run(net, name, controller="device"), _block_run(net, name, controller="device")
    return a, b, len(net.last_block_steps)


@pytest.mark.parametrize("name", sorted(BLOCK_CASES))
def test_flow_block_deferred_has_the_bits_of_the_device_controller(name):
    a, b, n = _block_ref(name)
    assert len(a) == 4 + 16 and all(v is not None for v in a.values())
    for k in a:                                             # the precondition: the reference agrees with itself
        assert k in UNSTABLE or torch.equal(a[k], b[k]), ("two controller='device' runs differ", k)
    assert not set(UNSTABLE) & {"x'", "dlogp", "xbar"}
    net = _net()
    got = _block_run(net, name, controller="deferred", attempts=64, cap=32)
    assert net.check_train_logs() == 0 and net.last_skipped_steps == 0
    assert net.last_block_steps == [] and int(net.last_block_tape["log"][6]) == n
    for k in a:
        if k not in UNSTABLE:
            assert torch.equal(got[k], a[k]), k
    assert bool(torch.isfinite(got["x'"]).all()) and float(got["xbar"].abs().max()) > 0


@pytest.mark.parametrize("name,attempts,cap,status", [("b5_g_R4", 1, 32, 4), ("b1_g_R2", 64, 1, 3)])
def test_a_shortfall_is_recorded_and_survivable(name, attempts, cap, status):
    """Too few attempts (sticky status 4) or too short a tape (3): NaN out, the run in the sticky row, `check_train_logs` returns 1
    and doubles that budget - and the same log row then runs a clean integration with the bits of case 2, and keeps its counts."""
    from puflow_amd.cnf import _log_row
    block, T, R, reverse = BLOCK_CASES[name]
    a, _, n = _block_ref(name)
    assert n >= 2                                           # so that one attempt / a one-step tape IS a shortfall
    net = _net()
    got = _block_run(net, name, controller="deferred", attempts=attempts, cap=cap)
    assert bool(torch.isnan(got["x'"]).all()) and bool(torch.isnan(got["dlogp"]).all())
    k = _log_row(block, reverse)
    sticky = net._train_tables(torch.device(DEV))[1]
    assert sticky[k, :3].tolist() == [1, 1, status] and 1 <= int(sticky[k, 3]) <= max(attempts, cap)
    assert net.check_train_logs() == 1 and net.last_skipped_steps == 1
    assert net.tape_budget[(block, reverse)] == ((2, 32) if status == 4 else (64, 2))
    assert net.check_train_logs() == 0                      # reported once
    for run in range(3):                                    # the row is reusable; its counts survive
        got = _block_run(net, name, controller="deferred", attempts=64, cap=32)
        for key in a:
            if key not in UNSTABLE:
                assert torch.equal(got[key], a[key]), (run, key)
        assert sticky[k, :3].tolist() == [2 + run, 1, status]
    assert int(sticky[k, 3]) >= n and net.check_train_logs() == 0


# ---- 4. whole forward + backward ----------------------------------------------------------------------------------------------------
class _HostReads:
    """Counts the calls that bring a GPU tensor's value to the host."""
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


def test_deferred_forward_backward_has_the_bits_of_the_host_read_one_and_reads_once(monkeypatch):
    B, N, R = 2, 128, 4
    g = torch.Generator().manual_seed(3)
    xyz = synth_patches(B, N, seed=9).to(DEV)
    noise = [torch.randn(B, N, 3, generator=g).to(DEV) for _ in range(6)]
    gx = torch.randn(B, N * R, 3, generator=g).to(DEV)

    def run(net):
        net.zero_grad(set_to_none=True)
        x, logp = net(xyz, R, noise=noise)
        loss = 0.5 * logp + (x * gx).sum()
        loss.backward()
        return loss.detach(), x.detach(), {k: p.grad for k, p in net.named_parameters()}

    # Both nets take two runs and are compared run by run: a net's SECOND forward + backward does not have the bits of its first
    # (host-read path too, before this switch existed: the interpolation branch's gradients, x and the loss move in the last
    # bits), while fresh nets agree with each other run for run - which is what the bit-reproducible mode promises.
    host = _net(deterministic=True)
    first = run(host)
    net = _net(deterministic=True, deferred=True)
    warm = run(net)                                         # no budgets yet: the host-read loop, which leaves them
    assert len(net.tape_budget) == 12 and net.last_train_steps == host.last_train_steps
    assert torch.equal(warm[0], first[0]) and torch.equal(warm[1], first[1])
    ref = run(host)
    ref_steps = host.last_train_steps
    torch.cuda.synchronize()
    reads = _HostReads(monkeypatch)
    got = run(net)
    assert reads.n == 0, "the deferred forward + backward read the device"
    assert net.check_train_logs() == 0
    assert reads.n == 1, "check_train_logs is ONE read"
    monkeypatch.undo()
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert all(v is not None for v in got[2].values())
    for k in ref[2]:
        assert torch.equal(got[2][k], ref[2][k]), k
    assert net.last_train_steps == ref_steps and len(ref_steps) == 12
    st = net.train_log_stats()
    assert [r["runs"] for r in st["rows"]] == [1] * 12 and all(r["max_took"] <= r["attempts"] for r in st["rows"])


# ---- 5. captured step ---------------------------------------------------------------------------------------------------------------
def _trainer(deferred=True):
    from puflow_amd.trainer import TrainerModule, default_cfg
    m = TrainerModule(default_cfg(model="continuous", cnf_deferred=deferred, emd_workgroups=1, deterministic=True))
    m.network.load_state_dict(_sd(), strict=True)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(17)                   # the Hutchinson vectors held fixed, the same for both sides
    m.network.train_noise = [torch.randn(2, 64, 3, generator=g).to(DEV) for _ in range(6)]
    return m


def test_graphed_train_step_replays_the_eager_deferred_steps():
    """One warm-up step (eager: it learns the budgets) and three replays against four eager deferred steps: every parameter as
    bits.  Then a shortfall written into the sticky table by the test: it survives two replays and `check()` marks the step stale."""
    from puflow_amd.cnf import _log_row
    dense = synth_patches(2, 256, seed=21).to(DEV)
    sparse = dense[:, ::4].contiguous()
    batch = (sparse, dense)
    eager = _trainer()
    opt_e = eager.configure_optimizers()["optimizer"]
    losses_e = [eager.train_step(batch, opt_e) for _ in range(4)]
    m = _trainer()
    opt = m.configure_optimizers()["optimizer"]
    step = m.graphed_train_step(batch, opt, warmup=1)       # the parent raises GRAPH_ERROR here
    assert len(m.network.tape_budget) == 12 and step.stale is False
    losses = [step.warmup_loss.clone()] + [step(batch).clone() for _ in range(3)]
    assert step.check() == (0, 0) and step.stale is False
    print("\nlosses eager", [float(v) for v in losses_e], "captured", [float(v) for v in losses])
    pe, pg = dict(eager.network.named_parameters()), dict(m.network.named_parameters())
    diff = [k for k in pe if not torch.equal(pe[k].detach(), pg[k].detach())]
    assert not diff, (len(diff), diff[:5])
    assert all(torch.equal(a, b) for a, b in zip(losses_e, losses))
    st = m.network.train_log_stats()
    assert [r["runs"] for r in st["rows"]] == [3] * 12 and all(r["not_clean"] == 0 for r in st["rows"])
    # a shortfall nobody has looked at yet: integration g of block 2 ran out of attempts once
    k = _log_row(2, True)
    sticky = m.network._train_tables(torch.device(DEV))[1]
    before = m.network.tape_budget[(2, True)]
    sticky[k, 1] += 1
    sticky[k, 2] = 4
    step(batch); step(batch)
    assert sticky[k, :3].tolist() == [5, 1, 4]
    assert step.check() == (0, 1) and step.stale is True and step.skipped == 1
    assert m.network.tape_budget[(2, True)] == (2 * before[0], before[1])


def test_capture_needs_the_switch_and_one_process(monkeypatch):
    m = _trainer(deferred=False)
    opt = m.configure_optimizers()["optimizer"]
    dense = synth_patches(2, 256, seed=21).to(DEV)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        m.graphed_train_step((dense[:, ::4].contiguous(), dense), opt)
    from puflow_amd import dist
    m = _trainer()
    monkeypatch.setattr(dist, "multi_rank", lambda: True)
    with pytest.raises(RuntimeError, match="single-process"):
        m.graphed_train_step((dense[:, ::4].contiguous(), dense), m.configure_optimizers()["optimizer"])


# ---- 6. entry -----------------------------------------------------------------------------------------------------------------------
def test_train_entry_captures_the_continuous_model(tmp_path):
    from puflow_amd import train
    from puflow_amd.cnf import PointInterpFlow
    argv = ["--model", "continuous", "--graph", "--cnf_deferred", "--synthetic", "--batch_size", "2", "--max_epochs", "1", "--seed", "3",
            "--checkpoint_path", str(tmp_path / "cnf.ckpt")]
    module, hist = train.main(argv)
    assert hist["epochs"] == 1 and len(hist["CD"]) == 1 and hist["loss"][0] == hist["loss"][0]
    assert module.network.train_deferred and len(module.network.tape_budget) == 12
    runs = [r["runs"] for r in module.network.train_log_stats()["rows"]]
    assert runs == [runs[0]] * 12 and runs[0] >= 1          # replays ran the deferred integrations
    torch.save(module.network.state_dict(), tmp_path / "cnf.ckpt")
    fresh = PointInterpFlow(3)
    res = fresh.load_state_dict(torch.load(tmp_path / "cnf.ckpt", map_location="cpu"), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    fresh = fresh.to(DEV).eval()
    x, _ = fresh(synth_patches(1, 64, seed=2).to(DEV), 4)
    assert x.shape == (1, 256, 3) and bool(torch.isfinite(x).all())
    with pytest.raises(RuntimeError, match="cannot be captured"):
        train.main([a for a in argv if a != "--cnf_deferred"])
