"""The one-launch reverse sweep of a recorded CNF integration (csrc/cnf_bwd.hip: pf_cnf_tape_vjp) and the tape recorded by the
device-side controller (csrc/cnf.hip: pf_cnf_steps_taped) against the float64 CPU references of tests/cnf_grad_ref.py.

Error measure: cnf_grad_ref.rel_err per tensor, max|got - ref64| / max(1, max|ref64|).  Bound, as tests/test_gpu_cnf_grad.py has it
for quantities that went through the steps: max(2e-5, 4 x err32), err32 = the same float64 helper run in float32 on the CPU on the
same steps; a case counts only if err32 <= 1e-4, so that a wrong term cannot hide.  Weights: synth_cnf_state_dict(7)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import cnf_grad_ref as G
from oracle import cnf_ref as C
from puflow_amd.weights import synth_cnf_state_dict

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _sd():
    return synth_cnf_state_dict(7)


def _inputs(block, T, R, seed):
    sd = _sd()
    g = torch.Generator().manual_seed(seed)
    cd = sd[f"flow_blocks.{block}.cnf.odefunc.diffeq.layers.0._hyper_gate.weight"].shape[1] - 1
    c = torch.randn(T, cd, generator=g) * 0.7
    e = torch.randn(T, 3, generator=g)
    x = torch.randn(T * R, 3, generator=g) * 0.8
    return g, x, c, e


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _bound_ok(err, err32, what):
    assert err32 <= 1e-4, ("the float32 yardstick is too coarse for this seed", what, err32)
    assert err <= max(2e-5, 4 * err32), (what, err, err32)


def _slot_sweep(sd, i, x, c, e, reverse, steps, dtype, ybar):
    """The per-point gradients with respect to the hyper networks' outputs (what pf_cnf_*_vjp adds into ctxbar), summed over the
    evaluations of the reverse sweep: cnf_grad_ref.steps_backward's loop, keeping oracle rhs_vjp's gate_pre / bias_pre per row
    instead of contracting them with the context.  -> {"gate_pre0": [T, 64], "bias_pre0": ..} summed over a point's R rows."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    x, c, e, ybar = x.to(dtype), c.to(dtype), e.to(dtype), ybar.to(dtype)
    rows, T = x.shape[0], c.shape[0]
    R = rows // T
    cr, er = torch.repeat_interleave(c, R, dim=0), torch.repeat_interleave(e, R, dim=0)
    sgn = -1.0 if reverse else 1.0
    F = lambda s, Y: sgn * C.rhs(sd, i, sgn * s, Y, cr, er)
    Y = torch.cat([x, torch.zeros(rows, 1, dtype=dtype)], dim=-1)
    stages = []
    for s, h in steps:
        k, Ys = [], []
        for j in range(6):
            Yj = Y
            for m in range(j):
                Yj = Yj + (h * C.DP_BETA[j - 1][m]) * k[m]
            Ys.append(Yj)
            k.append(F(s + G.ALPHA[j] * h, Yj))
        stages.append(Ys)
        for j in range(6):
            Y = Y + (h * G.B6[j]) * k[j]
    out = {}
    for (s, h), Ys in zip(reversed(list(steps)), reversed(stages)):
        y0bar = ybar.clone()
        kbar = [h * G.B6[j] * ybar for j in range(6)]
        for j in reversed(range(6)):
            v = C.rhs_vjp(sd, i, sgn * (s + G.ALPHA[j] * h), Ys[j][:, :3], cr, er, sgn * kbar[j][:, :3], sgn * kbar[j][:, 3])
            Ybar = torch.cat([v["y"], torch.zeros(rows, 1, dtype=dtype)], dim=-1)
            y0bar = y0bar + Ybar
            for m in range(j):
                kbar[m] = kbar[m] + (h * C.DP_BETA[j - 1][m]) * Ybar
            for l in range(3):
                for n in (f"gate_pre{l}", f"bias_pre{l}"):
                    out[n] = out.get(n, 0) + v[n].view(T, R, -1).sum(1)
        ybar = y0bar
    return out


# ---- 1 - 4. the kernel on a step list chosen here --------------------------------------------------------------------------------
# (block, T, R, reverse, step sizes): see test_tape_vjp_matches_float64_sweep for what each shape exercises
KCASES = {"b0_T200_R1_fwd": (0, 200, 1, False, (0.05, 0.11, 0.07)),
          "b0_T200_R1_fwd_one_step": (0, 200, 1, False, (0.05,)),
          "b5_T100_R4_rev": (5, 100, 4, True, (0.05, 0.11, 0.07)),
          "b3_T67_R3_rev": (3, 67, 3, True, (0.05, 0.11, 0.07)),
          "b2_T10_R4_fwd": (2, 10, 4, False, (0.05, 0.11, 0.07)),
          "b1_T16500_R1_rev": (1, 16500, 1, True, (0.05, 0.11))}


@functools.lru_cache(maxsize=None)
def _kernel_run(name):
    """One case: three GPU sweeps (fresh buffers; again into the same ctxbar / grad; fresh buffers once more) and the float64 /
    float32 CPU references on the same step list."""
    from puflow_amd.cnf import _BlockTapeEngine
    from puflow_amd.packing import CNF_CTX, CNF_GRAD
    block, T, R, reverse, hs = KCASES[name]
    sd = _sd()
    g, x, c, e = _inputs(block, T, R, 70 + block)
    rows = T * R
    ybar_in = torch.randn(rows, 4, generator=g)
    sgn = -1.0 if reverse else 1.0
    t = _f32(-float(sd[G.end_key(block)]) ** 2 if reverse else 0.0)
    steps = []
    for h in hs:                                                        # (s, h) as the fp32 values the kernels are given
        steps.append((t, _f32(h)))
        t = _f32(t + _f32(h))

    eng = _BlockTapeEngine({k: v for k, v in sd.items() if k.startswith(f"flow_blocks.{block}.")}, block, torch.device(DEV))
    cd_, ed = c.to(DEV), e.to(DEV)
    ctx = eng.context(block, cd_)
    y = torch.zeros(rows, 4, device=DEV)
    y[:, :3] = x.to(DEV)
    f0 = torch.empty_like(y)
    eng._rhs(block, y, y, [], 0.0, sgn * steps[0][0], sgn, ctx, ed, f0, None, rows, R)
    states = []
    for s, h in steps:                                                  # the states from pf_cnf_step on exactly these steps
        states.append(y)
        y1, f1 = torch.empty_like(y), torch.empty_like(y)
        eng.step(block, y, f0, s, h, reverse, ctx, ed, y1, f1, rows, R)
        y, f0 = y1, f1
    states = torch.stack(states).contiguous()
    steps_dev = torch.tensor(steps, dtype=torch.float32, device=DEV).reshape(-1, 2)

    def sweep(ctxbar, grad):
        yb = ybar_in.to(DEV)
        eng.tape_vjp(block, states, steps_dev, sgn, ctx, ed, yb, ctxbar, grad, rows, R)
        torch.cuda.synchronize()
        return yb.cpu(), ctxbar.cpu(), grad.cpu()

    ctxbar, grad = torch.zeros(T, CNF_CTX, device=DEV), torch.zeros(CNF_GRAD, device=DEV)
    first = sweep(ctxbar, grad)
    second = sweep(ctxbar, grad)
    third = sweep(torch.zeros(T, CNF_CTX, device=DEV), torch.zeros(CNF_GRAD, device=DEV))

    gx, gl = ybar_in[:, :3], ybar_in[:, 3]
    ref = {d: G.steps_backward(sd, block, x, c, e, reverse, steps, d, gx, gl) for d in (torch.float64, torch.float32)}
    slots = {d: _slot_sweep(sd, block, x, c, e, reverse, steps, d, ybar_in) for d in (torch.float64, torch.float32)}
    return dict(first=first, second=second, third=third, ref=ref, slots=slots, c=c, ybar_in=ybar_in, Hplain=eng.Hplain.cpu())


@pytest.mark.parametrize("name", list(KCASES))
def test_tape_vjp_matches_float64_sweep(name):
    """(0, 200, 1): the plain case, also with a single step; (5, 100, 4): four rows per point; (3, 67, 3): 15 rows per wave tile
    and a last workgroup with one wave of rows; (2, 10, 4): less than one tile; (1, 16500, 1), two steps: 258 tiles on 256
    workgroups, so two of them keep their accumulators over a second tile and over its steps.  ybar columns 0..2, the per-point
    ctxbar slots, the context gradient and all fifteen state-dict-keyed gradients; ybar's column 3 passes through; layer 3's
    replicated ctxbar columns stay untouched."""
    from puflow_amd.packing import CNF_CTX_SLOTS, unpack_cnf_grads
    block, T, R, reverse, hs = KCASES[name]
    r = _kernel_run(name)
    yb, cb, gr = r["first"]
    ref64, ref32 = dict(r["ref"][torch.float64]), dict(r["ref"][torch.float32])       # copies: the slots are added below
    got = {"x": yb[:, :3], "c": cb.double() @ r["Hplain"].double()}
    got.update(unpack_cnf_grads(block, gr.double(), cb.double().t() @ r["c"].double(), cb.double().sum(0)))
    keys = ["x", "c"] + G.block_keys(block)
    assert sorted(got) == sorted(keys)
    lines = []
    for k in keys:
        assert got[k].shape == ref64[k].shape, k
        err, err32 = G.rel_err(got[k], ref64[k]), G.rel_err(ref32[k], ref64[k])
        lines.append(f"  {k:66s} err32 {err32:.2e}  gpu {err:.2e}  max|ref| {float(ref64[k].abs().max()):.2e}")
    for l in range(3):
        for kind, (c0, n) in ((f"gate_pre{l}", CNF_CTX_SLOTS[2 * l]), (f"bias_pre{l}", CNF_CTX_SLOTS[2 * l + 1])):
            s64, s32 = r["slots"][torch.float64][kind], r["slots"][torch.float32][kind]
            got[kind], ref64[kind], ref32[kind] = cb[:, c0:c0 + n], s64, s32
            keys.append(kind)
            lines.append(f"  {kind:66s} err32 {G.rel_err(s32, s64):.2e}  gpu {G.rel_err(cb[:, c0:c0 + n], s64):.2e}  "
                         f"max|ref| {float(s64.abs().max()):.2e}")
    print(f"\ntape_vjp {name}: {len(hs)} steps\n" + "\n".join(lines))
    assert all(float(ref64[k].abs().max()) > 0 for k in keys)
    for k in keys:
        _bound_ok(G.rel_err(got[k], ref64[k]), G.rel_err(ref32[k], ref64[k]), k)
    assert torch.equal(yb[:, 3], r["ybar_in"][:, 3])                  # log p never enters f: its cotangent passes through
    assert torch.all(cb[:, 259:272] == 0) and torch.all(cb[:, 275:288] == 0)


@pytest.mark.parametrize("name", list(KCASES))
def test_tape_vjp_accumulates_into_ctxbar_and_grad(name):
    r = _kernel_run(name)
    (yb1, cb1, g1), (yb2, cb2, g2) = r["first"], r["second"]
    assert G.rel_err(cb2, 2 * cb1.double()) <= 1e-6 and G.rel_err(g2, 2 * g1.double()) <= 1e-6
    assert torch.equal(yb1, yb2)                                        # ybar is overwritten, from the same input: the same bits


def test_tape_vjp_is_bit_reproducible():
    r = _kernel_run("b3_T67_R3_rev")
    for a, b in zip(r["first"], r["third"]):
        assert torch.equal(a, b)


# ---- 5, 6. through flow_block ------------------------------------------------------------------------------------------------------
CASES = {"b0_fwd_R1": (0, 200, 1, False, True), "b5_rev_R4": (5, 100, 4, True, False), "b3_rev_R3": (3, 67, 3, True, True)}


def _net():
    from puflow_amd.cnf import PointInterpFlow
    net = PointInterpFlow(3)
    net.load_state_dict(_sd(), strict=True)
    return net.to(DEV).train()


def _case(name):
    block, T, R, reverse, use_logp = CASES[name]
    g, x, c, e = _inputs(block, T, R, 40 + block)                        # tests/test_gpu_cnf_grad.py's inputs
    gx = torch.randn(T * R, 3, generator=g)
    gl = torch.randn(T * R, generator=g) if use_logp else torch.zeros(T * R)
    return block, R, reverse, x, c, e, gx, gl


@functools.lru_cache(maxsize=None)
def _device_tape(name):
    block, R, reverse, x, c, e, _, _ = _case(name)
    net = _net()
    with torch.no_grad():
        ox, ol = net.flow_block(block, x.to(DEV), c.to(DEV), e.to(DEV), R, reverse)
        steps = list(net.last_block_steps)
        net.tape_capacity[(block, reverse)] = 1                           # a tape of one step: filled, doubled, started again
        ox1, ol1 = net.flow_block(block, x.to(DEV), c.to(DEV), e.to(DEV), R, reverse)
        steps1 = list(net.last_block_steps)
    sd = _sd()
    ref = {d: G.steps_forward(sd, block, x, c, e, reverse, steps, d) for d in (torch.float64, torch.float32)}
    return dict(out=(ox.cpu(), ol.cpu()), steps=steps, out1=(ox1.cpu(), ol1.cpu()), steps1=steps1, ref=ref)


@pytest.mark.parametrize("name", list(CASES))
def test_device_recorded_tape(name):
    """The step list the device-side controller records: starts at the start time, contiguous in the controller's fp32
    arithmetic (s' = s + h, bit for bit), ends at the end time; the block's outputs are the float64 forward on that list; a tape
    that starts too short gives the same list and the same bits."""
    block, T, R, reverse, _ = CASES[name]
    r = _device_tape(name)
    steps = r["steps"]
    T_end = float(_sd()[G.end_key(block)]) ** 2
    t0, t1 = (-T_end, 0.0) if reverse else (0.0, T_end)
    print(f"\n{name}: {len(steps)} recorded steps")
    assert len(steps) >= 2
    assert steps[0][0] == _f32(t0)
    for (s, h), (s_next, _) in zip(steps[:-1], steps[1:]):
        assert all(_f32(v) == v for v in (s, h)) and h > 0
        assert s_next == float(torch.tensor(s, dtype=torch.float32) + torch.tensor(h, dtype=torch.float32)), (s, h, s_next)
    assert abs(steps[-1][0] + steps[-1][1] - t1) < 1e-6
    for k, got in zip(("out_x", "out_l"), r["out"]):
        ref64, ref32 = (r["ref"][d][0 if k == "out_x" else 1] for d in (torch.float64, torch.float32))
        err, err32 = G.rel_err(got, ref64), G.rel_err(ref32, ref64)
        print(f"  {k} err32 {err32:.2e}  gpu {err:.2e}")
        _bound_ok(err, err32, k)
    assert r["steps1"] == steps
    assert torch.equal(r["out1"][0], r["out"][0]) and torch.equal(r["out1"][1], r["out"][1])


def test_fused_and_per_evaluation_sweeps_agree_with_float64():
    """The one-launch sweep and the per-evaluation sweep behind the same host-controlled forward: the same step list, and every
    gradient of both within the bound of float64 autograd on that list (not bit for bit: the summation order differs)."""
    name = "b5_rev_R4"
    block, R, reverse, x, c, e, gx, gl = _case(name)
    loss = lambda ox, ol: (ox * gx.to(ox)).sum() + (ol * gl.to(ol)).sum()
    runs = {}
    for sweep in ("fused", "per_eval"):
        net = _net()
        xd, cd_ = x.to(DEV).requires_grad_(True), c.to(DEV).requires_grad_(True)
        ox, ol = net.flow_block(block, xd, cd_, e.to(DEV), R, reverse, sweep=sweep, controller="host")
        loss(ox, ol).backward()
        got = {"x": xd.grad.cpu(), "c": cd_.grad.cpu()}
        got.update({f"flow_blocks.{block}.{n}": p.grad.detach().cpu() for n, p in net.flow_blocks[block].named_parameters()})
        runs[sweep] = (list(net.last_block_steps), got)
    steps = runs["fused"][0]
    assert steps == runs["per_eval"][0] and len(steps) >= 2
    sd = _sd()
    ek = G.end_key(block)
    ref = {}
    for d in (torch.float64, torch.float32):
        ref[d] = G.autograd_grads(sd, block, x, c, e, reverse, steps, d, loss)
        ref[d][ek] = G.steps_backward(sd, block, x, c, e, reverse, steps, d, gx, gl)[ek]
    for k in ["x", "c"] + G.block_keys(block) + [ek]:
        err32 = G.rel_err(ref[torch.float32][k], ref[torch.float64][k])
        errs = {s: G.rel_err(runs[s][1][k], ref[torch.float64][k]) for s in runs}
        print(f"  {k:66s} err32 {err32:.2e}  fused {errs['fused']:.2e}  per_eval {errs['per_eval']:.2e}")
        for s in runs:
            _bound_ok(errs[s], err32, (s, k))
