"""One-launch replay of a CNF block on a given step list (csrc/cnf_replay.hip: pf_cnf_replay; puflow_amd/cnf.py: _CnfKernels.replay,
flow_block(controller="schedule")) on the GPU.

  1. bit identity with the path it replaces: the taped device controller's states, f_start and f_end on the steps it recorded;
  2. float64: a hand-made non-uniform schedule against cnf_grad_ref.steps_forward, bound max(2e-5, 4 x err32) in rel_err, err32 =
     the same helper in float32, counted only if err32 <= 1e-4 (the project's bar for quantities that went through the steps);
  3. invariances: x_stride 3 / 4, states / errsq NULL or not, two runs of errsq;
  4. the embedded error estimate against tests/cnf_err_ref.py in float64;
  5. gradients through flow_block(controller="schedule") against cnf_grad_ref.autograd_grads, the bound of tests/test_gpu_cnf_grad.py.

Weights: synth_cnf_state_dict(7, CNF_PU1K_DYNAMICS, CNF_PU1K_END_TIMES), the bench's stand-in for the trained checkpoint; inputs
as tests/test_gpu_cnf_tape.py::_inputs makes them."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import cnf_err_ref as E
import cnf_grad_ref as G
from puflow_amd.weights import CNF_PU1K_DYNAMICS, CNF_PU1K_END_TIMES, synth_cnf_state_dict

DEV = "cuda:0"
GRID = (0.0, 0.02, 0.1, 0.3, 0.6, 1.0)                     # the hand-made non-uniform schedule of 2. and 5.


@functools.lru_cache(maxsize=None)
def _sd():
    return synth_cnf_state_dict(7, CNF_PU1K_DYNAMICS, CNF_PU1K_END_TIMES)


def _inputs(block, T, R, seed):
    sd = _sd()
    g = torch.Generator().manual_seed(seed)
    cd = sd[f"flow_blocks.{block}.cnf.odefunc.diffeq.layers.0._hyper_gate.weight"].shape[1] - 1
    c = torch.randn(T, cd, generator=g) * 0.7
    e = torch.randn(T, 3, generator=g)
    x = torch.randn(T * R, 3, generator=g) * 0.8
    return g, x, c, e


@functools.lru_cache(maxsize=None)
def _engine(block):
    from puflow_amd.cnf import _BlockTapeEngine
    return _BlockTapeEngine({k: v for k, v in _sd().items() if k.startswith(f"flow_blocks.{block}.")}, block, torch.device(DEV))


def _grid_steps(block, reverse, grid):
    """The fp32 (s, h) list of `grid` on block's interval, as the library makes it -> (host list of python floats, [n, 2] tensor)."""
    from puflow_amd.cnf import schedule_step_lists
    T_end = float(_sd()[G.end_key(block)].double()) ** 2
    g = torch.tensor(grid, dtype=torch.float64)
    st = schedule_step_lists((g[1:] - g[:-1])[None], torch.tensor([len(grid) - 2]), torch.tensor([reverse]),
                             torch.tensor([T_end], dtype=torch.float64))[0]
    return [(float(s), float(h)) for s, h in st.tolist()], st


def _bound_ok(err, err32, what):
    assert err32 <= 1e-4, ("the float32 yardstick is too coarse for this seed", what, err32)
    assert err <= max(2e-5, 4 * err32), (what, err, err32)


def _replay_raw(eng, block, x, steps_dev, reverse, ctx, e, R, states=False, errsq=False, f_ends=True):
    """pf_cnf_replay called directly, any combination of its nullable outputs -> dict of what was asked for (+ y)."""
    from puflow_amd import _lib
    from puflow_amd.cnf import ATOL, RTOL
    rows, n = x.shape[0], steps_dev.shape[0]
    out = dict(y=torch.full((rows, 4), float("nan"), device=DEV))
    if states:
        out["states"] = torch.full((n + 1, rows, 4), float("nan"), device=DEV)
    if f_ends:
        out["f_start"], out["f_end"] = (torch.full((rows, 4), float("nan"), device=DEV) for _ in range(2))
    ws = None
    if errsq:
        out["errsq"] = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
        ws = torch.empty(eng.lib.pf_cnf_replay_workspace_bytes(rows, n) // 8, dtype=torch.float64, device=DEV)
    ptr = lambda k: out[k].data_ptr() if k in out else None
    _lib.check(eng.lib.pf_cnf_replay(x.data_ptr(), int(x.stride(0)), steps_dev.data_ptr(), n, 1 if reverse else 0, ctx.data_ptr(),
                                     e.data_ptr(), eng.rec[block].data_ptr(), ptr("states"), ptr("y"), ptr("f_start"), ptr("f_end"),
                                     ptr("errsq"), RTOL, ATOL, rows, R, ws.data_ptr() if ws is not None else None,
                                     torch.cuda.current_stream().cuda_stream), "pf_cnf_replay")
    torch.cuda.synchronize()
    return out


# ---- 1. the bits of the taped adaptive path -----------------------------------------------------------------------------------------
# (block, reverse, R, T | rows): rows not a multiple of 64 on the long block, whose integration rejects attempts; four rows per
# point (context rows through LDS); three rows per point, points straddling 16-row groups; more tiles than workgroups
BIT_CASES = {"b5_fwd_R1_T50": (5, False, 1, 50), "b5_rev_R4_T37": (5, True, 4, 37), "b4_rev_R3_T43": (4, True, 3, 43),
             "b0_fwd_R1_grid_stride": (0, False, 1, 1024 * 64 + 197)}


@pytest.mark.parametrize("name", list(BIT_CASES))
def test_replay_of_the_recorded_steps_has_the_bits_of_the_taped_controller(name):
    block, reverse, R, T = BIT_CASES[name]
    _, x, c, e = _inputs(block, T, R, 90 + block)
    eng = _engine(block)
    xd, cd_, ed = x.to(DEV), c.to(DEV), e.to(DEV)
    y, tape = eng.tape_forward(block, xd, cd_, ed, R, reverse)
    n = len(tape["steps"])
    print(f"\n{name}: {n} accepted steps, {tape['took'] - n} rejected attempts, rows {T * R}")
    assert n >= 2
    y2, tape2 = eng.replay(block, xd, tape["steps_dev"].contiguous(), reverse, tape["ctx"], ed, R, tape=True)
    torch.cuda.synchronize()
    assert tape2["states"].shape == (n + 1, T * R, 4)
    assert torch.equal(tape2["states"][:n], tape["states"])
    assert torch.equal(tape2["states"][n], y) and torch.equal(y2, y)
    assert torch.equal(tape2["f_start"], tape["f_start"])
    assert torch.equal(tape2["f_end"], tape["f_end"])
    assert bool(torch.isfinite(y2).all()) and not torch.equal(y2[:, :3], xd)


# ---- 2. float64 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("R", [1, 4])
def test_replay_matches_float64_on_a_hand_made_schedule(R, reverse):
    block, T = 4, 32
    _, x, c, e = _inputs(block, T, R, 60 + R)
    steps, st = _grid_steps(block, reverse, GRID)
    assert len(steps) == 5
    eng = _engine(block)
    ctx = eng.context(block, c.to(DEV))
    y, _ = eng.replay(block, x.to(DEV), st.to(DEV), reverse, ctx, e.to(DEV), R)
    ref = {d: G.steps_forward(_sd(), block, x, c, e, reverse, steps, d) for d in (torch.float64, torch.float32)}
    for k, got in (("x'", y[:, :3].cpu()), ("dlogp", y[:, 3].cpu())):
        r64, r32 = (ref[d][0 if k == "x'" else 1].detach() for d in (torch.float64, torch.float32))
        err, err32 = G.rel_err(got, r64), G.rel_err(r32, r64)
        print(f"\nblock 4 R {R} reverse {reverse} {k}: err32 {err32:.2e}  gpu {err:.2e}  max|ref| {float(r64.abs().max()):.2e}")
        assert float(r64.abs().max()) > 0
        _bound_ok(err, err32, k)


# ---- 3. invariances -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block,reverse,R,T", [(4, True, 4, 37), (1, False, 1, 150)])
def test_replay_invariances(block, reverse, R, T):
    g, x, c, e = _inputs(block, T, R, 21)
    _, st = _grid_steps(block, reverse, GRID)
    eng = _engine(block)
    st, ed = st.to(DEV), e.to(DEV)
    ctx = eng.context(block, c.to(DEV))
    x3 = x.to(DEV)
    x4 = torch.cat([x, torch.randn(T * R, 1, generator=g)], dim=1).to(DEV)            # a fourth column that must not be read
    full = _replay_raw(eng, block, x3, st, reverse, ctx, ed, R, states=True, errsq=True)
    assert all(bool(torch.isfinite(v).all()) for v in full.values()) and float(full["errsq"].min()) > 0
    assert torch.equal(full["states"][0, :, :3], x3) and not bool(full["states"][0, :, 3].any())
    assert torch.equal(full["states"][-1], full["y"])
    other = _replay_raw(eng, block, x4, st, reverse, ctx, ed, R, states=True, errsq=True)
    for k in full:
        assert torch.equal(full[k], other[k]), ("x_stride 4", k)                     # (errsq too: the second run's bits)
    for states, errsq in ((False, True), (True, False), (False, False)):
        got = _replay_raw(eng, block, x3, st, reverse, ctx, ed, R, states=states, errsq=errsq)
        for k in got:
            assert torch.equal(got[k], full[k]), (states, errsq, k)
    bare = _replay_raw(eng, block, x3, st, reverse, ctx, ed, R, f_ends=False)
    assert torch.equal(bare["y"], full["y"])


# ---- 4. the error estimate ----------------------------------------------------------------------------------------------------------
ERR_BOUND = 3.6e-5                                        # 4 x the deviation measured once (the test's docstring); never above 5e-2


def test_error_ratios_match_the_float64_helper():
    """Block 4, reverse, R = 4, T = 64, seed 11, two uniform steps: the float64 helper gives ratios 1.654 and 0.806 (the float32
    CPU helper agrees to five digits).  Measured once on an MI355X (profiles/cnf_schedule/error_ratio.txt): the device's ratios
    1.6544013 and 0.8059071 deviate from float64 by 2.4e-6 and 8.9e-6 relative (the CPU float32 helper by 4.5e-6 and 3.2e-6; the
    hardware exp / rcp activations add ~2e-7 absolute per evaluation).  The bound is 4 x the larger, 3.6e-5; a dropped tableau
    term or a missing h moves a ratio by O(1)."""
    block, reverse, R, T = 4, True, 4, 64
    _, x, c, e = _inputs(block, T, R, 11)
    steps, st = _grid_steps(block, reverse, (0.0, 0.5, 1.0))
    eng = _engine(block)
    ctx = eng.context(block, c.to(DEV))
    got = _replay_raw(eng, block, x.to(DEV), st.to(DEV), reverse, ctx, e.to(DEV), R, errsq=True)
    n_tot = float(T * R * 4 + c.numel() * R)
    ratios = [float(v / n_tot) ** 0.5 for v in got["errsq"].cpu()]
    ref, _ = E.step_error_ratios(_sd(), block, x, c, e, reverse, steps, torch.float64)
    ref32, _ = E.step_error_ratios(_sd(), block, x, c, e, reverse, steps, torch.float32)
    dev = [abs(a - b) / b for a, b in zip(ratios, ref)]
    print(f"\nerror ratios: gpu {ratios}  float64 {ref}  float32 cpu {ref32}  relative deviation {dev}")
    assert abs(ref[0] - 1.65) < 0.01 and abs(ref[1] - 0.81) < 0.01
    assert all(r >= 0.05 for r in ref)                     # below that the estimate is rounding noise
    for d in dev:
        assert d <= ERR_BOUND, (dev, ERR_BOUND)


# ---- 5. gradients through flow_block -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse,R", [(False, 1), (True, 4)])
def test_flow_block_on_a_schedule_matches_float64_autograd(reverse, R):
    from puflow_amd.cnf import PointInterpFlow
    block, T = 4, 32
    g, x, c, e = _inputs(block, T, R, 60 + R)
    gx, gl = torch.randn(T * R, 3, generator=g), torch.randn(T * R, generator=g)
    loss = lambda ox, ol: (ox * gx.to(ox)).sum() + (ol * gl.to(ol)).sum()
    net = PointInterpFlow(3)
    net.load_state_dict(_sd(), strict=True)
    net = net.to(DEV).train()
    xd, cd_ = x.to(DEV).requires_grad_(True), c.to(DEV).requires_grad_(True)
    ox, ol = net.flow_block(block, xd, cd_, e.to(DEV), R, reverse, controller="schedule", schedule=GRID)
    loss(ox, ol).backward()
    steps, _ = _grid_steps(block, reverse, GRID)
    tape = net.last_block_tape
    assert [(float(s), float(h)) for s, h in tape["steps_dev"].cpu().tolist()] == steps     # made on the device: the same list
    assert tape["states"].shape == (len(steps) + 1, T * R, 4) and net.check_train_logs() == 0
    got = {"out_x": ox.detach().cpu(), "out_l": ol.detach().cpu(), "x": xd.grad.cpu(), "c": cd_.grad.cpu()}
    got.update({f"flow_blocks.{block}.{n}": p.grad.detach().cpu() for n, p in net.flow_blocks[block].named_parameters()})
    ek = G.end_key(block)
    ref = {}
    for d in (torch.float64, torch.float32):
        ref[d] = G.autograd_grads(_sd(), block, x, c, e, reverse, steps, d, loss)
        ref[d][ek] = G.steps_backward(_sd(), block, x, c, e, reverse, steps, d, gx, gl)[ek]   # the continuous end-time formula
    print()
    for k in ["out_x", "out_l", "x", "c"] + G.block_keys(block) + [ek]:
        err, err32 = G.rel_err(got[k], ref[torch.float64][k]), G.rel_err(ref[torch.float32][k], ref[torch.float64][k])
        print(f"  {k:66s} err32 {err32:.2e}  gpu {err:.2e}  max|ref| {float(ref[torch.float64][k].abs().max()):.2e}")
        assert float(ref[torch.float64][k].abs().max()) > 0, k
        _bound_ok(err, err32, k)
    with pytest.raises(ValueError):
        net.flow_block(block, xd, cd_, e.to(DEV), R, reverse, controller="schedule")
    with pytest.raises(ValueError):
        net.flow_block(block, xd, cd_, e.to(DEV), R, reverse, controller="schedule", schedule=(0.0, 0.6, 0.4, 1.0))
