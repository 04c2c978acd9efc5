"""Gradient through a CNF flow block on the GPU (csrc/cnf_bwd.hip: pf_cnf_rhs_vjp; puflow_amd/cnf.py: flow_block) against the
float64 CPU references: one right-hand-side VJP against oracle/cnf_ref.py::rhs_vjp, the taped forward and the block's gradients
against tests/cnf_grad_ref.py on the step list the GPU recorded.

Error measure everywhere: max|got - ref64| / max(1, max|ref64|) per tensor.
  * one evaluation: 2e-5, the figure tests/test_gpu_cnf.py::test_rhs_matches_autograd_oracle has for this arithmetic (hardware
    exp / rcp, split-fp16 products);
  * through the steps: max(2e-5, 4 x err32), err32 = the same helper in float32 on the CPU against float64 on the same steps
    (the factor 4: hardware transcendentals at ~2e-7 absolute each and the fp16-split products on top of plain fp32 rounding),
    on seeds for which err32 <= 1e-4 so that a wrong term cannot hide."""
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


def _inputs(block, T, R, seed, state_cols):
    sd = _sd()
    g = torch.Generator().manual_seed(seed)
    cd = sd[f"flow_blocks.{block}.cnf.odefunc.diffeq.layers.0._hyper_gate.weight"].shape[1] - 1
    c = torch.randn(T, cd, generator=g) * 0.7
    e = torch.randn(T, 3, generator=g)
    y = torch.randn(T * R, state_cols, generator=g) * 0.8
    return g, y, c, e


# ---- 1. one evaluation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block,T,R,sgn", [(0, 200, 1, 1.0), (5, 200, 4, -1.0), (3, 67, 3, -1.0), (2, 10, 4, 1.0), (1, 16500, 1, -1.0)])
def test_rhs_vjp_matches_float64_oracle(block, T, R, sgn):
    """(3, 67, 3): 201 rows, 15 rows per wave tile and a last workgroup with one wave's worth of rows; (2, 10, 4): 40 rows, less
    than one workgroup tile; (1, 16500, 1): 258 workgroup tiles on the 256 workgroups of the largest grid, so two of them keep
    their accumulators over a second tile.  ybar, the per-point context gradients and every state-dict-keyed gradient; a second
    call into the same buffers doubles what accumulates and leaves ybar as it was."""
    from puflow_amd.cnf import _BlockTapeEngine
    from puflow_amd.packing import CNF_CTX, CNF_CTX_SLOTS, CNF_GRAD, unpack_cnf_grads
    sd = _sd()
    g, y, c, e = _inputs(block, T, R, block, 4)
    rows = T * R
    kbar = torch.randn(rows, 4, generator=g)
    t = 0.137
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    cr, er = torch.repeat_interleave(c, R, dim=0).double(), torch.repeat_interleave(e, R, dim=0).double()
    ref = C.rhs_vjp(sd64, block, t, y[:, :3].double(), cr, er, sgn * kbar[:, :3].double(), sgn * kbar[:, 3].double())
    p = f"flow_blocks.{block}.cnf.odefunc.diffeq.layers"
    tc = torch.cat([torch.full((rows, 1), t, dtype=torch.float64), cr], dim=-1)
    ref_keyed = {}
    for l in range(3):
        ref_keyed[f"{p}.{l}._layer.weight"], ref_keyed[f"{p}.{l}._layer.bias"] = ref[f"W{l}"], ref[f"b{l}"]
        ref_keyed[f"{p}.{l}._hyper_gate.weight"] = ref[f"gate_pre{l}"].t() @ tc
        ref_keyed[f"{p}.{l}._hyper_gate.bias"] = ref[f"gate_pre{l}"].sum(0)
        ref_keyed[f"{p}.{l}._hyper_bias.weight"] = ref[f"bias_pre{l}"].t() @ tc

    eng = _BlockTapeEngine({k: v for k, v in sd.items() if k.startswith(f"flow_blocks.{block}.")}, block, torch.device(DEV))
    cd_, ed = c.to(DEV), e.to(DEV)
    ctx = eng.context(block, cd_)
    yd, kd = y.to(DEV), kbar.to(DEV)
    ybar = torch.full((rows, 4), 7.0, device=DEV)                      # overwritten, column 3 included
    ctxbar = torch.zeros(T, CNF_CTX, device=DEV)
    grad = torch.zeros(CNF_GRAD, device=DEV)
    eng.vjp(block, yd, kd, t, sgn, ctx, ed, ybar, ctxbar, grad, rows, R)
    torch.cuda.synchronize()
    yb1, cb1, g1 = ybar.cpu(), ctxbar.cpu(), grad.cpu()
    eng.vjp(block, yd, kd, t, sgn, ctx, ed, ybar, ctxbar, grad, rows, R)
    torch.cuda.synchronize()
    yb2, cb2, g2 = ybar.cpu(), ctxbar.cpu(), grad.cpu()

    errs = {"ybar": G.rel_err(yb1[:, :3], ref["y"])}
    assert torch.all(yb1[:, 3] == 0)
    for l in range(3):
        (g0, n), (b0, _) = CNF_CTX_SLOTS[2 * l], CNF_CTX_SLOTS[2 * l + 1]
        errs[f"gate_pre{l}"] = G.rel_err(cb1[:, g0:g0 + n], ref[f"gate_pre{l}"].view(T, R, n).sum(1))
        errs[f"bias_pre{l}"] = G.rel_err(cb1[:, b0:b0 + n], ref[f"bias_pre{l}"].view(T, R, n).sum(1))
    assert torch.all(cb1[:, 259:272] == 0) and torch.all(cb1[:, 275:288] == 0)       # layer 3's replicated slots stay untouched
    got = unpack_cnf_grads(block, g1.double(), cb1.double().t() @ c.double(), cb1.double().sum(0))
    assert sorted(got) == sorted(ref_keyed)
    for k in ref_keyed:
        assert got[k].shape == ref_keyed[k].shape, k
        errs[k] = G.rel_err(got[k], ref_keyed[k])
    print(f"rhs_vjp block {block} T {T} R {R} sgn {sgn:+.0f}: " + ", ".join(f"{k.split('layers.')[-1]} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= 2e-5, (k, v)
    assert torch.equal(yb1, yb2)
    assert G.rel_err(cb2, 2 * cb1.double()) <= 1e-6 and G.rel_err(g2, 2 * g1.double()) <= 1e-6


# ---- 2 - 4. the block through its recorded steps -------------------------------------------------------------------------------
CASES = {"b0_fwd_R1": (0, 200, 1, False, True), "b5_rev_R4": (5, 100, 4, True, False), "b3_rev_R3": (3, 67, 3, True, True)}


@functools.lru_cache(maxsize=None)
def _run(name):
    """One case: the GPU's outputs and gradients (after one and after two backward passes), the float64 references on the
    step list the GPU recorded, and err32 (the helper in float32 on those steps) per tensor."""
    from puflow_amd.cnf import PointInterpFlow
    block, T, R, reverse, use_logp = CASES[name]
    sd = _sd()
    g, x, c, e = _inputs(block, T, R, 40 + block, 3)
    gx = torch.randn(T * R, 3, generator=g)
    gl = torch.randn(T * R, generator=g) if use_logp else torch.zeros(T * R)       # x' only: what g sees in training
    loss = lambda ox, ol: (ox * gx.to(ox)).sum() + (ol * gl.to(ol)).sum()
    net = PointInterpFlow(3)
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).train()                                                    # flow_block works whatever .training says
    params = {f"flow_blocks.{block}.{n}": p for n, p in net.flow_blocks[block].named_parameters()}
    xd, cd_ = x.to(DEV).requires_grad_(True), c.to(DEV).requires_grad_(True)
    ox, ol = net.flow_block(block, xd, cd_, e.to(DEV), R, reverse)
    steps = list(net.last_block_steps)
    loss(ox, ol).backward()
    got = {"out_x": ox.detach().cpu(), "out_l": ol.detach().cpu(), "x": xd.grad.cpu(), "c": cd_.grad.cpu()}
    got.update({k: p.grad.detach().cpu().clone() for k, p in params.items()})
    ox2, ol2 = net.flow_block(block, x.to(DEV), c.to(DEV), e.to(DEV), R, reverse)      # a fresh forward: grads accumulate
    loss(ox2, ol2).backward()
    twice = {k: p.grad.detach().cpu().clone() for k, p in params.items()}
    untouched = all(p.grad is None for n, p in net.named_parameters() if not n.startswith(f"flow_blocks.{block}."))
    ref64 = G.autograd_grads(sd, block, x, c, e, reverse, steps, torch.float64, loss)
    ref32 = G.autograd_grads(sd, block, x, c, e, reverse, steps, torch.float32, loss)
    ek = G.end_key(block)
    ref64[ek] = G.steps_backward(sd, block, x, c, e, reverse, steps, torch.float64, gx, gl)[ek]
    ref32[ek] = G.steps_backward(sd, block, x, c, e, reverse, steps, torch.float32, gx, gl)[ek]
    err32 = {k: G.rel_err(ref32[k], ref64[k]) for k in ref64}
    err = {k: G.rel_err(got[k], ref64[k]) for k in ref64}
    disc = float(G.end_time_autograd(sd, block, x, c, e, reverse, steps, loss))
    print(f"\n{name}: {len(steps)} accepted steps; d/d sqrt_end_time: continuous formula {float(ref64[ek]):+.6e}, autograd with "
          f"the steps scaled by T {disc:+.6e}")
    for k in ref64:
        print(f"  {k:66s} err32 {err32[k]:.2e}  gpu {err[k]:.2e}  max|ref| {float(ref64[k].abs().max()):.2e}")
    return dict(got=got, twice=twice, ref64=ref64, err32=err32, err=err, steps=steps, untouched=untouched, ek=ek)


def _check(r, keys):
    for k in keys:
        assert r["err32"][k] <= 1e-4, ("the float32 yardstick is too coarse for this seed", k, r["err32"][k])
        assert r["err"][k] <= max(2e-5, 4 * r["err32"][k]), (k, r["err"][k], r["err32"][k])


@pytest.mark.parametrize("name", list(CASES))
def test_taped_forward_matches_float64_on_the_recorded_steps(name):
    r = _run(name)
    block, T, R, reverse, _ = CASES[name]
    T_end = float(_sd()[G.end_key(block)]) ** 2
    s0, (sl, hl) = r["steps"][0][0], r["steps"][-1]
    assert len(r["steps"]) >= 2 and abs(s0 - (-T_end if reverse else 0.0)) < 1e-6 and abs(sl + hl - (0.0 if reverse else T_end)) < 1e-6
    _check(r, ["out_x", "out_l"])


@pytest.mark.parametrize("name", list(CASES))
def test_block_gradients_match_float64_autograd_on_the_recorded_steps(name):
    r = _run(name)
    block = CASES[name][0]
    keys = ["x", "c"] + G.block_keys(block)
    assert all(float(r["ref64"][k].abs().max()) > 0 for k in keys)
    _check(r, keys)
    assert r["untouched"]                                       # no other parameter of the model got a gradient
    for k in G.block_keys(block) + [r["ek"]]:                   # a second backward of a fresh forward doubles .grad
        assert G.rel_err(r["twice"][k], 2 * r["got"][k].double()) <= 1e-6, k


@pytest.mark.parametrize("name", list(CASES))
def test_sqrt_end_time_gradient_is_the_continuous_formula(name):
    r = _run(name)
    assert abs(float(r["ref64"][r["ek"]])) > 0
    _check(r, [r["ek"]])
