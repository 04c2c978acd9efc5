"""Reference of a differentiable CNF flow block on a FIXED list of Dormand-Prince steps, built from oracle/cnf_ref.py.
TEST INFRASTRUCTURE ONLY (a helper module like tests/poisson_ref.py; tests/test_cnf_grad_ref.py pins it, tests/test_gpu_cnf_grad.py
holds `PointInterpFlow.flow_block` to it).

  steps_forward    the block's forward on a given step list [(s, h), ..] (solver time: s = -t and f' = -f when reversed, as in
                   oracle/cnf_ref.py::cnf_block), differentiable by torch (Hutchinson term with create_graph=True);
  steps_backward   the reverse sweep of DESIGN 9a written out with oracle `rhs_vjp`, no autograd through the steps: per step
                       y0bar = y1bar;  kbar_j = h b_j y1bar  (j = 1..6)
                       for j = 6 .. 1:  Ybar_j = VJP_F(Y_j, t_j; kbar_j);  y0bar += Ybar_j;  kbar_m += h a_jm Ybar_j  (m < j)
                   plus the continuous end-time formula for sqrt_end_time;
  autograd_grads   gradients of a loss through steps_forward (what steps_backward and the GPU are compared with).
x [rows,3] with rows = T R (the R rows of a point adjacent), c [T,cd], e [T,3]."""
from __future__ import annotations

from typing import Callable, Dict, List, Sequence, Tuple

import torch

from oracle import cnf_ref as C

Tensor = torch.Tensor
B6 = C.DP_BETA[5]
ALPHA = [0.0] + C.DP_ALPHA[:5]


def block_keys(i: int) -> List[str]:
    p = f"flow_blocks.{i}.cnf.odefunc.diffeq.layers"
    return [f"{p}.{l}.{n}" for l in range(3) for n in ("_layer.weight", "_layer.bias", "_hyper_gate.weight", "_hyper_gate.bias",
                                                        "_hyper_bias.weight")]


def end_key(i: int) -> str:
    return f"flow_blocks.{i}.cnf.sqrt_end_time"


def _cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def _rhs_graph(sd, i: int, t, Y: Tensor, cr: Tensor, er: Tensor) -> Tensor:
    """oracle `rhs` kept on the autograd graph: (f, -e^T (df/dy) e) at net time t (a float or a 0-d tensor)."""
    y = Y[:, :3]
    if not y.requires_grad:
        y = y.detach().requires_grad_(True)
    tcol = torch.ones((y.shape[0], 1), dtype=y.dtype) * t
    dy = C.odenet(sd, i, torch.cat([tcol, cr], dim=-1), y)
    e_dzdx = torch.autograd.grad(dy, y, er, create_graph=True)[0]
    return torch.cat([dy, -(e_dzdx * er).sum(-1, keepdim=True)], dim=-1)


def steps_forward(sd, i: int, x: Tensor, c: Tensor, e: Tensor, reverse: bool, steps: Sequence[Tuple], dtype=torch.float64):
    """-> (x' [rows,3], delta logp [rows]).  Differentiable with respect to x, c and whatever entries of sd require grad (sd is
    used as given when its tensors already have `dtype`); the entries of `steps` may be tensors."""
    sd = _cast(sd, dtype)
    x, c, e = x.to(dtype), c.to(dtype), e.to(dtype)
    R = x.shape[0] // c.shape[0]
    cr, er = torch.repeat_interleave(c, R, dim=0), torch.repeat_interleave(e, R, dim=0)
    sgn = -1.0 if reverse else 1.0
    Y = torch.cat([x, torch.zeros(x.shape[0], 1, dtype=dtype)], dim=-1)
    with torch.enable_grad():
        for s, h in steps:
            k = []
            for j in range(6):
                Yj = Y
                for m in range(j):
                    if C.DP_BETA[j - 1][m] != 0:
                        Yj = Yj + (h * C.DP_BETA[j - 1][m]) * k[m]
                k.append(sgn * _rhs_graph(sd, i, sgn * (s + ALPHA[j] * h), Yj, cr, er))
            for j in range(6):
                if B6[j] != 0:
                    Y = Y + (h * B6[j]) * k[j]
    return Y[:, :3], Y[:, 3]


def autograd_grads(sd, i: int, x: Tensor, c: Tensor, e: Tensor, reverse: bool, steps, dtype, loss: Callable[[Tensor, Tensor], Tensor]):
    """-> dict: "out_x", "out_l", and the gradients of loss(x', dlogp) under "x", "c" and the block's state-dict keys."""
    sd = _cast(sd, dtype)
    keys = block_keys(i)
    leaf = {k: sd[k].clone().requires_grad_(True) for k in keys}
    sdl = dict(sd); sdl.update(leaf)
    xv, cv = x.to(dtype).clone().requires_grad_(True), c.to(dtype).clone().requires_grad_(True)
    ox, ol = steps_forward(sdl, i, xv, cv, e, reverse, steps, dtype)
    g = torch.autograd.grad(loss(ox, ol), [xv, cv] + [leaf[k] for k in keys])
    out = dict(zip(["x", "c"] + keys, g))
    out["out_x"], out["out_l"] = ox.detach(), ol.detach()
    return out


def steps_backward(sd, i: int, x: Tensor, c: Tensor, e: Tensor, reverse: bool, steps, dtype, gx: Tensor, gl: Tensor) -> Dict[str, Tensor]:
    """The reverse sweep for the cotangents gx [rows,3] of x' and gl [rows] of delta logp -> dict with "x", "c", the block's
    state-dict keys, and end_key(i): the CONTINUOUS end-time formula dL/dT x 2 sqrt_end_time with
    dL/dT = sum(ybar(T) . k(T)) forward, -sum(xbar_in . k(T)) reversed (k = oracle `rhs` at net time T)."""
    sd = _cast(sd, dtype)
    x, c, e, gx, gl = x.to(dtype), c.to(dtype), e.to(dtype), gx.to(dtype), gl.to(dtype)
    rows, T = x.shape[0], c.shape[0]
    R = rows // T
    cr, er = torch.repeat_interleave(c, R, dim=0), torch.repeat_interleave(e, R, dim=0)
    sgn = -1.0 if reverse else 1.0
    p = f"flow_blocks.{i}.cnf.odefunc.diffeq.layers"
    F = lambda s, Y: sgn * C.rhs(sd, i, sgn * s, Y, cr, er)
    Y = torch.cat([x, torch.zeros(rows, 1, dtype=dtype)], dim=-1)
    tape = []
    for s, h in steps:
        tape.append(Y)
        k = []
        for j in range(6):
            Yj = Y
            for m in range(j):
                Yj = Yj + (h * C.DP_BETA[j - 1][m]) * k[m]
            k.append(F(s + ALPHA[j] * h, Yj))
        for j in range(6):
            Y = Y + (h * B6[j]) * k[j]
    y_end = Y
    out = {k: torch.zeros_like(sd[k]) for k in block_keys(i)}
    cbar = torch.zeros_like(cr)
    ybar_end = torch.cat([gx, gl[:, None]], dim=-1)
    ybar = ybar_end
    for (s, h), y0 in zip(reversed(list(steps)), reversed(tape)):
        k, Ys = [], []
        for j in range(6):                                            # stage states, recomputed from y0
            Yj = y0
            for m in range(j):
                Yj = Yj + (h * C.DP_BETA[j - 1][m]) * k[m]
            Ys.append(Yj)
            k.append(F(s + ALPHA[j] * h, Yj))
        y0bar = ybar.clone()
        kbar = [h * B6[j] * ybar for j in range(6)]
        for j in reversed(range(6)):
            t = sgn * (s + ALPHA[j] * h)
            v = C.rhs_vjp(sd, i, t, Ys[j][:, :3], cr, er, sgn * kbar[j][:, :3], sgn * kbar[j][:, 3])
            Ybar = torch.cat([v["y"], torch.zeros(rows, 1, dtype=dtype)], dim=-1)
            y0bar = y0bar + Ybar
            for m in range(j):
                kbar[m] = kbar[m] + (h * C.DP_BETA[j - 1][m]) * Ybar
            tc = torch.cat([torch.full((rows, 1), t, dtype=dtype), cr], dim=-1)
            for l in range(3):
                out[f"{p}.{l}._layer.weight"] += v[f"W{l}"]
                out[f"{p}.{l}._layer.bias"] += v[f"b{l}"]
                out[f"{p}.{l}._hyper_gate.weight"] += v[f"gate_pre{l}"].t() @ tc
                out[f"{p}.{l}._hyper_gate.bias"] += v[f"gate_pre{l}"].sum(0)
                out[f"{p}.{l}._hyper_bias.weight"] += v[f"bias_pre{l}"].t() @ tc
                cbar = cbar + v[f"gate_pre{l}"] @ sd[f"{p}.{l}._hyper_gate.weight"][:, 1:] \
                    + v[f"bias_pre{l}"] @ sd[f"{p}.{l}._hyper_bias.weight"][:, 1:]
        ybar = y0bar
    out["x"] = ybar[:, :3]
    out["c"] = cbar.view(T, R, -1).sum(1)
    s_first, (s_last, h_last) = steps[0][0], steps[-1]
    if not reverse:
        dT = (ybar_end * C.rhs(sd, i, s_last + h_last, y_end, cr, er)).sum()
    else:
        dT = -(ybar * C.rhs(sd, i, -s_first, tape[0], cr, er)).sum()
    out[end_key(i)] = dT * 2.0 * sd[end_key(i)]
    return out


def end_time_autograd(sd, i: int, x: Tensor, c: Tensor, e: Tensor, reverse: bool, steps, loss) -> Tensor:
    """d loss / d sqrt_end_time by autograd in float64 with the step list SCALED by the end time (s, h) -> (s, h) T / T0:
    what the discrete scheme would give if its steps stretched with T.  Reported beside the continuous formula, not asserted."""
    sd = _cast(sd, torch.float64)
    q = sd[end_key(i)].clone().requires_grad_(True)
    T0 = float(sd[end_key(i)]) ** 2
    scaled = [((s / T0) * q * q, (h / T0) * q * q) for s, h in steps]
    ox, ol = steps_forward(sd, i, x.double().clone().requires_grad_(True), c, e, reverse, scaled, torch.float64)
    return torch.autograd.grad(loss(ox, ol), q)[0]


def rel_err(got: Tensor, ref: Tensor) -> float:
    """max|got - ref| / max(1, max|ref|)"""
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))
