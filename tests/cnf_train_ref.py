"""Reference of the continuous model's TRAIN-mode forward on FIXED Dormand-Prince step lists, in torch on the CPU (float64 by
default).  TEST INFRASTRUCTURE ONLY (a helper module like tests/cnf_grad_ref.py, which it chains; tests/test_cnf_train_ref.py pins
it, tests/test_gpu_cnf_train.py holds `cnf.PointInterpFlow` in train() mode to it).

  features        the train-mode feature extractor (oracle.ref_cpu.edgeconv_unit_train, feat_merge) -> cs
  interp_logits   the train-mode interpolation weights before the softmax, as oracle.ref_cpu.forward_train computes them, in
                  the layout of the training step: [B N 8, 32], row (b N + n) 8 + k
  interp_latent   u [B, N R, 3] from z, the logits and the 8-neighbour lists
  run             f over six blocks, log-likelihood, interpolation, g over six blocks, each block integrated by
                  cnf_grad_ref.steps_forward on its step list (an empty list is the identity); `step_lists`: twelve lists in
                  the order the forward runs them - f's blocks 0 .. 5, then g's blocks 5 .. 0
  gradients       autograd through all of it; sqrt_end_time by DESIGN 9a's continuous formula, with the cotangents taken from
                  the graph (retain_grad) at each integration's ends, summed over the block's two directions"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

import cnf_grad_ref as G
from oracle import cnf_ref as C
from oracle import ref_cpu as O

Tensor = torch.Tensor
NB = 6
_NOT_PARAMS = ("running_mean", "running_var", "num_batches_tracked", "_num_evals")


def param_keys(sd) -> List[str]:
    return [k for k, v in sd.items() if v.is_floating_point() and not k.endswith(_NOT_PARAMS)]


def leaves(sd, dtype=torch.float64) -> Dict[str, Tensor]:
    """sd in `dtype` with every parameter a fresh leaf that requires grad."""
    out = {k: (v.detach().to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    for k in param_keys(sd):
        out[k] = out[k].clone().requires_grad_(True)
    return out


def features(sd, xyz: Tensor, idx16: Tensor) -> List[Tensor]:
    ts = O.TrainState()
    cs, h = [], xyz
    for i in range(NB):
        h = O.edgeconv_unit_train(sd, f"feat_convs.{i}", h, idx16, ts)
        cs.append(O.feat_merge(sd, i, h))
    return cs


def interp_logits(sd, xyz: Tensor, idx8: Tensor) -> Tensor:
    B, N, _ = xyz.shape
    ts = O.TrainState()
    nb = O.knn_gather(xyz, idx8)
    xi = xyz.unsqueeze(2).expand_as(nb)
    vec = xi - nb
    dist = torch.sqrt(torch.sum(vec ** 2, dim=-1, keepdim=True))
    d = torch.cat([xi, nb, vec, dist], dim=-1).permute(0, 3, 1, 2)
    pd = "interp.knn_context.distance_encoder.mlp"
    for a in (0, 3):
        d = F.conv2d(d, sd[f"{pd}.{a}.weight"], sd[f"{pd}.{a}.bias"])
        d = F.leaky_relu(O._bn_train(sd, f"{pd}.{a + 1}", d, ts), 0.01)
    d = F.conv2d(d, sd[pd + ".6.weight"], sd[pd + ".6.bias"])
    feat = O.edgeconv_unit_train(sd, "interp.knn_context.feat_conv", xyz, idx8, ts, pooling=False)
    w = torch.cat([d, feat], dim=1)
    pw = "interp.weight_unit.mlp"
    for a in (0, 3):
        w = F.conv2d(w, sd[f"{pw}.{a}.weight"], sd[f"{pw}.{a}.bias"])
        w = F.leaky_relu(O._bn_train(sd, f"{pw}.{a + 1}", w, ts), 0.01)
    w = F.conv2d(w, sd[pw + ".6.weight"], sd[pw + ".6.bias"])          # [B,32,N,k]
    return w.permute(0, 2, 3, 1).reshape(B * N * idx8.shape[-1], -1)


def interp_latent(z: Tensor, w: Tensor, idx8: Tensor, R: int) -> Tensor:
    """z [B,N,3], w [B N 8, >= R] logits -> u [B, N R, 3], row n R + r (interpflow.py:153-186)."""
    B, N, _ = z.shape
    K = idx8.shape[-1]
    a = F.softmax(w.view(B, N, K, -1)[..., :R], dim=2)                  # over the neighbours
    return torch.einsum("bnkc,bnkr->bnrc", O.knn_gather(z, idx8), a).reshape(B, N * R, 3)


class Run:
    """One forward: outputs, the leaves it was differentiated from, and both ends of every integration."""

    def __init__(self):
        self.x = self.logp = None
        self.sd: Dict[str, Tensor] = {}
        self.inputs: Dict[str, Tensor] = {}                 # "xyz", "w", "cs.<i>" where they were fed as leaves
        self.ends: list = []                                # (block, reverse, steps, y_in [rows,3], x_out, dl_out, c, e)


def run(sd, xyz: Tensor, R: int, step_lists: Sequence[Sequence], noise: Sequence[Tensor], dtype=torch.float64,
        idx16: Optional[Tensor] = None, cs: Optional[List[Tensor]] = None, w: Optional[Tensor] = None,
        idx8: Optional[Tensor] = None, xyz_leaf: bool = False) -> Run:
    """sd: a state dict (made leaves here).  cs / w given: fed as leaves in place of the feature extractor / the interpolation
    branch (then idx16 is not needed; idx8 is).  xyz_leaf: xyz requires grad where it enters flow f (the extractor and the
    interpolation branch always see it detached, as in the training step)."""
    assert len(step_lists) == 2 * NB and len(noise) == NB
    r = Run()
    r.sd = sdl = leaves(sd, dtype)
    B, N, _ = xyz.shape
    T = B * N
    xyz = xyz.detach().to(dtype)
    if idx8 is None:
        idx8 = idx16[..., :8].contiguous()
    idx8 = idx8.long()
    if cs is None:
        cs = features(sdl, xyz, idx16.long())
    else:
        cs = [c.detach().to(dtype).clone().requires_grad_(True) for c in cs]
        r.inputs.update({f"cs.{i}": c for i, c in enumerate(cs)})
    if w is None:
        w = interp_logits(sdl, xyz, idx8)
    else:
        w = r.inputs["w"] = w.detach().to(dtype).clone().requires_grad_(True)
    p = xyz.reshape(T, 3)
    if xyz_leaf:
        p = r.inputs["xyz"] = p.clone().requires_grad_(True)
    es = [n.detach().to(dtype).reshape(T, 3) for n in noise]
    cf = [c.reshape(T, -1) for c in cs]

    def block(i, y_in, reverse, steps):
        if y_in.requires_grad and not y_in.is_leaf:
            y_in.retain_grad()
        ox, ol = G.steps_forward(sdl, i, y_in, cf[i], es[i], reverse, steps, dtype)
        if ox.requires_grad and not ox.is_leaf:
            ox.retain_grad()
        if ol.requires_grad:
            ol.retain_grad()
        r.ends.append((i, reverse, list(steps), y_in, ox, ol, cf[i], es[i]))
        return ox, ol

    ldj = torch.zeros(B, dtype=dtype)
    for i in range(NB):
        p, dl = block(i, p, False, step_lists[i])
        ldj = ldj + dl.view(B, N).sum(1)
    z = p.view(B, N, 3)
    r.logp = -torch.mean(torch.sum(-0.5 * (z ** 2 + math.log(2 * math.pi)), dim=(1, 2)) - ldj)       # oracle/cnf_ref.py::forward
    u = interp_latent(z, w, idx8, R).reshape(T * R, 3)
    for j, i in enumerate(reversed(range(NB))):
        u, _ = block(i, u, True, step_lists[NB + j])
    r.x = u.view(B, N * R, 3)
    return r


def gradients(r: Run, loss: Callable[[Tensor, Tensor], Tensor]) -> Dict[str, Tensor]:
    """d loss(x, logp) / d every parameter and fed input.  sqrt_end_time (which the fixed step lists do not depend on) by the
    continuous formula of DESIGN 9a per integration: dL/dT = sum(ybar(T) . k(T)) forward, -sum(ybar_in . k(T)) reversed, with k
    the right-hand side at net time T and the cotangents read off the graph; x 2 sqrt_end_time, summed over f and g."""
    loss(r.x, r.logp).backward()
    out = {}
    for k in param_keys(r.sd):
        g = r.sd[k].grad
        out[k] = torch.zeros_like(r.sd[k]) if g is None else g.clone()
    for k, v in r.inputs.items():
        out[k] = torch.zeros_like(v) if v.grad is None else v.grad.clone()
    sd = {k: v.detach() for k, v in r.sd.items()}
    z = lambda t, like: torch.zeros_like(like) if t is None else t
    for i, reverse, steps, y_in, ox, ol, c, e in r.ends:
        if not steps:
            continue
        Rr = y_in.shape[0] // c.shape[0]
        cr, er = torch.repeat_interleave(c.detach(), Rr, dim=0), torch.repeat_interleave(e, Rr, dim=0)
        gl = z(ol.grad, ol.detach())                            # column 3 passes through a block: the same at both ends
        if not reverse:
            y_end = torch.cat([ox.detach(), ol.detach()[:, None]], dim=-1)
            ybar = torch.cat([z(ox.grad, ox.detach()), gl[:, None]], dim=-1)
            dT = (ybar * C.rhs(sd, i, steps[-1][0] + steps[-1][1], y_end, cr, er)).sum()
        else:
            y0 = torch.cat([y_in.detach(), torch.zeros_like(gl)[:, None]], dim=-1)
            ybar = torch.cat([z(y_in.grad, y_in.detach()), gl[:, None]], dim=-1)
            dT = -(ybar * C.rhs(sd, i, -steps[0][0], y0, cr, er)).sum()
        out[G.end_key(i)] = out[G.end_key(i)] + dT * 2.0 * sd[G.end_key(i)]
    return out
