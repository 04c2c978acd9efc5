"""The embedded error estimate of Dormand-Prince steps on a GIVEN step list, on the CPU.  TEST INFRASTRUCTURE ONLY (a helper module
like tests/cnf_grad_ref.py): the error formula of oracle/cnf_ref.py::dopri5's loop - err = h sum_j (b_j - b*_j) k_j over the seven
stage derivatives, scaled by atol + rtol max(|y0|, |y1|) - without the controller around it, built on oracle.cnf_ref.rhs.

  step_error_ratios   per step sqrt(sum_i (err_i / tol_i)^2 / n_tot), n_tot = rows 4 + the context's elements x R (the context is
                      a state of the reference's ODE: it enters the norm's element count with zero error), and the final state.
x [rows,3] with rows = T R (the R rows of a point adjacent), c [T,cd], e [T,3]; steps [(s, h), ..] in solver time (s = -t and
f' = -f when reversed, as in oracle/cnf_ref.py::cnf_block)."""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import torch

from oracle import cnf_ref as C

Tensor = torch.Tensor


def step_error_ratios(sd, i: int, x: Tensor, c: Tensor, e: Tensor, reverse: bool, steps: Sequence[Tuple[float, float]],
                      dtype=torch.float64, rtol: float = C.RTOL, atol: float = C.ATOL) -> Tuple[List[float], Tensor]:
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    x, c, e = x.to(dtype), c.to(dtype), e.to(dtype)
    rows, T = x.shape[0], c.shape[0]
    R = rows // T
    cr, er = torch.repeat_interleave(c, R, dim=0), torch.repeat_interleave(e, R, dim=0)
    sgn = -1.0 if reverse else 1.0
    F = lambda s, Y: sgn * C.rhs(sd, i, sgn * s, Y, cr, er)
    n_tot = float(rows * 4 + c.numel() * R)
    Y = torch.cat([x, torch.zeros(rows, 1, dtype=dtype)], dim=-1)
    ratios = []
    k1 = F(steps[0][0], Y)
    for s, h in steps:
        k = [k1]
        for j in range(6):
            Yj = Y
            for m in range(j + 1):
                Yj = Yj + (h * C.DP_BETA[j][m]) * k[m]
            k.append(F(s + C.DP_ALPHA[j] * h, Yj))
        Y1 = Yj                                                        # the sixth stage's state IS the step's solution
        err = h * sum(cj * kj for cj, kj in zip(C.DP_C_ERR, k))
        tol = atol + rtol * torch.maximum(Y.abs(), Y1.abs())
        ratios.append(math.sqrt(float(((err / tol) ** 2).sum().double()) / n_tot))
        Y, k1 = Y1, k[6]                                               # FSAL
    return ratios, Y
