"""The reverse sweep through recorded Dormand-Prince steps (tests/cnf_grad_ref.py::steps_backward) against autograd
through the same steps, in float64 on the CPU.  This pins the sweep that puflow_amd/cnf.py's backward restates on the GPU."""
import pytest
import torch

import cnf_grad_ref as G
from puflow_amd.weights import synth_cnf_state_dict


def _case(block, R, reverse, seed):
    sd = synth_cnf_state_dict(7)
    g = torch.Generator().manual_seed(seed)
    T = 40 // R
    cd = sd[f"flow_blocks.{block}.cnf.odefunc.diffeq.layers.0._hyper_gate.weight"].shape[1] - 1
    x = torch.randn(40, 3, generator=g, dtype=torch.float64) * 0.8
    c = torch.randn(T, cd, generator=g, dtype=torch.float64) * 0.7
    e = torch.randn(T, 3, generator=g, dtype=torch.float64)
    gx = torch.randn(40, 3, generator=g, dtype=torch.float64)
    gl = torch.randn(40, generator=g, dtype=torch.float64)
    s0 = -float(sd[G.end_key(block)]) ** 2 if reverse else 0.0
    steps = [(s0, 0.05), (s0 + 0.05, 0.11), (s0 + 0.16, 0.07)]                     # three steps of unequal size
    return sd, x, c, e, gx, gl, steps


@pytest.mark.parametrize("block", [0, 5])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("R", [1, 4])
def test_reverse_sweep_matches_autograd_through_the_steps(block, reverse, R):
    sd, x, c, e, gx, gl, steps = _case(block, R, reverse, 100 + 10 * block + R)
    loss = lambda ox, ol: (ox * gx).sum() + (ol * gl).sum()                        # cotangents on x' AND delta logp
    ref = G.autograd_grads(sd, block, x, c, e, reverse, steps, torch.float64, loss)
    got = G.steps_backward(sd, block, x, c, e, reverse, steps, torch.float64, gx, gl)
    for k in ["x", "c"] + G.block_keys(block):
        assert float(ref[k].abs().max()) > 0, k
        err = float((got[k] - ref[k]).abs().max())
        assert err <= 1e-9 * max(1.0, float(ref[k].abs().max())), (k, err)
    # column 3 never enters F: the cotangent of delta logp passes through the steps unchanged - checked through x alone
    only_l = G.steps_backward(sd, block, x, c, e, reverse, steps, torch.float64, torch.zeros_like(gx), gl)
    ref_l = G.autograd_grads(sd, block, x, c, e, reverse, steps, torch.float64, lambda ox, ol: (ol * gl).sum())
    assert float((only_l["x"] - ref_l["x"]).abs().max()) <= 1e-9 * max(1.0, float(ref_l["x"].abs().max()))
    # the continuous end-time formula beside the discrete scheme's own derivative with the steps scaled by T (reported only)
    disc = float(G.end_time_autograd(sd, block, x, c, e, reverse, steps, loss))
    print(f"block {block} R {R} reverse {reverse}: d/d sqrt_end_time continuous {float(got[G.end_key(block)]):+.6e} "
          f"scaled steps {disc:+.6e}")


def test_forward_in_float32_is_close_to_float64():
    """The yardstick of the GPU tests is this helper in float32: it has to be a sane one."""
    sd, x, c, e, gx, gl, steps = _case(5, 4, True, 3)
    a = G.steps_forward(sd, 5, x, c, e, True, steps, torch.float32)
    b = G.steps_forward(sd, 5, x, c, e, True, steps, torch.float64)
    assert a[0].dtype == torch.float32 and G.rel_err(a[0], b[0]) < 1e-5 and G.rel_err(a[1], b[1]) < 1e-5
