"""tests/flow_train_ref.py (the float64 restatement that tests/test_gpu_flow_train.py holds the training kernels of the flow
blocks to) against the pinned oracle, and the evidence that its bar notices a subtly wrong kernel: every deliberate error,
applied to the restatement itself, breaks the bar on at least one named quantity of every chain case it applies to.  No GPU."""
import pytest
import torch

import flow_train_ref as R
from oracle import ref_cpu as O

CASES = R.chain_cases()


def _conditioning(sd, B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, N, sd[f"flow_blocks.{i}.coupling2.bias_net.layers.0.weight"].shape[1], generator=g)
            for i in range(O.NUM_BLOCKS)]


def test_restatement_equals_the_pinned_oracle_in_float32():
    """chain_f / chain_g with the injector nets evaluated (st = None) on the model's own state dict: O.flow_f, O.log_prob and
    O.flow_g to float32 rounding (the same torch ops in nearly the same order)."""
    from puflow_amd.weights import synth_state_dict
    sd = synth_state_dict(2021)
    B, N, Rr = 2, 64, 4
    g = torch.Generator().manual_seed(3)
    xyz = torch.randn(B, N, 3, generator=g) * 0.5
    cs = _conditioning(sd, B, N, 4)
    z, ssum, ld, logp = R.chain_f(sd, xyz, cs)
    z_o, logp_o, ldj_o = O.log_prob(sd, xyz, cs)
    assert float((z - z_o).abs().max()) <= 2e-6 * float(z_o.abs().max())
    assert abs(float(logp) - float(logp_o)) <= 2e-6 * abs(float(logp_o))
    assert abs(float(B * ld.sum() - ssum.sum()) - float(ldj_o.sum())) <= 2e-6 * float(ldj_o.abs().sum())
    _, _, trace = O.flow_f(sd, xyz, cs)
    p = xyz
    for i in range(O.NUM_BLOCKS):                                     # block by block, with the per-sample log-determinant
        p, ld_i, _ = R.block_f(sd, i, p, cs[i])
        s = R.lin_a1d(sd, f"flow_blocks.{i}.coupling2.scale_net", cs[i])
        assert float((p - trace[i][0]).abs().max()) <= 2e-6 * float(trace[i][0].abs().max()), i
        assert float((ld_i - s.sum(dim=(1, 2)) - trace[i][1]).abs().max()) <= 2e-6 * float(trace[i][1].abs().max()), i
    u = torch.randn(B, N * Rr, 3, generator=g)
    x = R.chain_g(sd, u, cs, Rr)
    x_o = O.flow_g(sd, u.view(B, N, Rr, 3).transpose(2, 3), cs, Rr)
    assert float((x - x_o).abs().max()) <= 2e-6 * float(x_o.abs().max())
    # a leaf `st` holding the nets' outputs is the same function
    st = torch.stack([R.lin_a1d(sd, f"flow_blocks.{k // 2}.coupling2.{'scale' if k % 2 == 0 else 'bias'}_net", cs[k // 2]).reshape(B * N, 3)
                      for k in range(2 * O.NUM_BLOCKS)])
    assert torch.equal(R.chain_g(sd, u, cs, Rr, st), x) and torch.equal(R.chain_f(sd, xyz, cs, st)[0], z)


def test_make_blocks_has_both_determinant_signs_and_float32_values():
    sd = R.make_blocks(4, [32, 64, 128, 32], [1, 2, 2, 1], 5)
    for i in range(4):
        W = sd[f"flow_blocks.{i}.permutate1.permutater.W"]
        assert (float(torch.det(W)) < 0) == (i % 2 == 1)
        assert R._td(sd, i, torch.empty(1, 1, [32, 64, 128, 32][i])) == [1, 2, 2, 1][i]
    for k, v in sd.items():
        if v.dtype == torch.float64:
            assert torch.equal(v.float().double(), v), k
    sd32 = R.make_blocks(4, [32, 64, 128, 32], [1, 2, 2, 1], 5, torch.float32)
    assert all(torch.equal(sd32[k].double(), sd[k].double()) for k in sd)


def test_every_deliberate_error_applies_somewhere():
    for bug in R.BUGS:
        assert sum(R.bug_applies(bug, c) for c in CASES) >= 3, bug


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_the_bar_catches_every_deliberate_error(case):
    """The bar of the GPU test, 16 max|ref32 - ref64| + 2^-21 max|ref64| per tensor, applied to the float64 restatement with one
    deliberate error: every error that changes the case's function at all must leave at least one quantity outside it."""
    inputs, upstream, ref = R.chain_problem(case)
    assert R.min_preactivation(lambda: ref(inputs)) >= R.MIN_PREACT           # the seed keeps every tier off the kinks
    r64 = R.grads(ref, inputs, upstream)
    r32 = R.grads(ref, inputs, upstream, dtype=torch.float32)
    assert not R.failures(R.compare(r64, r64, r32))
    # float32 against float64 stays at rounding level: the bar is about a thousand times tighter than a per-cent bar
    for k, v in r64.items():
        assert R.bar_of(v, r32[k]) <= 2e-4 * float(v.abs().max()) + 1e-30, (k, R.bar_of(v, r32[k]), float(v.abs().max()))
    for bug in R.BUGS:
        if not R.bug_applies(bug, case):
            continue
        wrong = R.grads(lambda lv: ref(lv, (bug,)), inputs, upstream)
        broken = R.failures(R.compare(wrong, r64, r32))
        assert broken, f"{bug} stays inside the bar on every quantity of {case['id']}"
