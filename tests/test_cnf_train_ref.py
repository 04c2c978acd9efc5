"""tests/cnf_train_ref.py (the CPU reference of the continuous model's train-mode forward on fixed step lists) pinned in float64:
with only ONE integration's step list non-empty and the conditioning features fed as leaves the whole-model helper IS that
block followed by the log-likelihood and the interpolation, so its gradients must be cnf_grad_ref.autograd_grads' through the
same tail; plus the identities an empty model gives, the whole-model wiring and the end-time formula's two directions."""
import math

import pytest
import torch

import cnf_grad_ref as G
import cnf_train_ref as TR
from oracle import ref_cpu as O
from puflow_amd.weights import synth_cnf_state_dict

B, N, R = 2, 12, 2
CDS = [32, 64, 128, 128, 128, 128]


def _inputs(seed):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.randn(B, N, 3, generator=g, dtype=torch.float64) * 0.6
    cs = [torch.randn(B, N, cd, generator=g, dtype=torch.float64) * 0.7 for cd in CDS]
    w = torch.randn(B * N * 8, 32, generator=g, dtype=torch.float64)
    noise = [torch.randn(B, N, 3, generator=g, dtype=torch.float64) for _ in range(6)]
    gx = torch.randn(B, N * R, 3, generator=g, dtype=torch.float64)
    _, idx8 = O.knn_canonical(xyz.float(), xyz.float(), 8)
    return xyz, cs, w, noise, gx, idx8


def _loss(gx):
    return lambda x, logp: 0.3 * logp + (x * gx).sum()


@pytest.mark.parametrize("block", [0, 2, 5])
def test_one_forward_block_reduces_to_the_block_reference(block):
    sd = synth_cnf_state_dict(7)
    xyz, cs, w, noise, gx, idx8 = _inputs(20 + block)
    steps = [(0.0, 0.05), (0.05, 0.11), (0.16, 0.07)]
    lists = [[] for _ in range(12)]
    lists[block] = steps
    r = TR.run(sd, xyz, R, lists, noise, torch.float64, cs=cs, w=w, idx8=idx8, xyz_leaf=True)
    got = TR.gradients(r, _loss(gx))

    def tail(ox, ol):                                   # what the helper does behind the block, written out
        z = ox.view(B, N, 3)
        logp = -torch.mean(torch.sum(-0.5 * (z ** 2 + math.log(2 * math.pi)), dim=(1, 2)) - ol.view(B, N).sum(1))
        return _loss(gx)(TR.interp_latent(z, w, idx8, R), logp)

    ref = G.autograd_grads(sd, block, xyz.reshape(B * N, 3), cs[block].reshape(B * N, -1), noise[block].reshape(B * N, 3), False,
                           steps, torch.float64, tail)
    pairs = [("xyz", "x"), (f"cs.{block}", "c")] + [(k, k) for k in G.block_keys(block)]
    for mine, theirs in pairs:
        a, b = got[mine].reshape(ref[theirs].shape), ref[theirs]
        assert float(b.abs().max()) > 0, theirs
        assert float((a - b).abs().max()) <= 1e-9 * max(1.0, float(b.abs().max())), (mine, float((a - b).abs().max()))
    for i in range(6):                                   # nothing reaches the blocks that did not run
        if i != block:
            assert float(got[f"cs.{i}"].abs().max()) == 0.0
            assert all(float(got[k].abs().max()) == 0.0 for k in G.block_keys(i))
    # the end time: the forward formula of cnf_grad_ref.steps_backward with the cotangents this tail sends back
    x1 = ref["out_x"].clone().requires_grad_(True)
    l1 = ref["out_l"].clone().requires_grad_(True)
    gx1, gl1 = torch.autograd.grad(tail(x1, l1), [x1, l1])
    want = G.steps_backward(sd, block, xyz.reshape(B * N, 3), cs[block].reshape(B * N, -1), noise[block].reshape(B * N, 3), False,
                            steps, torch.float64, gx1, gl1)[G.end_key(block)]
    assert abs(float(got[G.end_key(block)] - want)) <= 1e-9 * max(1.0, abs(float(want)))


def test_one_reverse_block_gets_the_reversed_end_time_formula():
    block = 4
    sd = synth_cnf_state_dict(7)
    xyz, cs, w, noise, gx, idx8 = _inputs(31)
    T_end = float(sd[G.end_key(block)]) ** 2
    steps = [(-T_end, 0.04), (-T_end + 0.04, 0.09)]
    lists = [[] for _ in range(12)]
    lists[6 + (5 - block)] = steps                      # g runs the blocks 5 .. 0
    r = TR.run(sd, xyz, R, lists, noise, torch.float64, cs=cs, w=w, idx8=idx8)
    got = TR.gradients(r, _loss(gx))
    u = TR.interp_latent(xyz, w, idx8, R).reshape(B * N * R, 3)     # f is the identity: z = xyz
    c, e = cs[block].reshape(B * N, -1), noise[block].reshape(B * N, 3)
    want = G.steps_backward(sd, block, u, c, e, True, steps, torch.float64, gx.reshape(-1, 3), torch.zeros(B * N * R, dtype=torch.float64))
    for k in G.block_keys(block) + [G.end_key(block)]:
        assert float(want[k].abs().max()) > 0, k
        assert float((got[k] - want[k]).abs().max()) <= 1e-9 * max(1.0, float(want[k].abs().max())), k
    assert float((got[f"cs.{block}"].reshape(B * N, -1) - want["c"]).abs().max()) <= 1e-9 * max(1.0, float(want["c"].abs().max()))


def test_empty_lists_are_the_identity_and_both_directions_add():
    sd = synth_cnf_state_dict(7)
    xyz, cs, w, noise, gx, idx8 = _inputs(5)
    r = TR.run(sd, xyz, R, [[] for _ in range(12)], noise, torch.float64, cs=cs, w=w, idx8=idx8)
    assert torch.equal(r.x, TR.interp_latent(xyz, w, idx8, R))
    assert float(r.logp) == pytest.approx(float(-torch.mean(torch.sum(-0.5 * (xyz ** 2 + math.log(2 * math.pi)), dim=(1, 2)))), rel=1e-12)
    # block 3 in f AND in g: every gradient is the sum of the two one-direction runs' (the loss is linear in x; logp off)
    T_end = float(sd[G.end_key(3)]) ** 2
    f_steps, g_steps = [(0.0, 0.02)], [(-T_end, 0.03)]
    lin = lambda x, logp: (x * gx).sum()
    both = [[] for _ in range(12)]; both[3] = f_steps; both[8] = g_steps
    rb = TR.run(sd, xyz, R, both, noise, torch.float64, cs=cs, w=w, idx8=idx8)
    gb = TR.gradients(rb, lin)
    # the same graph with one direction's block parameters detached is not expressible through `run`; instead: the context's
    # gradient must exceed either direction's alone and the record keys must be non-zero from both
    only_g = [[] for _ in range(12)]; only_g[8] = g_steps
    gg = TR.gradients(TR.run(sd, xyz, R, only_g, noise, torch.float64, cs=cs, w=w, idx8=idx8), lin)
    k = G.block_keys(3)[0]
    assert float((gb[k] - gg[k]).abs().max()) > 0 and float((gb["cs.3"] - gg["cs.3"]).abs().max()) > 0


def test_whole_model_runs_the_train_mode_extractor_and_interpolation():
    """Nothing fed: the features and logits come from the train-mode units; every parameter group gets a gradient."""
    sd = synth_cnf_state_dict(7)
    g = torch.Generator().manual_seed(2)
    Nw = 20                                                             # >= 17 for the 16-neighbour lists
    xyz = torch.randn(1, Nw, 3, generator=g) * 0.6
    noise = [torch.randn(1, Nw, 3, generator=g) for _ in range(6)]
    _, idx16 = O.knn_canonical(xyz, xyz, 16)
    lists = [[] for _ in range(12)]
    lists[1] = [(0.0, 0.05)]
    lists[10] = [(-float(sd[G.end_key(1)]) ** 2, 0.05)]
    r = TR.run(sd, xyz, 2, lists, noise, torch.float64, idx16=idx16)
    assert r.x.shape == (1, 2 * Nw, 3) and r.x.dtype == torch.float64
    got = TR.gradients(r, lambda x, logp: logp + x.sum())
    for k in ("feat_convs.0.convs.0.0.weight", "feat_convs.1.conv_out.weight", "merge_convs.1.conv2.weight",
              "interp.weight_unit.mlp.6.weight", "interp.knn_context.feat_conv.conv_out.weight", G.block_keys(1)[0], G.end_key(1)):
        assert float(got[k].abs().max()) > 0, k
    assert float(got["merge_convs.4.conv2.weight"].abs().max()) == 0.0   # block 4 did not run: its context is unused
