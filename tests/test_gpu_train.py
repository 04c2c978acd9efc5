"""Training path on the GPU: every HIP training op against torch-CPU autograd, then a whole training step
(train-mode forward, loss, all parameter gradients, BN running stats, ActNorm init) against the golden vectors
captured from the reference's own module (tools/make_golden_train.py) and against the train-mode oracle."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as O
from puflow_amd.weights import synth_patches, synth_state_dict

DEV = "cuda:0"


def _close(a, b, rtol=2e-4, atol=1e-6):
    np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), rtol=rtol, atol=atol)


@pytest.mark.parametrize("R,Cin,Cout,bias", [(1000, 9, 8, True), (4096, 96, 16, True), (333, 130, 64, False),
                                             (70000, 40, 32, True), (64, 3, 3, False), (5000, 512, 128, True),
                                             (3000, 256, 32, True), (2048, 64, 64, True), (999, 128, 3, True),
                                             (4100, 33, 8, True), (131072, 10, 64, True)])
def test_linear_fwd_bwd(R, Cin, Cout, bias):
    from puflow_amd.train_ops import linear
    g = torch.Generator().manual_seed(R)
    x = torch.randn(R, Cin, generator=g, requires_grad=True)
    W = torch.randn(Cout, Cin, generator=g, requires_grad=True)
    b = torch.randn(Cout, generator=g, requires_grad=True) if bias else None
    gy = torch.randn(R, Cout, generator=g)
    y = F.linear(x, W, b); y.backward(gy)
    xd, Wd = x.detach().to(DEV).requires_grad_(True), W.detach().to(DEV).requires_grad_(True)
    bd = b.detach().to(DEV).requires_grad_(True) if bias else None
    yd = linear(xd, Wd, bd); yd.backward(gy.to(DEV))
    _close(yd, y, atol=2e-6 * float(y.abs().max()) + 1e-6); _close(xd.grad, x.grad, atol=2e-6 * float(x.grad.abs().max()) + 1e-6)
    _close(Wd.grad, W.grad, rtol=1e-3, atol=1e-3 * float(W.grad.abs().max()))       # K = R long reductions
    if bias:
        _close(bd.grad, b.grad, rtol=1e-3, atol=1e-3 * float(b.grad.abs().max()))


@pytest.mark.parametrize("R,C,slope", [(4096, 8, 0.05), (131072, 32, 0.05), (1000, 128, 0.01), (50000, 64, 0.01)])
def test_bn_lrelu_fwd_bwd(R, C, slope):
    from puflow_amd.train_ops import BnLreluFn
    g = torch.Generator().manual_seed(C)
    x = (torch.randn(R, C, generator=g) * 2 + 0.5).requires_grad_(True)
    ga = (torch.rand(C, generator=g) + 0.5).requires_grad_(True)
    be = torch.randn(C, generator=g).requires_grad_(True)
    rm, rv = torch.zeros(C), torch.ones(C)
    y = F.leaky_relu(F.batch_norm(x, rm, rv, ga, be, training=True, momentum=0.1, eps=1e-5), slope)
    gy = torch.randn(R, C, generator=g)
    y.backward(gy)
    xd = x.detach().to(DEV).requires_grad_(True)
    gd, bd = ga.detach().to(DEV).requires_grad_(True), be.detach().to(DEV).requires_grad_(True)
    rmd, rvd = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    yd = BnLreluFn.apply(xd, gd, bd, rmd, rvd, slope, 1e-5, 0.1)
    yd.backward(gy.to(DEV))
    _close(yd, y, atol=1e-5); _close(rmd, rm, atol=1e-6); _close(rvd, rv, rtol=1e-5)
    # LeakyReLU' is discontinuous at 0: an element whose pre-activation is within rounding of 0 may take the other branch
    bad = ~torch.isclose(xd.grad.cpu(), x.grad, rtol=1e-3, atol=1e-5)
    assert int(bad.sum()) <= max(1, R * C // 1_000_000)
    _close(gd.grad, ga.grad, rtol=1e-3, atol=1e-3 * float(ga.grad.abs().max()))
    _close(bd.grad, be.grad, rtol=1e-3, atol=1e-3 * float(be.grad.abs().max()))


def test_edge_pool_gather_softmax_ops():
    from puflow_amd import ops
    from puflow_amd.train_ops import ActFn, EdgeFeatureFn, GatherRowsFn, MaxPoolKFn, RepeatRowsFn, SoftmaxWsumFn
    B, N, C, K = 3, 100, 20, 16
    g = torch.Generator().manual_seed(1)
    pts = torch.rand(B, N, 3, generator=g)
    _, idx = O.knn_canonical(pts, pts, K)
    x = torch.randn(B, N, C, generator=g, requires_grad=True)
    nb = O.knn_gather(x, idx); xi = x.unsqueeze(2).expand_as(nb)
    e = torch.cat([xi, nb, nb - xi], -1).reshape(B * N * K, 3 * C)
    pooled = e.view(B * N, K, 3 * C).max(1)[0]
    ge = torch.randn(B * N, 3 * C, generator=g)
    pooled.backward(ge)
    xd = x.detach().to(DEV).requires_grad_(True)
    idx32 = idx.to(torch.int32).to(DEV)
    ed = EdgeFeatureFn.apply(xd, idx32)
    pd = MaxPoolKFn.apply(ed, K)
    pd.backward(ge.to(DEV))
    _close(ed, e); _close(pd, pooled); _close(xd.grad, x.grad, rtol=1e-4, atol=1e-5)
    # gather rows + softmax weighted sum
    z = torch.randn(B, N, 3, generator=g, requires_grad=True)
    w = torch.randn(B * N, 8, 32, generator=g, requires_grad=True)
    idx8 = idx[..., :8].contiguous()
    zj = O.knn_gather(z, idx8).reshape(B * N, 8, 3)
    a = F.softmax(w[:, :, :4], dim=1)
    fz = torch.einsum("tkc,tkr->tcr", zj, a)
    gf = torch.randn(B * N, 3, 4, generator=g)
    fz.backward(gf)
    zd, wd = z.detach().to(DEV).requires_grad_(True), w.detach().to(DEV).requires_grad_(True)
    fzd = SoftmaxWsumFn.apply(wd, GatherRowsFn.apply(zd, idx8.to(torch.int32).to(DEV)).view(B * N, 8, 3), 4)
    fzd.backward(gf.to(DEV))
    _close(fzd, fz, atol=1e-6); _close(zd.grad, z.grad, rtol=1e-4, atol=1e-6); _close(wd.grad, w.grad, rtol=1e-4, atol=1e-6)
    # repeat rows + activation
    c = torch.randn(B, N, C, generator=g, requires_grad=True)
    r = F.relu(torch.repeat_interleave(c, 4, dim=1)); gr = torch.randn(B, N * 4, C, generator=g); r.backward(gr)
    cd = c.detach().to(DEV).requires_grad_(True)
    rd = ActFn.apply(RepeatRowsFn.apply(cd, 4), 0.0); rd.backward(gr.to(DEV))
    _close(rd, r); _close(cd.grad, c.grad, rtol=1e-5, atol=1e-6)


def _chamfer_cpu(x, y):
    d = ((x[:, :, None] - y[:, None]) ** 2).sum(-1)
    return (d.min(2)[0].mean(1) + d.min(1)[0].mean(1)).mean()


def _assert_grads_elementwise(params, ref_grad, tol=1e-2):
    """EVERY gradient tensor element by element against the oracle's (a norm comparison passes a permuted channel
    or a transposed dW): max |g - g_ref| <= tol x max |g_ref| + a floor of 1e-5 x the largest gradient norm of the network (51
    tensors - conv biases in front of BatchNorm - have a mathematically zero gradient: both sides hold rounding residue).
    tol = 1 %: at 5e-3 ONE element fails at B = 4 - the first unit's first BatchNorm shift gradient, an 8-element tensor, 0.84 %
    off in one element while its norm agrees to 0.2 % (a max-pool route that two near-equal edges share); a permutation or a
    transposition is off by O(1)."""
    floor = 1e-5 * max(float(v.norm()) for v in ref_grad.values())
    worst = (0.0, None)
    for k, ref in ref_grad.items():
        got = params[k].grad
        got = torch.zeros_like(ref) if got is None else got.detach().cpu()
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        err, bound = float((got - ref).abs().max()), tol * float(ref.abs().max()) + floor
        worst = max(worst, (err / bound, k))
        assert err <= bound, (k, err, bound, float(ref.abs().max()))
    return worst


def test_training_step_matches_reference_golden(golden_dir):
    _golden_step(golden_dir)


def _golden_step(golden_dir, deterministic=False):
    """The step of tests/golden/train_step.npz against the golden vectors and the oracle; deterministic: net.deterministic
    (tests/test_gpu_deterministic.py), every assertion and bar the same."""
    from puflow_amd import ops
    from puflow_amd.interpflow import PointInterpFlow
    g = np.load(os.path.join(golden_dir, "train_step.npz"))
    B, N, R = int(g["meta_B"]), int(g["meta_N"]), 4
    sd = synth_state_dict(int(g["meta_wseed"]))
    dense = synth_patches(B, N * R, seed=int(g["meta_dseed"]))
    sparse = dense[:, ::R].contiguous()
    net = PointInterpFlow(3)
    net.load_state_dict(sd)
    net = net.to(DEV).train()                            # ActNorm not initialised: first-batch init, like the reference
    net.deterministic = deterministic
    x, logp = net(sparse.to(DEV), R)
    cd, _ = ops.chamfer_distance(x, dense.to(DEV))
    loss = logp * 1e-4 + cd * 1e-1
    loss.backward()
    np.testing.assert_allclose(x.detach().cpu().numpy(), g["x"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(float(logp), float(g["logp"]), rtol=1e-5)
    np.testing.assert_allclose(float(cd), float(g["cd"]), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(float(loss), float(g["loss"]), rtol=1e-5)
    norms = dict(zip(g["grad_names"].tolist(), g["grad_norms"].tolist()))
    params = dict(net.named_parameters())
    floor = 1e-5 * max(norms.values())
    for k, ref in norms.items():
        got = 0.0 if params[k].grad is None else float(params[k].grad.norm())
        assert abs(got - ref) <= 2e-3 * ref + floor, (k, got, ref)
    # every parameter gradient element-wise against the oracle (pinned to this golden on CPU: tests/test_oracle_train.py)
    sdr = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.clone()) for k, v in sd.items()}
    xr, lr, _ = O.forward_train(sdr, sparse, R, actnorm_init=True)
    (lr * 1e-4 + _chamfer_cpu(xr, dense) * 1e-1).backward()
    _assert_grads_elementwise(params, {k: v.grad for k, v in sdr.items() if v.requires_grad and v.grad is not None})
    sd2 = net.state_dict()
    for key in g.files:
        if key.startswith("grad::"):
            ref = g[key]
            np.testing.assert_allclose(params[key[6:]].grad.cpu().numpy(), ref, rtol=5e-3, atol=2e-3 * np.abs(ref).max() + floor)
        if key.startswith("state::"):
            np.testing.assert_allclose(sd2[key[7:]].cpu().numpy(), g[key], rtol=1e-4, atol=1e-6)


def test_trainer_module_step_and_eval_roundtrip():
    """TrainerModule.train_step with the reference's loss mix (EMD via HIP), then eval() uses the fused path."""
    from puflow_amd.trainer import TrainerModule, default_cfg
    torch.manual_seed(0)
    tm = TrainerModule(default_cfg(learning_rate=1e-3), loss_mix="pugan")
    tm.network.load_state_dict(synth_state_dict(21))
    tm = tm.to(DEV)
    opt = tm.configure_optimizers()["optimizer"]
    dense = synth_patches(4, 1024, seed=5)
    dense01 = ((dense + 1) / 2).to(DEV)                  # EMD expects coordinates in [0,1]
    sparse = dense01[:, ::4].contiguous()
    radius = torch.ones(4, device=DEV)
    w0 = tm.network.feat_convs[3].conv_out.weight.detach().clone()
    l1 = tm.train_step((sparse, dense01, radius), opt)
    l2 = tm.train_step((sparse, dense01, radius), opt)
    assert torch.isfinite(l1) and torch.isfinite(l2)
    assert not torch.equal(w0, tm.network.feat_convs[3].conv_out.weight.detach())   # weights moved
    assert set(tm.logged) >= {"EMD", "logpx", "CD"}
    out = tm.validation_step((sparse, dense01))
    assert torch.isfinite(out["CD"]) and tm.network.training
    # eval() after training: fused inference path agrees with the oracle on the trained weights
    tm.eval()
    x, logp = tm.network(sparse, 4)
    sd = {k: v.detach().cpu() for k, v in tm.network.state_dict().items()}
    xr, lr = O.forward(sd, sparse.cpu(), 4)
    assert (x.cpu() - xr).abs().max() < 1e-5


@pytest.mark.parametrize("graph", [False, True])
def test_eval_after_training_sees_the_new_weights(graph):
    """The eval path runs from a packed plan cached on the module.  The fused optimizer, a replayed training graph and the
    fused BatchNorm kernels write parameters / running statistics through raw pointers: the plan must still be rebuilt (an eval
    forward BEFORE training caches a plan; validation between epochs once kept returning the same CD)."""
    from puflow_amd.trainer import TrainerModule, default_cfg
    torch.manual_seed(0)
    tm = TrainerModule(default_cfg(learning_rate=1e-3), loss_mix="pugan")
    tm.network.load_state_dict(synth_state_dict(22))
    tm = tm.to(DEV)
    opt = tm.configure_optimizers()["optimizer"]
    dense01 = ((synth_patches(4, 1024, seed=6) + 1) / 2).to(DEV)
    sparse = dense01[:, ::4].contiguous()
    batch = (sparse, dense01, torch.ones(4, device=DEV))
    tm.network.set_to_initialized_state()
    tm.eval()
    x0, _ = tm.network(sparse, 4)                                   # caches the plan of the initial weights
    x0 = x0.clone()
    tm.train()
    if graph:
        step = tm.graphed_train_step(batch, opt, warmup=1)
        for _ in range(3):
            step(batch)
    else:
        for _ in range(3):
            tm.train_step(batch, opt)
    cd1 = float(tm.validation_step((sparse, dense01))["CD"])         # eval inside, back to train()
    if graph:
        step(batch)
    else:
        tm.train_step(batch, opt)
    cd2 = float(tm.validation_step((sparse, dense01))["CD"])
    assert cd1 != cd2                                                # another step, another validation value
    tm.eval()
    x1, _ = tm.network(sparse, 4)
    sd = {k: v.detach().cpu() for k, v in tm.network.state_dict().items()}
    xr, _ = O.forward(sd, sparse.cpu(), 4)
    err, moved = float((x1.cpu() - xr).abs().max()), float((x1 - x0).abs().max())
    assert err < 1e-5, (err, moved)                                  # the CURRENT weights and running statistics
    assert moved > 1e-4, moved                                       # and not the ones cached before training


def test_training_step_at_the_real_batch_size_matches_the_oracle():
    """BASELINE configs[2] shape: 32 patches of 256 -> 1024 points per rank.  The HIP train-mode forward + backward
    against the train-mode oracle (oracle/ref_cpu.py::forward_train, itself pinned to the reference's own training
    step at B = 4 by tests/golden/train_step.npz): x, logp, CD, loss and the gradient norm of every parameter."""
    _real_batch_step()


def _real_batch_step(deterministic=False):
    """test_training_step_at_the_real_batch_size_matches_the_oracle's body; deterministic: net.deterministic, bars unchanged."""
    from puflow_amd import ops
    from puflow_amd.interpflow import PointInterpFlow
    B, N, R = 32, 256, 4
    sd = synth_state_dict(77)
    dense = synth_patches(B, N * R, seed=78)
    sparse = dense[:, ::R].contiguous()
    # oracle on CPU (autograd over the restatement)
    sdr = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.clone()) for k, v in sd.items()}
    xr, lr, _ = O.forward_train(sdr, sparse, R, actnorm_init=True)
    cdr = _chamfer_cpu(xr, dense)
    lossr = lr * 1e-4 + cdr * 1e-1
    lossr.backward()
    net = PointInterpFlow(3)
    net.load_state_dict(sd)
    net = net.to(DEV).train()
    net.deterministic = deterministic
    x, logp = net(sparse.to(DEV), R)
    cd, _ = ops.chamfer_distance(x, dense.to(DEV))
    loss = logp * 1e-4 + cd * 1e-1
    loss.backward()
    assert (x.detach().cpu() - xr.detach()).abs().max() < 2e-5
    np.testing.assert_allclose(float(logp), float(lr), rtol=1e-5)
    np.testing.assert_allclose(float(cd), float(cdr), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(float(loss), float(lossr), rtol=1e-5)
    params = dict(net.named_parameters())
    ref_grad = {k: v.grad for k, v in sdr.items() if v.requires_grad and v.grad is not None}
    assert len(ref_grad) > 150
    _assert_grads_elementwise(params, ref_grad)


def test_train_entry_runs_epochs_on_the_gpu(tmp_path):
    """puflow_amd.train.train(): dict batches (the reference's PU1K form) from the synthetic data module, two epochs with
    validation; the scheduler sees the CD, the losses are finite, weights move, ActNorm gets its first-batch init."""
    from puflow_amd.data import SyntheticPatchData
    from puflow_amd.train import train
    from puflow_amd.trainer import default_cfg
    kw = dict(num_point_patch=256, up_ratio=4, batch_size=4, device=DEV)
    tr = SyntheticPatchData(num_patches=8, seed=1, **kw)
    va = SyntheticPatchData(num_patches=4, seed=2, is_augment=False, **kw)
    # EMD expects coordinates in about [0, 1]: shift the unit-ball patches
    for d in (tr, va):
        d.inp = d.inp * 0.5 + 0.5; d.gt = d.gt * 0.5 + 0.5; d.is_augment = False
    mod, hist = train("Train", str(tmp_path / "x.ckpt"), None, default_cfg(sched_patience=0), tr, va, max_epochs=2,
                      dataset="pu1k", device=DEV, log=None)
    assert hist["epochs"] == 2 and len(hist["CD"]) == 2 and all(np.isfinite(hist["CD"])) and all(np.isfinite(hist["loss"]))
    assert all(b.actnorm.is_inited for b in mod.network.flow_blocks)
    assert not os.path.exists(str(tmp_path / "x-epoch2.ckpt"))                  # <= 10 epochs: not saved (train_pu1k.py:173)
    assert mod.epoch == 2


def test_train_entry_with_graph_replay(tmp_path):
    """train(..., graph=True): each batch shape is captured once (its single warm-up step is that batch's optimisation step)
    and replayed afterwards; the scheduler's learning-rate change reaches the captured kernels; same bookkeeping as the eager
    loop."""
    from puflow_amd.data import SyntheticPatchData
    from puflow_amd.optim import FusedClipAdam
    from puflow_amd.train import train
    from puflow_amd.trainer import default_cfg
    kw = dict(num_point_patch=256, up_ratio=4, batch_size=4, device=DEV)
    tr = SyntheticPatchData(num_patches=12, seed=1, **kw)
    va = SyntheticPatchData(num_patches=4, seed=2, is_augment=False, **kw)
    for d in (tr, va):
        d.inp = d.inp * 0.5 + 0.5; d.gt = d.gt * 0.5 + 0.5; d.is_augment = False
    cfg = default_cfg(sched_patience=0, sched_factor=0.5, learning_rate=1e-3)
    mod, hist = train("Train", str(tmp_path / "x.ckpt"), None, cfg, tr, va, max_epochs=3, dataset="pu1k", device=DEV, log=None,
                      graph=True)
    assert hist["epochs"] == 3 and all(np.isfinite(hist["CD"])) and all(np.isfinite(hist["loss"]))
    assert all(b.actnorm.is_inited for b in mod.network.flow_blocks) and mod.epoch == 3
    assert len(hist["lr"]) == 3 and hist["lr"][-1] <= hist["lr"][0]


def test_graphed_train_step_follows_the_eager_trajectory():
    """TrainerModule.graphed_train_step: forward + loss + backward + clip + Adam replayed from a hipGraph (same kernels, same
    order as the eager step).  Its constructor runs `warmup` eager steps (ActNorm init, optimizer state) before the capture,
    so with warmup=1 the first replay is the second optimisation step and must return the eager path's second-step loss;
    replays keep training, take new batches and new learning rates."""
    from puflow_amd.trainer import TrainerModule, default_cfg
    dense = ((synth_patches(4, 1024, seed=5) + 1) / 2).to(DEV)
    sparse = dense[:, ::4].contiguous()
    batch = (sparse, dense, torch.ones(4, device=DEV))

    def make():
        torch.manual_seed(0)
        tm = TrainerModule(default_cfg(learning_rate=1e-3), loss_mix="pugan")
        tm.network.load_state_dict(synth_state_dict(21))
        tm = tm.to(DEV)
        return tm, tm.configure_optimizers()["optimizer"]

    tm, opt = make()
    eager = [float(tm.train_step(batch, opt)) for _ in range(3)]
    tg, optg = make()
    step = tg.graphed_train_step(batch, optg, warmup=1)       # one eager warm-up step (ActNorm init, optimizer state), then capture
    l2 = float(step(batch))
    # the first replay is the second optimisation step.  The loss is not bit-reproducible (float atomics in the remaining
    # scatter-adds reorder sums and the auction assignment amplifies that: the eager second-step loss itself varies by ~0.3 %
    # from run to run, the third by > 1 %), so the comparison is made as early as possible, with a 1.5 % bound
    assert abs(l2 - eager[1]) <= 1.5e-2 * abs(eager[1]), (l2, eager)
    l3 = float(step(batch))
    assert abs(l3 - eager[2]) <= 8e-2 * abs(eager[2]), (l3, eager)
    w0 = tg.network.feat_convs[2].conv_out.weight.detach().clone()
    losses = [float(step(batch)) for _ in range(5)]
    assert all(np.isfinite(losses)) and not torch.equal(w0, tg.network.feat_convs[2].conv_out.weight.detach())
    assert tg._bucket is None or True
    # a different batch through the same graph (static buffers are refilled)
    dense2 = ((synth_patches(4, 1024, seed=6) + 1) / 2).to(DEV)
    l_other = float(step((dense2[:, ::4].contiguous(), dense2, torch.ones(4, device=DEV))))
    assert np.isfinite(l_other) and l_other != losses[-1]
    step.set_lr(5e-4)
    assert float(optg.param_groups[0]["lr"]) == pytest.approx(5e-4)


def test_sticky_timeout_word_survives_graph_replays():
    """the persistent kernels' barrier / status words are cached per (device, stream) and zero-initialised; allocated
    INSIDE the capture their torch.zeros would be a memset node that clears the sticky time-out word sync[3] on every replay,
    so a time-out of replay i would be gone after replay i + 1.  GraphedTrainStep warms up on its capture stream (the words
    exist before capture_begin); train_ops refuses to allocate them while capturing.  Here: a set word survives two replays and
    check_persist_status raises."""
    from puflow_amd import _lib, train_ops
    from puflow_amd.trainer import TrainerModule, default_cfg
    dense = ((synth_patches(4, 1024, seed=5) + 1) / 2).to(DEV)
    batch = (dense[:, ::4].contiguous(), dense, torch.ones(4, device=DEV))
    torch.manual_seed(0)
    tm = TrainerModule(default_cfg(learning_rate=1e-3), loss_mix="pugan")
    tm.network.load_state_dict(synth_state_dict(21))
    tm = tm.to(DEV)
    opt = tm.configure_optimizers()["optimizer"]
    step = tm.graphed_train_step(batch, opt, warmup=1)
    key = (torch.device(DEV), step.capture_stream.cuda_stream)
    assert key in train_ops._SYNCW, "the capture stream's barrier words must exist before the capture (allocated by the warm-up)"
    words = train_ops._SYNCW[key]
    float(step(batch))
    assert words.tolist() == [0, 0, 0, 0]
    words[3] = 1                                   # what a timed-out grid barrier leaves
    float(step(batch)); float(step(batch))
    assert int(words[3]) == 1, "a replay cleared the sticky status word"
    with pytest.raises(_lib.PuflowHipError):
        train_ops.check_persist_status(DEV)
    assert words.tolist() == [0, 0, 0, 0]
    # and the guard: no zero-initialised scratch may be born inside a capture
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with pytest.raises(RuntimeError, match="inside a hipGraph capture"):
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            train_ops._sync_words(torch.device(DEV))
    train_ops._SYNCW.pop((torch.device(DEV), s.cuda_stream), None)


def test_deterministic_switch_makes_the_step_bit_reproducible():
    """cfg.deterministic (VERDICT / ADVICE r4): two runs of ONE training step with the full PU-GAN loss - the EMD term, whose
    auction turns a 1e-7 difference of x into other assignments, included - from the same state give the same bits in the loss
    and in every gradient element: BatchNorm statistics as exact fixed-point sums (PF_TRAIN_DETERMINISTIC), the latent's and
    Chamfer's gradients as ordered gathers, the dQ gather over sorted transposed lists.  The default mode (float / double
    atomics in arrival order, persistent kernels) computes the same step to rounding."""
    from puflow_amd.trainer import TrainerModule, default_cfg
    dense = ((synth_patches(8, 1024, seed=5) + 1) / 2).to(DEV)
    batch = (dense[:, ::4].contiguous(), dense, torch.ones(8, device=DEV))

    def run(det):
        torch.manual_seed(0)
        tm = TrainerModule(default_cfg(learning_rate=1e-3, deterministic=det), loss_mix="pugan")
        tm.network.load_state_dict(synth_state_dict(21))
        tm = tm.to(DEV).train()
        tm._sync_actnorm_init(batch)
        out = []
        for _ in range(2):         # the first pass initialises ActNorm (per-block autograd nodes), the second runs the chain kernels
            tm.zero_grad(set_to_none=True)
            loss = tm.training_step(batch, 0)
            loss.backward()
            torch.cuda.synchronize()
            out.append((float(loss), {k: p.grad.detach().clone() for k, p in tm.named_parameters() if p.grad is not None},
                        float(tm.logged["EMD"])))
        return out

    ra, rb = run(True), run(True)
    for (la, ga, ea), (lb, gb, eb) in zip(ra, rb):
        assert la == lb and ea == eb, (la, lb, ea, eb)
        assert ga.keys() == gb.keys() and len(ga) > 150
        bad = [k for k in ga if not torch.equal(ga[k], gb[k])]
        assert not bad, bad[:5]
    rd = run(False)                                       # the default mode: the same step to rounding (forward: x within 1e-6)
    assert abs(rd[0][0] - ra[0][0]) <= 5e-3 * abs(ra[0][0]), (rd[0][0], ra[0][0])
    from puflow_amd import train_ops
    train_ops.set_deterministic(False)


def test_weight_gradient_stream_changes_no_bit():
    """The split-K weight-gradient kernels of the EdgeConv units, the conditioner MLPs and the flow chains run on one more stream
    beside the backward chain (train_ops._dw_begin, csrc/api.hip pf_train_set_dw_stream), joined by an autograd end-of-pass
    callback.  Same kernels on the same data: under cfg.deterministic the loss and EVERY gradient element are the bits of the
    one-chain order (cfg.dw_stream = False), step after step - eagerly, and replayed from a captured graph with the graph's
    optimizer step applied (so the join really is ahead of the consumer)."""
    from puflow_amd.trainer import TrainerModule, default_cfg
    from puflow_amd import train_ops
    dense = ((synth_patches(8, 1024, seed=5) + 1) / 2).to(DEV)
    batch = (dense[:, ::4].contiguous(), dense, torch.ones(8, device=DEV))

    def run(dw, graphed):
        torch.manual_seed(0)
        tm = TrainerModule(default_cfg(learning_rate=1e-3, deterministic=True, dw_stream=dw), loss_mix="pugan")
        tm.network.load_state_dict(synth_state_dict(21))
        tm = tm.to(DEV).train()
        tm._sync_actnorm_init(batch)
        out = []
        if graphed:
            opt = tm.configure_optimizers()["optimizer"]
            gs = tm.graphed_train_step(batch, opt, warmup=1)
            for _ in range(3):
                out.append(float(gs(batch)))
            torch.cuda.synchronize()
            return out, {k: p.detach().clone() for k, p in tm.named_parameters()}
        for _ in range(3):         # the first pass initialises ActNorm (per-block autograd nodes), the next ones run the chain kernels
            tm.zero_grad(set_to_none=True)
            loss = tm.training_step(batch, 0)
            loss.backward()
            # no device-wide synchronize here: whoever reads .grad on the CURRENT stream must see finished gradients
            out.append((float(loss), {k: p.grad.detach().clone() for k, p in tm.named_parameters() if p.grad is not None}))
        return out

    try:
        ra, rb = run(True, False), run(False, False)
        assert train_ops._DW_STREAMS, "the weight-gradient stream was never used"
        for (la, ga), (lb, gb) in zip(ra, rb):
            assert la == lb, (la, lb)
            assert ga.keys() == gb.keys() and len(ga) > 150
            bad = [k for k in ga if not torch.equal(ga[k], gb[k])]
            assert not bad, bad[:5]
        (la, pa), (lb, pb) = run(True, True), run(False, True)
        assert la == lb, (la, lb)
        bad = [k for k in pa if not torch.equal(pa[k], pb[k])]
        assert not bad, bad[:5]
    finally:
        train_ops.set_deterministic(False)


def test_side_stream_branch_of_the_training_forward_changes_nothing():
    """The interpolation weights of the train-mode forward run on a side stream beside the feature extractor / flow f chain
    (a parallel branch of a captured step).  Same loss, same outputs, same gradients as the one-stream order (float atomics of
    the neighbour scatter make gradients equal to rounding, not to the bit), eagerly and from a captured graph."""
    from puflow_amd import ops
    from puflow_amd.interpflow import PointInterpFlow
    sd = synth_state_dict(31)
    dense = synth_patches(4, 1024, seed=32).to(DEV)
    sparse = dense[:, ::4].contiguous()
    res = {}
    for streams in (False, True):
        net = PointInterpFlow(3)
        net.load_state_dict(sd)
        net.set_to_initialized_state()
        net = net.to(DEV).train()
        net.train_streams = streams
        x, logp = net(sparse, 4)
        cd, _ = ops.chamfer_distance(x, dense)
        loss = logp * 1e-4 + cd * 1e-1
        loss.backward()
        torch.cuda.synchronize()
        res[streams] = (x.detach().clone(), float(loss), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None},
                        {k: b.detach().clone() for k, b in net.named_buffers()})
    xa, la, ga, ba = res[False]
    xb, lb, gb, bb = res[True]
    assert torch.equal(xa, xb) and la == lb
    assert ga.keys() == gb.keys() and len(ga) > 150
    floor = 1e-5 * max(float(g.abs().max()) for g in ga.values())        # a bias in front of a BatchNorm has gradient 0 + rounding noise
    for k in ga:
        assert float((ga[k] - gb[k]).abs().max()) <= 1e-4 * float(ga[k].abs().max()) + floor, k
    for k in ba:
        assert torch.allclose(ba[k].float(), bb[k].float(), rtol=1e-6, atol=1e-7), k


def test_weight_unit_fold_is_the_same_function():
    """WeightEstimationUnit's first conv sees cat[DistanceEncoder, EdgeConv] with no nonlinearity after the producers' last
    (linear) layers (interpflow.py:98,134,144-146,219-221): in the training step those layers run with the product weights
    (train_ops.FoldWuFn: pf_fold_wu_fwd / _bwd) and the first conv is the sum of their outputs (PF_BNMLP_SUM_INPUTS) - two
    [E8, 128] x [128, 128] products per direction less.  Same outputs, loss, running statistics and gradients (also of the six
    folded tensors, which now get theirs through the fold's chain rule) as the unfolded order, to rounding; and the fold kernels
    against torch's matmul autograd."""
    from puflow_amd import ops, train_ops as T
    from puflow_amd.interpflow import PointInterpFlow
    g = torch.Generator().manual_seed(3)
    W0, b0 = torch.randn(128, 256, 1, 1, generator=g).to(DEV).requires_grad_(), torch.randn(128, generator=g).to(DEV).requires_grad_()
    W6, b6 = torch.randn(128, 64, 1, 1, generator=g).to(DEV).requires_grad_(), torch.randn(128, generator=g).to(DEV).requires_grad_()
    Wo, bo = torch.randn(128, 137, 1, 1, generator=g).to(DEV).requires_grad_(), torch.randn(128, generator=g).to(DEV).requires_grad_()
    outs = T.FoldWuFn.apply(W0, b0, W6, b6, Wo, bo)
    W0m = W0.reshape(128, 256).double()
    refs = ((W0m[:, :128] @ W6.reshape(128, 64).double()).reshape(W6.shape), W0m[:, :128] @ b6.double() + b0.double(),
            (W0m[:, 128:] @ Wo.reshape(128, 137).double()).reshape(Wo.shape), W0m[:, 128:] @ bo.double())
    cot = [torch.randn(o.shape, generator=g).to(DEV) for o in outs]
    got = torch.autograd.grad(outs, (W0, b0, W6, b6, Wo, bo), cot)
    ref = torch.autograd.grad(refs, (W0, b0, W6, b6, Wo, bo), [c.double() for c in cot])
    for o, r in zip(outs, refs):
        assert float((o.double() - r).abs().max()) <= 1e-5 * float(r.abs().max())
    for a, r in zip(got, ref):
        assert float((a.double() - r.double()).abs().max()) <= 1e-5 * float(r.abs().max())

    sd = synth_state_dict(33)
    dense = synth_patches(4, 1024, seed=34).to(DEV)
    sparse = dense[:, ::4].contiguous()
    res = {}
    was = T._FOLD_WU
    try:
        for fold in (False, True):
            T._FOLD_WU = fold
            net = PointInterpFlow(3)
            net.load_state_dict(sd)
            net.set_to_initialized_state()
            net = net.to(DEV).train()
            x, logp = net(sparse, 4)
            cd, _ = ops.chamfer_distance(x, dense)
            loss = logp * 1e-4 + cd * 1e-1
            loss.backward()
            torch.cuda.synchronize()
            res[fold] = (x.detach().clone(), float(loss), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None},
                         {k: b.detach().clone() for k, b in net.named_buffers()})
    finally:
        T._FOLD_WU = was
    xa, la, ga, ba = res[False]
    xb, lb, gb, bb = res[True]
    assert float((xa - xb).abs().max()) <= 2e-5 and abs(la - lb) <= 1e-5 * abs(la)
    assert ga.keys() == gb.keys() and len(ga) > 150
    floor = 1e-4 * max(float(g_.abs().max()) for g_ in ga.values())       # a bias in front of a BatchNorm has gradient 0 + rounding noise
    for k in ga:
        assert float((ga[k] - gb[k]).abs().max()) <= 2e-3 * float(ga[k].abs().max()) + floor, k
    for k in ba:
        assert torch.allclose(ba[k].float(), bb[k].float(), rtol=1e-4, atol=1e-6), k


def test_batched_weight_fold_changes_no_bit():
    """The six feature units' folded edge-feature weights (W_p = W_a - W_c | W_q = W_b + W_c, interpflow.py:190-248 on
    cat[x_i, x_j, x_j - x_i]) come from ONE launch at the top of the forward (pf_ec_train_fold_batch) instead of one at the head of
    every unit: same expressions, so - in the bit-reproducible mode, where two runs can be compared at all - the same output,
    loss and gradients bit for bit; and the batched call against the expressions themselves."""
    from puflow_amd import ops, train_ops as T
    from puflow_amd.interpflow import PointInterpFlow
    sd = synth_state_dict(51)
    dense = synth_patches(4, 1024, seed=52).to(DEV)
    sparse = dense[:, ::4].contiguous()
    net = PointInterpFlow(3)
    net.load_state_dict(sd)
    net = net.to(DEV)
    pre = T.ec_prefold(list(net.feat_convs), sparse, 16)
    assert pre is not None and len(pre) == len(net.feat_convs)
    C = 3
    for (Wpq, bpq), u in zip(pre, net.feat_convs):
        convs = [seq[0] for seq in u.convs] + [u.conv_out]
        Ws = [c.weight.reshape(c.weight.shape[0], -1) for c in convs]
        Wp = torch.cat([w[:, :C] - w[:, 2 * C:3 * C] for w in Ws])
        Wq = torch.cat([w[:, C:2 * C] + w[:, 2 * C:3 * C] for w in Ws])
        assert torch.equal(Wpq, torch.cat([Wp, Wq]))
        assert torch.equal(bpq, torch.cat([torch.cat([c.bias for c in convs]), torch.zeros_like(bpq[:Wp.shape[0]])]))
        C = u.conv_out.weight.shape[0]
    res = _step_under_switch(T, "_PREFOLD", sd, sparse, dense)
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1], res[True][1])
    assert res[False][2].keys() == res[True][2].keys() and len(res[True][2]) > 150
    for k in res[False][2]:
        assert torch.equal(res[False][2][k], res[True][2][k]), k


def test_batch_hand_over_in_one_launch():
    """pf_copy_n: up to eight 32-bit regions copied by one launch (aligned and unaligned bases, sizes that are no multiple of 4),
    and GraphedTrainStep._copy_in through it: the tensors the captured step reads hold the new batch."""
    import ctypes
    from puflow_amd import _lib
    from puflow_amd.train_graph import GraphedTrainStep
    lib = _lib.load()
    g = torch.Generator().manual_seed(8)
    sizes = [1, 3, 4, 32 * 256 * 3, 32 * 1024 * 3, 32, 1023, 4099]
    base = [torch.randn(n + 1, generator=g).to(DEV) for n in sizes]
    src = [b[1:] if k % 2 else b[:-1] for k, b in enumerate(base)]             # odd ones start 4 bytes off a 16-byte boundary
    dst = [torch.zeros(n + 2, device=DEV) for n in sizes]
    dv = [d[2:] if k % 3 == 0 else d[:-2] for k, d in enumerate(dst)]
    n = len(sizes)
    assert lib.pf_copy_n((ctypes.c_void_p * n)(*[t.data_ptr() for t in src]), (ctypes.c_void_p * n)(*[t.data_ptr() for t in dv]),
                         (ctypes.c_longlong * n)(*sizes), n, None) == 0
    torch.cuda.synchronize()
    for a, b, d, k in zip(src, dv, dst, range(n)):
        assert torch.equal(a, b)
        assert float(d[:2].abs().sum() if k % 3 == 0 else d[-2:].abs().sum()) == 0.0       # nothing written outside the region
    assert lib.pf_copy_n(None, None, None, 1, None) == -1

    class _Holder:
        pass
    h = _Holder()
    h.static = (torch.zeros(4, 256, 3, device=DEV), torch.zeros(4, 1024, 3, device=DEV), torch.zeros(4, device=DEV),
                torch.zeros(5, dtype=torch.int64, device=DEV))
    new = (torch.randn(4, 256, 3, generator=g).to(DEV), torch.randn(4, 1024, 3, generator=g).to(DEV), torch.randn(4, generator=g).to(DEV),
           torch.arange(5, device=DEV))
    GraphedTrainStep._copy_in(h, new)
    torch.cuda.synchronize()
    for a, b in zip(h.static, new):
        assert torch.equal(a, b)


def _step_under_switch(T, name, sd, sparse, dense):
    """forward + backward of the bit-reproducible mode with train_ops.<name> off and on -> {flag: (x, loss, gradients)}"""
    from puflow_amd import ops
    from puflow_amd.interpflow import PointInterpFlow
    res = {}
    was = getattr(T, name)
    try:
        for on in (False, True):
            setattr(T, name, on)
            net = PointInterpFlow(3)
            net.load_state_dict(sd)
            net.set_to_initialized_state()
            net = net.to(DEV).train()
            net.deterministic = True
            x, logp = net(sparse, 4)
            cd, _ = ops.chamfer_distance(x, dense)
            loss = logp * 1e-4 + cd * 1e-1
            loss.backward()
            torch.cuda.synchronize()
            res[on] = (x.detach().clone(), loss.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None})
    finally:
        setattr(T, name, was)
        T.set_deterministic(False)
    return res


def test_gradient_fan_in_without_add_launches():
    """Two places where autograd summed a tensor's gradients with launches of its own, now inside kernels of ours:
    (a) a feature unit's output h_i feeds its FeatMergeUnit and unit i + 1 (interpflow.py:300-306): unit i + 1 hands h_i on to the
        merge unit as a second output (tap), so the merge unit's gradient arrives at unit i + 1's backward and is added in the
        epilogue of its dx GEMM (PfEcTrain.dx_add) - the same two addends, hence the same bits;
    (b) the flattened conditioning features feed both flow chains and both injector families: FanoutFn sums the four gradients in
        one launch (pf_sum_n) - another association of the same four addends, hence rounding-level differences only.
    And pf_sum_n against torch for every operand count."""
    from puflow_amd import _lib, train_ops as T
    import ctypes
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    for n in range(2, 9):
        ts = [torch.randn(4 * 1031, generator=g).to(DEV) for _ in range(n)]
        out = torch.empty_like(ts[0])
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
        assert lib.pf_sum_n(ptrs, n, out.data_ptr(), out.numel(), None) == 0
        ref = ts[0].clone()
        for t in ts[1:]:
            ref = ref + t
        torch.cuda.synchronize()
        assert torch.equal(out, ref), n
    assert lib.pf_sum_n(ptrs, 8, out.data_ptr(), 6, None) == -2 and lib.pf_sum_n(ptrs, 1, out.data_ptr(), 8, None) == -2

    sd = synth_state_dict(61)
    dense = synth_patches(4, 1024, seed=62).to(DEV)
    sparse = dense[:, ::4].contiguous()
    res = _step_under_switch(T, "_TAP", sd, sparse, dense)
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1], res[True][1])
    assert res[False][2].keys() == res[True][2].keys() and len(res[True][2]) > 150
    for k in res[False][2]:
        assert torch.equal(res[False][2][k], res[True][2][k]), k
    res = _step_under_switch(T, "_FANOUT", sd, sparse, dense)
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1], res[True][1])
    assert res[False][2].keys() == res[True][2].keys()
    floor = 1e-5 * max(float(v.abs().max()) for v in res[False][2].values())      # the sums' rounding, carried through six units' backward
    for k in res[False][2]:
        a, b = res[False][2][k], res[True][2][k]
        assert float((a - b).abs().max()) <= 2e-4 * float(a.abs().max()) + floor, k


@pytest.mark.parametrize("B,N", [(4, 256), (3, 100)])
def test_flow_chain_node_matches_the_per_block_nodes(B, N):
    """All flow blocks of a direction as one autograd node (csrc/train_flowchain.hip, FlowChainFn) against one node per block
    piece (PF_TRAIN_CHAIN=0: train_flow.hip + train_mlp.hip): outputs, loss and every gradient.  Same products in the same
    MFMA order; sums over rows are taken in a different (fixed) order, hence rounding-level differences.  N = 100: partial
    16-row tiles in both directions."""
    from puflow_amd import ops, train_ops as T
    from puflow_amd._prof import profile_calls
    from puflow_amd.interpflow import PointInterpFlow
    sd = synth_state_dict(41)
    dense = synth_patches(B, 4 * N, seed=42).to(DEV)
    sparse = dense[:, ::4].contiguous()
    res = {}
    keep = T._CHAIN
    try:
        for chain in (False, True):
            T._CHAIN = chain
            net = PointInterpFlow(3)
            net.load_state_dict(sd)
            net.set_to_initialized_state()
            net = net.to(DEV).train()
            with profile_calls() as prof:
                x, logp = net(sparse, 4)
                cd, _ = ops.chamfer_distance(x, dense)
                loss = logp * 1e-4 + cd * 1e-1
                loss.backward()
            torch.cuda.synchronize()
            assert len(prof.events.get("pf_flowchain_fwd", [])) == (2 if chain else 0)        # the path under test really ran
            assert len(prof.events.get("pf_flowchain_bwd", [])) == (2 if chain else 0)
            res[chain] = (x.detach().clone(), float(logp), float(loss),
                          {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None})
    finally:
        T._CHAIN = keep
    xa, pa, la, ga = res[False]
    xb, pb, lb, gb = res[True]
    assert float((xa - xb).abs().max()) <= 2e-6
    assert abs(pa - pb) <= 1e-6 * abs(pa) and abs(la - lb) <= 1e-6 * abs(la)
    assert ga.keys() == gb.keys() and len(ga) > 150
    floor = 1e-5 * max(float(g.abs().max()) for g in ga.values())
    for k in ga:
        assert float((ga[k] - gb[k]).abs().max()) <= 2e-4 * float(ga[k].abs().max()) + floor, k


def test_fused_glue_of_the_training_step_matches_the_torch_expressions():
    """PF_TRAIN_GLUE: the log-likelihood from the f chain kernel's epilogue, the latent interpolation as one kernel and the PU-GAN
    loss head as one autograd node (csrc/train_glue.hip, loss.PuganLossFn) against the torch expressions they replace: the
    training step's loss, its logged terms and every gradient, with per-sample radii."""
    import copy
    from puflow_amd import train_ops as T
    from puflow_amd._prof import profile_calls
    from puflow_amd.trainer import TrainerModule, default_cfg
    dense = ((synth_patches(4, 1024, seed=52) + 1) / 2).to(DEV)
    batch = (dense[:, ::4].contiguous(), dense, torch.tensor([0.8, 1.0, 1.3, 0.9], device=DEV))
    tm = TrainerModule(default_cfg(learning_rate=1e-3), loss_mix="pugan")
    tm.network.load_state_dict(synth_state_dict(51))
    tm.network.set_to_initialized_state()
    tm = tm.to(DEV).train()
    state = copy.deepcopy(tm.state_dict())
    res = {}
    keep = T._GLUE
    try:
        for glue in (False, True):
            T._GLUE = glue
            tm.load_state_dict(state)
            for p in tm.parameters():
                p.grad = None
            with profile_calls() as prof:
                loss = tm.training_step(batch, 0)
                loss.backward()
            torch.cuda.synchronize()
            # (the loss head's backward: pf_pugan_grad - two launches; pf_pugan_loss_bwd + pf_chamfer_bwd + pf_emd_backward remain
            # for a ground truth that wants its gradient and for the bit-reproducible mode)
            for name in ("pf_pugan_loss_fwd", "pf_pugan_grad", "pf_interp_wsum_fwd", "pf_interp_wsum_bwd"):
                assert len(prof.events.get(name, [])) == (1 if glue else 0), name
            assert "pf_pugan_loss_bwd" not in prof.events
            res[glue] = (float(loss), tm.logged_values(), {k: p.grad.detach().clone() for k, p in tm.named_parameters() if p.grad is not None})
    finally:
        T._GLUE = keep
    (la, ta, ga), (lb, tb, gb) = res[False], res[True]
    assert abs(la - lb) <= 2e-6 * abs(la)
    for k in ("CD", "EMD", "logpx"):
        assert abs(ta[k] - tb[k]) <= 2e-6 * abs(ta[k]) + 1e-9, k
    assert ga.keys() == gb.keys() and len(ga) > 150
    floor = 1e-5 * max(float(g.abs().max()) for g in ga.values())
    for k in ga:
        assert float((ga[k] - gb[k]).abs().max()) <= 2e-4 * float(ga[k].abs().max()) + floor, k


@pytest.mark.parametrize("B,N,R", [(2, 100, 4), (3, 256, 2), (1, 37, 1)])
def test_latent_interpolation_kernel_matches_torch(B, N, R):
    """pf_interp_wsum (csrc/train_glue.hip) against the torch expression it replaces (interpflow.py:153-186, 312-318): gather of
    the neighbours' latent rows, softmax over the 8 neighbours of the first R weight channels, weighted sum, [B, N R, 3] layout -
    forward and both gradients."""
    from puflow_amd import train_ops as T
    g = torch.Generator(device="cpu").manual_seed(7 + N)
    ldw = 32
    w0 = torch.randn(B * N, 8, ldw, generator=g).to(DEV)
    z0 = torch.randn(B, N, 3, generator=g).to(DEV)
    idx = torch.randint(0, N, (B, N, 8), generator=g, dtype=torch.int32).to(DEV)
    gu = torch.randn(B, N * R, 3, generator=g).to(DEV)

    def ref(w, z):
        zj = z[torch.arange(B, device=DEV).view(B, 1, 1), idx.long()]                   # [B,N,8,3]
        a = torch.softmax(w.view(B, N, 8, ldw)[..., :R].double(), dim=2)                # [B,N,8,R]
        return torch.einsum("bnkr,bnkc->bnrc", a, zj.double()).reshape(B, N * R, 3)

    w1, z1 = w0.clone().requires_grad_(True), z0.clone().requires_grad_(True)
    u1 = T.InterpWsumFn.apply(w1, z1, idx, R)
    (u1 * gu).sum().backward()
    w2, z2 = w0.clone().requires_grad_(True), z0.clone().requires_grad_(True)
    u2 = ref(w2, z2)
    (u2 * gu.double()).sum().backward()
    assert float((u1.double() - u2).abs().max()) <= 2e-6
    assert float((w1.grad.double() - w2.grad.double()).abs().max()) <= 2e-6 * max(1.0, float(w2.grad.abs().max()))
    assert float((z1.grad.double() - z2.grad.double()).abs().max()) <= 1e-5 * max(1.0, float(z2.grad.abs().max()))
    assert float(w1.grad[..., R:].abs().max()) == 0.0


def test_loss_node_without_the_chamfer_term_matches_the_pu1k_mix():
    """w_cd = 0 (train_pu1k.py:62-67: logp + EMD, no radius): no nearest-neighbour search runs, value and gradient as the torch
    expression."""
    from puflow_amd._prof import profile_calls
    from puflow_amd.loss import EarthMoverDistance, PuganLossFn
    B, n = 2, 512
    pred0 = ((synth_patches(B, n, seed=71) + 1) / 2).to(DEV)
    gt = ((synth_patches(B, n, seed=72) + 1) / 2).to(DEV)
    lp0 = torch.tensor(-50.0, device=DEV)
    p1, l1 = pred0.clone().requires_grad_(True), lp0.clone().requires_grad_(True)
    with profile_calls() as prof:
        loss1, terms = PuganLossFn.apply(p1, gt, None, l1, 0.005, 50, 0, (1e-4, 5e-2, 0.0))
        loss1.backward()
    torch.cuda.synchronize()
    assert "pf_chamfer_fwd" not in prof.events and "pf_chamfer_bwd" not in prof.events
    p2, l2 = pred0.clone().requires_grad_(True), lp0.clone().requires_grad_(True)
    loss2 = l2 * 1e-4 + EarthMoverDistance()(p2, gt) * 5e-2
    loss2.backward()
    assert abs(float(loss1) - float(loss2)) <= 2e-6 * abs(float(loss2))
    assert float(terms[2]) == 0.0
    assert float((p1.grad - p2.grad).abs().max()) <= 2e-6 * float(p2.grad.abs().max())
    assert abs(float(l1.grad) - float(l2.grad)) <= 1e-9


@pytest.mark.parametrize("with_radius", [True, False])
def test_pugan_loss_node_matches_the_separate_losses(with_radius):
    """loss.PuganLossFn against EarthMoverDistance + ChamferCUDA + the weighted sum (train_pugan.py:52-67): value, logged terms,
    gradient of the prediction and of logp."""
    from puflow_amd.loss import ChamferCUDA, EarthMoverDistance, PuganLossFn
    B, n = 3, 512
    pred0 = ((synth_patches(B, n, seed=61) + 1) / 2).to(DEV)
    gt = ((synth_patches(B, n, seed=62) + 1) / 2).to(DEV)
    radius = torch.tensor([0.7, 1.0, 1.4], device=DEV) if with_radius else None
    lp0 = torch.tensor(123.456, device=DEV)
    p1, l1 = pred0.clone().requires_grad_(True), lp0.clone().requires_grad_(True)
    loss1, terms = PuganLossFn.apply(p1, gt, radius, l1, 0.005, 50, 0, (1e-4, 5e-2, 1e-1))
    loss1.backward()
    p2, l2 = pred0.clone().requires_grad_(True), lp0.clone().requires_grad_(True)
    emd = EarthMoverDistance()(p2, gt, radius=radius)
    cd, _ = ChamferCUDA()(p2, gt)
    loss2 = l2 * 1e-4 + emd * 5e-2 + cd * 1e-1
    loss2.backward()
    torch.cuda.synchronize()
    assert abs(float(loss1) - float(loss2)) <= 2e-6 * abs(float(loss2))
    for got, want in zip(terms.tolist(), (float(emd) * 5e-2, float(lp0) * 1e-4, float(cd) * 1e-1)):
        assert abs(got - want) <= 2e-6 * abs(want) + 1e-9
    assert float((p1.grad - p2.grad).abs().max()) <= 2e-6 * float(p2.grad.abs().max())
    assert abs(float(l1.grad) - float(l2.grad)) <= 1e-9
    # a ground truth that wants its gradient takes the four-launch backward (pf_pugan_loss_bwd + pf_chamfer_bwd + pf_emd_backward):
    # the same prediction gradient as the two-launch form above, and the Chamfer term's gradient for the ground truth
    p3, l3, g3 = pred0.clone().requires_grad_(True), lp0.clone().requires_grad_(True), gt.clone().requires_grad_(True)
    loss3, _ = PuganLossFn.apply(p3, g3, radius, l3, 0.005, 50, 0, (1e-4, 5e-2, 1e-1))
    loss3.backward()
    p4, g4 = pred0.clone().requires_grad_(True), gt.clone().requires_grad_(True)
    cd4, _ = ChamferCUDA()(p4, g4)
    (cd4 * 1e-1).backward()
    assert float((p3.grad - p1.grad).abs().max()) <= 2e-6 * float(p1.grad.abs().max())
    assert float((g3.grad - g4.grad).abs().max()) <= 2e-6 * float(g4.grad.abs().max())
