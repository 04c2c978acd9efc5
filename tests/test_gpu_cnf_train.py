"""The continuous model in train() mode on the GPU (puflow_amd/cnf.py: flow_train, forward_train; trainer / train entry) against
tests/cnf_train_ref.py, the float64 CPU reference on the step lists the GPU recorded.  Weights: synth_cnf_state_dict(7).

  1. the flow wiring alone (cs, interpolation logits, noise and xyz fed as leaves): per tensor max|got - ref64| / max(1, max|ref64|)
     <= max(2e-5, 4 x err32), err32 = the helper in float32 - the project's bar for a CNF block (tests/test_gpu_cnf_grad.py);
  2. the whole step: every parameter gradient element by element, measure and bar of tests/test_gpu_train.py
     (`_assert_grads_elementwise`, tol 1 % of the tensor's largest reference element + 1e-5 of the largest gradient norm);
  3. net.deterministic: two steps from the same state and noise are bit-identical;
  4. TrainerModule(default_cfg(model="continuous")).train_step; 5. python -m puflow_amd.train --model continuous.

Shapes: (B, N, R) = (2, 128, 4): 1 024 g rows, sixteen 64-row tiles; (3, 50, 2): 150 f rows - a partial tile - and 8 points per
16-row MFMA tile in g.  N >= 17 for the 16-neighbour lists.  The bare net keeps `train_persistent` off."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import cnf_grad_ref as G
import cnf_train_ref as TR
from puflow_amd.weights import synth_cnf_state_dict, synth_patches

DEV = "cuda:0"
SHAPES = [(2, 128, 4), (3, 50, 2)]
CDS = [32, 64, 128, 128, 128, 128]


@functools.lru_cache(maxsize=None)
def _sd():
    return synth_cnf_state_dict(7)


def _net(deterministic=False):
    from puflow_amd.cnf import PointInterpFlow
    net = PointInterpFlow(3)
    net.load_state_dict(_sd(), strict=True)
    net = net.to(DEV).train()
    net.deterministic = deterministic
    return net


def _flow_keys():
    return [k for i in range(6) for k in G.block_keys(i) + [G.end_key(i)]]


# ---- 1. flow wiring ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _flow_case(B, N, R):
    from puflow_amd import cnf, ops, train_ops
    g = torch.Generator().manual_seed(1000 * B + N)
    xyz = synth_patches(B, N, seed=11 + N)
    cs = [torch.randn(B, N, cd, generator=g) * 0.7 for cd in CDS]
    w = torch.randn(B * N * 8, 32, generator=g)
    noise = [torch.randn(B, N, 3, generator=g) for _ in range(6)]
    gx = torch.randn(B, N * R, 3, generator=g)
    loss = lambda x, logp: 0.5 * logp + (x * gx.to(x)).sum()
    net = _net()
    xd = xyz.to(DEV).requires_grad_(True)
    csd = [c.to(DEV).requires_grad_(True) for c in cs]
    wd = w.to(DEV).requires_grad_(True)
    idx16, _ = ops.knn_idx32(xyz.to(DEV), xyz.to(DEV), 16)
    idx8 = idx16[..., :8].contiguous()
    train_ops.set_deterministic(False)
    x, logp = cnf.flow_train(net, xd, R, csd, (None, wd, None, None, idx8), [n.to(DEV) for n in noise])
    steps = [list(s) for s in net.last_train_steps]
    loss(x, logp).backward()
    params = dict(net.named_parameters())
    got = {"x": x.detach().cpu(), "logp": logp.detach().cpu(), "xyz": xd.grad.cpu().reshape(B * N, 3), "w": wd.grad.cpu()}
    got.update({f"cs.{i}": c.grad.cpu() for i, c in enumerate(csd)})
    got.update({k: params[k].grad.detach().cpu() for k in _flow_keys()})
    others = [n for n, p in params.items() if not n.startswith("flow_blocks.") and p.grad is not None]
    ref = {}
    for dt in (torch.float64, torch.float32):
        r = TR.run(_sd(), xyz, R, steps, noise, dt, cs=cs, w=w, idx8=idx8.cpu(), xyz_leaf=True)
        gr = TR.gradients(r, loss)
        gr["x"], gr["logp"] = r.x.detach(), r.logp.detach()
        ref[dt] = gr
    keys = ["x", "logp", "xyz", "w"] + [f"cs.{i}" for i in range(6)] + _flow_keys()
    err = {k: G.rel_err(got[k], ref[torch.float64][k].reshape(got[k].shape)) for k in keys}
    err32 = {k: G.rel_err(ref[torch.float32][k], ref[torch.float64][k]) for k in keys}
    print(f"\nflow wiring {B} x {N} x {R}: steps per integration {[len(s) for s in steps]}")
    for k in keys:
        print(f"  {k:66s} err32 {err32[k]:.2e}  gpu {err[k]:.2e}  max|ref| {float(ref[torch.float64][k].abs().max()):.2e}")
    return dict(keys=keys, err=err, err32=err32, ref=ref[torch.float64], steps=steps, others=others)


@pytest.mark.parametrize("B,N,R", SHAPES)
def test_flow_wiring_matches_float64_on_the_recorded_steps(B, N, R):
    """x, logp and the gradients of every cs[i], the logits, xyz and all 16 x 6 flow-block tensors.  Both directions of a block
    feed its context gradient and its gradient record: a wiring that drops or doubles one is off by O(1) in cs.<i> and in
    every tensor of the block."""
    r = _flow_case(B, N, R)
    assert len(r["steps"]) == 12 and all(len(s) >= 1 for s in r["steps"])
    assert not r["others"]                                         # nothing outside the flow blocks got a gradient
    for k in r["keys"]:
        if k not in ("x", "logp"):
            assert float(r["ref"][k].abs().max()) > 0, k
        assert r["err32"][k] <= 1e-4, ("the float32 yardstick is too coarse for this seed", k, r["err32"][k])
        assert r["err"][k] <= max(2e-5, 4 * r["err32"][k]), (k, r["err"][k], r["err32"][k])


# ---- 2. whole step -----------------------------------------------------------------------------------------------------------------
GROUPS = (("extractor", "feat_convs."), ("merge", "merge_convs."), ("interpolation", "interp."), ("flow blocks", "flow_blocks."))


@functools.lru_cache(maxsize=None)
def _step_case(B, N, R):
    from puflow_amd import ops
    g = torch.Generator().manual_seed(77 + N)
    xyz = synth_patches(B, N, seed=5 + N)
    noise = [torch.randn(B, N, 3, generator=g) for _ in range(6)]
    gx = torch.randn(B, N * R, 3, generator=g)
    loss = lambda x, logp: 0.5 * logp + (x * gx.to(x)).sum()
    net = _net()
    x, logp = net(xyz.to(DEV), R, noise=[n.to(DEV) for n in noise])
    steps = [list(s) for s in net.last_train_steps]
    loss(x, logp).backward()
    idx16, _ = ops.knn_idx32(xyz.to(DEV), xyz.to(DEV), 16)
    r = TR.run(_sd(), xyz, R, steps, noise, torch.float64, idx16=idx16.cpu())
    ref = TR.gradients(r, loss)
    return dict(net=net, x=x.detach().cpu(), logp=logp.detach().cpu(), ref=ref, rx=r.x.detach(), rlogp=r.logp.detach(), steps=steps)


@pytest.mark.parametrize("B,N,R", SHAPES)
def test_whole_step_gradients_match_float64_elementwise(B, N, R):
    from test_gpu_train import _assert_grads_elementwise
    c = _step_case(B, N, R)
    params = dict(c["net"].named_parameters())
    assert set(c["ref"]) == set(params)
    print(f"\nwhole step {B} x {N} x {R}: steps per integration {[len(s) for s in c['steps']]}; "
          f"x {G.rel_err(c['x'], c['rx']):.2e}  logp {G.rel_err(c['logp'], c['rlogp']):.2e}")
    floor = 1e-5 * max(float(v.norm()) for v in c["ref"].values())
    for name, pfx in GROUPS:                                       # reported per group: err / bound of the worst tensor
        worst = (0.0, None)
        for k, ref in c["ref"].items():
            if k.startswith(pfx):
                got = params[k].grad
                got = torch.zeros_like(ref) if got is None else got.detach().cpu().double()
                worst = max(worst, (float((got - ref).abs().max()) / (1e-2 * float(ref.abs().max()) + floor), k))
        print(f"  {name:14s} worst err / bound {worst[0]:.3f}  ({worst[1]})")
    _assert_grads_elementwise(params, {k: v.float() for k, v in c["ref"].items()})


# ---- 3. bit-reproducible mode ------------------------------------------------------------------------------------------------------
def test_deterministic_steps_are_bit_identical():
    B, N, R = 2, 128, 4
    g = torch.Generator().manual_seed(3)
    xyz = synth_patches(B, N, seed=9).to(DEV)
    noise = [torch.randn(B, N, 3, generator=g).to(DEV) for _ in range(6)]
    gx = torch.randn(B, N * R, 3, generator=g).to(DEV)
    runs = []
    for _ in range(2):
        net = _net(deterministic=True)
        x, logp = net(xyz, R, noise=noise)
        loss = 0.5 * logp + (x * gx).sum()
        loss.backward()
        runs.append((loss.detach(), x.detach(), {k: p.grad for k, p in net.named_parameters()}, net.last_train_steps))
    a, b = runs
    assert a[3] == b[3] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(v is not None for v in a[2].values())
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


# ---- 4. trainer --------------------------------------------------------------------------------------------------------------------
def test_trainer_step_updates_every_parameter_and_invalidates_the_eval_plan():
    from puflow_amd.trainer import TrainerModule, default_cfg
    torch.manual_seed(0)
    m = TrainerModule(default_cfg(model="continuous", emd_workgroups=1))
    m.network.load_state_dict(_sd(), strict=True)
    m = m.to(DEV)
    assert m.network.train_persistent is False
    dense = synth_patches(2, 256, seed=21).to(DEV)
    sparse = dense[:, ::4].contiguous()
    noise = [torch.randn(2, 64, 3, device=DEV) for _ in range(6)]
    m.eval()
    with torch.no_grad():
        x0, _ = m(sparse, upratio=4, noise=noise)
    opt = m.configure_optimizers()["optimizer"]
    before = {k: p.detach().clone() for k, p in m.network.named_parameters()}
    loss = m.train_step((sparse, dense), opt)
    assert torch.isfinite(loss)
    # "with a gradient": above the floor tests/test_gpu_train.py uses to tell a gradient from rounding residue (the conv biases in
    # front of a BatchNorm have a mathematically zero one), 1e-5 of the largest gradient norm.  Clipped to a global norm of 1e-2
    # such an element is > 1e-7, ten times Adam's epsilon: the first update moves it by ~lr = 1e-3.
    grads = {k: p.grad for k, p in m.network.named_parameters()}
    assert all(v is not None for v in grads.values())
    floor = 1e-5 * max(float(v.norm()) for v in grads.values())
    changed = {k for k, p in m.network.named_parameters() if not torch.equal(p.detach(), before[k])}
    assert {k for k, v in grads.items() if float(v.abs().max()) > floor} <= changed
    assert {k for k in before if k.startswith("flow_blocks.")} <= changed and len([k for k in changed if k.startswith("flow_blocks.")]) == 96
    m.eval()
    with torch.no_grad():
        x1, _ = m(sparse, upratio=4, noise=noise)
    assert x1.shape == x0.shape and not torch.equal(x1, x0)        # the eval plan was packed anew from the updated weights
    with pytest.raises(RuntimeError, match="cannot be captured"):
        m.graphed_train_step((sparse, dense), opt)
    with pytest.raises(ValueError):
        default_cfg(model="other")
    assert default_cfg().model == "discrete"


# ---- 5. entry ----------------------------------------------------------------------------------------------------------------------
def test_train_entry_runs_the_continuous_model(tmp_path):
    from puflow_amd import train
    from puflow_amd.cnf import PointInterpFlow
    argv = ["--model", "continuous", "--synthetic", "--batch_size", "2", "--max_epochs", "1", "--seed", "3",
            "--checkpoint_path", str(tmp_path / "cnf.ckpt")]
    module, hist = train.main(argv)
    assert hist["epochs"] == 1 and len(hist["CD"]) == 1 and hist["loss"][0] == hist["loss"][0]
    sd = module.network.state_dict()
    fresh = PointInterpFlow(3)
    res = fresh.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    fresh = fresh.to(DEV).eval()
    x, _ = fresh(synth_patches(1, 64, seed=2).to(DEV), 4)
    assert x.shape == (1, 256, 3) and bool(torch.isfinite(x).all())
    with pytest.raises(RuntimeError, match="cannot be captured"):
        train.main(argv + ["--graph"])
