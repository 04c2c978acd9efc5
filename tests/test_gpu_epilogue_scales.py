"""interp_kernel on its scale plan (no rescale multiply in front of an activation; packing.interp_scaled) and the one-instruction
exp / rcp / sqrt of flow_kernel and interp_kernel (pf_mfma.h pf_exp, pf_rcp, pf_sqrt), against the CPU oracle at the bars of
tests/test_gpu_parity.py: x, z, fz and cs[u] within 1e-5 absolute, ldj and logp within 1e-5 relative, g(f(x)) within 2e-6.
Every test prints the deviations it measured.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as O
from puflow_amd.weights import synth_patches, synth_state_dict

DEV = "cuda:0"
SEEDS = (2021, 5, 11)


@pytest.fixture(scope="module")
def lib():
    from puflow_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _lib.load()


def _net(sd):
    from puflow_amd.interpflow import PointInterpFlow
    net = PointInterpFlow(3)
    net.load_state_dict(sd)
    net.set_to_initialized_state()
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def nets(lib):
    """One network per seed, shared by the tests (read-only)."""
    out = {}
    for s in SEEDS:
        sd = synth_state_dict(s)
        out[s] = (sd, _net(sd))
    return out


def _devs(st, ref):
    d = {"x": (st["x"].cpu() - ref["x"]).abs().max().item(),
         "z": (st["z"].cpu() - ref["z"]).abs().max().item(),
         "fz": (st["fz"].cpu() - ref["fz"]).abs().max().item(),
         "ldj_rel": ((st["ldj"].cpu() - ref["ldj"]).abs() / ref["ldj"].abs()).max().item(),
         "logp_rel": abs(float(st["logp"]) - float(ref["logp"])) / abs(float(ref["logp"]))}
    for u in range(6):
        d[f"cs{u}"] = (st["cs"][u].cpu() - ref["cs"][u]).abs().max().item()
    return d


@pytest.mark.parametrize("B,N", [(2, 256), (3, 250)])
def test_forward_against_oracle(nets, B, N):
    """(3, 250): T = 750 is no multiple of 16 - partial wave tiles in interp_kernel (2 points per tile: 375 tiles over 12
    waves), flow f (the two-launch log-likelihood path) and flow g; N >= 16 for the kNN."""
    worst = {}
    for s in SEEDS:
        sd, net = nets[s]
        xyz = synth_patches(B, N, seed=s)
        ref = O.forward(sd, xyz, 4, stages=True)
        st = net.forward_stages(xyz.to(DEV), 4)
        assert torch.equal(st["idx16"].cpu().long(), ref["idx16"])
        d = _devs(st, ref)
        print(f"({B}, {N}) seed {s}: " + "  ".join(f"{k} {v:.2e}" for k, v in d.items()))
        for k, v in d.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"({B}, {N}) maxima over seeds: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v < 1e-5, k


@pytest.mark.parametrize("R", [1, 3, 4, 8])
def test_interp_against_oracle(nets, R):
    """pf_interp alone: R <= 4 the four-row fast path, R = 8 the BIG instantiation (all 32 rows of the last weight conv)."""
    sd, net = nets[SEEDS[0]]
    xyz = synth_patches(2, 256, seed=3)
    ref = O.forward(sd, xyz, R, stages=True)
    st = net.forward_stages(xyz.to(DEV), R)
    dfz = (st["fz"].cpu() - ref["fz"]).abs().max().item()
    dx = (st["x"].cpu() - ref["x"]).abs().max().item()
    print(f"R = {R}: max |fz - oracle| {dfz:.2e}  max |x - oracle| {dx:.2e}")
    assert tuple(st["fz"].shape) == tuple(ref["fz"].shape)
    assert dfz < 1e-5 and dx < 1e-5


def test_flow_f_then_g_against_oracle(nets):
    """pf_flow_fwd_logp, then pf_flow_inv at R = 4 on the oracle's interpolated latents, and g(f(x)) with one replica."""
    from puflow_amd import ops
    sd, net = nets[SEEDS[1]]
    xyz = synth_patches(2, 256, seed=8)
    ref = O.forward(sd, xyz, 4, stages=True)
    xd = xyz.to(DEV)
    _, knn_idx, _ = ops.knn_points(xd, xd, K=16, return_nn=False, return_sorted=False)
    cs = net.feat_extract(xd, knn_idx)
    z, logp = net.log_prob(xd, cs)
    _, ldj = net.f(xd, cs)
    x = net.g(ref["fz"].to(DEV), cs, 4)
    back = net.g(z.unsqueeze(-1), cs, 1)
    dz = (z.cpu() - ref["z"]).abs().max().item()
    dl = ((ldj.cpu() - ref["ldj"]).abs() / ref["ldj"].abs()).max().item()
    dp = abs(float(logp) - float(ref["logp"])) / abs(float(ref["logp"]))
    dx = (x.cpu() - ref["x"]).abs().max().item()
    db = (back - xd).abs().max().item()
    print(f"flow: z {dz:.2e}  ldj rel {dl:.2e}  logp rel {dp:.2e}  x = g(oracle fz) {dx:.2e}  g(f(x)) - x {db:.2e}")
    assert dz < 1e-5 and dl < 1e-5 and dp < 1e-5 and dx < 1e-5
    assert db < 2e-6


@pytest.mark.parametrize("B,N,R", [(2, 256, 4), (3, 250, 3)])
def test_split_path_and_graph_replay_are_bit_equal(nets, B, N, R):
    """pf_interp_weights + pf_flow_inv_interp return the bits of pf_interp + pf_flow_inv, and a captured graph those of eager."""
    _, net = nets[SEEDS[2]]
    xyz = synth_patches(B, N, seed=B * N).to(DEV)
    e = net._engine(4)
    try:
        e.split_interp = 0
        xa, la = net(xyz, R)
        xa, la = xa.clone(), la.clone()
        e.split_interp = 1
        xb, lb = net(xyz, R)
        assert torch.equal(xa, xb) and torch.equal(la, lb)
    finally:
        e.split_interp = 0
    run = net.graphed(B, N, R)
    xc, lc = run(xyz)
    assert torch.equal(xa, xc) and torch.equal(la, lc)
    print(f"({B}, {N}, R = {R}): split path and graph replay bit-equal to the fused eager forward")


def test_growth_activation_past_the_range_is_loud(nets, monkeypatch):
    """A cloud scaled by 1000: the CPU oracle's growth activations, times the 2^t they are stored with, pass fp16's 65504 - the
    interpolation weights come out non-finite (never finite and wrong), and with PF_CHECK_FINITE the forward raises."""
    import puflow_amd.interpflow as M
    sd, net = nets[SEEDS[0]]
    xyz = synth_patches(1, 256, seed=3)
    big = xyz * 1000.0
    from puflow_amd.packing import fold_state_dict, interp_exps
    exps = interp_exps(fold_state_dict(sd)["interp"])["g"]           # the growth blocks' exponents of the packed plan
    e = net._engine(4)
    idx16 = net.forward_stages(xyz.to(DEV), 4)["idx16"]                    # a uniform scale keeps the neighbour lists
    with torch.no_grad():
        nb = O.knn_gather(big, idx16[..., :8].cpu().long())
        xi = big.unsqueeze(2).expand_as(nb)
        f = torch.cat([xi, nb, nb - xi], dim=-1).permute(0, 3, 1, 2)
        stored = []
        for t in range(8):
            g = O._conv_bn_lrelu(sd, f"interp.knn_context.feat_conv.convs.{t}", f, 0.05)
            stored.append(float(g.abs().max()) * 2.0 ** exps[t])
            f = torch.cat([f, g], dim=1)
    print("stored growth maxima at scale 1000: " + " ".join(f"{v:.3g}" for v in stored))
    assert max(stored) > 65504.0
    aw = e.interp_weights(big.to(DEV).contiguous(), idx16.contiguous())
    ok = e.interp_weights(xyz.to(DEV).contiguous(), idx16.contiguous())
    assert not bool(torch.isfinite(aw).all())
    assert bool(torch.isfinite(ok).all())
    monkeypatch.setattr(M, "_CHECK_FINITE", True)
    with pytest.raises(M._lib.PuflowHipError):
        net(big.to(DEV), 4)

