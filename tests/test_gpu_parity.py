"""Parity of the HIP path (through the C ABI) against the CPU oracle and the committed golden
vectors.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as O
from puflow_amd.weights import synth_patches, synth_state_dict

DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from puflow_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _lib.load()          # raises if the HIP library is missing: no silent fallback


def _net(sd):
    from puflow_amd.interpflow import PointInterpFlow
    net = PointInterpFlow(3)
    net.load_state_dict(sd)
    net.set_to_initialized_state()
    return net.to(DEV).eval()


# ------------------------------------------------------------------------------------- kNN
@pytest.mark.parametrize("B,N,M,K", [(2, 256, 256, 16), (1, 2048, 2048, 16), (3, 100, 77, 8), (1, 65, 300, 4),
                                     (2, 130, 130, 32), (1, 16, 16, 16), (2, 1000, 5000, 16), (1, 3000, 2049, 8),
                                     (1, 257, 4096, 16), (8, 3072, 2048, 16), (32, 2048, 2048, 16), (4, 2048, 2048, 8),
                                     # >= 1024 workgroups and M <= 4096: the sweeps on the matrix pipe (knn5_kernel), K = 4 / 8 / 16,
                                     # M not a multiple of the 128-row table padding, N not a multiple of 64
                                     (16, 4096, 1024, 4), (17, 4000, 1100, 8), (9, 7300, 4096, 16),
                                     # 256 <= M < 1024 on small grids (the training step's 32 x 256): knn5_kernel as well
                                     (32, 256, 256, 16), (32, 256, 256, 8), (70, 130, 300, 8), (40, 200, 999, 4),
                                     # between 256 and 512 query strips of 128: knn5_kernel with 8 waves, K = 4 / 8
                                     (33, 1000, 1100, 4), (33, 1000, 1100, 8)])
def test_knn_bit_exact(lib, B, N, M, K):
    """The two-sweep kernel splits the references over 16 / 8 waves for grids of < 384 / < 1024 workgroups; larger grids run
    its sweeps as f32 MFMAs (knn5_kernel; knn4_kernel with 4 waves when M > 4096).  The shapes above exercise all of them,
    with the same results."""
    from puflow_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + N + K)
    p1 = torch.rand(B, N, 3, generator=g) * 2 - 1
    p2 = p1.clone() if N == M else torch.rand(B, M, 3, generator=g) * 2 - 1
    d_ref, i_ref = O.knn_canonical(p1, p2, K)
    d, i, _ = ops.knn_points(p1.to(DEV), p2.to(DEV), K)
    assert torch.equal(i.cpu(), i_ref)                       # indices bit-exact
    assert torch.equal(d.cpu(), d_ref)                       # distances bit-exact (unfused fp32)


def test_knn_any_k(lib):
    """K outside the register-resident set {4, 8, 16, 32} goes through the sort-based kernel, same order."""
    from puflow_amd import ops
    p = synth_patches(2, 500, seed=4, surface=False)
    for K in (1, 5, 20, 100):
        d_ref, i_ref = O.knn_canonical(p, p, K)
        d, i, _ = ops.knn_points(p.to(DEV), p.to(DEV), K)
        assert torch.equal(i.cpu(), i_ref) and torch.equal(d.cpu(), d_ref)


def test_knn_ties_and_duplicates(lib):
    from puflow_amd import ops
    p = synth_patches(1, 128, seed=3, surface=False)
    p[0, 10] = p[0, 3]; p[0, 50] = p[0, 3]; p[0, 77] = p[0, 76]      # exact duplicates
    p[0, 100:110] = torch.round(p[0, 100:110] * 4) / 4                # lattice points: many equal distances
    d_ref, i_ref = O.knn_canonical(p, p, 16)
    d, i, _ = ops.knn_points(p.to(DEV), p.to(DEV), 16)
    assert torch.equal(i.cpu(), i_ref)
    assert i[0, 3, 0] == 3 and i[0, 3, 1] == 10 and i[0, 3, 2] == 50  # (dist, idx) order on ties


@pytest.mark.parametrize("mode", ["lattice", "identical", "clusters"])
def test_knn_heavy_ties_two_sweep_kernel(lib, mode):
    """M >= 256 takes the two-sweep kernel; heavy ties overflow its candidate lists -> exact fallback."""
    from puflow_amd import ops
    g = torch.Generator().manual_seed(5)
    if mode == "lattice":
        p = torch.round(torch.rand(2, 600, 3, generator=g) * 4) / 4          # 5^3 lattice sites, many duplicates
    elif mode == "identical":
        p = torch.full((1, 300, 3), 0.25)
    else:
        c = torch.rand(1, 8, 3, generator=g)
        p = c[:, torch.randint(0, 8, (700,), generator=g)] + 0.001 * torch.rand(1, 700, 3, generator=g)
        p[0, 100:200] = p[0, 0]                                               # 101 exact copies of one point
    for K in (8, 16):
        d_ref, i_ref = O.knn_canonical(p, p, K)
        d, i, _ = ops.knn_points(p.to(DEV), p.to(DEV), K)
        assert torch.equal(i.cpu(), i_ref) and torch.equal(d.cpu(), d_ref)


@pytest.mark.parametrize("mode", ["offset", "far_offset", "tiny", "huge", "lattice", "clusters", "line"])
def test_knn_two_sweep_kernel_on_hard_clouds(lib, mode):
    """M >= 1024 runs knn4_kernel (threshold sweep, candidate lists, per-slice top K, 4-way merge of the slices): clouds far
    from the origin, tiny / huge scales, lattices and duplicate clusters (ties at the K-th distance, list overflow -> exact
    path), collinear points must give the oracle's result bit for bit."""
    from puflow_amd import ops
    g = torch.Generator().manual_seed(11)
    B, M = 2, 1536
    p = torch.rand(B, M, 3, generator=g) * 2 - 1
    if mode == "offset":
        p = p + torch.tensor([3.0, -2.0, 5.0])
    elif mode == "far_offset":
        p = p * 0.05 + torch.tensor([100.0, 250.0, -80.0])
    elif mode == "tiny":
        p = p * 1e-4
    elif mode == "huge":
        p = p * 3e4
    elif mode == "lattice":
        p = torch.round(p * 6) / 6                                           # 13^3 sites for 1536 points: many exact ties
    elif mode == "clusters":
        c = torch.rand(B, 40, 3, generator=g)
        p = c[:, torch.randint(0, 40, (M,), generator=g)] + 1e-3 * torch.rand(B, M, 3, generator=g)
        p[0, 200:260] = p[0, 0]                                              # 61 exact copies of one point
    elif mode == "line":
        t = torch.rand(B, M, 1, generator=g)
        p = t * torch.tensor([1.0, 2.0, -0.5]) + 0.25
    q = p[:, :700].contiguous()
    for K in (4, 8, 16):
        d_ref, i_ref = O.knn_canonical(q, p, K)
        i, d = ops.knn_idx32(q.to(DEV), p.to(DEV), K, want_dist=True)
        assert torch.equal(i.cpu().long(), i_ref) and torch.equal(d.cpu(), d_ref), (mode, K)
    # and with enough workgroups for the 4-slice variant (its per-slice top K + merge): B x ceil(N / 64) >= 1024
    pb = p[:1].repeat(24, 1, 1) + torch.arange(24).view(24, 1, 1) * (0.37 if mode != "huge" else 37.0)
    pb = pb[:, torch.randperm(M, generator=g)].contiguous() if mode in ("lattice", "clusters") else pb
    qb = torch.cat([pb, pb[:, :1536]], dim=1)[:, :2752].contiguous()          # 24 x 43 workgroups = 1032
    d_ref, i_ref = O.knn_canonical(qb, pb, 16)
    i, d = ops.knn_idx32(qb.to(DEV), pb.to(DEV), 16, want_dist=True)
    assert torch.equal(i.cpu().long(), i_ref) and torch.equal(d.cpu(), d_ref), mode


def test_nn1_first_minimum(lib):
    from puflow_amd import _lib
    x = synth_patches(2, 300, seed=5, surface=False)
    y = synth_patches(2, 200, seed=6, surface=False)
    y[0, 7] = y[0, 2]
    d1, i1, d2, i2 = O.chamfer_nn(x, y)
    xd, yd = x.to(DEV), y.to(DEV)
    dist = torch.empty(2, 300, device=DEV); idx = torch.empty(2, 300, dtype=torch.int32, device=DEV)
    _lib.check(lib.pf_nn1(xd.data_ptr(), yd.data_ptr(), 2, 300, 200, dist.data_ptr(), idx.data_ptr(), None))
    assert torch.equal(dist.cpu(), d1) and torch.equal(idx.cpu().long(), i1)


# --------------------------------------------------------------------------- stage parity
def _check_stages(st, ref, atol=1e-5):
    assert torch.equal(st["idx16"].cpu().long(), ref["idx16"])
    for i in range(6):
        assert (st["cs"][i].cpu() - ref["cs"][i]).abs().max() < atol, f"cs[{i}]"
    assert (st["z"].cpu() - ref["z"]).abs().max() < atol
    assert ((st["ldj"].cpu() - ref["ldj"]).abs() / ref["ldj"].abs()).max() < 1e-5     # relative: |ldj| ~ 1e3..1e4
    assert abs(float(st["logp"]) - float(ref["logp"])) / abs(float(ref["logp"])) < 1e-5
    assert (st["fz"].cpu() - ref["fz"]).abs().max() < atol
    assert (st["x"].cpu() - ref["x"]).abs().max() < atol                               # north_star: xyz within 1e-5


@pytest.mark.parametrize("wseed,dseed,B,N,surface", [(0, 0, 2, 256, True), (1, 1, 1, 256, False), (2, 9, 3, 512, True),
                                                     (3, 4, 1, 200, True), (4, 2, 5, 61, False)])
def test_forward_stages_match_oracle(lib, wseed, dseed, B, N, surface):
    sd = synth_state_dict(wseed)
    xyz = synth_patches(B, N, seed=dseed, surface=surface)
    ref = O.forward(sd, xyz, 4, stages=True)
    st = _net(sd).forward_stages(xyz.to(DEV), 4)
    _check_stages(st, ref)


@pytest.mark.parametrize("name", ["n256_s0", "n256_s1", "n2048_s1"])
def test_forward_matches_reference_golden(lib, golden_dir, name):
    """HIP output against what the REFERENCE's own Python produced (tools/make_golden.py)."""
    g = np.load(os.path.join(golden_dir, f"forward_{name}.npz"))
    sd = synth_state_dict(int(g["meta_wseed"]))
    xyz = synth_patches(int(g["meta_B"]), int(g["meta_N"]), seed=int(g["meta_dseed"]), surface=bool(g["meta_surface"]))
    net = _net(sd)
    st = net.forward_stages(xyz.to(DEV), 4)
    assert np.array_equal(st["idx16"].cpu().numpy().astype(np.int64), g["idx16"].astype(np.int64))
    np.testing.assert_allclose(st["x"].cpu().numpy(), g["x"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(st["z"].cpu().numpy(), g["z"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(st["fz"].cpu().numpy(), g["fz"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(st["ldj"].cpu().numpy(), g["ldj"], rtol=1e-5)
    np.testing.assert_allclose(float(st["logp"]), float(g["logp"]), rtol=1e-5)
    for i in range(6):
        n = g[f"cs{i}"].shape[1]
        np.testing.assert_allclose(st["cs"][i].cpu().numpy()[:, :n], g[f"cs{i}"], rtol=0, atol=1e-5)
    x, logp = net(xyz.to(DEV), 4)                         # plain forward == staged forward, bit for bit
    assert torch.equal(x, st["x"]) and torch.equal(logp, st["logp"])


@pytest.mark.parametrize("case", ["a", "b"])
def test_forward_matches_reference_with_pretrained_weights(lib, pretrained_pu1k, case):
    """HIP output against the REFERENCE's own Python running its own TRAINED checkpoint (pretrain/puflow-x4-pu1k.pt;
    tools/make_golden_pretrained.py): trained-scale activations (|cs| up to 480) through the split-fp16 kernels.
    The contract quantities hold their bars: kNN indices bit-exact, x within 1e-5, log-det / log-likelihood within 1e-5
    relative, the conditioning features within 2e-6 of their scale.  The LATENT z is a different matter with trained weights:
    the reference's own fp32 z is 2.5e-4 (case a) and 3.2e-4 (case b) from a float64 evaluation of the same network, 1.1e-4 and
    1.7e-4 of it from the flow's own arithmetic on exact features, while x, which g computes back with the same cs, is within
    4e-6 (tests/test_infer_ref.py::test_trained_checkpoint_conditioning_figures pins these figures and that the golden z is as
    far from float64 as the oracle's).  So any fp32 evaluation in another summation order, the f32-MFMA mode included, differs
    from the reference's z by a few 1e-4 and this test can only bound it at 2e-3; the bar that means something for the latent is
    the one against float64 in tests/test_gpu_infer_anchor.py::test_forward_end_to_end."""
    g = pretrained_pu1k
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g if k.startswith("sd/")}
    B, N, seed = (int(v) for v in g[f"{case}/meta"])
    xyz = synth_patches(B, N, seed=seed, surface=True)
    net = _net(sd)
    for mode in ("f16n", "f32") if case == "a" else ("f16n",):
        net.ec_mode = mode
        st = net.forward_stages(xyz.to(DEV), 4)
        assert np.array_equal(st["idx16"].cpu().numpy().astype(np.int64), g[f"{case}/idx16"].astype(np.int64))
        np.testing.assert_allclose(st["x"].cpu().numpy(), g[f"{case}/x"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(st["ldj"].cpu().numpy(), g[f"{case}/ldj"], rtol=1e-5)
        np.testing.assert_allclose(float(st["logp"]), float(g[f"{case}/logp"]), rtol=1e-5)
        for i in (0, 5):
            ref = g[f"{case}/cs{i}"]
            got = st["cs"][i].cpu().numpy()[..., :ref.shape[-1]]
            assert np.abs(got - ref).max() <= 2e-6 * np.abs(ref).max(), i
        np.testing.assert_allclose(st["z"].cpu().numpy(), g[f"{case}/z"], rtol=0, atol=2e-3)      # ill-conditioned: see above
        np.testing.assert_allclose(st["fz"].cpu().numpy(), g[f"{case}/fz"], rtol=0, atol=2e-3)


def test_edgeconv_arithmetic_modes(lib):
    """Both EdgeConv arithmetic modes meet the parity bar - split-fp16 with a natural-scale low half (the product) and the
    bit-exact f32 MFMA kernel (the in-library A/B reference) - and agree with each other to fp32 rounding; the removed
    round-1 generations are refused, not silently mapped."""
    sd = synth_state_dict(12)
    xyz = synth_patches(2, 512, seed=13)
    ref = O.forward(sd, xyz, 4, stages=True)
    net = _net(sd)
    outs = {}
    for mode in ("f16n", "f32"):
        net.ec_mode = mode                                   # re-packs the plan (the P|Q row scales depend on the mode)
        assert net._engine(4).ec_mode == mode
        st = net.forward_stages(xyz.to(DEV), 4)
        _check_stages(st, ref)
        outs[mode] = st
    assert (outs["f32"]["x"] - outs["f16n"]["x"]).abs().max() < 5e-6
    assert (outs["f32"]["cs"][5] - outs["f16n"]["cs"][5]).abs().max() < 5e-6
    net.ec_mode = "bf16x3"
    with pytest.raises(ValueError):
        net._engine(4)
    net.ec_mode = None
    h = torch.empty(8, 128, device=DEV)
    for cfg in (3, 4, 5, 6):                                 # the C ABI says so too
        assert lib.pf_edgeconv(cfg, h.data_ptr(), None, h.data_ptr(), h.data_ptr(), h.data_ptr(), 1, 16, None) != 0


@pytest.mark.parametrize("seed", [3, 5])
def test_trained_style_dynamic_range(lib, seed):
    """Weights with the wide dynamic range of the reference's pretrained checkpoints (features up to |h| ~ 300,
    BN variances ~1e3; statistics taken from pretrain/puflow-x4-pu1k.pt), calibrated on data by the oracle:
    xyz still within 1e-5 absolute, log-det within 1e-5 relative, features within 1e-5 of their range - in every
    EdgeConv arithmetic mode."""
    sd = O.calibrate(synth_state_dict(seed, style="trained"), synth_patches(4, 256, seed=1))
    xyz = synth_patches(2, 256, seed=2)
    ref = O.forward(sd, xyz, 4, stages=True)
    assert max(h.abs().max() for h in ref["hs"]) > 100          # the regime this test is about
    net = _net(sd)
    for mode in ("f16n", "f32"):
        net.ec_mode = mode
        assert net._engine(4).ec_mode == mode
        st = net.forward_stages(xyz.to(DEV), 4)
        assert torch.equal(st["idx16"].cpu().long(), ref["idx16"])
        assert (st["x"].cpu() - ref["x"]).abs().max() < 1e-5
        assert ((st["ldj"].cpu() - ref["ldj"]).abs() / ref["ldj"].abs()).max() < 1e-5
        assert (st["z"].cpu() - ref["z"]).abs().max() < 1e-5 * max(1.0, float(ref["z"].abs().max()))
        for i in range(6):
            assert (st["cs"][i].cpu() - ref["cs"][i]).abs().max() < 1e-5 * max(1.0, float(ref["cs"][i].abs().max())), (mode, i)


@pytest.mark.parametrize("R", [1, 2, 3, 5, 8, 16, 32])
def test_other_upsampling_ratios(lib, R):
    """--up_ratio other than 4: R <= 4 runs the 4-row fast path of the interpolation kernel, larger ratios all r_max = 32
    rows of the weight unit's last conv (interpflow.py:142,180); the packed plan is the same for every R."""
    sd = synth_state_dict(6)
    xyz = synth_patches(2, 256, seed=3)
    ref = O.forward(sd, xyz, R, stages=True)
    x, logp = _net(sd)(xyz.to(DEV), R)
    assert tuple(x.shape) == (2, 256 * R, 3)
    assert (x.cpu() - ref["x"]).abs().max() < 1e-5
    assert abs(float(logp) - float(ref["logp"])) / abs(float(ref["logp"])) < 1e-5


def test_reference_method_surface(lib):
    """feat_extract / f / log_prob / g / sample called the way the reference's callers do."""
    from puflow_amd import ops
    sd = synth_state_dict(7)
    xyz = synth_patches(2, 256, seed=8)
    ref = O.forward(sd, xyz, 4, stages=True)
    net = _net(sd)
    xd = xyz.to(DEV)
    _, knn_idx, _ = ops.knn_points(xd, xd, K=16, return_nn=False, return_sorted=False)
    assert knn_idx.dtype == torch.int64
    cs = net.feat_extract(xd, knn_idx)
    assert len(cs) == 6 and tuple(cs[5].shape) == (2, 256, 128)
    z, ldj = net.f(xd, cs)
    z2, logp = net.log_prob(xd, cs)
    assert torch.equal(z, z2)
    assert (z.cpu() - ref["z"]).abs().max() < 1e-5
    x = net.g(ref["fz"].to(DEV), cs, 4)
    assert (x.cpu() - ref["x"]).abs().max() < 1e-5
    assert (net.sample(xd, 4).cpu() - ref["x"]).abs().max() < 1e-5
    # exact invertibility of the flow: g(f(x)) with one replica returns x
    back = net.g(z.unsqueeze(-1), cs, 1)
    assert (back - xd).abs().max() < 2e-6
    g = ops.knn_gather(xd, knn_idx)
    assert torch.equal(g.cpu(), O.knn_gather(xyz, ref["idx16"]))


@pytest.mark.parametrize("B,N", [(1, 4096), (7, 333), (64, 256)])
def test_other_batch_shapes(lib, B, N):
    """Shapes off the benchmark point: one big patch, ragged sizes (no multiple of any tile), the CLI's 64 x 256."""
    sd = synth_state_dict(31)
    xyz = synth_patches(B, N, seed=B + N)
    net = _net(sd)
    x, logp = net(xyz.to(DEV), 4)
    nb = min(B, 3)
    ref = O.forward(sd, xyz[:nb], 4, stages=True)
    assert (x[:nb].cpu() - ref["x"]).abs().max() < 1e-5
    xs, _ = net(xyz[:nb].to(DEV).contiguous(), 4)                 # batch items are independent
    assert torch.equal(xs, x[:nb])
    st = net.forward_stages(xyz.to(DEV), 4)
    assert ((st["ldj"][:nb].cpu() - ref["ldj"]).abs() / ref["ldj"].abs()).max() < 1e-5


# ------------------------------------------------------------------- full-size properties
def test_full_size_properties(lib):
    """BASELINE config 2 shape (32 x 2048): size-independent properties + oracle on a slice."""
    sd = synth_state_dict(2021)
    xyz = synth_patches(32, 2048, seed=2021)
    net = _net(sd)
    xd = xyz.to(DEV)
    st = net.forward_stages(xd, 4)
    x, z = st["x"], st["z"]
    assert tuple(x.shape) == (32, 8192, 3) and torch.isfinite(x).all() and torch.isfinite(st["logp"])
    # self is the nearest neighbour; neighbour lists are sorted by distance
    idx = st["idx16"].long()
    assert torch.equal(idx[..., 0], torch.arange(2048, device=DEV).expand(32, -1))
    nb = xd[torch.arange(32, device=DEV).view(32, 1, 1), idx]
    d = ((nb - xd.unsqueeze(2)) ** 2).sum(-1)
    assert (d[..., 1:] >= d[..., :-1] - 1e-7).all()
    # flow invertibility at full size
    cs = net.feat_extract(xd, idx)
    back = net.g(z.unsqueeze(-1), cs, 1)
    assert (back - xd).abs().max() < 2e-6
    # patches are independent: a batch item alone gives the same bits
    xs, _ = net(xd[5:6].contiguous(), 4)
    assert torch.equal(xs[0], x[5])
    # interpolated latents are convex combinations of neighbour latents
    zn = z[torch.arange(32, device=DEV).view(32, 1, 1), idx[..., :8]]        # [B,N,8,3]
    fz = st["fz"]                                                            # [B,N,3,R]
    assert (fz <= zn.max(2)[0].unsqueeze(-1) + 1e-5).all() and (fz >= zn.min(2)[0].unsqueeze(-1) - 1e-5).all()
    # oracle on two batch items
    ref = O.forward(sd, xyz[3:5], 4, stages=True)
    assert (x[3:5].cpu() - ref["x"]).abs().max() < 1e-5
    assert ((st["ldj"][3:5].cpu() - ref["ldj"]).abs() / ref["ldj"].abs()).max() < 1e-5


def test_fp16_range_violation_is_loud(lib, monkeypatch):
    """The split-fp16 kernels need |activation| < 65504.  A grossly un-normalised input must not produce a plausible
    finite cloud: the output is non-finite, and with PF_CHECK_FINITE the forward raises."""
    import puflow_amd.interpflow as M
    sd = synth_state_dict(3)
    net = _net(sd)
    xyz = synth_patches(1, 256, seed=3).to(DEV) * 1e7
    x, _ = net(xyz, 4)
    assert not bool(torch.isfinite(x).all())
    monkeypatch.setattr(M, "_CHECK_FINITE", True)
    with pytest.raises(M._lib.PuflowHipError):
        net(xyz, 4)
    x_ok, _ = net(synth_patches(1, 256, seed=3).to(DEV), 4)          # the same net on a normalised patch is fine
    assert bool(torch.isfinite(x_ok).all())


def test_graphed_forward_is_bit_identical(lib):
    """hipGraph replay of the eval forward (one launch per step) returns the eager path's bits, for fresh inputs too."""
    sd = synth_state_dict(17)
    net = _net(sd)
    run = net.graphed(3, 256, 4)
    for seed in (1, 2):
        xyz = synth_patches(3, 256, seed=seed).to(DEV)
        x_e, lp_e = net(xyz, 4)
        x_g, lp_g = run(xyz)
        assert torch.equal(x_g, x_e) and torch.equal(lp_g, lp_e)
    with pytest.raises(ValueError):
        run(synth_patches(2, 256, seed=1).to(DEV))
    # zero-copy hand-over: the producer writes into the graph's own input buffer
    xyz = synth_patches(3, 256, seed=5).to(DEV)
    x_e, lp_e = net(xyz, 4)
    assert tuple(run.input.shape) == (3, 256, 3)
    run.input.copy_(xyz)
    x_g, lp_g = run(run.input)
    assert torch.equal(x_g, x_e) and torch.equal(lp_g, lp_e)
    x_g, lp_g = run(synth_patches(3, 256, seed=1).to(DEV))           # and a foreign tensor is still copied in
    assert torch.equal(x_g, net(synth_patches(3, 256, seed=1).to(DEV), 4)[0])


def test_graphed_forward_is_pinned_to_its_plan(lib):
    """The captured graph bakes pointers into the packed weight blob: it must keep that blob alive across eval() /
    train() toggles and allocator churn, replay bit-identically, and refuse to replay once the weights changed."""
    sd = synth_state_dict(21)
    xyz = synth_patches(2, 256, seed=22).to(DEV)
    net = _net(sd)
    x0, l0 = net(xyz, 4)
    x0, l0 = x0.clone(), l0.clone()
    run = net.graphed(2, 256, 4)
    x1, l1 = run(xyz)
    assert torch.equal(x1, x0) and torch.equal(l1, l0)
    net.eval()                                             # used to drop the engine the graph points into
    junk = [torch.randn(1 << 20, device=DEV) for _ in range(8)]      # allocator churn over any freed blob
    del junk
    torch.cuda.empty_cache()
    x2, l2 = run(xyz)
    assert torch.equal(x2, x0) and torch.equal(l2, l0)
    e_before = net._engine(4)
    net.train(); net.eval()                                # mode toggles alone do not re-pack
    assert net._engine(4) is e_before
    with torch.no_grad():
        net.flow_blocks[0].actnorm.bias.add_(0.25)         # in-place weight update while in eval mode after a train() phase
    net.train(); net.eval()
    from puflow_amd._lib import PuflowHipError
    with pytest.raises(PuflowHipError):
        run(xyz)                                           # stale capture: loud, not a silent replay of old weights
    x3, _ = net(xyz, 4)
    assert not torch.equal(x3, x0)                         # the eager path picked the new weights up
    run2 = net.graphed(2, 256, 4)
    assert torch.equal(run2(xyz)[0], x3)
    net.load_state_dict(sd)
    with pytest.raises(PuflowHipError):
        run2(xyz)


def test_data_rebind_invalidates_the_plan(lib):
    """`p.data = new_tensor` changes a parameter's address without bumping its version counter: the plan signature compares
    addresses on every use, so the next eval forward re-packs instead of silently keeping the old weights."""
    sd = synth_state_dict(21)
    xyz = synth_patches(2, 256, seed=22).to(DEV)
    net = _net(sd)
    x0, _ = net(xyz, 4)
    x0 = x0.clone()
    p = net.flow_blocks[0].actnorm.bias
    v = p._version
    p.data = p.data.clone() + 0.25
    assert p._version == v                                  # the rebind is invisible to version counters
    x1, _ = net(xyz, 4)
    assert not torch.equal(x1, x0)
    sd2 = {k: t.clone() for k, t in sd.items()}
    sd2["flow_blocks.0.actnorm.bias"] = sd2["flow_blocks.0.actnorm.bias"] + 0.25
    xr, _ = O.forward(sd2, xyz.cpu(), 4)
    assert (x1.cpu() - xr).abs().max() < 1e-5


def test_logp_reduction_in_the_flow_kernel_is_deterministic(lib):
    """Flow f and the log-likelihood run as ONE launch (the workgroup that finishes last reduces the wave tiles' sums in a
    fixed order): whichever workgroup that is, per-item log-dets and logp are bit-identical from run to run, at a shape with
    many workgroups and at one with a single tile; ragged N (not a multiple of 16) takes the two-launch path."""
    sd = synth_state_dict(4)
    net = _net(sd)
    for B, N in ((16, 2048), (1, 64), (3, 250)):
        xyz = synth_patches(B, N, seed=B).to(DEV)
        ref = O.forward(sd, xyz.cpu(), 4, stages=True) if B * N <= 4096 else None
        outs = [net.forward_stages(xyz, 4) for _ in range(4)]
        for o in outs[1:]:
            assert torch.equal(o["ldj"], outs[0]["ldj"]) and torch.equal(o["logp"], outs[0]["logp"])
        if ref is not None:
            assert ((outs[0]["ldj"].cpu() - ref["ldj"]).abs() / ref["ldj"].abs()).max() < 1e-5
            assert abs(float(outs[0]["logp"]) - float(ref["logp"])) / abs(float(ref["logp"])) < 1e-5


@pytest.mark.parametrize("B,N", [(4, 2048), (2, 250), (1, 64), (3, 1000)])
def test_fused_pq_epilogue_is_bit_identical(lib, B, N):
    """pf_edgeconv_pq: the next unit's P|Q vectors computed inside the EdgeConv launch (small batches: one 16-point workgroup
    tile = one MFMA column tile) against the two-kernel path - every stage output bit-identical, ragged tails included."""
    sd = synth_state_dict(8)
    net = _net(sd)
    xyz = synth_patches(B, N, seed=B + N).to(DEV)
    e = net._engine(4)
    e.fuse_pq = 0
    a = net.forward_stages(xyz, 4)
    e.fuse_pq = 1
    b = net.forward_stages(xyz, 4)
    e.fuse_pq = -1
    for k in ("x", "z", "ldj", "logp", "cp", "st"):
        assert torch.equal(a[k], b[k]), k
    for i in range(6):
        assert torch.equal(a["cs"][i], b["cs"][i]), i
    if B * N <= 4096:
        _check_stages(b, O.forward(sd, xyz.cpu(), 4, stages=True))


@pytest.mark.parametrize("B,N,R", [(4, 2048, 4), (2, 250, 3), (1, 64, 1), (3, 1000, 2)])
def test_split_interpolation_branch_is_bit_identical(lib, B, N, R):
    """Small batches: the interpolation weights on a side stream beside the feature chain (pf_interp_weights) and the weighted
    latent sum inside the flow-g kernel (pf_flow_inv_interp) - the bits of the fused pf_interp + pf_flow_inv, eagerly and from
    a captured graph (where the side stream is a parallel branch)."""
    sd = synth_state_dict(9)
    net = _net(sd)
    xyz = synth_patches(B, N, seed=B * N).to(DEV)
    e = net._engine(4)
    e.split_interp = 0
    xa, la = net(xyz, R)
    xa, la = xa.clone(), la.clone()
    e.split_interp = 1
    xb, lb = net(xyz, R)
    assert torch.equal(xa, xb) and torch.equal(la, lb)
    run = net.graphed(B, N, R)
    for _ in range(3):
        xc, lc = run(xyz)
    assert torch.equal(xa, xc) and torch.equal(la, lc)
    e.split_interp = 0
    if B * N <= 4096:
        ref = O.forward(sd, xyz.cpu(), R)
        assert (xb.cpu() - ref[0]).abs().max() < 1e-5
