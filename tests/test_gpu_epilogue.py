"""The layer epilogue of the fused inference kernels (csrc/pf_mfma.h pf_act_pairn: rescale, LeakyReLU, hi / lo split, one fp32
value at a time) leaves the bits of the 4-vector sequence it replaces, and the edge-table products issued as one MFMA
(pf_edge_operand / pf_mm1, packing._etab_frag1) keep the kernels that use them at the parity bar.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as O
from puflow_amd.weights import synth_patches, synth_state_dict

DEV = "cuda:0"
N_VALUES = 4096
INVS = (1.0, 2.0 ** -13, 2.0 ** -7)          # no rescale, and the two extremes of the power-of-two weight scales in use
SLOPES = (0.0, 0.01, 0.05)


@pytest.fixture(scope="module")
def lib():
    from puflow_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _lib.load()


def _values():
    """4096 fp32 inputs, the same for every (inv, slope): the special values of every inv first, random magnitudes after."""
    v = [0.0, -0.0, float("inf"), float("-inf")]
    tiny = np.float32(2.0 ** -149)
    for k in (1, 2, 3, 1000, 2 ** 22, 2 ** 23 - 1):                       # fp32 subnormals
        v += [float(k * tiny), -float(k * tiny)]
    v += [2.0 ** -126, -(2.0 ** -126), 1.5 * 2.0 ** -126, -1.5 * 2.0 ** -126]    # the smallest normals
    for e in (-40, -30, -26, -25, -24):                                    # both signs around 0, below fp16's subnormal range
        v += [2.0 ** e, -(2.0 ** e), 1.2345 * 2.0 ** e, -1.2345 * 2.0 ** e]
    for inv in INVS:
        s = 1.0 / inv
        for e in range(-25, -13):                                          # scaled result is an fp16 subnormal (or its edge)
            for m in (1.0, 1.0009765625, 1.5, 1.999):
                v += [m * 2.0 ** e * s, -m * 2.0 ** e * s]
        for m in (65504.0, 65503.99, 65519.99, 65520.0, 65536.0):          # fp16 max, the rounding boundary to inf, beyond
            v += [m * s, -m * s]
        for slope in SLOPES[1:]:                                           # negative inputs that land there after the slope
            v += [-65504.0 * s / slope, -(2.0 ** -20) * s / slope]
    v = np.asarray([x for x in v if abs(x) <= 3.4e38 or np.isinf(x)], dtype=np.float32)
    rng = np.random.default_rng(2021)
    n = N_VALUES - v.size
    assert n > 2048
    r = rng.standard_normal(n) * np.exp2(rng.uniform(-30.0, 22.0, n))      # every exponent the kernels can meet, both signs
    out = np.concatenate([v, r.astype(np.float32)])
    rng.shuffle(out)                                                       # specials next to ordinary values inside a register pair
    return out


@pytest.fixture(scope="module")
def values():
    return torch.from_numpy(_values()).to(DEV)


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("inv", INVS)
def test_act_pairn_bits(lib, values, inv, slope):
    """pf_test_act_pairn runs pf_pairn(pf_lrelu(pf_scale(.))) and pf_act_pairn on the same registers: the packed-fp16 hi and lo
    operand images must be bit-equal (the sign of a zero and the payload of a NaN included)."""
    n = values.numel()
    assert n == N_VALUES
    img = [torch.full((n // 2,), 0x5A5A5A5A, dtype=torch.int32, device=DEV) for _ in range(4)]
    rc = lib.pf_test_act_pairn(values.data_ptr(), n, inv, slope, *[t.data_ptr() for t in img], None)
    assert rc == 0
    torch.cuda.synchronize()
    old_h, old_l, new_h, new_l = [t.cpu().numpy().view(np.uint16) for t in img]
    bad_h, bad_l = np.flatnonzero(old_h != new_h), np.flatnonzero(old_l != new_l)
    print(f"inv {inv:g} slope {slope:g}: hi mismatches {bad_h.size}, lo mismatches {bad_l.size} of {old_h.size}")
    assert bad_h.size == 0, (bad_h[:8], old_h[bad_h[:8]], new_h[bad_h[:8]])
    assert bad_l.size == 0, (bad_l[:8], old_l[bad_l[:8]], new_l[bad_l[:8]])
    # the images are not trivially equal: hi is the fp16 rounding of the activated value wherever that is finite
    x = values.cpu().numpy().astype(np.float64) * inv
    with np.errstate(invalid="ignore"):                  # inf * 0 with slope 0: not among the values checked below
        act = np.maximum(x, x * np.float64(np.float32(slope)))
    # word w of thread i holds values (8 i + 2 w, 8 i + 2 w + 1) in its low / high half: the flat uint16 order is the input order
    fin = np.isfinite(act) & (np.abs(act) < 65504.0) & (np.abs(act) > 2.0 ** -14)
    got = new_h.view(np.float16).astype(np.float64)
    assert np.all(np.abs(got[fin] - act[fin]) <= np.abs(act[fin]) * 2.0 ** -10)


def test_act_pairn_rejects_bad_arguments(lib, values):
    t = torch.zeros(8, dtype=torch.int32, device=DEV)
    p = t.data_ptr()
    assert lib.pf_test_act_pairn(values.data_ptr(), 12, 1.0, 0.05, p, p, p, p, None) != 0       # n % 8 != 0
    assert lib.pf_test_act_pairn(None, 8, 1.0, 0.05, p, p, p, p, None) != 0


# ------------------------------------------------------------------------------------- edge tables as one MFMA
@pytest.fixture(scope="module")
def net(lib):
    from puflow_amd.interpflow import PointInterpFlow
    sd = synth_state_dict(2021)
    n = PointInterpFlow(3)
    n.load_state_dict(sd)
    n.set_to_initialized_state()
    return sd, n.to(DEV).eval()


def _idx16(idx):
    """[B, N, K] neighbour lists -> the [B, N, 16] int32 table the kernels index (K = 8: the unused half repeats the first)"""
    if idx.shape[-1] < 16:
        idx = torch.cat([idx, idx], dim=-1)
    return idx.to(torch.int32).contiguous().to(DEV)


@pytest.mark.parametrize("B,N,R", [(1, 8, 4), (2, 24, 3), (1, 40, 4)])
def test_interp_with_one_mfma_edge_tables(net, B, N, R):
    """pf_interp alone - the smallest legal N, a ragged last tile, N % 16 != 0, R < 4 - against the oracle's interpolation
    module: the distance encoder's first layer, the EdgeConv pre-activations and the weight unit's bracket all come from
    one-MFMA table products."""
    sd, n = net
    xyz = synth_patches(B, N, seed=100 + N)
    z = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(N))
    _, idx8 = O.knn_canonical(xyz, xyz, 8)
    fz, _ = O.interp(sd, z, xyz, idx8, R)                                          # [B, N, 3, R]
    u = n._engine(4).interp(xyz.to(DEV), z.to(DEV), _idx16(idx8), R)               # [B, N R, 3], row n R + r
    torch.cuda.synchronize()
    err = (u.cpu().view(B, N, R, 3) - fz.permute(0, 1, 3, 2)).abs().max().item()
    print(f"pf_interp ({B}, {N}, R = {R}): max |u - oracle| {err:.3e}")
    assert err < 1e-5


@pytest.mark.parametrize("B,N", [(1, 16), (3, 40)])
def test_edgeconv_unit0_with_one_mfma_edge_table(net, B, N):
    """Unit 0 (C = 3: every pre-activation is a table product) through pf_edgeconv cfg 8 and through pf_edgeconv_pq with the
    P|Q GEMM fused in, against the oracle's EdgeConv unit; the fused launch returns the two-kernel path's bits."""
    sd, n = net
    e = n._engine(4)
    assert e.ec_mode == "f16n"
    xyz = synth_patches(B, N, seed=200 + N)
    _, idx = O.knn_canonical(xyz, xyz, 16)
    ref = O.edgeconv_unit(sd, "feat_convs.0", xyz, idx)                            # [B, N, 32]
    xd, idx16 = xyz.to(DEV), _idx16(idx)
    T, s = B * N, e._stream()
    h = [torch.full((T, 32), float("nan"), device=DEV) for _ in range(3)]
    pq = [torch.full((T, 512), float("nan"), device=DEV) for _ in range(2)]
    e._edgeconv(0, xd.data_ptr(), idx16, h[0], B, N, s)
    w = e._p(e.ec1n_w[0])
    for k, fuse in enumerate((0, 1)):
        rc = e.lib.pf_edgeconv_pq(0, xd.data_ptr(), idx16.data_ptr(), w, h[1 + k].data_ptr(), e.base, e.post[0], pq[k].data_ptr(),
                                  B, N, fuse, s)
        assert rc == 0
    torch.cuda.synchronize()
    for k, name in enumerate(("pf_edgeconv cfg 8", "pf_edgeconv_pq fuse 0", "pf_edgeconv_pq fuse 1")):
        err = (h[k].cpu().view(B, N, 32) - ref).abs().max().item()
        print(f"{name} ({B}, {N}): max |h - oracle| {err:.3e}")
        assert err < 1e-5, name
    assert torch.equal(h[0], h[1]) and torch.equal(h[1], h[2])
    n_pq = T * 2 * (16 * 4 + 64)                                                   # unit 1's P|Q vectors: [T, 256], densely packed
    assert torch.equal(pq[0].view(-1)[:n_pq], pq[1].view(-1)[:n_pq]) and not torch.isnan(pq[1].view(-1)[:n_pq]).any()
