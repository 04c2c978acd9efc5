"""The next unit's P|Q vectors from inside the producing EdgeConv launch (pf_edgeconv_pq, csrc/edgeconv.hip), interleaved with
the tile loop (fuse = 1, pqf_gemm) and as the launch's TAIL phase (fuse = 2, pq_tail): the bits of the two-launch path (fuse = 0:
the EdgeConv kernel, then pointwise.hip pq_gemm_kernel; all three forms walk tiles around the one product of csrc/pf_pq.h), for
the three kernel instantiations (unit 0, unit 1, units 2 - 4) at the smallest shapes that reach each corner of the tile walks:
  (3, 24)      T = 72 is no multiple of 16, batch items straddle a tile, and there are fewer tiles than workgroups: most
               workgroups reach the tail, or the flush behind the loop, with an empty tile list
  (1, 272)     17 tiles: workgroups with one tile and with none, a partial staging round / a partial flush
  (17, 2048)   2 176 tiles: 8 or 9 per workgroup of the 128-channel kernel - more than one staging round, the second one partial,
               and holes in the XCD-aware tile walk; fuse = 1 is forced here (the size policy leaves it at 16 384 points)
Needs a real MI355X:  python -m pytest tests -m gpu"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from puflow_amd.packing import FEAT_CHANNELS
from puflow_amd.weights import synth_patches, synth_state_dict

DEV = "cuda:0"
SHAPES = [(3, 24), (1, 272), (17, 2048)]


@pytest.fixture(scope="module")
def net():
    from puflow_amd import _lib
    from puflow_amd.interpflow import PointInterpFlow
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _lib.load()                          # raises if the HIP library is missing: no silent fallback
    n = PointInterpFlow(3)
    n.load_state_dict(synth_state_dict(8))
    n.set_to_initialized_state()
    return n.to(DEV).eval()


def _unit(e, u, src, idx16, B, N, fuse):
    """pf_edgeconv_pq of unit u into NaN-poisoned buffers -> (out [T, odim], pq_next [T, rows])"""
    T = B * N
    rows = 256 if u == 0 else 512
    out = torch.full((T, FEAT_CHANNELS[u + 1]), float("nan"), device=DEV)
    nxt = torch.full((T, rows), float("nan"), device=DEV)
    w = e.ec1n_w[u] if u < 2 else e.ec4_w[u]
    rc = e.lib.pf_edgeconv_pq(u, src.data_ptr(), idx16.data_ptr(), e._p(w), out.data_ptr(), e.base, e.post[u], nxt.data_ptr(),
                              B, N, fuse, e._stream())
    assert rc == 0, (u, fuse, rc)
    return out, nxt


@pytest.fixture(scope="module")
def chain(net):
    """Per shape: the inputs of units 0, 1, 2 and their two-launch results (computed once, shared, never written again)."""
    e = net._engine(4)
    assert e.ec_mode == "f16n"
    memo = {}

    def get(B, N):
        if (B, N) not in memo:
            xyz = synth_patches(B, N, seed=B + N).to(DEV)
            idx16 = e.knn(xyz)
            src, units = xyz, []
            for u in range(3):
                out, nxt = _unit(e, u, src, idx16, B, N, 0)
                units.append((src, out, nxt))
                src = nxt
            torch.cuda.synchronize()
            memo[(B, N)] = (idx16, units)
        return memo[(B, N)]
    return get


@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("unit", [0, 1, 2])
@pytest.mark.parametrize("fuse", [1, 2])
def test_fused_forms_return_the_two_launch_bits(net, chain, fuse, unit, B, N):
    e = net._engine(4)
    idx16, units = chain(B, N)
    src, out0, nxt0 = units[unit]
    assert not torch.isnan(out0).any() and not torch.isnan(nxt0).any()       # the reference itself wrote every row
    out2, nxt2 = _unit(e, unit, src, idx16, B, N, fuse)
    torch.cuda.synchronize()
    assert torch.equal(out0, out2), "out"
    bad = (nxt0 != nxt2) | torch.isnan(nxt2)
    rows = torch.nonzero(bad.any(dim=1)).flatten()
    print(f"fuse {fuse} unit {unit} ({B}, {N}): pq_next rows that differ {rows.numel()} of {B * N}", rows[:8].tolist())
    assert torch.equal(nxt0, nxt2), "pq_next"


def test_fuse_value_out_of_range_is_refused(net, chain):
    e = net._engine(4)
    idx16, units = chain(3, 24)
    T = 72
    out = torch.zeros((T, 32), device=DEV)
    nxt = torch.zeros((T, 256), device=DEV)
    rc = e.lib.pf_edgeconv_pq(0, units[0][0].data_ptr(), idx16.data_ptr(), e._p(e.ec1n_w[0]), out.data_ptr(), e.base, e.post[0],
                              nxt.data_ptr(), 3, 24, 3, e._stream())
    assert rc != 0


def test_whole_forward_with_the_tail_form(net):
    """One forward at (2, 256) with every unit's P|Q product in its EdgeConv launch's tail, eagerly and from a captured graph:
    x and logp are the bits of the two-launch forward."""
    B, N, R = 2, 256, 4
    xyz = synth_patches(B, N, seed=B + N).to(DEV)
    e = net._engine(4)
    try:
        e.fuse_pq = 0
        x0, l0 = net(xyz, R)
        x0, l0 = x0.clone(), l0.clone()
        e.fuse_pq = 2
        x2, l2 = net(xyz, R)
        x2, l2 = x2.clone(), l2.clone()
        run = net.graphed(B, N, R)
        for _ in range(2):
            xg, lg = run(xyz)
        torch.cuda.synchronize()
    finally:
        e.fuse_pq = -1
    assert torch.isfinite(x0).all() and torch.isfinite(l0).all()
    assert torch.equal(x0, x2) and torch.equal(l0, l2)
    assert torch.equal(x0, xg) and torch.equal(l0, lg)
