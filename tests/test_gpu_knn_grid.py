"""pf_knn_grid / pf_knn_grid_ragged (csrc/knn_grid.hip) against pf_knn_large / pf_knn_large_ragged on the same inputs:
torch.equal on the indices AND on the squared distances, on the adversarial inputs of tests/knn_grid_ref.py (ties, duplicates,
degenerate boxes, far queries, offset coordinates, a cloud above the brute-force kernel's 16 384-reference chunk)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import knn_grid_ref as R

DEV = "cuda:0"
CASES = R.cases()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _equal(got, want):
    return torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_grid_search_equals_the_brute_force_kernel(name):
    from puflow_amd import ops
    ref, query, ks = CASES[name]
    ref_d, query_d = _dev(ref)[None], _dev(query)[None]
    for K in ks:
        want = ops.knn_large(ref_d, query_d, K)
        got = ops.knn_grid(ref_d, query_d, K)
        assert got[0].shape == (1, query.shape[0], K) and got[0].dtype == torch.int32 and got[1].dtype == torch.float32
        assert _equal(got, want), (name, K)


def test_against_numpy_brute_force():
    """the cube, K = 8: both kernels against np.float32 unfused d2 and np.lexsort((idx, d2))"""
    from puflow_amd import ops
    ref, query, _ = CASES["cube"]
    want_i, want_d = R.brute(ref, query, 8)
    idx, d2 = ops.knn_grid(_dev(ref)[None], _dev(query)[None], 8)
    assert np.array_equal(idx[0].cpu().numpy(), want_i)
    assert np.array_equal(d2[0].cpu().numpy().view(np.uint32), want_d.view(np.uint32))
    assert not d2[0, :300, 0].any() and torch.equal(idx[0, :300, 0].cpu(), torch.arange(300, dtype=torch.int32))


def test_dense_batch_gives_every_cloud_its_own_result():
    from puflow_amd import ops
    ref, query, _ = CASES["cube"]
    refs = torch.stack([_dev(ref), _dev(ref).flip(0) * 2 + 1, _dev(CASES["plane"][0][:300])])
    queries = torch.stack([_dev(query), _dev(query) * 2 + 1, _dev(query)])
    got, want = ops.knn_grid(refs, queries, 8), ops.knn_large(refs, queries, 8)
    assert _equal(got, want)
    for b in range(3):
        alone = ops.knn_grid(refs[b:b + 1], queries[b:b + 1], 8)
        assert torch.equal(alone[0][0], got[0][b]) and torch.equal(alone[1][0], got[1][b])


def test_ragged_equals_the_dense_call_on_each_cloud_alone():
    """clouds of 64, 300 and 5000 references with different query counts, K = 8"""
    from puflow_amd import ops
    rng = np.random.default_rng(21)
    sizes, qsizes = [64, 300, 5000], [100, 1000, 700]
    refs = [_dev((rng.uniform(-1, 1, (n, 3)) * (1 + i) + i).astype(np.float32)) for i, n in enumerate(sizes)]
    refs[2] = _dev(R.sphere(5000, 3))
    queries = [torch.cat([r[: m // 4], _dev((rng.uniform(-1.2, 1.2, (m - m // 4, 3)) * (1 + i) + i).astype(np.float32))])
               for i, (r, m) in enumerate(zip(refs, qsizes))]                 # a quarter of the queries ARE references
    got = ops.knn_grid_ragged(torch.cat(refs), sizes, torch.cat(queries), qsizes, 8)
    want = ops.knn_large_ragged(torch.cat(refs), sizes, torch.cat(queries), qsizes, 8)
    assert _equal(got, want)
    for r, q, i, d in zip(refs, queries, torch.split(got[0], qsizes), torch.split(got[1], qsizes)):
        alone = ops.knn_grid(r[None], q[None], 8)
        assert torch.equal(alone[0][0], i) and torch.equal(alone[1][0], d)
        assert int(i.max()) < r.shape[0] and int(i.min()) >= 0            # indices inside the cloud


def test_more_clouds_than_one_launch_holds():
    """70 small clouds: two launches of the ragged form (64 + 6), every cloud against the brute-force kernel"""
    from puflow_amd import ops
    rng = np.random.default_rng(22)
    sizes = [int(v) for v in rng.integers(20, 90, 70)]
    qsizes = [int(v) for v in rng.integers(5, 40, 70)]
    ref = _dev(rng.uniform(-1, 1, (sum(sizes), 3)).astype(np.float32))
    query = _dev(rng.uniform(-1, 1, (sum(qsizes), 3)).astype(np.float32))
    assert _equal(ops.knn_grid_ragged(ref, sizes, query, qsizes, 16), ops.knn_large_ragged(ref, sizes, query, qsizes, 16))


def test_workspace_reuse_shows_no_stale_content():
    """one caller-owned workspace, a larger cloud first and a smaller one second; the distances are optional"""
    from puflow_amd import _lib, ops
    from puflow_amd.ops import _stream
    lib = _lib.load()
    big, small = CASES["sphere_self"][0], CASES["lattice"][0]
    nbytes = lib.pf_knn_grid_ws_bytes(_lib.counts([5000]), 1)
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    for ref in (big, small, big[:700]):
        r = _dev(ref)
        idx = torch.empty((1, r.shape[0], 16), dtype=torch.int32, device=DEV)
        _lib.check(lib.pf_knn_grid(r.data_ptr(), r.data_ptr(), 1, r.shape[0], r.shape[0], 16, ws.data_ptr(), nbytes, idx.data_ptr(),
                                   None, _stream()), "pf_knn_grid")
        assert torch.equal(idx, ops.knn_large(r[None], r[None], 16)[0])
