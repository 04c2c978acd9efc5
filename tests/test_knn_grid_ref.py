"""The uniform-grid search's arithmetic (tests/knn_grid_ref.py, a float32 restatement of csrc/knn_grid.hip) against float32 brute
force, on the adversarial inputs of the GPU tests and on references one ulp around every cell edge: the stopping rule is pinned
here, without a device.  The large cases run on an even sample of their queries."""
import numpy as np
import pytest

import knn_grid_ref as R

CASES = R.cases()
MAX_QUERIES = 120


def _sample(query):
    m = query.shape[0]
    return query if m <= MAX_QUERIES else query[np.unique(np.linspace(0, m - 1, MAX_QUERIES).astype(int))]


@pytest.mark.parametrize("name", sorted(CASES))
def test_ring_search_equals_brute_force(name):
    ref, query, ks = CASES[name]
    query = _sample(query)
    grid = R.Grid(ref)
    assert all(1 <= g <= R.GMAX for g in grid.G) and grid.G[0] * grid.G[1] * grid.G[2] <= R.axis_cells(ref.shape[0]) ** 3
    before = dict(R.STATS)
    for K in ks:
        want_i, want_d = R.brute(ref, query, K)
        got = [R.search(grid, q, K) for q in query]
        got_i, got_d = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
        assert np.array_equal(got_i, want_i), (name, K)
        assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32)), (name, K)
    d = {k: R.STATS[k] - before[k] for k in R.STATS}
    print(f"{name}: N {ref.shape[0]} G {grid.G} h {grid.h:.4g}: {d['rings'] / d['queries']:.2f} rings and "
          f"{d['candidates'] / d['queries']:.1f} candidates per query, {d['unverified']} of {d['faces']} face edges unverified")
    assert d["unverified"] == 0                                          # the slack covers the roundings: no face fell back to 0


def test_identical_points_make_one_cell():
    ref, _, _ = CASES["identical"]
    grid = R.Grid(ref)
    assert grid.G == [1, 1, 1] and grid.h > 0
    idx, d2 = R.search(grid, ref[0], 16)
    assert np.array_equal(idx, np.arange(16)) and not d2.any()            # ties broken by index alone


def test_cell_edge_has_a_floor():
    """the extent-4 cloud at 2^20: the natural edge 4 / g is below the coordinates' ulp of 0.125; h stays 16 ulps wide"""
    ref, _, _ = CASES["offset_2p20"]
    grid = R.Grid(ref)
    assert grid.h == np.float32(np.abs(ref).max() * 2.0 ** -19) and grid.h >= 16 * 0.125 * 0.99
    assert max(grid.G) <= 3


@pytest.mark.parametrize("offset,scale", [(0.0, 1.0), (-3.0, 7.0), (4096.0, 1.0), (2.0 ** 20, 64.0)])
def test_references_one_ulp_around_every_cell_edge(offset, scale):
    ref, query = R.edge_cloud(offset, scale)
    grid = R.Grid(ref)
    cx = R.cell(ref[-30:, 0], grid.lo[0], grid.inv_h, grid.G[0]).reshape(-1, 3)
    assert (np.diff(cx, axis=1) >= 0).all()                               # cell_a is monotone across the edge
    j = np.arange(1, 11)[:, None]
    assert ((cx == j - 1) | (cx == j)).all()                              # ... and the points sit on either side of edge j: the
    #                                                                       cell function flips within an ulp or two of lo + j h
    before = dict(R.STATS)
    for K in (1, 8, 16):
        want_i, want_d = R.brute(ref, query, K)
        got_i, got_d = R.knn_grid(ref, query, K)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))
    assert R.STATS["unverified"] == before["unverified"] and R.STATS["faces"] > before["faces"]


def test_cell_is_monotone_and_clamped():
    grid = R.Grid(CASES["cube"][0])
    x = np.sort(np.random.default_rng(3).uniform(-50, 50, 20000).astype(np.float32))
    x = np.concatenate([[np.float32(-3e38)], x, [np.float32(3e38)]]).astype(np.float32)
    c = R.cell(x, grid.lo[0], grid.inv_h, grid.G[0])
    assert (np.diff(c) >= 0).all() and c[0] == 0 and c[-1] == grid.G[0] - 1
