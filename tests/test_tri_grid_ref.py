"""The triangle grid's arithmetic (tests/tri_grid_ref.py, a restatement of csrc/tri_grid.hip) without a GPU: the ring search
with its stopping rule returns the winners of a full scan under the same tie rule, on the inputs the GPU test uses; the grid's
structure has the properties the stopping rule rests on; the pruning cap of the GPU test holds in the restatement."""
import numpy as np
import pytest

import eval_ref as R
import tri_grid_ref as G

F32 = np.float32


def _queries(v, rng, n=40, spread=0.05):
    v = np.asarray(v, F32)
    lo, hi = v.min(0), v.max(0)
    near = v[rng.integers(0, len(v), n)] + rng.normal(0, spread, (n, 3))
    inside = rng.uniform(lo, hi, (n // 2, 3))
    return np.concatenate([near, inside]).astype(F32)


def _check(v, f, q, seed=None):
    tris = G.tris_of(v, f)
    grid = G.build(tris)
    got, cand = G.search(grid, q, tris, seed)
    want = G.full_scan(q, tris, seed)
    np.testing.assert_array_equal(got, want)
    return grid, cand


def test_axis_cells_rule():
    assert [G.axis_cells(F) for F in (1, 4, 5, 13, 14, 4096, 102400, 10 ** 6, 1 << 23, 1 << 28)] == \
        [2, 2, 3, 3, 4, 21, 59, 126, 256, 256]


def test_every_vertex_lies_in_its_triangles_block_and_cells_hold_what_the_blocks_say():
    v, f = R.torus(32, 16, bump=0.15)
    tris = G.tris_of(v, f)
    g = G.build(tris)
    for a in range(3):
        for k in range(3):
            c = G.cell(tris[:, 3 * k + a], g["lo"][a], g["inv_h"], g["G"][a])
            assert np.all((g["c0"][:, a] <= c) & (c <= g["c1"][:, a]))
    assert sum(len(s) for s in g["cells"].values()) == g["pairs"] and len(g["over"]) == 0
    assert max(g["cells"]) < g["G"][0] * g["G"][1] * g["G"][2] <= G.axis_cells(len(f)) ** 3
    assert max(g["G"]) == G.axis_cells(len(f))                                  # the longest extent spans g cells


def test_cell_function_is_monotone_at_the_edges():
    v, f = G.ulp_mesh()
    g = G.build(G.tris_of(v, f))
    for a in range(3):
        x = np.sort(v[:, a])
        c = G.cell(x, g["lo"][a], g["inv_h"], g["G"][a])
        assert np.all(np.diff(c) >= 0) and c.min() == 0 and c.max() == g["G"][a] - 1


@pytest.mark.parametrize("seeded", [False, True])
def test_small_bumpy_torus(seeded):
    v, f = R.torus(32, 16, bump=0.15)
    rng = np.random.default_rng(1)
    q = _queries(v, rng)
    seed = rng.integers(0, len(f), len(q)) if seeded else None
    _, cand = _check(v, f, q, seed)
    assert cand.mean() < len(f) / 2                                             # it prunes


def test_degenerate_sheet():
    v, f = R.sheet(degenerate=True)
    rng = np.random.default_rng(4)
    q = np.concatenate([rng.uniform(-1, 1, (40, 3)) * [1.2, 0.8, 0.8], v[-6:] + rng.normal(0, 1e-2, (6, 3))])
    _check(v, f, q.astype(F32))


def test_flat_mesh_has_one_layer_of_cells():
    v, f = G.flat_mesh()
    grid, _ = _check(v, f, _queries(v, np.random.default_rng(2), spread=0.2))
    assert grid["G"][2] == 1


def test_box_spanning_triangles_are_oversize():
    v, f = G.with_spanning_triangles(*R.torus(32, 16))
    grid, cand = _check(v, f, _queries(v, np.random.default_rng(3)))
    assert list(grid["over"]) == [len(f) - 2, len(f) - 1]


def test_single_triangle_and_coincident_vertices():
    v = np.array([[0.1, 0.2, 0.3], [1.0, 0.1, 0.2], [0.4, 0.9, 0.5]], F32)
    f = np.array([[0, 1, 2]])
    rng = np.random.default_rng(5)
    _check(v, f, rng.uniform(-1, 2, (20, 3)).astype(F32))
    vc = np.tile(np.array([[0.3, -0.2, 0.7]], F32), (9, 1))
    fc = np.arange(9).reshape(3, 3)
    grid, _ = _check(vc, fc, rng.uniform(-1, 1, (10, 3)).astype(F32))
    assert grid["G"] == [1, 1, 1] and np.isfinite(grid["inv_h"]) and grid["h"] > 0
    zero = np.zeros((3, 3), F32)
    grid, _ = _check(zero, f, rng.uniform(-1, 1, (4, 3)).astype(F32))
    assert grid["G"] == [1, 1, 1] and grid["h"] > 0


def test_queries_far_outside_the_box():
    v, f = R.torus(24, 12)
    diag = float(np.linalg.norm(np.ptp(v, axis=0)))
    rng = np.random.default_rng(6)
    d = rng.normal(size=(12, 3))
    q = (d / np.linalg.norm(d, axis=1, keepdims=True) * 100 * diag).astype(F32)
    q = np.concatenate([q, np.array([[100 * diag, 0, 0], [0, -100 * diag, 0], [0.5, 0.5, 100 * diag]], F32)])
    _check(v, f, q)


def test_queries_on_vertices_and_centroids():
    v, f = R.icosphere(1)
    v = v.astype(F32)
    q = np.concatenate([v, v.astype(np.float64)[f].mean(1).astype(F32)])
    _check(v, f, q)


def test_vertices_one_ulp_around_cell_faces():
    v, f = G.ulp_mesh()
    rng = np.random.default_rng(7)
    q = np.concatenate([_queries(v, rng), v[::7]])
    _check(v, f, q)


def test_pruning_cap_holds_in_the_restatement():
    """the GPU test asserts mean(cand) <= F / 20 on the near-surface queries of this fixture; here on every 42nd of them"""
    v, f, p = G.pruning_fixture()
    tris = G.tris_of(v, f)
    grid = G.build(tris)
    q = p[64::42]
    P = len(p)
    # the queries keep their own default seeds: seed = p F / P of their place among the 4096
    seed = np.array([k * len(f) // P for k in range(64, P, 42)])
    got, cand = G.search(grid, q, tris, seed)
    np.testing.assert_array_equal(got, G.full_scan(q, tris, seed))
    print(f"triangle grid on {len(f)} faces: G = {grid['G']}, pairs = {grid['pairs']}, candidates per query: "
          f"mean {cand.mean():.1f}, max {cand.max()}, cap {len(f) / 20:.0f}")
    assert cand.mean() <= len(f) / 20
