"""pf_point_mesh_grid (csrc/tri_grid.hip) against pf_point_mesh_dist(brute = 1) on the same inputs: torch.equal on the
distances AND on the faces - ties, degenerate faces, oversize triangles and the edge geometry of tests/tri_grid_ref.py included -,
the candidate count that shows the search prunes, and the grid's structure against the restatement."""
import numpy as np
import pytest
import torch

import eval_ref as R
import tri_grid_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(DEV)


def _faces(f):
    return torch.from_numpy(np.ascontiguousarray(f, dtype=np.int64)).to(DEV)


def _brute_raw(pts, tris, seed=None):
    """pf_point_mesh_dist(brute = 1) as it is, in the caller's order"""
    from puflow_amd import _lib, ops
    lib = _lib.load()
    P, F = pts.shape[0], tris.shape[0]
    nws = lib.pf_point_mesh_ws_floats(P, F)
    ws = torch.empty(int(nws), dtype=torch.float32, device=DEV)
    d = torch.empty(P, dtype=torch.float32, device=DEV)
    f = torch.empty(P, dtype=torch.int32, device=DEV)
    _lib.check(lib.pf_point_mesh_dist(pts.data_ptr(), P, tris.data_ptr(), F, None if seed is None else seed.data_ptr(), 1,
                                      d.data_ptr(), f.data_ptr(), ws.data_ptr(), int(nws), ops._stream()), "pf_point_mesh_dist")
    return d, f


def _same_through_the_library(p, v, f):
    from puflow_amd.metrics import point_to_mesh_distance
    args = (_t(p), _t(v), _faces(f))
    d0, f0 = point_to_mesh_distance(*args, return_face=True, search="grid")
    d1, f1 = point_to_mesh_distance(*args, return_face=True, brute=True)
    assert torch.equal(d0, d1) and torch.equal(f0, f1)
    return d0, f0


def _same_raw(p, v, f, seed=None):
    from puflow_amd.metrics import tri_grid_search
    pts, tris = _t(p), _t(G.tris_of(v, f))
    sd = None if seed is None else torch.from_numpy(np.asarray(seed, np.int32)).to(DEV)
    d0, f0 = tri_grid_search(pts, tris, sd)
    d1, f1 = _brute_raw(pts, tris, sd)
    assert torch.equal(d0, d1) and torch.equal(f0, f1)
    return d0, f0


@pytest.fixture(scope="module")
def pruning_fx():
    return G.pruning_fixture()


def test_parity_on_the_pruned_search_fixture(pruning_fx):
    v, f, p = pruning_fx
    _same_through_the_library(p, v, f)


def test_parity_three_ways_on_a_small_torus():
    v, f = R.torus(64, 32)
    rng = np.random.default_rng(11)
    p = (R.sample_surface(v, f, 1024, rng) + rng.normal(0, 0.02, (1024, 3))).astype(F32)
    _same_through_the_library(p, v, f)                                  # Morton order, Morton seeds
    _same_raw(p, v, f)                                                  # seed = None
    perm = rng.permutation(len(f))
    _same_raw(p[rng.permutation(1024)], v, f[perm])                     # shuffled points and triangles, default seeds
    _same_raw(p, v, f[perm], rng.integers(-5, len(f) + 5, 1024))        # arbitrary seeds, some outside the list


def test_vertex_region_ties():
    """a query displaced outwards along the vertex normal of a sphere's vertex is in the vertex region of its 5 - 6 faces: they all
    return the identical |b|^2"""
    v, f = R.icosphere(2)
    v32 = v.astype(F32)
    q = (v32.astype(np.float64) * 1.25).astype(F32)
    _, face = _same_through_the_library(q, v32, f)
    _same_raw(q, v32, f)
    _same_raw(q[::-1], v32, f[::-1])
    # really ties: the winner's vertex is shared with other faces at the same fp32 distance (float64 says so too)
    t3 = v32.astype(np.float64)[f]
    d = R.point_triangle_d2(q[0], t3)
    assert (np.abs(d - d.min()) <= 1e-12).sum() >= 5


def test_queries_on_vertices_and_centroids_have_distance_zero():
    v, f = R.icosphere(2)
    v32 = v.astype(F32)
    q = np.concatenate([v32, v32.astype(np.float64)[f].mean(1).astype(F32)])
    d, _ = _same_through_the_library(q, v32, f)
    _same_raw(q, v32, f)
    assert float(d[:len(v32)].max()) == 0.0 and float(d.max()) < 1e-6


def test_degenerate_faces():
    v, f = R.sheet(degenerate=True)
    v = v.astype(F32)
    rng = np.random.default_rng(4)
    q = np.concatenate([rng.uniform(-1, 1, (300, 3)) * [1.2, 0.8, 0.8], v[-6:] + rng.normal(0, 1e-2, (6, 3))]).astype(F32)
    d, _ = _same_through_the_library(q, v, f)
    _same_raw(q, v, f)
    ref = R.point_mesh_dist(q, v, f)
    assert np.all(np.abs(d.cpu().numpy() - ref) <= 1e-5 * ref + 1e-7 * 3.0)


def test_oversize_triangles():
    from puflow_amd.metrics import tri_grid_search
    v, f = G.with_spanning_triangles(*R.torus(64, 32))
    rng = np.random.default_rng(12)
    p = (R.sample_surface(v, f[:-2], 512, rng) + rng.normal(0, 0.05, (512, 3))).astype(F32)
    _same_through_the_library(p, v, f)
    _same_raw(p, v, f)
    *_, info = tri_grid_search(_t(p), _t(G.tris_of(v, f)), return_info=True)
    assert info["oversize"] == 2                                        # not vacuous
    over = info["ws"][info["over"]:info["over"] + 8].view(torch.int32).cpu().numpy()
    assert sorted(over.tolist()) == [len(f) - 2, len(f) - 1]


@pytest.mark.parametrize("case", ["flat", "one-face", "one-point", "coincident", "far", "ulp"])
def test_edge_geometry(case):
    rng = np.random.default_rng(13)
    if case == "flat":
        v, f = G.flat_mesh()
        q = rng.uniform(-1.2, 1.2, (200, 3))
    elif case == "one-face":
        v, f = np.array([[0.1, 0.2, 0.3], [1.0, 0.1, 0.2], [0.4, 0.9, 0.5]]), np.array([[0, 1, 2]])
        q = rng.uniform(-1, 2, (100, 3))
    elif case == "one-point":
        v, f = R.torus(24, 12)
        q = np.array([[1.1, 0.2, 0.3]])
    elif case == "coincident":
        v, f = np.tile(np.array([[0.3, -0.2, 0.7]]), (9, 1)), np.arange(9).reshape(3, 3)
        q = rng.uniform(-1, 1, (50, 3))
    elif case == "far":
        v, f = R.torus(24, 12)
        d = rng.normal(size=(64, 3))
        q = d / np.linalg.norm(d, axis=1, keepdims=True) * 100 * np.linalg.norm(np.ptp(v, axis=0))
    else:
        v, f = G.ulp_mesh()
        q = np.concatenate([v[::3] + rng.normal(0, 0.03, (len(v[::3]), 3)), v])
    v, q = np.asarray(v, F32), np.asarray(q, F32)
    _same_through_the_library(q, v, f)
    _same_raw(q, v, f)


def test_pruning_is_real(pruning_fx):
    """a condition, not a measurement: the mean number of triangle evaluations of the near-surface queries is at most F / 20
    (a search that scans everything gives F); tests/test_tri_grid_ref.py found 346 of 102 400 in the restatement"""
    from puflow_amd.metrics import tri_grid_search
    v, f, p = pruning_fx
    P, F = len(p), len(f)
    seed = torch.arange(P, dtype=torch.int64) * F // P                  # every query's default seed among the 4096
    _, _, cand = tri_grid_search(_t(p[64:]), _t(G.tris_of(v, f)), seed[64:].int().to(DEV), return_cand=True)
    cand = cand.cpu().numpy()
    print(f"triangle grid on {F} faces: candidates per near-surface query: mean {cand.mean():.1f}, max {cand.max()}, cap {F / 20:.0f}")
    assert cand.min() >= 64 and cand.mean() <= F / 20


def test_undersized_pair_list_scans_everything_and_stays_exact():
    """a workspace sized for fewer pairs than the mesh has: no pair list, every triangle evaluated, the same result"""
    from puflow_amd import _lib, ops
    lib = _lib.load()
    v, f = R.torus(24, 12)
    rng = np.random.default_rng(14)
    pts, tris = _t(rng.uniform(-1.5, 1.5, (65, 3))), _t(G.tris_of(v, f))
    P, F = 65, len(f)
    nb = lib.pf_point_mesh_grid_ws_bytes(P, F, 3)
    ws = torch.zeros(int(nb), dtype=torch.uint8, device=DEV)
    d = torch.empty(P, dtype=torch.float32, device=DEV)
    fa = torch.empty(P, dtype=torch.int32, device=DEV)
    cand = torch.empty(P, dtype=torch.int32, device=DEV)
    _lib.check(lib.pf_point_mesh_grid(pts.data_ptr(), P, tris.data_ptr(), F, None, d.data_ptr(), fa.data_ptr(), cand.data_ptr(),
                                      ws.data_ptr(), int(nb), 3, ops._stream()), "pf_point_mesh_grid")
    d1, f1 = _brute_raw(pts, tris)
    window = np.array([np.diff(G.seed_window(p, P, F)[1:])[0] for p in range(P)])      # clipped at the list's ends
    assert torch.equal(d, d1) and torch.equal(fa, f1) and np.array_equal(cand.cpu().numpy(), F + window)


def test_grid_structure_equals_the_restatement():
    """the cells' triangle sets and the oversize list read back from the workspace, as sets: the order inside a cell is whatever
    the scatter made it"""
    from puflow_amd.metrics import tri_grid_search
    v, f = G.with_spanning_triangles(*R.torus(64, 32))
    tris = G.tris_of(v, f)
    want = G.build(tris)
    *_, info = tri_grid_search(_t(v[:8]), _t(tris), return_info=True)
    assert list(info["G"]) == want["G"] and info["pairs"] == want["pairs"] and info["oversize"] == len(want["over"])
    ws = info["ws"]
    ncells = int(np.prod(want["G"]))
    cstart = ws[info["cstart"]:info["cstart"] + 4 * (ncells + 1)].view(torch.int32).cpu().numpy()
    pairs = ws[info["pair_list"]:info["pair_list"] + 4 * info["pairs"]].view(torch.int32).cpu().numpy()
    over = ws[info["over"]:info["over"] + 4 * info["oversize"]].view(torch.int32).cpu().numpy()
    assert cstart[0] == 0 and cstart[-1] == info["pairs"] and np.all(np.diff(cstart) >= 0)
    assert sorted(over.tolist()) == want["over"].tolist()
    for c in range(ncells):
        got = sorted(pairs[cstart[c]:cstart[c + 1]].tolist())
        assert got == sorted(want["cells"].get(c, [])), c
