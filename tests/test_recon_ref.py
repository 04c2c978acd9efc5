"""The reconstruction's numpy restatement (recon_ref) on analytic distance fields: marching tetrahedra with welded vertices gives
a closed, consistently oriented surface of the right genus that points outwards, with exact zeros in the field too; the table
covers every sign pattern; the grid rules (tables, cell of a point, band) hold what the contract says."""
import numpy as np
import pytest

import recon_ref as M

F = np.float32


def _tables(lo, hi, n):
    return [np.linspace(lo[a], hi[a], n[a]).astype(F) for a in range(3)]


def _field(fn, tables):
    z, y, x = np.meshgrid(tables[2].astype(np.float64), tables[1].astype(np.float64), tables[0].astype(np.float64), indexing="ij")
    return fn(np.stack([x, y, z], axis=-1)).astype(F)


def _sphere():
    t = _tables((-1.37, -1.41, -1.33), (1.43, 1.39, 1.45), (12, 13, 11))
    return _field(M.sphere_field, t), t


def _torus():
    t = _tables((-1.62, -1.58, -0.61), (1.6, 1.63, 0.59), (15, 14, 7))
    return _field(M.torus_field, t), t


def _with_zeros(f, seed):
    """put exact zeros (and a -0) where the field is smallest: vertices land on corners, triangles degenerate"""
    f = f.copy()
    flat = f.reshape(-1)
    near = np.argsort(np.abs(flat))[:40]
    pick = np.random.default_rng(seed).permutation(near)[:20]
    flat[pick[:16]] = 0.0
    flat[pick[16:]] = -0.0
    return f


CASES = {"sphere": (_sphere, 2), "torus": (_torus, 0)}


@pytest.mark.parametrize("zeros", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_closed_oriented_surface_of_the_right_genus(name, zeros):
    make, chi = CASES[name]
    f, tables = make()
    if zeros:
        f = _with_zeros(f, 3)
        assert (f == 0).sum() == 20
    flags = np.ones(f.shape, np.uint8)
    verts, faces, ids = M.extract(f, flags, tables)
    assert len(faces) > 100 and (np.diff(ids) > 0).all()
    assert M.is_oriented_manifold(faces) and M.open_edges(faces) == 0
    assert M.euler(verts, faces) == chi
    assert M.volume(verts, faces) > 0
    dist = (M.sphere_distance if name == "sphere" else M.torus_distance)(verts)
    h = max(float(t[1] - t[0]) for t in tables)
    assert dist.max() <= np.sqrt(3.0) * h                                # the sign changes on an edge of a cell the surface crosses
    if not zeros:                                                        # the volume, to the chord error of this grid
        exact = 4 / 3 * np.pi if name == "sphere" else 2 * np.pi ** 2 * 0.35 ** 2
        assert abs(M.volume(verts, faces) / exact - 1) < 0.1


def test_every_sign_pattern_occurs_in_every_tet():
    seen = np.zeros((6, 16), bool)
    for make, _ in CASES.values():
        f, _t = make()
        cells = np.flatnonzero(M.active_cells(np.ones(f.shape, np.uint8)).reshape(-1))
        masks = M.tet_masks(f, cells)
        for tet in range(6):
            seen[tet, np.unique(masks[:, tet])] = True
        assert seen[:, 1:15].all(), np.argwhere(~seen[:, 1:15])


def test_table_is_generated_and_complete():
    table = M.tet_table()
    assert len(table) == 6 * 14 and M.PERMS[0] == (0, 1, 2) and M.PERMS[5] == (2, 1, 0)
    for (tet, mask), tris in table.items():
        inside = bin(mask).count("1")
        assert len(tris) == (2 if inside == 2 else 1)
        for tri in tris:                                                 # every edge joins an inside and an outside vertex
            assert len(set(tri)) == 3 and all((mask >> i & 1) != (mask >> j & 1) and i < j for i, j in tri)
        # the complement pattern is the same surface seen from the other side
        other = table[tet, 15 - mask]
        assert sorted(map(sorted, tris)) == sorted(map(sorted, other)) and tris != other
    # the six tets tile the cell: same four corners never twice, all end on the main diagonal
    assert len({tuple(M.tet_vertex(t, v) for v in range(4)) for t in range(6)}) == 6
    assert all(M.tet_vertex(t, 0) == (0, 0, 0) and M.tet_vertex(t, 3) == (1, 1, 1) for t in range(6))


def test_triangle_order_and_edge_ids():
    f, tables = _sphere()
    flags = np.ones(f.shape, np.uint8)
    tri = M.triangles(f, flags)
    Dz, Dy, Dx = f.shape
    assert tri.dtype == np.int64 and tri.min() >= 0 and tri.max() < 7 * f.size
    # an edge's owner is a corner of the triangle's cell; cells come in ascending order
    owner = tri // 7
    low = owner.min(axis=1)
    assert (np.diff(low) >= -(Dx * Dy + Dx + 1)).all()
    verts, faces, ids = M.extract(f, flags, tables)
    assert faces.dtype == np.int32 and np.array_equal(ids[faces], tri)
    # a band that leaves out half the box gives an open surface along the cut, and only there
    half = flags.copy()
    half[:, :, Dx // 2:] = 0
    v2, f2, _ = M.extract(f, half, tables)
    assert 0 < len(f2) < len(faces) and M.open_edges(f2) > 0
    assert v2[:, 0].max() <= tables[0][Dx // 2 - 1]


def test_vertex_arithmetic_is_three_rounded_fp32_operations():
    tables = [np.array([0.1, 0.4, 0.7], F)] * 3
    f = np.full((3, 3, 3), 1.0, F)
    f[1, 1, 1] = F(-0.3)
    verts, faces, ids = M.extract(f, np.ones(f.shape, np.uint8), tables)
    assert M.is_oriented_manifold(faces) and M.euler(verts, faces) == 2 and M.volume(verts, faces) > 0
    assert len(verts) == 14                                             # the 14 grid edges at the centre corner
    first = ids[0]                                                       # owner (0,0,0), class (1,1,1): a = corner 0, b = the centre
    assert first == 6
    t = F(1.0) / (F(1.0) - F(-0.3))
    want = tables[0][0] + F(t * F(tables[0][1] - tables[0][0]))
    assert verts[0, 0] == want and verts.dtype == F


def test_grid_rules():
    lo, hi, h = np.array([-1, -0.5, 0], F), np.array([1, 0.5, 0.01], F), 0.1
    dims, tables = M.grid(lo, hi, h)
    assert dims == (20 + 7, 10 + 7, 1 + 7)
    assert all(t.dtype == F and len(t) == d for t, d in zip(tables, dims))
    assert tables[0][0] == F(-1.0 - 0.3) and tables[2][7] == F(np.float64(0 - 3 * 0.1) + 7 * 0.1)
    g = tables[0]
    e = g[5]
    assert M.cell(np.nextafter(e, F(-9)), g) == 4 and M.cell(e, g) == 5 and M.cell(np.nextafter(e, F(9)), g) == 5
    assert M.cell(F(-50), g) == 0 and M.cell(F(50), g) == len(g) - 2 and M.cell(g[-1], g) == len(g) - 2
    pts = np.array([[-1, -0.5, 0], [1, 0.5, 0.01]], F)
    flags = M.mark(pts, tables)
    assert flags.shape == (8, 17, 27) and flags.sum() == 128
    assert flags[:, :, 0].sum() == 0 and flags[:, :, -1].sum() == 0 and flags[0].sum() == 0 and flags[-1].sum() == 0
    assert M.active_cells(flags).sum() == 2 * 27
    c, x = M.corners(flags, tables)
    assert len(c) == 128 and (np.diff(c) > 0).all() and x.dtype == F


def test_imls_of_a_plane_is_the_signed_distance():
    rng = np.random.default_rng(1)
    pts = np.concatenate([rng.uniform(-1, 1, (200, 2)), np.zeros((200, 1))], axis=1).astype(F)
    nrm = np.tile(np.array([0, 0, 1], F), (200, 1))
    q = rng.uniform(-0.5, 0.5, (50, 3)).astype(F)
    idx = np.argsort(M.sqd(q[:, None], pts[None]), axis=1, kind="stable")[:, :8]
    for sigma_h in (0.05, 0.4):
        assert np.abs(M.imls(q, pts, nrm, idx, sigma_h) - q[:, 2].astype(np.float64)).max() < 1e-15
    assert np.abs(M.imls(q, pts, nrm, idx[:, :1], 0.1) - q[:, 2]).max() < 1e-15


def test_cell_size_is_the_lower_median_sixth_neighbour():
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 2)
    pts = np.concatenate([g, np.zeros((64, 1))], axis=1).astype(F)
    # an interior point of a square lattice: 4 at distance 1, 4 at sqrt 2 -> the 6th other point is at sqrt 2
    assert M.cell_size(pts) == pytest.approx(np.sqrt(2.0)) and M.cell_size(pts, 0.5) == pytest.approx(np.sqrt(0.5))
