"""The reconstruction on the device against its numpy restatement (recon_ref).  The band, the vertices (bitwise), the faces and
their order are exact: torch.equal to the restatement, which is fed the DEVICE's own implicit values so that a last-bit
difference in f cannot change a sign between the two sides.  The implicit value itself is held to the float64 restatement by a
derived bound.  The closed test surfaces must then come out closed, of the right genus, pointing outwards and within sqrt(3) h."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attr_ref as R
import orient_ref as O
import recon_ref as M

DEV = "cuda:0"
F = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tables(pts, h):
    """the host-side grid of puflow_amd.reconstruct on this cloud, checked against the restatement's: (dims, numpy, device)"""
    from puflow_amd import reconstruct as P
    pts = np.asarray(pts, F)
    dims, tables = P.corner_tables(pts.min(axis=0).astype(np.float64), pts.max(axis=0).astype(np.float64), h)
    wdims, wtables = M.grid_of(pts, h)
    assert dims == wdims and all(np.array_equal(a, b) for a, b in zip(tables, wtables))
    return dims, tables, [_dev(t) for t in tables]


@functools.lru_cache(maxsize=None)
def _cloud(name):
    """(points float32, unit normals float32, analytic distance or None)"""
    if name.startswith(("sphere", "torus")):
        kind, n, sigma = name.split("-")
        pts, nrm = R.surface(kind, float(sigma), int(n))
        return pts, nrm.astype(F), (M.sphere_distance if kind == "sphere" else M.torus_distance)
    if name == "disc":
        pts, nrm = M.disc(512, 5)
        return pts, nrm.astype(F), None
    if name == "beside":
        pts, nrm = O.two_spheres(False)
        return pts, nrm.astype(F), None
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _band(name):
    """the device's band of a cloud at its default cell size: everything the later stages share"""
    from puflow_amd import ops, reconstruct as P
    pts, nrm, _ = _cloud(name)
    h = P.cell_size(_dev(pts))
    assert h == M.cell_size(pts)                                         # the same search, the same lower median, one sqrt
    dims, tables, dtables = _tables(pts, h)
    flags = ops.recon_mark(_dev(pts), dtables)
    corner, query = M.corners(flags.cpu().numpy(), tables)
    return h, dims, tables, dtables, flags, corner, query


# ---- 1. the implicit value --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 2.0])
@pytest.mark.parametrize("name,k", [("sphere-512-0.0", 1), ("sphere-512-0.0", 8), ("sphere-512-0.0", 16), ("torus-2048-0.0", 8)])
def test_imls_against_float64(name, k, sigma):
    """|f - f_ref| <= 2^-23 |f_ref| + 2^-40 h: one fp32 rounding of the result, twice over, plus double-precision slack on terms
    of size h that cancel.  Queries: the band's corners, then the cloud's own points (d2_0 = 0)."""
    from puflow_amd import ops, reconstruct as P
    pts, nrm, _ = _cloud(name)
    h, _dims, _t, _dt, _flags, _corner, query = _band(name)
    query = np.concatenate([query, pts])
    p, n, q = _dev(pts), _dev(nrm), _dev(query)
    idx, _ = ops.knn_grid(p[None], q[None], k)
    f = ops.imls(q, p, n, idx[0], sigma * h)
    assert f.dtype == torch.float32 and f.shape == (len(query),)
    want = M.imls(query, pts, nrm, idx[0].cpu().numpy(), sigma * h)
    err = np.abs(f.cpu().numpy().astype(np.float64) - want)
    bound = 2.0 ** -23 * np.abs(want) + 2.0 ** -40 * h
    print(f"imls {name} k={k} sigma={sigma}: Q {len(query)} max err / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    assert torch.equal(P.implicit(p, n, q, k=k, sigma=sigma, h=h), f)   # the library entry is the same two calls


# ---- 2. the band ------------------------------------------------------------------------------------------------------------
def _check_mark(pts, tables):
    from puflow_amd import ops
    flags = ops.recon_mark(_dev(pts), [_dev(t) for t in tables])
    want = M.mark(pts, tables)
    assert flags.dtype == torch.uint8 and torch.equal(flags.cpu(), torch.from_numpy(want))
    return want


def test_mark_sphere():
    pts, _, _ = _cloud("sphere-512-0.0")
    h, dims, tables, _dt, flags, _c, _q = _band("sphere-512-0.0")
    want = _check_mark(pts, tables)
    assert torch.equal(flags.cpu(), torch.from_numpy(want))
    assert want[0].sum() == 0 and want[-1].sum() == 0 and want[:, 0].sum() == 0 and want[:, -1].sum() == 0     # pad = 3 holds the band
    assert want[:, :, 0].sum() == 0 and want[:, :, -1].sum() == 0 and 0 < want.sum() < want.size


def test_mark_flat_sheet_and_two_points():
    rng = np.random.default_rng(2)
    sheet = np.concatenate([rng.uniform(-1, 1, (700, 2)), np.zeros((700, 1))], axis=1).astype(F)
    dims, tables, _ = _tables(sheet, 0.07)
    assert dims[2] == 7                                                  # a thin box: the pad and nothing else
    want = _check_mark(sheet, tables)
    assert want[:1].sum() == 0 and want[6:].sum() == 0 and want[1:6].sum() > 0
    two = np.array([[0.1, 0.2, 0.3], [0.9, -0.4, 0.35]], F)
    _, tables, _ = _tables(two, 0.05)
    assert _check_mark(two, tables).sum() == 128
    _, tables, _ = _tables(two, 2.0)                                     # both in one cell
    assert _check_mark(two, tables).sum() == 64


def test_mark_points_one_ulp_around_table_entries():
    pts, _, _ = _cloud("sphere-512-0.0")
    _h, dims, tables, _dt, _f, _c, _q = _band("sphere-512-0.0")
    rows = []
    for i in range(0, dims[0], 3):
        for j, k in ((3, 4), (dims[1] - 4, dims[2] // 2)):
            e = np.array([tables[0][i], tables[1][j], tables[2][k]], F)
            rows += [np.nextafter(e, F(-9)).astype(F), e, np.nextafter(e, F(9)).astype(F)]
    rows += [np.array([-50, 0, 0], F), np.array([0, 50, 0], F), np.array([0, 0, tables[2][-1]], F)]      # outside: clamped, clipped
    _check_mark(np.stack(rows), tables)
    for row in rows[:9]:                                                 # and one at a time: -1, 0 and +1 ulp differ as the rule says
        _check_mark(row[None], tables)


# ---- 3. extraction ----------------------------------------------------------------------------------------------------------
def _check_extract(f, flags, tables):
    """the device's marching tetrahedra against the restatement on this very f; returns the device's mesh on the host"""
    from puflow_amd import ops, reconstruct as P
    df, dflags, dtables = _dev(f), _dev(flags), [_dev(t) for t in tables]
    want_tri = M.triangles(f, flags)
    count = ops.mtet_count(df, dflags)
    assert int(count.sum()) == len(want_tri)
    verts, faces = P.extract(df, dflags, dtables)
    wverts, wfaces, wids = M.extract(f, flags, tables)
    assert torch.equal(faces.cpu(), torch.from_numpy(wfaces.astype(np.int64)))
    assert torch.equal(verts.cpu().view(torch.int32), torch.from_numpy(wverts.view(np.int32)))
    first = (torch.cumsum(count.reshape(-1), 0) - count.reshape(-1)).reshape(count.shape)
    assert torch.equal(ops.mtet_emit(df, dflags, first, len(want_tri)).cpu(), torch.from_numpy(want_tri))
    return verts.cpu().numpy(), faces.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _field(name, k=8, sigma=1.0):
    """the device's own f over a cloud's band"""
    from puflow_amd import ops
    pts, nrm, _ = _cloud(name)
    h, dims, tables, dtables, flags, corner, query = _band(name)
    p, q = _dev(pts), _dev(query)
    idx, _ = ops.knn_grid(p[None], q[None], k)
    f = np.zeros(flags.shape, F)
    f.reshape(-1)[corner] = ops.imls(q, p, _dev(nrm), idx[0], sigma * h).cpu().numpy()
    return f


@pytest.mark.parametrize("name", ["sphere-512-0.0", "torus-2048-0.002", "disc", "beside"])
def test_extraction_equals_the_restatement(name):
    _h, _dims, tables, _dt, flags, _c, _q = _band(name)
    verts, faces = _check_extract(_field(name), flags.cpu().numpy(), tables)
    assert len(faces) > 100
    if name == "disc":
        assert M.open_edges(faces) > 0                                   # an open surface keeps its boundary
    # the whole pipeline in one call gives the same mesh
    from puflow_amd import reconstruct as P
    pts, nrm, _ = _cloud(name)
    v, fa, info = P.mesh_from_cloud(_dev(pts), _dev(nrm))
    assert fa.dtype == torch.int32 and np.array_equal(fa.cpu().numpy(), faces) and np.array_equal(v.cpu().numpy().view(np.int32), verts.view(np.int32))
    assert info["h"] == _h and info["dims"] == _dims and info["open_edges"] == M.open_edges(faces)


def test_extraction_random_values_with_exact_zeros():
    """a 6 x 5 x 4 all-active grid of random values, a fifth of them exactly 0 (some -0): every sign pattern, vertices on corners"""
    rng = np.random.default_rng(8)
    f = rng.standard_normal((4, 5, 6)).astype(F)
    z = rng.uniform(0, 1, f.shape)
    f[z < 0.15] = 0.0
    f[(z >= 0.15) & (z < 0.2)] = -0.0
    tables = [np.cumsum(rng.uniform(0.1, 0.3, d)).astype(F) for d in (6, 5, 4)]
    flags = np.ones(f.shape, np.uint8)
    masks = M.tet_masks(f, np.flatnonzero(M.active_cells(flags).reshape(-1)))
    assert all(len(np.unique(masks[:, t])) >= 14 for t in range(6))
    _check_extract(f, flags, tables)
    holes = flags.copy()
    holes[rng.uniform(0, 1, f.shape) < 0.1] = 0                          # and with cells missing from the band
    _check_extract(f, holes, tables)


# ---- 4. properties at the default cell size -----------------------------------------------------------------------------------
PROPERTY_CASES = [f"{kind}-{n}-{sigma}" for kind in ("sphere", "torus") for n in (512, 2048) for sigma in (0.0, 0.002)]


@pytest.mark.parametrize("name", PROPERTY_CASES)
def test_closed_surfaces_come_out_closed(name):
    from puflow_amd import reconstruct as P
    pts, nrm, distance = _cloud(name)
    verts, faces, info = P.mesh_from_cloud(_dev(pts), _dev(nrm))
    verts, faces = verts.cpu().numpy(), faces.cpu().numpy()
    worst = distance(verts).max() / info["h"]
    print(f"reconstruct {name}: h {info['h']:.5f} dims {info['dims']} V {len(verts)} F {len(faces)} open {info['open_edges']} "
          f"euler {M.euler(verts, faces)} volume {M.volume(verts, faces):.4f} worst vertex {worst:.3f} h")
    assert info["open_edges"] == 0 and M.open_edges(faces) == 0 and M.is_oriented_manifold(faces)
    assert M.euler(verts, faces) == (2 if name.startswith("sphere") else 0)
    assert M.volume(verts, faces) > 0
    assert worst <= np.sqrt(3.0)


# ---- 5. the pipeline: estimated, propagated normals -----------------------------------------------------------------------------
def test_estimated_normals_give_a_closed_torus():
    from puflow_amd import attributes as A, reconstruct as P
    pts, _, _ = _cloud("torus-2048-0.0")
    p = _dev(pts)
    nrm, _ = A.estimate_normals(p, 16, search="grid", orient="propagate")
    verts, faces, info = P.mesh_from_cloud(p, nrm)
    verts, faces = verts.cpu().numpy(), faces.cpu().numpy()
    print(f"pipeline torus 2048: open {info['open_edges']} euler {M.euler(verts, faces)} volume {M.volume(verts, faces):.4f}")
    assert info["open_edges"] == 0 and M.euler(verts, faces) == 0 and M.volume(verts, faces) > 0


# ---- 6. the CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_same_bytes_twice(tmp_path, capsys):
    from puflow_amd import metrics, reconstruct as P
    (tmp_path / "in").mkdir()
    for name in ("sphere-512-0.0", "torus-2048-0.002"):
        pts, nrm, _ = _cloud(name)
        np.savetxt(tmp_path / "in" / (name.split("-")[0] + ".xyz"), np.concatenate([pts, nrm], axis=1).astype(np.float64), fmt="%.6f")
    for out in ("a", "b"):
        P.main(["--source", str(tmp_path / "in"), "--target", str(tmp_path / out)])
    assert "open edges" not in capsys.readouterr().out
    for name, chi in (("sphere", 2), ("torus", 0)):
        raw = (tmp_path / "a" / (name + ".off")).read_bytes()
        assert raw == (tmp_path / "b" / (name + ".off")).read_bytes()
        verts, faces = metrics.read_off(tmp_path / "a" / (name + ".off"))
        assert M.open_edges(faces) == 0 and M.euler(verts, faces) == chi and M.volume(verts, faces) > 0
    # a cell of a third of the default is below the spacing: the surface tears, and the CLI says so
    P.main(["--source", str(tmp_path / "in"), "--target", str(tmp_path / "c"), "--cell_scale", "0.33"])
    said = capsys.readouterr().out
    assert "sphere.off" in said and "open edges" in said and "--cell" in said
    # normals elsewhere in the row
    pts, nrm, _ = _cloud("sphere-512-0.0")
    (tmp_path / "in7").mkdir()
    np.savetxt(tmp_path / "in7" / "sphere.xyz", np.concatenate([pts, pts[:, :1] * 0 + 7, nrm], axis=1).astype(np.float64), fmt="%.6f")
    P.main(["--source", str(tmp_path / "in7"), "--target", str(tmp_path / "d"), "--normal_column", "5"])
    assert (tmp_path / "d" / "sphere.off").read_bytes() == (tmp_path / "a" / "sphere.off").read_bytes()
    (tmp_path / "in3").mkdir()
    np.savetxt(tmp_path / "in3" / "bare.xyz", pts.astype(np.float64), fmt="%.6f")
    with pytest.raises(SystemExit, match="--estimate_normals K --normals_orient propagate"):
        P.main(["--source", str(tmp_path / "in3"), "--target", str(tmp_path / "e")])


def test_wrong_ranks_are_refused():
    from puflow_amd import _lib, reconstruct as P
    p = torch.zeros(64, 3, device=DEV)
    with pytest.raises(_lib.PuflowHipError):
        P.mesh_from_cloud(p[None], p[None])
    with pytest.raises(_lib.PuflowHipError):
        P.mesh_from_cloud(p, p[:32])
    with pytest.raises(_lib.PuflowHipError):
        P.implicit(p, p, p[:, :2], h=0.1)
    with pytest.raises(_lib.PuflowHipError, match="k = 65"):
        P.mesh_from_cloud(p, p, k=65)
    with pytest.raises(_lib.PuflowHipError, match="larger --cell"):
        P.mesh_from_cloud(torch.rand(64, 3, device=DEV), p, cell=1e-4)
