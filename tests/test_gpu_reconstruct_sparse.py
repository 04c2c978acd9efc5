"""The block-sparse reconstruction on the device.  Its layout (keys, list, links, block flags) equals the numpy restatement
(recon_sparse_ref) and, put back into dense form, the dense layout's band; its extraction equals recon_ref's on a random field;
mesh_from_cloud(layout="sparse") equals mesh_from_cloud() bit for bit wherever the dense layout runs; and beyond the dense cap it
returns the restatement's mesh, fed the device's own implicit values, from memory that follows the band.  Every comparison is
exact."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attr_ref as R
import orient_ref as O
import recon_ref as M
import recon_sparse_ref as S

DEV = "cuda:0"
F = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _cloud(name):
    """(points float32, unit normals float32)"""
    if name.startswith(("sphere", "torus")):
        kind, n, sigma = name.split("-")
        pts, nrm = R.surface(kind, float(sigma), int(n))
    elif name == "disc":
        pts, nrm = M.disc(512, 5)
    elif name == "beside":
        pts, nrm = O.two_spheres(False)
    elif name == "near pair":
        pts, nrm = S.far_pair((60, 70, 80))
    elif name == "far pair":
        pts, nrm = S.far_pair((100, 100, 100))
    else:
        raise KeyError(name)
    return pts, nrm.astype(F)


def _same_mesh(a, b):
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and a[1].dtype == b[1].dtype


# ---- 1. the layout ------------------------------------------------------------------------------------------------------------
def _check_layout(pts, tables, dense=True):
    """keys, list, links and block flags of this cloud against the restatement, and against the dense band"""
    from puflow_amd import ops, reconstruct as P
    p, dtables = _dev(pts), [_dev(t) for t in tables]
    dims = S.dims_of(tables)
    keys = ops.recon_block_keys(p, dtables)
    assert keys.dtype == torch.int64 and torch.equal(keys.cpu(), torch.from_numpy(S.block_keys(pts, tables)))
    blocks, links = P.block_list(p, dtables)
    wblocks = S.block_list(S.block_keys(pts, tables))
    assert blocks.dtype == torch.int64 and torch.equal(blocks.cpu(), torch.from_numpy(wblocks))
    assert links.dtype == torch.int32 and torch.equal(links.cpu(), torch.from_numpy(S.links(wblocks, dims)))
    flags = ops.recon_mark_sparse(p, dtables, blocks)
    want = S.mark(pts, tables, wblocks)
    assert flags.dtype == torch.uint8 and torch.equal(flags.cpu(), torch.from_numpy(want))
    if dense:
        band = ops.recon_mark(p, dtables)
        assert torch.equal(P.blocks_to_dense(flags, blocks, dims), band) and torch.equal(P.dense_to_blocks(band, blocks), flags)
        assert np.array_equal(S.from_blocks(want, wblocks, dims), band.cpu().numpy())
    return want, wblocks


@pytest.mark.parametrize("name", ["sphere-512-0.0", "disc", "beside"])
def test_layout_equals_the_restatement(name):
    pts, _ = _cloud(name)
    dims, tables = M.grid_of(pts, M.cell_size(pts))
    flags, blocks = _check_layout(pts, tables)
    assert flags.sum() > 0 and 1 < len(blocks) <= np.prod(S.block_dims(dims))


def test_layout_two_points():
    two = np.array([[0.1, 0.2, 0.3], [0.9, -0.4, 0.35]], F)
    flags, _ = _check_layout(two, M.grid_of(two, 0.05)[1])
    assert flags.sum() == 128
    flags, blocks = _check_layout(two, M.grid_of(two, 2.0)[1])            # both in one cell, a 7 x 7 x 7 grid: one block
    assert flags.sum() == 64 and len(blocks) == 1


def test_layout_points_one_ulp_around_block_faces():
    """points one ulp below, on and one ulp above the table entries with i = 7 and i = 0 (mod 8), where the cell, and with it the
    set of blocks, changes; then points outside the grid (clamped, clipped)"""
    pts, _ = _cloud("torus-2048-0.002")
    dims, tables = M.grid_of(pts, M.cell_size(pts))
    assert min(dims[:2]) > 17
    rows = []
    for i in [i for i in range(dims[0]) if i % 8 in (0, 7)]:
        for j, k in ((7, 3), (8, dims[2] - 4), (dims[1] - 1, 0)):
            e = np.array([tables[0][i], tables[1][j], tables[2][k]], F)
            rows += [np.nextafter(e, F(-9)).astype(F), e, np.nextafter(e, F(9)).astype(F)]
    rows += [np.array([-50, 0, 0], F), np.array([0, 50, 0], F), np.array([0, 0, tables[2][-1]], F), np.array([50, 50, 50], F)]
    _check_layout(np.stack(rows), tables)
    for row in rows[:18]:                                                # and one at a time: -1, 0 and +1 ulp differ as the rule says
        _check_layout(row[None], tables)


# ---- 2. extraction ------------------------------------------------------------------------------------------------------------
def _check_extract(f, flags, tables, blocks):
    """extract_sparse over the re-blocked field against recon_ref.extract over the flags that the list holds: emit order, faces,
    vertex bits"""
    from puflow_amd import ops, reconstruct as P
    dims = S.dims_of(tables)
    dblocks, dtables = _dev(blocks), [_dev(t) for t in tables]
    links = ops.recon_block_links(dblocks, dims)
    assert torch.equal(links.cpu(), torch.from_numpy(S.links(blocks, dims)))
    bf, bflags = P.dense_to_blocks(_dev(f), dblocks), P.dense_to_blocks(_dev(flags), dblocks)
    assert torch.equal(bf.cpu().view(torch.int32), torch.from_numpy(S.to_blocks(f, blocks).view(np.int32)))
    held = P.blocks_to_dense(bflags, dblocks, dims).cpu().numpy()
    want_tri = M.triangles(f, held)
    wverts, wfaces, _ = M.extract(f, held, tables)
    count = ops.mtet_count_sparse(bf, bflags, dblocks, links, dims)
    assert count.dtype == torch.int32 and int(count.sum()) == len(want_tri)
    verts, faces = P.extract_sparse(bf, bflags, dblocks, links, dtables)
    assert torch.equal(faces.cpu(), torch.from_numpy(wfaces.astype(np.int64)))
    assert torch.equal(verts.cpu().view(torch.int32), torch.from_numpy(wverts.view(np.int32)))
    # the emit order, through the ops themselves
    slots = torch.nonzero(count.reshape(-1)).reshape(-1)
    i, j, k = P.slot_corners(slots, dblocks, dims)
    cells = slots[torch.sort((k * dims[1] + j) * dims[0] + i).indices]
    n = count.reshape(-1)[cells].to(torch.int64)
    ids = ops.mtet_emit_sparse(bf, bflags, dblocks, links, dims, cells, torch.cumsum(n, 0) - n, len(want_tri))
    assert torch.equal(ids.cpu(), torch.from_numpy(want_tri))
    return len(want_tri)


def test_extraction_random_field_with_and_without_holes():
    """the 19 x 10 x 9 field of the CPU test (3 x 2 x 2 blocks, partial last blocks, a fifth exact +-0), all blocks listed, then with
    10 % holes, then with block (1, 1, 1) and others missing from the list"""
    from test_recon_sparse_ref import random_field
    f, tables, holes = random_field()
    every = np.arange(12, dtype=np.int64)
    assert _check_extract(f, np.ones(f.shape, np.uint8), tables, every) > 1000
    assert _check_extract(f, holes, tables, every) > 100
    assert _check_extract(f, holes, tables, np.array([b for b in range(12) if b != 10], np.int64)) > 100
    assert _check_extract(f, np.ones(f.shape, np.uint8), tables, np.array([0, 1, 3, 4, 6, 7, 8, 10], np.int64)) > 100
    # no sign change anywhere: an empty mesh
    from puflow_amd import ops, reconstruct as P
    blocks, dtables = _dev(every), [_dev(t) for t in tables]
    one = torch.ones((12, 512), device=DEV)
    verts, faces = P.extract_sparse(one, one.to(torch.uint8), blocks, ops.recon_block_links(blocks, (19, 10, 9)), dtables)
    assert verts.shape == (0, 3) and faces.shape == (0, 3)


# ---- 3. the whole pipeline under the dense cap ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere-512-0.0", "torus-2048-0.002", "disc", "beside", "near pair"])
def test_sparse_mesh_equals_the_dense_mesh(name):
    from puflow_amd import reconstruct as P
    pts, nrm = _cloud(name)
    p, n = _dev(pts), _dev(nrm)
    dense = P.mesh_from_cloud(p, n)
    sparse = P.mesh_from_cloud(p, n, layout="sparse")
    assert len(dense[1]) > 100 and _same_mesh(dense, sparse)
    a, b = dense[2], sparse[2]
    assert a["h"] == b["h"] and a["dims"] == b["dims"] and a["open_edges"] == b["open_edges"]
    assert (a["layout"], a["blocks"]) == ("dense", 0) and b["layout"] == "sparse" and b["blocks"] > 0
    auto = P.mesh_from_cloud(p, n, layout="auto")
    assert auto[2]["layout"] == "dense" and auto[2]["blocks"] == 0 and _same_mesh(dense, auto)
    if name == "near pair":
        assert a["dims"] == (297, 343, 390) and a["open_edges"] == 0


# ---- 4. beyond the dense cap ------------------------------------------------------------------------------------------------------
def _restated(pts, nrm, h, k=8, sigma=1.0):
    """the restatement's mesh of this cloud, fed the DEVICE's implicit values over the restatement's own layout"""
    from puflow_amd import ops
    dims, tables = M.grid_of(pts, h)
    blocks, lnk, flags = S.layout_of(pts, tables)
    s, x = S.corners(flags, blocks, tables)
    p, q = _dev(pts), _dev(x)
    idx, _ = ops.knn_grid(p[None], q[None], k)
    f = np.zeros(flags.shape, F)
    f.reshape(-1)[s] = ops.imls(q, p, _dev(nrm), idx[0], sigma * h).cpu().numpy()
    verts, faces, _, _ = S.extract(f, flags, blocks, lnk, tables)
    return verts, faces, dims, len(blocks)


def test_far_pair_is_refused_dense_and_meshed_sparse():
    from puflow_amd import _lib, reconstruct as P
    pts, nrm = _cloud("far pair")
    p, n = _dev(pts), _dev(nrm)
    with pytest.raises(_lib.PuflowHipError, match="larger --cell"):
        P.mesh_from_cloud(p, n)
    with pytest.raises(_lib.PuflowHipError, match="larger --cell"):
        P.mesh_from_cloud(p, n, layout="dense")
    P.mesh_from_cloud(p, n, layout="sparse")                             # warm: the searches' cached workspaces are no new memory
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    verts, faces, info = P.mesh_from_cloud(p, n, layout="sparse")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    h = M.cell_size(pts)
    wverts, wfaces, wdims, wblocks = _restated(pts, nrm, h)
    assert info["layout"] == "sparse" and info["h"] == h and info["dims"] == wdims == (483, 483, 483) and info["blocks"] == wblocks
    box = int(np.prod(wdims))
    print(f"far pair: {wblocks} blocks, V {len(verts)} F {len(faces)}, peak of new device memory {peak} bytes = 1 / {box / max(peak, 1):.0f} "
          f"of the dense flag array ({box} bytes)")
    assert box > M.MAX_CORNERS and peak * 16 < box
    assert faces.dtype == torch.int32 and np.array_equal(faces.cpu().numpy(), wfaces)
    assert np.array_equal(verts.cpu().numpy().view(np.int32), wverts.view(np.int32))
    v, fa = verts.cpu().numpy(), faces.cpu().numpy()
    assert info["open_edges"] == 0 and M.open_edges(fa) == 0 and M.is_oriented_manifold(fa)
    assert M.euler(v, fa) == 4 and M.volume(v, fa) > 0
    auto = P.mesh_from_cloud(p, n, layout="auto")
    assert auto[2]["layout"] == "sparse" and auto[2]["blocks"] == wblocks and _same_mesh((verts, faces), auto)
    assert _same_mesh((verts, faces), P.mesh_from_cloud(p, n, layout="sparse"))          # the same bits on a second call


def test_small_cell_that_the_default_refuses():
    from puflow_amd import reconstruct as P
    torch.manual_seed(3)
    pts = torch.rand(64, 3).numpy()
    nrm = np.tile(np.array([0, 0, 1], F), (64, 1))
    verts, faces, info = P.mesh_from_cloud(_dev(pts), _dev(nrm), cell=1e-4, layout="sparse")
    wverts, wfaces, wdims, wblocks = _restated(pts, nrm, 1e-4)
    assert info["layout"] == "sparse" and info["dims"] == wdims and info["blocks"] == wblocks and np.prod(wdims) > M.MAX_CORNERS
    assert np.array_equal(faces.cpu().numpy(), wfaces) and np.array_equal(verts.cpu().numpy().view(np.int32), wverts.view(np.int32))
    assert len(wfaces) > 64                                              # a little sheet around every point


def test_wrong_arguments_are_refused():
    from puflow_amd import _lib, ops, reconstruct as P
    p = torch.rand(64, 3, device=DEV)
    with pytest.raises(_lib.PuflowHipError, match="layout"):
        P.mesh_from_cloud(p, p, layout="hash")
    blocks = torch.arange(4, dtype=torch.int64, device=DEV)
    links = ops.recon_block_links(blocks, (20, 30, 40))
    f, flags = torch.zeros(4, 512, device=DEV), torch.zeros(4, 512, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.PuflowHipError, match="block array"):
        ops.mtet_count_sparse(f[:3], flags, blocks, links, (20, 30, 40))
    with pytest.raises(_lib.PuflowHipError, match="block array"):
        ops.mtet_count_sparse(f, flags.to(torch.int32), blocks, links, (20, 30, 40))
    with pytest.raises(_lib.PuflowHipError, match="block keys"):
        ops.recon_block_links(blocks.to(torch.int32), (20, 30, 40))
    with pytest.raises(_lib.PuflowHipError, match="shape"):
        ops.recon_block_links(torch.arange(61, dtype=torch.int64, device=DEV), (20, 30, 40))        # the grid has 60 blocks
    assert int(ops.mtet_count_sparse(f, flags, blocks, links, (20, 30, 40)).sum()) == 0


# ---- 5. the CLI -------------------------------------------------------------------------------------------------------------------
def test_cli_layouts(tmp_path, capsys):
    from puflow_amd import _lib, metrics, reconstruct as P
    (tmp_path / "in").mkdir()
    for name in ("sphere-512-0.0", "torus-2048-0.002"):
        pts, nrm = _cloud(name)
        np.savetxt(tmp_path / "in" / (name.split("-")[0] + ".xyz"), np.concatenate([pts, nrm], axis=1).astype(np.float64), fmt="%.6f")
    P.main(["--source", str(tmp_path / "in"), "--target", str(tmp_path / "a")])
    P.main(["--source", str(tmp_path / "in"), "--target", str(tmp_path / "b"), "--layout", "sparse"])
    for name in ("sphere", "torus"):
        raw = (tmp_path / "a" / (name + ".off")).read_bytes()
        assert len(raw) > 1000 and raw == (tmp_path / "b" / (name + ".off")).read_bytes()
    pts, nrm = _cloud("far pair")
    (tmp_path / "far").mkdir()
    np.savetxt(tmp_path / "far" / "pair.xyz", np.concatenate([pts, nrm], axis=1).astype(np.float64), fmt="%.6f")
    capsys.readouterr()
    P.main(["--source", str(tmp_path / "far"), "--target", str(tmp_path / "c"), "--layout", "auto"])
    assert "open edges" not in capsys.readouterr().out
    verts, faces = metrics.read_off(tmp_path / "c" / "pair.off")
    assert M.open_edges(faces) == 0 and M.euler(verts, faces) == 4 and M.volume(verts, faces) > 0
    with pytest.raises(_lib.PuflowHipError, match="larger --cell"):
        P.main(["--source", str(tmp_path / "far"), "--target", str(tmp_path / "d")])
    assert not (tmp_path / "d" / "pair.off").exists()
