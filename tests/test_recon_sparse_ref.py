"""The block-sparse restatement (recon_sparse_ref) against the dense one (recon_ref), on the CPU: the block flags are the dense
flags re-blocked, and the extraction over blocks gives the dense triangles (edge ids, in order), vertices (bitwise) and faces -
also where blocks are missing from the list.  Then the far pair, whose box is over the dense cap: a closed, oriented mesh of two
spheres from a layout that never holds the box."""
import functools

import numpy as np

import attr_ref as R
import recon_ref as M
import recon_sparse_ref as S

F = np.float32


def _same_extraction(f, flags, tables, blocks):
    """dense f / flags [D_z, D_y, D_x] and a block list: the sparse extraction over the re-blocked arrays equals the dense one over
    the part of the flags that the list holds"""
    dims = S.dims_of(tables)
    lnk = S.links(blocks, dims)
    bflags, bf = S.to_blocks(flags, blocks), S.to_blocks(f, blocks)
    held = S.from_blocks(bflags, blocks, dims)
    assert np.array_equal(S.from_blocks(bf, blocks, dims)[held != 0], f[held != 0])
    wverts, wfaces, wids = M.extract(f, held, tables)
    verts, faces, ids, tri = S.extract(bf, bflags, blocks, lnk, tables)
    assert np.array_equal(tri, M.triangles(f, held))                    # the edge ids, in the dense order
    assert np.array_equal(ids, wids) and np.array_equal(faces, wfaces)
    assert np.array_equal(verts.view(np.int32), wverts.view(np.int32))
    return held, tri


def random_field():
    """a 19 x 10 x 9 grid (3 x 2 x 2 blocks, every last block partial) of random values, a fifth of them exactly +-0; the flags with
    10 % holes"""
    rng = np.random.default_rng(8)
    f = rng.standard_normal((9, 10, 19)).astype(F)
    z = rng.uniform(0, 1, f.shape)
    f[z < 0.15] = 0.0
    f[(z >= 0.15) & (z < 0.2)] = -0.0
    tables = [np.cumsum(rng.uniform(0.1, 0.3, d)).astype(F) for d in (19, 10, 9)]
    holes = np.ones(f.shape, np.uint8)
    holes[rng.uniform(0, 1, f.shape) < 0.1] = 0
    return f, tables, holes


def test_random_field_all_blocks_and_holes():
    f, tables, holes = random_field()
    assert S.block_dims(S.dims_of(tables)) == (3, 2, 2)
    every = np.arange(12, dtype=np.int64)
    full = np.ones(f.shape, np.uint8)
    masks = M.tet_masks(f, np.flatnonzero(M.active_cells(full).reshape(-1)))
    assert all(len(np.unique(masks[:, t])) >= 14 for t in range(6))
    _, tri = _same_extraction(f, full, tables, every)
    assert len(tri) > 1000
    _same_extraction(f, holes, tables, every)


def test_random_field_with_blocks_missing_from_the_list():
    """block (1, 1, 1) - diagonal to block (0, 0, 0) - is not listed: the cell with lower corner (7, 7, 7) straddles all 8 blocks
    and reaches it through link 7 only; it and every cell that touches the missing block's corners must go"""
    f, tables, holes = random_field()
    dims = S.dims_of(tables)
    nb = S.block_dims(dims)
    missing = int(S.key_of(1, 1, 1, nb))
    blocks = np.array([b for b in range(12) if b != missing], np.int64)
    lnk = S.links(blocks, dims)
    assert lnk[S.find(blocks, [S.key_of(0, 0, 0, nb)])[0], 7] == -1
    for flags in (np.ones(f.shape, np.uint8), holes):
        held, tri = _same_extraction(f, flags, tables, blocks)
        assert held[8:, 8:, 8:16].sum() == 0 and held[:8, :8, :8].sum() > 400
        cells, _ = S.active_cells(S.to_blocks(flags, blocks), blocks, lnk, dims)
        at = set(zip(*(a.tolist() for a in S.slot_corners(cells, blocks, dims))))
        assert (7, 7, 7) not in at                                       # the straddling cell is gone, its neighbours below stay
        assert flags is holes or ((7, 7, 6) in at and (6, 7, 7) in at and (7, 6, 7) in at)
    # and with the far corner block of the list gone as well as an inner one
    _same_extraction(f, holes, tables, np.array([0, 1, 3, 4, 6, 7, 8, 10], np.int64))


@functools.lru_cache(maxsize=None)
def _sphere():
    pts, nrm = R.surface("sphere", 0.0, 512)
    h = M.cell_size(pts)
    dims, tables = M.grid_of(pts, h)
    flags = M.mark(pts, tables)
    x = np.stack(np.meshgrid(tables[2], tables[1], tables[0], indexing="ij")[::-1], axis=-1)
    return pts, nrm, h, dims, tables, flags, M.sphere_field(x).astype(F)


def test_sphere_layout_is_the_dense_band_in_blocks():
    pts, _nrm, _h, dims, tables, flags, f = _sphere()
    keys = S.block_keys(pts, tables)
    assert keys.shape == (512, 8) and (keys[:, 0] <= keys[:, 7]).all()
    blocks, lnk, bflags = S.layout_of(pts, tables)
    assert len(blocks) < np.prod(S.block_dims(dims)) or np.prod(S.block_dims(dims)) <= 27
    assert np.array_equal(bflags, S.to_blocks(flags, blocks)) and np.array_equal(S.from_blocks(bflags, blocks, dims), flags)
    s, x = S.corners(bflags, blocks, tables)
    c, wx = M.corners(flags, tables)
    i, j, k = S.slot_corners(s, blocks, dims)
    order = np.argsort((k * dims[1] + j) * dims[0] + i)
    assert np.array_equal(((k * dims[1] + j) * dims[0] + i)[order], c) and np.array_equal(x[order], wx)
    held, tri = _same_extraction(f, flags, tables, blocks)
    assert np.array_equal(held, flags) and len(tri) > 100


def _closed_pair(verts, faces):
    assert M.open_edges(faces) == 0 and M.is_oriented_manifold(faces)
    assert M.euler(verts, faces) == 4 and M.volume(verts, faces) > 0


@functools.lru_cache(maxsize=None)
def far_mesh():
    pts, nrm = S.far_pair((100, 100, 100))
    return (pts, nrm) + S.mesh_from_cloud(pts, nrm, M.cell_size(pts))


def test_far_pair_over_the_dense_cap():
    pts, nrm, verts, faces, info = far_mesh()
    assert info["dims"] == (483, 483, 483) and abs(info["h"] - 0.2143) < 5e-5 and np.prod(info["dims"]) > M.MAX_CORNERS
    assert max(info["dims"]) <= S.MAX_AXIS and len(info["blocks"]) <= S.MAX_BLOCKS
    assert int(info["flags"].sum()) == 3182 and len(info["blocks"]) * S.SLOTS * 16 < np.prod(info["dims"])
    _closed_pair(verts, faces)
    assert abs(M.volume(verts, faces) - 2 * 4.26) < 0.1
    near = np.linalg.norm(verts.astype(np.float64), axis=1) < 50          # the two pieces: each closed, a sphere
    piece = near[faces[:, 0]]
    assert (near[faces] == piece[:, None]).all() and 0 < piece.sum() < len(faces)
    for sel in (piece, ~piece):
        used, inv = np.unique(faces[sel], return_inverse=True)
        fa = inv.reshape(-1, 3)
        assert M.open_edges(fa) == 0 and M.euler(verts[used], fa) == 2 and abs(M.volume(verts[used], fa) - 4.26) < 0.05


def test_near_pair_both_layouts_agree_over_a_mostly_empty_box():
    """the pair moved by (60, 70, 80): 297 x 343 x 390 corners, under the dense cap - the dense restatement runs and must agree"""
    pts, nrm = S.far_pair((60, 70, 80))
    h = M.cell_size(pts)
    verts, faces, info = S.mesh_from_cloud(pts, nrm, h)
    dims, tables = info["dims"], info["tables"]
    assert dims == (297, 343, 390) and np.prod(dims) <= M.MAX_CORNERS
    flags = M.mark(pts, tables)
    assert np.array_equal(S.to_blocks(flags, info["blocks"]), info["flags"]) and flags.sum() == info["flags"].sum()
    f = np.zeros(flags.shape, F)
    s = np.flatnonzero(info["flags"].reshape(-1))
    i, j, k = S.slot_corners(s, info["blocks"], dims)
    f[k, j, i] = info["f"].reshape(-1)[s]
    wverts, wfaces, _ = M.extract(f, flags, tables)
    assert np.array_equal(faces, wfaces) and np.array_equal(verts.view(np.int32), wverts.view(np.int32))
    _closed_pair(verts, faces)
