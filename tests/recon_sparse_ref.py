"""The block-sparse layout of the reconstruction (include/puflow_hip.h, "the same surface in a block-sparse layout") restated on
the CPU in numpy with int64 keys: block keys per point, the distinct list, links, block flags, and the extraction in global
order.  Built on recon_ref's cell rule, tet table, edge classes and vertex arithmetic; nothing here is as large as the box.
Everything is exact: the device's arrays and its mesh must equal this, and this must equal recon_ref wherever that one runs."""
import itertools

import numpy as np

import recon_ref as M

F = np.float32
B = 8
SLOTS = B * B * B
MAX_AXIS = 1 << 20
MAX_BLOCKS = 1 << 21


def block_dims(dims):
    return tuple((int(d) + B - 1) // B for d in dims)


def dims_of(tables):
    return tuple(len(g) for g in tables)


def key_of(bi, bj, bk, nb):
    return (np.asarray(bk, np.int64) * nb[1] + bj) * nb[0] + bi


def slot_of(i, j, k):
    return (k & 7) << 6 | (j & 7) << 3 | (i & 7)


# ---- layout ---------------------------------------------------------------------------------------------------------------
def block_keys(pts, tables):
    """int64 [N, 8]: entry ox | oy << 1 | oz << 2 is the block of the first (0) / last (1) of the point's 4 corners per axis"""
    p = np.asarray(pts, F)
    dims = dims_of(tables)
    nb = block_dims(dims)
    lo, hi = [], []
    for a in range(3):
        c = M.cell(p[:, a], tables[a]).astype(np.int64)
        lo.append(np.maximum(c - 1, 0) >> 3)
        hi.append(np.minimum(c + 2, dims[a] - 1) >> 3)
    keys = np.empty((len(p), 8), np.int64)
    for o in range(8):
        keys[:, o] = key_of((hi if o & 1 else lo)[0], (hi if o & 2 else lo)[1], (hi if o & 4 else lo)[2], nb)
    return keys


def block_list(keys):
    return np.unique(np.asarray(keys, np.int64).reshape(-1))


def block_coords(blocks, nb):
    blocks = np.asarray(blocks, np.int64)
    return blocks % nb[0], (blocks // nb[0]) % nb[1], blocks // (nb[0] * nb[1])


def find(blocks, keys):
    """positions of keys in the ascending list, -1 where absent"""
    keys = np.asarray(keys, np.int64)
    at = np.minimum(np.searchsorted(blocks, keys), len(blocks) - 1)
    return np.where(blocks[at] == keys, at, -1).astype(np.int64)


def links(blocks, dims):
    """int32 [NB, 8]: the list positions of the blocks at offsets {0,1}^3, -1 where the list or the grid has none"""
    nb = block_dims(dims)
    bi, bj, bk = block_coords(blocks, nb)
    out = np.empty((len(blocks), 8), np.int32)
    for o in range(8):
        ni, nj, nk = bi + (o & 1), bj + (o >> 1 & 1), bk + (o >> 2 & 1)
        inside = (ni < nb[0]) & (nj < nb[1]) & (nk < nb[2])
        out[:, o] = np.where(inside, find(blocks, key_of(ni, nj, nk, nb)), -1)
    assert (out[:, 0] == np.arange(len(blocks))).all()
    return out


def mark(pts, tables, blocks):
    """uint8 flags [NB, 512]: recon_ref.mark's corners, stored by block (a corner in no listed block is skipped)"""
    p = np.asarray(pts, F)
    dims = dims_of(tables)
    nb = block_dims(dims)
    flags = np.zeros((len(blocks), SLOTS), np.uint8)
    c = [M.cell(p[:, a], tables[a]).astype(np.int64) for a in range(3)]
    for dz, dy, dx in itertools.product(range(-1, 3), repeat=3):
        i, j, k = c[0] + dx, c[1] + dy, c[2] + dz
        ok = (i >= 0) & (i < dims[0]) & (j >= 0) & (j < dims[1]) & (k >= 0) & (k < dims[2])
        i, j, k = i[ok], j[ok], k[ok]
        b = find(blocks, key_of(i >> 3, j >> 3, k >> 3, nb))
        flags[b[b >= 0], slot_of(i, j, k)[b >= 0]] = 1
    return flags


def slot_corners(slots, blocks, dims):
    """slot numbers (512 b + slot) -> the corners' global (i, j, k)"""
    slots = np.asarray(slots, np.int64)
    bi, bj, bk = block_coords(np.asarray(blocks, np.int64)[slots >> 9], block_dims(dims))
    s = slots & 511
    return bi * B + (s & 7), bj * B + (s >> 3 & 7), bk * B + (s >> 6)


def to_blocks(dense, blocks):
    """dense [D_z, D_y, D_x] -> [NB, 512] over this list; slots beyond the grid are 0"""
    dims = (dense.shape[2], dense.shape[1], dense.shape[0])
    i, j, k = slot_corners(np.arange(len(blocks) * SLOTS), blocks, dims)
    ok = (i < dims[0]) & (j < dims[1]) & (k < dims[2])
    out = np.zeros(len(blocks) * SLOTS, dense.dtype)
    out[ok] = dense[k[ok], j[ok], i[ok]]
    return out.reshape(-1, SLOTS)


def from_blocks(block_array, blocks, dims):
    """[NB, 512] -> dense [D_z, D_y, D_x], 0 outside the listed blocks (small grids only)"""
    i, j, k = slot_corners(np.arange(len(blocks) * SLOTS), blocks, dims)
    ok = (i < dims[0]) & (j < dims[1]) & (k < dims[2])
    out = np.zeros((dims[2], dims[1], dims[0]), block_array.dtype)
    out[k[ok], j[ok], i[ok]] = block_array.reshape(-1)[ok]
    return out


def corners(flags, blocks, tables):
    """the flagged slots in ascending slot number: (slot numbers [Q] int64, coordinates [Q,3] float32)"""
    s = np.flatnonzero(flags.reshape(-1)).astype(np.int64)
    i, j, k = slot_corners(s, blocks, dims_of(tables))
    return s, np.stack([tables[0][i], tables[1][j], tables[2][k]], axis=1)


# ---- extraction -------------------------------------------------------------------------------------------------------------
def _corner_slots(slots, lnk, off, blocks, dims):
    """the slot numbers of the corners at +off of the corners `slots`, through the links; -1: no such corner in the layout"""
    b, s = slots >> 9, slots & 511
    x, y, z = (s & 7) + off[0], (s >> 3 & 7) + off[1], (s >> 6) + off[2]
    n = lnk[b, (x >> 3) | (y >> 3) << 1 | (z >> 3) << 2].astype(np.int64)
    i, j, k = slot_corners(slots, blocks, dims)
    inside = (i + off[0] < dims[0]) & (j + off[1] < dims[1]) & (k + off[2] < dims[2])
    return np.where((n >= 0) & inside, n * SLOTS + slot_of(x, y, z), -1)


def active_cells(flags, blocks, lnk, dims):
    """slot numbers of the cells (by lower corner) whose 8 corners are all flagged, with their corners' slot numbers [n, 2, 2, 2]"""
    flat = flags.reshape(-1)
    slots = np.flatnonzero(flat).astype(np.int64)
    cs = np.empty((len(slots), 2, 2, 2), np.int64)                      # [z, y, x]
    ok = np.ones(len(slots), bool)
    for oz, oy, ox in itertools.product(range(2), repeat=3):
        c = _corner_slots(slots, lnk, (ox, oy, oz), blocks, dims)
        ok &= (c >= 0) & (flat[np.maximum(c, 0)] != 0)
        cs[:, oz, oy, ox] = c
    return slots[ok], cs[ok]


def triangles(f, flags, blocks, lnk, dims):
    """three edge ids (7 x global owner corner + class) per triangle, int64 [T, 3], in the order (GLOBAL cell index, tet, triangle)"""
    cells, cs = active_cells(flags, blocks, lnk, dims)
    i, j, k = slot_corners(cells, blocks, dims)
    c = (k * dims[1] + j) * dims[0] + i
    inside = np.asarray(f, F).reshape(-1)[cs] < 0                       # [n, z, y, x]
    table = M.tet_table()
    keys, ids = [], []
    for tet in range(6):
        mask = np.zeros(len(cells), np.int64)
        for v in range(4):
            o = M.tet_vertex(tet, v)
            mask |= inside[:, o[2], o[1], o[0]].astype(np.int64) << v
        for m in range(1, 15):
            sel = c[mask == m]
            for t, tri in enumerate(table[tet, m]):
                keys.append(np.stack([sel, np.full_like(sel, tet), np.full_like(sel, t)], axis=1))
                ids.append(np.stack([M._edge_id(sel, tet, e, dims[0], dims[1]) for e in tri], axis=1))
    keys, ids = np.concatenate(keys), np.concatenate(ids)
    return ids[np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))]


def vertices(edge_ids, f, blocks, lnk, tables):
    """recon_ref.vertices over the block layout: f_a by a search of the owner's block, f_b through its link; (0, 0, 0) where a
    corner lies in no listed block"""
    dims = dims_of(tables)
    nb = block_dims(dims)
    flat = np.asarray(f, F).reshape(-1)
    a, cls = np.asarray(edge_ids, np.int64) // 7, np.asarray(edge_ids, np.int64) % 7
    off = np.array(M.EDGE_CLASSES, np.int64)[cls]
    ia = np.stack([a % dims[0], (a // dims[0]) % dims[1], a // (dims[0] * dims[1])], axis=1)
    ib = ia + off
    ba = find(blocks, key_of(ia[:, 0] >> 3, ia[:, 1] >> 3, ia[:, 2] >> 3, nb))
    d = (ib >> 3) - (ia >> 3)
    bb = np.where(ba >= 0, lnk[np.maximum(ba, 0), d[:, 0] | d[:, 1] << 1 | d[:, 2] << 2], -1).astype(np.int64)
    ok = (bb >= 0) & (ib < np.array(dims)).all(axis=1)
    fa = flat[np.maximum(ba, 0) * SLOTS + slot_of(ia[:, 0], ia[:, 1], ia[:, 2])]
    fb = flat[np.maximum(bb, 0) * SLOTS + slot_of(ib[:, 0], ib[:, 1], ib[:, 2])]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (fa / (fa - fb)).astype(F)
    out = np.zeros((len(a), 3), F)
    for ax in range(3):
        ga, gb = tables[ax][ia[:, ax]], tables[ax][np.minimum(ib[:, ax], dims[ax] - 1)]
        out[:, ax] = np.where(ok, ga + (t * (gb - ga).astype(F)).astype(F), F(0))
    return out


def extract(f, flags, blocks, lnk, tables):
    """-> (verts float32 [V,3] in ascending edge id, faces int32 [T,3], edge ids int64 [V], the triangles' edge ids [T,3])"""
    tri = triangles(f, flags, blocks, lnk, dims_of(tables))
    ids, inv = np.unique(tri.reshape(-1), return_inverse=True)
    return vertices(ids, f, blocks, lnk, tables), inv.reshape(-1, 3).astype(np.int32), ids, tri


def layout_of(pts, tables):
    """(blocks, links, flags) of a cloud"""
    blocks = block_list(block_keys(pts, tables))
    return blocks, links(blocks, dims_of(tables)), mark(pts, tables, blocks)


def mesh_from_cloud(pts, normals, h, k=8, sigma=1.0, f=None):
    """the whole pipeline on the CPU over the block layout; f: the implicit value [NB, 512] to use (the device's), default a
    brute-force search by (fp32 distance, index) and recon_ref.imls"""
    pts = np.asarray(pts, F)
    dims, tables = M.grid_of(pts, h)
    blocks, lnk, flags = layout_of(pts, tables)
    if f is None:
        s, x = corners(flags, blocks, tables)
        idx = np.empty((len(s), k), np.int64)
        for a in range(0, len(s), 4096):
            idx[a:a + 4096] = np.argsort(M.sqd(x[a:a + 4096, None], pts[None]), axis=1, kind="stable")[:, :k]
        f = np.zeros(flags.shape, F)
        f.reshape(-1)[s] = M.imls(x, pts, normals, idx, sigma * h).astype(F)
    verts, faces, _, _ = extract(f, flags, blocks, lnk, tables)
    return verts, faces, {"h": h, "dims": dims, "flags": flags, "f": f, "tables": tables, "blocks": blocks, "links": lnk}


def far_pair(shift):
    """two copies of attr_ref.sphere(512, .), seeds 11 and 13, the second moved by `shift` in fp32, with analytic normals"""
    import attr_ref as R
    (a, na), (b, nb) = R.sphere(512, 11), R.sphere(512, 13)
    return np.concatenate([a, (b + np.asarray(shift, F)).astype(F)]), np.concatenate([na, nb]).astype(F)
