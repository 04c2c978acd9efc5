"""A triangle mesh from an oriented cloud (DESIGN.md 8e "Surface from an oriented cloud"; the contract is in puflow_hip.h).

Three stages, all on the device (csrc/recon.hip): a narrow band of grid corners around the points, an IMLS value - a weighted
mean of signed tangent-plane distances to the `k` nearest oriented points (pf_knn_grid) - at those corners, and its zero set by
marching tetrahedra.  Vertices are welded by grid-edge id, so a closed surface comes out closed, and the mesh is the same bytes
from run to run.  There is no CPU path.

  verts, faces, info = mesh_from_cloud(points, normals)       # [N,3], [N,3] -> [V,3] float32, [F,3] int32, {h, dims, open_edges, ..}
  mesh_from_cloud(points, normals, layout="sparse")           # the same mesh from 8 x 8 x 8 blocks around the band (csrc/
                                                              # recon_sparse.hip): nothing is as large as the box; "auto": dense
                                                              # while the box is within the dense cap, else sparse
  mesh_from_cloud(points, normals, close_holes=4)             # up to 4 rounds of band growth where the zero set leaves the band
                                                              # (pf_recon_grow): holes up to about 8 cells wider than the band close
  f = implicit(points, normals, query, h=cell_size(points))   # the implicit value at any points
  python -m puflow_amd.reconstruct --source DIR --target DIR  # every x y z nx ny nz file of DIR -> <name>.off
"""
from __future__ import annotations

import os
from argparse import ArgumentParser

import numpy as np
import torch

from . import _lib, ops

PAD = 3                                 # corners of margin on every side of the cloud's box: keeps the band inside
MAX_CORNERS = _lib.PF_RECON_MAX_CORNERS
CELL_NEIGHBOUR = 6                      # the cell size follows the distance to this nearest OTHER point
BLOCK = _lib.PF_RECON_BLOCK             # the sparse layout: corners per axis of a block, ...
SLOTS = BLOCK ** 3                      # ... corners of a block, ...
MAX_AXIS = _lib.PF_RECON_SPARSE_MAX_AXIS        # ... corners per axis of its virtual grid ...
MAX_BLOCKS = _lib.PF_RECON_SPARSE_MAX_BLOCKS    # ... and listed blocks
LAYOUTS = ("dense", "sparse", "auto")
GROW_MAX_ROUNDS = _lib.PF_RECON_GROW_MAX_ROUNDS  # band growth: rounds, each with one more corner of padding per side


def _cloud(points, normals, what: str):
    for t, name in ((points, "points"), (normals, "normals")):
        if t is None:
            continue
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.PuflowHipError(f"{what}: {name} is a GPU tensor (no CPU path)")
        if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] <= 0:
            raise _lib.PuflowHipError(f"{what}: {name} [N,3], got {tuple(t.shape)}")
    if normals is not None and normals.shape != points.shape:
        raise _lib.PuflowHipError(f"{what}: one normal per point, got {tuple(points.shape)} and {tuple(normals.shape)}")
    return ops._f32c(points), (ops._f32c(normals) if normals is not None else None)


def _k(k, n: int, what: str) -> int:
    k = int(k)
    if not 1 <= k <= _lib.PF_KNN_GRID_MAX_K or k > n:
        raise _lib.PuflowHipError(f"{what}: k = {k} neighbours in a cloud of {n} points; 1 .. {_lib.PF_KNN_GRID_MAX_K} (and at most "
                                  "the cloud) are supported")
    return k


def _positive(v, name: str, what: str) -> float:
    v = float(v)
    if not (v > 0.0 and np.isfinite(v)):
        raise _lib.PuflowHipError(f"{what}: {name} = {v} is not a positive number")
    return v


def _stats(points: torch.Tensor, want_median: bool):
    """(median squared distance to the 6th nearest other point or None, lo [3], hi [3]) of a cloud, float32 values as float64, from
    ONE host read"""
    parts = [points.min(dim=0).values, points.max(dim=0).values]
    if want_median:
        n = points.shape[0]
        if n <= CELL_NEIGHBOUR:
            raise _lib.PuflowHipError(f"cell_size: a cloud of {n} points has no {CELL_NEIGHBOUR}th neighbour; give the cell size")
        _, d2 = ops.knn_grid(points[None], points[None], CELL_NEIGHBOUR + 1)
        parts.append(torch.median(d2[0, :, CELL_NEIGHBOUR]).reshape(1))       # the lower median
    host = torch.cat(parts).cpu().numpy().astype(np.float64)
    return (float(host[6]) if want_median else None), host[0:3], host[3:6]


def cell_size(points: torch.Tensor, scale: float = 1.0) -> float:
    """scale x sqrt(m), m the lower median over the points of the fp32 squared distance to the 6th nearest other point"""
    points, _ = _cloud(points, None, "cell_size")
    m, _lo, _hi = _stats(points, True)
    return _positive(scale, "scale", "cell_size") * float(np.sqrt(m))


def _layout(layout, what: str) -> str:
    if layout not in LAYOUTS:
        raise _lib.PuflowHipError(f"{what}: layout is one of {', '.join(LAYOUTS)}, got {layout!r}")
    return layout


def _rounds(close_holes, what: str) -> int:
    if isinstance(close_holes, bool) or not isinstance(close_holes, (int, np.integer)) or not 0 <= close_holes <= GROW_MAX_ROUNDS:
        raise _lib.PuflowHipError(f"{what}: close_holes = {close_holes!r} is no whole number of rounds in 0 .. {GROW_MAX_ROUNDS}")
    return int(close_holes)


def _growth_is_dense(layout: str, rounds: int, what: str, how: str) -> None:
    """the one decision about growth and layouts: band growth (pf_recon_grow) is written against dense addresses, so a call that
    asks for rounds on the sparse layout is refused - in the caller's words: `how` names its way to the dense layout"""
    if rounds and layout == "sparse":
        raise _lib.PuflowHipError(f"{what}: close_holes = {rounds}: growth needs the dense layout{how}; a grown block list is not built")


def _box(cells, rounds: int = 0) -> str:
    return " x ".join(str(int(c) + 2 * (PAD + rounds) + 1) if np.isfinite(c) else "inf" for c in cells)


def _within_dense_cap(cells, rounds: int = 0) -> bool:
    pad = 2 * (PAD + rounds) + 1
    return bool((cells < MAX_CORNERS).all()) and int(cells[0] + pad) * int(cells[1] + pad) * int(cells[2] + pad) <= MAX_CORNERS


def corner_tables(lo, hi, h: float, layout: str = "dense", rounds: int = 0):
    """the fp32 box and the cell size -> ((D_x, D_y, D_z), three float32 numpy tables g_a[i] = float32(o_a + (i - rounds) h)).
    layout "dense": at most PF_RECON_MAX_CORNERS corners in the box; "sparse": at most PF_RECON_SPARSE_MAX_AXIS per axis; "auto":
    either.  rounds: that many more corners of padding per side for band growth (close_holes), dense only."""
    layout, rounds = _layout(layout, "corner_tables"), _rounds(rounds, "corner_tables")
    _growth_is_dense(layout, rounds, "reconstruct", " (--layout dense, or auto)")
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    o = lo - PAD * h
    cells = np.ceil((hi - lo) / h)
    unsupported = _lib.load().pf_error_string(_lib.PF_ERR_UNSUPPORTED).decode()
    dense = _within_dense_cap(cells, rounds)
    if rounds and not dense:
        raise _lib.PuflowHipError(
            f"reconstruct: close_holes = {rounds}: growth needs the dense layout"
            f", and the padded box of {_box(cells, rounds)} corners at cell size {h:.6g} is over its cap of {MAX_CORNERS} "
            f"({unsupported}): use a larger --cell (or --cell_scale) or fewer rounds")
    if layout == "dense" and not dense:
        raise _lib.PuflowHipError(
            f"reconstruct: a box of {_box(cells)} corners at "
            f"cell size {h:.6g} is over the cap of {MAX_CORNERS} ({unsupported}): "
            "use a larger --cell (or --cell_scale) or --layout sparse")
    if not (layout == "dense" or (layout == "auto" and dense) or (cells + 2 * PAD + 1 <= MAX_AXIS).all()):      # inf, nan: over
        raise _lib.PuflowHipError(
            f"reconstruct: a grid of {_box(cells)} corners at cell size {h:.6g} is over the sparse layout's cap of {MAX_AXIS} per "
            f"axis ({unsupported}): use a larger --cell (or --cell_scale)")
    dims = tuple(int(c) + 2 * (PAD + rounds) + 1 for c in cells)
    return dims, [(o[a] + (np.arange(dims[a], dtype=np.float64) - rounds) * h).astype(np.float32) for a in range(3)]


def implicit(points: torch.Tensor, normals: torch.Tensor, query: torch.Tensor, k: int = 8, sigma: float = 1.0, h: float = None):
    """The IMLS value at query [Q,3]: f = sum_k w_k n_k.(x - p_k) / sum_k w_k over the k nearest points, w_k = exp(-(d2_k - d2_0) /
    (sigma h)^2), in double on the device, float32 [Q].  h: the cell size (default: cell_size(points))."""
    points, normals = _cloud(points, normals, "implicit")
    if not torch.is_tensor(query) or not query.is_cuda or query.dim() != 2 or query.shape[1] != 3 or query.shape[0] <= 0:
        raise _lib.PuflowHipError("implicit: query is a GPU tensor [Q,3] (no CPU path)")
    k = _k(k, points.shape[0], "implicit")
    h = cell_size(points) if h is None else _positive(h, "h", "implicit")
    return _values(None, points, normals, ops._f32c(query), k, _positive(sigma, "sigma", "implicit") * h)


def _open_edges(faces: torch.Tensor, nv: int) -> torch.Tensor:
    """undirected mesh edges used by exactly one triangle, counted on the device (a 0-dim tensor)"""
    a = torch.cat([faces[:, 0], faces[:, 1], faces[:, 2]])
    b = torch.cat([faces[:, 1], faces[:, 2], faces[:, 0]])
    _, n = torch.unique(torch.minimum(a, b) * nv + torch.maximum(a, b), return_counts=True)
    return (n == 1).sum()


# ---- the block-sparse layout's index arithmetic (the contract is in puflow_hip.h) ----------------------------------------------
def block_dims(dims):
    """(D_x, D_y, D_z) -> blocks per axis (NB_x, NB_y, NB_z)"""
    return tuple((int(d) + BLOCK - 1) // BLOCK for d in dims)


def slot_corners(slots: torch.Tensor, blocks: torch.Tensor, dims):
    """slot numbers int64 [Q] (512 b + slot), the block list -> the corners' (i, j, k), three int64 [Q]"""
    nbx, nby, _ = block_dims(dims)
    key, s = blocks[slots >> 9], slots & (SLOTS - 1)
    return ((key % nbx) * BLOCK + (s & 7), ((key // nbx) % nby) * BLOCK + ((s >> 3) & 7), (key // (nbx * nby)) * BLOCK + (s >> 6))


def dense_to_blocks(dense: torch.Tensor, blocks: torch.Tensor) -> torch.Tensor:
    """a dense [D_z, D_y, D_x] array -> its block form [NB, 512] over this block list; slots beyond the grid are 0"""
    dims = (int(dense.shape[2]), int(dense.shape[1]), int(dense.shape[0]))
    slots = torch.arange(blocks.shape[0] * SLOTS, dtype=torch.int64, device=dense.device)
    i, j, k = slot_corners(slots, blocks, dims)
    inside = (i < dims[0]) & (j < dims[1]) & (k < dims[2])
    out = torch.zeros((blocks.shape[0] * SLOTS,), dtype=dense.dtype, device=dense.device)
    out[inside] = dense.reshape(-1)[((k * dims[1] + j) * dims[0] + i)[inside]]
    return out.reshape(-1, SLOTS)


def blocks_to_dense(block_array: torch.Tensor, blocks: torch.Tensor, dims) -> torch.Tensor:
    """a block array [NB, 512] -> the dense [D_z, D_y, D_x] array, 0 outside the listed blocks (tests and small grids: this one
    IS as large as the box)"""
    slots = torch.arange(blocks.shape[0] * SLOTS, dtype=torch.int64, device=block_array.device)
    i, j, k = slot_corners(slots, blocks, dims)
    inside = (i < dims[0]) & (j < dims[1]) & (k < dims[2])
    out = torch.zeros((dims[2] * dims[1] * dims[0],), dtype=block_array.dtype, device=block_array.device)
    out[((k * dims[1] + j) * dims[0] + i)[inside]] = block_array.reshape(-1)[inside]
    return out.reshape(dims[2], dims[1], dims[0])


def block_list(points: torch.Tensor, tables):
    """the layout of a cloud: (blocks int64 [NB], the ascending distinct keys of the blocks its band touches; links int32 [NB, 8])"""
    blocks = torch.unique(ops.recon_block_keys(points, tables).reshape(-1))          # sorted
    if blocks.shape[0] > MAX_BLOCKS:
        raise _lib.PuflowHipError(
            f"reconstruct: the band touches {blocks.shape[0]} blocks of {BLOCK}^3 corners, over the cap of {MAX_BLOCKS} "
            f"({_lib.load().pf_error_string(_lib.PF_ERR_UNSUPPORTED).decode()}): use a larger --cell (or --cell_scale)")
    return blocks, ops.recon_block_links(blocks, tuple(int(t.shape[0]) for t in tables))


# ---- the seam: the flag and value at a corner, in this layout -----------------------------------------------------------------
# A layout holds the corner tables and what addresses its flags / f arrays, and provides mark(points) -> flags, corners(index) ->
# the (i, j, k) of entries of those arrays, triangles(f, flags, stage) -> the triangles' edge ids [T, 3] in the mesh's order
# (ascending global cell, tet, triangle; None: no triangle), vertices(edge, f) and blocks (0 for dense).  Values, extraction
# and mesh_from_cloud are written once on top of that.  Band growth is not part of it: pf_recon_grow reads dense addresses, and a
# layout whose block list grows with the band is not built (_growth_is_dense).
def _call(_name, thunk):
    return thunk()


class _Dense:
    """arrays [D_z, D_y, D_x] over the box"""
    blocks = 0

    def __init__(self, tables, dims):
        self.tables, self.dims = tables, dims

    def mark(self, points):
        return ops.recon_mark(points, self.tables)

    def corners(self, index):
        Dx, Dy, _ = self.dims
        return index % Dx, (index // Dx) % Dy, index // (Dx * Dy)

    def triangles(self, f, flags, stage=_call):
        def count():
            n = ops.mtet_count(f, flags)
            incl = torch.cumsum(n.reshape(-1), dim=0)
            return (incl - n.reshape(-1)).reshape(n.shape), int(incl[-1])   # a size: the triangle array's
        first, total = stage("count", count)
        return stage("emit", lambda: ops.mtet_emit(f, flags, first, total)) if total else None

    def vertices(self, edge, f):
        return ops.mtet_vertices(edge, f, self.tables)


class _Blocks:
    """arrays [NB, 512] over the listed 8 x 8 x 8 blocks: keys, the ascending block list, and its links"""

    def __init__(self, tables, dims, keys, links):
        self.tables, self.dims, self.keys, self.links, self.blocks = tables, dims, keys, links, int(keys.shape[0])

    def mark(self, points):
        return ops.recon_mark_sparse(points, self.tables, self.keys)

    def corners(self, index):
        return slot_corners(index, self.keys, self.dims)

    def triangles(self, f, flags, stage=_call):
        def count():
            n = ops.mtet_count_sparse(f, flags, self.keys, self.links, self.dims).reshape(-1)
            slots = torch.nonzero(n).reshape(-1)                            # block-major: not the order of the mesh
            if slots.shape[0] == 0:                                         # a size
                return None, None, 0
            i, j, k = self.corners(slots)
            _, order = torch.sort((k * self.dims[1] + j) * self.dims[0] + i)                        # distinct keys: the order is determined
            cells = slots[order]
            n = n[cells].to(torch.int64)
            incl = torch.cumsum(n, dim=0)
            return cells, incl - n, int(incl[-1])                           # a size: the triangle array's
        cells, first, total = stage("count", count)
        if not total:
            return None
        return stage("emit", lambda: ops.mtet_emit_sparse(f, flags, self.keys, self.links, self.dims, cells, first, total))

    def vertices(self, edge, f):
        return ops.mtet_vertices_sparse(edge, f, self.keys, self.links, self.tables)


def _values(layout, points, normals, index, k: int, sigma_h: float, stage=_call):
    """the IMLS value at entries `index` of a layout's arrays (layout None: at the points `index` [Q,3] themselves), float32 [Q]"""
    if layout is None:
        query = index
    else:
        i, j, kk = layout.corners(index)
        query = torch.stack([layout.tables[0][i], layout.tables[1][j], layout.tables[2][kk]], dim=1)
    idx, _ = stage("K search", lambda: ops.knn_grid(points[None], query[None], k))
    return stage("IMLS", lambda: ops.imls(query, points, normals, idx[0], sigma_h))


def _extract(layout, f: torch.Tensor, flags: torch.Tensor, stage=_call):
    """marching tetrahedra over the active cells -> (verts float32 [V,3] in ascending edge id, faces int64 [T,3] in the order
    (global cell, tet, triangle))"""
    ids = layout.triangles(f, flags, stage)
    if ids is None:
        return torch.zeros((0, 3), dtype=torch.float32, device=f.device), torch.zeros((0, 3), dtype=torch.int64, device=f.device)
    edge, inverse = stage("unique", lambda: torch.unique(ids.reshape(-1), sorted=True, return_inverse=True))
    return stage("vertices", lambda: layout.vertices(edge, f)), inverse.reshape(-1, 3)


def extract(f: torch.Tensor, flags: torch.Tensor, tables):
    """marching tetrahedra over the active cells: f float32 / flags uint8 [D_z, D_y, D_x], the corner tables (device) ->
    (verts float32 [V,3] in ascending edge id, faces int64 [T,3] in the order (cell, tet, triangle))"""
    return _extract(_Dense(tables, tuple(int(t.shape[0]) for t in tables)), f, flags)


def extract_sparse(f: torch.Tensor, flags: torch.Tensor, blocks: torch.Tensor, links: torch.Tensor, tables):
    """extract() over the block layout: f float32 / flags uint8 [NB, 512], the block list and its links, the corner tables
    (device) -> the same (verts, faces): triangles in ascending GLOBAL cell index, then tet, then triangle"""
    return _extract(_Blocks(tables, tuple(int(t.shape[0]) for t in tables), blocks, links), f, flags)


# ---- closing holes: the band grows at its exits (the rule is in puflow_hip.h) ---------------------------------------------------
EXITS_CHUNK = 1 << 17                   # new corners per pass of the exit count: its index tensors are [chunk, 8, 8] int64


def _exits(f: torch.Tensor, born: torch.Tensor, corners) -> list:
    """the exits of every round, counted ONCE after the last round, for info["grown_cells"] only (what grows is pf_recon_grow's
    business).  born int8 [D_z, D_y, D_x]: the round that flagged a corner (0: the band of the points, 127: never), so the flags
    round r saw are born < r; f: the final values - a round reads f at the corners of cells active by then, and those never
    change.  corners: per round r = 1, 2, .. the indices of its new corners.  Every exit has a new corner, so the candidates are
    the 8 cells around each new corner - torch gathers over [Q, 8], nothing over the box - and a cell counts at its first new
    corner.  One host read."""
    Dz, Dy, Dx = born.shape
    dev = born.device
    bits = torch.arange(8, device=dev)
    off = torch.stack([bits & 1, (bits >> 1) & 1, bits >> 2], dim=1)                           # [8, 3]: x, y, z of corner b
    stride = torch.tensor([1, Dx, Dx * Dy], device=dev)
    last = torch.tensor([Dx - 2, Dy - 2, Dz - 2], device=dev)                                  # the last cell of an axis
    flat, values, size = born.reshape(-1), f.reshape(-1), born.numel()
    count = torch.zeros(len(corners) + 1, dtype=torch.int64, device=dev)
    every = torch.cat(corners)
    rounds = torch.cat([torch.full((c.shape[0],), r, dtype=torch.int64, device=dev) for r, c in enumerate(corners, 1)])
    for corner, r in zip(every.split(EXITS_CHUNK), rounds.split(EXITS_CHUNK)):
        cell = torch.stack([corner % Dx, (corner // Dx) % Dy, corner // (Dx * Dy)], dim=1)[:, None] - off       # [Q, 8, 3]
        is_cell = ((cell >= 0) & (cell <= last)).all(dim=2)
        cell = torch.minimum(cell.clamp(min=0), last)                                          # clamped: every gather stays inside
        at = (cell[:, :, None] + off).mul(stride).sum(dim=3)                                   # [Q, 8, 8]: the cell's corners
        when = flat[at]
        own = when < r[:, None, None]
        first = ~((when == r[:, None, None]) & (bits[None, :] < bits[:, None])).any(dim=2)     # no new corner before corner b
        crossed = torch.zeros_like(is_cell)
        for a in range(3):
            for s in (0, 1):
                face = [b for b in range(8) if (b >> a) & 1 == s]                              # the four corners on that side
                n = cell[:, :, a] + (2 * s - 1)
                far = (at[:, :, face] + (2 * s - 1) * stride[a]).clamp(0, size - 1)            # the neighbour's other four
                active = own[:, :, face].all(dim=2) & (flat[far] < r[:, None, None]).all(dim=2) & (n >= 0) & (n <= last[a])
                inside = (values[at[:, :, face]] < 0).sum(dim=2)
                crossed |= active & (inside != 0) & (inside != 4)
        count.index_add_(0, r, (is_cell & ~own.all(dim=2) & crossed & first).sum(dim=1))
    return count[1:].tolist()


def mesh_from_cloud(points: torch.Tensor, normals: torch.Tensor, cell: float = None, cell_scale: float = 1.0, k: int = 8,
                    sigma: float = 1.0, layout: str = "dense", close_holes: int = 0, *, _stage=None):
    """points, normals [N,3] on the GPU (unit normals with consistent signs: estimate_normals(..., orient="propagate") or a
    scanner's) -> (verts [V,3] float32, faces [F,3] int32, info).  cell: the grid's cell size; default cell_scale x the median
    distance to the 6th nearest other point.  layout: "dense" - arrays over the cloud's box, refused over PF_RECON_MAX_CORNERS;
    "sparse" - 8 x 8 x 8 blocks around the band, the same mesh bit for bit, nothing allocated by the size of the box; "auto" -
    dense while the box is within the dense cap, else sparse.  info: h, dims (D_x, D_y, D_z), layout (the one used), blocks (0
    for dense) and open_edges, the number of mesh edges used by one triangle only - 0 for a closed surface; a cell below the
    sampling spacing tears holes, and a scan's real boundary stays one.  close_holes = R (0 .. PF_RECON_GROW_MAX_ROUNDS, dense
    layout): up to R rounds in which the band grows by the cells into which the zero set leaves it (pf_recon_grow) - a hole
    shrinks from all sides by at most a cell per round, a real boundary moves outward by at most R cells and stays one; the
    filled patch follows the nearest points' tangent planes.  info then has grow_rounds, the rounds that added something, and
    grown_cells, the exits of each.  R = 0 is the call without it, byte for byte.
    _stage (the timing tools' hook): a callable (name, thunk) -> thunk() that every stage runs through, in this order - "cell-size
    search", "block list" (sparse), "mark", "compaction", "K search", "IMLS"; per round of growth "grow", "compaction" and, if the
    round added corners, "K search", "IMLS"; then "count" and, if there are triangles, "emit", "unique", "vertices"."""
    points, normals = _cloud(points, normals, "mesh_from_cloud")
    k = _k(k, points.shape[0], "mesh_from_cloud")
    sigma = _positive(sigma, "sigma", "mesh_from_cloud")
    layout, rounds = _layout(layout, "mesh_from_cloud"), _rounds(close_holes, "mesh_from_cloud")
    _growth_is_dense(layout, rounds, "mesh_from_cloud",
                     " (layout=\"dense\", or \"auto\" while the padded box is within the dense cap)")
    stage = _call if _stage is None else _stage
    given = cell is not None                                                # the cell size, or a scale of the cloud's spacing
    size = _positive(cell, "cell", "mesh_from_cloud") if given else _positive(cell_scale, "cell_scale", "mesh_from_cloud")
    m, lo, hi = stage("cell-size search", lambda: _stats(points, not given))
    h = size if given else _positive(size * float(np.sqrt(m)), "the cell size from the cloud's spacing", "mesh_from_cloud")
    if layout == "auto":
        layout = "dense" if rounds or _within_dense_cap(np.ceil((hi - lo) / h)) else "sparse"      # growth: dense, or refused
    dims, host_tables = corner_tables(lo, hi, h, layout, rounds)
    tables = [torch.from_numpy(t).to(points.device) for t in host_tables]
    grid = _Dense(tables, dims) if layout == "dense" else _Blocks(tables, dims, *stage("block list", lambda: block_list(points, tables)))
    flags = stage("mark", lambda: grid.mark(points))
    f = torch.empty(flags.shape, dtype=torch.float32, device=points.device)                        # read at flagged corners only
    index = stage("compaction", lambda: torch.nonzero(flags.reshape(-1)).reshape(-1))              # ascending
    f.reshape(-1)[index] = _values(grid, points, normals, index, k, sigma * h, stage)
    born, grown = None, []
    for r in range(1, rounds + 1):                                          # rounds: on the dense layout only (refused above)
        added = stage("grow", lambda: ops.recon_grow(f, flags))
        index = stage("compaction", lambda: torch.nonzero((added & ~flags).reshape(-1)).reshape(-1))   # its size: a round's one host read
        if index.shape[0] == 0:                                             # no new corner, no exit
            break
        if born is None:
            born = (flags == 0).to(torch.int8) * 127
        born.reshape(-1)[index] = r
        grown.append(index)
        f.reshape(-1)[index] = _values(grid, points, normals, index, k, sigma * h, stage)
        flags |= added
    grown = _exits(f, born, grown) if grown else []
    verts, faces = _extract(grid, f, flags, stage)
    open_edges = int(_open_edges(faces, verts.shape[0])) if faces.shape[0] else 0
    return verts, faces.to(torch.int32), {"h": h, "dims": dims, "open_edges": open_edges, "layout": layout, "blocks": grid.blocks,
                                          "grow_rounds": len(grown), "grown_cells": grown}


def write_off(path, verts, faces) -> None:
    """an OFF file: vertex rows as save_xyz formats them (%.6f), face rows `3 a b c`"""
    import ctypes
    verts = np.ascontiguousarray(verts.detach().cpu().numpy() if torch.is_tensor(verts) else verts, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces.detach().cpu().numpy() if torch.is_tensor(faces) else faces).reshape(-1, 3)
    with open(path, "wb") as fh:
        fh.write(b"OFF\n%d %d 0\n" % (len(verts), len(faces)))
        if len(verts):
            lib = _lib.load()
            cap = lib.pf_format_xyz_bound(len(verts), 3)
            buf = ctypes.create_string_buffer(cap)
            m = lib.pf_format_xyz(verts.ctypes.data, len(verts), 3, ctypes.addressof(buf), cap)
            if m < 0:
                _lib.check(int(m), "pf_format_xyz")
            fh.write(memoryview(buf)[:m])
        fh.write((("3 %d %d %d\n" * len(faces)) % tuple(faces.ravel().tolist())).encode())


OPEN_EDGES_LINE = ("{name}: {n} open edges - the mesh has a boundary: the cell ({h:.6g}) is below the sampling spacing somewhere "
                   "(try a larger --cell or --cell_scale), or the scan really ends there")


@torch.no_grad()
def reconstruct_files(paths, target: str, cell=None, cell_scale: float = 1.0, k: int = 8, sigma: float = 1.0,
                      normal_column: int = 4, device="cuda:0", layout: str = "dense", close_holes: int = 0):
    from .upsample import load_xyz
    c0 = int(normal_column) - 1
    if c0 < 3:
        raise SystemExit("--normal_column is the 1-based first column of the normal, after x y z: 4 or more")
    clouds = []
    for p in sorted(paths):
        rows = np.atleast_2d(load_xyz(p))
        if rows.shape[1] < c0 + 3:
            raise SystemExit(f"{p}: {rows.shape[1]} columns, no normal in columns {c0 + 1} .. {c0 + 3}; write oriented normals with "
                             "--estimate_normals K --normals_orient propagate (upsample / upsample_cnf)")
        clouds.append((p, rows))
    os.makedirs(target, exist_ok=True)
    out = []
    for p, rows in clouds:
        xyz = torch.from_numpy(np.ascontiguousarray(rows[:, :3])).to(device)
        nrm = torch.from_numpy(np.ascontiguousarray(rows[:, c0:c0 + 3])).to(device)
        nrm = nrm / nrm.norm(dim=1, keepdim=True).clamp_min(1e-30)          # six printed decimals are not unit length
        verts, faces, info = mesh_from_cloud(xyz, nrm, cell=cell, cell_scale=cell_scale, k=k, sigma=sigma, layout=layout,
                                             close_holes=close_holes)
        name = os.path.splitext(os.path.basename(p))[0] + ".off"
        write_off(os.path.join(target, name), verts, faces)
        if info["open_edges"] > 0:
            print(OPEN_EDGES_LINE.format(name=name, n=info["open_edges"], h=info["h"]), flush=True)
        out.append((os.path.join(target, name), info))
    return out


def main(argv=None):
    parser = ArgumentParser(description="x y z nx ny nz clouds of a directory -> <name>.off triangle meshes")
    parser.add_argument("--source", type=str, required=True, help="Path of input directory")
    parser.add_argument("--target", type=str, required=True, help="Path of output directory")
    size = parser.add_mutually_exclusive_group()
    size.add_argument("--cell", type=float, default=None, help="the grid's cell size")
    size.add_argument("--cell_scale", type=float, default=1.0,
                      help="cell size as a multiple of the median distance to the 6th nearest other point")
    parser.add_argument("--k", type=int, default=8, help="oriented points per implicit value")
    parser.add_argument("--sigma", type=float, default=1.0, help="width of the weights, in cells")
    parser.add_argument("--normal_column", type=int, default=4, help="1-based first column of the normal")
    parser.add_argument("--layout", type=str, default="dense", choices=LAYOUTS,
                        help="dense: arrays over the cloud's box; sparse: blocks around the band, for a box that is mostly empty; "
                             "auto: dense while the box is within the dense cap")
    parser.add_argument("--close_holes", type=int, default=0, metavar="R",
                        help=f"up to R (0 .. {GROW_MAX_ROUNDS}) rounds of band growth where the surface leaves the band: a hole closes "
                             "by a cell per round from every side, a real boundary moves out by at most R cells; dense layout only")
    args = parser.parse_args(argv)
    paths = []
    for root, _dirs, files in os.walk(args.source):
        paths.extend([os.path.join(root, f) for f in files if ".xyz" in f])
    reconstruct_files(paths, args.target, cell=args.cell, cell_scale=args.cell_scale, k=args.k, sigma=args.sigma,
                      normal_column=args.normal_column, layout=args.layout, close_holes=args.close_holes)


if __name__ == "__main__":
    main()
