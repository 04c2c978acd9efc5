"""The surface reconstruction's contract (include/puflow_hip.h, "surface from an oriented cloud") restated on the CPU in numpy:
the corner tables, the cell of a point, the band (pf_recon_mark), the IMLS value in float64 (pf_imls) and marching tetrahedra
with vertices welded by grid-edge id (pf_mtet_count / pf_mtet_emit / pf_mtet_vertices).  Everything but the IMLS value is exact:
the device's flags, vertices (bitwise), faces and their order must equal this.  The test surfaces come from attr_ref."""
import itertools

import numpy as np

F = np.float32
PAD = 3
MAX_CORNERS = 1 << 26
EDGE_CLASSES = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
PERMS = sorted(itertools.permutations(range(3)))          # lexicographic


# ---- grid -----------------------------------------------------------------------------------------------------------------
def sqd(a, b):
    """the unfused fp32 ((dx*dx)+(dy*dy))+(dz*dz) of the searches"""
    d = np.asarray(a, F) - np.asarray(b, F)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def cell_size(pts, scale=1.0):
    """scale * sqrt(lower median over the points of the fp32 squared distance to the 6th nearest other point), in double"""
    p = np.asarray(pts, F)
    d2 = np.sort(sqd(p[:, None], p[None]), axis=1)[:, 6]               # entry 0 is the point itself (or a twin)
    m = np.sort(d2)[(len(d2) - 1) // 2]
    return float(scale) * float(np.sqrt(np.float64(m)))


def grid(lo, hi, h):
    """fp32 box and the cell size -> (dims (D_x, D_y, D_z), [g_x, g_y, g_z] float32 corner tables)"""
    lo, hi, h = np.asarray(lo, F).astype(np.float64), np.asarray(hi, F).astype(np.float64), float(h)
    o = lo - PAD * h
    dims = [int(np.ceil((hi[a] - lo[a]) / h)) + 2 * PAD + 1 for a in range(3)]
    return tuple(dims), [(o[a] + np.arange(dims[a], dtype=np.float64) * h).astype(F) for a in range(3)]


def grid_of(pts, h):
    p = np.asarray(pts, F)
    return grid(p.min(axis=0), p.max(axis=0), h)


def cell(p, g):
    """(number of entries of g that are <= p) - 1, clamped to 0 .. D - 2"""
    return np.clip(np.searchsorted(g, np.asarray(p, F), side="right") - 1, 0, len(g) - 2)


def mark(pts, tables):
    """uint8 flags [D_z, D_y, D_x]: the 4 x 4 x 4 corners cell - 1 .. cell + 2 of every point's cell (inside the box)"""
    p = np.asarray(pts, F)
    D = [len(g) for g in tables]
    flags = np.zeros((D[2], D[1], D[0]), np.uint8)
    c = [cell(p[:, a], tables[a]) for a in range(3)]
    for dz, dy, dx in itertools.product(range(-1, 3), repeat=3):
        i, j, k = c[0] + dx, c[1] + dy, c[2] + dz
        ok = (i >= 0) & (i < D[0]) & (j >= 0) & (j < D[1]) & (k >= 0) & (k < D[2])
        flags[k[ok], j[ok], i[ok]] = 1
    return flags


def corners(flags, tables):
    """the active corners in ascending corner index: (index [Q] int64, coordinates [Q,3] float32)"""
    Dz, Dy, Dx = flags.shape
    c = np.flatnonzero(flags.reshape(-1)).astype(np.int64)
    return c, np.stack([tables[0][c % Dx], tables[1][(c // Dx) % Dy], tables[2][c // (Dx * Dy)]], axis=1)


def active_cells(flags):
    """bool [D_z, D_y, D_x]: cells (by lower corner) whose 8 corners are all flagged; the last index of an axis is no cell"""
    a = np.zeros(flags.shape, bool)
    f = flags != 0
    a[:-1, :-1, :-1] = (f[:-1, :-1, :-1] & f[:-1, :-1, 1:] & f[:-1, 1:, :-1] & f[:-1, 1:, 1:] &
                        f[1:, :-1, :-1] & f[1:, :-1, 1:] & f[1:, 1:, :-1] & f[1:, 1:, 1:])
    return a


# ---- implicit value -------------------------------------------------------------------------------------------------------
def imls(query, pts, normals, idx, sigma_h):
    """f(x) = sum_k w_k n_k.(x - p_k) / sum_k w_k, w_k = exp(-(d2_k - d2_0) / sigma_h^2), in float64 (not rounded to fp32)"""
    x = np.asarray(query, F).astype(np.float64)
    p = np.asarray(pts, F).astype(np.float64)[np.asarray(idx)]           # [Q,K,3]
    n = np.asarray(normals, F).astype(np.float64)[np.asarray(idx)]
    d = x[:, None] - p
    d2 = (d * d).sum(axis=2)
    w = np.exp(-(d2 - d2[:, :1]) / (float(sigma_h) ** 2))
    return (w * (n * d).sum(axis=2)).sum(axis=1) / w.sum(axis=1)


# ---- marching tetrahedra --------------------------------------------------------------------------------------------------
def tet_vertex(tet, v):
    """offset of vertex v of tet `tet` from the cell's lower corner: v0 = 0, v1 = e_p0, v2 = e_p0 + e_p1, v3 = (1, 1, 1)"""
    o = [0, 0, 0]
    for s in range(v if v < 3 else 3):
        o[PERMS[tet][s]] = 1
    return tuple(o)


def _oriented(tet, tri, direction):
    """tri: three edges (vi, vj); swap the last two unless the normal of the midpoints' triangle agrees with `direction`"""
    m = [np.array(tet_vertex(tet, i)) + np.array(tet_vertex(tet, j)) for i, j in tri]          # twice the midpoints
    s = int(np.dot(np.cross(m[1] - m[0], m[2] - m[0]), direction))
    assert s != 0
    return tri if s > 0 else [tri[0], tri[2], tri[1]]


def tet_table():
    """{(tet, mask): [triangle, ...]}, mask bit v = vertex v inside, a triangle = three tet edges (vi, vj) with vi < vj, in the
    order that makes its normal (vertices at the edges' midpoints) point to the outside"""
    edge = lambda i, j: (min(i, j), max(i, j))
    table = {}
    for tet in range(6):
        P = [np.array(tet_vertex(tet, v)) for v in range(4)]
        for mask in range(1, 15):
            ins = [v for v in range(4) if mask >> v & 1]
            out = [v for v in range(4) if not mask >> v & 1]
            if len(ins) == 2:
                (a, b), (c, d) = ins, out
                direction = P[c] + P[d] - P[a] - P[b]
                tris = [[edge(a, c), edge(a, d), edge(b, d)], [edge(a, c), edge(b, d), edge(b, c)]]
            else:
                lone, others = (ins[0], out) if len(ins) == 1 else (out[0], ins)
                direction = (P[others[0]] + P[others[1]] + P[others[2]] - 3 * P[lone]) * (1 if len(ins) == 1 else -1)
                tris = [[edge(lone, o) for o in others]]
            table[tet, mask] = [_oriented(tet, t, direction) for t in tris]
    return table


def _edge_id(c, tet, e, Dx, Dy):
    """id of edge e = (vi, vj) of tet `tet` in the cells with lower corners c: 7 * (owner corner) + class"""
    a, b = tet_vertex(tet, e[0]), tet_vertex(tet, e[1])
    cls = EDGE_CLASSES.index((b[0] - a[0], b[1] - a[1], b[2] - a[2]))
    return 7 * (c + a[0] + a[1] * Dx + a[2] * Dx * Dy) + cls


def tet_masks(f, cells):
    """f [D_z, D_y, D_x], cells: lower corner indices [n] -> masks [n, 6] (bit v: f < 0 at vertex v of the tet)"""
    Dz, Dy, Dx = f.shape
    flat = np.asarray(f, F).reshape(-1)
    masks = np.zeros((len(cells), 6), np.int64)
    for tet in range(6):
        for v in range(4):
            o = tet_vertex(tet, v)
            masks[:, tet] |= (flat[cells + o[0] + o[1] * Dx + o[2] * Dx * Dy] < 0).astype(np.int64) << v
    return masks


def triangles(f, flags):
    """three edge ids per triangle, int64 [T, 3], in the order (cell index, tet, triangle)"""
    Dz, Dy, Dx = f.shape
    cells = np.flatnonzero(active_cells(flags).reshape(-1)).astype(np.int64)
    masks = tet_masks(f, cells)
    table = tet_table()
    keys, ids = [], []
    for (tet, mask), tris in table.items():
        sel = cells[masks[:, tet] == mask]
        for t, tri in enumerate(tris):
            keys.append(np.stack([sel, np.full_like(sel, tet), np.full_like(sel, t)], axis=1))
            ids.append(np.stack([_edge_id(sel, tet, e, Dx, Dy) for e in tri], axis=1))
    keys, ids = np.concatenate(keys), np.concatenate(ids)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return ids[order]


def vertices(edge_ids, f, tables):
    """edge ids [V] -> float32 [V, 3]: g[a] + t * (g[b] - g[a]), t = f_a / (f_a - f_b), every operation rounded to float32"""
    Dz, Dy, Dx = f.shape
    flat = np.asarray(f, F).reshape(-1)
    a, cls = np.asarray(edge_ids, np.int64) // 7, np.asarray(edge_ids, np.int64) % 7
    off = np.array(EDGE_CLASSES, np.int64)[cls]
    ia = np.stack([a % Dx, (a // Dx) % Dy, a // (Dx * Dy)], axis=1)
    ib = ia + off
    fa, fb = flat[a], flat[(ib[:, 2] * Dy + ib[:, 1]) * Dx + ib[:, 0]]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (fa / (fa - fb)).astype(F)
    out = np.empty((len(a), 3), F)
    for ax in range(3):
        ga, gb = tables[ax][ia[:, ax]], tables[ax][ib[:, ax]]
        out[:, ax] = ga + (t * (gb - ga).astype(F)).astype(F)
    return out


def extract(f, flags, tables):
    """-> (verts float32 [V,3] in ascending edge id, faces int32 [T,3], edge ids int64 [V])"""
    tri = triangles(f, flags)
    ids, inv = np.unique(tri.reshape(-1), return_inverse=True)
    return vertices(ids, f, tables), inv.reshape(-1, 3).astype(np.int32), ids


def mesh_from_cloud(pts, normals, h, k=8, sigma=1.0):
    """the whole pipeline on the CPU with a brute-force search by (fp32 distance, index): (verts, faces, info)"""
    pts = np.asarray(pts, F)
    dims, tables = grid_of(pts, h)
    flags = mark(pts, tables)
    c, x = corners(flags, tables)
    idx = np.empty((len(c), k), np.int64)
    for s in range(0, len(c), 4096):                                    # in slabs: [Q, N] would be large
        idx[s:s + 4096] = np.argsort(sqd(x[s:s + 4096, None], pts[None]), axis=1, kind="stable")[:, :k]
    f = np.zeros(flags.shape, F)
    f.reshape(-1)[c] = imls(x, pts, normals, idx, sigma * h).astype(F)
    verts, faces, _ = extract(f, flags, tables)
    return verts, faces, {"h": h, "dims": dims, "flags": flags, "f": f, "tables": tables}


# ---- mesh properties ------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    fa = np.asarray(faces, np.int64)
    return np.concatenate([fa[:, [0, 1]], fa[:, [1, 2]], fa[:, [2, 0]]])


def open_edges(faces):
    """undirected edges used by exactly one triangle"""
    e = np.sort(directed_edges(faces), axis=1)
    _, n = np.unique(e, axis=0, return_counts=True)
    return int((n == 1).sum())


def is_oriented_manifold(faces):
    """every undirected edge is used by exactly two triangles, once in each direction"""
    e = directed_edges(faces)
    V = int(e.max()) + 1
    d = e[:, 0] * V + e[:, 1]
    u, n = np.unique(d, return_counts=True)
    if (n != 1).any():
        return False
    return bool(np.isin(e[:, 1] * V + e[:, 0], u).all())


def euler(verts, faces):
    e = np.unique(np.sort(directed_edges(faces), axis=1), axis=0)
    return len(verts) - len(e) + len(faces)


def volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float((v[:, 0] * np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def sphere_distance(p, r=1.0):
    return np.abs(np.linalg.norm(np.asarray(p, np.float64), axis=1) - r)


def torus_distance(p, R=1.0, r=0.35):
    p = np.asarray(p, np.float64)
    return np.abs(np.hypot(np.hypot(p[:, 0], p[:, 1]) - R, p[:, 2]) - r)


def sphere_field(x, r=1.0):
    return np.linalg.norm(np.asarray(x, np.float64), axis=-1) - r


def torus_field(x, R=1.0, r=0.35):
    x = np.asarray(x, np.float64)
    return np.hypot(np.hypot(x[..., 0], x[..., 1]) - R, x[..., 2]) - r


def disc(n, seed):
    """n points of the flat unit disc z = 0 (an open surface), uniform by area, with the normal (0, 0, 1)"""
    rng = np.random.default_rng(seed)
    r, a = np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
    return np.stack([r * np.cos(a), r * np.sin(a), np.zeros(n)], axis=1).astype(F), np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))
