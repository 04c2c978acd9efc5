"""numpy restatement of the uniform grid of triangles and its ring search (puflow_amd/csrc/tri_grid.hip): the box, g, h and the
cell function in the kernel's own float32 operations, the set of triangles per cell, the oversize list, and the search with its
stopping rule and tie rule.  Distances are float64 (eval_ref.point_triangle_d2), so the winners are compared with a full scan
of the SAME float64 distances under the same tie rule - this checks the grid and the stopping rule, not the fp32 distance.

Grid rule (the header's): g = the smallest integer with g^3 >= 2 F, at most 256, cells along the longest extent of the fp32 box
of all vertices; h = max(extent / g, 2^-19 x the largest |coordinate|, 2^-100); G_a = cell_a(hi_a) + 1; a triangle is registered
in every cell of the block cell(min corner) .. cell(max corner); more than 64 cells: the oversize list."""
from __future__ import annotations

import numpy as np

import eval_ref as R

F32 = np.float32
GMAX, CELLS_PER_TRI, MAXCELLS, SEED = 256, 2, 64, 64


def axis_cells(F: int) -> int:
    g = 1
    while g < GMAX and g * g * g < CELLS_PER_TRI * F:
        g += 1
    return g


def cell(x, lo, inv_h, G):
    """kg_cell: clamp(floor((x - lo) * inv_h), 0, G - 1), every operation rounded to float32"""
    t = np.floor((np.asarray(x, F32) - F32(lo)).astype(F32) * F32(inv_h)).astype(F32)
    return np.clip(t, F32(0), F32(G - 1)).astype(np.int64)


def build(tris):
    """tris float32 [F,9] -> the grid: lo, h, inv_h, amax, G (x, y, z), c0 / c1 [F,3] (every triangle's block of cells), over
    (ascending indices of the oversize triangles) and cells {linear cell index (x fastest): sorted triangle indices}"""
    tris = np.ascontiguousarray(tris, F32).reshape(-1, 9)
    F = tris.shape[0]
    v = tris.reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    g = axis_cells(F)
    e = F32(np.max((hi - lo).astype(F32)))
    ma = F32(max(np.abs(lo).max(), np.abs(hi).max()))
    h = F32(e / F32(g))
    h = max(h, F32(ma * F32(2.0 ** -19)))
    h = F32(max(h, F32(2.0 ** -100)))
    inv_h = F32(F32(1) / h)
    G = [int(cell(hi[a], lo[a], inv_h, g)) + 1 for a in range(3)]
    c = np.stack([np.stack([cell(tris[:, 3 * k + a], lo[a], inv_h, G[a]) for a in range(3)], -1) for k in range(3)], 0)
    c0, c1 = c.min(0), c.max(0)
    n = np.prod(c1 - c0 + 1, axis=1)
    over = np.nonzero(n > MAXCELLS)[0]
    cells = {}
    for f in np.nonzero(n <= MAXCELLS)[0]:
        for z in range(c0[f, 2], c1[f, 2] + 1):
            for y in range(c0[f, 1], c1[f, 1] + 1):
                for x in range(c0[f, 0], c1[f, 0] + 1):
                    cells.setdefault((z * G[1] + y) * G[0] + x, []).append(int(f))
    return dict(lo=lo, h=h, inv_h=inv_h, amax=ma, G=G, c0=c0, c1=c1, over=over, cells=cells, F=F,
                pairs=int(n[n <= MAXCELLS].sum()))


def face_bound(q, lo, h, inv_h, G, c, r):
    """kg_face_bound in float32: (lower bound of the squared gap to the unvisited cells of one axis, an interior face exists)"""
    b, face = F32(np.inf), False
    q, lo, h = F32(q), F32(lo), F32(h)
    lc, hc = c - r, c + r
    if lc > 0:
        face = True
        E = F32(lo + F32(F32(lc) * h))
        E = F32(E + F32(max(abs(lo), abs(E)) * F32(2.0 ** -20)))
        gap = F32(q - E)
        b = min(b, F32(gap * gap) if (int(cell(E, lo, inv_h, G)) >= lc and gap > 0) else F32(0))
    if hc < G - 1:
        face = True
        E = F32(lo + F32(F32(hc + 1) * h))
        E = F32(E - F32(max(abs(lo), abs(E)) * F32(2.0 ** -20)))
        gap = F32(E - q)
        b = min(b, F32(gap * gap) if (int(cell(E, lo, inv_h, G)) <= hc and gap > 0) else F32(0))
    return b, face


def seed_window(p: int, P: int, F: int, seed=None):
    c = int(seed[p]) if seed is not None else p * F // P
    c = min(max(c, 0), F - 1)
    f0 = max(c - SEED // 2, 0)
    return c, f0, min(f0 + SEED, F)


def _update(state, d, idx):
    """candidates (d [n], idx [n]) against (best, face, from_seed): d < best wins and clears from_seed; d == best wins only when
    not from_seed and the index is lower.  Order-free: the lexicographic minimum of what beats the state."""
    best, face, from_seed = state
    wins = (d < best) | ((d == best) & (not from_seed) & (idx < face))
    if not wins.any():
        return state
    d, idx = d[wins], idx[wins]
    k = np.lexsort((idx, d))[0]
    return float(d[k]), int(idx[k]), False


def _seed_state(q, t3, p, P, seed):
    F = t3.shape[0]
    c, f0, f1 = seed_window(p, P, F, seed)
    d = R.point_triangle_d2(q, t3[f0:f1])
    k = int(np.argmin(d))                                   # the first minimiser
    return (float(d[k]), f0 + k, True) if np.isfinite(d[k]) else (np.inf, c, True), f1 - f0


def full_scan(pts, tris, seed=None):
    """the winners of the tie rule over ALL triangles: the seed window's first minimiser unless a triangle is strictly nearer,
    then the lowest index of the nearest"""
    t3 = np.asarray(tris, F32).reshape(-1, 3, 3)
    out = np.empty(len(pts), np.int64)
    for p, q in enumerate(np.asarray(pts, F32)):
        state, _ = _seed_state(q, t3, p, len(pts), seed)
        out[p] = _update(state, R.point_triangle_d2(q, t3), np.arange(t3.shape[0]))[1]
    return out


def search(grid, pts, tris, seed=None):
    """(face [P], cand [P]) of the ring search; cand counts the seed window, the oversize list and every pair of the rings"""
    t3 = np.asarray(tris, F32).reshape(-1, 3, 3)
    pts = np.asarray(pts, F32)
    lo, h, inv_h, G, cells = grid["lo"], grid["h"], grid["inv_h"], grid["G"], grid["cells"]
    face, cand = np.empty(len(pts), np.int64), np.empty(len(pts), np.int64)
    for p, q in enumerate(pts):
        state, n = _seed_state(q, t3, p, len(pts), seed)
        ov = grid["over"]
        if len(ov):
            state = _update(state, R.point_triangle_d2(q, t3[ov]), ov)
        n += len(ov)
        c = [int(cell(q[a], lo[a], inv_h, G[a])) for a in range(3)]
        sc = F32(max(np.abs(q).max(), grid["amax"])) * F32(2.0 ** -19)
        for r in range(GMAX + 1):
            rng = [(max(c[a] - r, 0), min(c[a] + r, G[a] - 1)) for a in range(3)]
            ids = []
            for z in range(rng[2][0], rng[2][1] + 1):
                for y in range(rng[1][0], rng[1][1] + 1):
                    for x in range(rng[0][0], rng[0][1] + 1):
                        if max(abs(x - c[0]), abs(y - c[1]), abs(z - c[2])) == r:
                            ids += cells.get((z * G[1] + y) * G[0] + x, [])
            if ids:
                ids = np.array(ids, np.int64)
                state = _update(state, R.point_triangle_d2(q, t3[ids]), ids)
                n += len(ids)
            bounds = [face_bound(q[a], lo[a], h, inv_h, G[a], c[a], r) for a in range(3)]
            if not any(b[1] for b in bounds):
                break
            if float(min(b[0] for b in bounds)) > state[0] * (1.0 + 2.0 ** -12) + float(sc) * float(sc):
                break
        face[p], cand[p] = state[1], n
    return face, cand


# ---- the fixtures the CPU and the GPU tests share ---------------------------------------------------------------------------
def tris_of(verts, faces) -> np.ndarray:
    return np.asarray(verts, F32)[np.asarray(faces)].reshape(-1, 9)


def with_spanning_triangles(verts, faces):
    """the mesh plus two triangles across its whole box (oversize whatever the grid)"""
    v = np.asarray(verts, F32)
    lo, hi = v.min(0), v.max(0)
    extra = np.array([[lo[0], lo[1], lo[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], hi[2]],
                      [hi[0], lo[1], lo[2]], [lo[0], hi[1], lo[2]], [hi[0], hi[1], hi[2]]], F32)
    n0 = len(v)
    return np.concatenate([v, extra]), np.concatenate([np.asarray(faces), np.arange(n0, n0 + 6).reshape(2, 3)])


def flat_mesh(n: int = 12):
    """a triangulated square in the plane z = 0.25: one axis of zero extent"""
    x, y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-0.5, 0.7, n), indexing="ij")
    v = np.stack([x, y, np.full_like(x, 0.25)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a, b, c, d = i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1
    return v, np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])


def ulp_mesh(nu: int = 24, nv: int = 12):
    """a torus whose vertex coordinates sit one float32 ulp below, on and above the faces of its own grid's cells"""
    v, f = R.torus(nu, nv)
    v = v.astype(F32)
    g = build(tris_of(v, f))
    k = np.arange(len(v))
    for a in range(3):
        edge = (g["lo"][a] + np.round((v[:, a] - g["lo"][a]) / g["h"]).astype(F32) * g["h"]).astype(F32)
        edge = np.clip(edge, v[:, a].min(), v[:, a].max())                    # the box, hence the grid, stays what it was
        moved = np.where(k % 3 == 0, np.nextafter(edge, F32(-np.inf)), np.where(k % 3 == 1, edge, np.nextafter(edge, F32(np.inf))))
        v[:, a] = np.clip(moved, v[:, a].min(), v[:, a].max()).astype(F32)
    return v, f


def pruning_fixture():
    """(verts, faces, points [4096,3]) of the pruned-search fixture: a 102 400-face bumpy torus, 4096 noisy surface points of
    which the first 64 are uniform in [-2, 2]^3"""
    v, f = R.torus(320, 160, bump=0.15)
    rng = np.random.default_rng(9)
    p = R.sample_surface(v, f, 4096, rng) + rng.normal(0, 0.02, (4096, 3))
    p[:64] = rng.uniform(-2, 2, (64, 3))
    return v.astype(F32), f, p.astype(F32)
