"""float64 numpy restatements of the evaluation metrics (the checkers of puflow_amd.metrics): approx-match EMD with any level
schedule, point-to-triangle distance, the sphere-clipped occupancy grid and its JSD, the reference's normalisations and
the OFF / mesh helpers the fixtures and tests share.  Written from the algorithms' statements, not from the reference's code."""
from __future__ import annotations

import numpy as np


# ---- normalisation --------------------------------------------------------------------------------------------------------
def normalize(pc: np.ndarray) -> np.ndarray:
    """Centroid to the origin, furthest point at distance 1 (per cloud, pc [..., N, 3])."""
    pc = np.asarray(pc, dtype=np.float64)
    c = pc - pc.mean(axis=-2, keepdims=True)
    return c / np.sqrt((c ** 2).sum(-1)).max(-1)[..., None, None]


# ---- approx-match EMD -----------------------------------------------------------------------------------------------------
def approx_match_cost(a: np.ndarray, b: np.ndarray, top: int = 7) -> float:
    """Multi-level soft assignment of a [n,3] to b [m,3]; returns sum_kl w_kl |a_k - b_l| / n."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    n, m = len(a), len(b)
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    dist = np.sqrt(d2)
    satL = np.full(n, float(max(n, m) // n))
    satR = np.full(m, float(max(n, m) // m))
    cost = 0.0
    for j in range(top, -3, -1):
        level = 0.0 if j == -2 else -(4.0 ** j)
        e = np.exp(level * d2)
        s = 1e-9 + e @ satR
        ratio = satL / s
        ss = 1e-9 + satR * (ratio @ e)
        r = np.minimum(satR / ss, 1.0)
        w = e * ratio[:, None] * (satR * r)[None, :]
        satL = np.maximum(satL - w.sum(1), 0.0)
        satR = np.maximum(satR - w.sum(0), 0.0)
        cost += (w * dist).sum()
    return cost / n


# ---- point to triangle ----------------------------------------------------------------------------------------------------
def _seg_d2(a, b):
    e = b - a
    ee = (e * e).sum(-1)
    t = np.where(ee > 0, -(a * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    q = a + t[..., None] * e
    return (q * q).sum(-1)


def point_triangle_d2(p: np.ndarray, tris: np.ndarray) -> np.ndarray:
    """Squared distance of the point p [3] to every triangle of tris [F,3,3], by projecting onto the plane and, where the
    projection falls outside the triangle, taking the closest of the three edges."""
    t = np.asarray(tris, dtype=np.float64) - np.asarray(p, dtype=np.float64)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    nrm = np.cross(b - a, c - a)
    nn = (nrm * nrm).sum(-1)
    ok = nn > 0
    nns = np.where(ok, nn, 1.0)
    h = (nrm * a).sum(-1) / nns                          # the projection of the origin is h * nrm
    q = h[:, None] * nrm
    inside = ok.copy()
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(u - q, v - q) * nrm).sum(-1) >= 0
    face = h * h * nn
    edges = np.minimum(np.minimum(_seg_d2(a, b), _seg_d2(b, c)), _seg_d2(c, a))
    return np.where(inside, face, edges)


def point_mesh_dist(points: np.ndarray, verts: np.ndarray, faces: np.ndarray) -> np.ndarray:
    tris = np.asarray(verts, dtype=np.float64)[np.asarray(faces)]
    return np.array([np.sqrt(point_triangle_d2(p, tris).min()) for p in np.asarray(points, dtype=np.float64)])


# ---- occupancy grid and JSD -----------------------------------------------------------------------------------------------
def sphere_grid(resolution: int = 28) -> np.ndarray:
    """Centres of a resolution^3 grid over [-0.5, 0.5]^3 (float32, i-major), those with norm <= 0.5."""
    ax = (np.arange(resolution, dtype=np.float64) * (1.0 / float(resolution - 1)) - 0.5).astype(np.float32)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    return g[np.linalg.norm(g, axis=1) <= 0.5]


def nearest_cells(pc: np.ndarray, grid: np.ndarray):
    """(index of the nearest cell, squared-distance gap to the second nearest) of every point, in float64."""
    d = ((np.asarray(pc, np.float64)[:, None, :] - np.asarray(grid, np.float64)[None, :, :]) ** 2).sum(-1)
    part = np.partition(d, 1, axis=1)
    return d.argmin(1), part[:, 1] - part[:, 0]


def occupancy(pc: np.ndarray, resolution: int = 28) -> np.ndarray:
    grid = sphere_grid(resolution)
    idx, _ = nearest_cells(pc, grid)
    return np.bincount(idx, minlength=len(grid)).astype(np.float64)


def jsd_counts(P: np.ndarray, Q: np.ndarray) -> float:
    """Jensen-Shannon divergence (base 2) of two histograms."""
    p = P / P.sum()
    q = Q / Q.sum()

    def h(x):
        x = x[x > 0]
        return -(x * np.log2(x)).sum()
    return float(h((p + q) / 2.0) - (h(p) + h(q)) / 2.0)


# ---- meshes ---------------------------------------------------------------------------------------------------------------
def write_off(path, verts, faces) -> None:
    """Vertices written as the exact decimal of their float32 values (a double parser reads the same numbers)."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    with open(path, "w") as f:
        f.write(f"OFF\n{len(v)} {len(faces)} 0\n")
        f.write("".join("%.17g %.17g %.17g\n" % tuple(r) for r in v))
        f.write("".join("3 %d %d %d\n" % tuple(t) for t in np.asarray(faces)))


def write_points(path, pts) -> None:
    p = np.asarray(pts, dtype=np.float32).astype(np.float64)
    with open(path, "w") as f:
        f.write("".join("%.17g %.17g %.17g\n" % tuple(r) for r in p))


def icosphere(subdiv: int):
    t = (1.0 + 5 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    faces = list(f)
    for _ in range(subdiv):
        cache, nf = {}, []

        def mid(i, j):
            k = (min(i, j), max(i, j))
            if k not in cache:
                m = verts[i] + verts[j]
                verts.append(m / np.linalg.norm(m))
                cache[k] = len(verts) - 1
            return cache[k]
        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nf
    return np.array(verts), np.array(faces, dtype=np.int64)


def torus(nu: int, nv: int, R: float = 1.0, r: float = 0.35, bump: float = 0.0):
    u = np.arange(nu) * 2 * np.pi / nu
    v = np.arange(nv) * 2 * np.pi / nv
    U, V = np.meshgrid(u, v, indexing="ij")
    rr = r * (1.0 + bump * np.sin(5 * U) * np.cos(3 * V))
    verts = np.stack([(R + rr * np.cos(V)) * np.cos(U), (R + rr * np.cos(V)) * np.sin(U), rr * np.sin(V)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return verts, faces


def sheet(nx: int = 24, ny: int = 16, seed: int = 3, degenerate: bool = True):
    """A thin folded (non-convex) double-sided sheet with a few sliver triangles (and two zero-area ones: `degenerate`)."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.linspace(-1, 1, nx), np.linspace(-0.6, 0.6, ny), indexing="ij")
    z = 0.3 * np.sin(3 * x) * np.cos(2 * y)
    top = np.stack([x, y, z + 0.01], -1).reshape(-1, 3)
    bot = np.stack([x, y, z - 0.01], -1).reshape(-1, 3)
    verts = np.concatenate([top, bot])
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a, b, c, d = i * ny + j, (i + 1) * ny + j, (i + 1) * ny + j + 1, i * ny + j + 1
    q = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    faces = np.concatenate([q, q[:, ::-1] + nx * ny])
    n0 = len(verts)
    sl = rng.uniform(-0.8, 0.8, (6, 3)) * [1, 1, 0.2]
    extra = []
    for k, p in enumerate(sl):                                   # slivers: one long edge, a tiny height
        extra += [p, p + [0.5, 0.02, 0.0], p + [0.25, 0.01, 1e-4 * (k + 1)]]
    if degenerate:
        extra += [[0.1, 0.2, 0.5], [0.3, 0.2, 0.5], [0.2, 0.2, 0.5]]  # collinear
        extra += [[-0.3, 0.1, 0.45]] * 3                             # a point
    verts = np.concatenate([verts, np.array(extra, dtype=np.float64)])
    faces = np.concatenate([faces, np.arange(n0, len(verts)).reshape(-1, 3)])
    return verts, faces


def sample_surface(verts, faces, n: int, rng) -> np.ndarray:
    tri = np.asarray(verts, np.float64)[faces]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    f = rng.choice(len(faces), n, p=area / area.sum())
    u, v = rng.random(n), rng.random(n)
    flip = u + v > 1
    u[flip], v[flip] = 1 - u[flip], 1 - v[flip]
    t = tri[f]
    return t[:, 0] + u[:, None] * (t[:, 1] - t[:, 0]) + v[:, None] * (t[:, 2] - t[:, 0])
