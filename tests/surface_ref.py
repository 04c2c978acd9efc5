"""float64 numpy restatement of the surface-connected neighbourhoods (the checker of csrc/surface_reach.hip and of
puflow_amd.metrics.surface_reach / disks(reach=) / sampling.surface_pool), by another method than the kernel's relaxation:
d2 per face from the Voronoi-region classification in float64, rounded once to float32; faces sorted by d2 and inserted into a
union-find over faces and welded vertices; b2(f) is the d2 of the insertion that first joins f to the source face's set.
Disks and patch pools follow from D2(q) = max(|q - s|^2, b2(face(q))).  Also the small meshes the tests share."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

INF = np.float32(np.inf)


# ---- d2: squared distance from a point to the closest point of every triangle ----------------------------------------------
def _seg_rel(a, b):
    e = b - a
    ee = (e * e).sum(-1)
    t = np.where(ee > 0, -(a * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0)
    return a + np.clip(t, 0.0, 1.0)[:, None] * e


def _div(num, den):
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def tri_d2(p, tris) -> np.ndarray:
    """[F] float32: |closest point of triangle f - p|^2, the regions tested in the order vertex a, vertex b, edge ab, vertex c,
    edge ac, edge bc, degenerate, face (Ericson 5.1.5), everything relative to p, in float64, rounded once."""
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3) - np.asarray(p, np.float64)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    ab, ac = b - a, c - a
    d1, d2 = -(ab * a).sum(-1), -(ac * a).sum(-1)
    d3, d4 = -(ab * b).sum(-1), -(ac * b).sum(-1)
    d5, d6 = -(ab * c).sum(-1), -(ac * c).sum(-1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    n = np.cross(ab, ac)
    nn = (n * n).sum(-1)
    edges = np.stack([_seg_rel(a, b), _seg_rel(b, c), _seg_rel(c, a)], 1)
    k = (edges ** 2).sum(-1).argmin(1)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0),
             ~(va + vb + vc > 0) | ~(nn > 0)]
    picks = [a, b, a + _div(d1, d1 - d3)[:, None] * ab, c, a + _div(d2, d2 - d6)[:, None] * ac,
             b + _div(d4 - d3, (d4 - d3) + (d5 - d6))[:, None] * (c - b), edges[np.arange(len(t)), k]]
    q = (_div((n * a).sum(-1), nn))[:, None] * n                              # the foot of the normal
    for cond, pick in zip(conds[::-1], picks[::-1]):
        q = np.where(cond[:, None], pick, q)
    out = (q * q).sum(-1)
    # a point next to the plane of a face it projects into (a source on its own face): n . a is all cancellation in float64,
    # so the distance to the plane is taken in exact rational arithmetic there
    for i in np.flatnonzero(~np.any(conds, axis=0) & (out < 1e-12 * (a * a).sum(-1))):
        A, u, w = ([Fraction(float(x)) for x in r] for r in (a[i], ab[i], ac[i]))
        nx, ny, nz = u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]
        out[i] = float((nx * A[0] + ny * A[1] + nz * A[2]) ** 2 / (nx * nx + ny * ny + nz * nz))
    return out.astype(np.float32)


# ---- b2: the bottleneck field, by sorted insertion into a union-find ----------------------------------------------------------
def weld(verts, faces) -> np.ndarray:
    """faces with every vertex replaced by the index of its coordinates among the distinct ones."""
    _, inv = np.unique(np.asarray(verts, np.float32), axis=0, return_inverse=True)
    return inv.reshape(-1)[np.asarray(faces, np.int64)]


def bottleneck(p, f0: int, verts, faces, r_stop=None):
    """(rface [n] int64 ascending, rd2 [n] float32, rb2 [n] float32) of the source p on face f0: the faces with
    d2 <= float32(r_stop^2) (all faces when r_stop is None), their d2 and b2 (+inf when not joined to f0 among them).  An f0
    that is no candidate gives empty arrays."""
    wf = weld(verts, faces)
    F = len(wf)
    d2 = tri_d2(p, np.asarray(verts, np.float32)[np.asarray(faces, np.int64)])
    stop = INF if r_stop is None else np.float32(np.float64(r_stop) * np.float64(r_stop))
    cand = d2 <= stop
    if not (0 <= f0 < F) or not cand[f0]:
        return np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.float32)
    parent = np.arange(F + int(wf.max()) + 1)                                  # faces, then vertices
    members = {}                                                               # root -> faces of the set

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    b2 = np.full(F, INF, np.float32)
    seen_f0 = False
    for f in np.argsort(d2, kind="stable"):
        if not cand[f]:
            break
        f = int(f)
        src_root = find(f0) if seen_f0 else -1
        roots = {find(f)} | {find(F + int(v)) for v in wf[f]}
        big = max(roots, key=lambda r: len(members.get(r, ())))
        fresh = [f]                                                            # the faces that were not in the source's set
        for r in roots:
            if r != src_root:
                fresh += members.get(r, [])
        whole = members.pop(big, [])
        for r in roots:
            if r != big:
                whole += members.pop(r, [])
                parent[r] = big
        whole.append(f)
        members[big] = whole
        seen_f0 |= f == f0
        if seen_f0 and (f == f0 or src_root in roots):
            b2[fresh] = d2[f]                                                  # first joined to the source's set now
    rface = np.flatnonzero(cand)
    return rface, d2[rface], b2[rface]


def field(p, f0, verts, faces) -> np.ndarray:
    """b2 [F] float32 over the whole mesh."""
    return bottleneck(p, f0, verts, faces)[2]


def euclid2(points, s) -> np.ndarray:
    """|q - s|^2 as float32 sums of float32 squares, the seed subtracted first."""
    d = np.asarray(points, np.float32) - np.asarray(s, np.float32)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def surface_d2(points, points_face, s, f0, verts, faces) -> np.ndarray:
    """D2 [N] float32 of every point (on face points_face) from the source s on face f0."""
    return np.maximum(euclid2(points, s), field(s, f0, verts, faces)[np.asarray(points_face, np.int64)])


def disks(mapped, mapped_face, seeds, seed_face, verts, faces, radii):
    """(counts [S,J], offsets [S+1], member [nnz], level [nnz], D [S,N]) of the surface disks: the layout of
    uniform_ref.disks, with D = sqrt(D2) in float64 compared with the radii."""
    radii = np.asarray(radii, np.float64)
    J = len(radii)
    D = np.stack([np.sqrt(surface_d2(mapped, mapped_face, s, int(f0), verts, faces).astype(np.float64))
                  for s, f0 in zip(np.asarray(seeds, np.float32), seed_face)])
    lev = (D[:, :, None] > radii[None, None, :]).sum(-1)
    counts = np.stack([(lev <= j).sum(1) for j in range(J)], 1)
    offsets, member, level = [0], [], []
    for s in range(len(D)):
        idx = np.flatnonzero(lev[s] < J)
        member.append(idx)
        level.append(lev[s, idx])
        offsets.append(offsets[-1] + len(idx))
    return counts, np.array(offsets, np.int64), np.concatenate(member).astype(np.int64), np.concatenate(level).astype(np.int64), D


def patch_pool(samples, sample_face, s, f0, verts, faces, k: int):
    """(idx [k] the samples with the smallest (D2, index), D2 [N], d2 [F] of the faces)."""
    d = surface_d2(samples, sample_face, s, f0, verts, faces)
    return np.lexsort((np.arange(len(d)), d))[:k], d, tri_d2(s, np.asarray(verts, np.float32)[np.asarray(faces, np.int64)])


def radius_margin(D, radii) -> float:
    """The smallest |D^2 - r^2| / r^2 over all finite D and all radii."""
    D = np.asarray(D, np.float64)
    D = D[np.isfinite(D)]
    r2 = np.asarray(radii, np.float64) ** 2
    return float((np.abs(D[:, None] ** 2 - r2[None, :]) / r2[None, :]).min()) if D.size else np.inf


def pool_margin(d, k: int, other=()) -> float:
    """How contested the pool's last place is: the smallest relative distance from the k-th smallest D2 to any value that
    differs from it - among the samples' D2 and `other` (the faces' d2, from which every b2 is taken).  Samples whose D2 is
    the same b2 tie exactly, here and on the GPU, and the index decides; values that differ by less could fall either way."""
    d = np.asarray(d, np.float64)
    last = np.sort(d)[k - 1]
    v = np.concatenate([d, np.asarray(other, np.float64)])
    v = v[np.isfinite(v) & (v != last)]
    return float((np.abs(v - last) / last).min()) if v.size else np.inf


# ---- meshes -----------------------------------------------------------------------------------------------------------------
def grid(nx: int, ny: int, sx: float = 1.0, sy: float = 1.0, z: float = 0.0, x0: float = 0.0, y0: float = 0.0):
    """A flat nx x ny-quad rectangle [x0, x0 + sx] x [y0, y0 + sy] at height z: 2 nx ny faces."""
    x, y = np.meshgrid(x0 + np.linspace(0, sx, nx + 1), y0 + np.linspace(0, sy, ny + 1), indexing="ij")
    verts = np.stack([x, y, np.full_like(x, z)], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    a, b, c, d = i * (ny + 1) + j, (i + 1) * (ny + 1) + j, (i + 1) * (ny + 1) + j + 1, i * (ny + 1) + j + 1
    faces = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3).astype(np.int64)
    return verts, faces


def join(*meshes):
    """Meshes side by side, no vertex shared (equal coordinates weld later)."""
    vs, fs, n = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + n)
        n += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs)


def unwelded(verts, faces):
    """Every face with its own three vertices."""
    return np.asarray(verts, np.float32)[faces].reshape(-1, 3), np.arange(3 * len(faces)).reshape(-1, 3)


def sandwich(gap: float = 0.05, n: int = 8):
    """Two parallel n x n-quad unit sheets, `gap` apart, no shared vertex; faces [0, 2 n^2) are the lower sheet."""
    return join(grid(n, n), grid(n, n, z=gap))


def u_strip(L: float = 2.0, g: float = 0.1, w: float = 0.25, nx: int = 16, ny: int = 2):
    """Two arms [0, L] x [0, w] at z = 0 and z = g, joined only at x = L by a wall of one quad row; faces [0, 2 nx ny) are
    the lower arm, the next 2 nx ny the upper arm, the last 2 ny the wall."""
    lower, upper = grid(nx, ny, L, w), grid(nx, ny, L, w, z=g)
    y = np.linspace(0, w, ny + 1)
    wv = np.concatenate([np.stack([np.full_like(y, L), y, np.zeros_like(y)], -1), np.stack([np.full_like(y, L), y, np.full_like(y, g)], -1)])
    j = np.arange(ny)
    wf = np.concatenate([np.stack([j, j + 1, j + ny + 2], -1), np.stack([j, j + ny + 2, j + ny + 1], -1)])
    return join(lower, upper, (wv, wf))


def sheet_of(mesh_name: str, face) -> np.ndarray:
    """The part (0 lower, 1 upper, 2 wall) a face of `sandwich()` / `u_strip()` with the default sizes belongs to."""
    n = {"sandwich": 128, "u_strip": 64}[mesh_name]
    return np.minimum(np.asarray(face) // n, 2)


# ---- the cases both test files use ---------------------------------------------------------------------------------------------
GAP = 0.03                                     # the sandwich of the disk tests: below r_0 = sqrt(0.004 * 2 / pi) = 0.0505
DISK_POINTS, DISK_SEEDS = 640, 24              # points and seeds of the disk tests on the small meshes
DISK_KEY = 8                                   # Philox key of those seeds (the points: + 50), chosen for the margins
SHEET_SEEDS = 200                              # seeds of the folded-sheet fixture that are restated
PATCH = dict(num_point=16, up_ratio=4, cloud_points=64, n_patches=4, ratio=5)


def strip(n: int = 512):
    """A 1 x n-quad strip (2 n faces) of unit squares."""
    return grid(n, 1, float(n), 1.0)


def small_component():
    """A unit sheet and a 0.2 x 0.2 one far from it: 4 % of the area, too small for a pool of a quarter of the samples."""
    return join(grid(8, 8), grid(2, 2, 0.2, 0.2, x0=3.0))


def stop_margin(p, verts, faces, r_stop) -> float:
    """The smallest |d2 - r_stop^2| / r_stop^2 over the faces: how far the candidate set is from changing."""
    d2 = tri_d2(p, np.asarray(verts, np.float32)[np.asarray(faces, np.int64)]).astype(np.float64)
    return float((np.abs(d2 - r_stop * r_stop) / (r_stop * r_stop)).min())


FIELD_KEY = 23                                 # Philox key of the field tests' sources, chosen for the margins


def field_cases(golden_dir):
    """name -> (verts, faces, r_stop) of the field tests: r_stop 0.37 of the bounding box's diagonal, so that the candidates
    are a proper subset on the larger meshes; the strip is swept whole."""
    import os
    fx = np.load(os.path.join(golden_dir, "eval_uniform.npz"))
    tri = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]]))
    meshes = {"triangle": tri, "quad": grid(1, 1), "grid": grid(8, 8), "u_strip": u_strip(), "sandwich": sandwich(GAP),
              "icosphere": (fx["c0_verts"], fx["c0_faces"].astype(np.int64)), "sheet": (fx["c2_verts"], fx["c2_faces"].astype(np.int64))}
    out = {k: (np.asarray(v, np.float32), f, 0.37 * float(np.linalg.norm(np.ptp(v, axis=0)))) for k, (v, f) in meshes.items()}
    v, f = strip()
    out["strip"] = (v, f, 2.0 * 512)
    return out


def field_sources(name, verts, faces, S):
    """(sources [S,3] float32, faces [S]): area-weighted samples of key FIELD_KEY (what metrics.sample_mesh draws, restated);
    the strip's source is the centroid of its first face, at one end."""
    import uniform_ref as U
    if name == "strip":
        return np.asarray(verts, np.float64)[faces[0]].mean(0).astype(np.float32)[None], np.array([0])
    s, face = U.seeds_from_uniforms(verts, faces, U.uniforms(FIELD_KEY, S))
    return s.astype(np.float32), face


# ---- pools whose last place lies beyond the first stop -----------------------------------------------------------------------
POOL_KEY = {"sandwich": 41, "u_strip": 42}         # Philox keys of the seeds of the direct surface_pool test, chosen so that
                                                   # taking the first k finite values inside the first stop picks wrong samples
POOL_SEEDS, POOL_SET, POOL_K = 12, 320, 80         # seeds, samples (key + 1) and pool size of that test


def first_stop(samples, s, k: int) -> float:
    """The radius surface_pool starts from: the Euclidean distance of the min(2k, n)-th nearest sample."""
    d = np.sort(euclid2(samples, s).astype(np.float64))
    return float(np.sqrt(d[min(2 * k, len(d)) - 1]))


def shown_d2(samples, sample_face, s, f0, verts, faces, r_stop) -> np.ndarray:
    """D2 as it shows with the field computed inside r_stop only: faces that are no candidates, or not reached, give +inf."""
    rf, _, rb2 = bottleneck(s, f0, verts, faces, r_stop)
    b2 = np.full(len(faces), INF, np.float32)
    b2[rf] = rb2
    return np.maximum(euclid2(samples, s), b2[np.asarray(sample_face, np.int64)])


def pool_case(mesh: str):
    """(verts, faces, samples, sample_face, seeds, seed_face) of the direct surface_pool test."""
    import uniform_ref as U
    v, f = sandwich() if mesh == "sandwich" else u_strip()
    s, sf = U.seeds_from_uniforms(v, f, U.uniforms(POOL_KEY[mesh], POOL_SEEDS))
    q, qf = U.seeds_from_uniforms(v, f, U.uniforms(POOL_KEY[mesh] + 1, POOL_SET))
    return v, f, q.astype(np.float32), qf, s.astype(np.float32), sf


def order_defects(got, d) -> int:
    """How many places of the selection `got` are out of the (D2, index) order of the values d: a value more than 1e-6 below
    its predecessor's, or an index below its predecessor's where the two values are equal bits.  (Values that differ by less
    than 1e-6 may fall either way between two roundings of |q - s|^2.)"""
    v = np.asarray(d, np.float64)[got]
    return int(((v[1:] < v[:-1] * (1 - 1e-6)) | ((v[1:] == v[:-1]) & (np.asarray(got)[1:] < np.asarray(got)[:-1]))).sum())
