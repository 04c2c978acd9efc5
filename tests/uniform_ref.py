"""float64 numpy restatement of the uniformity measure (the checker of puflow_amd.metrics' uniformity functions and of
csrc/eval_uniform.hip): radii from the mesh area, seeds from given uniforms, closest points on the mesh, brute-force
Euclidean disks, brute-force nearest neighbour inside every disk, and the statistic of the reference's analyze_uniform
(evaluation/evaluate.py:116-165) written from its definition.  No sklearn, like tests/eval_ref.py."""
from __future__ import annotations

import numpy as np

import philox_ref as PH

PERCENTAGES = np.array([0.004, 0.006, 0.008, 0.010, 0.012])


def area_radii(verts, faces, percentages=PERCENTAGES):
    """(radii [J], cumulative areas [F]): r_j = sqrt(p_j A / pi)."""
    t = np.asarray(verts, np.float64)[np.asarray(faces)]
    cum = np.cumsum(0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1))
    return np.sqrt(np.asarray(percentages, np.float64) * cum[-1] / np.pi), cum


def uniforms(seed: int, S: int) -> np.ndarray:
    """[S,3] float32: the words x0 x1 x2 of Philox-4x32-10 with key `seed` and counter (s, 0, 0, 0), mapped to (0, 1)."""
    return PH.u01(PH.draw(seed, 0, 0, np.arange(S))[:, :3], np.float32)


def seed_faces(cum, u0):
    """The first face whose cumulative area exceeds u0 A (the last face when none does)."""
    return np.minimum(np.searchsorted(cum, np.asarray(u0, np.float64) * cum[-1], side="right"), len(cum) - 1)


def seeds_from_uniforms(verts, faces, u):
    """(seeds [S,3] float64, face [S]): area-weighted face from u[:,0], then (1 - sqrt u1) a + sqrt u1 (1 - u2) b + sqrt u1 u2 c."""
    u = np.asarray(u, np.float64)
    _, cum = area_radii(verts, faces)
    f = seed_faces(cum, u[:, 0])
    t = np.asarray(verts, np.float64)[np.asarray(faces)[f]]
    r = np.sqrt(u[:, 1])
    return (1 - r)[:, None] * t[:, 0] + (r * (1 - u[:, 2]))[:, None] * t[:, 1] + (r * u[:, 2])[:, None] * t[:, 2], f


def _seg_closest(p, a, b):
    e = b - a
    ee = (e * e).sum(-1)
    t = np.where(ee > 0, ((p - a) * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0)
    return a + np.clip(t, 0.0, 1.0)[:, None] * e


def closest_on_triangles(p, tris):
    """The closest point of every triangle of tris [F,3,3] to p [3]: the foot of the normal where it falls inside, else the
    closest of the closest points of the three edges."""
    p = np.asarray(p, np.float64)
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    nrm = np.cross(b - a, c - a)
    nn = (nrm * nrm).sum(-1)
    ok = nn > 0
    foot = p - (((p - a) * nrm).sum(-1) / np.where(ok, nn, 1.0))[:, None] * nrm
    inside = ok.copy()
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(u - foot, v - foot) * nrm).sum(-1) >= 0
    cand = np.stack([_seg_closest(p, a, b), _seg_closest(p, b, c), _seg_closest(p, c, a)], 1)          # [F,3,3]
    k = ((cand - p) ** 2).sum(-1).argmin(1)
    edge = cand[np.arange(len(tris)), k]
    return np.where(inside[:, None], foot, edge)


def closest_points(points, verts, faces):
    """(closest point [P,3], its face [P], distance [P]) of every point to the mesh, by brute force."""
    tris = np.asarray(verts, np.float64)[np.asarray(faces)]
    out, face, dist = [], [], []
    for p in np.asarray(points, np.float64):
        q = closest_on_triangles(p, tris)
        d2 = ((q - p) ** 2).sum(-1)
        f = int(d2.argmin())
        out.append(q[f])
        face.append(f)
        dist.append(np.sqrt(d2[f]))
    return np.array(out), np.array(face), np.array(dist)


def seed_distances(mapped, seeds):
    """[S,N] Euclidean distances."""
    m, s = np.asarray(mapped, np.float64), np.asarray(seeds, np.float64)
    return np.sqrt(((s[:, None, :] - m[None, :, :]) ** 2).sum(-1))


def disks(mapped, seeds, radii):
    """(counts [S,J], offsets [S+1], member [nnz], level [nnz]): per seed the points within the largest radius in ascending
    index, each with the smallest j whose ball holds it; counts[s, j] = members with level <= j."""
    d = seed_distances(mapped, seeds)
    radii = np.asarray(radii, np.float64)
    lev = (d[:, :, None] > radii[None, None, :]).sum(-1)                  # radii ascending: the number of balls it is outside of
    J = len(radii)
    counts = np.stack([(lev <= j).sum(1) for j in range(J)], 1)
    offsets, member, level = [0], [], []
    for s in range(len(d)):
        idx = np.flatnonzero(lev[s] < J)
        member.append(idx)
        level.append(lev[s, idx])
        offsets.append(offsets[-1] + len(idx))
    return counts, np.array(offsets, np.int64), np.concatenate(member).astype(np.int64), np.concatenate(level).astype(np.int64)


def disk_statistics(mapped, csr, radii, dtype=np.float64):
    """(n [S,J], dis_mean [S,J]): dis_mean = mean over the disk's members of (d - e)^2 / e, d the distance to the nearest other
    member (another entry of the list), e = sqrt(2 (pi r^2 / n) / 1.732); nan below two members.  dtype: the format of the
    coordinate differences and of the squared distances (float32 repeats the kernel's roundings; the rest is float64)."""
    offsets, member, level = csr
    m = np.asarray(mapped, dtype)
    radii = np.asarray(radii, np.float64)
    S, J = len(offsets) - 1, len(radii)
    n, dis = np.zeros((S, J)), np.full((S, J), np.nan)
    for s in range(S):
        mem, lev = member[offsets[s]:offsets[s + 1]], level[offsets[s]:offsets[s + 1]]
        pts = m[mem]
        diff = pts[:, None, :] - pts[None, :, :]
        d2 = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
        d2 = d2.astype(np.float64)
        np.fill_diagonal(d2, np.inf)
        for j in range(J):
            k = lev <= j
            n[s, j] = k.sum()
            if n[s, j] >= 2:
                near = np.sqrt(d2[np.ix_(k, k)].min(1))
                e = np.sqrt(2 * (np.pi * radii[j] ** 2 / n[s, j]) / 1.732)
                dis[s, j] = np.mean((near - e) ** 2 / e)
    return n, dis


def uniformity_from_statistics(n, dis, N, percentages=None):
    """uniform_j = mean over the disks with at least 5 members of float32(coverage dis_mean), coverage = (n - p N)^2 / (p N);
    the mean of the float32 values as numpy takes it (the reference's np.mean of a float32 array); nan when no disk is kept."""
    J = n.shape[1]
    p = PERCENTAGES[:J] if percentages is None else np.asarray(percentages, np.float64)
    out = np.full(J, np.nan)
    for j in range(J):
        keep = n[:, j] >= 5
        if keep.any():
            out[j] = np.mean(((n[keep, j] - p[j] * N) ** 2 / (p[j] * N) * dis[keep, j]).astype(np.float32))
    return out


def uniformity(mapped, csr, radii, percentages=None, dtype=np.float64):
    n, dis = disk_statistics(mapped, csr, radii, dtype)
    return uniformity_from_statistics(n, dis, len(mapped), percentages)
