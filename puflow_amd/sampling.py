"""Poisson-disk ("blue noise") sampling of triangle meshes on the GPU: what PU-GAN's Meshlab preparation gave the reference
ready-made - training patches (`poisson_256` / `poisson_1024`) and the 2048- / 8192-point test clouds.  The reference holds no
counterpart; the method is weighted sample elimination (Yuksel 2015, "Sample Elimination for Generating Poisson Disk Sample
Sets") over area-weighted surface samples (metrics.sample_mesh), in HIP (csrc/poisson.hip).

Every function takes torch tensors on the GPU; a CPU tensor raises PuflowHipError (there is no CPU fallback).  The
elimination's neighbour graph is Euclidean, not geodesic: on parts thinner than 2 r_max candidates of the opposite side count
as neighbours, so such parts get about the density of one side shared between both ("Poisson-disk sampling").  A
patch's pool is cropped either by Euclidean distance from its seed (`metric="ball"`: on a thin part a two-sided slab) or by
the surface distance of metrics.surface_reach (`metric="surface"`: only samples connected to the seed along the surface inside
the ball that holds them) - this project's own surface restriction, not a geodesic length; its parity with PU-GAN's
geodesic crop is unpinned.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib, metrics, ops

ROUND_BATCH = 16                       # rounds enqueued between two host reads of the "pools unfinished" word
ST_DEGREE, ST_WEIGHT = _lib.PF_POISSON_ST_DEGREE, _lib.PF_POISSON_ST_WEIGHT


def elimination_params(area: float, s: int, m: int):
    """(r_max, r_min) of a pool of s candidates on a surface of `area` thinned to m, in float64:
    r_max = sqrt(area / (2 sqrt(3) m)), the spacing of m points in a hexagonal packing; r_min = r_max (1 - (m/s)^1.5) 0.65
    (Yuksel's weight limiting; (m/s)^1.5 as t sqrt(t), which every implementation rounds alike)."""
    s, m = int(s), int(m)
    if m < 1 or m > s:
        raise ValueError(f"elimination_params: need 1 <= m <= s, got m = {m}, s = {s}")
    if not (float(area) > 0.0 and math.isfinite(float(area))):
        raise ValueError(f"elimination_params: need a positive area, got {area}")
    t = m / s
    r_max = math.sqrt(float(area) / (2.0 * math.sqrt(3.0) * m))
    return r_max, r_max * (1.0 - t * math.sqrt(t)) * 0.65


class _Pools:
    """The per-pool table on the host and the device (pf_poisson_pools)."""

    def __init__(self, points: torch.Tensor, sizes, targets, areas, flags: int = 0):
        lib = _lib.load()
        self.points = ops._f32c(points)
        self.sizes, self.targets = [int(v) for v in sizes], [int(v) for v in targets]
        self.areas = [float(v) for v in areas]
        B = self.B = len(self.sizes)
        if B == 0 or len(self.targets) != B or len(self.areas) != B:
            raise ValueError("sizes, targets and areas must list the same pools (at least one)")
        if self.points.dim() != 2 or self.points.shape[1] != 3 or self.points.shape[0] != sum(self.sizes) or min(self.sizes) < 1:
            raise ValueError(f"points {tuple(self.points.shape)} are not the {B} pools of sizes {self.sizes} back to back")
        for s, m, a in zip(self.sizes, self.targets, self.areas):
            elimination_params(a, s, m)                                     # the argument errors, by name
        self.host = (_lib.PfPoissonPool * B)()
        _lib.check(lib.pf_poisson_pools(_lib.counts(self.sizes), _lib.counts(self.targets), (ctypes.c_double * B)(*self.areas),
                                        B, int(flags), self.host), "pf_poisson_pools")
        table = np.frombuffer(self.host, dtype=np.int32).reshape(B, 8).copy()
        self.dev = torch.from_numpy(table).to(self.points.device)
        self.max_s, self.total, self.kept = max(self.sizes), sum(self.sizes), sum(self.targets)
        self.wg = [bool(p.path) for p in self.host]
        self.status = torch.zeros(1, dtype=torch.int32, device=self.points.device)

    def graph(self):
        lib, dev = _lib.load(), self.points.device
        deg = torch.empty(self.total, dtype=torch.int32, device=dev)
        _lib.check(lib.pf_poisson_degree(self.points.data_ptr(), self.dev.data_ptr(), self.B, self.max_s, self.total, deg.data_ptr(),
                                         self.status.data_ptr(), ops._stream()), "pf_poisson_degree")
        offsets = torch.zeros(self.total + 1, dtype=torch.int64, device=dev)
        offsets[1:] = deg.long().cumsum(0)
        nnz = int(offsets[-1])                                              # the host sizes the edge arrays
        nbr = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
        q = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
        w = torch.empty(self.total, dtype=torch.int32, device=dev)          # uint32 bits
        _lib.check(lib.pf_poisson_graph(self.points.data_ptr(), self.dev.data_ptr(), self.B, self.max_s, self.total,
                                        offsets.data_ptr(), nbr.data_ptr(), q.data_ptr(), w.data_ptr(), self.status.data_ptr(),
                                        ops._stream()), "pf_poisson_graph")
        return offsets, nbr[:nnz], q[:nnz], w


def neighbour_graph(points: torch.Tensor, sizes, areas, targets):
    """The elimination's graph of B pools stored back to back (points [sum sizes, 3]): (offsets [sum sizes + 1] int64,
    nbr [nnz] int32, q [nnz] int32).  Row i lists the candidates of i's pool within 2 r_max of it, as ascending indices inside
    the pool, with the integer weights q_ij = rint(65536 (1 - max(d, 2 r_min) / (2 r_max))^8) (pf_poisson_degree / _graph)."""
    offsets, nbr, q, _ = _Pools(points, sizes, targets, areas).graph()
    return offsets, nbr, q


def eliminate(points: torch.Tensor, sizes, targets, areas, single_workgroup: bool = True):
    """Thin every pool to its target: keep [sum targets] int64, per pool the ascending indices (inside the pool) that the
    sequential process "remove the candidate with the largest (weight, smaller index first), lower its neighbours' weights"
    leaves alive.  info: `phases` / `rounds` [B] (what each pool took), `status` (PF_POISSON_ST_* bits; non-zero raises unless
    it is only the degree warning), `launches` (kernel launches of the elimination, the graph's two not counted), `paths`.
    Pools of at most 8192 candidates run in one launch, one workgroup each; larger ones three launches a round, with one host
    read per ROUND_BATCH rounds.  single_workgroup = False sends every pool the second way (the same indices)."""
    lib = _lib.load()
    P = _Pools(points, sizes, targets, areas, 0 if single_workgroup else 1)
    offsets, nbr, q, w = P.graph()
    dev = P.points.device
    if nbr.numel() == 0:
        nbr, q = nbr.new_zeros(1), q.new_zeros(1)
    state = torch.empty(P.total, dtype=torch.int32, device=dev)
    st = torch.empty((P.B, 8), dtype=torch.int32, device=dev)
    keep = torch.full((P.kept,), -1, dtype=torch.int32, device=dev)
    _lib.check(lib.pf_poisson_begin(P.dev.data_ptr(), P.B, P.max_s, P.total, state.data_ptr(), st.data_ptr(), ops._stream()),
               "pf_poisson_begin")
    launches = 0
    if any(P.wg):
        _lib.check(lib.pf_poisson_eliminate_wg(P.dev.data_ptr(), P.B, offsets.data_ptr(), nbr.data_ptr(), q.data_ptr(), w.data_ptr(),
                                               state.data_ptr(), st.data_ptr(), keep.data_ptr(), ops._stream()),
                   "pf_poisson_eliminate_wg")
        launches += 1
    if not all(P.wg):
        unfinished = torch.zeros(1, dtype=torch.int32, device=dev)
        r, limit = 0, max(s for s, g in zip(P.sizes, P.wg) if not g) + 1      # a round removes at least one candidate
        while True:
            _lib.check(lib.pf_poisson_rounds(P.dev.data_ptr(), P.B, P.max_s, P.total, offsets.data_ptr(), nbr.data_ptr(),
                                             q.data_ptr(), w.data_ptr(), state.data_ptr(), st.data_ptr(), keep.data_ptr(), r,
                                             ROUND_BATCH, unfinished.data_ptr(), ops._stream()), "pf_poisson_rounds")
            r += ROUND_BATCH
            launches += 3 * ROUND_BATCH
            if int(unfinished) != r:
                break
            if r > limit + ROUND_BATCH:
                raise _lib.PuflowHipError("eliminate: a pool did not finish within its candidate count of rounds")
    sth = st.cpu().numpy()
    status = int(P.status)
    if status & ST_WEIGHT:
        raise _lib.PuflowHipError("eliminate: a candidate's weight left 32 bits (a pool far denser than its radius assumes)")
    if not bool((sth[:, 3] == 1).all()) or bool((keep < 0).any()):
        raise _lib.PuflowHipError("eliminate: a pool was not finished")
    info = {"phases": sth[:, 4].copy(), "rounds": sth[:, 5].copy(), "status": status, "launches": launches,
            "paths": ["workgroup" if g else "rounds" for g in P.wg]}
    return keep.long(), info


def _area(verts, faces) -> float:
    _, cum = metrics.mesh_area_radii(verts, faces)
    return float(cum[-1])


def poisson_disk(verts: torch.Tensor, faces: torch.Tensor, m: int, seed: int = 0, ratio: int = 5):
    """m blue-noise points of the mesh: (points [m,3] float32, face [m] int64).  The pool is the ratio * m surface samples of
    metrics.sample_mesh with this seed, the area the mesh's: the result depends on (mesh, m, seed, ratio) only."""
    m, ratio = int(m), int(ratio)
    if m < 1 or ratio < 1:
        raise ValueError(f"poisson_disk: need m >= 1 and ratio >= 1, got {m}, {ratio}")
    pool, face, _ = metrics.sample_mesh(verts, faces, ratio * m, seed)
    keep, _ = eliminate(pool, [ratio * m], [m], [_area(verts, faces)])
    return pool[keep], face[keep]


POOL_GROWTHS = 8                       # surface_pool: times r_stop is multiplied by 1.5 before a seed's component is called too small


def surface_pool(samples: torch.Tensor, sample_face: torch.Tensor, seeds: torch.Tensor, seed_face: torch.Tensor,
                 verts: torch.Tensor, faces: torch.Tensor, k: int, adjacency=None) -> torch.Tensor:
    """idx [P,k] int64: per seed the k samples with the smallest (D2, index), D2 = max(|q - seed|^2, b2(face(q))) the surface
    distance (metrics.surface_reach / surface_distances), nearest first.  The field is computed inside the ball of r_stop = the
    Euclidean distance of the min(2k, n)-th nearest sample (pf_knn_large; at most its 8192-th on sets beyond 16384, the
    largest that search takes there).  A value at or below fp32(r_stop^2) is exact and a true value above it shows as itself or
    as +inf, so a seed is finished once its k-th smallest value is at or below fp32(r_stop^2): those k are then the k smallest
    over the whole mesh, wherever r_stop started.  Until then its r_stop grows by 1.5, at most POOL_GROWTHS times; a seed still
    short after that lies on a component of the mesh too small for its pool, and raises."""
    k = int(k)
    n, P = samples.shape[0], seeds.shape[0]
    if k > n:
        raise ValueError(f"surface_pool: {k} samples wanted of {n}")
    if adjacency is None:
        adjacency = metrics.face_adjacency(verts, faces)
    kk = min(2 * k, n) if n <= 16384 else min(2 * k, 8192)
    dist, _ = ops.KNN(kk, transpose_mode=True)(samples[None], seeds[None])
    r_stop = dist[0, :, -1].double().sqrt().cpu().numpy()                   # KNN's distances are squared, ascending
    idx = torch.empty((P, k), dtype=torch.int64, device=samples.device)
    todo = np.arange(P)
    for growth in range(POOL_GROWTHS + 1):
        sel = torch.from_numpy(todo).to(samples.device)
        reach = metrics.surface_reach(seeds[sel], seed_face[sel], verts, faces, r_stop[todo], adjacency)
        d2 = metrics.surface_distances(samples, sample_face, seeds[sel], reach)
        val, order = torch.sort(d2, dim=1, stable=True)                     # (D2, index)
        r2 = torch.from_numpy(r_stop[todo] * r_stop[todo]).float().to(val.device)      # fp32(r^2), as surface_reach rounds it
        ok_t = val[:, k - 1] <= r2
        idx[sel[ok_t]] = order[:, :k][ok_t]
        ok = ok_t.cpu().numpy()
        if ok.all():
            return idx
        if growth == POOL_GROWTHS:
            b = int(np.flatnonzero(~ok)[0])                                 # the first seed still short
            faces_reached = int(torch.isfinite(reach[2][int(reach[0][b]):int(reach[0][b + 1])]).sum())
            raise _lib.PuflowHipError(f"surface_pool: seed {int(todo[b])} lies on a component of the mesh too small for its pool: "
                                      f"after {POOL_GROWTHS} growths of r_stop {faces_reached} faces are connected to it, holding "
                                      f"{int(torch.isfinite(val[b]).sum())} of the {k} samples wanted")
        todo = todo[~ok]
        r_stop[todo] *= 1.5


def make_patches(verts: torch.Tensor, faces: torch.Tensor, n_patches: int, num_point: int = 256, up_ratio: int = 4,
                 cloud_points: int = 2500, seed: int = 0, ratio: int = 5, return_pools: bool = False, metric: str = "ball"):
    """Training patches of one mesh, un-normalised (data.load_patch_arrays normalises):
    {"poisson_<num_point>": [P, num_point, 3], "poisson_<num_point * up_ratio>": [P, num_point * up_ratio, 3]} on the GPU.
    The patch seeds are a farthest-point sample of poisson_disk(cloud_points, seed).  A patch's ground truth is the
    ratio * num_point * up_ratio samples nearest its seed out of ratio * cloud_points * up_ratio surface samples (seed + 1),
    eliminated to num_point * up_ratio; its input the same with ratio * num_point out of ratio * cloud_points samples
    (seed + 2), eliminated to num_point - drawn independently of the ground truth, as in PU-GAN's files.  A pool's area is the
    mesh's times its share of the sample set.  All 2 P pools go through one elimination call.
    return_pools: also {"seeds" [P,3], "input_pool" [P, ratio * num_point, 3], "gt_pool" [P, ratio * num_point * up_ratio, 3],
    "seed_face" [P], "input_idx" / "gt_idx": the pools' indices into their sample sets}.
    metric: "ball" - nearest by Euclidean distance (pf_knn_large); "surface" - the ratio * n_out samples with the smallest
    (D2, index), D2 = max(|q - seed|^2, b2(face(q))) the surface distance of metrics.surface_reach (`surface_pool`)."""
    if metric not in ("ball", "surface"):
        raise ValueError(f"make_patches: metric is 'ball' or 'surface', got {metric!r}")
    n_patches, num_point, up_ratio, cloud_points, ratio = (int(v) for v in (n_patches, num_point, up_ratio, cloud_points, ratio))
    if min(n_patches, num_point, up_ratio, ratio) < 1 or cloud_points < max(n_patches, num_point):
        raise ValueError("make_patches: need positive counts and cloud_points >= max(n_patches, num_point)")
    area = _area(verts, faces)
    cloud, cloud_face = poisson_disk(verts, faces, cloud_points, seed, ratio)
    pick = ops.furthest_point_sample(cloud[None], n_patches)[0].long()
    seeds, seed_face = cloud[pick], cloud_face[pick]
    adjacency = metrics.face_adjacency(verts, faces) if metric == "surface" else None
    pools, sizes, targets, areas, idxs = [], [], [], [], []
    for n_out, n_set, sd in ((num_point, ratio * cloud_points, seed + 2), (num_point * up_ratio, ratio * cloud_points * up_ratio, seed + 1)):
        samples, sface, _ = metrics.sample_mesh(verts, faces, n_set, sd)
        if metric == "surface":
            idx = surface_pool(samples, sface, seeds, seed_face, verts, faces, ratio * n_out, adjacency)[None]
        else:
            _, idx = ops.KNN(ratio * n_out, transpose_mode=True)(samples[None], seeds[None])
        idxs.append(idx[0].long())
        pools.append(samples[idx[0].long()])                                # [P, ratio * n_out, 3], nearest first
        sizes += [ratio * n_out] * n_patches
        targets += [n_out] * n_patches
        areas += [area * (ratio * n_out) / n_set] * n_patches
    keep, _ = eliminate(torch.cat([p.reshape(-1, 3) for p in pools]), sizes, targets, areas)
    k_in = keep[:n_patches * num_point].view(n_patches, num_point)
    k_gt = keep[n_patches * num_point:].view(n_patches, num_point * up_ratio)
    out = {f"poisson_{num_point}": torch.gather(pools[0], 1, k_in[..., None].expand(-1, -1, 3)),
           f"poisson_{num_point * up_ratio}": torch.gather(pools[1], 1, k_gt[..., None].expand(-1, -1, 3))}
    if return_pools:
        return out, {"seeds": seeds, "input_pool": pools[0], "gt_pool": pools[1], "seed_face": seed_face, "input_idx": idxs[0],
                     "gt_idx": idxs[1]}
    return out
