"""Evaluation metrics of the reference's scoring step (evaluation/evaluate.py, evaluation/jsd.py and the CGAL point-to-surface
binary evaluation/evaluation_code/evaluation.cpp) on the GPU.

Every function takes torch tensors on the GPU; a CPU tensor raises PuflowHipError (there is no CPU fallback).  The hot parts are
HIP (csrc/eval_metrics.hip: approx-match EMD and point-to-mesh distance; csrc/knn.hip pf_nn1: the nearest-neighbour searches
of CD / Hausdorff and of the JSD occupancy lookup; csrc/eval_uniform.hip: the seeds, disks and in-disk statistic of the
uniformity columns; csrc/surface_reach.hip: the bottleneck field behind surface disks); torch only gathers, sorts and reduces
small arrays around them.

Uniformity (evaluate.py:105-165 analyze_uniform): `disks` makes either Euclidean balls around seeds on the surface - which on
parts thinner than the radius also take in the opposite side - or, given `surface_reach`, surface disks: a point belongs when
it is inside the ball AND its face is connected to the seed's face along the surface inside a ball no larger than the radius
(the bottleneck field).  That restriction is this project's own definition.  It is not a geodesic
length, and its parity with the CGAL geodesic disks of PU-GAN's definition (evaluation.cpp:88-107) is unpinned: the
reference's binary never writes its disks.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, ops


def normalize_point_cloud(pc: torch.Tensor):
    """evaluate.py:48-57: pc [B,N,3] (or [N,3]) -> (pc - centroid) / furthest distance, centroid [B,1,3], furthest [B,1,1]."""
    squeeze = pc.dim() == 2
    out, cen, fd = ops.normalize_pc(pc[None] if squeeze else pc)
    return (out[0], cen[0], fd[0]) if squeeze else (out, cen, fd)


def chamfer_hausdorff(pred: torch.Tensor, gt: torch.Tensor):
    """(cd, hd), both [B], of pred [B,N,3] and gt [B,M,3] after each cloud's own normalisation (evaluate.py:97-103, 228-236):
    with d1 / d2 the squared nearest-neighbour distances pred -> gt / gt -> pred,
        cd = mean(d1) + mean(d2),    hd = max(d1) + max(d2).
    This "Hausdorff" is the reference's own definition (evaluate.py:231): the SUM of the two one-sided maxima, of SQUARED
    distances - not the symmetric Hausdorff distance."""
    p, _, _ = normalize_point_cloud(pred)
    g, _, _ = normalize_point_cloud(gt)
    d1 = ops.nearest_distance(p, g)
    d2 = ops.nearest_distance(g, p)
    return d1.mean(1) + d2.mean(1), d1.amax(1) + d2.amax(1)


def approx_match_emd(pred: torch.Tensor, gt: torch.Tensor, levels_top: int = 7) -> torch.Tensor:
    """Approx-match EMD [B] of pred [B,n,3] and gt [B,m,3] as given (the CLI normalises first, as evaluate.py:97-103 does):
    the multi-level soft assignment of tf_ops/approxmatch with levels -4^j, j = levels_top .. -1, then 0, and the cost / n
    (evaluate.py:59-65).  levels_top = 7 is the schedule of the CUDA op (the published numbers), 8 that of the CPU op.
    Deterministic; a cloud's value does not depend on the batch it is in (pf_approxmatch_emd)."""
    lib = _lib.load()
    a, b = ops._f32c(pred), ops._f32c(gt)
    if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] or a.shape[2] != 3 or b.shape[2] != 3:
        raise _lib.PuflowHipError(f"approx_match_emd: shapes {tuple(a.shape)} / {tuple(b.shape)}, want [B,n,3] / [B,m,3]")
    B, n, m = a.shape[0], a.shape[1], b.shape[1]
    nws = lib.pf_approxmatch_ws_floats(B, n, m, int(levels_top))
    if nws < 0:
        _lib.check(int(nws), "pf_approxmatch_emd")
    ws = torch.empty(int(nws), dtype=torch.float32, device=a.device)
    cost = torch.empty(B, dtype=torch.float32, device=a.device)
    _lib.check(lib.pf_approxmatch_emd(a.data_ptr(), b.data_ptr(), B, n, m, int(levels_top), cost.data_ptr(), ws.data_ptr(),
                                      int(nws), ops._stream()), "pf_approxmatch_emd")
    return cost


# ---- JSD ------------------------------------------------------------------------------------------------------------------
_GRIDS = {}


def sphere_grid(resolution: int = 28) -> np.ndarray:
    """jsd.py:33-51: the centres of a resolution^3 grid over the cube [-0.5, 0.5]^3 (float32, i-major order) whose norm is at
    most 0.5."""
    if resolution not in _GRIDS:
        ax = (np.arange(resolution, dtype=np.float64) * (1.0 / float(resolution - 1)) - 0.5).astype(np.float32)
        g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
        _GRIDS[resolution] = np.ascontiguousarray(g[np.linalg.norm(g, axis=1) <= 0.5])
    return _GRIDS[resolution]


def occupancy(pc: torch.Tensor, resolution: int = 28) -> np.ndarray:
    """Occupancy histograms [B, cells] (float64, host) of the clouds pc [B,N,3] as given: every point counts into its nearest
    cell of sphere_grid (pf_nn1).  pf_nn1 takes the first of equally near cells; sklearn's NearestNeighbors, which jsd.py uses,
    may take another for a point exactly halfway between two centres - the test fixtures hold no such point."""
    lib = _lib.load()
    pc = ops._f32c(pc)
    B, N, _ = pc.shape
    grid = torch.from_numpy(sphere_grid(resolution)).to(pc.device)
    G = grid.shape[0]
    grid = grid[None].expand(B, G, 3).contiguous()
    d = torch.empty((B, N), dtype=torch.float32, device=pc.device)
    idx = torch.empty((B, N), dtype=torch.int32, device=pc.device)
    _lib.check(lib.pf_nn1(pc.data_ptr(), grid.data_ptr(), B, N, G, d.data_ptr(), idx.data_ptr(), ops._stream()), "pf_nn1")
    flat = idx.long() + torch.arange(B, device=pc.device)[:, None] * G
    return torch.bincount(flat.view(-1), minlength=B * G).view(B, G).cpu().numpy().astype(np.float64)


def jsd_from_counts(P: np.ndarray, Q: np.ndarray) -> float:
    """Jensen-Shannon divergence with base 2 of two histograms, in float64 (jsd.py:70-89)."""
    p = P / P.sum()
    q = Q / Q.sum()

    def ent(x):
        x = x[x > 0]
        return float(-(x * np.log2(x)).sum())
    return ent((p + q) / 2.0) - (ent(p) + ent(q)) / 2.0


def jsd(pred: torch.Tensor, gt: torch.Tensor, resolution: int = 28) -> np.ndarray:
    """JSD [B] (float64, host) of every pair of pred [B,N,3] and gt [B,M,3] (jsd.py:54-105 with one cloud per set): both
    clouds normalised and halved (evaluate.py:84-90 np_normalize), counted into the sphere-clipped grid (`occupancy`)."""
    if pred.dim() == 2:
        pred, gt = pred[None], gt[None]
    p, _, _ = normalize_point_cloud(pred)
    g, _, _ = normalize_point_cloud(gt)
    cp, cg = occupancy(p * 0.5, resolution), occupancy(g * 0.5, resolution)
    return np.array([jsd_from_counts(cp[i], cg[i]) for i in range(cp.shape[0])])


# ---- point to mesh --------------------------------------------------------------------------------------------------------
def _morton(x: torch.Tensor, lo: torch.Tensor, ext: torch.Tensor) -> torch.Tensor:
    """30-bit Morton codes of x [K,3] in the box lo + [0, ext]."""
    q = ((x - lo) / ext * 1023.0).clamp(0, 1023).long()
    code = torch.zeros(x.shape[0], dtype=torch.long, device=x.device)
    for bit in range(10):
        for c in range(3):
            code |= ((q[:, c] >> bit) & 1) << (3 * bit + c)
    return code


P2F_SEARCHES = ("tiles", "grid")


def tri_grid_search(pts: torch.Tensor, tris: torch.Tensor, seed: torch.Tensor = None, return_cand: bool = False,
                    return_info: bool = False):
    """pf_point_mesh_grid as it is: pts [P,3], tris [F,9] float32 on the GPU in the caller's order, seed int32 [P] or None ->
    (dist float32 [P], face int32 [P]) - what pf_point_mesh_dist(brute = 1) returns for the same arguments, bit for bit, from
    a uniform grid of the triangles (csrc/tri_grid.hip).  return_cand: also the triangle evaluations per query (int32 [P]).
    return_info: also {"pairs", "oversize", "G", "cstart", "over", "pair_list", "ws"}: the grid's sizes, the byte offsets of
    its lists in the workspace and the workspace itself (uint8).  One host read (the pair count sizes the workspace)."""
    lib = _lib.load()
    if not (pts.is_cuda and tris.is_cuda):
        raise _lib.PuflowHipError("tri_grid_search needs GPU tensors (no CPU fallback)")
    pts, tris = ops._f32c(pts), ops._f32c(tris)
    P, F = pts.shape[0], tris.shape[0]
    if pts.dim() != 2 or pts.shape[1] != 3 or tris.dim() != 2 or tris.shape[1] != 9:
        raise _lib.PuflowHipError(f"tri_grid_search: pts [P,3] and tris [F,9], got {tuple(pts.shape)} and {tuple(tris.shape)}")
    if seed is not None:
        seed = seed.to(device=pts.device, dtype=torch.int32).contiguous()
        if seed.shape[0] != P:
            raise _lib.PuflowHipError(f"tri_grid_search: {seed.shape[0]} seeds for {P} points")
    n0 = lib.pf_point_mesh_grid_ws_bytes(P, F, 0)
    if n0 < 0:
        _lib.check(int(n0), "pf_point_mesh_grid_ws_bytes")
    ws = torch.empty(int(n0), dtype=torch.uint8, device=pts.device)
    info = torch.zeros(8, dtype=torch.int64, device=pts.device)
    _lib.check(lib.pf_point_mesh_grid_count(tris.data_ptr(), F, ws.data_ptr(), int(n0), info.data_ptr(), ops._stream()),
               "pf_point_mesh_grid_count")
    info = info.cpu().tolist()                                                   # the host sizes the pair list
    pairs = int(info[0])
    nb = lib.pf_point_mesh_grid_ws_bytes(P, F, pairs)
    if nb < 0:
        _lib.check(int(nb), "pf_point_mesh_grid_ws_bytes")
    ws = torch.empty(int(nb), dtype=torch.uint8, device=pts.device)
    dist = torch.empty(P, dtype=torch.float32, device=pts.device)
    face = torch.empty(P, dtype=torch.int32, device=pts.device)
    cand = torch.empty(P, dtype=torch.int32, device=pts.device) if return_cand else None
    _lib.check(lib.pf_point_mesh_grid(pts.data_ptr(), P, tris.data_ptr(), F, None if seed is None else seed.data_ptr(),
                                      dist.data_ptr(), face.data_ptr(), None if cand is None else cand.data_ptr(), ws.data_ptr(),
                                      int(nb), pairs, ops._stream()), "pf_point_mesh_grid")
    out = (dist, face) + ((cand,) if return_cand else ())
    if return_info:
        out += ({"pairs": pairs, "oversize": int(info[1]), "G": tuple(int(g) for g in info[2:5]), "cstart": int(info[5]),
                 "over": int(info[6]), "pair_list": int(info[7]), "ws": ws},)
    return out


def point_to_mesh_distance(points: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, return_face: bool = False,
                           brute: bool = False, search: str = "tiles"):
    """Distance [P] of every point of points [P,3] to the closest point of the triangle mesh (verts [V,3], faces [F,3]):
    what evaluation.cpp:224-232 gets from CGAL's AABB tree.  return_face: also the index of the closest face [P] (int64;
    the first of equally near faces in the search's order).  Points and faces go to pf_point_mesh_dist in Morton order
    (the order makes its box pruning effective, not the result); brute = True disables the pruning.  search = "grid": the
    same sort and seeds, then pf_point_mesh_grid (a uniform grid of the triangles, `tri_grid_search`) - the same dist and face,
    bit for bit; meant for many points near a large mesh.  It has no unpruned form: brute = True with it is refused."""
    if search not in P2F_SEARCHES:
        raise ValueError(f"search is one of {P2F_SEARCHES}, got {search!r}")
    if brute and search == "grid":
        raise ValueError("brute=True goes with search='tiles': the grid search has no unpruned form")
    lib = _lib.load()
    pts = ops._f32c(points)
    v = ops._f32c(verts)
    if not faces.is_cuda:
        raise _lib.PuflowHipError("point_to_mesh_distance needs GPU tensors (no CPU fallback)")
    f = faces.long()
    P, F = pts.shape[0], f.shape[0]
    tris = v[f]                                                                  # [F,3,3]
    lo = torch.minimum(pts.amin(0), v.amin(0))
    ext = (torch.maximum(pts.amax(0), v.amax(0)) - lo).clamp_min(1e-30)
    ct = _morton(tris.mean(1), lo, ext)
    cp = _morton(pts, lo, ext)
    ct_sorted, ot = torch.sort(ct, stable=True)
    cp_sorted, op = torch.sort(cp, stable=True)
    seed = torch.searchsorted(ct_sorted, cp_sorted).clamp_(max=F - 1).int()
    tris_s = tris[ot].reshape(F, 9).contiguous()
    pts_s = pts[op].contiguous()
    if search == "grid":
        d_s, f_s = tri_grid_search(pts_s, tris_s, seed)
    else:
        nws = lib.pf_point_mesh_ws_floats(P, F)
        if nws < 0:
            _lib.check(int(nws), "pf_point_mesh_dist")
        ws = torch.empty(int(nws), dtype=torch.float32, device=pts.device)
        d_s = torch.empty(P, dtype=torch.float32, device=pts.device)
        f_s = torch.empty(P, dtype=torch.int32, device=pts.device)
        _lib.check(lib.pf_point_mesh_dist(pts_s.data_ptr(), P, tris_s.data_ptr(), F, seed.data_ptr(), 1 if brute else 0,
                                          d_s.data_ptr(), f_s.data_ptr(), ws.data_ptr(), int(nws), ops._stream()),
                   "pf_point_mesh_dist")
    dist = torch.empty_like(d_s)
    dist[op] = d_s
    if not return_face:
        return dist
    face = torch.empty(P, dtype=torch.long, device=pts.device)
    face[op] = ot[f_s.long()]
    return dist, face


def read_off(path):
    """(verts [V,3] float32, faces [F,3] int64) of an OFF file.  The header is `OFF` alone on its line or followed by the
    counts on the same line; `#` starts a comment.  Polygons with more than three corners are fan-triangulated (0, i, i+1) -
    the reference only defines triangle meshes (CGAL's reader, evaluation.cpp); values after a face's indices (colours) are
    ignored."""
    with open(path) as fh:
        lines = [ln.split("#", 1)[0].split() for ln in fh]
    lines = [ln for ln in lines if ln]
    if not lines or not lines[0][0].endswith("OFF"):
        raise ValueError(f"{path}: not an OFF file")
    head = lines[0][1:]
    rest = lines[1:]
    if not head:
        head, rest = rest[0], rest[1:]
    nv, nf = int(head[0]), int(head[1])
    if len(rest) < nv + nf:
        raise ValueError(f"{path}: {nv} vertices and {nf} faces declared, {len(rest)} lines follow")
    verts = np.array([[float(t) for t in ln[:3]] for ln in rest[:nv]], dtype=np.float32).reshape(nv, 3)
    tris = []
    for ln in rest[nv:nv + nf]:
        k = int(ln[0])
        idx = [int(t) for t in ln[1:1 + k]]
        if len(idx) < 3:
            raise ValueError(f"{path}: a face with {len(idx)} corners")
        tris += [(idx[0], idx[i], idx[i + 1]) for i in range(1, k - 1)]
    return verts, np.array(tris, dtype=np.int64).reshape(-1, 3)


# ---- uniformity -----------------------------------------------------------------------------------------------------------
PERCENTAGES = (0.004, 0.006, 0.008, 0.010, 0.012)          # evaluate.py:105: the disks' share of the surface area


def _tris(verts: torch.Tensor, faces: torch.Tensor, what: str) -> torch.Tensor:
    if not (torch.is_tensor(verts) and torch.is_tensor(faces) and verts.is_cuda and faces.is_cuda):
        raise _lib.PuflowHipError(f"{what} needs GPU tensors (no CPU fallback)")
    return ops._f32c(verts)[faces.long()].reshape(-1, 9).contiguous()


def _radii(radii):
    r = np.ascontiguousarray(np.atleast_1d(np.asarray(radii, dtype=np.float64)))
    return r, (ctypes.c_double * len(r))(*r.tolist())


def mesh_area_radii(verts, faces, percentages=PERCENTAGES):
    """(radii [J], cumulative triangle areas [F]) of a mesh, host float64 (verts / faces: arrays or tensors):
    r_j = sqrt(p_j A / pi) with A the total area - a disk of radius r_j covers the share p_j of a flat surface of area A."""
    v = np.asarray(verts.cpu() if torch.is_tensor(verts) else verts, dtype=np.float64)
    f = np.asarray(faces.cpu() if torch.is_tensor(faces) else faces, dtype=np.int64)
    t = v[f]
    cum = np.cumsum(0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1))
    return np.sqrt(np.asarray(percentages, dtype=np.float64) * cum[-1] / np.pi), cum


def sample_mesh(verts: torch.Tensor, faces: torch.Tensor, S: int = 1000, seed: int = 0):
    """S seeds on the surface (pf_mesh_sample): the face area-weighted, the position uniform inside it, from Philox-4x32-10
    with key `seed` and counter s - seed s depends on (mesh, seed, s) only.  -> (seeds [S,3] float32, face [S] int64,
    uniforms [S,3] float32: the three numbers behind every seed)."""
    lib = _lib.load()
    tris = _tris(verts, faces, "sample_mesh")
    _, cum = mesh_area_radii(verts, faces)
    cum_d = torch.from_numpy(cum).to(tris.device)
    seeds = torch.empty((S, 3), dtype=torch.float32, device=tris.device)
    uni = torch.empty((S, 3), dtype=torch.float32, device=tris.device)
    face = torch.empty(S, dtype=torch.int32, device=tris.device)
    _lib.check(lib.pf_mesh_sample(tris.data_ptr(), tris.shape[0], cum_d.data_ptr(), int(S), int(seed) & (2 ** 64 - 1),
                                  seeds.data_ptr(), face.data_ptr(), uni.data_ptr(), ops._stream()), "pf_mesh_sample")
    return seeds, face.long(), uni


def mapped_points(points: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, face: torch.Tensor = None) -> torch.Tensor:
    """The closest point of the mesh to every point of points [P,3] (evaluation.cpp:225-228): the closest point of the
    triangle `point_to_mesh_distance(..., return_face=True)` finds (face [P]: that result, when the caller has it)."""
    lib = _lib.load()
    tris = _tris(verts, faces, "mapped_points")
    pts = ops._f32c(points)
    if face is None:
        _, face = point_to_mesh_distance(pts, verts, faces, return_face=True)
    fi = face.to(device=pts.device, dtype=torch.int32).contiguous()
    out = torch.empty_like(pts)
    _lib.check(lib.pf_tri_closest_points(pts.data_ptr(), pts.shape[0], tris.data_ptr(), tris.shape[0], fi.data_ptr(),
                                         out.data_ptr(), ops._stream()), "pf_tri_closest_points")
    return out


REACH_ST_START, REACH_ST_ITER, REACH_ST_ROW = _lib.PF_REACH_ST_START, _lib.PF_REACH_ST_ITER, _lib.PF_REACH_ST_ROW


def face_adjacency(verts: torch.Tensor, faces: torch.Tensor):
    """(offsets [F+1] int64, adj [nnz] int32): row f lists, ascending, the other faces that share a vertex with face f, after
    welding vertices of equal coordinates (torch.unique(dim=0) on the device; +0 and -0 weld) - a triangle soup in which every
    face has its own three vertices gets the adjacency of its indexed mesh.  torch ops only: sorts of [3F] and [sum deg^2]."""
    if not (torch.is_tensor(verts) and torch.is_tensor(faces) and verts.is_cuda and faces.is_cuda):
        raise _lib.PuflowHipError("face_adjacency needs GPU tensors (no CPU fallback)")
    return _vertex_sharing_faces(ops._f32c(verts), faces.long())


def _vertex_sharing_faces(v: torch.Tensor, f: torch.Tensor):
    F = f.shape[0]
    _, weld = torch.unique(v, dim=0, return_inverse=True)
    vid = weld[f].reshape(-1)                                                    # [3F] welded vertex of every corner
    fid = torch.arange(F, device=f.device).repeat_interleave(3)
    vs, order = torch.sort(vid, stable=True)
    fs = fid[order]                                                              # faces grouped by vertex
    deg = torch.bincount(vs, minlength=int(weld.max()) + 1)
    start = torch.cumsum(deg, 0) - deg
    d = deg[vs]                                                                  # every corner pairs with its vertex's whole group
    a = fs.repeat_interleave(d)
    first = start[vs].repeat_interleave(d)
    within = torch.arange(a.shape[0], device=f.device) - (torch.cumsum(d, 0) - d).repeat_interleave(d)
    b = fs[first + within]
    key = torch.unique(a[a != b] * F + b[a != b])                                # sorted: by face, then by neighbour
    offsets = torch.zeros(F + 1, dtype=torch.int64, device=f.device)
    offsets[1:] = torch.bincount(key // F, minlength=F).cumsum(0)
    return offsets, (key % F).int()


def surface_reach(src: torch.Tensor, src_face: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, r_stop,
                  adjacency=None, return_info: bool = False):
    """The bottleneck field around the sources src [S,3], each on face src_face [S] of the mesh, inside the balls of radius
    r_stop (a number, or [S]): the CSR (offsets [S+1] int64, rface [nnz] int32, rb2 [nnz] float32).  Row s lists, ascending,
    the faces whose closest point is within r_stop[s] of the source, with b2 = the smallest squared radius of a ball around the
    source inside which the face is connected to the source's face over vertex-sharing faces (`face_adjacency`, or
    `adjacency` when the caller has it) - +inf when no such path stays inside r_stop.  Finite values are exact, whatever
    r_stop.  The surface distance of a point q on face f is D2 = max(|q - s|^2, b2(f)) (`disks(..., reach=)`,
    `surface_distances`).  return_info: also {"rd2" [nnz], "sweeps" [S], "status"}.  (pf_reach_count / _fill / _relax)"""
    lib = _lib.load()
    tris = _tris(verts, faces, "surface_reach")
    sd = ops._f32c(src)
    dev, S, F = sd.device, sd.shape[0], tris.shape[0]
    sf = src_face.to(device=dev, dtype=torch.int32).contiguous()
    rs = torch.from_numpy(np.asarray(r_stop.cpu() if torch.is_tensor(r_stop) else r_stop, dtype=np.float64).reshape(-1))
    if rs.numel() == 1:
        rs = rs.expand(S)
    if sd.dim() != 2 or sd.shape[1] != 3 or sf.shape[0] != S or rs.shape[0] != S:
        raise _lib.PuflowHipError(f"surface_reach: src {tuple(sd.shape)}, src_face {tuple(sf.shape)}, r_stop {tuple(rs.shape)}")
    r2 = (rs * rs).float().to(dev).contiguous()                                  # fp32(r^2), as the disks round their radii
    adj_off, adj = face_adjacency(verts, faces) if adjacency is None else adjacency
    adj_off, adj = adj_off.long().contiguous(), adj.int().contiguous()
    if adj_off.shape[0] != F + 1 or int(adj_off[-1]) != adj.shape[0]:
        raise _lib.PuflowHipError("surface_reach: the adjacency is not a CSR over the mesh's faces")
    if adj.numel() == 0:
        adj = adj.new_zeros(1)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    counts = torch.empty(S, dtype=torch.int32, device=dev)
    _lib.check(lib.pf_reach_count(tris.data_ptr(), F, sd.data_ptr(), sf.data_ptr(), r2.data_ptr(), S, counts.data_ptr(),
                                  status.data_ptr(), ops._stream()), "pf_reach_count")
    offsets = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    offsets[1:] = counts.long().cumsum(0)
    nnz = int(offsets[-1])                                                       # the host sizes the buffers
    rface = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    rd2 = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)
    rb2 = torch.full((max(nnz, 1),), float("inf"), dtype=torch.float32, device=dev)
    sweeps = torch.zeros(S, dtype=torch.int32, device=dev)
    _lib.check(lib.pf_reach_fill(tris.data_ptr(), F, sd.data_ptr(), sf.data_ptr(), r2.data_ptr(), S, offsets.data_ptr(),
                                 rface.data_ptr(), rd2.data_ptr(), status.data_ptr(), ops._stream()), "pf_reach_fill")
    _lib.check(lib.pf_reach_relax(offsets.data_ptr(), rface.data_ptr(), rd2.data_ptr(), F, adj_off.data_ptr(), adj.data_ptr(),
                                  sf.data_ptr(), S, rb2.data_ptr(), sweeps.data_ptr(), status.data_ptr(), ops._stream()),
               "pf_reach_relax")
    st = int(status)
    if st & (REACH_ST_ITER | REACH_ST_ROW):
        raise _lib.PuflowHipError("surface_reach: a row did not settle within its length + 1 sweeps, or lists a face outside the mesh")
    csr = (offsets, rface[:nnz], rb2[:nnz])
    if return_info:
        return csr, {"rd2": rd2[:nnz], "sweeps": sweeps, "status": st}
    return csr


def _reach_args(reach, face, S: int, N: int, dev, what: str):
    if reach is None or face is None:
        raise _lib.PuflowHipError(f"{what}: reach and the points' faces go together")
    off, rface, rb2 = reach
    if not (off.is_cuda and rface.is_cuda and rb2.is_cuda and face.is_cuda):
        raise _lib.PuflowHipError(f"{what} needs GPU tensors (no CPU fallback)")
    off, rface, rb2 = off.long().contiguous(), rface.int().contiguous(), rb2.float().contiguous()
    fi = face.to(device=dev, dtype=torch.int32).contiguous()
    nnz = rface.shape[0]
    if off.shape[0] != S + 1 or fi.shape[0] != N or rb2.shape[0] != nnz or int(off[0]) < 0 or int(off[-1]) > nnz or \
            bool((off[1:] < off[:-1]).any()):
        raise _lib.PuflowHipError(f"{what}: the reach CSR does not describe {S} sources, or the faces not {N} points")
    if nnz == 0:
        rface, rb2 = rface.new_zeros(1), rb2.new_zeros(1)
    return fi, off, rface, rb2


def surface_distances(points: torch.Tensor, points_face: torch.Tensor, src: torch.Tensor, reach) -> torch.Tensor:
    """D2 [S,N] float32: max(|q - s|^2, b2(face(q))) of every point of points [N,3] (on faces points_face [N]) from every
    source - +inf for a point whose face the source's reach row does not hold (pf_reach_point_d2)."""
    lib = _lib.load()
    p, sd = ops._f32c(points), ops._f32c(src)
    N, S = p.shape[0], sd.shape[0]
    fi, off, rface, rb2 = _reach_args(reach, points_face, S, N, p.device, "surface_distances")
    out = torch.empty((S, N), dtype=torch.float32, device=p.device)
    _lib.check(lib.pf_reach_point_d2(p.data_ptr(), N, fi.data_ptr(), sd.data_ptr(), S, off.data_ptr(), rface.data_ptr(),
                                     rb2.data_ptr(), out.data_ptr(), ops._stream()), "pf_reach_point_d2")
    return out


def disks(mapped: torch.Tensor, seeds: torch.Tensor, radii, reach=None, mapped_face: torch.Tensor = None):
    """The points of mapped [N,3] inside the Euclidean balls of radii [J] (ascending) around seeds [S,3].
    -> (counts [S,J] int32, (offsets [S+1] int64, member [nnz] int32, level [nnz] int32)): row s of the CSR lists the members
    of the largest ball of seed s in ascending index, each with the smallest j whose ball holds it (pf_disk_count / _fill).
    reach (`surface_reach` of the seeds with r_stop >= the largest radius) and mapped_face [N] (the face every mapped point
    lies on): surface disks instead - a point is in disk j when max(|q - s|^2, b2(face(q))) <= fp32(r_j^2), so a ball's
    members on a part of the surface not connected to the seed inside that ball are left out (pf_disk_count_reach /
    _fill_reach: the same kernels, the same CSR)."""
    lib = _lib.load()
    m, sd = ops._f32c(mapped), ops._f32c(seeds)
    r, rc = _radii(radii)
    N, S, J = m.shape[0], sd.shape[0], len(r)
    counts = torch.empty((S, J), dtype=torch.int32, device=m.device)
    if reach is not None or mapped_face is not None:
        fi, roff, rface, rb2 = _reach_args(reach, mapped_face, S, N, m.device, "disks")
        extra = (fi.data_ptr(), roff.data_ptr(), rface.data_ptr(), rb2.data_ptr())
        _lib.check(lib.pf_disk_count_reach(m.data_ptr(), N, sd.data_ptr(), S, rc, J, *extra, counts.data_ptr(), ops._stream()),
                   "pf_disk_count_reach")
        offsets = torch.zeros(S + 1, dtype=torch.int64, device=m.device)
        offsets[1:] = counts[:, J - 1].long().cumsum(0)
        nnz = int(offsets[-1])
        member = torch.empty(max(nnz, 1), dtype=torch.int32, device=m.device)
        level = torch.empty(max(nnz, 1), dtype=torch.int32, device=m.device)
        _lib.check(lib.pf_disk_fill_reach(m.data_ptr(), N, sd.data_ptr(), S, rc, J, *extra, offsets.data_ptr(), member.data_ptr(),
                                          level.data_ptr(), ops._stream()), "pf_disk_fill_reach")
        return counts, (offsets, member[:nnz], level[:nnz])
    _lib.check(lib.pf_disk_count(m.data_ptr(), N, sd.data_ptr(), S, rc, J, counts.data_ptr(), ops._stream()), "pf_disk_count")
    offsets = torch.zeros(S + 1, dtype=torch.int64, device=m.device)
    offsets[1:] = counts[:, J - 1].long().cumsum(0)
    nnz = int(offsets[-1])                                       # the host sizes the buffer
    member = torch.empty(max(nnz, 1), dtype=torch.int32, device=m.device)
    level = torch.empty(max(nnz, 1), dtype=torch.int32, device=m.device)
    _lib.check(lib.pf_disk_fill(m.data_ptr(), N, sd.data_ptr(), S, rc, J, offsets.data_ptr(), member.data_ptr(),
                                level.data_ptr(), ops._stream()), "pf_disk_fill")
    return counts, (offsets, member[:nnz], level[:nnz])


def disk_statistics(mapped: torch.Tensor, csr, radii):
    """(n [S,J], dis_mean [S,J]) float64 on the device of every disk of the CSR (`disks`, or `read_disk_files`): the member
    count and the mean of (d - e)^2 / e over the members, d the distance to the nearest other member of the same disk,
    e = sqrt(2 (pi r_j^2 / n) / 1.732) (evaluate.py:153-158).  A row's values depend on that row alone (pf_disk_uniformity)."""
    lib = _lib.load()
    m = ops._f32c(mapped)
    offsets, member, level = csr
    if not (offsets.is_cuda and member.is_cuda and level.is_cuda):
        raise _lib.PuflowHipError("disk_statistics needs GPU tensors (no CPU fallback)")
    r, rc = _radii(radii)
    N, S, J = m.shape[0], offsets.shape[0] - 1, len(r)
    offsets = offsets.long().contiguous()
    member, level = member.int().contiguous(), level.int().contiguous()
    nnz = member.shape[0]
    if level.shape[0] != nnz or S < 1 or int(offsets[0]) < 0 or int(offsets[-1]) > nnz or bool((offsets[1:] < offsets[:-1]).any()):
        raise _lib.PuflowHipError("disk_statistics: the CSR's offsets do not describe its member list")
    if nnz and (int(member.min()) < 0 or int(member.max()) >= N or int(level.min()) < 0):
        raise _lib.PuflowHipError(f"disk_statistics: a member index outside [0, {N}) or a negative level")
    if nnz == 0:
        member, level = member.new_zeros(1), level.new_zeros(1)
    n = torch.empty((S, J), dtype=torch.float64, device=m.device)
    dis = torch.empty((S, J), dtype=torch.float64, device=m.device)
    _lib.check(lib.pf_disk_uniformity(m.data_ptr(), N, offsets.data_ptr(), member.data_ptr(), level.data_ptr(), S, rc, J,
                                      n.data_ptr(), dis.data_ptr(), ops._stream()), "pf_disk_uniformity")
    return n, dis


def uniformity_from_statistics(n, dis_mean, N: int, percentages=None) -> np.ndarray:
    """The host finish in float64 (evaluate.py:132-162): coverage = (n - p_j N)^2 / (p_j N); disks with fewer than 5 members
    are left out; uniform_j = the mean over the kept disks of float32(coverage dis_mean) - nan when none is kept."""
    n = np.asarray(n.cpu() if torch.is_tensor(n) else n, dtype=np.float64)
    d = np.asarray(dis_mean.cpu() if torch.is_tensor(dis_mean) else dis_mean, dtype=np.float64)
    J = n.shape[1]
    p = np.asarray(PERCENTAGES[:J] if percentages is None else percentages, dtype=np.float64)
    if len(p) != J:
        raise ValueError(f"{J} radii and {len(p)} percentages")
    out = np.full(J, np.nan)
    for j in range(J):
        keep = n[:, j] >= 5
        if keep.any():
            expect = p[j] * N
            out[j] = np.mean(((n[keep, j] - expect) ** 2 / expect * d[keep, j]).astype(np.float32))
    return out


def uniformity(mapped: torch.Tensor, csr, radii, percentages=None) -> np.ndarray:
    """uniform_j [J] (host float64) of the mapped points and their disks: `disk_statistics` and its host finish."""
    n, dis = disk_statistics(mapped, csr, radii)
    return uniformity_from_statistics(n, dis, mapped.shape[0], percentages)


# the three files of evaluate.py:256-262 (what the reference's CGAL binary was meant to write)
def write_disk_files(prefix: str, points, dist, mapped, csr, radii) -> None:
    """`<prefix>_disk_idx.txt`: line s J + j = `count:idx idx ...` (the members of disk (s, j), ascending);
    `<prefix>_radius.txt`: the J radii; `<prefix>_point2mesh_distance.txt`: `x y z d mx my mz` per point, the mapped point
    in columns 4-6.  %.9g: float32 values read back exactly."""
    host = lambda a: np.asarray(a.cpu() if torch.is_tensor(a) else a)      # noqa: E731
    offsets, member, level = (host(a) for a in csr)
    r = np.atleast_1d(np.asarray(radii, dtype=np.float64))
    with open(prefix + "_disk_idx.txt", "w") as f:
        for s in range(len(offsets) - 1):
            mem, lev = member[offsets[s]:offsets[s + 1]], level[offsets[s]:offsets[s + 1]]
            for j in range(len(r)):
                idx = mem[lev <= j]
                f.write("%d:%s\n" % (len(idx), " ".join(map(str, idx.tolist()))))
    with open(prefix + "_radius.txt", "w") as f:
        f.write("".join("%.17g\n" % x for x in r))
    rows = np.concatenate([host(points).reshape(-1, 3), host(dist).reshape(-1, 1), host(mapped).reshape(-1, 3)], axis=1)
    with open(prefix + "_point2mesh_distance.txt", "w") as f:
        f.write("".join(("%.9g %.9g %.9g %.9g %.9g %.9g %.9g\n" % tuple(row)) for row in rows.tolist()))


def read_disk_files(prefix: str):
    """-> (mapped [N,3] float32, radii [J] float64, (offsets, member, level) as host arrays) of the three files, whoever wrote
    them.  The disks of a seed need not be nested there: a member's level is the first j that lists it, and the row holds the
    union of the seed's J lines - a file whose later disks drop members of earlier ones is refused."""
    mapped = np.atleast_2d(np.loadtxt(prefix + "_point2mesh_distance.txt", dtype=np.float32))[:, 4:7]
    radii = np.atleast_1d(np.loadtxt(prefix + "_radius.txt", dtype=np.float64))
    J = len(radii)
    with open(prefix + "_disk_idx.txt") as f:
        lines = [ln for ln in f.read().split("\n") if ln.strip()]
    if len(lines) % J:
        raise ValueError(f"{prefix}_disk_idx.txt: {len(lines)} lines for {J} radii")
    offsets, member, level = [0], [], []
    for s in range(len(lines) // J):
        seen = np.zeros(0, dtype=np.int64)
        for j in range(J):
            idx = np.array(lines[s * J + j].split(":", 1)[1].split(), dtype=np.int64)
            new = np.setdiff1d(idx, seen)
            if len(idx) != len(seen) + len(new) or len(np.unique(idx)) != len(idx):
                raise ValueError(f"{prefix}_disk_idx.txt: the disks of seed {s} are not nested sets")
            member.append(new)
            level.append(np.full(len(new), j, dtype=np.int32))
            seen = idx
        offsets.append(offsets[-1] + len(seen))
    member = np.concatenate(member).astype(np.int32) if member else np.zeros(0, np.int32)
    level = np.concatenate(level) if level else np.zeros(0, np.int32)
    out_m, out_l = np.empty_like(member), np.empty_like(level)
    for s in range(len(offsets) - 1):                             # ascending index inside every row, like `disks`
        a, b = offsets[s], offsets[s + 1]
        o = np.argsort(member[a:b], kind="stable")
        out_m[a:b], out_l[a:b] = member[a:b][o], level[a:b][o]
    return np.ascontiguousarray(mapped), radii, (np.array(offsets, dtype=np.int64), out_m, out_l)
