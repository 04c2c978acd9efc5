"""Evaluation metrics of the reference's scoring step (evaluation/evaluate.py, evaluation/jsd.py and the CGAL point-to-surface
binary evaluation/evaluation_code/evaluation.cpp) on the GPU.

Every function takes torch tensors on the GPU; a CPU tensor raises PuflowHipError (there is no CPU fallback).  The hot parts are
HIP (csrc/eval_metrics.hip: approx-match EMD and point-to-mesh distance; csrc/knn.hip pf_nn1: the nearest-neighbour searches
of CD / Hausdorff and of the JSD occupancy lookup); torch only gathers, sorts and reduces small arrays around them.
"""
from __future__ import annotations

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


def point_to_mesh_distance(points: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, return_face: bool = False,
                           brute: bool = False):
    """Distance [P] of every point of points [P,3] to the closest point of the triangle mesh (verts [V,3], faces [F,3]):
    what evaluation.cpp:224-232 gets from CGAL's AABB tree.  return_face: also the index of the closest face [P] (int64;
    the first of equally near faces in the search's order).  Points and faces go to pf_point_mesh_dist in Morton order
    (the order makes its box pruning effective, not the result); brute = True disables the pruning."""
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
