"""Scores of a triangle mesh against a ground-truth mesh, on the GPU: what the surface-reconstruction literature reports for a
reconstructed surface (accuracy, completeness, Chamfer-L1, Hausdorff, normal consistency, F-score) beside the mesh's own
counts (open edges, Euler characteristic, area, signed volume).

`score` draws `samples` area-weighted points on each mesh (metrics.sample_mesh: Philox, so a result depends on the meshes, the
sample count and the seed only; the prediction's samples use key `seed`, the ground truth's `seed + 1`), finds every sample's
closest triangle of the OTHER mesh (metrics.point_to_mesh_distance, search = "grid" or "tiles": the same bits either way) and
reduces in double.  Everything takes GPU tensors; there is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib, metrics
from .reconstruct import _open_edges

COLUMNS = ["name", "vertices", "faces", "open_edges", "euler", "area", "volume", "accuracy", "completeness", "chamfer_l1",
           "hausdorff", "normal_consistency", "normal_signed", "fscore"]


def _mesh(verts, faces, what: str):
    if not (torch.is_tensor(verts) and torch.is_tensor(faces) and verts.is_cuda and faces.is_cuda):
        raise _lib.PuflowHipError(f"mesh_metrics.{what} needs GPU tensors (no CPU fallback)")
    v, f = verts.float().contiguous(), faces.long().contiguous()
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3 or f.shape[0] == 0:
        raise ValueError(f"mesh_metrics.{what}: verts [V,3] and faces [F,3] with F > 0, got {tuple(v.shape)} and {tuple(f.shape)}")
    return v, f


def face_normals(verts: torch.Tensor, faces: torch.Tensor):
    """(unit normals [F,3] float64 - zero rows for zero-area faces -, doubled areas [F] float64) of the triangles"""
    t = verts.double()[faces]
    n = torch.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], dim=1)
    a2 = n.norm(dim=1)
    return torch.where(a2[:, None] > 0, n / a2.clamp_min(1e-300)[:, None], torch.zeros_like(n)), a2


def mesh_counts(verts: torch.Tensor, faces: torch.Tensor) -> dict:
    """vertices, faces, open_edges (edges of exactly one triangle), euler = V - E + F over the undirected edges, area and the
    signed volume sum_f v0 . (v1 x v2) / 6 (the divergence theorem; positive for outward-oriented closed meshes) - double sums."""
    v, f = _mesh(verts, faces, "mesh_counts")
    nv = v.shape[0]
    a = torch.cat([f[:, 0], f[:, 1], f[:, 2]])
    b = torch.cat([f[:, 1], f[:, 2], f[:, 0]])
    edges = torch.unique(torch.minimum(a, b) * nv + torch.maximum(a, b)).shape[0]
    t = v.double()[f]
    _, a2 = face_normals(v, f)
    vol = (t[:, 0] * torch.cross(t[:, 1], t[:, 2], dim=1)).sum(1).sum() / 6.0
    return {"vertices": nv, "faces": f.shape[0], "open_edges": int(_open_edges(f, nv)), "euler": nv - edges + f.shape[0],
            "area": float(a2.sum() * 0.5), "volume": float(vol)}


def draw(pred_v, pred_f, gt_v, gt_f, samples: int = 100000, seed: int = 0):
    """The samples `score` uses: (points [S,3], their faces [S]) on the prediction (key seed) and on the ground truth (seed + 1)"""
    pv, pf = _mesh(pred_v, pred_f, "draw")
    gv, gf = _mesh(gt_v, gt_f, "draw")
    sp, fp, _ = metrics.sample_mesh(pv, pf, int(samples), int(seed))
    sg, fg, _ = metrics.sample_mesh(gv, gf, int(samples), int(seed) + 1)
    return (sp, fp), (sg, fg)


def score(pred_v, pred_f, gt_v, gt_f, samples: int = 100000, seed: int = 0, tau: float = 0.01, search: str = "grid") -> dict:
    """The columns of mesh_evaluation.csv but the name.  accuracy / completeness: the mean distance of the prediction's samples
    to the ground truth / of the ground truth's samples to the prediction; chamfer_l1 their mean; hausdorff the larger of the
    two maxima; normal_consistency / normal_signed: the mean of |n . n'| / n . n' of the sample's face and its closest face over
    both directions (samples on or nearest to a zero-area face left out; nan when none is left); fscore = 2 P R / (P + R) with
    P / R the share of the two distance sets below tau x the ground truth's box diagonal."""
    if int(samples) < 1:
        raise ValueError(f"samples >= 1, got {samples}")
    pv, pf = _mesh(pred_v, pred_f, "score")
    gv, gf = _mesh(gt_v, gt_f, "score")
    out = mesh_counts(pv, pf)
    (sp, fp), (sg, fg) = draw(pv, pf, gv, gf, samples, seed)
    d_pg, c_pg = metrics.point_to_mesh_distance(sp, gv, gf, return_face=True, search=search)
    d_gp, c_gp = metrics.point_to_mesh_distance(sg, pv, pf, return_face=True, search=search)
    d_pg, d_gp = d_pg.double(), d_gp.double()
    np_, ap = face_normals(pv, pf)
    ng, ag = face_normals(gv, gf)
    dots = []
    for own_n, own_a, own_f, other_n, other_a, other_f in ((np_, ap, fp, ng, ag, c_pg), (ng, ag, fg, np_, ap, c_gp)):
        keep = (own_a[own_f] > 0) & (other_a[other_f] > 0)
        dots.append((own_n[own_f] * other_n[other_f]).sum(1)[keep])
    dots = torch.cat(dots)
    diag = float((gv.double().amax(0) - gv.double().amin(0)).norm())
    thr = float(tau) * diag
    prec, rec = float((d_pg < thr).double().mean()), float((d_gp < thr).double().mean())
    acc, comp = float(d_pg.mean()), float(d_gp.mean())
    out.update({"accuracy": acc, "completeness": comp, "chamfer_l1": 0.5 * (acc + comp),
                "hausdorff": max(float(d_pg.max()), float(d_gp.max())),
                "normal_consistency": float(dots.abs().mean()) if dots.numel() else float("nan"),
                "normal_signed": float(dots.mean()) if dots.numel() else float("nan"),
                "fscore": 2.0 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0})
    return out
