"""Per-point attributes on the upsampled cloud (the reference writes bare xyz).

A scan's columns after x y z - normals, colour, intensity, labels - are carried to the new points: every output point takes
the `k` nearest INPUT points (pf_knn_large, exact; `search="grid"`: pf_knn_grid, the same neighbours bit for bit from a uniform
grid of the cloud) and blends their rows by inverse squared distance, column segment by column segment as a plan says
(`parse_plan`).  `estimate_normals` fits a plane to every output point's own neighbourhood instead
(PCA in double on the device) and, asked to, gives the normals consistent signs by propagation along a minimum spanning
forest of the neighbour graph (csrc/normals_orient.hip).  All are HIP kernels (csrc/attr.hip); there is no CPU path.

  plan = parse_plan("normal,lin3,near1", columns=10)         # a 10-column file: xyz | normal | 3 blended | 1 label
  out_attr = transfer(pred, cloud_xyz, cloud_attr, plan)     # [M,3], [N,3], [N,7] -> [M,7]
  normals, variation = estimate_normals(pred, 16)            # [M,3] -> [M,3], [M]
  normals, variation = estimate_normals(pred, 16, orient="propagate")       # signs consistent over the surface
  normals, comp = orient_normals(pred, file_normals, 16)     # the same for normals that came from elsewhere
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import torch

from . import _lib, ops

MAX_COLUMNS = _lib.PF_ATTR_MAX_C
MAX_K = _lib.PF_ATTR_MAX_K
NORMALS_MIN_K, NORMALS_MAX_K = _lib.PF_NORMALS_MIN_K, _lib.PF_NORMALS_MAX_K
KINDS = {"lin": _lib.PF_ATTR_LIN, "unit": _lib.PF_ATTR_UNIT, "near": _lib.PF_ATTR_NEAR}


class Segment(NamedTuple):
    kind: str            # "lin": weighted sum | "unit": a direction (3 columns) | "near": the nearest input point's values
    cols: int


def parse_plan(text: str, columns: Optional[int] = None) -> List[Segment]:
    """"normal,lin3,near1" -> [Segment("unit", 3), Segment("lin", 3), Segment("near", 1)].  `normal` is 3 columns of kind unit
    (at most once), lin<C> / near<C> are C >= 1 columns each, at most MAX_COLUMNS in all.  columns: the file's column count - the
    plan must cover exactly its columns 4 ... .  Raises ValueError."""
    import re
    plan: List[Segment] = []
    for tok in (t.strip() for t in str(text).split(",")):
        m = re.fullmatch(r"(lin|near)(\d+)", tok)
        if tok == "normal":
            if any(s.kind == "unit" for s in plan):
                raise ValueError(f"attribute plan {text!r}: `normal` appears twice")
            plan.append(Segment("unit", 3))
        elif m and int(m.group(2)) >= 1:
            plan.append(Segment(m.group(1), int(m.group(2))))
        else:
            raise ValueError(f"attribute plan {text!r}: {tok!r} is not `normal`, `lin<C>` or `near<C>` with C >= 1")
    total = sum(s.cols for s in plan)
    if total > MAX_COLUMNS:
        raise ValueError(f"attribute plan {text!r} covers {total} columns; at most {MAX_COLUMNS} are carried")
    if columns is not None and total != int(columns) - 3:
        raise ValueError(f"attribute plan {text!r} covers {total} columns, the file has {int(columns) - 3} after x y z")
    return plan


def has_normal(plan: Sequence[Segment]) -> bool:
    return any(s.kind == "unit" for s in plan)


def _segments(plan):
    if isinstance(plan, str):
        plan = parse_plan(plan)
    return [(KINDS[kind], int(cols)) for kind, cols in plan]


def _k(k: int, n: int) -> int:
    k = int(k)
    if not 1 <= k <= MAX_K or k > int(n):
        raise _lib.PuflowHipError(f"attributes: k = {k} neighbours in a cloud of {int(n)} points; 1 .. {MAX_K} (and at most the "
                                  "cloud) are supported")
    return k


SEARCHES = ("brute", "grid")


def _search(search: str, ragged: bool):
    """the neighbour search of a `search=` argument: "brute" = pf_knn_large (one workgroup sorts the whole cloud per query), "grid"
    = pf_knn_grid (a uniform grid of the cloud, csrc/knn_grid.hip) - the same indices and distances bit for bit, so everything
    below produces the same bytes with either"""
    if search not in SEARCHES:
        raise ValueError(f"search = {search!r}: one of {', '.join(SEARCHES)}")
    if search == "grid":
        return ops.knn_grid_ragged if ragged else ops.knn_grid
    return ops.knn_large_ragged if ragged else ops.knn_large


def transfer(pred: torch.Tensor, cloud_xyz: torch.Tensor, cloud_attr: torch.Tensor, plan, k: int = 8,
             search: str = "brute") -> torch.Tensor:
    """The input cloud's attribute rows on the output points: pred [M,3] (or [B,M,3]), cloud_xyz [N,3] ([B,N,3]), cloud_attr
    [N,C] ([B,N,C]) -> [M,C] ([B,M,C]).  An output point that IS an input point gets that point's row bit for bit.  One search
    and one blend launch for the whole batch."""
    knn = _search(search, False)
    single = pred.dim() == 2
    if single:
        pred, cloud_xyz, cloud_attr = pred[None], cloud_xyz[None], cloud_attr[None]
    idx, d2 = knn(cloud_xyz, pred, _k(k, cloud_xyz.shape[1]))
    out = ops.attr_blend(idx, d2, cloud_attr, _segments(plan))
    return out[0] if single else out


def transfer_ragged(preds, clouds_xyz, clouds_attr, plan, k: int = 8, search: str = "brute") -> List[torch.Tensor]:
    """transfer for clouds of different sizes (lists of [M_i,3], [N_i,3], [N_i,C]) in one search and one blend launch; every
    cloud gets what transfer gives it alone."""
    knn = _search(search, True)
    nl, ml = [int(c.shape[0]) for c in clouds_xyz], [int(p.shape[0]) for p in preds]
    idx, d2 = knn(torch.cat(list(clouds_xyz), dim=0), nl, torch.cat(list(preds), dim=0), ml, _k(k, min(nl)))
    out = ops.attr_blend_ragged(idx, d2, torch.cat(list(clouds_attr), dim=0), nl, ml, _segments(plan))
    return list(torch.split(out, ml))


def _normals_k(k: int, m: int) -> int:
    k = int(k)
    if not _lib.PF_NORMALS_MIN_K <= k <= _lib.PF_NORMALS_MAX_K or k > m:
        raise _lib.PuflowHipError(f"estimate_normals: k = {k} neighbours on a cloud of {m} points; "
                                  f"{_lib.PF_NORMALS_MIN_K} .. {_lib.PF_NORMALS_MAX_K} (and at most the cloud) are supported")
    return k


ORIENTS = ("point", "propagate")


def _orient(orient: str) -> bool:
    if orient not in ORIENTS:
        raise ValueError(f"orient = {orient!r}: one of {', '.join(ORIENTS)}")
    return orient == "propagate"


def _orient_k(k: int, m: int) -> int:
    k = int(k)
    if not 2 <= k <= _lib.PF_KNN_GRID_MAX_K or k > m:
        raise _lib.PuflowHipError(f"orient_normals: k = {k} neighbours on a cloud of {m} points; 2 .. {_lib.PF_KNN_GRID_MAX_K} "
                                  "(and at most the cloud) are supported")
    return k


def estimate_normals(pred: torch.Tensor, k: int, viewpoint=None, search: str = "brute", orient: str = "point"):
    """A unit normal and the surface variation l0 / (l0 + l1 + l2) per point of pred [M,3] (or [B,M,3]) from the PCA of its k
    nearest points (itself included).  Sign, orient="point": every point on its own, towards `viewpoint` (three numbers) when
    given; else away from the cloud's centroid, a heuristic that is right for star-shaped objects seen from their centroid and
    wrong in cavities and on inner walls (the whole inner ring of a torus).  orient="propagate": the signs are carried along
    the minimum spanning forest of the same k-neighbour graph (orient_normals; no second search), which is right on every
    closed piece the graph holds together."""
    knn, propagate = _search(search, False), _orient(orient)
    single = pred.dim() == 2
    if single:
        pred = pred[None]
    idx, _ = knn(pred, pred, _normals_k(k, pred.shape[1]))
    normal, var = ops.normals_pca(pred, idx, viewpoint)
    if propagate:
        normal, _ = ops.normals_orient(pred, normal, idx, viewpoint, out=normal)
    return (normal[0], var[0]) if single else (normal, var)


def estimate_normals_ragged(preds, k: int, viewpoint=None, search: str = "brute", orient: str = "point"):
    """estimate_normals for clouds of different sizes in one search and one launch: ([normals_i], [variation_i])"""
    knn, propagate = _search(search, True), _orient(orient)
    ml = [int(p.shape[0]) for p in preds]
    pts = torch.cat(list(preds), dim=0)
    idx, _ = knn(pts, ml, pts, ml, _normals_k(k, min(ml)))
    normal, var = ops.normals_pca_ragged(pts, idx, ml, viewpoint)
    if propagate:
        normal, _ = ops.normals_orient_ragged(pts, normal, idx, ml, viewpoint)
    return list(torch.split(normal, ml)), list(torch.split(var, ml))


def orient_normals(pts: torch.Tensor, normals: torch.Tensor, k: int, viewpoint=None, search: str = "brute", idx=None):
    """Consistent signs for any normals (estimated, or carried from a file): pts, normals [M,3] (or [B,M,3]) -> (normals with
    every row kept or negated, comp int32 [M]: the smallest index of the row's connected component).  The graph is the k
    nearest neighbours of every point (idx int32 [.., M, k] from ops.knn_large / knn_grid skips the search), the signs follow
    its minimum spanning forest under the weights 1 - |n_i . n_j| (Hoppe et al. 1992), and each component's highest point - with
    `viewpoint` the one nearest to it - looks up, or at the viewpoint.  The result does not depend on the signs that came in.
    A graph that falls into several components is oriented piece by piece: right for closed pieces, a guess for fragments;
    components are not joined, and sheets closer together than a neighbourhood can still flip."""
    knn = _search(search, False)
    single = pts.dim() == 2
    if single:
        pts, normals = pts[None], normals[None]
        idx = idx[None] if idx is not None else None
    if idx is None:
        idx, _ = knn(pts, pts, _orient_k(k, pts.shape[1]))
    out, comp = ops.normals_orient(pts, normals, idx, viewpoint)
    return (out[0], comp[0]) if single else (out, comp)


def orient_normals_ragged(pts_list, normals_list, k: int, viewpoint=None, search: str = "brute", idx=None):
    """orient_normals for clouds of different sizes in one search and one pass: ([normals_i], [comp_i]); idx: the packed
    [sum M_i, k] int32 lists of ops.knn_large_ragged / knn_grid_ragged"""
    knn = _search(search, True)
    ml = [int(p.shape[0]) for p in pts_list]
    pts, normals = torch.cat(list(pts_list), dim=0), torch.cat(list(normals_list), dim=0)
    if idx is None:
        idx, _ = knn(pts, ml, pts, ml, _orient_k(k, min(ml)))
    out, comp = ops.normals_orient_ragged(pts, normals, idx, ml, viewpoint)
    return list(torch.split(out, ml)), list(torch.split(comp, ml))
