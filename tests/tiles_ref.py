"""Numpy restatements for the tiled passes (puflow_amd/tiles.py, csrc/tiles.hip, pf_fps_ragged_ctx).  TEST INFRASTRUCTURE ONLY.

FPS arithmetic is oracle/patch_ref.py's: fp32 (dx^2 + dy^2) + dz^2 on coordinate planes, running minimum, first maximal value,
1e10 as the initial distance of a cloud without a context."""
from __future__ import annotations

import math

import numpy as np


def sqd_to(p: np.ndarray, c: np.ndarray) -> np.ndarray:
    """squared fp32 distances of the points p [N,3] to the point c [3], unfused: ((dx dx) + (dy dy)) + (dz dz)"""
    p = np.asarray(p, np.float32)
    c = np.asarray(c, np.float32)
    t0 = p[:, 0] - c[0]
    t0 = t0 * t0
    t1 = p[:, 1] - c[1]
    t1 = t1 * t1
    t0 = t0 + t1
    t1 = p[:, 2] - c[2]
    t1 = t1 * t1
    return (t0 + t1).astype(np.float32)


def fps_ctx(p: np.ndarray, npoint: int, ctx=None):
    """FPS of p [N,3] with a fixed context ctx [C,3] (None / empty: plain FPS from index 0) -> (idx int64 [npoint],
    d float32 [npoint]: the min-distance every sample had when it was taken; d[-1] is the kernel's r2_out)."""
    p = np.ascontiguousarray(np.asarray(p, np.float32))
    N = p.shape[0]
    mind = np.full(N, 1e10, np.float32)
    idx = np.zeros(npoint, np.int64)
    d = np.zeros(npoint, np.float32)
    if ctx is not None and len(ctx):
        for c in np.asarray(ctx, np.float32):
            np.minimum(mind, sqd_to(p, c), out=mind)
        start = 0
    else:
        idx[0], d[0] = 0, mind[0]
        np.minimum(mind, sqd_to(p, p[0]), out=mind)
        start = 1
    for j in range(start, npoint):
        cur = int(np.argmax(mind))                   # first maximal value
        idx[j], d[j] = cur, mind[cur]
        np.minimum(mind, sqd_to(p, p[cur]), out=mind)
    return idx, d


def min_pair_sqd(p: np.ndarray) -> np.float32:
    """smallest squared distance between two different rows of p, in the FPS arithmetic (fp32)"""
    p = np.asarray(p, np.float32)
    best = np.float32(np.inf)
    for i in range(1, p.shape[0]):
        best = min(best, sqd_to(p[:i], p[i]).min())
    return np.float32(best)


def kd_depth(n: int, tile_points: int) -> int:
    return max(0, math.ceil(math.log2(n / tile_points))) if n > tile_points else 0


def kd_tiles(pc: np.ndarray, tile_points: int):
    """-> (order int64 [N]: point indices leaf after leaf, offsets int64 [T+1], (axis int32 [T-1], split float32 [T-1]) in heap
    order, boxes float32 [T,6]).  Every leaf at depth L = ceil(log2(N / tile_points)); a node splits the widest axis of its
    points' bounding box (first of equals) by rank: the left child gets floor(n/2) points in (coordinate, index) order, the
    split value is the first right point's coordinate.  Leaf boxes from the split planes, outer faces +-inf."""
    pc = np.asarray(pc, np.float32)
    N = pc.shape[0]
    L = kd_depth(N, tile_points)
    T = 1 << L
    axis, split = np.zeros(T - 1, np.int32), np.zeros(T - 1, np.float32)
    nodes = [(np.arange(N, dtype=np.int64), np.array([-np.inf] * 3 + [np.inf] * 3, np.float32))]
    for l in range(L):
        nxt = []
        for k, (ids, box) in enumerate(nodes):
            node = (1 << l) - 1 + k
            pts = pc[ids]
            a = int(np.argmax(pts.max(0) - pts.min(0)))
            srt = ids[np.lexsort((ids, pts[:, a]))]              # by coordinate, then by index
            h = len(ids) // 2
            s = pc[srt[h], a]
            axis[node], split[node] = a, s
            lb, rb = box.copy(), box.copy()
            lb[3 + a], rb[a] = s, s
            nxt += [(srt[:h], lb), (srt[h:], rb)]
        nodes = nxt
    order = np.concatenate([ids for ids, _ in nodes])
    offsets = np.concatenate([[0], np.cumsum([len(ids) for ids, _ in nodes])]).astype(np.int64)
    return order, offsets, (axis, split), np.stack([b for _, b in nodes])


def kd_descend(pts: np.ndarray, axis: np.ndarray, split: np.ndarray, L: int) -> np.ndarray:
    """leaf of every point: right iff p[axis] >= split"""
    pts = np.asarray(pts, np.float32)
    k = np.zeros(pts.shape[0], np.int64)
    for _ in range(L):
        k = 2 * k + 1 + (pts[np.arange(pts.shape[0]), axis[k]] >= split[k])
    return k - ((1 << L) - 1)


def box_members(pts: np.ndarray, boxes: np.ndarray):
    pts = np.asarray(pts, np.float32)
    return [np.nonzero(((pts >= b[:3]) & (pts <= b[3:])).all(1))[0] for b in np.asarray(boxes, np.float32)]


def box_gap2(a: np.ndarray, b: np.ndarray) -> float:
    """squared distance between two boxes (0 when they touch or overlap)"""
    gap = np.maximum(0.0, np.maximum(a[:3].astype(np.float64) - b[3:], b[:3].astype(np.float64) - a[3:]))
    return float((gap * gap).sum())


def conflicts(boxes: np.ndarray, h: float):
    T = len(boxes)
    return [[u for u in range(T) if u != t and box_gap2(boxes[t], boxes[u]) < h * h] for t in range(T)]


def colour_greedy(boxes: np.ndarray, h: float):
    """colours of the tiles, greedily in index order: the smallest colour no conflicting earlier tile has"""
    con = conflicts(boxes, h)
    col = []
    for t in range(len(boxes)):
        used = {col[u] for u in con[t] if u < t}
        c = 0
        while c in used:
            c += 1
        col.append(c)
    return col


def quotas(npoint: int, cores):
    """largest remainder apportionment of npoint over the tiles by core point count (ties: lower tile first)"""
    tot = sum(cores)
    base = [npoint * c // tot for c in cores]
    rem = sorted(range(len(cores)), key=lambda t: (-(npoint * cores[t] % tot), t))
    for t in rem[: npoint - sum(base)]:
        base[t] += 1
    return base
