"""Tiled passes: one large cloud through the patch pipeline in k-d tiles, merged by FPS with a fixed context (DESIGN.md 8,
"Tiled passes"; no reference counterpart).

The FPS merge of `PatchHelper.upsample` selects 4N points out of 20N candidates and is O(N^2); beyond 13 107 input points it
also leaves the cooperative kernel.  Here the cloud is cut into cells of about `tile_points` points by a k-d tree, every cell
makes its candidates from its points plus a halo, keeps the candidates that fall into the cell, and selects its share of the
output by FPS.  Cells that are close to each other are merged one after the other (greedy colouring), and a later cell starts
from the samples earlier cells have put within `h` of it: pf_fps_ragged_ctx.

The invariant: with r2[t] the min-distance of tile t's last sample, every two output points are at least sqrt(min_t r2[t])
apart - as in a global FPS, whose last min-distance bounds all pairs.  (Two samples of one tile, or a sample and a context
point: the later one had at least r2[t] to the earlier when it was taken.  Anything else is more than h apart, and r2[t] <= h^2
is checked.)

The geometry queries run in the HIP library (csrc/tiles.hip: box query, cell assignment); sorting, index arithmetic and the
host-side colouring are plumbing in torch / Python.
"""
from __future__ import annotations

import math

import torch
from torch import Tensor

from . import _lib, ops

FPS_COOP_MAX = 262144            # candidates the cooperative FPS kernel takes per cloud (FPSC_GMAX x 1024 x 8)


def kd_depth(n: int, tile_points: int) -> int:
    return max(0, math.ceil(math.log2(n / tile_points))) if n > tile_points else 0


def kd_tiles(pc: Tensor, tile_points: int):
    """pc [N,3] -> (order int64 [N]: point indices leaf after leaf, offsets: HOST list of T + 1 ints, tree = (axis int32 [T-1],
    split float32 [T-1], depth L) in heap order for ops.kd_assign, boxes float32 [T,6]).  Every leaf sits at depth
    L = ceil(log2(N / tile_points)).  A node splits the widest axis of its points' bounding box (the first of equals) by rank:
    the left child gets floor(n/2) points in (coordinate, index) order, the split value is the first right point's coordinate.
    Leaf boxes come from the split planes; outer faces are +-inf.  The leaf sizes follow from N alone: nothing is read back."""
    pc = pc.reshape(-1, 3).float()
    N, dev = pc.shape[0], pc.device
    L = kd_depth(N, int(tile_points))
    T = 1 << L
    if N < T:
        raise _lib.PuflowHipError(f"kd_tiles: {N} points cannot fill {T} tiles")
    inf = float("inf")
    order = torch.arange(N, device=dev)
    sizes = [N]
    axis_all = torch.zeros((T - 1,), dtype=torch.int32, device=dev)
    split_all = torch.zeros((T - 1,), dtype=torch.float32, device=dev)
    boxes = torch.tensor([[-inf] * 3 + [inf] * 3], dtype=torch.float32, device=dev)
    for l in range(L):
        nn = len(sizes)
        cnt = torch.tensor(sizes, dtype=torch.int64)
        first = (torch.cumsum(cnt, 0) - cnt).to(dev)
        seg = torch.repeat_interleave(torch.arange(nn, device=dev), cnt.to(dev), output_size=N)
        p = pc[order]
        seg3 = seg.view(-1, 1).expand(-1, 3)
        lo = torch.full((nn, 3), inf, device=dev).scatter_reduce_(0, seg3, p, "amin")
        hi = torch.full((nn, 3), -inf, device=dev).scatter_reduce_(0, seg3, p, "amax")
        ext = hi - lo
        a = torch.where(ext[:, 1] > ext[:, 0], 1, 0)                       # the first of equal extents
        a = torch.where(ext[:, 2] > torch.maximum(ext[:, 0], ext[:, 1]), 2, a)
        key = p.gather(1, a[seg].view(-1, 1))[:, 0]
        # positions by (node, coordinate, point index): three stable sorts, least significant key first
        idx = torch.argsort(order, stable=True)
        idx = idx[torch.argsort(key[idx], stable=True)]
        idx = idx[torch.argsort(seg[idx], stable=True)]
        order = order[idx]
        half = [s // 2 for s in sizes]
        s_val = pc[order[first + torch.tensor(half, dtype=torch.int64).to(dev)], a]
        axis_all[nn - 1: 2 * nn - 1] = a.int()
        split_all[nn - 1: 2 * nn - 1] = s_val
        rows = torch.arange(nn, device=dev)
        lb, rb = boxes.clone(), boxes.clone()
        lb[rows, 3 + a] = s_val
        rb[rows, a] = s_val
        boxes = torch.stack([lb, rb], dim=1).reshape(-1, 6)
        sizes = [v for s, h in zip(sizes, half) for v in (h, s - h)]
    offsets = [0]
    for s in sizes:
        offsets.append(offsets[-1] + s)
    return order, offsets, (axis_all, split_all, L), boxes


def box_gap2(a, b) -> float:
    """squared distance between two boxes [lo xyz, hi xyz] (0 when they touch or overlap)"""
    g2 = 0.0
    for c in range(3):
        g = max(0.0, float(a[c]) - float(b[3 + c]), float(b[c]) - float(a[3 + c]))
        g2 += g * g
    return g2


def colour_tiles(boxes, h: float):
    """Greedy colouring in index order on the host: two tiles conflict when their boxes are closer than h; a tile takes the
    smallest colour no conflicting earlier tile has.  boxes: T rows of 6 floats."""
    col = []
    for t in range(len(boxes)):
        used = {col[u] for u in range(t) if box_gap2(boxes[t], boxes[u]) < h * h}
        c = 0
        while c in used:
            c += 1
        col.append(c)
    return col


def quotas(npoint: int, cores):
    """largest-remainder apportionment of npoint over the tiles by core point count (equal remainders: the lower tile first)"""
    tot = sum(cores)
    base = [npoint * c // tot for c in cores]
    rem = sorted(range(len(cores)), key=lambda t: (-(npoint * cores[t] % tot), t))
    for t in rem[: npoint - sum(base)]:
        base[t] += 1
    return base


@torch.no_grad()
def upsample_tiled(helper, upsampler, pc: Tensor, npoint: int, upratio=None, tile_points: int = 4096, halo: float = 1.0,
                   tiles_per_pass: int = 64, return_stats: bool = False, _stage=None, **kwargs):
    """PatchHelper.upsample_tiled.  _stage(name): called when a stage has been queued (tools/time_tiled.py synchronises there)."""
    stage = _stage if _stage is not None else (lambda name: None)
    pc = pc.reshape(-1, 3)
    N, k, dev = pc.shape[0], helper._npoint_patch, pc.device
    npoint = int(npoint)
    if int(tile_points) >= N:                                    # a single tile with no context: the untiled pipeline itself
        out = helper.upsample(upsampler, pc[None], npoint, upratio, **kwargs)[0]
        if not return_stats:
            return out
        n_patch = int(N / k * helper._patch_expand_ratio)
        return out, {"tiles": 1, "colours": 1, "colour": [0], "core": [N], "working": [N],
                     "candidates": [n_patch * k * ((upratio or 4) + 1)], "quota": [npoint], "context": [0], "h": None, "r2": None,
                     "normalised": None}
    # 1. normalise; tile in normalised space
    pcn, g_centroid, g_furthest_distance = ops.normalize_pc(pc[None])
    order, offsets, (axis, split, L), boxes = kd_tiles(pcn[0], tile_points)
    pts = pcn[0][order].contiguous()                             # the cloud in tile order
    T = len(offsets) - 1
    core = [offsets[t + 1] - offsets[t] for t in range(T)]
    stage("tiling")
    # 2. patch radius: the median over the tiles' first points of the distance to the k-th neighbour in the whole cloud
    first = torch.tensor(offsets[:-1], dtype=torch.int64).to(dev)
    dist, _ = ops.KNN(k=k, transpose_mode=True)(pts[None], pts[first][None])
    h_dev = float(halo) * dist[0, :, k - 1].sqrt().median()
    # 3. working sets: the points inside the tile's box grown by h (its core and the halo from the other tiles)
    grow = torch.cat([-h_dev.expand(3), h_dev.expand(3)])
    grown = (boxes + grow).contiguous()
    ws_count = ops.box_count(pts, grown)
    host = torch.cat([h_dev.double().view(1), ws_count.double(), boxes.double().flatten()]).cpu()      # the one host read
    h = float(host[0])
    working = [int(v) for v in host[1: 1 + T].tolist()]
    boxes_host = host[1 + T:].view(T, 6).tolist()
    for t in range(T):
        if working[t] < k:
            raise _lib.PuflowHipError(f"tile {t}: {working[t]} points in its working set, fewer than one patch ({k})")
    ws_off, ws_member = ops.box_fill(pts, grown, working)
    w_first = [0]
    for w in working:
        w_first.append(w_first[-1] + w)
    stage("halo")
    # 4. + 5. candidates of the working sets, `tiles_per_pass` tiles at a time; a tile keeps those that fall into its own cell
    kept, kept_cnt = [], []
    per_pass = max(int(tiles_per_pass), 1)
    for t0 in range(0, T, per_pass):
        t1 = min(T, t0 + per_pass)
        lens = working[t0:t1]
        index = helper._ragged_index(lens, upratio, dev)
        cand = helper._ragged_candidates(upsampler, pts[ws_member[w_first[t0]: w_first[t1]].long()], lens, upratio, index, **kwargs)
        stage("network")
        leaf = ops.kd_assign(cand, axis, split, L)
        cnt = torch.tensor(index[3], dtype=torch.int64)
        tile = torch.repeat_interleave(torch.arange(t0, t1), cnt, output_size=int(cnt.sum())).to(dev)
        own = leaf.long() == tile
        kept.append(cand[own])
        kept_cnt.append(torch.zeros((t1 - t0,), dtype=torch.int64, device=dev).scatter_add_(0, tile[own] - t0, own[own].long()))
        stage("ownership")
    cands = [int(v) for v in torch.cat(kept_cnt).tolist()]
    kept = torch.cat(kept)
    k_first = [0]
    for c in cands:
        k_first.append(k_first[-1] + c)
    # 6. quotas
    quota = quotas(npoint, core)
    for t in range(T):
        if cands[t] < quota[t]:
            raise _lib.PuflowHipError(f"tile {t}: {cands[t]} candidates in its cell, fewer than its share of the output "
                                      f"({quota[t]} of {npoint})")
        if cands[t] > FPS_COOP_MAX:
            raise _lib.PuflowHipError(f"tile {t}: {cands[t]} candidates, more than the cooperative FPS kernel takes "
                                      f"({FPS_COOP_MAX}); choose a smaller `tile_points`")
    # 7. colouring
    h_ctx = h
    colour = colour_tiles(boxes_host, h_ctx)
    h2 = float(torch.tensor(h_ctx, dtype=torch.float32) * torch.tensor(h_ctx, dtype=torch.float32))
    # 8. merging: colours in sequence, one colour's tiles in one pass; a tile's context = the samples of earlier colours inside
    # its box grown by h_ctx
    samples = [None] * T
    r2 = [None] * T
    n_ctx = [0] * T
    selected = None
    for c in range(max(colour) + 1):
        ts = [t for t in range(T) if colour[t] == c and quota[t] > 0]
        if not ts:
            continue
        xyz = torch.cat([kept[k_first[t]: k_first[t + 1]] for t in ts]).contiguous()
        ctx, ctx_len = None, None
        if selected is not None:
            g = grown[torch.tensor(ts, dtype=torch.int64).to(dev)].contiguous()
            ctx_cnt, _, member = ops.box_query(selected, g)
            ctx_len = [int(v) for v in ctx_cnt.tolist()]
            ctx = selected[member.long()].contiguous() if sum(ctx_len) else None
            for t, n in zip(ts, ctx_len):
                n_ctx[t] = n
        try:
            idx, rad = ops.furthest_point_sample_ragged(xyz, [cands[t] for t in ts], [quota[t] for t in ts], context=ctx,
                                                        context_lengths=ctx_len if ctx is not None else None, return_radius=True,
                                                        radius_limit=h2)
        except ops.FpsRadiusError as e:
            raise _lib.PuflowHipError(f"tiles {[ts[i] for i in e.clouds]}: too sparse for the context radius ({h_ctx:g}): the last "
                                      "sample lies farther than that from every sample and context point; choose a larger "
                                      "`tile_points` or `halo`") from None
        x_first, _, _ = helper._rows([cands[t] for t in ts], dev)
        _, o_cloud, _ = helper._rows([quota[t] for t in ts], dev)
        got = xyz[idx.long() + x_first[o_cloud]]
        for t, s, r in zip(ts, torch.split(got, [quota[t] for t in ts]), rad.unbind(0)):
            samples[t], r2[t] = s, r
        selected = got if selected is None else torch.cat([selected, got])
        stage(f"merge colour {c}")
    # 9. de-normalise; the tiles' samples in tile order
    out_n = torch.cat([s for s in samples if s is not None])
    out = (out_n * g_furthest_distance.view(1, 1) + g_centroid.view(1, 3)).contiguous()
    if not return_stats:
        return out
    r2_all = torch.stack([r if r is not None else torch.zeros((), device=dev) for r in r2]).cpu()
    return out, {"tiles": T, "colours": max(colour) + 1, "colour": colour, "core": core, "working": working, "candidates": cands,
                 "quota": quota, "context": n_ctx, "h": h, "h2": h2, "r2": r2_all, "normalised": out_n, "boxes": boxes,
                 "tree": (axis, split, L), "kept": kept, "kept_first": k_first}
