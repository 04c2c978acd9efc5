"""Operator surface the reference model calls, backed by the HIP library.

Signatures mirror the third-party ops the reference imports:
  knn_points / knn_gather     pytorch3d.ops           (modules/discrete/interpflow.py:9,104,229,328)
  chamfer_distance            pytorch3d.loss          (metric/loss.py:14,42)
  history_chamfer_distance    kaolin.metrics.pointcloud (metric/loss.py:12,35)
All tensors must live on the GPU; there is no CPU path here.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.PuflowHipError("puflow_amd ops need GPU tensors (no CPU fallback)")
    return t.detach().contiguous().float()


def knn_idx32(p1: torch.Tensor, p2: torch.Tensor, K: int, want_dist: bool = False):
    """int32 device-format kNN: idx [B,N,K] (+ dists)."""
    lib = _lib.load()
    p1, p2 = _f32c(p1), _f32c(p2)
    B, N, _ = p1.shape
    M = p2.shape[1]
    idx = torch.empty((B, N, K), dtype=torch.int32, device=p1.device)
    dist = torch.empty((B, N, K), dtype=torch.float32, device=p1.device) if want_dist else None
    dptr = dist.data_ptr() if want_dist else None
    if K in (4, 8, 16, 32):
        _lib.check(lib.pf_knn(p1.data_ptr(), p2.data_ptr(), B, N, M, K, idx.data_ptr(), dptr, _stream()), "pf_knn")
    else:                       # any other K: sort-based kernel (same (distance, index) order), M <= 16384
        _lib.check(lib.pf_knn_large(p2.data_ptr(), p1.data_ptr(), B, M, N, K, idx.data_ptr(), dptr, _stream()), "pf_knn_large")
    return idx, dist


def _chamfer_bwd(lib):
    """pf_chamfer_bwd, or its atomics-free form under train_state.set_deterministic(True) (a debugging switch)."""
    from . import train_state
    return lib.pf_chamfer_bwd_det if train_state.deterministic() else lib.pf_chamfer_bwd


def knn_points(p1: torch.Tensor, p2: torch.Tensor, K: int, return_nn: bool = False, return_sorted: bool = True,
               **_unused) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """(dists [B,N,K] squared L2, idx [B,N,K] int64, nn or None); always sorted by (dist, idx)."""
    idx, dist = knn_idx32(p1, p2, K, want_dist=True)
    idx64 = idx.long()
    nn = knn_gather(p2, idx64) if return_nn else None
    return dist, idx64, nn


def knn_gather(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """out[b,n,k,:] = x[b, idx[b,n,k], :]  (plain indexing; data movement only)."""
    B = x.shape[0]
    return x[torch.arange(B, device=x.device).view(B, 1, 1), idx.long()]


# ----------------------------------------------------------------------------------------
# Chamfer
# ----------------------------------------------------------------------------------------
def chamfer_nn(x: torch.Tensor, y: torch.Tensor):
    """dist1 [B,N], dist2 [B,M], idx1, idx2 (int32) + per-sample (mean+mean) [B] and {mean_b, sum_b} [2]."""
    lib = _lib.load()
    x, y = _f32c(x), _f32c(y)
    B, N, _ = x.shape
    M = y.shape[1]
    dev = x.device
    d1 = torch.empty((B, N), dtype=torch.float32, device=dev)
    d2 = torch.empty((B, M), dtype=torch.float32, device=dev)
    i1 = torch.empty((B, N), dtype=torch.int32, device=dev)
    i2 = torch.empty((B, M), dtype=torch.int32, device=dev)
    per = torch.empty((B,), dtype=torch.float32, device=dev)
    ms = torch.empty((2,), dtype=torch.float32, device=dev)
    _lib.check(lib.pf_chamfer_fwd(x.data_ptr(), y.data_ptr(), B, N, M, d1.data_ptr(), i1.data_ptr(), d2.data_ptr(),
                                  i2.data_ptr(), per.data_ptr(), ms.data_ptr(), _stream()), "pf_chamfer_fwd")
    return d1, d2, i1, i2, per, ms


class _ChamferFn(torch.autograd.Function):
    """outputs: per-sample chamfer [B] (mean over points of both directions)."""

    @staticmethod
    def forward(ctx, x, y):
        xc, yc = _f32c(x), _f32c(y)
        d1, d2, i1, i2, per, _ = chamfer_nn(xc, yc)
        ctx.save_for_backward(xc, yc, i1, i2)
        return per

    @staticmethod
    def backward(ctx, gper):
        x, y, i1, i2 = ctx.saved_tensors
        lib = _lib.load()
        B, N, _ = x.shape
        M = y.shape[1]
        gper = gper.contiguous().float()
        g1 = (gper / N).view(B, 1).expand(B, N).contiguous()
        g2 = (gper / M).view(B, 1).expand(B, M).contiguous()
        gx, gy = torch.zeros_like(x), torch.zeros_like(y)
        _lib.check(_chamfer_bwd(lib)(x.data_ptr(), y.data_ptr(), i1.data_ptr(), i2.data_ptr(), g1.data_ptr(),
                                      g2.data_ptr(), gx.data_ptr(), gy.data_ptr(), B, N, M, _stream()), "pf_chamfer_bwd")
        return gx, gy


def chamfer_distance(x, y, x_normals=None, y_normals=None, batch_reduction="mean", point_reduction="mean"):
    """pytorch3d.loss.chamfer_distance surface used by the reference (metric/loss.py:42): -> (loss, None)."""
    if x_normals is not None or y_normals is not None:
        raise NotImplementedError("normals are never passed on the PU-Flow path (train_pugan.py:60)")
    if point_reduction != "mean" or batch_reduction not in ("mean", "sum"):
        raise NotImplementedError("only the reductions the reference uses are built")
    per = _ChamferFn.apply(x, y)
    return (per.mean() if batch_reduction == "mean" else per.sum()), None


def history_chamfer_distance(p1, p2):
    """kaolin.metrics.pointcloud.chamfer_distance surface (metric/loss.py:35): per-sample [B]."""
    return _ChamferFn.apply(p1, p2)


def nearest_distance(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """dist1 of chamfer_3DDist alone: squared distance of every point of x [B,N,3] to its nearest point of y [B,M,3] -> [B,N]
    (pf_nn1; PatchHelper.remove_outliers uses only this half, modules/utils/patch.py:199-203)."""
    lib = _lib.load()
    x, y = _f32c(x), _f32c(y)
    B, N, _ = x.shape
    d1 = torch.empty((B, N), dtype=torch.float32, device=x.device)
    _lib.check(lib.pf_nn1(x.data_ptr(), y.data_ptr(), B, N, y.shape[1], d1.data_ptr(), None, _stream()), "pf_nn1")
    return d1


class chamfer_3DDist:
    """ChamferDistancePytorch surface used by PatchHelper.remove_outliers (modules/utils/patch.py:199-203)."""

    def __call__(self, a, b):
        d1, d2, i1, i2, _, _ = chamfer_nn(a, b)
        return d1, d2, i1, i2


# ----------------------------------------------------------------------------------------
# Patch pipeline operators (pointnet2_ops / knn_cuda surfaces used by modules/utils/patch.py)
# ----------------------------------------------------------------------------------------
def furthest_point_sample(xyz: torch.Tensor, npoint: int, group: int = 0) -> torch.Tensor:
    """pointnet2_ops.pointnet2_utils.furthest_point_sample: xyz [B,N,3] -> int32 [B,npoint] (starts at index 0).
    group > 0: a layout hint, not a change of the result - every `group` consecutive points are one spatial neighbourhood
    (pf_fps_grouped: the cooperative kernel then gives a wave exactly one neighbourhood when it can)."""
    lib = _lib.load()
    xyz = _f32c(xyz)
    B, N, _ = xyz.shape
    idx = torch.zeros((B, npoint), dtype=torch.int32, device=xyz.device)
    mind = torch.empty((B, N), dtype=torch.float32, device=xyz.device)
    _lib.check(lib.pf_fps_grouped(xyz.data_ptr(), B, N, npoint, int(group), mind.data_ptr(), idx.data_ptr(), _stream()), "pf_fps")
    _check_fps_abort(lib, mind, B, N)
    return idx


def _check_fps_abort(lib, mind: torch.Tensor, B: int, N: int) -> None:
    """The cooperative FPS kernel's workgroups wait for each other with a BOUNDED spin.  A cloud's status word is 0 only when
    all of its steps completed (2 = never finished / never started, 1 = its workgroups gave up waiting): anything else means
    an invalid index row.  One small device -> host read per call (FPS itself is tens of ms)."""
    import ctypes
    stride, word = ctypes.c_longlong(0), ctypes.c_longlong(0)
    if not lib.pf_fps_scratch_layout(N, ctypes.byref(stride), ctypes.byref(word)):
        return
    words = mind.view(-1)[: (B * N) // 2 * 2].view(torch.int64)
    pos = torch.arange(B, device=mind.device, dtype=torch.int64) * stride.value + word.value
    if bool((words[pos] != 0).any()):
        raise _lib.PuflowHipError("pf_fps: the cooperative kernel did not complete every cloud (its workgroups timed out "
                                  "waiting for each other or were never co-resident); the sampled indices are invalid")


def normalize_pc(pc: torch.Tensor):
    """PatchHelper.normalize_pc (modules/utils/patch.py:168-178) on the GPU: pc [B,N,3] -> (normalised [B,N,3],
    centroid [B,1,3], furthest distance [B,1,1]).  Fixed summation order per cloud: independent of the batch size."""
    lib = _lib.load()
    pc = _f32c(pc)
    B, N, _ = pc.shape
    out = torch.empty_like(pc)
    cen = torch.empty((B, 1, 3), dtype=torch.float32, device=pc.device)
    fd = torch.empty((B, 1, 1), dtype=torch.float32, device=pc.device)
    _lib.check(lib.pf_normalize_pc(pc.data_ptr(), B, N, out.data_ptr(), cen.data_ptr(), fd.data_ptr(), _stream()),
               "pf_normalize_pc")
    return out, cen, fd


def gather_operation(features: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """pointnet2 gather_operation: features [B,C,N], idx [B,M] -> [B,C,M] (indexing only)."""
    B, C, _ = features.shape
    return torch.gather(features, 2, idx.long().unsqueeze(1).expand(B, C, idx.shape[1]))


class KNN:
    """knn_cuda.KNN surface (modules/utils/patch.py:33,107): KNN(k, transpose_mode=False)(ref [B,C,N], query [B,C,M])
    -> (dist [B,k,M] squared L2, idx [B,k,M] int64), ordered by (distance, index)."""

    def __init__(self, k: int, transpose_mode: bool = False):
        self.k = k
        self.transpose_mode = transpose_mode

    def __call__(self, ref: torch.Tensor, query: torch.Tensor):
        lib = _lib.load()
        if not self.transpose_mode:
            ref, query = ref.transpose(1, 2), query.transpose(1, 2)
        ref, query = _f32c(ref), _f32c(query)
        B, N, _ = ref.shape
        M = query.shape[1]
        idx = torch.empty((B, M, self.k), dtype=torch.int32, device=ref.device)
        dist = torch.empty((B, M, self.k), dtype=torch.float32, device=ref.device)
        if self.k <= 32 and self.k in (4, 8, 16, 32):
            _lib.check(lib.pf_knn(query.data_ptr(), ref.data_ptr(), B, M, N, self.k, idx.data_ptr(), dist.data_ptr(),
                                  _stream()), "pf_knn")
        else:
            _lib.check(lib.pf_knn_large(ref.data_ptr(), query.data_ptr(), B, N, M, self.k, idx.data_ptr(), dist.data_ptr(),
                                        _stream()), "pf_knn_large")
        idx = idx.long()
        if not self.transpose_mode:
            return dist.transpose(1, 2).contiguous(), idx.transpose(1, 2).contiguous()
        return dist, idx


# ----------------------------------------------------------------------------------------
# Ragged ("packed") patch operators: B clouds of lengths[i] points stored back to back as one [sum, 3] tensor.
# Every cloud gets, bit for bit, what the dense operator above gives it alone; the lengths are host integers.
# ----------------------------------------------------------------------------------------
def _lengths(lengths, total: int, what: str):
    lengths = [int(v) for v in lengths]
    if not lengths or min(lengths) <= 0 or sum(lengths) != total:
        raise _lib.PuflowHipError(f"{what}: lengths {lengths} do not describe a packed tensor of {total} rows")
    return lengths


def _packed(t: torch.Tensor, what: str) -> torch.Tensor:
    t = _f32c(t)
    if t.dim() != 2 or t.shape[1] != 3:
        raise _lib.PuflowHipError(f"{what}: a packed cloud tensor is [sum of lengths, 3], got {tuple(t.shape)}")
    return t


def normalize_pc_ragged(pc: torch.Tensor, lengths):
    """normalize_pc per cloud of a packed tensor: pc [sum, 3] -> (normalised [sum, 3], centroid [B,1,3], furthest distance
    [B,1,1])."""
    lib = _lib.load()
    pc = _packed(pc, "normalize_pc_ragged")
    lengths = _lengths(lengths, pc.shape[0], "normalize_pc_ragged")
    B = len(lengths)
    out = torch.empty_like(pc)
    cen = torch.empty((B, 1, 3), dtype=torch.float32, device=pc.device)
    fd = torch.empty((B, 1, 1), dtype=torch.float32, device=pc.device)
    _lib.check(lib.pf_normalize_pc_ragged(pc.data_ptr(), _lib.counts(lengths), B, out.data_ptr(), cen.data_ptr(), fd.data_ptr(),
                                          _stream()), "pf_normalize_pc_ragged")
    return out, cen, fd


def fps_ragged_layout(lengths, group: int = 0):
    """pf_fps_ragged_layout (host only): dict with the scratch size in floats, every cloud's scratch offset (floats), its
    workgroups in the cooperative launch (0: single-workgroup kernel), the points per thread of that launch and the positions of
    the clouds' status words (64-bit words of the scratch)."""
    import ctypes
    lib = _lib.load()
    lengths = [int(v) for v in lengths]
    B = len(lengths)
    off, wgs = (ctypes.c_longlong * B)(), (ctypes.c_int * B)()
    total, word, stride = ctypes.c_longlong(0), ctypes.c_longlong(0), ctypes.c_longlong(0)
    ppt = lib.pf_fps_ragged_layout(_lib.counts(lengths), B, int(group), off, wgs, ctypes.byref(total), ctypes.byref(word),
                                   ctypes.byref(stride))
    if ppt < 0:
        _lib.check(int(ppt), "pf_fps_ragged_layout")
    return {"total_floats": total.value, "scratch_off": list(off), "workgroups": list(wgs), "ppt": int(ppt),
            "status_words": [word.value + i * stride.value for i in range(B)]}


def furthest_point_sample_ragged(xyz: torch.Tensor, lengths, npoints, group: int = 0, context=None, context_lengths=None,
                                 return_radius: bool = False, radius_limit=None):
    """furthest_point_sample per cloud of a packed tensor: xyz [sum, 3], npoints[i] samples of cloud i -> int32 [sum npoints],
    indices inside each cloud (every cloud starts at its index 0).  `group`: the layout hint of furthest_point_sample.
    context [sum context_lengths, 3] (pf_fps_ragged_ctx; no reference counterpart): points that are already taken, cloud after
    cloud - cloud i's min-distances start at the distance to its context and every sample, the first included, is the
    arg-max; a cloud with context_lengths[i] = 0 gets the samples it gets without the argument.  return_radius: also return
    float32 [B], the min-distance (squared) every cloud's last sample had when it was taken.  radius_limit: raise when a
    cloud's radius exceeds it - checked on the device and read back with the status words, in the same host read."""
    lib = _lib.load()
    xyz = _packed(xyz, "furthest_point_sample_ragged")
    lengths = _lengths(lengths, xyz.shape[0], "furthest_point_sample_ragged")
    npoints = [int(v) for v in npoints]
    if len(npoints) != len(lengths):
        raise _lib.PuflowHipError("furthest_point_sample_ragged: one sample count per cloud")
    B = len(lengths)
    lay = fps_ragged_layout(lengths, group)
    idx = torch.zeros((max(sum(npoints), 0),), dtype=torch.int32, device=xyz.device)
    scratch = torch.empty((lay["total_floats"],), dtype=torch.float32, device=xyz.device)
    if context is None and context_lengths is None and not return_radius and radius_limit is None:
        _lib.check(lib.pf_fps_ragged(xyz.data_ptr(), _lib.counts(lengths), _lib.counts(npoints), B, int(group),
                                     scratch.data_ptr(), idx.data_ptr(), _stream()), "pf_fps_ragged")
        _check_fps_abort_ragged(scratch, lay["status_words"])
        return idx
    cl = [0] * B if context_lengths is None else [int(v) for v in context_lengths]
    if len(cl) != B or min(cl) < 0:
        raise _lib.PuflowHipError("furthest_point_sample_ragged: one context length >= 0 per cloud")
    if sum(cl) > 0:
        context = _packed(context, "furthest_point_sample_ragged (context)") if context is not None else None
        if context is None or context.shape[0] != sum(cl) or context.device != xyz.device:
            raise _lib.PuflowHipError(f"furthest_point_sample_ragged: context lengths {cl} do not describe the context tensor")
    r2 = torch.empty((B,), dtype=torch.float32, device=xyz.device)
    _lib.check(lib.pf_fps_ragged_ctx(xyz.data_ptr(), _lib.counts(lengths), _lib.counts(npoints),
                                     context.data_ptr() if sum(cl) > 0 else None, _lib.counts(cl), B, int(group),
                                     scratch.data_ptr(), idx.data_ptr(), r2.data_ptr(), _stream()), "pf_fps_ragged_ctx")
    _check_fps_abort_ragged(scratch, lay["status_words"], None if radius_limit is None else (r2, float(radius_limit)))
    return (idx, r2) if return_radius else idx


def _check_fps_abort_ragged(scratch: torch.Tensor, status_words, radius=None) -> None:
    """_check_fps_abort for a ragged pass: one status word per cloud (whichever kernel ran it), all read in ONE device -> host
    read; anything but 0 means that cloud's index row is invalid.  radius = (r2 [B], limit): the comparison r2 <= limit is made
    on the device and travels in the same read."""
    words = scratch.view(-1)[: scratch.numel() // 2 * 2].view(torch.int64)
    pos = torch.tensor(list(status_words), dtype=torch.int64).to(scratch.device, non_blocking=True)
    bad = words[pos] != 0
    if radius is not None:
        bad = torch.cat([bad, ~(radius[0] <= radius[1])])
    bad = bad.cpu()
    B = len(status_words)
    if bool(bad[:B].any()):
        which = [i for i, b in enumerate(bad[:B].tolist()) if b]
        raise _lib.PuflowHipError(f"pf_fps_ragged: clouds {which} of the pass did not complete (the cooperative kernel's workgroups "
                                  "timed out waiting for each other or were never co-resident); the sampled indices are invalid")
    if bool(bad[B:].any()):
        which = [i for i, b in enumerate(bad[B:].tolist()) if b]
        raise FpsRadiusError(which, f"pf_fps_ragged_ctx: the last sample of clouds {which} of the pass lies farther than "
                                    f"sqrt({radius[1]:g}) from every sample and context point")


class FpsRadiusError(_lib.PuflowHipError):
    """furthest_point_sample_ragged(radius_limit=...): .clouds are the clouds of the pass whose radius exceeds the limit."""

    def __init__(self, clouds, msg):
        super().__init__(msg)
        self.clouds = clouds


def box_query(pts: torch.Tensor, boxes: torch.Tensor):
    """pf_box_count / pf_box_fill: pts [M,3], boxes [T,6] (lo xyz, hi xyz; +-inf allowed, faces inside) -> (counts [T] int64 on
    the device, offsets [T+1] int64 on the device, member [sum counts] int32: per box the ascending indices of its points).
    One host read (the total) between the two passes."""
    counts = box_count(pts, boxes)
    host = counts.tolist()
    offsets, member = box_fill(pts, boxes, host)
    return counts.long(), offsets, member


def box_count(pts: torch.Tensor, boxes: torch.Tensor) -> torch.Tensor:
    """pf_box_count: int32 [T] on the device (the first pass of box_query; a caller with other values to read reads them along)"""
    lib = _lib.load()
    pts, boxes = _packed(pts, "box_count"), _f32c(boxes)
    if boxes.dim() != 2 or boxes.shape[1] != 6 or boxes.shape[0] == 0:
        raise _lib.PuflowHipError(f"box_count: boxes are [T,6], got {tuple(boxes.shape)}")
    counts = torch.empty((boxes.shape[0],), dtype=torch.int32, device=pts.device)
    _lib.check(lib.pf_box_count(pts.data_ptr(), pts.shape[0], boxes.data_ptr(), boxes.shape[0], counts.data_ptr(), _stream()),
               "pf_box_count")
    return counts


def box_fill(pts: torch.Tensor, boxes: torch.Tensor, counts):
    """pf_box_fill for the HOST counts of box_count -> (offsets int64 [T+1] on the device, member int32 [sum counts])"""
    lib = _lib.load()
    pts, boxes = _packed(pts, "box_fill"), _f32c(boxes)
    counts = [int(c) for c in counts]
    if boxes.dim() != 2 or boxes.shape[1] != 6 or boxes.shape[0] != len(counts) or min(counts) < 0:
        raise _lib.PuflowHipError(f"box_fill: one count >= 0 per box of [T,6], got {tuple(boxes.shape)} and {len(counts)} counts")
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    offsets = torch.tensor(off, dtype=torch.int64).to(pts.device)
    member = torch.empty((max(off[-1], 1),), dtype=torch.int32, device=pts.device)
    _lib.check(lib.pf_box_fill(pts.data_ptr(), pts.shape[0], boxes.data_ptr(), len(counts), offsets.data_ptr(), member.data_ptr(),
                               _stream()), "pf_box_fill")
    return offsets, member[: off[-1]]


def kd_assign(pts: torch.Tensor, axis: torch.Tensor, split: torch.Tensor, depth: int) -> torch.Tensor:
    """pf_kd_assign: the leaf (int32 [M]) of every point of pts [M,3] in the complete k-d tree of this depth, axis int32 /
    split float32 [2^depth - 1] in heap order; a point goes right iff p[axis] >= split."""
    lib = _lib.load()
    pts = _packed(pts, "kd_assign")
    depth = int(depth)
    axis = axis.to(device=pts.device, dtype=torch.int32).contiguous()
    split = split.to(device=pts.device, dtype=torch.float32).contiguous()
    if axis.numel() != (1 << depth) - 1 or split.numel() != axis.numel():
        raise _lib.PuflowHipError(f"kd_assign: a tree of depth {depth} has {(1 << depth) - 1} inner nodes")
    leaf = torch.empty((pts.shape[0],), dtype=torch.int32, device=pts.device)
    _lib.check(lib.pf_kd_assign(pts.data_ptr(), pts.shape[0], axis.data_ptr() if depth else None,
                                split.data_ptr() if depth else None, depth, leaf.data_ptr(), _stream()), "pf_kd_assign")
    return leaf


def knn_ragged(ref: torch.Tensor, ref_lengths, query: torch.Tensor, query_lengths, k: int):
    """KNN(k) per cloud of packed tensors: the query_lengths[i] queries of cloud i against its own ref_lengths[i] references
    -> (dist [sum queries, k] squared L2, idx [sum queries, k] int64 inside the cloud), ordered by (distance, index)."""
    lib = _lib.load()
    ref, query = _packed(ref, "knn_ragged"), _packed(query, "knn_ragged")
    rl = _lengths(ref_lengths, ref.shape[0], "knn_ragged")
    ql = _lengths(query_lengths, query.shape[0], "knn_ragged")
    if len(rl) != len(ql):
        raise _lib.PuflowHipError("knn_ragged: one query count per cloud")
    idx = torch.empty((query.shape[0], k), dtype=torch.int32, device=ref.device)
    dist = torch.empty((query.shape[0], k), dtype=torch.float32, device=ref.device)
    _lib.check(lib.pf_knn_large_ragged(ref.data_ptr(), query.data_ptr(), _lib.counts(rl), _lib.counts(ql), len(rl), int(k),
                                       idx.data_ptr(), dist.data_ptr(), _stream()), "pf_knn_large_ragged")
    return dist, idx.long()


def nearest_distance_ragged(x: torch.Tensor, x_lengths, y: torch.Tensor, y_lengths) -> torch.Tensor:
    """nearest_distance per cloud of packed tensors: squared distance of every point of x's cloud i to the nearest point of y's
    cloud i -> [sum x_lengths]."""
    lib = _lib.load()
    x, y = _packed(x, "nearest_distance_ragged"), _packed(y, "nearest_distance_ragged")
    xl = _lengths(x_lengths, x.shape[0], "nearest_distance_ragged")
    yl = _lengths(y_lengths, y.shape[0], "nearest_distance_ragged")
    if len(xl) != len(yl):
        raise _lib.PuflowHipError("nearest_distance_ragged: the two packed tensors hold different numbers of clouds")
    d1 = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    _lib.check(lib.pf_nn1_ragged(x.data_ptr(), y.data_ptr(), _lib.counts(xl), _lib.counts(yl), len(xl), d1.data_ptr(), None,
                                 _stream()), "pf_nn1_ragged")
    return d1


# ----------------------------------------------------------------------------------------
# Per-point attributes on the upsampled cloud (csrc/attr.hip; puflow_amd/attributes.py is the caller): the search is
# pf_knn_large / pf_knn_large_ragged in its device format (int32 indices), the kernels take exactly what it writes.
# ----------------------------------------------------------------------------------------
def knn_large(ref: torch.Tensor, query: torch.Tensor, k: int):
    """pf_knn_large: ref [B,N,3], query [B,M,3] -> (idx int32 [B,M,k], squared distances [B,M,k]), ordered by (distance, index)"""
    lib = _lib.load()
    ref, query = _f32c(ref), _f32c(query)
    if ref.dim() != 3 or query.dim() != 3 or ref.shape[2] != 3 or query.shape[2] != 3 or ref.shape[0] != query.shape[0]:
        raise _lib.PuflowHipError(f"knn_large: ref [B,N,3] and query [B,M,3], got {tuple(ref.shape)} and {tuple(query.shape)}")
    B, N, _ = ref.shape
    M = query.shape[1]
    idx = torch.empty((B, M, int(k)), dtype=torch.int32, device=ref.device)
    dist = torch.empty((B, M, int(k)), dtype=torch.float32, device=ref.device)
    _lib.check(lib.pf_knn_large(ref.data_ptr(), query.data_ptr(), B, N, M, int(k), idx.data_ptr(), dist.data_ptr(), _stream()),
               "pf_knn_large")
    return idx, dist


def knn_large_ragged(ref: torch.Tensor, ref_lengths, query: torch.Tensor, query_lengths, k: int):
    """pf_knn_large_ragged in the device format: (idx int32 [sum queries, k] inside each cloud, squared distances)"""
    lib = _lib.load()
    ref, query = _packed(ref, "knn_large_ragged"), _packed(query, "knn_large_ragged")
    rl = _lengths(ref_lengths, ref.shape[0], "knn_large_ragged")
    ql = _lengths(query_lengths, query.shape[0], "knn_large_ragged")
    if len(rl) != len(ql):
        raise _lib.PuflowHipError("knn_large_ragged: one query count per cloud")
    idx = torch.empty((query.shape[0], int(k)), dtype=torch.int32, device=ref.device)
    dist = torch.empty((query.shape[0], int(k)), dtype=torch.float32, device=ref.device)
    _lib.check(lib.pf_knn_large_ragged(ref.data_ptr(), query.data_ptr(), _lib.counts(rl), _lib.counts(ql), len(rl), int(k),
                                       idx.data_ptr(), dist.data_ptr(), _stream()), "pf_knn_large_ragged")
    return idx, dist


def _knn_grid_ws(lib, lengths, device):
    """the grid search's workspace (box, cells and cell-sorted references per cloud), rebuilt by every call"""
    nbytes = lib.pf_knn_grid_ws_bytes(_lib.counts(lengths), len(lengths))
    if nbytes < 0:
        _lib.check(int(nbytes), "pf_knn_grid_ws_bytes")
    return torch.empty((int(nbytes),), dtype=torch.uint8, device=device), int(nbytes)


def knn_grid(ref: torch.Tensor, query: torch.Tensor, k: int):
    """pf_knn_grid: what knn_large returns, bit for bit, for k <= PF_KNN_GRID_MAX_K, found over a uniform grid of the cloud
    (csrc/knn_grid.hip): ref [B,N,3], query [B,M,3] -> (idx int32 [B,M,k], squared distances [B,M,k])"""
    lib = _lib.load()
    ref, query = _f32c(ref), _f32c(query)
    if ref.dim() != 3 or query.dim() != 3 or ref.shape[2] != 3 or query.shape[2] != 3 or ref.shape[0] != query.shape[0]:
        raise _lib.PuflowHipError(f"knn_grid: ref [B,N,3] and query [B,M,3], got {tuple(ref.shape)} and {tuple(query.shape)}")
    B, N, _ = ref.shape
    M = query.shape[1]
    if B <= 0 or N <= 0:
        raise _lib.PuflowHipError(f"knn_grid: empty input {tuple(ref.shape)}")
    ws, nbytes = _knn_grid_ws(lib, [N] * B, ref.device)
    idx = torch.empty((B, M, int(k)), dtype=torch.int32, device=ref.device)
    dist = torch.empty((B, M, int(k)), dtype=torch.float32, device=ref.device)
    _lib.check(lib.pf_knn_grid(ref.data_ptr(), query.data_ptr(), B, N, M, int(k), ws.data_ptr(), nbytes, idx.data_ptr(),
                               dist.data_ptr(), _stream()), "pf_knn_grid")
    return idx, dist


def knn_grid_ragged(ref: torch.Tensor, ref_lengths, query: torch.Tensor, query_lengths, k: int):
    """pf_knn_grid_ragged: what knn_large_ragged returns, bit for bit, for k <= PF_KNN_GRID_MAX_K"""
    lib = _lib.load()
    ref, query = _packed(ref, "knn_grid_ragged"), _packed(query, "knn_grid_ragged")
    rl = _lengths(ref_lengths, ref.shape[0], "knn_grid_ragged")
    ql = _lengths(query_lengths, query.shape[0], "knn_grid_ragged")
    if len(rl) != len(ql):
        raise _lib.PuflowHipError("knn_grid_ragged: one query count per cloud")
    ws, nbytes = _knn_grid_ws(lib, rl, ref.device)
    idx = torch.empty((query.shape[0], int(k)), dtype=torch.int32, device=ref.device)
    dist = torch.empty((query.shape[0], int(k)), dtype=torch.float32, device=ref.device)
    _lib.check(lib.pf_knn_grid_ragged(ref.data_ptr(), query.data_ptr(), _lib.counts(rl), _lib.counts(ql), len(rl), int(k),
                                      ws.data_ptr(), nbytes, idx.data_ptr(), dist.data_ptr(), _stream()), "pf_knn_grid_ragged")
    return idx, dist


def _segments(segments):
    """[(kind, columns), ...] with kind a PF_ATTR_* value -> the two host arrays of the entry points and the column total"""
    segments = [(int(kind), int(cols)) for kind, cols in segments]
    return _lib.counts([s[0] for s in segments]), _lib.counts([s[1] for s in segments]), len(segments), sum(s[1] for s in segments)


def _i32c(t: torch.Tensor, what: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.PuflowHipError("puflow_amd ops need GPU tensors (no CPU fallback)")
    if t.dtype != torch.int32:
        raise _lib.PuflowHipError(f"{what}: neighbour indices are int32 (the search's device format), got {t.dtype}")
    return t.contiguous()


def attr_blend(idx: torch.Tensor, d2: torch.Tensor, attr: torch.Tensor, segments) -> torch.Tensor:
    """pf_attr_blend: idx int32 / d2 [B,M,K] from knn_large(ref = input cloud, query = output points), attr [B,N,C] the input
    points' rows, segments [(PF_ATTR_LIN | PF_ATTR_UNIT | PF_ATTR_NEAR, columns), ...] covering the C columns -> [B,M,C]"""
    lib = _lib.load()
    idx, d2, attr = _i32c(idx, "attr_blend"), _f32c(d2), _f32c(attr)
    if idx.dim() != 3 or attr.dim() != 3 or d2.shape != idx.shape or attr.shape[0] != idx.shape[0]:
        raise _lib.PuflowHipError(f"attr_blend: idx / d2 [B,M,K] and attr [B,N,C], got {tuple(idx.shape)}, {tuple(d2.shape)} and "
                                  f"{tuple(attr.shape)}")
    kind, cols, nseg, total = _segments(segments)
    B, M, K = idx.shape
    N, C = attr.shape[1], attr.shape[2]
    if total != C:
        raise _lib.PuflowHipError(f"attr_blend: the plan covers {total} columns, the attributes have {C}")
    out = torch.empty((B, M, C), dtype=torch.float32, device=attr.device)
    _lib.check(lib.pf_attr_blend(idx.data_ptr(), d2.data_ptr(), attr.data_ptr(), B, N, M, K, C, kind, cols, nseg, out.data_ptr(),
                                 _stream()), "pf_attr_blend")
    return out


def attr_blend_ragged(idx: torch.Tensor, d2: torch.Tensor, attr: torch.Tensor, lengths, out_lengths, segments) -> torch.Tensor:
    """pf_attr_blend_ragged: attr [sum lengths, C], idx int32 / d2 [sum out_lengths, K] from knn_large_ragged -> [sum
    out_lengths, C]; every cloud gets what attr_blend gives it alone"""
    lib = _lib.load()
    idx, d2, attr = _i32c(idx, "attr_blend_ragged"), _f32c(d2), _f32c(attr)
    if idx.dim() != 2 or attr.dim() != 2 or d2.shape != idx.shape:
        raise _lib.PuflowHipError(f"attr_blend_ragged: idx / d2 [sum m, K] and attr [sum n, C], got {tuple(idx.shape)}, "
                                  f"{tuple(d2.shape)} and {tuple(attr.shape)}")
    nl = _lengths(lengths, attr.shape[0], "attr_blend_ragged")
    ml = _lengths(out_lengths, idx.shape[0], "attr_blend_ragged")
    kind, cols, nseg, total = _segments(segments)
    if len(nl) != len(ml) or total != attr.shape[1]:
        raise _lib.PuflowHipError("attr_blend_ragged: one output count per cloud and a plan that covers the attribute columns")
    out = torch.empty((idx.shape[0], attr.shape[1]), dtype=torch.float32, device=attr.device)
    _lib.check(lib.pf_attr_blend_ragged(idx.data_ptr(), d2.data_ptr(), attr.data_ptr(), _lib.counts(nl), _lib.counts(ml), len(nl),
                                        idx.shape[1], attr.shape[1], kind, cols, nseg, out.data_ptr(), _stream()),
               "pf_attr_blend_ragged")
    return out


def _viewpoint(viewpoint):
    if viewpoint is None:
        return None
    import ctypes
    v = [float(x) for x in viewpoint]
    if len(v) != 3:
        raise _lib.PuflowHipError("a viewpoint is three numbers")
    return (ctypes.c_float * 3)(*v)


def normals_pca(pts: torch.Tensor, idx: torch.Tensor, viewpoint=None):
    """pf_normals_pca: pts [B,M,3], idx int32 [B,M,K] from knn_large(pts, pts, K) -> (unit normals [B,M,3], surface variation
    [B,M]).  viewpoint (three numbers): the normals look at it; None: they look away from the cloud's centroid."""
    lib = _lib.load()
    pts, idx = _f32c(pts), _i32c(idx, "normals_pca")
    if pts.dim() != 3 or pts.shape[2] != 3 or idx.dim() != 3 or idx.shape[:2] != pts.shape[:2]:
        raise _lib.PuflowHipError(f"normals_pca: pts [B,M,3] and idx [B,M,K], got {tuple(pts.shape)} and {tuple(idx.shape)}")
    B, M, K = idx.shape
    normal = torch.empty((B, M, 3), dtype=torch.float32, device=pts.device)
    var = torch.empty((B, M), dtype=torch.float32, device=pts.device)
    cen = torch.empty((B, 3), dtype=torch.float64, device=pts.device) if viewpoint is None else None
    _lib.check(lib.pf_normals_pca(pts.data_ptr(), idx.data_ptr(), B, M, K, _viewpoint(viewpoint),
                                  cen.data_ptr() if cen is not None else None, normal.data_ptr(), var.data_ptr(), _stream()),
               "pf_normals_pca")
    return normal, var


def normals_pca_ragged(pts: torch.Tensor, idx: torch.Tensor, lengths, viewpoint=None):
    """pf_normals_pca_ragged: pts [sum lengths, 3], idx int32 [sum lengths, K] from knn_large_ragged(pts, lengths, pts, lengths,
    K) -> (normals [sum lengths, 3], variation [sum lengths]); every cloud gets what normals_pca gives it alone"""
    lib = _lib.load()
    pts, idx = _packed(pts, "normals_pca_ragged"), _i32c(idx, "normals_pca_ragged")
    if idx.dim() != 2 or idx.shape[0] != pts.shape[0]:
        raise _lib.PuflowHipError(f"normals_pca_ragged: idx [sum lengths, K], got {tuple(idx.shape)}")
    ml = _lengths(lengths, pts.shape[0], "normals_pca_ragged")
    normal = torch.empty_like(pts)
    var = torch.empty((pts.shape[0],), dtype=torch.float32, device=pts.device)
    cen = torch.empty((len(ml), 3), dtype=torch.float64, device=pts.device) if viewpoint is None else None
    _lib.check(lib.pf_normals_pca_ragged(pts.data_ptr(), idx.data_ptr(), _lib.counts(ml), len(ml), idx.shape[1],
                                         _viewpoint(viewpoint), cen.data_ptr() if cen is not None else None, normal.data_ptr(),
                                         var.data_ptr(), _stream()), "pf_normals_pca_ragged")
    return normal, var


def _normals_orient_ws(lib, lengths, device):
    """the orientation's workspace (component, flip, link and offers per point), rebuilt by every call"""
    nbytes = lib.pf_normals_orient_ws_bytes(_lib.counts(lengths), len(lengths))
    if nbytes < 0:
        _lib.check(int(nbytes), "pf_normals_orient_ws_bytes")
    return torch.empty((int(nbytes),), dtype=torch.uint8, device=device), int(nbytes)


def normals_orient(pts: torch.Tensor, normals: torch.Tensor, idx: torch.Tensor, viewpoint=None, out: torch.Tensor = None):
    """pf_normals_orient: pts, normals [B,M,3] (any signs), idx int32 [B,M,K] from knn_large(pts, pts, K) -> (the normals with
    consistent signs [B,M,3], every point's component int32 [B,M]: its smallest point index).  Signs are carried along the
    minimum spanning forest of the neighbour graph; each component's seed - its highest point, or the one nearest to `viewpoint`
    (three numbers) - looks up, or at the viewpoint (csrc/normals_orient.hip).  out: where the normals go (float32, contiguous, the shape of
    `normals`; it may be `normals` itself); default: a new tensor."""
    lib = _lib.load()
    pts, normals, idx = _f32c(pts), _f32c(normals), _i32c(idx, "normals_orient")
    if pts.dim() != 3 or pts.shape[2] != 3 or normals.shape != pts.shape or idx.dim() != 3 or idx.shape[:2] != pts.shape[:2]:
        raise _lib.PuflowHipError(f"normals_orient: pts / normals [B,M,3] and idx [B,M,K], got {tuple(pts.shape)}, "
                                  f"{tuple(normals.shape)} and {tuple(idx.shape)}")
    B, M, K = idx.shape
    if B <= 0 or M <= 0:
        raise _lib.PuflowHipError(f"normals_orient: empty input {tuple(pts.shape)}")
    if out is None:
        out = torch.empty_like(normals)
    elif out.dtype != torch.float32 or out.shape != normals.shape or not out.is_contiguous() or out.device != normals.device:
        raise _lib.PuflowHipError("normals_orient: out is a contiguous float32 tensor of the normals' shape, on their device")
    ws, nbytes = _normals_orient_ws(lib, [M] * B, pts.device)
    comp = torch.empty((B, M), dtype=torch.int32, device=pts.device)
    _lib.check(lib.pf_normals_orient(pts.data_ptr(), normals.data_ptr(), idx.data_ptr(), B, M, K, _viewpoint(viewpoint),
                                     ws.data_ptr(), nbytes, out.data_ptr(), comp.data_ptr(), _stream()), "pf_normals_orient")
    return out, comp


def normals_orient_ragged(pts: torch.Tensor, normals: torch.Tensor, idx: torch.Tensor, lengths, viewpoint=None):
    """pf_normals_orient_ragged: pts, normals [sum lengths, 3], idx int32 [sum lengths, K] from knn_large_ragged -> (normals [sum
    lengths, 3], components int32 [sum lengths], indices inside the cloud); every cloud gets what normals_orient gives it alone"""
    lib = _lib.load()
    pts, normals, idx = _packed(pts, "normals_orient_ragged"), _f32c(normals), _i32c(idx, "normals_orient_ragged")
    if normals.shape != pts.shape or idx.dim() != 2 or idx.shape[0] != pts.shape[0]:
        raise _lib.PuflowHipError(f"normals_orient_ragged: normals [sum lengths, 3] and idx [sum lengths, K], got "
                                  f"{tuple(normals.shape)} and {tuple(idx.shape)}")
    ml = _lengths(lengths, pts.shape[0], "normals_orient_ragged")
    ws, nbytes = _normals_orient_ws(lib, ml, pts.device)
    out = torch.empty_like(normals)
    comp = torch.empty((pts.shape[0],), dtype=torch.int32, device=pts.device)
    _lib.check(lib.pf_normals_orient_ragged(pts.data_ptr(), normals.data_ptr(), idx.data_ptr(), _lib.counts(ml), len(ml),
                                            idx.shape[1], _viewpoint(viewpoint), ws.data_ptr(), nbytes, out.data_ptr(),
                                            comp.data_ptr(), _stream()), "pf_normals_orient_ragged")
    return out, comp


# ---- surface from an oriented cloud (csrc/recon.hip; the contract is in puflow_hip.h) -------------------------------------------
def _recon_box(tables, what: str):
    """three float32 corner tables on the device -> (contiguous tables, (D_x, D_y, D_z))"""
    tables = [_f32c(t) for t in tables]
    if len(tables) != 3 or any(t.dim() != 1 for t in tables):
        raise _lib.PuflowHipError(f"{what}: three corner tables [D_x], [D_y], [D_z]")
    return tables, tuple(int(t.shape[0]) for t in tables)


def _recon_dense(t: torch.Tensor, dims, dtype, what: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.PuflowHipError("puflow_amd ops need GPU tensors (no CPU fallback)")
    if t.dtype != dtype or tuple(t.shape) != (dims[2], dims[1], dims[0]):
        raise _lib.PuflowHipError(f"{what}: a {dtype} array [D_z, D_y, D_x] = {(dims[2], dims[1], dims[0])}, got {t.dtype} "
                                  f"{tuple(t.shape)}")
    return t.contiguous()


def _recon_dense_field(f, flags, what: str):
    """f float32 / flags uint8 [D_z, D_y, D_x] -> (f, flags, (D_x, D_y, D_z)): the dims are the flags array's"""
    if flags.dim() != 3:
        raise _lib.PuflowHipError(f"{what}: flags [D_z, D_y, D_x], got {tuple(flags.shape)}")
    dims = (int(flags.shape[2]), int(flags.shape[1]), int(flags.shape[0]))
    return _recon_dense(f, dims, torch.float32, what), _recon_dense(flags, dims, torch.uint8, what), dims


def _recon_pts(pts: torch.Tensor, what: str) -> torch.Tensor:
    pts = _f32c(pts)
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] <= 0:
        raise _lib.PuflowHipError(f"{what}: pts [N,3], got {tuple(pts.shape)}")
    return pts


def _recon_edge_ids(edge_ids: torch.Tensor, what: str) -> torch.Tensor:
    if not edge_ids.is_cuda or edge_ids.dtype != torch.int64 or edge_ids.dim() != 1 or edge_ids.shape[0] <= 0:
        raise _lib.PuflowHipError(f"{what}: edge ids int64 [V] on the GPU, got {edge_ids.dtype} {tuple(edge_ids.shape)}")
    return edge_ids.contiguous()


def recon_mark(pts: torch.Tensor, tables) -> torch.Tensor:
    """pf_recon_mark: pts [N,3], the corner tables -> uint8 flags [D_z, D_y, D_x], 1 at the 4 x 4 x 4 corners around every
    point's cell"""
    lib = _lib.load()
    pts = _recon_pts(pts, "recon_mark")
    (gx, gy, gz), (Dx, Dy, Dz) = _recon_box(tables, "recon_mark")
    flags = torch.empty((Dz, Dy, Dx), dtype=torch.uint8, device=pts.device)
    _lib.check(lib.pf_recon_mark(pts.data_ptr(), pts.shape[0], gx.data_ptr(), gy.data_ptr(), gz.data_ptr(), Dx, Dy, Dz,
                                 flags.data_ptr(), _stream()), "pf_recon_mark")
    return flags


def imls(query: torch.Tensor, pts: torch.Tensor, normals: torch.Tensor, idx: torch.Tensor, sigma_h: float) -> torch.Tensor:
    """pf_imls: query [Q,3], pts / normals [N,3], idx int32 [Q,K] from knn_grid(ref = pts, query) -> the implicit value [Q]"""
    lib = _lib.load()
    query, pts, normals, idx = _f32c(query), _f32c(pts), _f32c(normals), _i32c(idx, "imls")
    if query.dim() != 2 or query.shape[1] != 3 or pts.dim() != 2 or pts.shape[1] != 3 or normals.shape != pts.shape or \
            idx.dim() != 2 or idx.shape[0] != query.shape[0] or query.shape[0] <= 0:
        raise _lib.PuflowHipError(f"imls: query [Q,3], pts / normals [N,3] and idx [Q,K], got {tuple(query.shape)}, {tuple(pts.shape)}, "
                                  f"{tuple(normals.shape)} and {tuple(idx.shape)}")
    f = torch.empty((query.shape[0],), dtype=torch.float32, device=query.device)
    _lib.check(lib.pf_imls(query.data_ptr(), pts.data_ptr(), normals.data_ptr(), idx.data_ptr(), query.shape[0], pts.shape[0],
                           idx.shape[1], float(sigma_h), f.data_ptr(), _stream()), "pf_imls")
    return f


def recon_grow(f: torch.Tensor, flags: torch.Tensor) -> torch.Tensor:
    """pf_recon_grow: f float32 / flags uint8 [D_z, D_y, D_x] -> uint8 added [D_z, D_y, D_x], 1 at the 8 corners of every exit (an
    inactive cell that shares a face the zero set crosses with an active one)"""
    lib = _lib.load()
    f, flags, dims = _recon_dense_field(f, flags, "recon_grow")
    added = torch.empty(flags.shape, dtype=torch.uint8, device=f.device)
    _lib.check(lib.pf_recon_grow(f.data_ptr(), flags.data_ptr(), dims[0], dims[1], dims[2], added.data_ptr(), _stream()),
               "pf_recon_grow")
    return added


def mtet_count(f: torch.Tensor, flags: torch.Tensor) -> torch.Tensor:
    """pf_mtet_count: f float32 / flags uint8 [D_z, D_y, D_x] -> triangles per cell, int32 [D_z, D_y, D_x]"""
    lib = _lib.load()
    f, flags, dims = _recon_dense_field(f, flags, "mtet_count")
    count = torch.empty(flags.shape, dtype=torch.int32, device=f.device)
    _lib.check(lib.pf_mtet_count(f.data_ptr(), flags.data_ptr(), dims[0], dims[1], dims[2], count.data_ptr(), _stream()),
               "pf_mtet_count")
    return count


def mtet_emit(f: torch.Tensor, flags: torch.Tensor, first: torch.Tensor, total: int) -> torch.Tensor:
    """pf_mtet_emit: first int64 [D_z, D_y, D_x] (the exclusive prefix sum of mtet_count), total its sum -> the triangles' edge
    ids, int64 [total, 3], in the order (cell, tet, triangle)"""
    lib = _lib.load()
    f, flags, dims = _recon_dense_field(f, flags, "mtet_emit")
    first = _recon_dense(first, dims, torch.int64, "mtet_emit")
    ids = torch.empty((int(total), 3), dtype=torch.int64, device=f.device)
    _lib.check(lib.pf_mtet_emit(f.data_ptr(), flags.data_ptr(), dims[0], dims[1], dims[2], first.data_ptr(), int(total),
                                ids.data_ptr(), _stream()), "pf_mtet_emit")
    return ids


def mtet_vertices(edge_ids: torch.Tensor, f: torch.Tensor, tables) -> torch.Tensor:
    """pf_mtet_vertices: the distinct edge ids int64 [V], f [D_z, D_y, D_x], the corner tables -> float32 [V,3]"""
    lib = _lib.load()
    (gx, gy, gz), dims = _recon_box(tables, "mtet_vertices")
    f = _recon_dense(f, dims, torch.float32, "mtet_vertices")
    edge_ids = _recon_edge_ids(edge_ids, "mtet_vertices")
    verts = torch.empty((edge_ids.shape[0], 3), dtype=torch.float32, device=f.device)
    _lib.check(lib.pf_mtet_vertices(edge_ids.data_ptr(), edge_ids.shape[0], f.data_ptr(), gx.data_ptr(), gy.data_ptr(),
                                    gz.data_ptr(), dims[0], dims[1], dims[2], verts.data_ptr(), _stream()), "pf_mtet_vertices")
    return verts


# ---- the same surface in a block-sparse layout (csrc/recon_sparse.hip; the contract is in puflow_hip.h) -------------------------
RECON_BLOCK = _lib.PF_RECON_BLOCK
RECON_SLOTS = RECON_BLOCK ** 3


def _recon_dims(dims, what: str):
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3:
        raise _lib.PuflowHipError(f"{what}: dims (D_x, D_y, D_z), got {dims}")
    return dims


def _recon_list(blocks: torch.Tensor, what: str) -> torch.Tensor:
    """the ascending list of block keys, int64 [NB] on the device"""
    if not torch.is_tensor(blocks) or not blocks.is_cuda:
        raise _lib.PuflowHipError("puflow_amd ops need GPU tensors (no CPU fallback)")
    if blocks.dtype != torch.int64 or blocks.dim() != 1 or blocks.shape[0] <= 0:
        raise _lib.PuflowHipError(f"{what}: block keys int64 [NB], got {blocks.dtype} {tuple(blocks.shape)}")
    return blocks.contiguous()


def _recon_block(t: torch.Tensor, nb: int, width: int, dtype, what: str) -> torch.Tensor:
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.PuflowHipError("puflow_amd ops need GPU tensors (no CPU fallback)")
    if t.dtype != dtype or tuple(t.shape) != (nb, width):
        raise _lib.PuflowHipError(f"{what}: a {dtype} block array [NB, {width}] = {(nb, width)}, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def recon_block_keys(pts: torch.Tensor, tables) -> torch.Tensor:
    """pf_recon_block_keys: pts [N,3], the corner tables -> int64 [N, 8], the keys of the blocks every point's 4 x 4 x 4 corners
    touch; torch.unique of it is the block list"""
    lib = _lib.load()
    pts = _recon_pts(pts, "recon_block_keys")
    (gx, gy, gz), (Dx, Dy, Dz) = _recon_box(tables, "recon_block_keys")
    keys = torch.empty((pts.shape[0], 8), dtype=torch.int64, device=pts.device)
    _lib.check(lib.pf_recon_block_keys(pts.data_ptr(), pts.shape[0], gx.data_ptr(), gy.data_ptr(), gz.data_ptr(), Dx, Dy, Dz,
                                       keys.data_ptr(), _stream()), "pf_recon_block_keys")
    return keys


def recon_block_links(blocks: torch.Tensor, dims) -> torch.Tensor:
    """pf_recon_block_links: the block list, (D_x, D_y, D_z) -> int32 [NB, 8], the list positions of the blocks at offsets {0,1}^3
    (-1: absent)"""
    lib = _lib.load()
    blocks, (Dx, Dy, Dz) = _recon_list(blocks, "recon_block_links"), _recon_dims(dims, "recon_block_links")
    links = torch.empty((blocks.shape[0], 8), dtype=torch.int32, device=blocks.device)
    _lib.check(lib.pf_recon_block_links(blocks.data_ptr(), blocks.shape[0], Dx, Dy, Dz, links.data_ptr(), _stream()),
               "pf_recon_block_links")
    return links


def recon_mark_sparse(pts: torch.Tensor, tables, blocks: torch.Tensor) -> torch.Tensor:
    """pf_recon_mark_sparse: pts [N,3], the corner tables, the block list -> uint8 flags [NB, 512]"""
    lib = _lib.load()
    pts = _recon_pts(pts, "recon_mark_sparse")
    (gx, gy, gz), (Dx, Dy, Dz) = _recon_box(tables, "recon_mark_sparse")
    blocks = _recon_list(blocks, "recon_mark_sparse")
    flags = torch.empty((blocks.shape[0], RECON_SLOTS), dtype=torch.uint8, device=pts.device)
    _lib.check(lib.pf_recon_mark_sparse(pts.data_ptr(), pts.shape[0], gx.data_ptr(), gy.data_ptr(), gz.data_ptr(), Dx, Dy, Dz,
                                        blocks.data_ptr(), blocks.shape[0], flags.data_ptr(), _stream()), "pf_recon_mark_sparse")
    return flags


def _recon_sparse_field(f, flags, blocks, links, dims, what: str):
    blocks, dims = _recon_list(blocks, what), _recon_dims(dims, what)
    nb = int(blocks.shape[0])
    return (_recon_block(f, nb, RECON_SLOTS, torch.float32, what), _recon_block(flags, nb, RECON_SLOTS, torch.uint8, what), blocks,
            _recon_block(links, nb, 8, torch.int32, what), nb, dims)


def mtet_count_sparse(f: torch.Tensor, flags: torch.Tensor, blocks: torch.Tensor, links: torch.Tensor, dims) -> torch.Tensor:
    """pf_mtet_count_sparse: f float32 / flags uint8 [NB, 512], the block list and its links -> triangles per slot (the cell whose
    lower corner it is), int32 [NB, 512]"""
    lib = _lib.load()
    f, flags, blocks, links, nb, (Dx, Dy, Dz) = _recon_sparse_field(f, flags, blocks, links, dims, "mtet_count_sparse")
    count = torch.empty((nb, RECON_SLOTS), dtype=torch.int32, device=f.device)
    _lib.check(lib.pf_mtet_count_sparse(f.data_ptr(), flags.data_ptr(), blocks.data_ptr(), links.data_ptr(), nb, Dx, Dy, Dz,
                                        count.data_ptr(), _stream()), "pf_mtet_count_sparse")
    return count


def mtet_emit_sparse(f: torch.Tensor, flags: torch.Tensor, blocks: torch.Tensor, links: torch.Tensor, dims, cells: torch.Tensor,
                     first: torch.Tensor, total: int) -> torch.Tensor:
    """pf_mtet_emit_sparse: cells int64 [M], the slot numbers with triangles sorted by global cell index; first int64 [M], the
    exclusive prefix sum of their counts; total its sum -> the triangles' edge ids, int64 [total, 3]"""
    lib = _lib.load()
    f, flags, blocks, links, nb, (Dx, Dy, Dz) = _recon_sparse_field(f, flags, blocks, links, dims, "mtet_emit_sparse")
    for t, name in ((cells, "cells"), (first, "first")):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.int64 or t.dim() != 1 or t.shape != cells.shape or t.shape[0] <= 0:
            raise _lib.PuflowHipError(f"mtet_emit_sparse: {name} int64 [M] on the GPU, got {getattr(t, 'dtype', type(t))} "
                                      f"{tuple(getattr(t, 'shape', ()))}")
    cells, first = cells.contiguous(), first.contiguous()
    ids = torch.empty((int(total), 3), dtype=torch.int64, device=f.device)
    _lib.check(lib.pf_mtet_emit_sparse(f.data_ptr(), flags.data_ptr(), blocks.data_ptr(), links.data_ptr(), nb, Dx, Dy, Dz,
                                       cells.data_ptr(), first.data_ptr(), cells.shape[0], int(total), ids.data_ptr(), _stream()),
               "pf_mtet_emit_sparse")
    return ids


def mtet_vertices_sparse(edge_ids: torch.Tensor, f: torch.Tensor, blocks: torch.Tensor, links: torch.Tensor, tables) -> torch.Tensor:
    """pf_mtet_vertices_sparse: the distinct edge ids int64 [V], f [NB, 512], the block list and its links, the corner tables ->
    float32 [V,3]"""
    lib = _lib.load()
    (gx, gy, gz), dims = _recon_box(tables, "mtet_vertices_sparse")
    blocks = _recon_list(blocks, "mtet_vertices_sparse")
    nb = int(blocks.shape[0])
    f = _recon_block(f, nb, RECON_SLOTS, torch.float32, "mtet_vertices_sparse")
    links = _recon_block(links, nb, 8, torch.int32, "mtet_vertices_sparse")
    edge_ids = _recon_edge_ids(edge_ids, "mtet_vertices_sparse")
    verts = torch.empty((edge_ids.shape[0], 3), dtype=torch.float32, device=f.device)
    _lib.check(lib.pf_mtet_vertices_sparse(edge_ids.data_ptr(), edge_ids.shape[0], f.data_ptr(), blocks.data_ptr(), links.data_ptr(), nb,
                                           gx.data_ptr(), gy.data_ptr(), gz.data_ptr(), dims[0], dims[1], dims[2], verts.data_ptr(),
                                           _stream()), "pf_mtet_vertices_sparse")
    return verts
