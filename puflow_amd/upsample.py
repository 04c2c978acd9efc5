"""Inference CLI - same flags, defaults, file handling and output format as the reference's
`modules/discrete/upsample.py:20-86`:

  python -m puflow_amd.upsample --source=path/to/input --target=path/to/output --checkpoint=ckpt.pt --up_ratio=4
"""
from __future__ import annotations

import os
from argparse import ArgumentParser
from pathlib import Path
from typing import List

import numpy as np
import torch

from .interpflow import PointInterpFlow
from .patch import PatchHelper


def shard_paths(paths: List[str], rank: int, world: int) -> List[str]:
    """Files of rank `rank` out of `world`: sorted, then strided (balanced for any count)."""
    return sorted(paths)[rank::world] if world > 1 else list(paths)


def pass_is_full(count: int, points: int, next_points: int, cloud_batch: int, pass_points=None) -> bool:
    """Must a pass that holds `count` files / `points` input points be flushed before a file of `next_points` joins it?"""
    if count == 0:
        return False                                     # a file larger than pass_points is a pass of its own
    return count >= max(int(cloud_batch), 1) or (pass_points is not None and points + next_points > int(pass_points))


def plan_passes(sizes, cloud_batch: int, pass_points=None):
    """How the CLI groups consecutive files into passes: [(first, last + 1), ...] over the files in order.  A pass takes up to
    `cloud_batch` files whatever their point counts and, with `pass_points`, at most that many input points (a single larger
    file is a pass of its own).  The CLI's loop applies the same rule (pass_is_full) file by file."""
    passes, first, points = [], 0, 0
    for i, n in enumerate(sizes):
        if pass_is_full(i - first, points, int(n), cloud_batch, pass_points):
            passes.append((first, i))
            first, points = i, 0
        points += int(n)
    if len(sizes) > first:
        passes.append((first, len(sizes)))
    return passes


def save_xyz(path, points: np.ndarray) -> None:
    """`np.savetxt(path, points, fmt="%.6f")` (upsample.py:57) - the same bytes - formatted by the library's host-side
    `pf_format_xyz` (~1 ms for a 20 000-point cloud instead of 36 ms; the call releases the GIL, so the writer thread really
    runs beside the GPU work).  With the GPU part batched, writing was what the CLI waited for."""
    points = np.atleast_2d(np.asarray(points))
    if points.dtype != np.float32:                       # the library formats float32 values; anything else: one format call
        line = " ".join(["%.6f"] * points.shape[1]) + "\n"
        with open(path, "w") as f:
            f.write((line * points.shape[0]) % tuple(points.ravel().tolist()))
        return
    import ctypes
    from . import _lib
    lib = _lib.load()
    pts = np.ascontiguousarray(points)
    n, c = pts.shape
    cap = lib.pf_format_xyz_bound(n, c)
    buf = ctypes.create_string_buffer(cap)
    m = lib.pf_format_xyz(pts.ctypes.data, n, c, ctypes.addressof(buf), cap)
    if m < 0:
        _lib.check(int(m), "pf_format_xyz")
    with open(path, "wb") as f:
        f.write(memoryview(buf)[:m])


def load_xyz(path) -> np.ndarray:
    """`np.loadtxt(path, dtype=np.float32)` (upsample.py:42) through the library's host-side parser (`pf_parse_xyz`: the same
    values, ~0.3 ms instead of 2-3 ms per 5000-point file); anything the parser does not take (a token that is not a plain
    number, other delimiters) goes to numpy."""
    import ctypes
    from . import _lib
    with open(path, "rb") as f:
        raw = f.read()
    lib = _lib.load()
    buf = ctypes.create_string_buffer(raw, len(raw) + 1)          # + terminating 0
    cap = len(raw) // 2 + 1                                       # a value takes at least one character and a separator
    out = np.empty(cap, dtype=np.float32)
    ncols = ctypes.c_int(0)
    n = lib.pf_parse_xyz(ctypes.addressof(buf), len(raw), out.ctypes.data, cap, ctypes.byref(ncols))
    if n <= 0 or ncols.value <= 0:
        return np.loadtxt(path, dtype=np.float32)                 # unusual file: numpy decides (and raises its own errors)
    arr = out[:n].reshape(-1, ncols.value)
    return arr[0].copy() if arr.shape[0] == 1 else (arr[:, 0].copy() if ncols.value == 1 else arr.copy())


@torch.no_grad()
def upsampling(data_paths: List[str], target_path: str, checkpoint_path: str, up_ratio: int, num_outlier: int,
               num_patch: int, num_upsampling: int = None, seed=None, state_dict=None, network_cls=PointInterpFlow,
               cloud_batch: int = None, pass_points: int = None, network_setup=None, tile_points: int = None,
               attributes: str = None, attr_k: int = 8, estimate_normals: int = None, normals_viewpoint=None,
               attr_search: str = "brute", normals_orient: str = "point"):
    # normals_orient: the sign of the estimated normals - "point": every point on its own (towards the viewpoint, or away from the
    # centroid); "propagate": carried along the minimum spanning forest of the neighbour graph (attributes.orient_normals)
    # attr_search: the neighbour search behind the two options below - "brute" (pf_knn_large) or "grid" (pf_knn_grid, a uniform
    # grid of the cloud); the same neighbours bit for bit, hence the same files
    # attributes / attr_k / estimate_normals / normals_viewpoint (not in the reference; puflow_amd/attributes.py): the
    # files' columns after x y z are carried to the output points as the plan says, and / or a PCA normal is appended to every
    # output row.  All None: bare xyz in, bare xyz out, as the reference.
    # tile_points (not in the reference): a file with more points than this is upsampled in k-d tiles of about that many points
    # (PatchHelper.upsample_tiled), as a pass of its own; None = off, every file takes the passes below
    # network_setup(network): called once on the loaded eval-mode network before the first pass (upsample_cnf's schedule options)
    # The continuous model integrates all patches of a pass with ONE adaptive step sequence (the error norm is taken over the
    # whole batch, cnf.py:97-113), so a cloud's result depends on what shares its pass: it keeps the reference's one file at a
    # time unless asked otherwise.  The discrete model's patches never interact.
    if cloud_batch is None:
        cloud_batch = 16 if network_cls is PointInterpFlow else 1
    # The host side of this loop is a 5000-element permutation and two small copies per file: ONE intra-op thread.  torch's
    # default is one thread per visible CPU (128 on the MI355X boxes, whose containers own 16 CPUs' worth of quota): every tiny
    # CPU op then wakes a pool of spinning OpenMP threads, the cgroup's CPU quota is gone within a few ms of each 100 ms period
    # and the WHOLE process - the thread waiting for the GPU included - is throttled for the rest of it: a third of the clouds took
    # 70 ms instead of 11 (tools/fps_interplay_probe.py shuffle [1]; round 5).
    host_threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _upsampling(data_paths, target_path, checkpoint_path, up_ratio, num_outlier, num_patch, num_upsampling, seed,
                           state_dict, network_cls, cloud_batch, pass_points, network_setup, tile_points, attributes, attr_k,
                           estimate_normals, normals_viewpoint, attr_search, normals_orient)
    finally:
        torch.set_num_threads(host_threads)


def _upsampling(data_paths, target_path, checkpoint_path, up_ratio, num_outlier, num_patch, num_upsampling, seed, state_dict,
                network_cls, cloud_batch, pass_points=None, network_setup=None, tile_points=None, attributes=None, attr_k=8,
                estimate_normals=None, normals_viewpoint=None, attr_search="brute", normals_orient="point"):
    from . import attributes as A
    if normals_orient not in A.ORIENTS:
        raise SystemExit(f"--normals_orient: one of {', '.join(A.ORIENTS)}, got {normals_orient!r}")
    if normals_orient != "point" and estimate_normals is None:
        raise SystemExit("--normals_orient goes with --estimate_normals")
    if attr_search not in A.SEARCHES:
        raise SystemExit(f"--attr_search: one of {', '.join(A.SEARCHES)}, got {attr_search!r}")
    plan = None
    try:
        if attributes is not None:
            plan = A.parse_plan(attributes)
    except ValueError as e:
        raise SystemExit(f"--attributes: {e}")
    if estimate_normals is not None and plan is not None and A.has_normal(plan):
        raise SystemExit("--estimate_normals: the --attributes plan already carries the files' normals (`normal`); "
                         "drop one of the two")
    if plan is not None and not 1 <= int(attr_k) <= A.MAX_K:
        raise SystemExit(f"--attr_k: 1 .. {A.MAX_K} input points are blended per output point, got {attr_k}")
    if estimate_normals is not None and not A.NORMALS_MIN_K <= int(estimate_normals) <= A.NORMALS_MAX_K:
        raise SystemExit(f"--estimate_normals: a neighbourhood of {A.NORMALS_MIN_K} .. {A.NORMALS_MAX_K} points, got {estimate_normals}")
    if isinstance(normals_viewpoint, str):
        try:
            normals_viewpoint = [float(v) for v in normals_viewpoint.split(",")]
        except ValueError:
            normals_viewpoint = []
    if normals_viewpoint is not None and (estimate_normals is None or len(normals_viewpoint) != 3):
        raise SystemExit("--normals_viewpoint takes x,y,z and goes with --estimate_normals")
    if seed is not None:
        np.random.seed(seed)
        torch.random.manual_seed(seed)
        torch.cuda.manual_seed(seed)
    # One process per GPU (torchrun): every rank upsamples its own files - clouds are independent, so the CLI shards
    # by file with no collective at all (BASELINE configs[3]); a plain `python -m puflow_amd.upsample` is rank 0 of 1.
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    # The per-file shuffle is drawn from the process RNG in file order (upsample.py:43), so a file's result depends on the
    # files before it.  Under sharding every rank therefore walks the WHOLE sorted list and draws (and discards) the shuffles
    # of the other ranks' files: each file gets exactly the result of a one-process run, whatever the number of ranks.  The
    # list is sorted in every case (the reference takes os.walk's order, which depends on the file system: its outputs are
    # reproducible only on one machine).
    all_paths = sorted(data_paths)
    mine = set(shard_paths(data_paths, rank, world))
    device = torch.device(f"cuda:{int(os.environ.get('LOCAL_RANK', '0')) % max(torch.cuda.device_count(), 1)}")
    network = network_cls(3)
    network.load_state_dict(state_dict if state_dict is not None else torch.load(checkpoint_path, map_location="cpu"))
    network.set_to_initialized_state()
    network = network.to(device).eval()
    if network_setup is not None:
        network_setup(network)
    patch_helper = PatchHelper(num_patch, patch_expand_ratio=4)
    # The reference takes one file at a time (upsample.py:42-57).  Here up to `cloud_batch` consecutive files go through the
    # pipeline together, whatever their point counts: the FPS merge, which is sequential in its 4N output points and 95 % of a
    # cloud's GPU time, then runs for all of them at once (16 clouds take the time of 1.35).  Files of one size (or a single file)
    # take the dense [B, N, 3] path, mixed sizes the ragged one (PatchHelper.upsample_ragged: the clouds stored back to back).
    # Either way every cloud's result is the one it gets alone (clouds never interact; the per-file shuffles are drawn in file
    # order as before), and finished clouds are written by a worker thread while the GPU works on the next pass.
    from concurrent.futures import ThreadPoolExecutor
    writes = []
    pending = []                                                   # (file name, shuffled cloud [1,N,3] on the host, its
                                                                   # attribute rows [1,N,C] in the same order or None)

    # The extra columns of the output rows, on the final (de-normalised, outlier-free) points: the input's attribute rows blended
    # from every output point's attr_k nearest input points, then the estimated normals.  One search and one kernel launch each
    # per pass; a cloud's columns are the ones it gets alone.  Without the options: the points as they are.
    def with_columns(pred, cloud, attr):                           # a dense pass: [B,M,3], [B,N,3], [B,N,C] or None
        cols = [pred]
        if plan is not None:
            cols.append(A.transfer(pred, cloud, attr, plan, attr_k, search=attr_search))
        if estimate_normals is not None:
            cols.append(A.estimate_normals(pred, estimate_normals, normals_viewpoint, search=attr_search, orient=normals_orient)[0])
        return torch.cat(cols, dim=-1) if len(cols) > 1 else pred

    def with_columns_ragged(pred, clouds, attrs):                  # a ragged pass: lists of [M_i,3], [N_i,3], [N_i,C]
        cols = [pred]
        if plan is not None:
            cols.append(A.transfer_ragged(pred, clouds, attrs, plan, attr_k, search=attr_search))
        if estimate_normals is not None:
            cols.append(A.estimate_normals_ragged(pred, estimate_normals, normals_viewpoint, search=attr_search,
                                                  orient=normals_orient)[0])
        return [torch.cat(c, dim=-1) for c in zip(*cols)] if len(cols) > 1 else pred

    def npoint_of(n):
        return (n * up_ratio if num_upsampling is None else num_upsampling) + (num_outlier or 0)

    def flush(pool):
        if not pending:
            return
        sizes = [c.shape[1] for _, c, _ in pending]
        if len(set(sizes)) == 1:
            pt_input = torch.cat([c for _, c, _ in pending], dim=0).to(device)
            pred = patch_helper.upsample(network, pt_input, npoint=npoint_of(sizes[0]), upratio=up_ratio, jitter=False)
            if num_outlier is not None and num_outlier > 0:
                pred = PatchHelper.remove_outliers(pred, pt_input, num_outlier)
            pred = with_columns(pred, pt_input, torch.cat([a for _, _, a in pending], dim=0).to(device) if plan is not None else None)
            pred = list(pred.cpu().numpy())
        else:
            clouds = list(torch.split(torch.cat([c[0] for _, c, _ in pending], dim=0).to(device), sizes))
            pred = patch_helper.upsample_ragged(network, clouds, [npoint_of(n) for n in sizes], upratio=up_ratio,
                                                names=[name for name, _, _ in pending])
            if num_outlier is not None and num_outlier > 0:
                pred = PatchHelper.remove_outliers_ragged(pred, clouds, num_outlier)
            pred = with_columns_ragged(pred, clouds, list(torch.split(torch.cat([a[0] for _, _, a in pending], dim=0).to(device), sizes))
                                       if plan is not None else None)
            pred = [p.numpy() for p in torch.split(torch.cat(pred, dim=0).cpu(), [p.shape[0] for p in pred])]
        for (file_name, _, _), cloud in zip(pending, pred):
            writes.append(pool.submit(save_xyz, Path(target_path) / file_name, cloud))
        pending.clear()

    with ThreadPoolExecutor(max_workers=1) as pool:
        for path in all_paths:
            _, file_name = os.path.split(path)
            pt_input = torch.from_numpy(load_xyz(path)).unsqueeze(0)
            perm = torch.randperm(pt_input.shape[1])
            if path not in mine:
                continue                                            # another rank's file: only the RNG draw is replayed
            pt_input = pt_input[:, perm].contiguous()
            attr = None
            if plan is not None:                                    # columns 4 ...: beside the cloud, in the cloud's order
                try:
                    A.parse_plan(attributes, columns=pt_input.shape[-1] if pt_input.dim() == 3 else 0)
                except ValueError as e:
                    raise SystemExit(f"{path}: --attributes: {e}")
                pt_input, attr = pt_input[..., :3].contiguous(), pt_input[..., 3:].contiguous()
            elif pt_input.dim() == 3 and pt_input.shape[-1] > 3:
                raise SystemExit(f"{path}: {pt_input.shape[-1]} columns; the network takes x y z - name the others with "
                                 f"--attributes (for instance --attributes lin{pt_input.shape[-1] - 3})")
            if tile_points is not None and pt_input.shape[1] > int(tile_points):
                flush(pool)                                         # a pass of its own, in file order
                cloud = pt_input.to(device)
                pred = patch_helper.upsample_tiled(network, cloud[0], npoint_of(cloud.shape[1]), upratio=up_ratio,
                                                   tile_points=int(tile_points))[None]
                if num_outlier is not None and num_outlier > 0:
                    pred = PatchHelper.remove_outliers(pred, cloud, num_outlier)
                pred = with_columns(pred, cloud, attr.to(device) if attr is not None else None)      # against the whole input cloud
                writes.append(pool.submit(save_xyz, Path(target_path) / file_name, pred[0].cpu().numpy()))
                continue
            if pass_is_full(len(pending), sum(c.shape[1] for _, c, _ in pending), pt_input.shape[1], cloud_batch, pass_points):
                flush(pool)
            pending.append((file_name, pt_input, attr))
        flush(pool)
        for w in writes:
            w.result()                                             # re-raises a failed write


def main(argv=None, network_cls=PointInterpFlow, add_arguments=None, network_setup=None):
    """add_arguments(parser), network_setup(network, args): a model's own options (upsample_cnf)."""
    parser = ArgumentParser()
    parser.add_argument("--source", type=str, help="Path of input directory")
    parser.add_argument("--target", type=str, help="Path of output directory")
    parser.add_argument("--seed", type=int, default=2021)
    parser.add_argument("--checkpoint", type=str, help="Path of checkpoint")
    parser.add_argument("--up_ratio", type=int, help="upsampling ratio", default=4)
    parser.add_argument("--num_patch", type=int, help="number of point in each patch", default=256)
    parser.add_argument("--num_out", type=int, default=None, help="number of point of output point cloud")
    parser.add_argument("--cloud_batch", type=int, default=None,
                        help="(not in the reference) consecutive files, of any point counts, that share one pass; 1 = one file at a "
                             "time (default: 16 for the discrete model, 1 for the continuous one)")
    parser.add_argument("--pass_points", type=int, default=None,
                        help="(not in the reference) a pass is also closed before its input points would exceed this "
                             "(default: no limit); a larger file is a pass of its own")
    parser.add_argument("--tile_points", type=int, default=None,
                        help="(not in the reference) a file with more points than this is upsampled in k-d tiles of about this many "
                             "points, merged by FPS with a fixed context, as a pass of its own (default: off)")
    parser.add_argument("--attributes", type=str, default=None, metavar="PLAN",
                        help="(not in the reference) carry the files' columns after x y z to the output points: PLAN names them in "
                             "order, e.g. normal,lin3,near1 = a normal (3 columns, sign-aligned, blended, normalised), 3 columns "
                             "blended by inverse squared distance, 1 column copied from the nearest input point (labels); at most "
                             "16 columns (default: files hold x y z only)")
    parser.add_argument("--attr_k", type=int, default=8, help="(not in the reference) input points blended per output point, 1..8")
    parser.add_argument("--estimate_normals", type=int, default=None, metavar="K",
                        help="(not in the reference) append nx ny nz to every output row: the PCA normal of the output point's K "
                             "nearest output points (8..64), pointing away from the cloud's centroid (default: off)")
    parser.add_argument("--normals_viewpoint", type=str, default=None, metavar="X,Y,Z",
                        help="(not in the reference) estimated normals point towards this position instead")
    parser.add_argument("--attr_search", type=str, default=None, choices=("brute", "grid"),
                        help="(not in the reference) the neighbour search behind --attributes and --estimate_normals: brute = one "
                             "workgroup sorts the whole cloud per output point, grid = a uniform grid of the cloud, far faster on "
                             "large clouds; the same files either way (default: brute)")
    parser.add_argument("--normals_orient", type=str, default=None, choices=("point", "propagate"),
                        help="(not in the reference) the sign of the --estimate_normals columns: point = every point on its own, "
                             "away from the centroid or towards --normals_viewpoint; propagate = carried along a minimum spanning "
                             "tree of the neighbour graph from each piece's highest point (or the one nearest to the viewpoint), "
                             "consistent in cavities and on inner walls too (default: point)")
    if add_arguments is not None:
        add_arguments(parser)
    args = parser.parse_args(argv)
    if args.normals_orient is not None and args.estimate_normals is None:
        raise SystemExit("--normals_orient goes with --estimate_normals")
    if args.attr_search is not None and args.attributes is None and args.estimate_normals is None:
        raise SystemExit("--attr_search goes with --attributes or --estimate_normals")
    os.makedirs(args.target, exist_ok=True)            # exist_ok: several ranks may race to create it
    data_paths = []
    for root, _dirs, files in os.walk(args.source):
        data_paths.extend([os.path.join(root, f) for f in files if ".xyz" in f])
    upsampling(data_paths, args.target, args.checkpoint, up_ratio=args.up_ratio, num_outlier=24, num_patch=args.num_patch,
               num_upsampling=args.num_out, seed=args.seed, network_cls=network_cls, cloud_batch=args.cloud_batch,
               pass_points=args.pass_points, tile_points=args.tile_points, attributes=args.attributes, attr_k=args.attr_k,
               estimate_normals=args.estimate_normals, normals_viewpoint=args.normals_viewpoint,
               attr_search=args.attr_search or "brute", normals_orient=args.normals_orient or "point",
               network_setup=(lambda net: network_setup(net, args)) if network_setup is not None else None)


if __name__ == "__main__":
    main()
