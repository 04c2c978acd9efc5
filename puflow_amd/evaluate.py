"""Evaluation CLI - the reference's scoring step (evaluation/evaluate.py, with the CGAL binary evaluation/evaluation for the
point-to-surface column) on the GPU:

  python -m puflow_amd.evaluate --pred DIR --gt DIR --save_path DIR [--mesh DIR] [--write_p2m] [--cloud_batch N]
                                [--emd_levels_top 7] [--uniform [--uniform_seeds 1000] [--uniform_seed 0] [--write_disks]
                                                       [--uniform_disks ball|surface]]

Every `<name>.xyz` of --pred with a `<name>.xyz` in --gt is scored (evaluate.py:187-195): CD, EMD (approx-match), Hausdorff
and JSD (puflow_amd.metrics).  P2F, the point-to-surface distance of the predicted points: with --mesh it is computed from
`<mesh>/<name>.off`, and --write_p2m also writes `<pred>_point2mesh_distance.xyz` in the CGAL binary's format (`x y z d`, C++
default stream formatting, the coordinates formatted from the double values of the file's own tokens, as the binary parses
them); without --mesh an existing `<pred>_point2mesh_distance.xyz` (the binary's output) is read, as evaluate.py:247-251 does.
`<save_path>/evaluation.csv` gets the reference's header, one row per file and one summary row, and the summary line is printed
as evaluate.py:294-298 prints it.

Uniformity (uniform_0..4, evaluate.py:105-165 analyze_uniform) is filled with --uniform only; without it the columns read `-`.
With --mesh the disks are made on the GPU: --uniform_seeds seeds on the surface (Philox, --uniform_seed), the predicted points
mapped to their closest mesh points, and around every seed the mapped points within r_j = sqrt(p_j A / pi), p = 0.4 .. 1.2 % of
the area A; --write_disks also writes `<pred>_disk_idx.txt`, `<pred>_radius.txt` and `<pred>_point2mesh_distance.txt`, the
three files the reference reads.  Without --mesh those three files are read, whoever wrote them, as evaluate.py:256-262 does.
--uniform_disks ball (the default): disks made from a mesh are Euclidean balls (the pre-filter of evaluation.cpp:97-100,
without its geodesic refinement); on parts thinner than the radius a ball also takes in points of the opposite side.
--uniform_disks surface: a ball's member stays only when its face is connected to the seed's face along the surface inside a
ball no larger than the disk's (metrics.surface_reach, r_stop = the largest radius; the seeds' faces from the sampler, the
points' faces from the P2F search).  This restriction is the project's own: it is not a geodesic length, and its parity with
the reference's CGAL geodesic disks is unpinned - the reference's binary never writes them.  --write_disks writes whichever
disks were made.

The reference's quirks, kept or fixed:
  - kept: a file's JSD appears in its row only when it has a P2F (evaluate.py:255), for CSV compatibility; the summary JSD
    is over all files;
  - kept: P2F per file is nanmean / nanstd (population) of its points, the summary P2F is over all points of all files;
  - fixed: `load` is undefined in evaluate.py:94,220,248 - read here as np.loadtxt float32 (upsample.load_xyz for clouds);
  - fixed: the summary print raises KeyError when no file has a P2F - `-` is printed instead;
  - fixed: rows follow `glob`'s order there - sorted by name here;
  - kept: uniformity appears in a row only when the file has a P2F (evaluate.py:255-256); the summary is the mean over the
    files that have it (evaluate.py:283-287).
"""
from __future__ import annotations

import csv
import os
from argparse import ArgumentParser
from collections import OrderedDict
from glob import glob

import numpy as np
import torch

from . import metrics
from ._host import limit_host_threads
from .upsample import load_xyz

PERCENTAGES = 5                       # uniform_0 .. uniform_4 (evaluate.py:105)
FIELDNAMES = ["name", "CD", "EMD", "hausdorff", "p2f avg", "p2f std", "JSD"] + ["uniform_%d" % d for d in range(PERCENTAGES)]
SUMMARY_KEYS = ["CD", "EMD", "hausdorff", "p2f avg", "p2f std", "JSD"]


def pair_paths(pred_dir: str, gt_dir: str):
    """[(name, gt path, pred path)] of the .xyz files present in both directories, sorted by name."""
    gt = {os.path.basename(p)[:-4]: p for p in glob(os.path.join(gt_dir, "*.xyz"))}
    out = []
    for p in glob(os.path.join(pred_dir, "*.xyz")):
        name = os.path.basename(p)[:-4]
        if name in gt:
            out.append((name, gt[name], p))
    return sorted(out)


def format_p2m(xyz_tokens: np.ndarray, dist: np.ndarray) -> str:
    """The CGAL binary's `x y z d` lines: C++ default stream formatting (%g, 6 significant digits)."""
    return "".join("%g %g %g %g\n" % (x, y, z, float(d)) for (x, y, z), d in zip(xyz_tokens.tolist(), dist.tolist()))


def _batches(items, key, size):
    """Runs of up to `size` consecutive items with the same key."""
    run = []
    for it in items:
        if run and (key(it) != key(run[0]) or len(run) == size):
            yield run
            run = []
        run.append(it)
    if run:
        yield run


def evaluate(pred_dir: str, gt_dir: str, save_path: str, mesh_dir: str = None, write_p2m: bool = False,
             cloud_batch: int = 16, emd_levels_top: int = 7, device=None, uniform: bool = False, uniform_seeds: int = 1000,
             uniform_seed: int = 0, write_disks: bool = False, uniform_disks: str = "ball", p2f_search: str = "tiles"):
    """Score the directory; returns (per-file rows, summary row) as written to evaluation.csv.  p2f_search: the closest-triangle
    search of P2F, "tiles" or "grid" (metrics.point_to_mesh_distance) - the same numbers and files either way."""
    if p2f_search not in metrics.P2F_SEARCHES:
        raise ValueError(f"p2f_search is one of {metrics.P2F_SEARCHES}, got {p2f_search!r}")
    if uniform_disks not in ("ball", "surface"):
        raise ValueError(f"uniform_disks is 'ball' or 'surface', got {uniform_disks!r}")
    uni = dict(seeds=int(uniform_seeds), seed=int(uniform_seed), write=bool(write_disks),
               surface=uniform_disks == "surface") if uniform else None
    device = torch.device(device or "cuda:0")
    pairs = pair_paths(pred_dir, gt_dir)
    if not pairs:
        raise FileNotFoundError(f"no <name>.xyz is in both {pred_dir} and {gt_dir}")
    loaded = [(name, gp, pp, np.atleast_2d(load_xyz(pp))[:, :3], np.atleast_2d(load_xyz(gp))[:, :3]) for name, gp, pp in pairs]
    rows, g_cd, g_emd, g_hd, g_jsd, g_p2f, g_uni = [], [], [], [], [], [], []
    for run in _batches(loaded, lambda it: (it[3].shape[0], it[4].shape[0]), max(1, int(cloud_batch))):
        pred = torch.from_numpy(np.stack([it[3] for it in run])).to(device)
        gt = torch.from_numpy(np.stack([it[4] for it in run])).to(device)
        cd, hd = metrics.chamfer_hausdorff(pred, gt)
        pn, _, _ = metrics.normalize_point_cloud(pred)
        gn, _, _ = metrics.normalize_point_cloud(gt)
        emd = metrics.approx_match_emd(pn, gn, emd_levels_top)
        jsd = metrics.jsd(pred, gt)
        cd, hd, emd = cd.cpu().numpy(), hd.cpu().numpy(), emd.cpu().numpy()
        for i, (name, gp, pp, pred_np, _) in enumerate(run):
            row = {"name": os.path.basename(pp), "CD": cd[i], "EMD": emd[i], "hausdorff": hd[i]}
            g_cd.append(cd[i])
            g_hd.append(hd[i])
            g_emd.append(emd[i])
            g_jsd.append(float(jsd[i]))
            p2f, u = _p2f(pp, pred, i, name, mesh_dir, write_p2m, uni, p2f_search)
            if p2f is not None and p2f.size > 0:
                row["p2f avg"] = np.nanmean(p2f)
                row["p2f std"] = np.nanstd(p2f)
                g_p2f.append(p2f)
                row["JSD"] = float(jsd[i])
                if u is not None:
                    g_uni.append(u)
                    for j in range(PERCENTAGES):
                        row["uniform_%d" % j] = u[j]
            rows.append(row)
    summary = OrderedDict()
    summary["CD"] = np.nanmean(g_cd)
    summary["EMD"] = np.nanmean(g_emd)
    summary["hausdorff"] = np.nanmean(g_hd)
    if g_p2f:
        allp = np.concatenate(g_p2f, axis=0)
        summary["p2f avg"] = np.nanmean(allp)
        summary["p2f std"] = np.nanstd(allp)
    summary["JSD"] = np.nanmean(g_jsd)
    if g_uni:
        for j, v in enumerate(np.mean(np.array(g_uni), axis=0)):
            summary["uniform_%d" % j] = v
    os.makedirs(save_path, exist_ok=True)
    with open(os.path.join(save_path, "evaluation.csv"), "w") as f:
        writer = csv.DictWriter(f, fieldnames=FIELDNAMES, restval="-", extrasaction="ignore")
        writer.writeheader()
        for row in rows:
            writer.writerow(row)
        writer.writerow(summary)
    return rows, summary


def _p2f(pred_path, pred_gpu, i, name, mesh_dir, write_p2m, uni=None, search="tiles"):
    """(the file's point-to-surface distances (float32 [N]) or None, its uniformity [5] or None).  uni: None, or the
    --uniform settings dict(seeds, seed, write, surface)."""
    out_path = pred_path[:-4] + "_point2mesh_distance.xyz"
    prefix = pred_path[:-4]
    dev = pred_gpu.device
    if mesh_dir is None:
        if not os.path.isfile(out_path):
            return None, None
        d = np.atleast_2d(np.loadtxt(out_path, dtype=np.float32))
        u = None
        if uni is not None and all(os.path.isfile(prefix + t) for t in ("_disk_idx.txt", "_radius.txt", "_point2mesh_distance.txt")):
            mapped, radii, csr = metrics.read_disk_files(prefix)
            if len(radii) != PERCENTAGES:
                raise ValueError(f"{prefix}_radius.txt: {len(radii)} radii, the CSV has {PERCENTAGES} uniformity columns")
            u = metrics.uniformity(torch.from_numpy(mapped).to(dev), tuple(torch.from_numpy(a).to(dev) for a in csr), radii)
        return (d[:, 3] if d.size > 0 else d.reshape(-1)), u
    off = os.path.join(mesh_dir, name + ".off")
    if not os.path.isfile(off):
        return None, None
    verts, faces = metrics.read_off(off)
    vt, ft = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
    if uni is None:
        dist, face = metrics.point_to_mesh_distance(pred_gpu[i], vt, ft, search=search), None
    else:
        dist, face = metrics.point_to_mesh_distance(pred_gpu[i], vt, ft, return_face=True, search=search)
    dist = dist.cpu().numpy()
    if write_p2m:
        tokens = np.atleast_2d(np.loadtxt(pred_path, dtype=np.float64))[:, :3]
        with open(out_path, "w") as f:
            f.write(format_p2m(tokens, dist))
    u = None
    if uni is not None:
        radii, _ = metrics.mesh_area_radii(verts, faces)
        mapped = metrics.mapped_points(pred_gpu[i], vt, ft, face=face)
        seeds, seed_face, _ = metrics.sample_mesh(vt, ft, uni["seeds"], uni["seed"])
        if uni.get("surface"):
            reach = metrics.surface_reach(seeds, seed_face, vt, ft, float(radii[-1]))
            _, csr = metrics.disks(mapped, seeds, radii, reach=reach, mapped_face=face)
        else:
            _, csr = metrics.disks(mapped, seeds, radii)
        u = metrics.uniformity(mapped, csr, radii)
        if uni["write"]:
            metrics.write_disk_files(prefix, pred_gpu[i], dist, mapped, csr, radii)
    return dist, u


def summary_line(summary) -> str:
    return "\t" + "  ".join(f"[{k}]{summary[k]:>.8f}" if k in summary else f"[{k}]-" for k in SUMMARY_KEYS)


def main(argv=None):
    limit_host_threads()               # the host side within the CPUs this process owns
    ap = ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pred", type=str, required=True, help=".xyz")
    ap.add_argument("--gt", type=str, required=True, help=".xyz")
    ap.add_argument("--save_path", type=str, required=True, help="path to save the result")
    ap.add_argument("--mesh", type=str, default=None, help="directory of <name>.off meshes: compute P2F")
    ap.add_argument("--write_p2m", action="store_true", help="with --mesh: write <pred>_point2mesh_distance.xyz")
    ap.add_argument("--cloud_batch", type=int, default=16)
    ap.add_argument("--emd_levels_top", type=int, default=7)
    ap.add_argument("--uniform", action="store_true",
                    help="fill uniform_0..4: with --mesh from disks made on the GPU around seeds on the mesh (--uniform_disks); "
                         "without --mesh from <pred>_disk_idx.txt, _radius.txt and _point2mesh_distance.txt")
    ap.add_argument("--uniform_disks", choices=("ball", "surface"), default="ball",
                    help="ball: Euclidean balls, which on thin parts also take in the opposite side; surface: only the ball's "
                         "points connected to the seed along the surface inside it (not a geodesic length; parity with CGAL's "
                         "geodesic disks unpinned)")
    ap.add_argument("--uniform_seeds", type=int, default=1000, help="seeds (disks per radius) per mesh")
    ap.add_argument("--uniform_seed", type=int, default=0, help="key of the seeds' random numbers")
    ap.add_argument("--write_disks", action="store_true",
                    help="with --uniform --mesh: write <pred>_disk_idx.txt, _radius.txt and _point2mesh_distance.txt")
    ap.add_argument("--p2f_search", choices=metrics.P2F_SEARCHES, default="tiles",
                    help="closest-triangle search of P2F: tiles of 64 triangles and their boxes, or a uniform grid of the "
                         "triangles (for many points near a large mesh); the same numbers and files either way")
    a = ap.parse_args(argv)
    _, summary = evaluate(os.path.abspath(a.pred), os.path.abspath(a.gt), a.save_path, a.mesh, a.write_p2m, a.cloud_batch,
                          a.emd_levels_top, uniform=a.uniform, uniform_seeds=a.uniform_seeds, uniform_seed=a.uniform_seed,
                          write_disks=a.write_disks, uniform_disks=a.uniform_disks, p2f_search=a.p2f_search)
    print(f"Evaluation: {a.save_path}")
    print(summary_line(summary))


if __name__ == "__main__":
    main()
