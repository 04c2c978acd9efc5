"""Data preparation CLI - from meshes to what the other entry points read, on the GPU (puflow_amd.sampling):

  python -m puflow_amd.prepare --mesh DIR --out DIR [--seed 0] [--ratio 5]
                               [--patches P [--num_point 256] [--up_ratio 4] [--cloud_points 2500] [--patch_metric ball|surface]]
                               [--clouds 2048,8192]

--patches P writes `<out>/patches.npz`: P patches of every `<mesh>/<name>.off` (sorted by name), arrays `poisson_<num_point>`
[M,num_point,3] and `poisson_<num_point * up_ratio>`, what `python -m puflow_amd.train --data` loads (data.load_patch_arrays).
--clouds N0,N1,... writes one Poisson-disk cloud per mesh and count: `<out>/input_<N0>/<name>.xyz` for the first count (the
upsampler's input) and `<out>/gt_<Ni>/<name>.xyz` for the others (the evaluation's ground truth), through the upsampler's
writer.  Each count has its own Philox seed (--seed + 3 + its position; the patches use --seed .. --seed + 2), so the input is
no subset of the ground truth.  The reference has no counterpart: its files came from PU-GAN's Meshlab preparation.

The same arguments give the same bytes: the samples depend on (mesh, seed, counts) only, and the .npz is written with a fixed
time stamp.  The elimination's distances are Euclidean; a patch is cropped around its seed by Euclidean distance
(--patch_metric ball, the default) or by the surface distance of metrics.surface_reach (--patch_metric surface: on a thin part
a piece of one side instead of a two-sided slab; the project's own surface restriction, not a geodesic length - sampling.py's
head).
"""
from __future__ import annotations

import io
import os
import zipfile
from argparse import ArgumentParser
from glob import glob

import numpy as np
import torch

from . import metrics, sampling
from ._host import limit_host_threads
from .upsample import save_xyz


def save_npz(path: str, arrays) -> None:
    """An uncompressed .npz np.load reads, byte-identical for identical arrays (np.savez stamps every entry with the clock)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def mesh_paths(mesh_dir: str):
    paths = sorted(glob(os.path.join(mesh_dir, "*.off")))
    if not paths:
        raise FileNotFoundError(f"no .off mesh in {mesh_dir}")
    return paths


def prepare(mesh_dir: str, out_dir: str, seed: int = 0, ratio: int = 5, patches: int = 0, num_point: int = 256,
            up_ratio: int = 4, cloud_points: int = 2500, clouds=(), device=None, patch_metric: str = "ball"):
    """Returns the paths written."""
    device = torch.device(device or "cuda:0")
    os.makedirs(out_dir, exist_ok=True)
    written, per_mesh = [], []
    for i, n in enumerate(clouds):
        os.makedirs(os.path.join(out_dir, ("input_%d" if i == 0 else "gt_%d") % n), exist_ok=True)
    for path in mesh_paths(mesh_dir):
        name = os.path.basename(path)[:-4]
        verts, faces = metrics.read_off(path)
        vt, ft = torch.from_numpy(verts).to(device), torch.from_numpy(faces).to(device)
        if patches > 0:
            per_mesh.append({k: v.cpu().numpy() for k, v in
                             sampling.make_patches(vt, ft, patches, num_point, up_ratio, cloud_points, seed, ratio,
                                                   metric=patch_metric).items()})
        for i, n in enumerate(clouds):
            pts, _ = sampling.poisson_disk(vt, ft, n, seed + 3 + i, ratio)
            written.append(os.path.join(out_dir, ("input_%d" if i == 0 else "gt_%d") % n, name + ".xyz"))
            save_xyz(written[-1], pts.cpu().numpy())
    if per_mesh:
        written.append(os.path.join(out_dir, "patches.npz"))
        save_npz(written[-1], {k: np.concatenate([d[k] for d in per_mesh]) for k in per_mesh[0]})
    return written


def main(argv=None):
    limit_host_threads()
    ap = ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mesh", type=str, required=True, help="directory of <name>.off meshes")
    ap.add_argument("--out", type=str, required=True, help="directory to write into")
    ap.add_argument("--seed", type=int, default=0, help="key of the surface samples' random numbers")
    ap.add_argument("--ratio", type=int, default=5, help="candidates per kept point")
    ap.add_argument("--patches", type=int, default=0, help="patches per mesh: write patches.npz")
    ap.add_argument("--num_point", type=int, default=256)
    ap.add_argument("--up_ratio", type=int, default=4)
    ap.add_argument("--cloud_points", type=int, default=2500, help="points of the cloud the patch seeds are taken from")
    ap.add_argument("--patch_metric", choices=("ball", "surface"), default="ball",
                    help="how a patch is cropped around its seed: Euclidean ball, or surface-connected (metrics.surface_reach)")
    ap.add_argument("--clouds", type=str, default="", help="point counts, e.g. 2048,8192: input_<first> and gt_<others>")
    a = ap.parse_args(argv)
    clouds = [int(t) for t in a.clouds.split(",") if t.strip()]
    if a.patches <= 0 and not clouds:
        ap.error("nothing to do: give --patches and / or --clouds")
    for p in prepare(a.mesh, a.out, a.seed, a.ratio, a.patches, a.num_point, a.up_ratio, a.cloud_points, clouds,
                     patch_metric=a.patch_metric):
        print(p)


if __name__ == "__main__":
    main()
