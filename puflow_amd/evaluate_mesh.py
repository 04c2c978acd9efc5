"""Score reconstructed meshes against ground-truth meshes on the GPU.

    python -m puflow_amd.evaluate_mesh --pred DIR --gt DIR --save_path DIR [--samples 100000] [--seed 0] [--tau 0.01]
                                       [--search grid|tiles]

Every <name>.off present in both directories is scored, in sorted order (puflow_amd.mesh_metrics.score);
<save_path>/mesh_evaluation.csv gets one row per file and a last row of the columns' means.  A row depends on the two meshes,
--samples, --seed and --tau only; --search chooses the closest-triangle search and changes no value.
"""
from __future__ import annotations

import csv
import os
from argparse import ArgumentParser
from glob import glob

import numpy as np
import torch

from . import mesh_metrics, metrics

SKIPPED_LINE = "{name}.off: only in {where} - skipped"


def pair_paths(pred_dir: str, gt_dir: str):
    """([(name, gt path, pred path)] of the .off files present in both directories, sorted by name; [(name, directory)] of the
    files present in one of them only)"""
    gt = {os.path.basename(p)[:-4]: p for p in glob(os.path.join(gt_dir, "*.off"))}
    pred = {os.path.basename(p)[:-4]: p for p in glob(os.path.join(pred_dir, "*.off"))}
    both = sorted((n, gt[n], pred[n]) for n in pred if n in gt)
    alone = sorted([(n, pred_dir) for n in pred if n not in gt] + [(n, gt_dir) for n in gt if n not in pred])
    return both, alone


def evaluate_meshes(pred_dir: str, gt_dir: str, save_path: str, samples: int = 100000, seed: int = 0, tau: float = 0.01,
                    search: str = "grid", device=None):
    """Score the directory; returns (per-file rows, summary row) as written to mesh_evaluation.csv."""
    if search not in metrics.P2F_SEARCHES:
        raise ValueError(f"search is one of {metrics.P2F_SEARCHES}, got {search!r}")
    device = torch.device(device or "cuda:0")
    both, alone = pair_paths(pred_dir, gt_dir)
    for name, where in alone:
        print(SKIPPED_LINE.format(name=name, where=where), flush=True)
    if not both:
        raise FileNotFoundError(f"no <name>.off is in both {pred_dir} and {gt_dir}")
    rows = []
    for name, gp, pp in both:
        pv, pf = metrics.read_off(pp)
        gv, gf = metrics.read_off(gp)
        dev = lambda a: torch.from_numpy(a).to(device)      # noqa: E731
        row = {"name": name + ".off"}
        row.update(mesh_metrics.score(dev(pv), dev(pf), dev(gv), dev(gf), samples, seed, tau, search))
        rows.append(row)
    summary = {k: float(np.mean([float(r[k]) for r in rows])) for k in mesh_metrics.COLUMNS[1:]}
    os.makedirs(save_path, exist_ok=True)
    with open(os.path.join(save_path, "mesh_evaluation.csv"), "w") as f:
        writer = csv.DictWriter(f, fieldnames=mesh_metrics.COLUMNS, restval="-", extrasaction="ignore")
        writer.writeheader()
        for row in rows:
            writer.writerow({k: (repr(v) if isinstance(v, float) else v) for k, v in row.items()})
        writer.writerow({k: repr(v) for k, v in summary.items()})
    return rows, summary


def main(argv=None):
    ap = ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pred", type=str, required=True, help="directory of reconstructed <name>.off meshes")
    ap.add_argument("--gt", type=str, required=True, help="directory of ground-truth <name>.off meshes")
    ap.add_argument("--save_path", type=str, required=True, help="directory of mesh_evaluation.csv")
    ap.add_argument("--samples", type=int, default=100000, help="area-weighted samples per mesh")
    ap.add_argument("--seed", type=int, default=0, help="key of the samples' random numbers")
    ap.add_argument("--tau", type=float, default=0.01, help="F-score threshold, as a share of the ground truth's box diagonal")
    ap.add_argument("--search", choices=("grid", "tiles"), default="grid",
                    help="closest-triangle search: a uniform grid of the triangles, or tiles of 64 triangles (the same values)")
    a = ap.parse_args(argv)
    rows, summary = evaluate_meshes(os.path.abspath(a.pred), os.path.abspath(a.gt), a.save_path, a.samples, a.seed, a.tau, a.search)
    print(f"Mesh evaluation: {a.save_path} ({len(rows)} meshes)")
    print("\t" + "  ".join(f"[{k}]{summary[k]:>.8f}" for k in ("accuracy", "completeness", "chamfer_l1", "hausdorff",
                                                                  "normal_consistency", "fscore")))


if __name__ == "__main__":
    main()
