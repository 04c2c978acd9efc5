"""Generate tests/golden/eval_uniform.npz: what the REFERENCE's analyze_uniform (evaluation/evaluate.py:108-165) computes on
deterministic synthetic inputs.

Runs only in the build container (needs the reference checkout, read-only, and sklearn).  The text of `cal_nearest_distance`
and `analyze_uniform` is taken from the reference's evaluate.py at run time (the file itself cannot be imported: it builds a
TF 1 graph on import), executed with the undefined `load` supplied as np.loadtxt, on files written to a temporary directory.
Nothing of that text is kept; the fixture holds arrays only.

Three cases - a subdivided icosphere, a torus and a thin folded sheet (the generators of tests/eval_ref.py) - with one cloud
each: samples of the surface, an eighth of them jittered off it, a few duplicated.  Mapped points, 1000 seeds (from the Philox
uniforms of key 0) and the disks are those of the float64 restatement (tests/uniform_ref.py).  Every mapped point keeps a
distance of at least MARGIN r_j from the sphere of radius r_j around every seed, so that fp32 and fp64 membership agree;
points that do not are drawn again.  The cloud is smaller than the 2048 points a first plan named: the fixture is kept within
the size of the other eval_*.npz files, and the 1000 seeds are fixed by the reference.

  python tools/make_golden_uniform.py
"""
from __future__ import annotations

import contextlib
import io
import math
import os
import re
import sys
import tempfile
from time import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import eval_ref as R  # noqa: E402
import uniform_ref as U  # noqa: E402

REF = os.environ.get("PF_REF_ROOT", "/root/reference")
GOLDEN = os.path.join(ROOT, "tests", "golden")
S = 1000             # analyze_uniform hard-codes it
N = 640
MARGIN = 1e-5
SEED = 0


def reference_functions():
    """analyze_uniform of the reference, from its text."""
    src = open(os.path.join(REF, "evaluation", "evaluate.py")).read()
    body = src[src.index("def cal_nearest_distance("):src.index("#os.environ['TF_ENABLE_AUTO_MIXED_PRECISION']")]
    from sklearn.neighbors import NearestNeighbors
    ns = {"np": np, "math": math, "re": re, "time": time, "NearestNeighbors": NearestNeighbors, "load": np.loadtxt,
          "precentages": U.PERCENTAGES.copy()}
    exec(compile(body, "<analyze_uniform>", "exec"), ns)
    return ns["analyze_uniform"]


def meshes():
    v0, f0 = R.icosphere(2)
    v1, f1 = R.torus(24, 12)
    v2, f2 = R.sheet(nx=12, ny=8, degenerate=False)
    return [("icosphere", v0 * 0.8, f0), ("torus", v1, f1), ("sheet", v2, f2)]


def cloud(verts, faces, rng):
    scale = np.ptp(verts, axis=0).max()
    pts = R.sample_surface(verts, faces, N, rng)
    k = N // 8
    pts[k:2 * k] += rng.normal(0, 5e-3 * scale, (k, 3))
    pts[2 * k:2 * k + 6] = pts[:6]                                  # duplicated points
    return pts.astype(np.float32)


def near_a_radius(mapped, seeds, radii):
    d = U.seed_distances(mapped, seeds)                            # [S,N]
    return (np.abs(d[:, :, None] - radii[None, None, :]) <= MARGIN * radii[None, None, :]).any(-1).any(0)


def main():
    from puflow_amd.metrics import write_disk_files
    analyze_uniform = reference_functions()
    rng = np.random.default_rng(2025)
    uni = U.uniforms(SEED, S)
    out = {"uniforms": uni, "seed": np.array(SEED), "percentages": U.PERCENTAGES, "ncases": np.array(3)}
    for c, (name, verts, faces) in enumerate(meshes()):
        verts = verts.astype(np.float32)
        radii, cum = U.area_radii(verts, faces)
        assert np.abs(uni[:, :1].astype(np.float64) - (cum / cum[-1])[None, :]).min() > 1e-7     # no uniform on a face's boundary
        seeds = U.seeds_from_uniforms(verts, faces, uni)[0].astype(np.float32)
        pts = cloud(verts, faces, rng)
        k = N // 8
        for _ in range(100):
            mapped = U.closest_points(pts, verts, faces)[0].astype(np.float32)
            bad = near_a_radius(mapped, seeds, radii)
            if not bad.any():
                break
            pts[bad] = R.sample_surface(verts, faces, int(bad.sum()), rng).astype(np.float32)
            pts[2 * k:2 * k + 6] = pts[:6]
        else:
            raise RuntimeError("points stay near a disk's boundary")
        assert not near_a_radius(mapped, seeds, radii).any()
        _, dist = U.closest_points(pts, verts, faces)[1:]
        counts, offsets, member, level = U.disks(mapped, seeds, radii)
        with tempfile.TemporaryDirectory() as td:
            prefix = os.path.join(td, "case")
            write_disk_files(prefix, pts, dist.astype(np.float32), mapped, (offsets, member, level), radii)
            with contextlib.redirect_stdout(io.StringIO()):
                ref = analyze_uniform(prefix + "_disk_idx.txt", prefix + "_radius.txt", prefix + "_point2mesh_distance.txt")[:, 0]
        mine = U.uniformity(mapped, (offsets, member, level), radii)
        kept = counts >= 5
        assert (~kept).any() and kept.mean() >= 0.5, (name, kept.mean())
        assert np.all(np.abs(mine - ref) <= 1e-10 * np.abs(ref)), (name, mine, ref)
        f32 = U.uniformity(mapped, (offsets, member, level), radii, dtype=np.float32)
        print(f"{name}: F={len(faces)} N={N} members {len(member)} kept {kept.mean(0).round(3)} ref {ref} "
              f"restatement rel {np.abs(mine / ref - 1).max():.2e} fp32 differences rel {np.abs(f32 / ref - 1).max():.2e}")
        out[f"c{c}_name"] = np.frombuffer(name.encode(), np.uint8)
        out[f"c{c}_verts"], out[f"c{c}_faces"] = verts, faces.astype(np.int16)
        out[f"c{c}_cloud"], out[f"c{c}_mapped"], out[f"c{c}_seeds"] = pts, mapped, seeds
        out[f"c{c}_radii"] = radii
        out[f"c{c}_counts"], out[f"c{c}_offsets"] = counts.astype(np.int16), offsets.astype(np.int32)
        out[f"c{c}_member"], out[f"c{c}_level"] = member.astype(np.int16), level.astype(np.int8)
        out[f"c{c}_uniform"] = ref
    os.makedirs(GOLDEN, exist_ok=True)
    path = os.path.join(GOLDEN, "eval_uniform.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
