"""Generate tests/golden/eval_*.npz: what the REFERENCE's scoring step computes on deterministic synthetic inputs.

Runs only in the build container (needs the reference checkout, read-only).  The fixtures hold arrays only:
  eval_p2f.npz  - three synthetic meshes (subdivided icosphere, torus, thin folded sheet with
                  slivers), two clouds each (on-surface samples, 1e-3 and 1e-1 noise, far points) and the ground-truth clouds the CLI test
                  pairs them with; the distances and the output file of the reference's CGAL `evaluation/evaluation` binary.
  eval_emd.npz  - approx-match costs of the reference's CPU op (tf_approxmatch.cpp approxmatch_cpu + matchcost_cpu, levels
                  8 .. -2): n = m, n = 2m, clustered clouds, duplicated points.  The two functions are compiled from the
                  reference's file into a temporary directory outside the repository; nothing of their text is kept.
  eval_jsd.npz  - JSD values and grid counters of the reference's evaluation/jsd.py on pairs of clouds.
Every cloud that goes through the occupancy grid is kept clear of cell boundaries (see `clear_of_boundaries`).

  python tools/make_golden_eval.py
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_ref as R  # noqa: E402

REF = os.environ.get("PF_REF_ROOT", "/root/reference")
GOLDEN = os.path.join(ROOT, "tests", "golden")
GAP = 2e-5           # squared-distance gap a point keeps between its nearest and second-nearest grid cell (normalised * 0.5)


def np_normalize(pts):
    """evaluate.py's np_normalize in float32: centroid, furthest distance, then * 0.5."""
    pts = np.asarray(pts, dtype=np.float32)
    c = pts - pts.mean(axis=0, keepdims=True)
    return c / np.sqrt((c ** 2).sum(-1)).max() * np.float32(0.5)


def clear_of_boundaries(cand: np.ndarray, n: int) -> np.ndarray:
    """The first n candidate points, every point whose two nearest grid cells are within GAP of each other (after the cloud's
    own normalisation) moved halfway towards its nearest cell centre, until none is left: the nearest cell is then the same
    under any rounding of the normalisation or the distance."""
    grid = R.sphere_grid(28)
    pts = np.asarray(cand[:n], dtype=np.float64).copy()
    for _ in range(50):
        p32 = pts.astype(np.float32)
        q = np_normalize(p32).astype(np.float64)
        idx, gap = R.nearest_cells(q, grid)
        bad = gap < GAP
        if not bad.any():
            return p32
        c = (p32 - p32.mean(axis=0, keepdims=True)).astype(np.float64)
        r = np.sqrt((c ** 2).sum(-1))
        far = int(r.argmax())
        if bad[far]:                   # the furthest point sets the scale: it moves outwards, the others rescale with it
            pts[far] += c[far] * 1e-3
            bad[far] = False
        pts[bad] += (grid[idx[bad]].astype(np.float64) - q[bad]) * 0.5 * (r[far] / 0.5)
    raise RuntimeError("points stay near grid-cell boundaries")


def meshes():
    v0, f0 = R.icosphere(3)
    v1, f1 = R.torus(48, 24)
    v2, f2 = R.sheet(degenerate=False)        # CGAL's closest point on a zero-area face is NaN
    return [("icosphere", v0 * 0.8, f0), ("torus", v1, f1), ("sheet", v2, f2)]


def p2f_points(verts, faces, n, rng):
    scale = np.ptp(verts, axis=0).max()
    on = R.sample_surface(verts, faces, n, rng)
    k = n // 8
    on[k:2 * k] += rng.normal(0, 1e-3 * scale, (k, 3))
    on[2 * k:4 * k] += rng.normal(0, 1e-1 * scale, (2 * k, 3))
    on[4 * k:4 * k + 8] = rng.uniform(-1, 1, (8, 3)) * 3 * scale              # far points
    on[4 * k + 8:4 * k + 12] = verts[faces[rng.integers(0, len(faces), 4), 0]]  # exactly on vertices
    return on


def make_p2f():
    exe = os.path.join(REF, "evaluation", "evaluation")
    out = {}
    rng = np.random.default_rng(2024)
    with tempfile.TemporaryDirectory() as td:
        case = 0
        for name, verts, faces in meshes():
            verts = verts.astype(np.float32)
            off = os.path.join(td, f"{name}.off")
            R.write_off(off, verts, faces)
            for n in (256, 384):
                pred = clear_of_boundaries(p2f_points(verts, faces, n, rng), n)
                gt = clear_of_boundaries(R.sample_surface(verts, faces, n, rng), n)
                xyz = os.path.join(td, f"case{case}.xyz")
                R.write_points(xyz, pred)
                subprocess.run([exe, off, xyz], check=True, stdout=subprocess.DEVNULL, timeout=600)
                with open(os.path.join(td, f"case{case}_point2mesh_distance.xyz"), "rb") as f:
                    text = f.read()
                d = np.loadtxt(text.decode().splitlines())[:, 3]
                out[f"c{case}_name"] = np.frombuffer(f"{name}_{n}".encode(), np.uint8)
                out[f"c{case}_verts"] = verts
                out[f"c{case}_faces"] = faces.astype(np.int32)
                out[f"c{case}_pred"] = pred
                out[f"c{case}_gt"] = gt
                out[f"c{case}_cgal_dist"] = d
                out[f"c{case}_cgal_text"] = np.frombuffer(text, np.uint8)
                print(f"p2f case {case} {name} n={n}: F={len(faces)} mean {d.mean():.6g} max {d.max():.6g}")
                case += 1
    out["ncases"] = np.array(case)
    return out


def approxmatch_lib(td: str):
    """approxmatch_cpu + matchcost_cpu of the reference's CPU op, compiled as a shared library in td."""
    src = open(os.path.join(REF, "evaluation", "tf_ops", "approxmatch", "tf_approxmatch.cpp")).read()
    body = src[src.index("void approxmatch_cpu("):src.index("void matchcostgrad_cpu(")]
    cpp = os.path.join(td, "am.cpp")
    with open(cpp, "w") as f:
        f.write('#include <algorithm>\n#include <vector>\n#include <math.h>\nextern "C" {\n' + body + "}\n")
    so = os.path.join(td, "am.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, cpp])
    return ctypes.CDLL(so)


def ref_emd(lib, a, b):
    a = np.ascontiguousarray(a, np.float32)[None]
    b = np.ascontiguousarray(b, np.float32)[None]
    n, m = a.shape[1], b.shape[1]
    match = np.zeros((1, n, m), np.float32)
    cost = np.zeros(1, np.float32)
    P = ctypes.c_void_p
    lib.approxmatch_cpu(1, n, m, P(a.ctypes.data), P(b.ctypes.data), P(match.ctypes.data))
    lib.matchcost_cpu(1, n, m, P(a.ctypes.data), P(b.ctypes.data), P(match.ctypes.data), P(cost.ctypes.data))
    return float(cost[0]) / n


def make_emd():
    rng = np.random.default_rng(7)

    def cloud(n):
        return R.normalize(rng.normal(size=(n, 3))).astype(np.float32)
    cases = {
        "nm512": (cloud(512), cloud(512)),
        "n2m": (cloud(512), cloud(256)),
    }
    centres = rng.normal(size=(6, 3))
    cl = lambda n: R.normalize(centres[rng.integers(0, 6, n)] + 0.05 * rng.normal(size=(n, 3))).astype(np.float32)  # noqa: E731
    cases["clustered"] = (cl(384), cl(384))
    a = cloud(256)
    cases["duplicated"] = (np.concatenate([a[:128], a[:128]]), cloud(256))
    out = {}
    with tempfile.TemporaryDirectory() as td:
        lib = approxmatch_lib(td)
        for k, (a, b) in cases.items():
            out[f"{k}_a"], out[f"{k}_b"] = a, b
            out[f"{k}_cost8"] = np.array(ref_emd(lib, a, b))
            print(f"emd {k}: n={len(a)} m={len(b)} ref(top 8) {float(out[k + '_cost8']):.9g}  restated(top 8) "
                  f"{R.approx_match_cost(a, b, 8):.9g}  restated(top 7) {R.approx_match_cost(a, b, 7):.9g}")
    out["cases"] = np.array(list(cases))
    return out


def make_jsd():
    sys.path.insert(0, os.path.join(REF, "evaluation"))
    import warnings
    from jsd import entropy_of_occupancy_grid, jsd_between_point_cloud_sets
    rng = np.random.default_rng(11)
    out = {}
    pairs = []
    for n in (2048, 5000):
        a = R.normalize(rng.normal(size=(2 * n, 3)) * [1.0, 0.6, 0.3])
        b = R.normalize(rng.normal(size=(2 * n, 3)) * [1.0, 0.5, 0.35] + [0.05, 0, 0])
        pairs.append((clear_of_boundaries(a, n), clear_of_boundaries(b, n)))
    for i, (a, b) in enumerate(pairs):
        na, nb = np_normalize(a)[None], np_normalize(b)[None]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out[f"j{i}_jsd"] = np.array(jsd_between_point_cloud_sets(na, nb))
            out[f"j{i}_count_a"] = entropy_of_occupancy_grid(na, 28, True)[1]
            out[f"j{i}_count_b"] = entropy_of_occupancy_grid(nb, 28, True)[1]
        out[f"j{i}_a"], out[f"j{i}_b"] = a, b
        print(f"jsd pair {i}: n={len(a)} jsd {float(out[f'j{i}_jsd']):.12g}")
    out["npairs"] = np.array(len(pairs))
    return out


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    np.savez_compressed(os.path.join(GOLDEN, "eval_emd.npz"), **make_emd())
    np.savez_compressed(os.path.join(GOLDEN, "eval_jsd.npz"), **make_jsd())
    np.savez_compressed(os.path.join(GOLDEN, "eval_p2f.npz"), **make_p2f())


if __name__ == "__main__":
    main()
