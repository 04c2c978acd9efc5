"""The mesh scorer (puflow_amd.mesh_metrics, python -m puflow_amd.evaluate_mesh) against float64 numpy on the device's own
samples, and the search switch of both scorers: --p2f_search / --search change no byte of what is written."""
import csv
import filecmp
import os

import numpy as np
import pytest
import torch

import attr_ref
import eval_ref as R
import recon_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _mesh(v, f):
    return _dev(v, F32), _dev(f, np.int64)


@pytest.fixture(scope="module")
def p2f_fx(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_p2f.npz"))


def test_evaluate_writes_the_same_bytes_with_either_search(tmp_path, p2f_fx):
    from puflow_amd import evaluate
    for leg in ("tiles", "grid"):
        for d in ("pred", "gt", "mesh"):
            (tmp_path / leg / d).mkdir(parents=True)
        for c in range(int(p2f_fx["ncases"])):
            name = bytes(p2f_fx[f"c{c}_name"]).decode()
            R.write_points(tmp_path / leg / "pred" / f"{name}.xyz", p2f_fx[f"c{c}_pred"])
            R.write_points(tmp_path / leg / "gt" / f"{name}.xyz", p2f_fx[f"c{c}_gt"])
            R.write_off(tmp_path / leg / "mesh" / f"{name}.off", p2f_fx[f"c{c}_verts"], p2f_fx[f"c{c}_faces"])
        argv = ["--pred", str(tmp_path / leg / "pred"), "--gt", str(tmp_path / leg / "gt"), "--save_path", str(tmp_path / leg / "out"),
                "--mesh", str(tmp_path / leg / "mesh"), "--write_p2m", "--uniform", "--write_disks", "--uniform_seeds", "200"]
        evaluate.main(argv + (["--p2f_search", "grid"] if leg == "grid" else []))
    for sub in ("out", "pred"):
        names = sorted(os.listdir(tmp_path / "tiles" / sub))
        assert names == sorted(os.listdir(tmp_path / "grid" / sub))
        _, mismatch, errors = filecmp.cmpfiles(tmp_path / "tiles" / sub, tmp_path / "grid" / sub, names, shallow=False)
        assert not mismatch and not errors
    assert "evaluation.csv" in os.listdir(tmp_path / "grid" / "out")
    assert sum(n.endswith("_point2mesh_distance.xyz") for n in os.listdir(tmp_path / "grid" / "pred")) == int(p2f_fx["ncases"])
    assert sum(n.endswith("_disk_idx.txt") for n in os.listdir(tmp_path / "grid" / "pred")) == int(p2f_fx["ncases"])


def test_a_mesh_against_itself():
    from puflow_amd import mesh_metrics
    v, f = R.icosphere(3)
    s = mesh_metrics.score(*_mesh(v, f), *_mesh(v, f), samples=20000, seed=3)
    diag = float(np.linalg.norm(np.ptp(v.astype(F32).astype(np.float64), axis=0)))
    assert s["accuracy"] <= 1e-6 * diag and s["completeness"] <= 1e-6 * diag and s["hausdorff"] <= 1e-6 * diag
    assert s["normal_consistency"] >= 1 - 1e-6 and s["fscore"] == 1.0
    assert s["open_edges"] == 0 and s["euler"] == 2 and s["vertices"] == len(v) and s["faces"] == len(f)


def _unit_normals(v, f):
    t = np.asarray(v, np.float64)[f]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    a2 = np.linalg.norm(n, axis=1)
    return n / np.where(a2 > 0, a2, 1.0)[:, None], a2


def _closest(points, v, f):
    """(distance, closest face) in float64"""
    t3 = np.asarray(v, np.float64)[f]
    d2 = np.array([R.point_triangle_d2(p, t3) for p in np.asarray(points, np.float64)])
    return np.sqrt(d2.min(1)), d2.argmin(1)


PAIRS = {"icospheres": lambda: (R.icosphere(3), R.icosphere(4)),
         "tori": lambda: (R.torus(64, 32, bump=0.15), R.torus(64, 32))}


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_score_against_float64_on_the_same_samples(pair):
    from puflow_amd import mesh_metrics
    (pv, pf), (gv, gf) = PAIRS[pair]()
    pv, gv = pv.astype(F32), gv.astype(F32)
    S, seed = 1000, 5
    pm, gm = _mesh(pv, pf), _mesh(gv, gf)
    (sp, fp), (sg, fg) = mesh_metrics.draw(*pm, *gm, S, seed)
    sp, fp, sg, fg = sp.cpu().numpy(), fp.cpu().numpy(), sg.cpu().numpy(), fg.cpu().numpy()
    d_pg, c_pg = _closest(sp, gv, gf)
    d_gp, c_gp = _closest(sg, pv, pf)
    diag = float(np.linalg.norm(np.ptp(gv.astype(np.float64), axis=0)))
    bar = lambda ref: 1e-5 * ref + 1e-7 * diag                           # noqa: E731  the project's P2F bar
    # tau: the middle of the widest gap among the 100 central distances, so that no sample is within the bar of the threshold
    alld = np.sort(np.concatenate([d_pg, d_gp]))
    k = len(alld) // 2 - 50 + int(np.argmax(np.diff(alld[len(alld) // 2 - 50:len(alld) // 2 + 50])))
    tau = 0.5 * (alld[k] + alld[k + 1]) / diag
    thr = tau * diag
    assert np.all(np.abs(np.concatenate([d_pg, d_gp]) - thr) > bar(np.concatenate([d_pg, d_gp])))
    s = mesh_metrics.score(*pm, *gm, samples=S, seed=seed, tau=tau)
    print(f"mesh score {pair}: " + " ".join(f"{k}={v:.6g}" for k, v in s.items()))
    acc, comp, hd = d_pg.mean(), d_gp.mean(), max(d_pg.max(), d_gp.max())
    assert abs(s["accuracy"] - acc) <= bar(acc) and abs(s["completeness"] - comp) <= bar(comp)
    assert abs(s["chamfer_l1"] - 0.5 * (acc + comp)) <= bar(0.5 * (acc + comp)) and abs(s["hausdorff"] - hd) <= bar(hd)
    prec, rec = float((d_pg < thr).mean()), float((d_gp < thr).mean())
    assert 0 < prec < 1 or 0 < rec < 1
    assert s["fscore"] == 2.0 * prec * rec / (prec + rec)
    # the normal columns: "the closest face" is not unique - a sample on the convex side of an edge or a vertex is exactly as
    # near to every face around it, and those faces' normals differ by degrees (argmin over float64 and the device's tie rule
    # then pick different ones: 1.2e-4 on the mean of the tori).  So the device's faces are first shown to BE closest faces -
    # their float64 distance is the minimum within the distance bar - and the float64 normals are taken there.
    from puflow_amd import metrics
    for pts, mesh, (mv, mf), dmin, name in ((sp, gm, (gv, gf), d_pg, "c_pg"), (sg, pm, (pv, pf), d_gp, "c_gp")):
        _, face = metrics.point_to_mesh_distance(_dev(pts), *mesh, return_face=True)
        face = face.cpu().numpy()
        t3 = mv.astype(np.float64)[mf[face]]
        own = np.sqrt(np.array([R.point_triangle_d2(p, t[None])[0] for p, t in zip(pts.astype(np.float64), t3)]))
        assert np.all(own <= dmin + bar(dmin)), name
        if name == "c_pg":
            c_pg = face
        else:
            c_gp = face
    npn, npa = _unit_normals(pv, pf)
    ngn, nga = _unit_normals(gv, gf)
    dots = np.concatenate([(npn[fp] * ngn[c_pg]).sum(1)[(npa[fp] > 0) & (nga[c_pg] > 0)],
                           (ngn[fg] * npn[c_gp]).sum(1)[(nga[fg] > 0) & (npa[c_gp] > 0)]])
    assert abs(s["normal_consistency"] - np.abs(dots).mean()) <= 1e-5 and abs(s["normal_signed"] - dots.mean()) <= 1e-5
    t = pv.astype(np.float64)[pf]
    area = 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1).sum()
    vol = M.volume(pv, pf)
    assert abs(s["area"] - area) <= 1e-9 * area and abs(s["volume"] - vol) <= 1e-9 * abs(vol)
    assert s["euler"] == M.euler(pv, pf) == (2 if pair == "icospheres" else 0) and s["open_edges"] == M.open_edges(pf) == 0
    assert s["vertices"] == len(pv) and s["faces"] == len(pf)


def test_degenerate_faces_are_left_out_of_the_normal_columns_only():
    from puflow_amd import mesh_metrics
    v, f = R.sheet(degenerate=True)
    gv, gf = R.sheet(degenerate=False)
    s = mesh_metrics.score(*_mesh(v, f), *_mesh(gv, gf), samples=2000, seed=1)
    assert all(np.isfinite(s[k]) for k in mesh_metrics.COLUMNS[1:])
    assert 0 <= s["normal_consistency"] <= 1 + 1e-12 and abs(s["normal_signed"]) <= s["normal_consistency"] + 1e-12


def _write_pairs(tmp_path):
    from puflow_amd import reconstruct as P
    pts, nrm = attr_ref.surface("sphere", 0.0, 512)
    v, f, _ = P.mesh_from_cloud(_dev(pts, F32), _dev(nrm, F32))
    pred, gt = tmp_path / "pred", tmp_path / "gt"
    pred.mkdir()
    gt.mkdir()
    P.write_off(pred / "sphere.off", v, f)
    P.write_off(gt / "sphere.off", *R.icosphere(4))
    P.write_off(pred / "ico.off", *R.icosphere(3))
    P.write_off(gt / "ico.off", *R.icosphere(4))
    P.write_off(pred / "alone.off", *R.icosphere(1))
    return pred, gt


def test_cli_end_to_end_and_search_switch(tmp_path, capsys):
    from puflow_amd import evaluate_mesh, mesh_metrics, metrics
    pred, gt = _write_pairs(tmp_path)
    base = ["--pred", str(pred), "--gt", str(gt), "--samples", "20000", "--seed", "2", "--tau", "0.02"]
    evaluate_mesh.main(base + ["--save_path", str(tmp_path / "grid")])
    printed = capsys.readouterr().out
    assert evaluate_mesh.SKIPPED_LINE.format(name="alone", where=str(pred)) in printed
    evaluate_mesh.main(base + ["--save_path", str(tmp_path / "tiles"), "--search", "tiles"])
    assert (tmp_path / "grid" / "mesh_evaluation.csv").read_bytes() == (tmp_path / "tiles" / "mesh_evaluation.csv").read_bytes()
    with open(tmp_path / "grid" / "mesh_evaluation.csv") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == mesh_metrics.COLUMNS and len(rows) == 1 + 2 + 1
    scores = []
    for name, row in zip(("ico", "sphere"), rows[1:3]):                  # sorted order
        r = dict(zip(rows[0], row))
        assert r["name"] == name + ".off"
        pv, pf = metrics.read_off(pred / f"{name}.off")
        gv, gf = metrics.read_off(gt / f"{name}.off")
        s = mesh_metrics.score(*_mesh(pv, pf), *_mesh(gv, gf), samples=20000, seed=2, tau=0.02)
        for k in mesh_metrics.COLUMNS[1:]:
            assert (int(r[k]) if isinstance(s[k], int) else float(r[k])) == s[k], (name, k)
        scores.append(s)
    assert scores[1]["open_edges"] == 0 and scores[1]["euler"] == 2      # the reconstructed sphere is closed, of genus 0
    last = dict(zip(rows[0], rows[-1]))
    assert last["name"] == "-"
    for k in mesh_metrics.COLUMNS[1:]:
        assert float(last[k]) == float(np.mean([float(s[k]) for s in scores])), k
