"""The evaluation metrics on the GPU (csrc/eval_metrics.hip, puflow_amd.metrics, python -m puflow_amd.evaluate) against the
reference's scoring step (tests/golden/eval_*.npz) and the float64 restatements (tests/eval_ref.py)."""
import csv
import os

import numpy as np
import pytest
import torch

import eval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def emd_fx(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_emd.npz"))


@pytest.fixture(scope="module")
def p2f_fx(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_p2f.npz"))


@pytest.fixture(scope="module")
def jsd_fx(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_jsd.npz"))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def test_approx_match_matches_reference_cpu_op_and_restatement(emd_fx):
    from puflow_amd.metrics import approx_match_emd
    for k in emd_fx["cases"]:
        a, b = emd_fx[f"{k}_a"], emd_fx[f"{k}_b"]
        c8 = float(approx_match_emd(_t(a)[None], _t(b)[None], 8)[0])
        ref8 = float(emd_fx[f"{k}_cost8"])
        assert abs(c8 - ref8) <= 1e-4 * ref8, (k, c8, ref8)
        c7 = float(approx_match_emd(_t(a)[None], _t(b)[None], 7)[0])
        ref7 = R.approx_match_cost(a, b, 7)
        assert abs(c7 - ref7) <= 1e-4 * ref7, (k, c7, ref7)


def test_approx_match_is_deterministic_and_batch_independent():
    from puflow_amd.metrics import approx_match_emd
    g = torch.Generator().manual_seed(5)
    a = torch.randn(5, 1000, 3, generator=g).to(DEV)
    b = torch.randn(5, 1000, 3, generator=g).to(DEV) * 0.9
    full = approx_match_emd(a, b)
    again = approx_match_emd(a, b)
    assert torch.equal(full, again)
    for i in range(5):
        one = approx_match_emd(a[i:i + 1].contiguous(), b[i:i + 1].contiguous())
        assert torch.equal(one[0], full[i]), i


def test_identical_clouds_score_zero():
    from puflow_amd.metrics import approx_match_emd, chamfer_hausdorff, normalize_point_cloud
    g = torch.Generator().manual_seed(3)
    a = torch.randn(4, 128, 3, generator=g).to(DEV)
    cd, hd = chamfer_hausdorff(a, a)
    assert float(cd.abs().max()) == 0.0 and float(hd.abs().max()) == 0.0
    n, _, _ = normalize_point_cloud(a)
    emd = approx_match_emd(n, n).cpu().numpy()
    # not exactly 0: the finest level still spreads a point's mass over close neighbours - with 128 points the soft
    # assignment is a permutation to 1e-6 (the restatement: 5e-10 .. 5.5e-7 for these clouds)
    assert emd.max() < 1e-6
    for i in range(4):
        ref = R.approx_match_cost(R.normalize(a[i].cpu().numpy()), R.normalize(a[i].cpu().numpy()), 7)
        assert abs(emd[i] - ref) <= 1e-4 * ref + 1e-9, (i, emd[i], ref)      # 1e-9: the float rounding of the summed costs


def test_chamfer_hausdorff_jsd_match_restatement(jsd_fx):
    from puflow_amd import metrics
    for i in range(int(jsd_fx["npairs"])):
        a, b = jsd_fx[f"j{i}_a"], jsd_fx[f"j{i}_b"]
        cd, hd = metrics.chamfer_hausdorff(_t(a)[None], _t(b)[None])
        na, nb = R.normalize(a), R.normalize(b)
        d = ((na[:, None, :] - nb[None, :, :]) ** 2).sum(-1)
        cd_r = d.min(1).mean() + d.min(0).mean()
        hd_r = d.min(1).max() + d.min(0).max()
        assert abs(float(cd[0]) - cd_r) <= 1e-4 * cd_r and abs(float(hd[0]) - hd_r) <= 1e-4 * hd_r
        pa, _, _ = metrics.normalize_point_cloud(_t(a)[None])
        pb, _, _ = metrics.normalize_point_cloud(_t(b)[None])
        np.testing.assert_array_equal(metrics.occupancy(pa * 0.5)[0], jsd_fx[f"j{i}_count_a"])
        np.testing.assert_array_equal(metrics.occupancy(pb * 0.5)[0], jsd_fx[f"j{i}_count_b"])
        j = metrics.jsd(_t(a), _t(b))
        assert abs(float(j[0]) - float(jsd_fx[f"j{i}_jsd"])) <= 1e-9


def test_point_mesh_distance_matches_cgal(p2f_fx):
    from puflow_amd.metrics import point_to_mesh_distance
    for c in range(int(p2f_fx["ncases"])):
        v, f, p = p2f_fx[f"c{c}_verts"], p2f_fx[f"c{c}_faces"], p2f_fx[f"c{c}_pred"]
        d = point_to_mesh_distance(_t(p), _t(v), torch.from_numpy(f).to(DEV)).cpu().numpy().astype(np.float64)
        ref = p2f_fx[f"c{c}_cgal_dist"]
        diag = float(np.linalg.norm(np.ptp(v, axis=0)))
        err = np.abs(d - ref)
        assert np.all(err <= 1e-5 * ref + 1e-7 * diag), (c, float(err.max()))


def test_points_on_vertices_and_centroids_are_on_the_surface(p2f_fx):
    from puflow_amd.metrics import point_to_mesh_distance
    for c in (0, 2, 4):
        v, f = p2f_fx[f"c{c}_verts"], p2f_fx[f"c{c}_faces"]
        tris = v.astype(np.float64)[f]
        q = np.concatenate([v, tris.mean(1)]).astype(np.float32)
        d = point_to_mesh_distance(_t(q), _t(v), torch.from_numpy(f).to(DEV))
        assert float(d.max()) < 1e-6, c


def test_degenerate_faces_match_restatement():
    """Zero-area faces (collinear corners, one repeated point) are the closest of their edges."""
    from puflow_amd.metrics import point_to_mesh_distance
    v, f = R.sheet(degenerate=True)
    v = v.astype(np.float32)
    rng = np.random.default_rng(4)
    q = np.concatenate([rng.uniform(-1, 1, (300, 3)) * [1.2, 0.8, 0.8], v[-6:] + rng.normal(0, 1e-2, (6, 3))]).astype(np.float32)
    d = point_to_mesh_distance(_t(q), _t(v), torch.from_numpy(f).to(DEV)).cpu().numpy()
    ref = R.point_mesh_dist(q, v, f)
    assert np.all(np.abs(d - ref) <= 1e-5 * ref + 1e-7 * 3.0)


def test_pruned_search_equals_brute_force():
    from puflow_amd.metrics import point_to_mesh_distance
    v, f = R.torus(320, 160, bump=0.15)                     # 102 400 faces
    rng = np.random.default_rng(9)
    p = R.sample_surface(v, f, 4096, rng) + rng.normal(0, 0.02, (4096, 3))
    p[:64] = rng.uniform(-2, 2, (64, 3))
    args = (_t(p), _t(v), torch.from_numpy(f).to(DEV))
    d0, f0 = point_to_mesh_distance(*args, return_face=True)
    d1, f1 = point_to_mesh_distance(*args, return_face=True, brute=True)
    assert torch.equal(d0, d1) and torch.equal(f0, f1)


def _write_case_dirs(tmp_path, fx):
    pred, gt, mesh = tmp_path / "pred", tmp_path / "gt", tmp_path / "mesh"
    for d in (pred, gt, mesh):
        d.mkdir()
    names = []
    for c in range(int(fx["ncases"])):
        name = bytes(fx[f"c{c}_name"]).decode()
        R.write_points(pred / f"{name}.xyz", fx[f"c{c}_pred"])
        R.write_points(gt / f"{name}.xyz", fx[f"c{c}_gt"])
        R.write_off(mesh / f"{name}.off", fx[f"c{c}_verts"], fx[f"c{c}_faces"])
        names.append((name, c))
    return pred, gt, mesh, sorted(names)


def _num(s):
    return float(s)


def test_cli_end_to_end(tmp_path, p2f_fx, capsys):
    from puflow_amd import evaluate
    pred, gt, mesh, names = _write_case_dirs(tmp_path, p2f_fx)
    out = tmp_path / "out"
    evaluate.main(["--pred", str(pred), "--gt", str(gt), "--save_path", str(out), "--mesh", str(mesh), "--write_p2m",
                   "--cloud_batch", "2"])
    printed = capsys.readouterr().out
    with open(out / "evaluation.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == evaluate.FIELDNAMES
    assert len(rows) == 1 + len(names) + 1
    all_d, jsds, cds = [], [], []
    for (name, c), row in zip(names, rows[1:-1]):
        r = dict(zip(rows[0], row))
        assert r["name"] == f"{name}.xyz"
        p, g = p2f_fx[f"c{c}_pred"], p2f_fx[f"c{c}_gt"]
        np_, ng = R.normalize(p), R.normalize(g)
        d = ((np_[:, None, :] - ng[None, :, :]) ** 2).sum(-1)
        cd_r, hd_r = d.min(1).mean() + d.min(0).mean(), d.min(1).max() + d.min(0).max()
        emd_r = R.approx_match_cost(np_, ng, 7)
        jsd_r = R.jsd_counts(R.occupancy(np_ * 0.5), R.occupancy(ng * 0.5))
        cgal = p2f_fx[f"c{c}_cgal_dist"]
        diag = float(np.linalg.norm(np.ptp(p2f_fx[f"c{c}_verts"], axis=0)))
        assert abs(_num(r["CD"]) - cd_r) <= 1e-4 * cd_r
        assert abs(_num(r["hausdorff"]) - hd_r) <= 1e-4 * hd_r
        assert abs(_num(r["EMD"]) - emd_r) <= 1e-4 * emd_r
        assert abs(_num(r["JSD"]) - jsd_r) <= 1e-9
        assert abs(_num(r["p2f avg"]) - cgal.mean()) <= 1e-5 * cgal.mean() + 1e-7 * diag
        assert abs(_num(r["p2f std"]) - cgal.std()) <= 1e-5 * cgal.std() + 1e-7 * diag
        assert all(r[f"uniform_{i}"] == "-" for i in range(5))
        # the written P2F file: the binary's x y z columns byte for byte, distances within the bars above
        mine = (pred / f"{name}_point2mesh_distance.xyz").read_text().splitlines()
        ref = bytes(p2f_fx[f"c{c}_cgal_text"]).decode().splitlines()
        assert [ln.rsplit(" ", 1)[0] for ln in mine] == [ln.rsplit(" ", 1)[0] for ln in ref]
        dm = np.array([float(ln.split()[3]) for ln in mine])
        assert np.all(np.abs(dm - cgal) <= 1e-5 * cgal + 1e-7 * diag)
        all_d.append(cgal)
        jsds.append(jsd_r)
        cds.append(cd_r)
    s = dict(zip(rows[0], rows[-1]))
    assert s["name"] == "-" and s["uniform_0"] == "-"
    alld = np.concatenate(all_d)
    assert abs(_num(s["p2f avg"]) - alld.mean()) <= 1e-5 * alld.mean()
    assert abs(_num(s["JSD"]) - np.mean(jsds)) <= 1e-9
    assert abs(_num(s["CD"]) - np.mean(cds)) <= 1e-4 * np.mean(cds)
    assert f"Evaluation: {out}" in printed and "[CD]" in printed and "[p2f avg]" in printed

    # the same directory without --mesh: the P2F files just written are read back (the CGAL binary's output is read the same way)
    out2 = tmp_path / "out2"
    evaluate.main(["--pred", str(pred), "--gt", str(gt), "--save_path", str(out2)])
    with open(out2 / "evaluation.csv") as f:
        rows2 = list(csv.reader(f))
    for a, b in zip(rows[1:], rows2[1:]):
        ra, rb = dict(zip(rows[0], a)), dict(zip(rows[0], b))
        assert ra["CD"] == rb["CD"] and ra["EMD"] == rb["EMD"] and ra["JSD"] == rb["JSD"]
        assert abs(_num(ra["p2f avg"]) - _num(rb["p2f avg"])) <= 1e-5 * _num(ra["p2f avg"])
    capsys.readouterr()

    # no P2F anywhere: no JSD in the rows (evaluate.py:255), '-' in the summary line instead of the reference's KeyError
    for p in pred.glob("*_point2mesh_distance.xyz"):
        p.unlink()
    out3 = tmp_path / "out3"
    evaluate.main(["--pred", str(pred), "--gt", str(gt), "--save_path", str(out3)])
    printed = capsys.readouterr().out
    assert "[p2f avg]-" in printed and "[p2f std]-" in printed
    with open(out3 / "evaluation.csv") as f:
        rows3 = list(csv.reader(f))
    assert all(dict(zip(rows3[0], r))["JSD"] == "-" for r in rows3[1:-1])
    assert dict(zip(rows3[0], rows3[-1]))["JSD"] != "-"
