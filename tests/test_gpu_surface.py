"""Surface-connected neighbourhoods on the GPU (csrc/surface_reach.hip, the reach option of csrc/eval_uniform.hip's disks,
puflow_amd.metrics / sampling / evaluate / prepare) against the float64 restatement (tests/surface_ref.py) and against
identities that need no oracle.  The margins that make exact comparisons fair are asserted in tests/test_surface_ref.py for
the restated seeds and again here for the seeds the GPU drew."""
import csv
import os

import numpy as np
import pytest
import torch

import eval_ref as R
import surface_ref as SR
import uniform_ref as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COLS = ["uniform_%d" % j for j in range(5)]


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _n(t):
    return t.cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ulp_diff(a, b):
    """The distance of two arrays of non-negative float32 in units in the last place (inf only equals inf)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert np.array_equal(np.isinf(a), np.isinf(b))
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()) if a.size else 0


def _rows_of(csr, s):
    off = _n(csr[0])
    return [_n(a)[off[s]:off[s + 1]] for a in csr[1:]]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_uniform.npz"))


@pytest.fixture(scope="module")
def cases(golden_dir):
    return SR.field_cases(golden_dir)


def _gpu_sources(name, v, f, S):
    """The sources of a field case: drawn by metrics.sample_mesh (the strip: the centroid of its first face)."""
    from puflow_amd.metrics import sample_mesh
    ref_s, ref_f = SR.field_sources(name, v, f, S)
    if name == "strip":
        return _t(ref_s), _t(ref_f, np.int64)
    s, face, _ = sample_mesh(_t(v), _t(f, np.int64), S, SR.FIELD_KEY)
    np.testing.assert_array_equal(_n(face), ref_f)
    return s, face


# ---- the field ------------------------------------------------------------------------------------------------------------------
FIELD = [(n, S) for n in ("triangle", "quad", "grid", "u_strip", "sandwich", "icosphere", "sheet") for S in (1, 3, 65)] + [("strip", 1)]


@pytest.mark.parametrize("name,S", FIELD)
def test_field_equals_the_restatement(cases, name, S):
    from puflow_amd.metrics import surface_reach
    v, f, r_stop = cases[name]
    src, face = _gpu_sources(name, v, f, S)
    csr, info = surface_reach(src, face, _t(v), _t(f, np.int64), r_stop, return_info=True)
    assert info["status"] == 0 and csr[2].dtype == torch.float32 and csr[1].dtype == torch.int32
    sweeps = _n(info["sweeps"])
    worst = 0
    for s in range(src.shape[0]):
        p = _n(src[s])
        assert SR.stop_margin(p, v, f, r_stop) > 1e-5
        rf, rd2, rb2 = SR.bottleneck(p, int(face[s]), v, f, r_stop)
        g_rf, g_rb2 = _rows_of(csr, s)
        g_rd2 = _n(info["rd2"])[_n(csr[0])[s]:_n(csr[0])[s + 1]]
        np.testing.assert_array_equal(g_rf, rf)
        worst = max(worst, _ulp_diff(g_rd2, rd2), _ulp_diff(g_rb2, rb2))
        assert 2 <= sweeps[s] <= len(rf) + 1 or len(rf) == 1
    print(f"{name} S={S}: worst difference {worst} ulp, sweeps min/median/max {sweeps.min()}/{int(np.median(sweeps))}/{sweeps.max()}")
    assert worst <= 4
    if name == "sandwich":
        assert bool(torch.isinf(csr[2]).any())                     # the other sheet is a candidate and is not reached


def _lds_mesh(extra: bool):
    from puflow_amd import _lib
    n = _lib.load().pf_reach_lds_faces()
    assert n % 128 == 0
    v, f = SR.grid(64, n // 128, 64.0, float(n // 128))
    if extra:                                                      # one more face, hung on the first boundary edge
        v = np.concatenate([v, np.array([[-1.0, 0.5, 0.0]], np.float32)])
        f = np.concatenate([f, np.array([[0, len(v) - 1, 1]])])
    return v, f, n


def test_rows_at_the_lds_limit_and_one_beyond():
    from puflow_amd.metrics import surface_reach
    rows = []
    for extra in (False, True):
        v, f, n = _lds_mesh(extra)
        src = np.stack([v[f[5]].astype(np.float64).mean(0), v[f[n - 3]].astype(np.float64).mean(0)]).astype(np.float32)
        face = np.array([5, n - 3])
        csr, info = surface_reach(_t(src), _t(face, np.int64), _t(v), _t(f, np.int64), 1000.0, return_info=True)
        assert info["status"] == 0 and _n(csr[0]).tolist() == [0, len(f), 2 * len(f)]
        for s in range(2):
            rf, rd2, rb2 = SR.bottleneck(src[s], int(face[s]), v, f, 1000.0)
            g_rf, g_rb2 = _rows_of(csr, s)
            np.testing.assert_array_equal(g_rf, rf)
            assert _ulp_diff(g_rb2, rb2) <= 4 and np.all(np.isfinite(g_rb2))
        rows.append([_rows_of(csr, s)[1][:n] for s in range(2)])
        print("faces", len(f), "sweeps", _n(info["sweeps"]).tolist())
    for a, b in zip(*rows):                                        # LDS and global rows: the same bits on the shared faces
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))


def test_a_source_does_not_depend_on_its_batch_the_call_or_the_stop(cases):
    from puflow_amd.metrics import surface_reach
    for name in ("u_strip", "sheet"):
        v, f, r_stop = cases[name]
        vt, ft = _t(v), _t(f, np.int64)
        src, face = _gpu_sources(name, v, f, 65)
        full = surface_reach(src, face, vt, ft, r_stop)
        again = surface_reach(src, face, vt, ft, r_stop)
        assert all(torch.equal(a, b) for a, b in zip(full[:2], again[:2])) and torch.equal(_bits(full[2]), _bits(again[2]))
        half = surface_reach(src, face, vt, ft, 0.5 * r_stop)
        small = np.float32((0.5 * r_stop) ** 2)
        for s in (0, 17, 64):
            alone = surface_reach(src[s:s + 1], face[s:s + 1], vt, ft, r_stop)
            for a, b in zip(_rows_of(full, s), _rows_of(alone, 0)):
                np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
            rf, rb2 = _rows_of(full, s)
            hf, hb2 = _rows_of(half, s)
            keep = rb2 <= small
            assert set(rf[keep]) <= set(hf)
            np.testing.assert_array_equal(hb2[np.isin(hf, rf[keep])].view(np.int32), rb2[keep].view(np.int32))
            assert np.all(np.isinf(hb2[~np.isin(hf, rf[keep])]))


def test_status_and_argument_errors(cases):
    from puflow_amd import _lib
    from puflow_amd.metrics import REACH_ST_START, surface_reach
    lib = _lib.load()
    v, f, _ = cases["grid"]
    src = v[f[0]].mean(0)[None]
    for wrong in (127, len(f) + 5, -1):                            # far from the source; outside the mesh
        csr, info = surface_reach(_t(src), _t([wrong], np.int64), _t(v), _t(f, np.int64), 0.2, return_info=True)
        assert info["status"] == REACH_ST_START and _n(csr[0]).tolist() == [0, 0] and csr[1].numel() == 0
    both = surface_reach(_t(np.concatenate([src, src])), _t([0, 127], np.int64), _t(v), _t(f, np.int64), 0.2)
    assert _n(both[0])[1] == _n(both[0])[2] > 0                    # the good source keeps its row
    assert lib.pf_reach_count(None, 1, None, None, None, 1, None, None, None) == -1
    assert lib.pf_reach_count(8, 0, 8, 8, 8, 1, 8, 8, None) == -2 and lib.pf_reach_fill(8, 4, 8, 8, 8, 0, 8, 8, 8, 8, None) == -2
    assert lib.pf_reach_relax(8, 8, 8, 4, 8, None, 8, 1, 8, None, 8, None) == -1
    assert lib.pf_reach_point_d2(8, 0, 8, 8, 1, 8, 8, 8, 8, None) == -2
    assert lib.pf_disk_count_reach(8, 4, 8, 1, None, 1, 8, 8, 8, 8, 8, None) == -1
    with pytest.raises(_lib.PuflowHipError):
        surface_reach(torch.zeros(1, 3), torch.zeros(1, dtype=torch.long), torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.long), 1.0)


def test_adjacency_welds_and_matches_the_definition(cases):
    from puflow_amd.metrics import face_adjacency
    v, f, _ = cases["u_strip"]
    off, adj = (_n(a) for a in face_adjacency(_t(v), _t(f, np.int64)))
    wf = SR.weld(v, f)
    want = [sorted(g for g in range(len(f)) if g != i and set(wf[i]) & set(wf[g])) for i in range(len(f))]
    assert [adj[off[i]:off[i + 1]].tolist() for i in range(len(f))] == want
    uv, uf = SR.unwelded(v, f)
    off2, adj2 = (_n(a) for a in face_adjacency(_t(uv), _t(uf, np.int64)))
    np.testing.assert_array_equal(off, off2)
    np.testing.assert_array_equal(adj, adj2)


# ---- disks ------------------------------------------------------------------------------------------------------------------------
def _disk_case(v, f):
    from puflow_amd.metrics import mesh_area_radii, sample_mesh
    vt, ft = _t(v), _t(f, np.int64)
    mapped, mf, _ = sample_mesh(vt, ft, SR.DISK_POINTS, SR.DISK_KEY + 50)
    seeds, sf, _ = sample_mesh(vt, ft, SR.DISK_SEEDS, SR.DISK_KEY)
    return vt, ft, mapped, mf, seeds, sf, mesh_area_radii(v, f)[0]


def test_surface_disks_on_a_flat_grid_are_the_balls():
    from puflow_amd.metrics import disks, surface_reach
    v, f = SR.grid(8, 8)
    vt, ft, mapped, mf, seeds, sf, radii = _disk_case(v, f)
    assert SR.radius_margin(U.seed_distances(_n(mapped), _n(seeds)), radii) > 1e-5
    reach = surface_reach(seeds, sf, vt, ft, radii[-1])
    c0, csr0 = disks(mapped, seeds, radii)
    c1, csr1 = disks(mapped, seeds, radii, reach=reach, mapped_face=mf)
    assert torch.equal(c0, c1) and all(torch.equal(a, b) for a, b in zip(csr0, csr1)) and int(c0[:, -1].min()) > 0


def test_surface_disks_on_the_sandwich_are_the_balls_of_one_sheet():
    from puflow_amd.metrics import disks, surface_reach
    v, f = SR.sandwich(SR.GAP)
    vt, ft, mapped, mf, seeds, sf, radii = _disk_case(v, f)
    assert SR.GAP < radii[0] and SR.radius_margin(U.seed_distances(_n(mapped), _n(seeds)), radii) > 1e-5
    reach = surface_reach(seeds, sf, vt, ft, radii[-1])
    counts, csr = disks(mapped, seeds, radii, reach=reach, mapped_face=mf)
    ball_counts, _ = disks(mapped, seeds, radii)
    assert int(ball_counts.sum()) > int(counts.sum())              # the balls do take in the other sheet
    for sheet in (0, 1):
        pts = torch.nonzero(torch.from_numpy(SR.sheet_of("sandwich", _n(mf)) == sheet).to(DEV))[:, 0]
        sel = torch.nonzero(torch.from_numpy(SR.sheet_of("sandwich", _n(sf)) == sheet).to(DEV))[:, 0]
        assert len(sel) > 2
        c_sub, (o_sub, m_sub, l_sub) = disks(mapped[pts], seeds[sel], radii)
        assert torch.equal(c_sub, counts[sel])
        for k, s in enumerate(_n(sel)):
            mem, lev = _rows_of(csr, s)
            np.testing.assert_array_equal(mem, _n(pts)[_n(m_sub)[_n(o_sub)[k]:_n(o_sub)[k + 1]]])
            np.testing.assert_array_equal(lev, _n(l_sub)[_n(o_sub)[k]:_n(o_sub)[k + 1]])


def test_surface_disks_of_the_folded_sheet_equal_the_restatement(fx):
    from puflow_amd.metrics import disks, point_to_mesh_distance, surface_reach, uniformity
    v, f = fx["c2_verts"], fx["c2_faces"].astype(np.int64)
    S, radii = SR.SHEET_SEEDS, fx["c2_radii"]
    vt, ft, mapped = _t(v), _t(f, np.int64), _t(fx["c2_mapped"])
    seeds = _t(fx["c2_seeds"][:S])
    sf = U.seeds_from_uniforms(v, f, fx["uniforms"])[1][:S]
    _, mf = point_to_mesh_distance(_t(fx["c2_cloud"]), vt, ft, return_face=True)      # the faces of the P2F search
    reach = surface_reach(seeds, _t(sf, np.int64), vt, ft, radii[-1])
    counts, csr = disks(mapped, seeds, radii, reach=reach, mapped_face=mf)
    rc, ro, rm, rl, D = SR.disks(fx["c2_mapped"], _n(mf), fx["c2_seeds"][:S], sf, v, f, radii)
    assert SR.radius_margin(D, radii) > 1e-5
    np.testing.assert_array_equal(_n(counts), rc)
    for a, b in zip(csr, (ro, rm, rl)):
        np.testing.assert_array_equal(_n(a), b)
    u = uniformity(mapped, csr, radii)
    ur = uniformity(mapped, (_t(ro, np.int64), _t(rm, np.int32), _t(rl, np.int32)), radii)
    np.testing.assert_allclose(u, ur, rtol=1e-6)
    ball = fx["c2_counts"][:S].astype(np.int64)
    assert np.all(rc <= ball) and rc[:, -1].sum() < ball[:, -1].sum()
    print("folded sheet, surface / ball members per radius:", np.round(rc.sum(0) / ball.sum(0), 4))


# ---- patches ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["sandwich", "u_strip"])
def test_patch_pools_are_cropped_along_the_surface(mesh):
    from puflow_amd import metrics, sampling
    v, f = SR.sandwich() if mesh == "sandwich" else SR.u_strip()
    vt, ft = _t(v), _t(f, np.int64)
    P, key = SR.PATCH, 3
    kw = dict(n_patches=P["n_patches"], num_point=P["num_point"], up_ratio=P["up_ratio"], cloud_points=P["cloud_points"], seed=key,
              ratio=P["ratio"], return_pools=True)
    out, pools = sampling.make_patches(vt, ft, metric="surface", **kw)
    ball_out, ball = sampling.make_patches(vt, ft, metric="ball", **kw)
    plain = sampling.make_patches(vt, ft, P["n_patches"], P["num_point"], P["up_ratio"], P["cloud_points"], key, P["ratio"])
    assert all(torch.equal(plain[k], ball_out[k]) for k in plain) and sorted(plain) == sorted(out)      # "ball" is today's call
    assert out["poisson_16"].shape == (4, 16, 3) and out["poisson_64"].shape == (4, 64, 3)
    assert torch.equal(pools["seeds"], ball["seeds"])
    seeds, sf = _n(pools["seeds"]), _n(pools["seed_face"])
    stray_ball = checked = 0
    for which, n_out, n_set, sd in (("input", 16, 320, key + 2), ("gt", 64, 1280, key + 1)):
        samples, face, _ = metrics.sample_mesh(vt, ft, n_set, sd)
        samples, face = _n(samples), _n(face)
        for p in range(P["n_patches"]):
            idx, d, fd2 = SR.patch_pool(samples, face, seeds[p], int(sf[p]), v, f, P["ratio"] * n_out)
            assert SR.pool_margin(d, P["ratio"] * n_out, fd2) > 1e-6
            got = _n(pools[which + "_idx"][p])
            np.testing.assert_array_equal(np.sort(got), np.sort(idx))
            assert SR.order_defects(got, d) == 0                   # nearest first, by (D2, index)
            np.testing.assert_array_equal(_n(pools[which + "_pool"][p]), samples[got])
            near = mesh == "sandwich" or seeds[p][0] <= 1.0      # U strip: a seed in the half away from the bend
            side, own = SR.sheet_of(mesh, face[got]), SR.sheet_of(mesh, sf[p])
            if near:
                checked += 1
                assert np.all(side == own), (which, p)
                stray_ball += int((SR.sheet_of(mesh, face[_n(ball[which + "_idx"][p])]) != own).sum())
    assert checked >= 2 and stray_ball > 0                         # seeds were checked; the Euclidean crop takes in the other side


@pytest.mark.parametrize("mesh", ["sandwich", "u_strip"])
def test_surface_pool_grows_until_its_last_place_is_inside_the_stop(mesh):
    """Seeds whose k-th place lies beyond the first r_stop (tests/test_surface_ref.py asserts that premise, and that the
    first k finite values inside that stop would be other samples): the pool is the whole mesh's selection, in its order."""
    from puflow_amd import sampling
    v, f, q, qf, seeds, sf = SR.pool_case(mesh)
    idx = _n(sampling.surface_pool(_t(q), _t(qf, np.int64), _t(seeds), _t(sf, np.int64), _t(v), _t(f, np.int64), SR.POOL_K))
    for p in range(len(seeds)):
        want, d, fd2 = SR.patch_pool(q, qf, seeds[p], int(sf[p]), v, f, SR.POOL_K)
        assert SR.pool_margin(d, SR.POOL_K, fd2) > 1e-6
        np.testing.assert_array_equal(np.sort(idx[p]), np.sort(want))
        assert SR.order_defects(idx[p], d) == 0


def test_a_component_too_small_for_its_pool_is_named():
    from puflow_amd import _lib, sampling
    v, f = SR.small_component()
    P = SR.PATCH
    with pytest.raises(_lib.PuflowHipError, match="component of the mesh too small"):
        sampling.make_patches(_t(v), _t(f, np.int64), P["n_patches"], P["num_point"], P["up_ratio"], P["cloud_points"], 3, P["ratio"],
                              metric="surface")
    with pytest.raises(ValueError):
        sampling.make_patches(_t(v), _t(f, np.int64), 2, metric="geodesic")


# ---- command lines ------------------------------------------------------------------------------------------------------------------
def _rows(path):
    with open(path) as fh:
        rows = list(csv.reader(fh))
    return [dict(zip(rows[0], r)) for r in rows[1:]]


def test_evaluate_surface_disks_round_trip_and_ball_default(tmp_path, fx, capsys):
    from puflow_amd import evaluate
    pred, gt, mesh = tmp_path / "pred", tmp_path / "gt", tmp_path / "mesh"
    for d in (pred, gt, mesh):
        d.mkdir()
    for c in range(int(fx["ncases"])):
        name = bytes(fx[f"c{c}_name"]).decode()
        R.write_points(pred / f"{name}.xyz", fx[f"c{c}_cloud"])
        R.write_points(gt / f"{name}.xyz", fx[f"c{c}_cloud"][::-1])
        R.write_off(mesh / f"{name}.off", fx[f"c{c}_verts"], fx[f"c{c}_faces"].astype(np.int64))
    base = ["--pred", str(pred), "--gt", str(gt), "--uniform", "--uniform_seeds", "200"]
    evaluate.main(base + ["--save_path", str(tmp_path / "plain"), "--mesh", str(mesh)])
    evaluate.main(base + ["--save_path", str(tmp_path / "ball"), "--mesh", str(mesh), "--uniform_disks", "ball"])
    assert (tmp_path / "plain" / "evaluation.csv").read_bytes() == (tmp_path / "ball" / "evaluation.csv").read_bytes()
    evaluate.main(base + ["--save_path", str(tmp_path / "s1"), "--mesh", str(mesh), "--write_p2m", "--uniform_disks", "surface",
                          "--write_disks"])
    evaluate.main(base + ["--save_path", str(tmp_path / "s2")])                    # the files read back, without the mesh
    capsys.readouterr()
    r0, r1, r2 = (_rows(tmp_path / d / "evaluation.csv") for d in ("plain", "s1", "s2"))
    differs = False
    for a, b, c in zip(r0, r1, r2):
        ub, uc = (np.array([float(r[k]) for k in COLS]) for r in (b, c))
        assert np.all(np.isfinite(ub)) and np.all(np.abs(ub - uc) <= 1e-5 * np.abs(ub)), (ub, uc)
        assert {k: x for k, x in a.items() if k not in COLS} == {k: x for k, x in b.items() if k not in COLS}
        differs |= any(a[k] != b[k] for k in COLS)
    assert differs                                                 # the folded sheet's columns change


def test_prepare_patch_metric_surface(tmp_path, capsys):
    from puflow_amd import prepare
    (tmp_path / "mesh").mkdir()
    R.write_off(tmp_path / "mesh" / "u.off", *SR.u_strip())
    prepare.main(["--mesh", str(tmp_path / "mesh"), "--out", str(tmp_path / "out"), "--patches", "2", "--num_point", "16",
                  "--up_ratio", "4", "--cloud_points", "64", "--patch_metric", "surface"])
    capsys.readouterr()
    z = np.load(tmp_path / "out" / "patches.npz")
    assert z["poisson_16"].shape == (2, 16, 3) and z["poisson_64"].shape == (2, 64, 3) and np.isfinite(z["poisson_64"]).all()
