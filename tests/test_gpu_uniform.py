"""The uniformity columns on the GPU (csrc/eval_uniform.hip, puflow_amd.metrics, python -m puflow_amd.evaluate --uniform)
against the reference's analyze_uniform (tests/golden/eval_uniform.npz) and the float64 restatement (tests/uniform_ref.py)."""
import csv
import os

import numpy as np
import pytest
import torch

import eval_ref as R
import uniform_ref as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COLS = ["uniform_%d" % j for j in range(5)]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_uniform.npz"))


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _csr(fx, c):
    return fx[f"c{c}_offsets"].astype(np.int64), fx[f"c{c}_member"].astype(np.int64), fx[f"c{c}_level"].astype(np.int64)


def _csr_t(csr):
    return _t(csr[0], np.int64), _t(csr[1], np.int32), _t(csr[2], np.int32)


def _mesh(fx, c):
    return fx[f"c{c}_verts"], fx[f"c{c}_faces"].astype(np.int64)


def _diag(v):
    return float(np.linalg.norm(np.ptp(v, axis=0)))


def _rows(path):
    with open(path) as f:
        rows = list(csv.reader(f))
    return [dict(zip(rows[0], r)) for r in rows[1:]]


def _write_clouds(tmp_path, fx, with_mesh):
    """pred / gt (/ mesh) directories of the golden cases; -> (pred, gt, mesh, [name])."""
    from puflow_amd import evaluate
    pred, gt, mesh = tmp_path / "pred", tmp_path / "gt", tmp_path / "mesh"
    names = []
    for d in (pred, gt, mesh):
        d.mkdir()
    for c in range(int(fx["ncases"])):
        name = bytes(fx[f"c{c}_name"]).decode()
        cloud = fx[f"c{c}_cloud"]
        R.write_points(pred / f"{name}.xyz", cloud)
        R.write_points(gt / f"{name}.xyz", cloud[::-1])
        if with_mesh:
            R.write_off(mesh / f"{name}.off", *_mesh(fx, c))
        else:                                     # the files of a run that made disks elsewhere
            from puflow_amd.metrics import write_disk_files
            dist = np.linalg.norm(cloud.astype(np.float64) - fx[f"c{c}_mapped"], axis=1).astype(np.float32)
            (pred / f"{name}_point2mesh_distance.xyz").write_text(evaluate.format_p2m(cloud.astype(np.float64), dist))
            write_disk_files(str(pred / name), cloud, dist, fx[f"c{c}_mapped"], _csr(fx, c), fx[f"c{c}_radii"])
        names.append(name)
    return pred, gt, mesh, sorted(names)


def test_cli_reads_disk_files_and_matches_reference(tmp_path, fx, capsys):
    from puflow_amd import evaluate
    pred, gt, _, names = _write_clouds(tmp_path, fx, with_mesh=False)
    out = tmp_path / "out"
    evaluate.main(["--pred", str(pred), "--gt", str(gt), "--save_path", str(out), "--uniform"])
    capsys.readouterr()
    rows = _rows(out / "evaluation.csv")
    by_name = {bytes(fx[f"c{c}_name"]).decode(): c for c in range(int(fx["ncases"]))}
    got = []
    for name, r in zip(names, rows[:-1]):
        assert r["name"] == f"{name}.xyz"
        ref = fx[f"c{by_name[name]}_uniform"]
        u = np.array([float(r[k]) for k in COLS])
        print(name, "rel", np.abs(u / ref - 1))
        assert np.all(np.abs(u - ref) <= 1e-4 * np.abs(ref)), (name, u, ref)
        got.append(u)
    s = np.array([float(rows[-1][k]) for k in COLS])                       # evaluate.py:283-287: the mean over the files
    np.testing.assert_allclose(s, np.mean(got, axis=0), rtol=1e-12)


def test_disks_equal_the_fixture_exactly(fx):
    from puflow_amd.metrics import disks
    for c in range(int(fx["ncases"])):
        counts, (off, mem, lev) = disks(_t(fx[f"c{c}_mapped"]), _t(fx[f"c{c}_seeds"]), fx[f"c{c}_radii"])
        o, m, l = _csr(fx, c)
        assert counts.dtype == torch.int32 and mem.dtype == torch.int32
        np.testing.assert_array_equal(counts.cpu().numpy(), fx[f"c{c}_counts"])
        np.testing.assert_array_equal(off.cpu().numpy(), o)
        np.testing.assert_array_equal(mem.cpu().numpy(), m)
        np.testing.assert_array_equal(lev.cpu().numpy(), l)


def test_mapped_points_are_the_closest_points(fx):
    from puflow_amd.metrics import mapped_points, point_to_mesh_distance
    for c in range(int(fx["ncases"])):
        v, f = _mesh(fx, c)
        cloud = fx[f"c{c}_cloud"]
        args = (_t(cloud), _t(v), _t(f, np.int64))
        q = mapped_points(*args).cpu().numpy().astype(np.float64)
        diag = _diag(v)
        assert np.abs(q - fx[f"c{c}_mapped"]).max() <= 1e-6 * diag, c
        d = point_to_mesh_distance(*args).cpu().numpy().astype(np.float64)
        assert np.abs(np.linalg.norm(q - cloud, axis=1) - d).max() <= 1e-6 * diag, c
    # a degenerate mesh (zero-area faces, slivers) and points off the surface, against the restatement
    v, f = R.sheet(degenerate=True)
    v = v.astype(np.float32)
    rng = np.random.default_rng(4)
    p = np.concatenate([rng.uniform(-1, 1, (150, 3)) * [1.2, 0.8, 0.8], v[-6:] + rng.normal(0, 1e-2, (6, 3))]).astype(np.float32)
    q = mapped_points(_t(p), _t(v), _t(f, np.int64)).cpu().numpy().astype(np.float64)
    ref, _, dref = U.closest_points(p, v, f)
    assert np.abs(np.linalg.norm(q - p, axis=1) - dref).max() <= 1e-6 * _diag(v)
    assert np.abs(q - ref).max() <= 1e-6 * _diag(v)


def test_seeds(fx):
    from puflow_amd.metrics import sample_mesh
    uni_ref = fx["uniforms"]
    S = len(uni_ref)
    for c in range(int(fx["ncases"])):
        v, f = _mesh(fx, c)
        vt, ft = _t(v), _t(f, np.int64)
        seeds, face, uni = sample_mesh(vt, ft, S, int(fx["seed"]))
        np.testing.assert_array_equal(uni.cpu().numpy(), uni_ref)                    # Philox and the word-to-uniform mapping
        u = uni.cpu().numpy()
        _, cum = U.area_radii(v, f)
        near = np.abs(u[:, :1].astype(np.float64) - (cum / cum[-1])[None, :]).min(1) <= 1e-7
        assert near.sum() == 0
        ref, fref = U.seeds_from_uniforms(v, f, u)
        np.testing.assert_array_equal(face.cpu().numpy(), fref)
        assert np.abs(seeds.cpu().numpy().astype(np.float64) - ref).max() <= 1e-6 * _diag(v)
        again = sample_mesh(vt, ft, S, int(fx["seed"]))
        assert all(torch.equal(a, b) for a, b in zip((seeds, face, uni), again))
        few = sample_mesh(vt, ft, 10, int(fx["seed"]))
        assert torch.equal(few[0], seeds[:10]) and torch.equal(few[1], face[:10]) and torch.equal(few[2], uni[:10])
        other = sample_mesh(vt, ft, 10, int(fx["seed"]) + 1)
        assert not torch.equal(other[2], uni[:10])
    # the seeds follow the area: a mesh of two triangles, one with 3/4 of the area
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 3, 0], [2, 0, 0]], np.float32)
    f = np.array([[0, 1, 2], [1, 4, 3]], np.int64)
    _, face, _ = sample_mesh(_t(v), _t(f, np.int64), 4000, 3)
    share = float((face == 1).float().mean())
    a1 = 0.5 * np.linalg.norm(np.cross(v[4] - v[1], v[3] - v[1]))
    p1 = a1 / (a1 + 0.5)
    assert abs(share - p1) < 4 * np.sqrt(p1 * (1 - p1) / 4000)                       # four standard deviations of the count


def _random_case(rng, N, S, J):
    """Points in a slab, seeds among them, radii with several members per disk; no point within 1e-5 r of a radius."""
    pts = (rng.random((N, 3)) * [1.0, 1.0, 0.05]).astype(np.float32)
    seeds = pts[rng.choice(N, S, replace=False)] + np.float32(1e-3)
    radii = np.array([0.18, 0.22, 0.27, 0.31, 0.36])[:J] if J > 1 else np.array([0.3])
    d = U.seed_distances(pts, seeds)
    assert (np.abs(d[:, :, None] - radii) > 1e-5 * radii).all()
    return pts, seeds, radii


def _check_statistics(pts, csr, radii, percentages=None, rtol=1e-5):
    from puflow_amd.metrics import disk_statistics, uniformity
    n, dis = disk_statistics(_t(pts), _csr_t(csr), radii)
    nr, dr = U.disk_statistics(pts, csr, radii)
    np.testing.assert_array_equal(n.cpu().numpy(), nr)
    np.testing.assert_allclose(dis.cpu().numpy(), dr, rtol=rtol, atol=0, equal_nan=True)
    u = uniformity(_t(pts), _csr_t(csr), radii, percentages)
    np.testing.assert_allclose(u, U.uniformity(pts, csr, radii, percentages), rtol=rtol, atol=0, equal_nan=True)
    return n.cpu().numpy(), u


@pytest.mark.parametrize("J", [1, 5])
def test_small_cloud_matches_restatement(J):
    from puflow_amd.metrics import disks
    pts, seeds, radii = _random_case(np.random.default_rng(10 + J), 70, 3, J)
    counts, csr = disks(_t(pts), _t(seeds), radii)
    cr, o, m, l = U.disks(pts, seeds, radii)
    np.testing.assert_array_equal(counts.cpu().numpy(), cr)
    for a, b in zip(csr, (o, m, l)):
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    n, u = _check_statistics(pts, (o, m, l), radii, U.PERCENTAGES[:J] * 10)
    assert (n >= 5).any() and np.isfinite(u).any()


def test_disks_of_0_1_4_and_5_members():
    rng = np.random.default_rng(2)
    pts = rng.random((40, 3)).astype(np.float32)
    sizes = [0, 1, 4, 5, 0, 9]
    member = np.concatenate([rng.choice(40, k, replace=False) for k in sizes]).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    level = np.zeros(len(member), np.int64)                                      # every member in every disk
    radii = np.array([0.4, 0.5])
    n, u = _check_statistics(pts, (offsets, member, level), radii, [0.1, 0.1])
    np.testing.assert_array_equal(n[:, 0], sizes)
    # only the disks of 5 and 9 members count: the 4-member disk is left out, not counted as zero
    nr, dr = U.disk_statistics(pts, (offsets, member, level), radii)
    keep = np.array(sizes) >= 5
    want = np.mean(((nr[keep, 0] - 4.0) ** 2 / 4.0 * dr[keep, 0]).astype(np.float32))
    np.testing.assert_allclose(u[0], want, rtol=1e-5)
    # levels: member k of the last row enters at disk k % 2
    level[offsets[5]:] = np.arange(9) % 2
    _check_statistics(pts, (offsets, member, level), radii, [0.1, 0.1])


def test_duplicated_points_give_distance_zero():
    from puflow_amd.metrics import disk_statistics
    rng = np.random.default_rng(5)
    half = rng.random((12, 3)).astype(np.float32)
    pts = np.concatenate([half, half])
    csr = (np.array([0, 24], np.int64), np.arange(24, dtype=np.int64), np.zeros(24, np.int64))
    radii = np.array([0.7])
    n, dis = disk_statistics(_t(pts), _csr_t(csr), radii)
    e = np.sqrt(2 * (np.pi * 0.7 ** 2 / 24) / 1.732)
    np.testing.assert_allclose(dis.cpu().numpy(), [[e]], rtol=1e-12)             # every d is 0: the mean of e^2 / e
    _check_statistics(pts, csr, radii, [0.5])


def test_a_disk_larger_than_the_lds_tile():
    """One disk holds every point, a second row lists them in another split of levels: N just above the tile, so the kernel
    stages the row in more than one tile and a member's own entry lies in a tile it has to find."""
    from puflow_amd import _lib
    tile = _lib.load().pf_disk_tile()
    N = tile + 7
    rng = np.random.default_rng(8)
    pts = rng.random((N, 3)).astype(np.float32)
    pts[N - 1] = pts[3]                                                        # a duplicate across the tile boundary
    member = np.concatenate([np.arange(N), np.arange(N)]).astype(np.int64)
    level = np.concatenate([np.zeros(N), np.arange(N) % 3]).astype(np.int64)
    offsets = np.array([0, N, 2 * N], np.int64)
    n, _ = _check_statistics(pts, (offsets, member, level), np.array([1.0, 1.5, 2.0]), [0.5, 0.8, 1.0])
    assert n[0, 0] == N and n[1, 2] == N and n[1, 0] == (N + 2) // 3


def test_statistics_are_deterministic_and_independent_of_the_batch(fx):
    from puflow_amd.metrics import disk_statistics
    c = 1
    mapped, radii = _t(fx[f"c{c}_mapped"]), fx[f"c{c}_radii"]
    o, m, l = _csr(fx, c)
    full = disk_statistics(mapped, _csr_t((o, m, l)), radii)
    again = disk_statistics(mapped, _csr_t((o, m, l)), radii)
    assert torch.equal(full[0], again[0]) and torch.equal(full[1].view(torch.int64), again[1].view(torch.int64))
    h = 437                                                                    # the seeds split over two calls
    a = disk_statistics(mapped, _csr_t((o[:h + 1], m[:o[h]], l[:o[h]])), radii)
    b = disk_statistics(mapped, _csr_t((o[h:] - o[h], m[o[h]:], l[o[h]:])), radii)
    for k in range(2):
        both = torch.cat([a[k], b[k]])
        assert torch.equal(both.view(torch.int64), full[k].view(torch.int64))


def test_cli_makes_disks_writes_them_and_reads_them_back(tmp_path, fx, capsys):
    from puflow_amd import evaluate
    pred, gt, mesh, names = _write_clouds(tmp_path, fx, with_mesh=True)
    base = ["--pred", str(pred), "--gt", str(gt)]
    evaluate.main(base + ["--save_path", str(tmp_path / "o1"), "--mesh", str(mesh), "--write_p2m", "--uniform", "--write_disks",
                          "--uniform_seeds", "300"])
    r1 = _rows(tmp_path / "o1" / "evaluation.csv")
    for name, r in zip(names, r1):
        u = np.array([float(r[k]) for k in COLS])
        assert np.all(np.isfinite(u)) and np.all(u > 0), (name, u)
        for tail in ("_disk_idx.txt", "_radius.txt", "_point2mesh_distance.txt"):
            assert (pred / (name + tail)).is_file()
        assert len((pred / (name + "_disk_idx.txt")).read_text().splitlines()) == 300 * 5
    assert all(np.isfinite(float(r1[-1][k])) for k in COLS)
    # the files read back, without the mesh
    evaluate.main(base + ["--save_path", str(tmp_path / "o2"), "--uniform"])
    r2 = _rows(tmp_path / "o2" / "evaluation.csv")
    for a, b in zip(r1, r2):
        ua, ub = np.array([float(a[k]) for k in COLS]), np.array([float(b[k]) for k in COLS])
        assert np.all(np.abs(ua - ub) <= 1e-5 * np.abs(ua)), (ua, ub)
    # without --uniform: `-`, and every other column as in the first run
    evaluate.main(base + ["--save_path", str(tmp_path / "o3"), "--mesh", str(mesh)])
    r3 = _rows(tmp_path / "o3" / "evaluation.csv")
    assert len(r3) == len(r1)
    for a, b in zip(r1, r3):
        assert all(b[k] == "-" for k in COLS)
        assert {k: v for k, v in a.items() if k not in COLS} == {k: v for k, v in b.items() if k not in COLS}
    capsys.readouterr()


def test_cli_writes_nan_when_every_disk_is_below_five_members(tmp_path, fx, capsys):
    from puflow_amd import evaluate
    v, f = _mesh(fx, 0)
    rng = np.random.default_rng(6)
    for d in ("pred", "gt", "mesh"):
        (tmp_path / d).mkdir()
    cloud = R.sample_surface(v, f, 48, rng).astype(np.float32)                   # 1.2 % of 48 points: 0.6 expected per disk
    R.write_points(tmp_path / "pred" / "a.xyz", cloud)
    R.write_points(tmp_path / "gt" / "a.xyz", cloud[::-1])
    R.write_off(tmp_path / "mesh" / "a.off", v, f)
    evaluate.main(["--pred", str(tmp_path / "pred"), "--gt", str(tmp_path / "gt"), "--save_path", str(tmp_path / "out"),
                   "--mesh", str(tmp_path / "mesh"), "--uniform", "--uniform_seeds", "64"])
    capsys.readouterr()
    mapped = U.closest_points(cloud, v, f)[0]
    seeds = U.seeds_from_uniforms(v, f, U.uniforms(0, 64))[0]
    assert U.disks(mapped, seeds, U.area_radii(v, f)[0])[0].max() < 5             # the premise, by the restatement
    rows = _rows(tmp_path / "out" / "evaluation.csv")
    assert all(rows[0][k] == "nan" for k in COLS) and all(rows[-1][k] == "nan" for k in COLS)
