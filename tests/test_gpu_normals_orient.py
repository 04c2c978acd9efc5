"""pf_normals_orient on the device against its numpy restatement (orient_ref), bit for bit.  The restatement is always fed the
DEVICE's own normals (pf_normals_pca, or constructed ones) and neighbour lists, so everything from there is exact: normal_out and
comp must be torch.equal to it.  On the closed test surfaces no row may then be opposed to the analytic normal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attr_ref as R
import orient_ref as O
from puflow_amd.weights import synth_state_dict

DEV = "cuda:0"
F = np.float32


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _lists(pts, k, search="brute"):
    from puflow_amd import ops
    p = _dev(pts)[None]
    return (ops.knn_grid if search == "grid" else ops.knn_large)(p, p, k)[0][0]


def _pca(pts, idx):
    from puflow_amd import ops
    return ops.normals_pca(_dev(pts)[None], idx[None])[0][0].cpu().numpy()


def _orient(pts, normal, idx, viewpoint=None):
    from puflow_amd import ops
    out, comp = ops.normals_orient(_dev(pts)[None], _dev(normal)[None], idx[None], viewpoint)
    return out[0], comp[0]


def _check(pts, normal, idx, viewpoint=None):
    """the device against the restatement on these very inputs; returns the device's output on the host"""
    out, comp = _orient(pts, normal, idx, viewpoint)
    want, wcomp = O.orient(pts, normal, idx.cpu().numpy(), viewpoint)
    assert torch.equal(comp.cpu(), torch.from_numpy(wcomp))
    assert torch.equal(out.cpu().view(torch.int32), torch.from_numpy(want.view(np.int32)))
    return out.cpu().numpy(), comp.cpu().numpy()


SURFACE_CASES = [("torus", n, k, sigma) for n in (512, 2048) for k in (8, 16) for sigma in (0.0, 0.002)] + \
                [("beside", 1024, 16, 0.0), ("nested", 1024, 16, 0.0)]


@pytest.mark.parametrize("search", ["brute", "grid"])
@pytest.mark.parametrize("name,n,k,sigma", SURFACE_CASES)
def test_tori_and_spheres(name, n, k, sigma, search):
    pts, analytic = R.torus(n, 12, sigma) if name == "torus" else O.two_spheres(name == "nested")
    idx = _lists(pts, k, search)
    normal = O.scramble(_pca(pts, idx), n + k)
    out, comp = _check(pts, normal, idx)
    assert np.array_equal(np.abs(out), np.abs(normal))
    if name == "torus":
        assert (comp == 0).all()
    else:
        assert (comp[:600] == 0).all() and (comp[600:] == 600).all()
    # the method on these bits: a finding if it ever fails while the comparison above holds
    assert O.opposed(out, analytic) == 0


def test_planar_grid_all_weights_zero():
    """constructed normals (0, 0, +-1): every weight is exactly 0, the indices alone decide the forest"""
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), indexing="ij"), axis=-1).reshape(-1, 2)
    pts = np.concatenate([g, np.zeros((256, 1))], axis=1).astype(F)
    normal = O.scramble(np.tile(np.array([0, 0, 1], F), (256, 1)), 5)
    for k in (5, 9):
        out, comp = _check(pts, normal, _lists(pts, k))
        assert (out == np.array([0, 0, 1], F)).all() and (comp == 0).all()


def test_identical_points_and_exact_zero_dots():
    same = np.full((64, 3), 0.37, F)
    idx = _lists(same, 8)
    out, _ = _check(same, _pca(same, idx), idx)                          # pf_normals_pca: (0, 0, 1) for all
    assert (out == np.array([0, 0, 1], F)).all()
    _check(same, O.scramble(_pca(same, idx), 1), idx)
    # normals that alternate between +-x and +-y along a line: every dot across an edge is an exact 0, so no edge flips
    # anything; the seed (z ties: point 0) has n_z = +-0 and keeps its sign: the input comes back as it is
    line = np.stack([np.arange(64), np.zeros(64), np.zeros(64)], axis=1).astype(F)
    normal = np.where((np.arange(64) % 2 == 0)[:, None], np.array([1, 0, 0], F), np.array([0, 1, 0], F)).astype(F)
    normal = O.scramble(normal, 9)
    out, comp = _check(line, normal, _lists(line, 2))                    # lists: the point and its left neighbour
    assert np.array_equal(out.view(np.uint32), normal.view(np.uint32)) and (comp == 0).all()


@pytest.mark.parametrize("m,k", [(8, 8), (9, 8), (65, 8), (257, 8), (1029, 16)])
def test_small_and_awkward_sizes(m, k):
    """M = K (a complete graph), one more, across the edges of a wave and of a workgroup, more than four workgroups"""
    rng = np.random.default_rng(m)
    pts = (R.sphere(m, m)[0] + 0.05 * rng.standard_normal((m, 3))).astype(F)
    idx = _lists(pts, k)
    _check(pts, O.scramble(_pca(pts, idx), m), idx)
    v = rng.standard_normal((m, 3))
    _check(pts, (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F), idx)        # unrelated normals: all weights differ
    _check(pts, O.scramble(_pca(pts, idx), m + 1), idx, viewpoint=(0.5, -2.0, 7.0))


def test_one_long_path():
    """K = 2 on 300 collinear points with equal normals: every point's list is itself and its left neighbour, every weight ties,
    so round 0 hooks every point to its left neighbour - one chain of 300 links, the worst case for the pointer jumping"""
    pts = np.stack([np.arange(300), np.zeros(300), np.zeros(300)], axis=1).astype(F)
    idx = _lists(pts, 2)
    assert torch.equal(idx[1:, 1].cpu(), torch.arange(299, dtype=torch.int32))
    out, comp = _check(pts, O.scramble(np.tile(np.array([0, 0, 1], F), (300, 1)), 2), idx)
    assert (out == np.array([0, 0, 1], F)).all() and (comp == 0).all()
    tilted = np.tile(np.array([0.6, 0, 0.8], F), (300, 1))
    _check(pts, O.scramble(tilted, 3), idx, viewpoint=(150.0, 0.0, -4.0))


def test_viewpoint_seed_with_an_exact_distance_tie():
    """every point has a mirror image at exactly the same distance from a viewpoint on the mirror plane: the lowest index is the
    seed.  Two pieces (x > 0.2 and its mirror image), each with its own tie-free and tied candidates"""
    p = R.sphere(400, 21)[0]
    p = p[np.abs(p[:, 0]) > 0.2]
    pts = np.concatenate([p, p * np.array([-1, 1, 1], F)]).astype(F)
    idx = _lists(pts, 8)
    normal = O.scramble(_pca(pts, idx), 4)
    for view in ((0.0, 0.0, 5.0), (0.0, -3.0, 0.25)):
        _check(pts, normal, idx, viewpoint=view)
    # the tie inside a component: two clusters of four (even indices at x = 1, odd at x = -1); seen from (0, 0, 2) the points
    # with y = +-0.001 of a cluster are equally near, as are the two clusters: the seeds are points 0 and 1
    y = np.repeat(np.array([0.001, -0.001, 0.003, -0.003], F), 2)
    sq = np.stack([np.tile(np.array([1, -1], F), 4), y, np.zeros(8, F)], axis=1)
    idx = _lists(sq, 4)
    out, comp = _check(sq, O.scramble(np.tile(np.array([0, 0, 1], F), (8, 1)), 6), idx, viewpoint=(0.0, 0.0, 2.0))
    assert comp.tolist() == [0, 1] * 4 and (out[:, 2] == 1).all()


def _ragged_clouds():
    return [R.surface("sphere", 0.002, 300)[0], R.torus(512, 12, 0.002)[0] * F(2) + F(2), R.surface("sphere", 0.0, 1029)[0] * F(0.5)]


@pytest.mark.parametrize("viewpoint", [None, (0.5, -2.0, 7.0)])
def test_ragged_equals_the_dense_call_on_each_cloud_alone(viewpoint):
    from puflow_amd import attributes as A
    clouds = [_dev(c) for c in _ragged_clouds()]
    normals, _ = A.estimate_normals_ragged(clouds, 16, viewpoint)
    normals = [_dev(O.scramble(n.cpu().numpy(), i)) for i, n in enumerate(normals)]
    for search in ("brute", "grid"):
        got, comp = A.orient_normals_ragged(clouds, normals, 16, viewpoint, search=search)
        for c, n, g, l in zip(clouds, normals, got, comp):
            alone, lalone = A.orient_normals(c, n, 16, viewpoint)
            assert torch.equal(g.view(torch.int32), alone.view(torch.int32)) and torch.equal(l, lalone)
    want, wcomp = O.orient(clouds[1].cpu().numpy(), normals[1].cpu().numpy(), _lists(clouds[1].cpu().numpy(), 16).cpu().numpy(), viewpoint)
    assert torch.equal(got[1].cpu().view(torch.int32), torch.from_numpy(want.view(np.int32))) and torch.equal(comp[1].cpu(), torch.from_numpy(wcomp))
    # estimate_normals_ragged(orient="propagate") is the same thing on the PCA's own lists
    prop, _ = A.estimate_normals_ragged(clouds, 16, viewpoint, search="grid", orient="propagate")
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(prop, got))


def test_ragged_pass_of_65_tiny_clouds():
    """more clouds than one setup launch takes (64), 8 .. 20 points each"""
    from puflow_amd import attributes as A
    rng = np.random.default_rng(65)
    clouds = [_dev(rng.standard_normal((int(m), 3)).astype(F)) for m in rng.integers(8, 21, 65)]
    normals = []
    for c in clouds:
        v = rng.standard_normal((c.shape[0], 3))
        normals.append(_dev((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)))
    got, comp = A.orient_normals_ragged(clouds, normals, 8)
    for i, (c, n, g, l) in enumerate(zip(clouds, normals, got, comp)):
        alone, lalone = A.orient_normals(c, n, 8)
        assert torch.equal(g.view(torch.int32), alone.view(torch.int32)) and torch.equal(l, lalone), i
        if i in (0, 63, 64):
            want, wcomp = O.orient(c.cpu().numpy(), n.cpu().numpy(), R.knn_brute(c.cpu().numpy(), 8))
            assert torch.equal(g.cpu().view(torch.int32), torch.from_numpy(want.view(np.int32))) and torch.equal(l.cpu(), torch.from_numpy(wcomp))


def test_dense_batch_aliasing_and_two_runs():
    from puflow_amd import attributes as A, ops
    pts = torch.stack([_dev(R.torus(700, s, 0.002)[0]) for s in (1, 2, 3)])
    idx, _ = ops.knn_grid(pts, pts, 16)
    normal, _ = ops.normals_pca(pts, idx)
    normal = torch.stack([_dev(O.scramble(n.cpu().numpy(), i)) for i, n in enumerate(normal)])
    a, ca = ops.normals_orient(pts, normal, idx)
    b, cb = ops.normals_orient(pts, normal, idx)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ca, cb)               # the same bits from run to run
    for i in range(3):                                                   # a batch is its clouds alone
        alone, lalone = A.orient_normals(pts[i], normal[i], 16, idx=idx[i])
        assert torch.equal(a[i].view(torch.int32), alone.view(torch.int32)) and torch.equal(ca[i], lalone)
    inplace = normal.clone()
    c, cc = ops.normals_orient(pts, inplace, idx, out=inplace)           # normal_out aliasing normal_in
    assert c.data_ptr() == inplace.data_ptr() and torch.equal(c.view(torch.int32), a.view(torch.int32)) and torch.equal(cc, ca)


def test_a_cloud_of_many_workgroups_does_not_depend_on_the_input_signs():
    """20 000 points (79 workgroups of vertices, 15 rounds enqueued): no restatement, the properties - the same bits whatever the
    signs that came in, one component, nothing opposed to the analytic normal"""
    from puflow_amd import attributes as A
    pts, analytic = R.torus(20000, 12, 0.002)
    p = _dev(pts)
    normal, _ = A.estimate_normals(p, 16, search="grid")
    a, ca = A.orient_normals(p, normal, 16, search="grid")
    b, cb = A.orient_normals(p, _dev(O.scramble(normal.cpu().numpy(), 7)), 16, search="grid")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ca, cb)
    assert int(ca.max()) == 0 and O.opposed(a.cpu().numpy(), analytic) == 0
    prop, _ = A.estimate_normals(p, 16, search="grid", orient="propagate")
    assert torch.equal(prop.view(torch.int32), a.view(torch.int32))


@pytest.mark.parametrize("viewpoint", [None, (0.5, -2.0, 7.0)])
def test_the_default_rule_is_unchanged(viewpoint):
    from puflow_amd import attributes as A
    clouds = [_dev(c) for c in _ragged_clouds()]
    for c in clouds:
        for search in ("brute", "grid"):
            a, b = A.estimate_normals(c, 16, viewpoint, search=search), A.estimate_normals(c, 16, viewpoint, search=search, orient="point")
            assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    a, b = A.estimate_normals_ragged(clouds, 16, viewpoint), A.estimate_normals_ragged(clouds, 16, viewpoint, orient="point")
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[0] + a[1], b[0] + b[1]))
    # and "propagate" keeps the lines and the variation: only signs move
    p = A.estimate_normals(clouds[1], 16, viewpoint, orient="propagate")
    q = A.estimate_normals(clouds[1], 16, viewpoint)
    assert torch.equal(p[0].abs(), q[0].abs()) and torch.equal(p[1], q[1])


# ---- the CLI ---------------------------------------------------------------------------------------------------------------
FILES = {"a.xyz": 600, "b.xyz": 600, "c.xyz": 777, "d.xyz": 1500}


@pytest.fixture(scope="module")
def scans(tmp_path_factory):
    root = tmp_path_factory.mktemp("normals_orient")
    (root / "in3").mkdir()
    for k, (name, n) in enumerate(FILES.items()):
        np.savetxt(root / "in3" / name, R.sphere(n, 70 + k)[0].astype(np.float64), fmt="%.6f")
    torch.save(synth_state_dict(9), root / "ckpt.pt")
    return root


class _Capture:
    """records the points every estimate_normals call of a CLI run was given, per cloud, with what it returned"""

    def __init__(self, monkeypatch):
        from puflow_amd import attributes as A
        self.clouds, self.dense, self.ragged = [], 0, 0
        dense, ragged = A.estimate_normals, A.estimate_normals_ragged

        def one(pred, k, viewpoint=None, search="brute", orient="point"):
            out = dense(pred, k, viewpoint, search=search, orient=orient)
            self.dense += 1
            self.clouds += [(p.clone(), n.clone(), k, viewpoint, orient) for p, n in zip(pred, out[0])]
            return out

        def many(preds, k, viewpoint=None, search="brute", orient="point"):
            out = ragged(preds, k, viewpoint, search=search, orient=orient)
            self.ragged += 1
            self.clouds += [(p.clone(), n.clone(), k, viewpoint, orient) for p, n in zip(preds, out[0])]
            return out
        monkeypatch.setattr(A, "estimate_normals", one)
        monkeypatch.setattr(A, "estimate_normals_ragged", many)
        self.alone = dense


def _cli(root, tag, names, *flags):
    from puflow_amd import upsample as U
    src = root / ("src_" + tag)
    src.mkdir()
    for name in names:
        (src / name).write_bytes((root / "in3" / name).read_bytes())
    U.main(["--source", str(src), "--target", str(root / tag), "--checkpoint", str(root / "ckpt.pt"), "--estimate_normals", "16", *flags])
    return root / tag


def _check_files(cap, out, names, viewpoint=None):
    """every file's normal columns are estimate_normals(pred, 16, orient="propagate") on that run's points, alone"""
    assert len(cap.clouds) == len(names)
    for name, (pred, normal, k, view, orient) in zip(sorted(names), cap.clouds):
        assert k == 16 and orient == "propagate" and view == viewpoint
        want = cap.alone(pred, 16, viewpoint, orient="propagate")[0]
        assert torch.equal(normal.view(torch.int32), want.view(torch.int32))
        rows = np.loadtxt(out / name)
        assert rows.shape == (4 * FILES[name], 6)
        assert np.abs(rows[:, :3] - pred.cpu().numpy()).max() < 1e-6 and np.abs(rows[:, 3:] - want.cpu().numpy()).max() < 1e-6
        assert ((rows[:, 3:] * rows[:, :3]).sum(axis=1) > 0).mean() > 0.99      # a sphere: outwards


def test_cli_dense_and_ragged_passes(scans, monkeypatch):
    """--cloud_batch 2: the dense pair 600 / 600, then the ragged pair 777 / 1500"""
    cap = _Capture(monkeypatch)
    out = _cli(scans, "batched", FILES, "--normals_orient", "propagate", "--cloud_batch", "2", "--attr_search", "grid")
    assert (cap.dense, cap.ragged) == (1, 1)
    _check_files(cap, out, FILES)


def test_cli_tiled_file_with_a_viewpoint(scans, monkeypatch):
    cap = _Capture(monkeypatch)
    out = _cli(scans, "tiled", ["d.xyz"], "--normals_orient", "propagate", "--tile_points", "512", "--normals_viewpoint", "0,0,5")
    assert (cap.dense, cap.ragged) == (1, 0)
    _check_files(cap, out, ["d.xyz"], viewpoint=[0.0, 0.0, 5.0])


def test_cli_without_the_flag_writes_the_same_bytes_as_point(scans):
    import filecmp
    a = _cli(scans, "plain", ["a.xyz"])
    b = _cli(scans, "point", ["a.xyz"], "--normals_orient", "point")
    assert filecmp.cmp(a / "a.xyz", b / "a.xyz", shallow=False)


def test_cli_continuous_model_takes_the_flag(tmp_path, monkeypatch):
    from puflow_amd import cnf, upsample_cnf
    from puflow_amd.weights import synth_cnf_state_dict
    (tmp_path / "in").mkdir()
    np.savetxt(tmp_path / "in" / "a.xyz", R.sphere(600, 70)[0].astype(np.float64), fmt="%.6f")
    torch.save(synth_cnf_state_dict(7), tmp_path / "cnf.pt")
    cnf.save_schedule(cnf.uniform_schedule(3), tmp_path / "sched.json")
    cap = _Capture(monkeypatch)
    upsample_cnf.main(["--source", str(tmp_path / "in"), "--target", str(tmp_path / "out"), "--checkpoint", str(tmp_path / "cnf.pt"),
                       "--num_patch", "128", "--schedule", str(tmp_path / "sched.json"), "--estimate_normals", "16",
                       "--normals_orient", "propagate"])
    assert len(cap.clouds) == 1 and cap.clouds[0][4] == "propagate"
    pred, normal = cap.clouds[0][:2]
    assert torch.equal(normal.view(torch.int32), cap.alone(pred, 16, orient="propagate")[0].view(torch.int32))
    rows = np.loadtxt(tmp_path / "out" / "a.xyz")
    assert rows.shape == (2400, 6) and np.abs(rows[:, 3:] - normal.cpu().numpy()).max() < 1e-6
