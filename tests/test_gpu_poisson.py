"""Poisson-disk sampling on the GPU (csrc/poisson.hip, puflow_amd.sampling, python -m puflow_amd.prepare) against the numpy
restatement of its definition (tests/poisson_ref.py): the graph edge for edge, the kept sets index for index."""
import os

import numpy as np
import pytest
import torch

import poisson_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def square_mesh():
    return (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], dtype=np.float32),
            np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64))


def torus_mesh(nu=24, nv=12, R0=1.0, r0=0.4):
    u = np.arange(nu) * (2.0 * np.pi / nu)
    v = np.arange(nv) * (2.0 * np.pi / nv)
    uu, vv = np.meshgrid(u, v, indexing="ij")
    verts = np.stack([(R0 + r0 * np.cos(vv)) * np.cos(uu), (R0 + r0 * np.cos(vv)) * np.sin(uu), r0 * np.sin(vv)], -1)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b = idx, np.roll(idx, -1, 0)
    c, d = np.roll(b, -1, 1), np.roll(idx, -1, 1)
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return verts.reshape(-1, 3).astype(np.float32), faces.astype(np.int64)


MESHES = {"square": square_mesh(), "torus": torus_mesh()}
_CACHE = {}


def mesh_area(name):
    from puflow_amd import metrics
    return float(metrics.mesh_area_radii(*MESHES[name])[1][-1])


def pool(name, s, seed, triple=False):
    """s surface samples of the mesh (pf_mesh_sample) as a device tensor; triple: candidates 1 and 2 are copies of 0."""
    from puflow_amd import metrics
    key = ("pool", name, s, seed, triple)
    if key not in _CACHE:
        v, f = MESHES[name]
        p = metrics.sample_mesh(_t(v), _t(f, np.int64), s, seed)[0].clone()
        if triple:
            p[1] = p[0]
            p[2] = p[0]
        _CACHE[key] = p
    return _CACHE[key]


def ref_graph(name, s, seed, m, triple=False):
    """The restatement's graph of that pool, made once and never written to."""
    key = ("graph", name, s, seed, m, triple)
    if key not in _CACHE:
        g = R.neighbour_graph(pool(name, s, seed, triple).cpu().numpy(), mesh_area(name), m)
        for a in g:
            a.setflags(write=False)
        _CACHE[key] = g
    return _CACHE[key]


def ref_keep(name, s, seed, m, triple=False):
    key = ("keep", name, s, seed, m, triple)
    if key not in _CACHE:
        _CACHE[key] = R.eliminate_sequential(*ref_graph(name, s, seed, m, triple), m)
    return _CACHE[key]


@pytest.mark.parametrize("name,s,m,triple", [("square", 64, 16, False), ("torus", 1280, 256, False), ("square", 600, 120, True)])
def test_neighbour_graph_equals_the_restatement(name, s, m, triple):
    from puflow_amd import sampling
    offsets, nbr, q = sampling.neighbour_graph(pool(name, s, 11, triple), [s], [mesh_area(name)], [m])
    ro, rn, rq = ref_graph(name, s, 11, m, triple)
    assert len(rn) > s                                                    # a real graph: more than one neighbour on average
    assert np.array_equal(offsets.cpu().numpy(), ro)
    assert np.array_equal(nbr.cpu().numpy(), rn)
    assert np.array_equal(q.cpu().numpy().astype(np.int64), rq)


# 8192 / 8193: one pool on each side of the single-workgroup path's size limit (PF_POISSON_WG_MAX)
CASES = [("square", 64, 16, False), ("square", 600, 120, True), ("torus", 1280, 256, False), ("torus", 5120, 1024, False),
         ("square", 1280, 1279, False), ("square", 1280, 1280, False), ("square", 300, 1, False),
         ("torus", 8192, 1638, False), ("torus", 8193, 1638, False)]


@pytest.mark.parametrize("name,s,m,triple", CASES)
def test_eliminate_equals_the_sequential_restatement(name, s, m, triple):
    from puflow_amd import sampling
    keep, info = sampling.eliminate(pool(name, s, 11, triple), [s], [m], [mesh_area(name)])
    print(f"{name} {s} -> {m}: path {info['paths'][0]}, {int(info['phases'][0])} phases, {int(info['rounds'][0])} rounds, "
          f"{info['launches']} launches")
    assert info["paths"] == ["workgroup" if s <= 8192 else "rounds"] and info["status"] == 0
    assert keep.dtype == torch.int64 and np.array_equal(keep.cpu().numpy(), ref_keep(name, s, 11, m, triple))
    if m < s:
        assert 1 <= info["phases"][0] <= info["rounds"][0] <= s - m


@pytest.mark.parametrize("name,s,m,triple", [("torus", 1280, 256, False), ("square", 600, 120, True), ("square", 300, 1, False)])
def test_round_launches_equal_the_single_workgroup(name, s, m, triple):
    """The three-launches-a-round path on pools the single-workgroup path also takes: the same indices."""
    from puflow_amd import sampling
    keep, info = sampling.eliminate(pool(name, s, 11, triple), [s], [m], [mesh_area(name)], single_workgroup=False)
    assert info["paths"] == ["rounds"] and info["launches"] % 3 == 0
    assert np.array_equal(keep.cpu().numpy(), ref_keep(name, s, 11, m, triple))


RAGGED = [("torus", 1280, 256), ("torus", 5120, 1024), ("square", 700, 100)]


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1), (1, 2, 0)])
@pytest.mark.parametrize("single_workgroup", [True, False])
def test_ragged_batch_equals_each_pool_alone(order, single_workgroup):
    from puflow_amd import sampling
    alone = {}
    for i, (name, s, m) in enumerate(RAGGED):
        key = ("alone", i)
        if key not in _CACHE:
            _CACHE[key] = sampling.eliminate(pool(name, s, 5), [s], [m], [mesh_area(name)])[0].cpu().numpy()
        alone[i] = _CACHE[key]
    pts = torch.cat([pool(RAGGED[i][0], RAGGED[i][1], 5) for i in order])
    keep, info = sampling.eliminate(pts, [RAGGED[i][1] for i in order], [RAGGED[i][2] for i in order],
                                    [mesh_area(RAGGED[i][0]) for i in order], single_workgroup=single_workgroup)
    got = np.split(keep.cpu().numpy(), np.cumsum([RAGGED[i][2] for i in order])[:-1])
    for i, g in zip(order, got):
        assert np.array_equal(g, alone[i]), RAGGED[i]
    assert len(info["phases"]) == 3 and info["status"] == 0


def test_mixed_paths_in_one_call():
    """A pool beyond the single-workgroup limit beside two within it: every pool as alone."""
    from puflow_amd import sampling
    specs = [("torus", 1280, 256), ("torus", 8193, 1638), ("square", 600, 120)]
    pts = torch.cat([pool(n, s, 11, n == "square") for n, s, _ in specs])
    keep, info = sampling.eliminate(pts, [s for _, s, _ in specs], [m for _, _, m in specs], [mesh_area(n) for n, _, _ in specs])
    assert info["paths"] == ["workgroup", "rounds", "workgroup"]
    got = np.split(keep.cpu().numpy(), np.cumsum([m for _, _, m in specs])[:-1])
    for (n, s, m), g in zip(specs, got):
        assert np.array_equal(g, ref_keep(n, s, 11, m, n == "square"))


def test_two_calls_are_bit_identical():
    from puflow_amd import sampling
    p, a = pool("torus", 5120, 11), mesh_area("torus")
    g1, g2 = sampling.neighbour_graph(p, [5120], [a], [1024]), sampling.neighbour_graph(p, [5120], [a], [1024])
    assert all(torch.equal(x, y) for x, y in zip(g1, g2))
    for sw in (True, False):
        k1, i1 = sampling.eliminate(p, [5120], [1024], [a], single_workgroup=sw)
        k2, i2 = sampling.eliminate(p, [5120], [1024], [a], single_workgroup=sw)
        assert torch.equal(k1, k2) and np.array_equal(i1["rounds"], i2["rounds"]) and np.array_equal(i1["phases"], i2["phases"])


def _nn_cv(p):
    """std / mean of the nearest-neighbour distance inside the device point set p [n,3], in float64."""
    p = p.double()
    best = []
    for a in range(0, len(p), 1024):
        d2 = (p[a:a + 1024, None, :] - p[None, :, :]).pow(2).sum(-1)
        d2[torch.arange(d2.shape[0]), torch.arange(a, a + d2.shape[0])] = float("inf")
        best.append(d2.amin(1))
    d = torch.cat(best).sqrt()
    return float(d.std(unbiased=False) / d.mean())


def _blue_noise(pool_pts, kept, seed=3):
    rand = torch.from_numpy(np.random.default_rng(seed).choice(len(pool_pts), len(kept), replace=False)).to(DEV)
    cv_kept, cv_rand = _nn_cv(kept), _nn_cv(pool_pts[rand])
    print(f"nearest-neighbour distance std/mean: kept {cv_kept:.3f}, random subset {cv_rand:.3f}")
    assert cv_kept <= 0.5 * cv_rand


def test_poisson_disk_on_the_torus():
    from puflow_amd import metrics, sampling
    v, f = MESHES["torus"]
    vt, ft = _t(v), _t(f, np.int64)
    pts, face = sampling.poisson_disk(vt, ft, 256, seed=4)
    assert pts.shape == (256, 3) and pts.dtype == torch.float32 and face.shape == (256,) and face.dtype == torch.int64
    # every point on its face: barycentric coordinates in float64, the residual within fp32 rounding of coordinates of O(1.4)
    tri = v[f[face.cpu().numpy()]].astype(np.float64)
    p = pts.cpu().numpy().astype(np.float64)
    for k in range(256):
        M = np.stack([tri[k, 1] - tri[k, 0], tri[k, 2] - tri[k, 0]], 1)
        uv, *_ = np.linalg.lstsq(M, p[k] - tri[k, 0], rcond=None)
        assert np.abs(M @ uv + tri[k, 0] - p[k]).max() <= 4 * 2.0 ** -24 * 1.4
        assert uv.min() >= -1e-6 and uv.sum() <= 1.0 + 1e-6
    # a function of (mesh, m, seed, ratio) only - not of what ran before, and of each of them
    again, face2 = sampling.poisson_disk(vt.clone(), ft.clone(), 256, seed=4)
    assert torch.equal(pts, again) and torch.equal(face, face2)
    assert not torch.equal(pts, sampling.poisson_disk(vt, ft, 256, seed=5)[0])
    assert not torch.equal(pts, sampling.poisson_disk(vt, ft, 256, seed=4, ratio=4)[0])
    assert len(np.unique(pts.cpu().numpy(), axis=0)) == 256
    _blue_noise(metrics.sample_mesh(vt, ft, 1280, 4)[0], pts)


def test_make_patches():
    from puflow_amd import metrics, sampling
    v, f = MESHES["torus"]
    vt, ft = _t(v), _t(f, np.int64)
    out, pools = sampling.make_patches(vt, ft, 3, seed=2, return_pools=True)
    inp, gt = out["poisson_256"], out["poisson_1024"]
    assert inp.shape == (3, 256, 3) and gt.shape == (3, 1024, 3) and sorted(out) == ["poisson_1024", "poisson_256"]
    assert pools["seeds"].shape == (3, 3) and pools["input_pool"].shape == (3, 1280, 3) and pools["gt_pool"].shape == (3, 5120, 3)
    # the candidate ball of a patch: the seed's K nearest of the sample set (seed + 2: input, seed + 1: ground truth)
    for arr, n_set, sd, K in ((inp, 12500, 4, 1280), (gt, 50000, 3, 5120)):
        samples = metrics.sample_mesh(vt, ft, n_set, sd)[0].double()
        for p in range(3):
            seed_pt = pools["seeds"][p].double()
            ball = (samples - seed_pt).norm(dim=1).kthvalue(K).values
            assert float((arr[p].double() - seed_pt).norm(dim=1).max()) <= float(ball) * (1.0 + 1e-6)
            assert len(np.unique(arr[p].cpu().numpy(), axis=0)) == arr.shape[1]
    rows = lambda a: {r.tobytes() for r in a.reshape(-1, 3).cpu().numpy()}          # noqa: E731
    assert not rows(inp) & rows(gt)
    again = sampling.make_patches(vt, ft, 3, seed=2)
    assert torch.equal(again["poisson_256"], inp) and torch.equal(again["poisson_1024"], gt)


def _write_off(path, v, f):
    with open(path, "w") as fh:
        fh.write("OFF\n%d %d 0\n" % (len(v), len(f)))
        fh.write("".join("%.9g %.9g %.9g\n" % tuple(r) for r in v.tolist()))
        fh.write("".join("3 %d %d %d\n" % tuple(r) for r in f.tolist()))


def test_cli_round_trip(tmp_path):
    from puflow_amd import data, evaluate, prepare
    from puflow_amd.upsample import load_xyz
    mesh = tmp_path / "mesh"
    mesh.mkdir()
    _write_off(mesh / "torus.off", *MESHES["torus"])
    _write_off(mesh / "square.off", *MESHES["square"])
    args = ["--mesh", str(mesh), "--seed", "9", "--patches", "3", "--cloud_points", "600", "--clouds", "256,1024"]
    prepare.main(args + ["--out", str(tmp_path / "a")])
    prepare.main(args + ["--out", str(tmp_path / "b")])
    files = ["patches.npz"] + [os.path.join(d, n + ".xyz") for d in ("input_256", "gt_1024") for n in ("square", "torus")]
    for rel in files:
        assert (tmp_path / "a" / rel).read_bytes() == (tmp_path / "b" / rel).read_bytes(), rel
    # patches -> the training loader
    inp, gt, rad = data.load_patch_arrays(str(tmp_path / "a" / "patches.npz"))
    assert inp.shape == (6, 256, 3) and gt.shape == (6, 1024, 3) and rad.shape == (6,)
    batch = next(iter(data.PatchData(inp, gt, rad, batch_size=4, is_augment=False, device=DEV)))
    x, y = batch["input_sparse_xyz_pl"], batch["gt_dense_xyz_pl"]
    assert x.shape == (4, 256, 3) and y.shape == (4, 1024, 3) and bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all())
    assert torch.allclose(x.norm(dim=2).amax(1), torch.ones(4, device=DEV), atol=1e-6)
    # clouds -> the stated counts, and the evaluation reads them
    for d, n in (("input_256", 256), ("gt_1024", 1024)):
        for name in ("square", "torus"):
            assert load_xyz(tmp_path / "a" / d / f"{name}.xyz").shape == (n, 3)
    inp_cloud, gt_cloud = load_xyz(tmp_path / "a" / "input_256" / "torus.xyz"), load_xyz(tmp_path / "a" / "gt_1024" / "torus.xyz")
    assert not {r.tobytes() for r in inp_cloud} & {r.tobytes() for r in gt_cloud}      # another seed per count
    _, summary = evaluate.evaluate(str(tmp_path / "a" / "gt_1024"), str(tmp_path / "a" / "gt_1024"), str(tmp_path / "eval"))
    assert float(summary["CD"]) == 0.0 and float(summary["hausdorff"]) == 0.0


def test_large_pool_40960_to_8192():
    """Beyond the single-workgroup limit and too slow to restate on the CPU: the count, the indices' form and the blue noise."""
    from puflow_amd import metrics, sampling
    v, f = MESHES["torus"]
    pts = metrics.sample_mesh(_t(v), _t(f, np.int64), 40960, 21)[0]
    keep, info = sampling.eliminate(pts, [40960], [8192], [mesh_area("torus")])
    print(f"40960 -> 8192: {int(info['phases'][0])} phases, {int(info['rounds'][0])} rounds, {info['launches']} launches")
    k = keep.cpu().numpy()
    assert k.shape == (8192,) and info["paths"] == ["rounds"] and info["status"] == 0
    assert k.min() >= 0 and k.max() < 40960 and bool((np.diff(k) > 0).all())
    _blue_noise(pts, pts[keep])
