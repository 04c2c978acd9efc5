"""search="grid" (pf_knn_grid) behind the per-point attributes and the PCA normals: torch.equal to search="brute" in the library,
and the same files from both CLIs with --attr_search grid as without it (a directory of mixed-size files, one tiled file)."""
import filecmp

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attr_ref as R
from puflow_amd.weights import synth_state_dict

DEV = "cuda:0"
SIZES, OUT_SIZES = [300, 512, 1029], [700, 333, 1500]
PLAN = "normal,lin3,near1"
FILES = {"a.xyz": 600, "b.xyz": 600, "c.xyz": 777, "d.xyz": 1500}


def _rows(rng, n):
    """7 attribute columns for PLAN: a unit vector of either sign, three N(0, 3) columns, an integer label"""
    v = rng.standard_normal((n, 3))
    return np.concatenate([v / np.linalg.norm(v, axis=1, keepdims=True), 3.0 * rng.standard_normal((n, 3)),
                           rng.integers(0, 9, (n, 1)).astype(np.float64)], axis=1).astype(np.float32)


def _clouds():
    rng = np.random.default_rng(8)
    clouds = [torch.from_numpy((rng.uniform(-1, 1, (n, 3)) * (1 + i) + i).astype(np.float32)).to(DEV) for i, n in enumerate(SIZES)]
    preds = [torch.cat([c[: m // 3], torch.from_numpy((rng.uniform(-1, 1, (m - m // 3, 3)) * (1 + i) + i).astype(np.float32)).to(DEV)])
             for i, (c, m) in enumerate(zip(clouds, OUT_SIZES))]
    attrs = [torch.from_numpy(_rows(rng, n)).to(DEV) for n in SIZES]
    return clouds, preds, attrs


@pytest.mark.parametrize("k", [1, 3, 8])
def test_transfer_with_either_search(k):
    from puflow_amd import attributes as A
    clouds, preds, attrs = _clouds()
    for p, c, a in zip(preds, clouds, attrs):
        assert torch.equal(A.transfer(p, c, a, PLAN, k=k, search="grid"), A.transfer(p, c, a, PLAN, k=k, search="brute"))
        assert torch.equal(A.transfer(p, c, a, PLAN, k=k, search="brute"), A.transfer(p, c, a, PLAN, k=k))       # the default
    batch = (torch.stack([preds[0], preds[0].flip(0)]), torch.stack([clouds[0], clouds[0]]), torch.stack([attrs[0], attrs[0] * 2]))
    assert torch.equal(A.transfer(*batch, PLAN, k=k, search="grid"), A.transfer(*batch, PLAN, k=k))
    grid, brute = A.transfer_ragged(preds, clouds, attrs, PLAN, k=k, search="grid"), A.transfer_ragged(preds, clouds, attrs, PLAN, k=k)
    assert len(grid) == 3 and all(torch.equal(g, b) for g, b in zip(grid, brute))


@pytest.mark.parametrize("k,viewpoint", [(8, None), (16, (0.5, -2.0, 7.0)), (64, None)])
def test_normals_with_either_search(k, viewpoint):
    from puflow_amd import attributes as A
    clouds = [torch.from_numpy(R.surface(name, 0.002, n)[0] * s + s).to(DEV) for name, n, s in
              (("sphere", 300, 1.0), ("torus", 512, 2.0), ("sphere", 1029, 0.5))]
    for c in clouds:
        g, b = A.estimate_normals(c, k, viewpoint, search="grid"), A.estimate_normals(c, k, viewpoint)
        assert torch.equal(g[0], b[0]) and torch.equal(g[1], b[1])
    g, b = A.estimate_normals_ragged(clouds, k, viewpoint, search="grid"), A.estimate_normals_ragged(clouds, k, viewpoint)
    assert all(torch.equal(x, y) for x, y in zip(g[0] + g[1], b[0] + b[1]))
    flat = torch.full((64, 3), 0.37, device=DEV)                                      # one point 64 times: one cell
    g, b = A.estimate_normals(flat, k, viewpoint, search="grid"), A.estimate_normals(flat, k, viewpoint)
    assert torch.equal(g[0], b[0]) and torch.equal(g[1], b[1])


def _sphere_rows(n, seed):
    """xyz on the unit sphere | normal = p | three blended columns | label = the octant"""
    p = R.sphere(n, seed)[0].astype(np.float64)
    octant = (p[:, 0] > 0) * 1 + (p[:, 1] > 0) * 2 + (p[:, 2] > 0) * 4
    return np.concatenate([p, p, p[:, :1], p[:, :1] + p[:, 1:2], p[:, 2:] * 2, octant[:, None].astype(np.float64)], axis=1)


@pytest.fixture(scope="module")
def scans(tmp_path_factory):
    root = tmp_path_factory.mktemp("attr_search")
    (root / "in10").mkdir()
    (root / "in3").mkdir()
    (root / "big10").mkdir()
    (root / "big3").mkdir()
    for k, (name, n) in enumerate(FILES.items()):
        rows = _sphere_rows(n, 70 + k)
        np.savetxt(root / "in10" / name, rows, fmt="%.6f")
        np.savetxt(root / "in3" / name, rows[:, :3], fmt="%.6f")
    np.savetxt(root / "big10" / "d.xyz", _sphere_rows(1500, 73), fmt="%.6f")
    np.savetxt(root / "big3" / "d.xyz", _sphere_rows(1500, 73)[:, :3], fmt="%.6f")
    torch.save(synth_state_dict(9), root / "ckpt.pt")
    return root


def _cli(root, src, tag, *flags):
    from puflow_amd import upsample as U
    U.main(["--source", str(root / src), "--target", str(root / tag), "--checkpoint", str(root / "ckpt.pt"), *flags])
    return root / tag


def _same(a, b, names):
    match, mismatch, errors = filecmp.cmpfiles(a, b, list(names), shallow=False)
    return sorted(match) == sorted(names) and not mismatch and not errors


@pytest.mark.parametrize("src,names,flags", [
    ("in10", FILES, ("--attributes", PLAN)),
    ("in3", FILES, ("--estimate_normals", "16")),
    ("big10", ["d.xyz"], ("--attributes", PLAN, "--tile_points", "512")),
    ("big3", ["d.xyz"], ("--estimate_normals", "16", "--tile_points", "512")),
])
def test_cli_writes_the_same_files_with_either_search(scans, src, names, flags):
    tag = src + "_" + flags[0].strip("-")
    brute = _cli(scans, src, tag + "_brute", *flags)
    grid = _cli(scans, src, tag + "_grid", *flags, "--attr_search", "grid")
    assert _same(brute, grid, names)
    if src == "in10":
        assert _same(brute, _cli(scans, src, tag + "_explicit", *flags, "--attr_search", "brute"), names)
    cols = np.loadtxt(grid / list(names)[0]).shape[1]
    assert cols == (10 if "--attributes" in flags else 6)


def test_cli_really_takes_the_grid_search(scans, monkeypatch):
    """--attr_search grid calls pf_knn_grid's wrappers and not pf_knn_large's (mixed sizes: the ragged pass)"""
    from puflow_amd import ops
    calls = {"grid": 0, "brute": 0}

    def counted(fn, key):
        def f(*a, **kw):
            calls[key] += 1
            return fn(*a, **kw)
        return f
    for name, key in (("knn_grid", "grid"), ("knn_grid_ragged", "grid"), ("knn_large_ragged", "brute")):
        monkeypatch.setattr(ops, name, counted(getattr(ops, name), key))
    _cli(scans, "in10", "counted", "--attributes", PLAN, "--attr_search", "grid", "--cloud_batch", "2")
    assert calls["grid"] == 2 and calls["brute"] == 0                    # the dense pair 600 / 600 and the ragged pair 777 / 1500


def test_cli_continuous_model_takes_the_flag(tmp_path):
    from puflow_amd import cnf, upsample_cnf
    from puflow_amd.weights import synth_cnf_state_dict
    (tmp_path / "in").mkdir()
    np.savetxt(tmp_path / "in" / "a.xyz", _sphere_rows(600, 70), fmt="%.6f")
    torch.save(synth_cnf_state_dict(7), tmp_path / "cnf.pt")
    cnf.save_schedule(cnf.uniform_schedule(3), tmp_path / "sched.json")
    argv = ["--source", str(tmp_path / "in"), "--checkpoint", str(tmp_path / "cnf.pt"), "--num_patch", "128", "--schedule",
            str(tmp_path / "sched.json"), "--attributes", PLAN, "--attr_k", "4"]
    upsample_cnf.main(argv + ["--target", str(tmp_path / "brute")])
    upsample_cnf.main(argv + ["--target", str(tmp_path / "grid"), "--attr_search", "grid"])
    assert filecmp.cmp(tmp_path / "brute" / "a.xyz", tmp_path / "grid" / "a.xyz", shallow=False)
    assert np.loadtxt(tmp_path / "grid" / "a.xyz").shape == (2400, 10)
