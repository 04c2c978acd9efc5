"""Uniformity without a GPU: the float64 restatement (tests/uniform_ref.py) against the reference's analyze_uniform
(tests/golden/eval_uniform.npz, tools/make_golden_uniform.py), the three files' writer and parser, and the new entry points'
declarations and argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import uniform_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pf_tri_closest_points", "pf_mesh_sample", "pf_disk_count", "pf_disk_fill", "pf_disk_tile", "pf_disk_uniformity")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_uniform.npz"))


def _csr(fx, c):
    return fx[f"c{c}_offsets"].astype(np.int64), fx[f"c{c}_member"].astype(np.int64), fx[f"c{c}_level"].astype(np.int64)


def test_restatement_equals_reference(fx):
    for c in range(int(fx["ncases"])):
        ref = fx[f"c{c}_uniform"]
        mine = U.uniformity(fx[f"c{c}_mapped"], _csr(fx, c), fx[f"c{c}_radii"])
        assert np.all(np.abs(mine - ref) <= 1e-10 * np.abs(ref)), (c, mine, ref)
        counts = fx[f"c{c}_counts"]
        assert (counts < 5).any() and (counts >= 5).mean() >= 0.5          # the n < 5 skip is exercised


def test_fixture_is_what_the_restatement_makes(fx):
    """Radii, seeds and disks of the fixture from its meshes, uniforms and mapped points; no point within 1e-5 r of a radius."""
    np.testing.assert_array_equal(fx["uniforms"], U.uniforms(int(fx["seed"]), len(fx["uniforms"])))
    for c in range(int(fx["ncases"])):
        v, f = fx[f"c{c}_verts"], fx[f"c{c}_faces"].astype(np.int64)
        radii, cum = U.area_radii(v, f)
        np.testing.assert_array_equal(radii, fx[f"c{c}_radii"])
        assert np.abs(fx["uniforms"][:, :1].astype(np.float64) - (cum / cum[-1])[None, :]).min() > 1e-7
        seeds = U.seeds_from_uniforms(v, f, fx["uniforms"])[0]
        np.testing.assert_array_equal(seeds.astype(np.float32), fx[f"c{c}_seeds"])
        d = U.seed_distances(fx[f"c{c}_mapped"], fx[f"c{c}_seeds"])
        assert (np.abs(d[:, :, None] - radii) > 1e-5 * radii).all()
        counts, offsets, member, level = U.disks(fx[f"c{c}_mapped"], fx[f"c{c}_seeds"], radii)
        o, m, l = _csr(fx, c)
        np.testing.assert_array_equal(counts, fx[f"c{c}_counts"])
        np.testing.assert_array_equal(offsets, o)
        np.testing.assert_array_equal(member, m)
        np.testing.assert_array_equal(level, l)


def test_disk_files_round_trip(tmp_path, fx):
    from puflow_amd.metrics import read_disk_files, write_disk_files
    c = 2
    cloud, mapped, radii = fx[f"c{c}_cloud"], fx[f"c{c}_mapped"], fx[f"c{c}_radii"]
    dist = np.linalg.norm(cloud.astype(np.float64) - mapped, axis=1).astype(np.float32)
    o, m, l = _csr(fx, c)
    prefix = str(tmp_path / "case")
    write_disk_files(prefix, cloud, dist, mapped, (o, m, l), radii)
    mapped2, radii2, (o2, m2, l2) = read_disk_files(prefix)
    assert mapped2.dtype == np.float32 and (mapped2.view(np.uint32) == mapped.view(np.uint32)).all()
    np.testing.assert_array_equal(radii2, radii)
    np.testing.assert_array_equal(o2, o)
    np.testing.assert_array_equal(m2, m)
    np.testing.assert_array_equal(l2, l)
    rows = np.loadtxt(prefix + "_point2mesh_distance.txt", dtype=np.float32)
    assert (rows[:, :3].view(np.uint32) == cloud.view(np.uint32)).all() and (rows[:, 3] == dist).all()
    # the layout the reference reads: line s J + j = `count:idx idx ...`
    lines = open(prefix + "_disk_idx.txt").read().split("\n")
    s, j = 17, 3
    mem = m[o[s]:o[s + 1]][l[o[s]:o[s + 1]] <= j]
    assert lines[s * 5 + j] == "%d:%s" % (len(mem), " ".join(map(str, mem)))
    # disks that are not nested sets are refused
    lines[0], lines[1] = "2:0 1", "2:1 2"
    open(prefix + "_disk_idx.txt", "w").write("\n".join(lines))
    with pytest.raises(ValueError):
        read_disk_files(prefix)


def test_host_finish_matches_restatement():
    from puflow_amd.metrics import uniformity_from_statistics
    rng = np.random.default_rng(1)
    n = rng.integers(0, 12, (50, 5)).astype(np.float64)
    dis = rng.random((50, 5))
    dis[n < 2] = np.nan
    np.testing.assert_array_equal(uniformity_from_statistics(n, dis, 700), U.uniformity_from_statistics(n, dis, 700))
    n[:, 0] = 4                                   # no disk kept: nan, as numpy gives the reference
    assert np.isnan(uniformity_from_statistics(n, dis, 700)[0])


def test_new_entry_points_are_declared_and_exported():
    from puflow_amd import _lib, build
    build.build(verbose=False)
    hdr = open(os.path.join(ROOT, "include", "puflow_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(pf_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.pf_disk_tile() >= 64


def test_new_entry_points_validate_arguments_without_gpu():
    from puflow_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    r5 = (ctypes.c_double * 5)(0.1, 0.2, 0.3, 0.4, 0.5)
    bad = (ctypes.c_double * 5)(0.1, 0.3, 0.2, 0.4, 0.5)                       # not ascending
    r9 = (ctypes.c_double * 9)(*[0.1 * (i + 1) for i in range(9)])
    assert lib.pf_tri_closest_points(None, 4, 8, 4, 8, 8, None) == -1
    assert lib.pf_tri_closest_points(8, 0, 8, 4, 8, 8, None) == -2
    assert lib.pf_tri_closest_points(8, 4, 8, 0, 8, 8, None) == -2
    assert lib.pf_mesh_sample(8, 4, None, 10, 0, 8, 8, 8, None) == -1
    assert lib.pf_mesh_sample(8, 0, 8, 10, 0, 8, 8, 8, None) == -2
    assert lib.pf_mesh_sample(8, 4, 8, 0, 0, 8, 8, 8, None) == -2
    assert lib.pf_disk_count(None, 10, 8, 3, r5, 5, 8, None) == -1
    assert lib.pf_disk_count(8, 10, 8, 3, None, 5, 8, None) == -1
    assert lib.pf_disk_count(8, 0, 8, 3, r5, 5, 8, None) == -2
    assert lib.pf_disk_count(8, 10, 8, 3, bad, 5, 8, None) == -2
    assert lib.pf_disk_count(8, 10, 8, 3, r9, 9, 8, None) == -2                # J <= 8
    assert lib.pf_disk_fill(8, 10, 8, 3, r5, 5, None, 8, 8, None) == -1
    assert lib.pf_disk_fill(8, 10, 8, 0, r5, 5, 8, 8, 8, None) == -2
    assert lib.pf_disk_uniformity(8, 10, 8, None, 8, 3, r5, 5, 8, 8, None) == -1
    assert lib.pf_disk_uniformity(8, 10, 8, 8, 8, 3, r5, 0, 8, 8, None) == -2
    assert lib.pf_disk_uniformity(8, 10, 8, 8, 8, 3, bad, 5, 8, 8, None) == -2


def test_uniformity_functions_refuse_cpu_tensors(fx):
    import torch
    from puflow_amd import _lib, metrics
    v, f = torch.from_numpy(fx["c0_verts"]), torch.from_numpy(fx["c0_faces"].astype(np.int64))
    pts = torch.from_numpy(fx["c0_cloud"])
    with pytest.raises(_lib.PuflowHipError):
        metrics.sample_mesh(v, f, 10, 0)
    with pytest.raises(_lib.PuflowHipError):
        metrics.mapped_points(pts, v, f)
    with pytest.raises(_lib.PuflowHipError):
        metrics.disks(pts, pts[:4], fx["c0_radii"])
    csr = tuple(torch.from_numpy(a) for a in _csr(fx, 0))
    with pytest.raises(_lib.PuflowHipError):
        metrics.uniformity(pts, csr, fx["c0_radii"])
