"""The reconstruction's surface without a GPU: pf_recon_mark / pf_imls / pf_mtet_* reject bad arguments before any device work,
the triangle table the kernels hold equals the restatement's, the host-side grid rules of puflow_amd.reconstruct equal the
restatement's, and the Python entries and the CLI refuse what they cannot take."""
import ctypes

import numpy as np
import pytest

import recon_ref as M


@pytest.fixture(scope="module")
def lib():
    from puflow_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


PTR = 4096                  # a non-null address that is never dereferenced: every call below fails before a launch
BIG = (1024, 1024, 65)      # 65 * 2^20 corners: over the cap; (1024, 1024, 64) is exactly on it


def _mark(lib, **kw):
    a = dict(pts=PTR, N=100, gx=PTR, gy=PTR, gz=PTR, D=(20, 30, 40), flags=PTR)
    a.update(kw)
    return lib.pf_recon_mark(a["pts"], a["N"], a["gx"], a["gy"], a["gz"], *a["D"], a["flags"], None)


def _imls(lib, **kw):
    a = dict(query=PTR, pts=PTR, normals=PTR, idx=PTR, Q=500, N=100, K=8, sigma_h=0.1, f=PTR)
    a.update(kw)
    return lib.pf_imls(a["query"], a["pts"], a["normals"], a["idx"], a["Q"], a["N"], a["K"], a["sigma_h"], a["f"], None)


def _count(lib, **kw):
    a = dict(f=PTR, flags=PTR, D=(20, 30, 40), count=PTR)
    a.update(kw)
    return lib.pf_mtet_count(a["f"], a["flags"], *a["D"], a["count"], None)


def _emit(lib, **kw):
    a = dict(f=PTR, flags=PTR, D=(20, 30, 40), first=PTR, T=1000, ids=PTR)
    a.update(kw)
    return lib.pf_mtet_emit(a["f"], a["flags"], *a["D"], a["first"], a["T"], a["ids"], None)


def _verts(lib, **kw):
    a = dict(ids=PTR, V=1000, f=PTR, gx=PTR, gy=PTR, gz=PTR, D=(20, 30, 40), verts=PTR)
    a.update(kw)
    return lib.pf_mtet_vertices(a["ids"], a["V"], a["f"], a["gx"], a["gy"], a["gz"], *a["D"], a["verts"], None)


def test_null_pointers(lib):
    for call, names in ((_mark, ("pts", "gx", "gy", "gz", "flags")), (_imls, ("query", "pts", "normals", "idx", "f")),
                        (_count, ("f", "flags", "count")), (_emit, ("f", "flags", "first", "ids")),
                        (_verts, ("ids", "f", "gx", "gy", "gz", "verts"))):
        for name in names:
            assert call(lib, **{name: None}) == -1, (call.__name__, name)
    assert lib.pf_mtet_table(None, 696) == -1


def test_shape_errors(lib):
    assert _mark(lib, N=0) == -2 and _mark(lib, N=-5) == -2 and _mark(lib, N=(1 << 31) // 3 + 1) == -2
    for call in (_mark, _count, _emit, _verts):
        for D in ((1, 30, 40), (20, 1, 40), (20, 30, 1), (0, 30, 40), (20, -3, 40)):
            assert call(lib, D=D) == -2, (call.__name__, D)
    assert _imls(lib, Q=0) == -2 and _imls(lib, N=0) == -2 and _imls(lib, N=7, K=8) == -2
    assert _imls(lib, sigma_h=0.0) == -2 and _imls(lib, sigma_h=-1.0) == -2 and _imls(lib, sigma_h=float("nan")) == -2
    assert _imls(lib, sigma_h=1e-200) == -2                             # 1 / sigma_h^2 is not finite
    assert _emit(lib, T=0) == -2 and _emit(lib, T=12 * 20 * 30 * 40 + 1) == -2
    assert _verts(lib, V=0) == -2 and _verts(lib, V=7 * 20 * 30 * 40 + 1) == -2
    assert lib.pf_mtet_table((ctypes.c_ubyte * 695)(), 695) == -2


def test_unsupported_k_and_a_box_over_the_cap(lib):
    from puflow_amd import _lib
    assert _lib.PF_RECON_MAX_CORNERS == M.MAX_CORNERS == 1 << 26 and 1024 * 1024 * 64 == 1 << 26
    for k in (0, -1, _lib.PF_KNN_GRID_MAX_K + 1, 1000):
        assert _imls(lib, K=k) == -3, k
    for call in (_mark, _count, _emit, _verts):
        assert call(lib, D=BIG) == -3, call.__name__
        assert call(lib, D=(1 << 15, 1 << 15, 1 << 15)) == -3, call.__name__            # the product does not fit an int


def test_the_kernels_table_is_the_restatements(lib):
    from puflow_amd import _lib
    buf = (ctypes.c_ubyte * _lib.PF_MTET_TABLE_BYTES)()
    assert lib.pf_mtet_table(buf, len(buf)) == _lib.PF_MTET_TABLE_BYTES == 24 + 96 + 576
    raw = np.frombuffer(buf, np.uint8)
    corner, ntri, edge = raw[:24].reshape(6, 4), raw[24:120].reshape(6, 16), raw[120:].reshape(6, 16, 2, 3)
    table = M.tet_table()
    for tet in range(6):
        for v in range(4):
            o = M.tet_vertex(tet, v)
            assert corner[tet, v] == o[0] | o[1] << 1 | o[2] << 2
        assert ntri[tet, 0] == 0 and ntri[tet, 15] == 0
        for mask in range(1, 15):
            tris = table[tet, mask]
            assert ntri[tet, mask] == len(tris)
            for s, tri in enumerate(tris):
                for e, (i, j) in enumerate(tri):
                    a, b = M.tet_vertex(tet, i), M.tet_vertex(tet, j)
                    cls = M.EDGE_CLASSES.index((b[0] - a[0], b[1] - a[1], b[2] - a[2]))
                    assert edge[tet, mask, s, e] == (a[0] | a[1] << 1 | a[2] << 2) << 3 | cls, (tet, mask, s, e)


def test_host_grid_rules_are_the_restatements():
    from puflow_amd import reconstruct as R
    rng = np.random.default_rng(4)
    assert R.PAD == M.PAD
    for _ in range(20):
        lo = rng.uniform(-3, 3, 3).astype(np.float32)
        hi = (lo + rng.uniform(0, 2, 3)).astype(np.float32)
        h = float(rng.uniform(0.01, 0.3))
        dims, tables = R.corner_tables(lo.astype(np.float64), hi.astype(np.float64), h)
        wdims, wtables = M.grid(lo, hi, h)
        assert dims == wdims and all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(tables, wtables))
    dims, _ = R.corner_tables(np.zeros(3), np.zeros(3), 0.5)                # a single point: 7 corners per axis
    assert dims == (7, 7, 7)


def test_python_entries_refuse_before_any_device_work():
    import torch
    from puflow_amd import _lib, reconstruct as R
    x = torch.zeros(16, 3)
    for call in (lambda: R.mesh_from_cloud(x, x), lambda: R.cell_size(x), lambda: R.implicit(x, x, x, h=0.1)):
        with pytest.raises(_lib.PuflowHipError, match="GPU"):
            call()
    with pytest.raises(_lib.PuflowHipError, match="larger --cell"):
        R.corner_tables(np.zeros(3), np.ones(3), 1e-3)
    with pytest.raises(_lib.PuflowHipError, match="larger --cell"):
        R.corner_tables(np.zeros(3), np.ones(3), 1e-300)


def test_cli_refuses_a_file_without_normals(tmp_path):
    from puflow_amd import reconstruct as R
    (tmp_path / "in").mkdir()
    np.savetxt(tmp_path / "in" / "a.xyz", np.random.default_rng(0).uniform(-1, 1, (50, 3)), fmt="%.6f")
    argv = ["--source", str(tmp_path / "in"), "--target", str(tmp_path / "out")]
    with pytest.raises(SystemExit, match="--estimate_normals K --normals_orient propagate"):
        R.main(argv)
    with pytest.raises(SystemExit, match="normal_column"):
        R.main(argv + ["--normal_column", "2"])
    assert not (tmp_path / "out").exists()                               # refused before anything is made
    with pytest.raises(SystemExit):                                      # argparse: one or the other
        R.main(argv + ["--cell", "0.1", "--cell_scale", "2"])


def test_write_off_round_trip(tmp_path):
    from puflow_amd import metrics, reconstruct as R
    f = np.full((3, 3, 3), 1.0, np.float32)
    f[1, 1, 1] = -0.3
    verts, faces, _ = M.extract(f, np.ones(f.shape, np.uint8), [np.array([0.1, 0.4, 0.7], np.float32)] * 3)
    R.write_off(tmp_path / "m.off", verts, faces)
    R.write_off(tmp_path / "m2.off", verts, faces)
    assert (tmp_path / "m.off").read_bytes() == (tmp_path / "m2.off").read_bytes()
    v, fa = metrics.read_off(tmp_path / "m.off")
    assert np.array_equal(fa, faces) and np.abs(v - verts).max() < 1e-6
    head = (tmp_path / "m.off").read_text().splitlines()
    assert head[0] == "OFF" and head[1] == f"{len(verts)} {len(faces)} 0" and head[2 + len(verts)].startswith("3 ")
