"""The block-sparse reconstruction's surface without a GPU: its constants, every new entry point rejecting bad arguments before
any device work, and the host-side grid rule of puflow_amd.reconstruct under the sparse layout's cap."""
import numpy as np
import pytest

import recon_ref as M
import recon_sparse_ref as S


@pytest.fixture(scope="module")
def lib():
    from puflow_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


PTR = 4096                  # a non-null address that is never dereferenced: every call below fails before a launch
D = (20, 30, 40)            # 3 x 4 x 5 = 60 blocks


def _keys(lib, **kw):
    a = dict(pts=PTR, N=100, gx=PTR, gy=PTR, gz=PTR, D=D, keys=PTR)
    a.update(kw)
    return lib.pf_recon_block_keys(a["pts"], a["N"], a["gx"], a["gy"], a["gz"], *a["D"], a["keys"], None)


def _links(lib, **kw):
    a = dict(blocks=PTR, NB=10, D=D, links=PTR)
    a.update(kw)
    return lib.pf_recon_block_links(a["blocks"], a["NB"], *a["D"], a["links"], None)


def _mark(lib, **kw):
    a = dict(pts=PTR, N=100, gx=PTR, gy=PTR, gz=PTR, D=D, blocks=PTR, NB=10, flags=PTR)
    a.update(kw)
    return lib.pf_recon_mark_sparse(a["pts"], a["N"], a["gx"], a["gy"], a["gz"], *a["D"], a["blocks"], a["NB"], a["flags"], None)


def _count(lib, **kw):
    a = dict(f=PTR, flags=PTR, blocks=PTR, links=PTR, NB=10, D=D, count=PTR)
    a.update(kw)
    return lib.pf_mtet_count_sparse(a["f"], a["flags"], a["blocks"], a["links"], a["NB"], *a["D"], a["count"], None)


def _emit(lib, **kw):
    a = dict(f=PTR, flags=PTR, blocks=PTR, links=PTR, NB=10, D=D, cells=PTR, first=PTR, M=100, T=1000, ids=PTR)
    a.update(kw)
    return lib.pf_mtet_emit_sparse(a["f"], a["flags"], a["blocks"], a["links"], a["NB"], *a["D"], a["cells"], a["first"], a["M"], a["T"],
                                   a["ids"], None)


def _verts(lib, **kw):
    a = dict(ids=PTR, V=1000, f=PTR, blocks=PTR, links=PTR, NB=10, gx=PTR, gy=PTR, gz=PTR, D=D, verts=PTR)
    a.update(kw)
    return lib.pf_mtet_vertices_sparse(a["ids"], a["V"], a["f"], a["blocks"], a["links"], a["NB"], a["gx"], a["gy"], a["gz"], *a["D"],
                                       a["verts"], None)


CALLS = ((_keys, ("pts", "gx", "gy", "gz", "keys")), (_links, ("blocks", "links")),
         (_mark, ("pts", "gx", "gy", "gz", "blocks", "flags")), (_count, ("f", "flags", "blocks", "links", "count")),
         (_emit, ("f", "flags", "blocks", "links", "cells", "first", "ids")),
         (_verts, ("ids", "f", "blocks", "links", "gx", "gy", "gz", "verts")))
WITH_LIST = (_links, _mark, _count, _emit, _verts)


def test_constants():
    from puflow_amd import _lib, ops, reconstruct as R
    assert _lib.PF_RECON_BLOCK == S.B == R.BLOCK == ops.RECON_BLOCK == 8 and R.SLOTS == ops.RECON_SLOTS == S.SLOTS == 512
    assert _lib.PF_RECON_SPARSE_MAX_AXIS == S.MAX_AXIS == R.MAX_AXIS == 1 << 20
    assert _lib.PF_RECON_SPARSE_MAX_BLOCKS == S.MAX_BLOCKS == R.MAX_BLOCKS == 1 << 21
    assert 7 * (1 << 20) ** 3 + 6 < 1 << 63 and (1 << 21) * 512 <= 1 << 31
    assert _lib.PF_RECON_MAX_CORNERS == 1 << 26                          # the dense cap stays


def test_null_pointers(lib):
    for call, names in CALLS:
        for name in names:
            assert call(lib, **{name: None}) == -1, (call.__name__, name)


def test_shape_errors(lib):
    for call, _ in CALLS:
        for dims in ((1, 30, 40), (20, 1, 40), (20, 30, 1), (0, 30, 40), (20, -3, 40)):
            assert call(lib, D=dims) == -2, (call.__name__, dims)
    for call in (_keys, _mark):
        for n in (0, -5, (1 << 31) // 3 + 1):
            assert call(lib, N=n) == -2, (call.__name__, n)
    for call in WITH_LIST:
        assert call(lib, NB=0) == -2 and call(lib, NB=-1) == -2, call.__name__
        assert call(lib, NB=61) == -2, call.__name__                     # the grid has 60 blocks
    assert _emit(lib, M=0) == -2 and _emit(lib, M=10 * 512 + 1, T=10 * 512 + 1) == -2
    assert _emit(lib, T=0) == -2 and _emit(lib, T=12 * 100 + 1) == -2
    assert _verts(lib, V=0) == -2 and _verts(lib, V=7 * 512 * 10 + 1) == -2


def test_an_axis_or_a_list_over_its_cap(lib):
    over = (1 << 20) + 1
    for call, _ in CALLS:
        for dims in ((over, 30, 40), (20, over, 40), (20, 30, over), (1 << 30, 1 << 30, 1 << 30)):
            assert call(lib, D=dims) == -3, (call.__name__, dims)
    grid = (1 << 11, 1 << 11, 1 << 11)                                   # 2^24 blocks
    for call in WITH_LIST:
        assert call(lib, D=grid, NB=(1 << 21) + 1) == -3, call.__name__
        assert call(lib, D=grid, NB=1 << 30) == -3, call.__name__


def test_corner_tables_under_the_sparse_cap():
    from puflow_amd import _lib, reconstruct as R
    rng = np.random.default_rng(4)
    for _ in range(20):                                                  # the dense tables where both are allowed
        lo = rng.uniform(-3, 3, 3).astype(np.float32)
        hi = (lo + rng.uniform(0, 2, 3)).astype(np.float32)
        h = float(rng.uniform(0.01, 0.3))
        want = R.corner_tables(lo.astype(np.float64), hi.astype(np.float64), h)
        assert want[0] == M.grid(lo, hi, h)[0]
        for layout in ("sparse", "auto"):
            dims, tables = R.corner_tables(lo.astype(np.float64), hi.astype(np.float64), h, layout=layout)
            assert dims == want[0] and all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(tables, want[1]))
    pts, _ = S.far_pair((100, 100, 100))                                 # the far pair: dense refuses, sparse takes it
    lo, hi, h = pts.min(axis=0).astype(np.float64), pts.max(axis=0).astype(np.float64), M.cell_size(pts)
    with pytest.raises(_lib.PuflowHipError, match=r"larger --cell \(or --cell_scale\) or --layout sparse"):
        R.corner_tables(lo, hi, h)
    wdims, wtables = M.grid_of(pts, h)
    for layout in ("sparse", "auto"):
        dims, tables = R.corner_tables(lo, hi, h, layout=layout)
        assert dims == wdims == (483, 483, 483) and all(np.array_equal(a, b) for a, b in zip(tables, wtables))
    dims, _ = R.corner_tables(np.zeros(3), np.ones(3), 1e-3, layout="sparse")        # 1007^3: over the dense cap only
    assert dims == (1007, 1007, 1007)
    for layout in ("dense", "sparse", "auto"):
        with pytest.raises(_lib.PuflowHipError, match="larger --cell"):
            R.corner_tables(np.zeros(3), np.ones(3), 1e-300, layout=layout)
        with pytest.raises(_lib.PuflowHipError, match="larger --cell"):
            R.corner_tables(np.zeros(3), np.ones(3), 1e-7, layout=layout)                # 10^7 corners per axis
    dims, _ = R.corner_tables(np.zeros(3), np.array([1.0, 0.0, 0.0]), 8e-7)         # a long thin box: dense takes what sparse cannot
    assert dims[0] > 1 << 20 and R.corner_tables(np.zeros(3), np.array([1.0, 0.0, 0.0]), 8e-7, layout="auto")[0] == dims
    with pytest.raises(_lib.PuflowHipError, match="larger --cell"):
        R.corner_tables(np.zeros(3), np.array([1.0, 0.0, 0.0]), 8e-7, layout="sparse")
    with pytest.raises(_lib.PuflowHipError, match="layout"):
        R.corner_tables(np.zeros(3), np.ones(3), 0.1, layout="hash")


def test_python_entries_refuse_before_any_device_work(tmp_path):
    import torch
    from puflow_amd import _lib, ops, reconstruct as R
    x = torch.zeros(16, 3)
    with pytest.raises(_lib.PuflowHipError, match="GPU"):
        R.mesh_from_cloud(x, x, layout="sparse")
    with pytest.raises(_lib.PuflowHipError, match="GPU"):
        ops.recon_block_links(torch.zeros(4, dtype=torch.int64), (20, 30, 40))
    with pytest.raises(_lib.PuflowHipError, match="GPU"):
        ops.mtet_count_sparse(torch.zeros(4, 512), torch.zeros(4, 512, dtype=torch.uint8), torch.zeros(4, dtype=torch.int64),
                              torch.zeros(4, 8, dtype=torch.int32), (20, 30, 40))
    (tmp_path / "in").mkdir()
    np.savetxt(tmp_path / "in" / "a.xyz", np.random.default_rng(0).uniform(-1, 1, (50, 6)), fmt="%.6f")
    with pytest.raises(SystemExit):                                      # argparse: not a layout
        R.main(["--source", str(tmp_path / "in"), "--target", str(tmp_path / "out"), "--layout", "hash"])
    assert not (tmp_path / "out").exists()
