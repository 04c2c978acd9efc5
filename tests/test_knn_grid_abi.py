"""The uniform-grid search's surface without a GPU: pf_knn_grid / pf_knn_grid_ragged reject bad arguments before any device work,
the workspace query is positive and monotone, `search=` takes "brute" or "grid" only, and the CLI refuses --attr_search alone."""
from ctypes import c_int

import pytest


@pytest.fixture(scope="module")
def lib():
    from puflow_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


PTR = 4096                  # a non-null, 16-byte aligned address that is never dereferenced: every call below fails before a launch


def _ws(lib, *n):
    return lib.pf_knn_grid_ws_bytes((c_int * len(n))(*n), len(n))


def _dense(lib, **kw):
    a = dict(ref=PTR, query=PTR, B=2, N=300, M=100, K=8, ws=PTR, ws_bytes=None, idx=PTR, dist=PTR)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(_ws(lib, *[max(a["N"], 1)] * max(a["B"], 1)), 0)
    return lib.pf_knn_grid(a["ref"], a["query"], a["B"], a["N"], a["M"], a["K"], a["ws"], a["ws_bytes"], a["idx"], a["dist"], None)


def _ragged(lib, n=(64, 300, 5000), m=(10, 20, 30), **kw):
    a = dict(ref=PTR, query=PTR, n_arr=(c_int * len(n))(*n), m_arr=(c_int * len(m))(*m), B=len(n), K=8, ws=PTR, ws_bytes=None,
             idx=PTR, dist=PTR)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(_ws(lib, *[max(v, 1) for v in n]), 0)
    return lib.pf_knn_grid_ragged(a["ref"], a["query"], a["n_arr"], a["m_arr"], a["B"], a["K"], a["ws"], a["ws_bytes"], a["idx"], a["dist"],
                                  None)


def test_max_k_is_in_the_header():
    from puflow_amd import _lib
    assert _lib.PF_KNN_GRID_MAX_K == 64 >= _lib.PF_NORMALS_MAX_K and _lib.PF_ATTR_MAX_K <= 64


def test_dense_rejections_without_a_device(lib):
    for name in ("ref", "query", "ws", "idx"):
        assert _dense(lib, **{name: None}) == -1, name
    assert _dense(lib, B=0) == -2 and _dense(lib, N=0) == -2 and _dense(lib, M=0) == -2 and _dense(lib, B=-1) == -2
    assert _dense(lib, K=0) == -3 and _dense(lib, K=65) == -3 and _dense(lib, K=-4) == -3
    assert _dense(lib, N=7, K=8) == -2                                   # K > N
    assert _dense(lib, ws=PTR + 4) == -2                                 # the workspace holds 16-byte records
    need = _ws(lib, 300, 300)
    assert _dense(lib, ws_bytes=need - 1) == -5 and _dense(lib, ws_bytes=0) == -5
    assert _dense(lib, B=3, ws_bytes=need) == -5                         # sized for two clouds


def test_ragged_rejections_without_a_device(lib):
    for name in ("ref", "query", "n_arr", "m_arr", "ws", "idx"):
        assert _ragged(lib, **{name: None}) == -1, name
    assert _ragged(lib, B=0) == -2
    assert _ragged(lib, n=(64, 0, 5000)) == -2 and _ragged(lib, m=(10, 0, 30)) == -2 and _ragged(lib, n=(64, -3, 5000)) == -2
    assert _ragged(lib, K=0) == -3 and _ragged(lib, K=65) == -3
    assert _ragged(lib, n=(63, 300, 5000), K=64) == -2 and _ragged(lib, n=(64, 300, 7), K=8) == -2     # K > one of the clouds
    assert _ragged(lib, ws_bytes=_ws(lib, 64, 300, 5000) - 1) == -5
    assert _ragged(lib, ws_bytes=_ws(lib, 64, 300)) == -5


def test_workspace_is_positive_monotone_and_modest(lib):
    assert lib.pf_knn_grid_ws_bytes(None, 1) == -1
    assert _ws(lib, 0) == -2 and lib.pf_knn_grid_ws_bytes((c_int * 1)(5), 0) == -2
    sizes = [1, 2, 7, 64, 300, 5000, 16384, 20000, 65536, 262144, 1 << 22, 1 << 25]
    got = [_ws(lib, n) for n in sizes]
    assert all(g > 0 and g % 16 == 0 for g in got) and got == sorted(got)
    assert all(_ws(lib, n + 1) >= _ws(lib, n) for n in range(1, 3000))
    assert _ws(lib, 300, 5000) == _ws(lib, 300) + _ws(lib, 5000)
    # at most 2 N cells (rounded up to a cube, 256 per axis at most) of two ints each beside 16 bytes per reference
    for n, g in zip(sizes, got):
        assert g <= 64 + 16 * n + 8 * min((round((2 * n) ** (1 / 3)) + 2) ** 3, 256 ** 3) + 32, n
    # a full ragged launch of 64 clouds of 5000 points: 64 (64 + 80 000 + 8 x 22^3 + 4) bytes = 10.1 MiB; the largest cloud a
    # 32-bit point index times 3 admits with some room, 2^25 points: 512 MiB of references + 128 MiB of cells
    assert _ws(lib, *[5000] * 64) == 64 * ((64 + 16 * 5000 + 8 * 22 ** 3 + 4 + 15) // 16 * 16) < 11 << 20
    assert _ws(lib, 1 << 25) < 700 << 20


def test_search_argument_is_checked_before_any_work():
    import torch
    from puflow_amd import attributes as A
    x, attr = torch.zeros(16, 3), torch.zeros(16, 1)
    assert A.SEARCHES == ("brute", "grid")
    with pytest.raises(ValueError, match="search"):
        A.transfer(x, x, attr, "lin1", search="x")
    with pytest.raises(ValueError, match="search"):
        A.transfer_ragged([x], [x], [attr], "lin1", search="kd")
    with pytest.raises(ValueError, match="search"):
        A.estimate_normals(x, 8, search="")
    with pytest.raises(ValueError, match="search"):
        A.estimate_normals_ragged([x], 8, search=None)


@pytest.mark.parametrize("module", ["upsample", "upsample_cnf"])
def test_cli_refuses_the_flag_alone(module, tmp_path):
    import importlib
    cli = importlib.import_module("puflow_amd." + module)
    argv = ["--source", str(tmp_path), "--target", str(tmp_path / "out"), "--checkpoint", str(tmp_path / "none.pt")]
    with pytest.raises(SystemExit, match="--attr_search goes with"):
        cli.main(argv + ["--attr_search", "grid"])
    assert not (tmp_path / "out").exists()                               # refused before anything is made
    with pytest.raises(SystemExit):                                      # argparse: not a search
        cli.main(argv + ["--attributes", "lin1", "--attr_search", "kd"])
