"""The triangle grid's surface without a GPU: pf_point_mesh_grid / _count / _ws_bytes are declared in the header, pass the export
map and are bound from the header's types; they reject bad arguments before any device work; the workspace query is positive and
monotone; `search=` takes "tiles" or "grid" only and refuses brute force over the grid; the CLIs know the switch."""
import ctypes
import re

import pytest

NEW = ("pf_point_mesh_grid_ws_bytes", "pf_point_mesh_grid_count", "pf_point_mesh_grid")
PTR = 4096                  # a non-null, 16-byte aligned address that is never dereferenced: every call below fails before a launch


@pytest.fixture(scope="module")
def lib():
    from puflow_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    from puflow_amd import _abi, build
    _, _, sigs = _abi.header()
    with open(build.EXPORTS) as f:
        glob = re.search(r"global:\s*([\w*]+)\s*;", f.read()).group(1)
    for name in NEW:
        assert name in sigs and name.startswith(glob[:-1]), name
        fn = getattr(lib, name)
        assert fn.restype is sigs[name][0] and list(fn.argtypes) == sigs[name][1], name
    assert sigs[NEW[0]][0] is ctypes.c_longlong and sigs[NEW[1]][0] is ctypes.c_int and sigs[NEW[2]][0] is ctypes.c_int
    el = lambda ts: [getattr(t, "elem", t) for t in ts]      # noqa: E731
    assert el(sigs[NEW[0]][1]) == [ctypes.c_int, ctypes.c_int, ctypes.c_longlong]
    assert el(sigs[NEW[1]][1]) == [ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p]
    assert el(sigs[NEW[2]][1]) == [ctypes.c_float, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p]
    # the tiles search beside it: the same leading arguments but `brute`
    assert el(sigs["pf_point_mesh_dist"][1])[:5] == el(sigs[NEW[2]][1])[:5]
    assert "tri_grid.hip" in build.SOURCES


def _search(lib, **kw):
    a = dict(pts=PTR, P=100, tris=PTR, F=300, seed=None, dist=PTR, face=None, cand=None, ws=PTR, ws_bytes=None, pairs=1000)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(lib.pf_point_mesh_grid_ws_bytes(max(a["P"], 1), max(a["F"], 1), min(max(a["pairs"], 0), 1 << 30)), 0)
    return lib.pf_point_mesh_grid(a["pts"], a["P"], a["tris"], a["F"], a["seed"], a["dist"], a["face"], a["cand"], a["ws"],
                                  a["ws_bytes"], a["pairs"], None)


def _count(lib, **kw):
    a = dict(tris=PTR, F=300, ws=PTR, ws_bytes=None, info=PTR)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(lib.pf_point_mesh_grid_ws_bytes(1, max(a["F"], 1), 0), 0)
    return lib.pf_point_mesh_grid_count(a["tris"], a["F"], a["ws"], a["ws_bytes"], a["info"], None)


def test_search_rejections_without_a_device(lib):
    for name in ("pts", "tris", "dist", "ws"):
        assert _search(lib, **{name: None}) == -1, name
    assert _search(lib, P=0) == -2 and _search(lib, P=-3) == -2 and _search(lib, F=0) == -2 and _search(lib, F=-1) == -2
    assert _search(lib, P=(1 << 26) + 1) == -2 and _search(lib, F=(1 << 28) + 1) == -2        # pf_point_mesh_dist's caps
    assert _search(lib, pairs=-1) == -2 and _search(lib, ws=PTR + 4) == -2
    assert _search(lib, pairs=1 << 31) == -3                             # more pairs than an int holds
    need = lib.pf_point_mesh_grid_ws_bytes(100, 300, 1000)
    assert _search(lib, ws_bytes=need - 1) == -5 and _search(lib, ws_bytes=0) == -5
    assert _search(lib, pairs=2000, ws_bytes=need) == -5                 # sized for fewer pairs


def test_count_rejections_without_a_device(lib):
    for name in ("tris", "ws", "info"):
        assert _count(lib, **{name: None}) == -1, name
    assert _count(lib, F=0) == -2 and _count(lib, F=-1) == -2 and _count(lib, ws=PTR + 8) == -2
    assert _count(lib, ws_bytes=lib.pf_point_mesh_grid_ws_bytes(1, 300, 0) - 1) == -5


def test_workspace_is_positive_monotone_and_modest(lib):
    ws = lib.pf_point_mesh_grid_ws_bytes
    assert ws(0, 10, 0) == -2 and ws(10, 0, 0) == -2 and ws(10, -1, 0) == -2 and ws(10, 10, -1) == -2
    assert ws(10, 10, 1 << 31) == -3 and ws(10, 10, (1 << 31) - 1) > 0
    sizes = [1, 2, 7, 64, 300, 5000, 102400, 10 ** 6, 5 * 10 ** 6, 1 << 28]
    got = [ws(8192, F, 4 * F) for F in sizes]
    assert all(g > 0 and g % 16 == 0 for g in got) and got == sorted(got)
    assert ws(1, 300, 1000) == ws(1 << 20, 300, 1000)                    # nothing per query
    assert ws(1, 300, 2000) - ws(1, 300, 1000) == 4000                   # one int per pair
    # header + two ints per cell (at most 2 F cells rounded up to a cube, 256 per axis at most) + one int per triangle and pair
    for F, g in zip(sizes, got):
        assert g <= 96 + 8 * min((round((2 * F) ** (1 / 3)) + 2) ** 3, 256 ** 3) + 4 + 4 * F + 16 * F + 16, F


def test_search_argument_is_checked_before_any_work():
    import torch
    from puflow_amd import metrics
    x, f = torch.zeros(8, 3), torch.zeros(4, 3, dtype=torch.long)
    assert metrics.P2F_SEARCHES == ("tiles", "grid")
    with pytest.raises(ValueError, match="search"):
        metrics.point_to_mesh_distance(x, x, f, search="bvh")
    with pytest.raises(ValueError, match="brute"):
        metrics.point_to_mesh_distance(x, x, f, brute=True, search="grid")


def test_clis_know_the_switch(tmp_path):
    from puflow_amd import evaluate, evaluate_mesh, mesh_metrics
    argv = ["--pred", str(tmp_path), "--gt", str(tmp_path), "--save_path", str(tmp_path / "out")]
    with pytest.raises(SystemExit):                                      # argparse: not a search
        evaluate.main(argv + ["--p2f_search", "bvh"])
    with pytest.raises(SystemExit):
        evaluate_mesh.main(argv + ["--search", "bvh"])
    with pytest.raises(ValueError, match="p2f_search"):
        evaluate.evaluate(str(tmp_path), str(tmp_path), str(tmp_path / "out"), p2f_search="bvh")
    assert not (tmp_path / "out").exists()
    assert mesh_metrics.COLUMNS[0] == "name" and "fscore" in mesh_metrics.COLUMNS
    (tmp_path / "a.off").write_text("OFF\n0 0 0\n")
    both, alone = evaluate_mesh.pair_paths(str(tmp_path), str(tmp_path / "none"))
    assert both == [] and alone == [("a", str(tmp_path))]
