"""The normal orientation's surface without a GPU: pf_normals_orient / pf_normals_orient_ragged reject bad arguments before any
device work, the workspace query is positive and monotone, `orient=` takes "point" or "propagate" only, and the CLI refuses
--normals_orient alone."""
from ctypes import c_int

import pytest


@pytest.fixture(scope="module")
def lib():
    from puflow_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


PTR = 4096                  # a non-null, 16-byte aligned address that is never dereferenced: every call below fails before a launch


def _ws(lib, *m):
    return lib.pf_normals_orient_ws_bytes((c_int * len(m))(*m), len(m))


def _dense(lib, **kw):
    a = dict(pts=PTR, normal_in=PTR, idx=PTR, B=2, M=300, K=8, view=None, ws=PTR, ws_bytes=None, out=PTR, comp=PTR)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(_ws(lib, *[max(a["M"], 1)] * max(a["B"], 1)), 0)
    return lib.pf_normals_orient(a["pts"], a["normal_in"], a["idx"], a["B"], a["M"], a["K"], a["view"], a["ws"], a["ws_bytes"], a["out"],
                                 a["comp"], None)


def _ragged(lib, m=(64, 300, 5000), **kw):
    a = dict(pts=PTR, normal_in=PTR, idx=PTR, m_arr=(c_int * len(m))(*m), B=len(m), K=8, view=None, ws=PTR, ws_bytes=None, out=PTR,
             comp=PTR)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(_ws(lib, *[max(v, 1) for v in m]), 0)
    return lib.pf_normals_orient_ragged(a["pts"], a["normal_in"], a["idx"], a["m_arr"], a["B"], a["K"], a["view"], a["ws"], a["ws_bytes"],
                                        a["out"], a["comp"], None)


def test_dense_rejections_without_a_device(lib):
    for name in ("pts", "normal_in", "idx", "ws", "out"):
        assert _dense(lib, **{name: None}) == -1, name
    assert _dense(lib, B=0) == -2 and _dense(lib, M=0) == -2 and _dense(lib, B=-1) == -2
    assert _dense(lib, K=1) == -3 and _dense(lib, K=0) == -3 and _dense(lib, K=65) == -3 and _dense(lib, K=-4) == -3
    assert _dense(lib, M=7, K=8) == -2                                   # K > M
    assert _dense(lib, ws=PTR + 4) == -2                                 # the workspace starts with 8-byte records
    need = _ws(lib, 300, 300)
    assert _dense(lib, ws_bytes=need - 1) == -5 and _dense(lib, ws_bytes=0) == -5
    assert _dense(lib, B=3, ws_bytes=need) == -5                         # sized for two clouds


def test_ragged_rejections_without_a_device(lib):
    for name in ("pts", "normal_in", "idx", "m_arr", "ws", "out"):
        assert _ragged(lib, **{name: None}) == -1, name
    assert _ragged(lib, B=0) == -2
    assert _ragged(lib, m=(64, 0, 5000)) == -2 and _ragged(lib, m=(64, -3, 5000)) == -2
    assert _ragged(lib, K=1) == -3 and _ragged(lib, K=65) == -3
    assert _ragged(lib, m=(63, 300, 5000), K=64) == -2 and _ragged(lib, m=(64, 300, 7), K=8) == -2     # K > one of the clouds
    assert _ragged(lib, ws_bytes=_ws(lib, 64, 300, 5000) - 1) == -5
    assert _ragged(lib, ws_bytes=_ws(lib, 64, 300)) == -5


def test_workspace_is_positive_monotone_and_modest(lib):
    assert lib.pf_normals_orient_ws_bytes(None, 1) == -1
    assert _ws(lib, 0) == -2 and lib.pf_normals_orient_ws_bytes((c_int * 1)(5), 0) == -2
    sizes = [1, 2, 7, 64, 300, 5000, 16384, 20000, 65536, 262144, 1 << 22, 1 << 25]
    got = [_ws(lib, m) for m in sizes]
    assert all(g > 0 and g % 16 == 0 for g in got) and got == sorted(got)
    assert all(_ws(lib, m + 1) >= _ws(lib, m) for m in range(1, 3000))
    # one forest over the packed tensor: the sum of the clouds decides, 37 bytes per point and the round flags
    assert _ws(lib, 300, 5000) == _ws(lib, 5300)
    assert all(37 * m <= g <= 37 * m + 256 + 16 for m, g in zip(sizes, got))


def test_orient_argument_is_checked_before_any_work():
    import torch
    from puflow_amd import attributes as A
    x = torch.zeros(16, 3)
    assert A.ORIENTS == ("point", "propagate")
    with pytest.raises(ValueError, match="orient"):
        A.estimate_normals(x, 8, orient="mst")
    with pytest.raises(ValueError, match="orient"):
        A.estimate_normals_ragged([x], 8, orient="")
    with pytest.raises(ValueError, match="orient"):
        A.estimate_normals(x, 8, search="grid", orient=None)
    with pytest.raises(ValueError, match="search"):
        A.orient_normals(x, x, 8, search="kd")
    with pytest.raises(ValueError, match="search"):
        A.orient_normals_ragged([x], [x], 8, search="kd")


@pytest.mark.parametrize("module", ["upsample", "upsample_cnf"])
def test_cli_refuses_the_flag_alone(module, tmp_path):
    import importlib
    cli = importlib.import_module("puflow_amd." + module)
    argv = ["--source", str(tmp_path), "--target", str(tmp_path / "out"), "--checkpoint", str(tmp_path / "none.pt")]
    for value in ("propagate", "point"):
        with pytest.raises(SystemExit, match="--normals_orient goes with --estimate_normals"):
            cli.main(argv + ["--normals_orient", value])
    with pytest.raises(SystemExit, match="--estimate_normals"):
        cli.main(argv + ["--attributes", "lin1", "--normals_orient", "propagate"])
    assert not (tmp_path / "out").exists()                               # refused before anything is made
    with pytest.raises(SystemExit):                                      # argparse: not a rule
        cli.main(argv + ["--estimate_normals", "16", "--normals_orient", "mst"])


def test_library_entry_refuses_the_option_alone(tmp_path):
    from puflow_amd import upsample as U
    with pytest.raises(SystemExit, match="--estimate_normals"):
        U.upsampling([], str(tmp_path), str(tmp_path / "none.pt"), 4, 24, 256, normals_orient="propagate")
    with pytest.raises(SystemExit, match="--normals_orient"):
        U.upsampling([], str(tmp_path), str(tmp_path / "none.pt"), 4, 24, 256, estimate_normals=16, normals_orient="mst")
