"""Band growth's surface without a GPU: pf_recon_grow's prototype and PF_RECON_GROW_MAX_ROUNDS as the header states them, the
entry rejecting bad arguments before any device work, the padded grid rule of puflow_amd.reconstruct against the restatement's,
the host's exit count against the restatement's exits, and the refusals of the Python entries and the CLI."""
import ctypes
import os
import re

import numpy as np
import pytest

import recon_grow_ref as G
import recon_ref as M

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "puflow_hip.h")


@pytest.fixture(scope="module")
def lib():
    from puflow_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


PTR = 4096                  # a non-null address that is never dereferenced: every call below fails before a launch


def _grow(lib, **kw):
    a = dict(f=PTR, flags=PTR, D=(20, 30, 40), added=PTR)
    a.update(kw)
    return lib.pf_recon_grow(a["f"], a["flags"], *a["D"], a["added"], None)


def test_prototype_and_constant_are_the_headers():
    from puflow_amd import _lib, reconstruct as R
    text = open(HEADER).read()
    assert re.search(r"^#define PF_RECON_GROW_MAX_ROUNDS 64$", text, flags=re.M)
    assert ("int pf_recon_grow(const float* f, const unsigned char* flags, int Dx, int Dy, int Dz, unsigned char* added, "
            "void* stream);") in text
    assert _lib.PF_RECON_GROW_MAX_ROUNDS == R.GROW_MAX_ROUNDS == G.MAX_ROUNDS == 64
    res, args = _lib.SIGNATURES["pf_recon_grow"]
    assert res is ctypes.c_int and len(args) == 7
    assert [a.elem for a in args[:2]] == [ctypes.c_float, ctypes.c_ubyte] and args[2:5] == [ctypes.c_int] * 3
    assert args[5].elem is ctypes.c_ubyte and args[6] is ctypes.c_void_p
    # the rule is stated in the header: the words the restatement and the kernel follow
    for words in ("an inactive cell c (not on the last index of any axis)", "the neighbour is ACTIVE (all 8 of its corners flagged)",
                  "not all agree in f < 0", "new = added & ~flags", "D_a = ceil((hi_a - lo_a) / h) + 7 + 2 R",
                  "g_a[i] = float32(o_a + (i - R) h)"):
        assert words in " ".join(text.replace(" * ", " ").split()), words


def test_bad_arguments_fail_before_any_device_work(lib):
    for name in ("f", "flags", "added"):
        assert _grow(lib, **{name: None}) == -1, name
    for D in ((1, 30, 40), (20, 1, 40), (20, 30, 1), (0, 30, 40), (20, -3, 40)):
        assert _grow(lib, D=D) == -2, D
    assert _grow(lib, D=(1024, 1024, 65)) == -3 and _grow(lib, D=(1 << 15, 1 << 15, 1 << 15)) == -3
    with pytest.raises(ctypes.ArgumentError):                            # the binding knows the pointees
        lib.pf_recon_grow((ctypes.c_int * 4)(), PTR, 20, 30, 40, PTR, None)


def test_padded_grid_rule_is_the_restatements():
    from puflow_amd import reconstruct as R
    rng = np.random.default_rng(4)
    for _ in range(20):
        lo = rng.uniform(-3, 3, 3).astype(np.float32)
        hi = (lo + rng.uniform(0, 2, 3)).astype(np.float32)
        h = float(rng.uniform(0.01, 0.3))
        for rounds in (0, 1, 7, 64):
            dims, tables = R.corner_tables(lo.astype(np.float64), hi.astype(np.float64), h, rounds=rounds)
            wdims, wtables = G.grid(lo, hi, h, rounds)
            assert dims == wdims and all(a.dtype == np.float32 and a.tobytes() == b.tobytes() for a, b in zip(tables, wtables))
        dims, tables = R.corner_tables(lo.astype(np.float64), hi.astype(np.float64), h, layout="auto", rounds=3)
        assert dims == G.grid(lo, hi, h, 3)[0]
    assert R.corner_tables(np.zeros(3), np.zeros(3), 0.5, rounds=2)[0] == (11, 11, 11)


def _born(history, start):
    """the round that flagged a corner (0: the band, 127: never) from the flags after every round"""
    born = np.where(start != 0, 0, 127).astype(np.int8)
    before = start
    for r, flags in enumerate(history, 1):
        born[(flags != 0) & (before == 0)] = r
        before = flags
    return born


def test_host_exit_count_is_the_restatements(monkeypatch):
    """reconstruct._exits counts after the last round, from every round's new corners and the round that flagged each corner,
    what the restatement's grow() calls exits round by round (torch on the CPU)"""
    import torch
    from puflow_amd import reconstruct as R
    total = 0
    for seed, density in ((1, 0.85), (2, 0.6), (3, 0.95)):                # one round on random fields
        f, flags = G.random_field(seed, density=density)
        exits, added = G.grow(flags, f)
        act = M.active_cells(flags)
        assert act[-2, -2, -2] and act[0, 0, 0] and exits.sum() > 10
        born = _born([flags | added], flags)
        got = R._exits(torch.from_numpy(f), torch.from_numpy(born), [torch.from_numpy(np.flatnonzero(born.reshape(-1) == 1))])
        assert got == [int(exits.sum())], (seed, got, int(exits.sum()))
        total += got[0]
    assert total > 100
    # every round of a cloud with a hole at once, in one pass and in passes of 7 corners
    pts, nrm = G.cloud("sphere-512-0.7")
    h = M.cell_size(pts)
    _, _, info = G.mesh_from_cloud(pts, nrm, h, close_holes=4)
    born = _born(info["history"], M.mark(pts, info["tables"]))
    corners = [torch.from_numpy(np.flatnonzero(born.reshape(-1) == r)) for r in (1, 2)]
    assert info["grown_cells"] == [12, 8] and R._exits(torch.from_numpy(info["f"]), torch.from_numpy(born), corners) == [12, 8]
    monkeypatch.setattr(R, "EXITS_CHUNK", 7)
    assert R._exits(torch.from_numpy(info["f"]), torch.from_numpy(born), corners) == [12, 8]


def test_refusals_by_name():
    from puflow_amd import _lib, reconstruct as R
    lo, hi = np.zeros(3), np.ones(3)
    for bad in (-1, 65, 2.0, "2", None, True):
        with pytest.raises(_lib.PuflowHipError, match="close_holes"):
            R.corner_tables(lo, hi, 0.1, rounds=bad)
    with pytest.raises(_lib.PuflowHipError, match="close_holes = 2: growth needs the dense layout"):
        R.corner_tables(lo, hi, 0.1, layout="sparse", rounds=2)
    # 406^3 corners are under the dense cap, 408^3 are over it: one round of padding is refused, by name, also under "auto"
    assert R.corner_tables(lo, 399 * hi, 1.0)[0] == (406, 406, 406) and 406 ** 3 <= _lib.PF_RECON_MAX_CORNERS < 408 ** 3
    for layout in ("dense", "auto"):
        with pytest.raises(_lib.PuflowHipError, match=r"close_holes = 1: growth needs the dense layout.*408 x 408 x 408"):
            R.corner_tables(lo, 399 * hi, 1.0, layout=layout, rounds=1)
    assert R.corner_tables(lo, 399 * hi, 1.0, layout="auto")[0] == (406, 406, 406)


def test_cli_takes_whole_numbers_only(tmp_path):
    from puflow_amd import reconstruct as R
    (tmp_path / "in").mkdir()
    np.savetxt(tmp_path / "in" / "a.xyz", np.random.default_rng(0).uniform(-1, 1, (50, 6)), fmt="%.6f")
    for bad in ("x", "1.5"):
        with pytest.raises(SystemExit):
            R.main(["--source", str(tmp_path / "in"), "--target", str(tmp_path / "out"), "--close_holes", bad])
    assert not (tmp_path / "out").exists()
