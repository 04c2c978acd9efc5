"""Band growth at the exits, by its numpy restatement alone (recon_grow_ref over recon_ref): the recorded figures of the clouds
with holes - rounds, exits, open edges, Euler characteristic - as integers; a closed result is an oriented manifold of positive
volume; "no exit left" and "no open edge" coincide; a real rim stays a rim; where nothing grows the padded grid gives the
unpadded mesh bit for bit; and zero rounds are recon_ref itself."""
import functools

import numpy as np
import pytest

import recon_grow_ref as G
import recon_ref as M

F = np.float32

# cloud: (rounds allowed, open edges and V - E + F at R = 0, exits per round (None: not recorded, only their number),
#         rounds that grow, open edges and V - E + F after them, volume or None)
TABLE = {
    "sphere-512-0.7": (8, 32, 1, [12, 8], 2, 0, 2, 4.38),
    "sphere-512-0.9": (8, 34, 1, None, 4, 0, 2, None),
    "sphere-2048-0.4": (8, 40, 1, [16], 1, 0, 2, 4.22),
    "sphere-2048-0.5": (8, 54, 1, None, 5, 0, 2, 4.23),
    "sphere-2048-0.9": (8, 94, 1, None, 8, 42, 1, None),                 # the bound holds: 8 rounds do not close it
    "torus": (8, 42, -1, None, 5, 0, 0, 2.49),
    "disc": (3, 160, 1, None, 3, 208, 1, None),                          # a rim stays a rim
}
POINTS = {"sphere-512-0.7": 454, "sphere-512-0.9": 412, "torus": 1952}


@functools.lru_cache(maxsize=None)
def _meshes(name, rounds):
    pts, nrm = G.cloud(name)
    h = M.cell_size(pts)
    return pts, nrm, h, G.mesh_from_cloud(pts, nrm, h), G.mesh_from_cloud(pts, nrm, h, close_holes=rounds)


@pytest.mark.parametrize("name", list(TABLE))
def test_recorded_figures(name):
    rounds, open0, chi0, exits, grow_rounds, open1, chi1, volume = TABLE[name]
    pts, _nrm, h, (v0, f0, i0), (v1, f1, i1) = _meshes(name, rounds)
    assert len(pts) == POINTS.get(name, len(pts))
    print(f"{name}: {len(pts)} points, h {h:.4f}; R = 0: open {M.open_edges(f0)} euler {M.euler(v0, f0)}; R = {rounds}: exits "
          f"{i1['grown_cells']} open {M.open_edges(f1)} euler {M.euler(v1, f1)} volume {M.volume(v1, f1):.3f} exits left "
          f"{G.exits_left(i1['flags'], i1['f'])}")
    assert (M.open_edges(f0), M.euler(v0, f0)) == (open0, chi0) and i0["grown_cells"] == [] and i0["grow_rounds"] == 0
    assert i1["grow_rounds"] == len(i1["grown_cells"]) == grow_rounds
    if exits is not None:
        assert i1["grown_cells"] == exits
    assert (M.open_edges(f1), M.euler(v1, f1)) == (open1, chi1)
    if open1 == 0:
        assert M.is_oriented_manifold(f1) and M.volume(v1, f1) > 0
    if volume is not None:
        assert abs(M.volume(v1, f1) - volume) < 0.005
    # no exit left <=> no open edge, before and after; the bound case keeps 16 exits
    for faces, info in ((f0, i0), (f1, i1)):
        assert (G.exits_left(info["flags"], info["f"]) == 0) == (M.open_edges(faces) == 0)
    if name == "sphere-2048-0.9":
        assert G.exits_left(i1["flags"], i1["f"]) == 16
    # growth only adds: the R = 0 band, shifted by the padding, is inside the grown one
    r = rounds
    assert (i1["flags"][r:-r, r:-r, r:-r] >= i0["flags"]).all() and i1["flags"].sum() > i0["flags"].sum()
    assert all((b >= a).all() for a, b in zip(i1["history"], i1["history"][1:]))


def test_nothing_to_grow_is_the_unpadded_mesh_bit_for_bit():
    pts, _nrm, h, (v0, f0, i0), (v4, f4, i4) = _meshes("noisy", 4)
    assert M.open_edges(f0) == 0 and i4["grown_cells"] == [] and i4["grow_rounds"] == 0
    assert i4["dims"] == tuple(d + 8 for d in i0["dims"])
    assert v4.tobytes() == v0.tobytes() and f4.tobytes() == f0.tobytes() and len(f0) > 100
    assert np.array_equal(i4["flags"][4:-4, 4:-4, 4:-4], i0["flags"]) and i4["flags"].sum() == i0["flags"].sum()


@pytest.mark.parametrize("name", ["sphere-512-0.7", "disc"])
def test_zero_rounds_are_recon_ref(name):
    pts, nrm, h, (v0, f0, i0), _ = _meshes(name, TABLE[name][0])
    wv, wf, wi = M.mesh_from_cloud(pts, nrm, h)
    assert v0.tobytes() == wv.tobytes() and f0.tobytes() == wf.tobytes() and i0["dims"] == wi["dims"]
    assert np.array_equal(i0["flags"], wi["flags"]) and i0["f"].tobytes() == wi["f"].tobytes()


def test_grid_is_the_old_one_shifted():
    rng = np.random.default_rng(4)
    for _ in range(20):
        lo = rng.uniform(-3, 3, 3).astype(F)
        hi = (lo + rng.uniform(0, 2, 3)).astype(F)
        h = float(rng.uniform(0.01, 0.3))
        dims0, t0 = M.grid(lo, hi, h)
        d, t = G.grid(lo, hi, h)
        assert d == dims0 and all(a.tobytes() == b.tobytes() for a, b in zip(t, t0))
        for r in (1, 5, G.MAX_ROUNDS):
            d, t = G.grid(lo, hi, h, r)
            assert d == tuple(n + 2 * r for n in dims0) and all(a.dtype == F and (np.diff(a) > 0).all() for a in t)
            assert all(a[r:len(a) - r].tobytes() == b.tobytes() for a, b in zip(t, t0))
            assert t[0][0] == F(np.float64(lo[0]) - 3 * h + (0 - r) * h)


def _two_cells(fa, fb):
    """a 3 x 2 x 2 grid (two cells side by side in x): the left cell flagged, values fa on its four outer corners, fb on the shared
    face's four"""
    flags = np.zeros((2, 2, 3), np.uint8)
    flags[:, :, :2] = 1
    f = np.zeros((2, 2, 3), F)
    f[:, :, 0] = fa
    f[:, :, 1] = np.asarray(fb, F).reshape(2, 2)
    return flags, f


def test_the_exit_rule_on_two_cells():
    # the face's corners disagree: the right cell is an exit and puts its 8 corners
    flags, f = _two_cells(1.0, [1.0, -1.0, 1.0, 1.0])
    exits, added = G.grow(flags, f)
    assert exits.sum() == 1 and exits[0, 0, 1] and added[:, :, 1:].all() and not added[:, :, 0].any()
    # they agree (all outside, all inside): the zero set does not cross the face, whatever the far corners say
    for fb in ([1.0] * 4, [-1.0] * 4):
        assert not G.grow(*_two_cells(-3.0, fb))[0].any()
    # -0.0 and +0.0 are both "not inside"
    assert not G.grow(*_two_cells(1.0, [0.0, -0.0, 0.0, 1.0]))[0].any()
    assert G.grow(*_two_cells(1.0, [0.0, -0.0, -1e-30, 1.0]))[0].sum() == 1
    # the neighbour must be active: one of its outer corners unflagged, and nothing is an exit
    flags, f = _two_cells(1.0, [1.0, -1.0, 1.0, 1.0])
    flags[0, 0, 0] = 0
    assert not G.grow(flags, f)[0].any()
    # an active cell is no exit; the last index of an axis is no cell
    flags, f = _two_cells(1.0, [1.0, -1.0, 1.0, 1.0])
    flags[:] = 1
    f[:, :, 2] = [[-1.0, 1.0], [1.0, 1.0]]
    assert not G.grow(flags, f)[0].any()
    # every axis and both sides: the same pair turned and mirrored
    flags, f = _two_cells(1.0, [1.0, -1.0, 1.0, 1.0])
    for axes in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        for flip in (False, True):
            fl, ff = np.transpose(flags, axes), np.transpose(f, axes)
            if flip:
                fl, ff = np.flip(fl, axis=axes.index(2)), np.flip(ff, axis=axes.index(2))
            exits, added = G.grow(np.ascontiguousarray(fl), np.ascontiguousarray(ff))
            assert exits.sum() == 1 and added.sum() == 8


def test_close_stops_when_nothing_is_new_and_keeps_its_inputs():
    flags, f = _two_cells(1.0, [1.0, -1.0, 1.0, 1.0])
    before = flags.copy()
    asked = []

    def value(c):
        asked.append(c.copy())
        return np.ones(len(c), F)
    out_flags, out_f, grown, history = G.close(flags, f, 5, value)
    assert np.array_equal(flags, before) and grown == [1] and len(history) == 1 and out_flags.all()
    assert len(asked) == 1 and np.array_equal(asked[0], [2, 5, 8, 11]) and (out_f[:, :, 2] == 1).all()
