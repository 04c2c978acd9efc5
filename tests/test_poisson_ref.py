"""Weighted sample elimination without a GPU: the phase / round form the kernels run (tests/poisson_ref.py) leaves the set the
sequential definition leaves, the parameters have their known values, bad arguments are refused before any device work, and
the kept set is blue noise."""
import ctypes
import math

import numpy as np
import pytest

import poisson_ref as R

POOLS = [(64, 16, False), (600, 120, True), (1280, 256, False), (1280, 1279, False), (300, 1, False), (2560, 512, False)]
_GRAPHS = {}


def pool_graph(s, m, triple):
    """(points, offsets, nbr, q) of a unit-square pool, made once and never written to."""
    key = (s, m, triple)
    if key not in _GRAPHS:
        p = R.square_pool(s, seed=100 + s + m, triple=triple)
        g = R.neighbour_graph(p, 1.0, m)
        for a in (p,) + g:
            a.setflags(write=False)
        _GRAPHS[key] = (p,) + g
    return _GRAPHS[key]


@pytest.mark.parametrize("s,m,triple", POOLS)
def test_phase_form_keeps_the_sequential_set(s, m, triple):
    _, offsets, nbr, q = pool_graph(s, m, triple)
    seq = R.eliminate_sequential(offsets, nbr, q, m)
    par, phases, rounds = R.eliminate_phases(offsets, nbr, q, m)
    print(f"s {s} m {m}: {phases} phases, {rounds} rounds")
    assert len(seq) == m and np.array_equal(seq, par)
    assert 1 <= phases <= rounds <= s - m


def test_graph_is_symmetric_and_the_triple_is_mutual():
    p, offsets, nbr, q = pool_graph(600, 120, True)
    rows = np.repeat(np.arange(600), np.diff(offsets))
    fwd = {(int(i), int(j)): int(v) for i, j, v in zip(rows, nbr, q)}
    assert all(fwd[(j, i)] == v for (i, j), v in fwd.items())
    top = max(fwd.values())
    assert fwd[(0, 1)] == fwd[(0, 2)] == fwd[(1, 2)] == top            # coincident points: d = 0 is held at 2 r_min
    assert 0 < top <= 65536


def test_elimination_params_known_values():
    from puflow_amd.sampling import elimination_params
    r_max, r_min = elimination_params(1.0, 1280, 256)
    assert r_max == pytest.approx(math.sqrt(1.0 / (2.0 * math.sqrt(3.0) * 256.0)), rel=1e-15)
    assert r_max == pytest.approx(0.0335803104, rel=1e-8)
    assert r_min == pytest.approx(r_max * (1.0 - 0.2 ** 1.5) * 0.65, rel=1e-14)
    assert r_min == pytest.approx(0.0198749175, rel=1e-8)
    assert elimination_params(4.0, 10, 10)[1] == 0.0                     # nothing to remove: no weight limiting
    assert elimination_params(4.0, 1280, 256)[0] == pytest.approx(2.0 * r_max, rel=1e-15)
    assert (r_max, r_min) == R.elimination_params(1.0, 1280, 256)
    # the library's host function: the same doubles, and the three fp32 constants of the kernels
    from puflow_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    a, b, c = ctypes.c_double(), ctypes.c_double(), (ctypes.c_float * 3)()
    assert lib.pf_poisson_params(1.0, 1280, 256, ctypes.byref(a), ctypes.byref(b), c) == 0
    assert (a.value, b.value) == (r_max, r_min)
    assert tuple(np.float32(v) for v in c) == R.constants(1.0, 1280, 256)


def test_bad_arguments_are_refused():
    from puflow_amd import _lib, build
    from puflow_amd.sampling import elimination_params
    for area, s, m in ((1.0, 10, 11), (1.0, 10, 0), (-1.0, 10, 5), (0.0, 10, 5), (float("nan"), 10, 5)):
        with pytest.raises(ValueError):
            elimination_params(area, s, m)
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.pf_poisson_params(1.0, 10, 11, None, None, None) == -2
    assert lib.pf_poisson_params(1.0, 10, 0, None, None, None) == -2
    assert lib.pf_poisson_params(-1.0, 10, 5, None, None, None) == -2
    table = (_lib.PfPoissonPool * 2)()
    one = (ctypes.c_double * 2)(1.0, 1.0)
    assert lib.pf_poisson_pools(None, None, None, 2, 0, None) == -1
    assert lib.pf_poisson_pools(_lib.counts([10, 20]), _lib.counts([5, 21]), one, 2, 0, table) == -2
    assert lib.pf_poisson_pools(_lib.counts([10, 0]), _lib.counts([5, 0]), one, 2, 0, table) == -2
    assert lib.pf_poisson_pools(_lib.counts([10, 9000]), _lib.counts([5, 100]), one, 2, 0, table) == 0
    assert (table[1].off, table[1].out_off, table[0].path, table[1].path) == (10, 5, 1, 0)
    assert lib.pf_poisson_degree(None, None, 1, 8, 8, None, None, None) == -1
    assert lib.pf_poisson_degree(8, 8, 0, 8, 8, 8, 8, None) == -2
    assert lib.pf_poisson_rounds(8, 1, 8, 8, 8, 8, 8, 8, 8, 8, 8, 0, 0, 8, None) == -2     # no rounds asked for
    import torch
    from puflow_amd.sampling import eliminate
    with pytest.raises(_lib.PuflowHipError):
        eliminate(torch.zeros(10, 3), [10], [5], [1.0])                  # a CPU tensor: no fallback


def test_kept_set_is_blue_noise():
    """std / mean of the nearest-neighbour distance: the kept 256 of 1280 at most half that of a random 256 of the same pool."""
    p, offsets, nbr, q = pool_graph(1280, 256, False)
    kept = R.eliminate_sequential(offsets, nbr, q, 256)
    rand = np.random.default_rng(7).choice(1280, 256, replace=False)
    cv_kept, cv_rand = R.nn_distance_cv(p[kept]), R.nn_distance_cv(p[rand])
    print(f"nearest-neighbour distance std/mean: kept {cv_kept:.3f}, random {cv_rand:.3f}")
    assert cv_kept <= 0.5 * cv_rand
