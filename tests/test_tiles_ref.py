"""Tiled passes without a GPU: the restated k-d tiling, colouring, quotas and FPS with a context (tests/tiles_ref.py), the host
functions of puflow_amd/tiles.py against them, and the new entry points' binding and argument validation."""
import ctypes

import numpy as np
import pytest
import torch

import tiles_ref as R
from oracle import patch_ref as P
from puflow_amd.weights import synth_patches

NEW = ("pf_fps_ragged_ctx", "pf_box_count", "pf_box_fill", "pf_kd_assign")


def cloud(n, seed):
    return synth_patches(1, n, seed=seed)[0].numpy()


@pytest.mark.parametrize("kind", ["surface", "equal_coordinates"])
def test_kd_tiling_restated(kind):
    """1000 points, tile_points = 128: 8 leaves, sizes within 1 of each other, every point in exactly one leaf, and the descent
    of every input point lands in a cell whose box contains it.  With many equal coordinates (coordinates rounded to halves: fewer than 60
    distinct points among the 1000) the split is still by rank."""
    pc = cloud(1000, 3)
    if kind == "equal_coordinates":
        pc = (np.round(pc * 2) / 2 + 0).astype(np.float32)
        assert len(np.unique(pc, axis=0)) < 60
    order, offsets, (axis, split), boxes = R.kd_tiles(pc, 128)
    assert R.kd_depth(1000, 128) == 3 and len(boxes) == 8 and len(axis) == 7
    sizes = np.diff(offsets)
    assert sizes.sum() == 1000 and sizes.max() - sizes.min() <= 1
    assert np.array_equal(np.sort(order), np.arange(1000))
    for t in range(8):                                                    # a leaf's points lie in its box (faces included)
        p = pc[order[offsets[t]:offsets[t + 1]]]
        assert np.all(p >= boxes[t, :3]) and np.all(p <= boxes[t, 3:])
    leaf = R.kd_descend(pc, axis, split, 3)
    assert np.all(pc >= boxes[leaf, :3]) and np.all(pc <= boxes[leaf, 3:])
    if kind == "surface":                                                 # distinct coordinates: the descent IS the tiling
        tile = np.empty(1000, np.int64)
        tile[order] = np.repeat(np.arange(8), sizes)
        assert np.array_equal(leaf, tile)
    assert R.kd_depth(128, 128) == 0 and R.kd_depth(129, 128) == 1 and R.kd_depth(16384, 4096) == 2
    assert R.kd_depth(16385, 4096) == 3


def test_host_functions_of_the_package_equal_the_restatement():
    from puflow_amd import tiles
    pc = cloud(1000, 5)
    _, _, _, boxes = R.kd_tiles(pc, 64)                                   # 16 leaves
    for n, tp in ((1000, 128), (128, 128), (129, 128), (16385, 4096), (5, 4096)):
        assert tiles.kd_depth(n, tp) == R.kd_depth(n, tp)
    for h in (0.0, 0.05, 0.3, 5.0):
        assert tiles.colour_tiles(boxes.tolist(), h) == R.colour_greedy(boxes, h)
    for a in range(16):
        for b in range(16):
            assert tiles.box_gap2(boxes[a].tolist(), boxes[b].tolist()) == R.box_gap2(boxes[a], boxes[b])
    for npoint, cores in ((8192, [512] * 4), (1001, [3, 3, 3]), (10, [1, 2, 3, 4]), (7, [5, 0, 5]), (4 * 1000 + 24, [125] * 8)):
        q = tiles.quotas(npoint, cores)
        assert q == R.quotas(npoint, cores) and sum(q) == npoint
        assert all(abs(v - npoint * c / sum(cores)) < 1 for v, c in zip(q, cores))


@pytest.mark.parametrize("h", [0.0, 0.05, 0.3, 5.0])
def test_greedy_colouring_separates_conflicting_tiles(h):
    _, _, _, boxes = R.kd_tiles(cloud(1000, 7), 64)
    col = R.colour_greedy(boxes, h)
    con = R.conflicts(boxes, h)
    assert all(col[t] != col[u] for t in range(len(boxes)) for u in con[t])
    if h == 0.0:
        assert set(col) == {0}                                            # nothing is closer than 0
    if h == 5.0:
        assert sorted(col) == list(range(16))                             # everything conflicts


def test_fps_with_an_empty_context_is_the_oracle_fps():
    p = cloud(700, 9)
    p[5] = p[9]
    idx, d = R.fps_ctx(p, 90, None)
    assert np.array_equal(idx, P.fps(torch.from_numpy(p)[None], 90)[0].numpy())
    idx2, _ = R.fps_ctx(p, 90, np.zeros((0, 3), np.float32))
    assert np.array_equal(idx, idx2)
    assert d[0] == np.float32(1e10) and np.all(d[1:] <= d[:-1])
    idx3, d3 = R.fps_ctx(p, 90, cloud(40, 10))
    assert np.all(d3[1:] <= d3[:-1]) and len(set(idx3.tolist())) == 90 and not np.array_equal(idx, idx3)


def test_sequence_with_context_keeps_the_fps_spacing_and_per_cell_fps_does_not():
    """Two cells of a planar cloud (cut at x = 0), 4000 candidates -> 800 samples.  Cell B started from cell A's samples keeps
    every pair at least sqrt(min r2) apart - exactly, in the float32 arithmetic of the kernel - while the two cells sampled on
    their own put points next to each other along the seam."""
    rng = np.random.default_rng(4)
    p = np.concatenate([rng.uniform(-1, 1, (4000, 2)), np.zeros((4000, 1))], 1).astype(np.float32)
    a, b = p[p[:, 0] < 0], p[p[:, 0] >= 0]
    qa, qb = R.quotas(800, [len(a), len(b)])
    ia, da = R.fps_ctx(a, qa)
    ib, db = R.fps_ctx(b, qb, a[ia])                                      # B starts from A's samples
    r2 = min(da[-1], db[-1])
    assert R.min_pair_sqd(np.concatenate([a[ia], b[ib]])) >= r2
    ib0, db0 = R.fps_ctx(b, qb)                                           # the same candidates, B unaware of A
    assert R.min_pair_sqd(np.concatenate([a[ia], b[ib0]])) < min(da[-1], db0[-1])


def test_new_entry_points_are_bound_as_the_header_declares_them():
    from ctypes import c_float, c_int, c_longlong, c_void_p
    from puflow_amd import _lib
    sig = _lib.SIGNATURES
    assert set(NEW) <= set(sig)
    elem = lambda name: [getattr(a, "elem", a) for a in sig[name][1]]
    assert all(sig[n][0] is c_int for n in NEW)
    assert elem("pf_fps_ragged_ctx") == [c_float, c_int, c_int, c_float, c_int, c_int, c_int, c_float, c_int, c_float, c_void_p]
    assert elem("pf_box_count") == [c_float, c_int, c_float, c_int, c_int, c_void_p]
    assert elem("pf_box_fill") == [c_float, c_int, c_float, c_int, c_longlong, c_int, c_void_p]
    assert elem("pf_kd_assign") == [c_float, c_int, c_int, c_float, c_int, c_int, c_void_p]
    with pytest.raises(TypeError):
        sig["pf_fps_ragged_ctx"][1][4].from_param(_lib.offsets([1, 2]))   # c_longlong array for const int* n_ctx


def test_new_entry_points_validate_before_any_launch():
    """Null and shape errors come back as codes from the host side of the library (no GPU is touched: validation precedes the
    first launch)."""
    from puflow_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    c = _lib.counts
    assert lib.pf_fps_ragged_ctx(None, c([300]), c([4]), 8, c([1]), 1, 0, 8, 8, None, None) == -1
    assert lib.pf_fps_ragged_ctx(8, c([300]), c([4]), 8, None, 1, 0, 8, 8, None, None) == -1      # n_ctx is required
    assert lib.pf_fps_ragged_ctx(8, c([300]), c([4]), None, c([2]), 1, 0, 8, 8, None, None) == -1  # a context without points
    assert lib.pf_fps_ragged_ctx(8, c([300]), c([4]), 8, c([-1]), 1, 0, 8, 8, None, None) == -2
    assert lib.pf_fps_ragged_ctx(8, c([300]), c([301]), 8, c([1]), 1, 0, 8, 8, None, None) == -2   # more samples than points
    assert lib.pf_fps_ragged_ctx(8, c([300]), c([4]), 8, c([1]), 1, 0, 12, 8, None, None) == -2    # scratch not 8-byte aligned
    assert lib.pf_box_count(None, 10, 8, 2, 8, None) == -1 and lib.pf_box_count(8, 0, 8, 2, 8, None) == -2
    assert lib.pf_box_count(8, 10, 8, 0, 8, None) == -2
    assert lib.pf_box_fill(8, 10, 8, 2, None, 8, None) == -1 and lib.pf_box_fill(8, 10, 8, 0, 8, 8, None) == -2
    assert lib.pf_kd_assign(8, 10, None, 8, 1, 8, None) == -1 and lib.pf_kd_assign(8, 10, 8, 8, 25, 8, None) == -2
    assert lib.pf_kd_assign(8, 0, 8, 8, 1, 8, None) == -2 and lib.pf_kd_assign(None, 10, None, None, 0, 8, None) == -1
