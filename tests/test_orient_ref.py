"""CPU: the numpy restatement of pf_normals_orient (orient_ref) does what the feature is for.  PCA normals (attr_ref.pca) with
scrambled signs over brute-force neighbour lists come out with ZERO rows opposed to the analytic normals on the torus and on two
spheres, where the per-point centroid rule leaves more than a fifth of the torus opposed; the result does not depend on the signs
that came in, and a far viewpoint on -z picks the mirror seed."""
import numpy as np
import pytest

import attr_ref as R
import orient_ref as O

TORI = [(n, k, sigma) for n in (512, 2048) for k in (8, 16) for sigma in (0.0, 0.002, 0.01)]


def _pca(pts, k):
    idx = R.knn_brute(pts, k)
    return idx, R.pca(pts, idx)[0].astype(np.float32)


@pytest.mark.parametrize("n,k,sigma", TORI)
def test_torus_is_one_component_with_no_row_opposed(n, k, sigma):
    pts, analytic = R.torus(n, 12, sigma)
    idx, normal = _pca(pts, k)
    out, comp = O.orient(pts, O.scramble(normal, n + k), idx)
    assert O.opposed(out, analytic) == 0
    assert (comp == 0).all()
    assert np.array_equal(np.abs(out), np.abs(normal))                  # rows kept or negated, nothing else
    # the reason the feature exists: every point on its own, away from the centroid, turns the inner ring the wrong way
    assert O.opposed(R.orient(normal, pts), analytic) > n / 5


@pytest.mark.parametrize("nested", [False, True])
def test_two_spheres_are_two_components_both_outwards(nested):
    pts, analytic = O.two_spheres(nested)
    idx, normal = _pca(pts, 16)
    out, comp = O.orient(pts, O.scramble(normal, 3), idx)
    assert O.opposed(out, analytic) == 0
    assert set(np.unique(comp)) == {0, 600} and (comp[:600] == 0).all() and (comp[600:] == 600).all()
    if not nested:
        assert O.opposed(R.orient(normal, pts), analytic) > 100           # the centroid lies between the two


def test_the_input_signs_do_not_matter():
    pts, _ = R.torus(512, 12, 0.002)
    idx, normal = _pca(pts, 8)
    a, ca = O.orient(pts, normal, idx)
    for seed in (1, 2):
        b, cb = O.orient(pts, O.scramble(normal, seed), idx)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(ca, cb)
    c, _ = O.orient(pts, -normal, idx, viewpoint=(0.3, -0.2, 40.0))
    d, _ = O.orient(pts, normal, idx, viewpoint=(0.3, -0.2, 40.0))
    assert np.array_equal(c.view(np.uint32), d.view(np.uint32))


def test_a_far_viewpoint_below_gives_the_mirror_seed():
    """seen from far on -z the seed is the LOWEST point and looks down: on a closed piece that is outwards again, the same
    normals as without a viewpoint; on an open cap it is the opposite of them"""
    pts, analytic = R.torus(512, 12, 0.0)
    idx, normal = _pca(pts, 8)
    up, _ = O.orient(pts, normal, idx)
    down, _ = O.orient(pts, normal, idx, viewpoint=(0.0, 0.0, -1000.0))
    assert np.array_equal(up.view(np.uint32), down.view(np.uint32)) and O.opposed(down, analytic) == 0
    sp, sn = R.sphere(2048, 11)
    cap = sp[sp[:, 2] > 0.6]                                             # an open cap: no inside, the seed decides
    cidx, cnormal = _pca(cap, 8)
    cup, ccomp = O.orient(cap, cnormal, cidx)
    cdown, _ = O.orient(cap, cnormal, cidx, viewpoint=(0.0, 0.0, -1000.0))
    assert (ccomp == 0).all()
    assert O.opposed(cup, sn[sp[:, 2] > 0.6]) == 0
    assert np.array_equal(cdown, -cup)
    lowest = int(np.argmin(((cap.astype(np.float32) - np.array([0, 0, -1000], np.float32)) ** 2).sum(axis=1)))
    assert cdown[lowest, 2] < 0 and cup[int(np.argmax(cap[:, 2])), 2] > 0


def test_ties_are_decided_by_the_indices():
    """all weights exactly 0 on a planar grid with normals (0, 0, +-1): the forest is the index order's, and every row ends up"""
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), indexing="ij"), axis=-1).reshape(-1, 2)
    pts = np.concatenate([g, np.zeros((256, 1))], axis=1).astype(np.float32)
    normal = O.scramble(np.tile(np.array([0, 0, 1], np.float32), (256, 1)), 5)
    idx = R.knn_brute(pts, 5)
    a, b, d, _ = O.forest(normal, idx)
    assert len(a) == 255 and (np.abs(d) == 1).all()
    out, comp = O.orient(pts, normal, idx)
    assert (out == np.array([0, 0, 1], np.float32)).all() and (comp == 0).all()
