"""Per-point attributes without a GPU: the column plan's grammar, the argument validation of the attribute entry points, and
the float64 restatements (tests/attr_ref.py) that the GPU tests use as their reference - checked here against constructed cases,
against the analytic normals of the test surfaces, and for the share of rows the GPU comparison has to leave out."""
import ctypes

import numpy as np
import pytest

import attr_ref as R


@pytest.fixture(scope="module")
def lib():
    from puflow_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_parse_plan_accepts():
    from puflow_amd.attributes import Segment, has_normal, parse_plan
    plan = parse_plan("normal,lin3,near1")
    assert plan == [Segment("unit", 3), Segment("lin", 3), Segment("near", 1)] and has_normal(plan)
    assert parse_plan("normal,lin3,near1", columns=10) == plan
    assert parse_plan(" lin2 , near1 ", columns=6) == [("lin", 2), ("near", 1)] and not has_normal(parse_plan("lin2"))
    assert sum(s.cols for s in parse_plan("lin13,normal")) == 16                     # the most that is carried
    assert parse_plan("near16", columns=19) == [("near", 16)]


@pytest.mark.parametrize("text,columns", [
    ("normal,lin3,near1", 9), ("normal,lin3,near1", 11), ("lin3", 3),               # a wrong column total
    ("normal,lin1,normal", None),                                                  # normal twice
    ("lin0", None), ("normal,near0", None),                                        # C = 0
    ("lin17", None), ("lin8,normal,near6", None),                                  # more than 16 columns
    ("", None), ("lin", None), ("normal3", None), ("unit3", None), ("lin-1", None), ("lin2;near1", None),
])
def test_parse_plan_rejects(text, columns):
    from puflow_amd.attributes import parse_plan
    with pytest.raises(ValueError):
        parse_plan(text, columns=columns)


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _blend(lib, **kw):
    a = dict(idx=8, d2=8, attr=8, B=1, N=300, M=1000, K=8, C=7, kind=_ints(1, 0, 2), cols=_ints(3, 3, 1), nseg=3, out=8)
    a.update(kw)
    return lib.pf_attr_blend(a["idx"], a["d2"], a["attr"], a["B"], a["N"], a["M"], a["K"], a["C"], a["kind"], a["cols"], a["nseg"],
                             a["out"], None)


def _blend_ragged(lib, **kw):
    a = dict(idx=8, d2=8, attr=8, n=_ints(300, 512), m=_ints(100, 50), B=2, K=8, C=7, kind=_ints(1, 0, 2), cols=_ints(3, 3, 1),
             nseg=3, out=8)
    a.update(kw)
    return lib.pf_attr_blend_ragged(a["idx"], a["d2"], a["attr"], a["n"], a["m"], a["B"], a["K"], a["C"], a["kind"], a["cols"],
                                    a["nseg"], a["out"], None)


def _normals(lib, **kw):
    a = dict(pts=8, idx=8, B=1, M=2048, K=16, view=None, cen=8, normal=8, var=8)
    a.update(kw)
    return lib.pf_normals_pca(a["pts"], a["idx"], a["B"], a["M"], a["K"], a["view"], a["cen"], a["normal"], a["var"], None)


def _normals_ragged(lib, **kw):
    a = dict(pts=8, idx=8, m=_ints(300, 512), B=2, K=16, view=None, cen=8, normal=8, var=8)
    a.update(kw)
    return lib.pf_normals_pca_ragged(a["pts"], a["idx"], a["m"], a["B"], a["K"], a["view"], a["cen"], a["normal"], a["var"], None)


def test_attribute_entry_points_validate_their_arguments_without_gpu(lib):
    """pf_attr_blend, pf_normals_pca and their ragged forms reject bad arguments before touching the device: -1 null pointers,
    -2 shapes, -3 sizes that are not built.  (Every pointer here is the address 8: a call that got past the checks would fault.)"""
    for call, names in ((_blend, ("idx", "d2", "attr", "kind", "cols", "out")),
                        (_blend_ragged, ("idx", "d2", "attr", "n", "m", "kind", "cols", "out")),
                        (_normals, ("pts", "idx", "normal", "var", "cen")),       # cen: required without a viewpoint
                        (_normals_ragged, ("pts", "idx", "m", "normal", "var", "cen"))):
        for name in names:
            assert call(lib, **{name: None}) == -1, (call.__name__, name)
    for call in (_blend, _blend_ragged):
        assert call(lib, K=0) == -3 and call(lib, K=9) == -3
        assert call(lib, C=0) == -3 and call(lib, C=17, cols=_ints(3, 13, 1)) == -3
        assert call(lib, kind=_ints(1, 3, 2)) == -3                                # not a segment kind
        assert call(lib, nseg=0) == -2 and call(lib, nseg=17) == -2
        assert call(lib, cols=_ints(3, 3, 2)) == -2 and call(lib, cols=_ints(3, 2, 1)) == -2     # the columns do not add up to C
        assert call(lib, cols=_ints(3, 0, 4)) == -2                                # an empty segment
        assert call(lib, kind=_ints(0, 1, 2), cols=_ints(2, 4, 1)) == -2           # a unit segment is 3 columns
        assert call(lib, B=0) == -2
    assert _blend(lib, N=0) == -2 and _blend(lib, M=0) == -2 and _blend(lib, N=7) == -2          # K <= N
    assert _blend_ragged(lib, n=_ints(300, 7)) == -2 and _blend_ragged(lib, m=_ints(0, 50)) == -2
    for call in (_normals, _normals_ragged):
        assert call(lib, K=7) == -3 and call(lib, K=65) == -3
        assert call(lib, B=0) == -2
    assert _normals(lib, M=0) == -2 and _normals(lib, M=15) == -2                                # K <= M
    assert _normals_ragged(lib, m=_ints(300, 15)) == -2 and _normals_ragged(lib, m=_ints(300, 0)) == -2
    assert lib.pf_error_string(-3) != lib.pf_error_string(-2)


def test_ops_have_no_cpu_fallback():
    import torch
    from puflow_amd import _lib, attributes, ops
    idx, d2, attr = torch.zeros((1, 4, 2), dtype=torch.int32), torch.ones((1, 4, 2)), torch.ones((1, 5, 1))
    with pytest.raises(_lib.PuflowHipError):
        ops.attr_blend(idx, d2, attr, [(_lib.PF_ATTR_LIN, 1)])
    with pytest.raises(_lib.PuflowHipError):
        ops.attr_blend_ragged(idx[0], d2[0], attr[0], [5], [4], [(_lib.PF_ATTR_LIN, 1)])
    with pytest.raises(_lib.PuflowHipError):
        ops.normals_pca(torch.zeros((1, 16, 3)), torch.zeros((1, 16, 8), dtype=torch.int32))
    with pytest.raises(_lib.PuflowHipError):
        ops.normals_pca_ragged(torch.zeros((16, 3)), torch.zeros((16, 8), dtype=torch.int32), [16])
    with pytest.raises(_lib.PuflowHipError):
        attributes.transfer(torch.zeros((4, 3)), torch.zeros((16, 3)), torch.zeros((16, 2)), "lin2")
    with pytest.raises(_lib.PuflowHipError):
        attributes.estimate_normals(torch.zeros((16, 3)), 8)


def test_blend_restatement_on_constructed_cases():
    attr = np.array([[0, 0, 1, 10.0, 5], [0, 0, -1, 20.0, 6], [1, 0, 0, 40.0, 7]])
    plan = [(R.UNIT, 3), (R.LIN, 1), (R.NEAR, 1)]
    # two neighbours with opposite normals at the same distance do not cancel; lin is their mean; near is neighbour 0's
    out, ln = R.blend(np.array([[0, 1]]), np.array([[0.5, 0.5]]), attr, plan)
    assert np.array_equal(out, [[0, 0, 1, 15.0, 5]]) and ln[0] == 1.0
    # weights 1/d2: d2 = (1, 4) -> 0.8, 0.2
    out, _ = R.blend(np.array([[2, 0]]), np.array([[1.0, 4.0]]), attr, plan)
    assert np.allclose(out, [[0.8 / np.hypot(0.8, 0.2), 0, 0.2 / np.hypot(0.8, 0.2), 34.0, 7]], rtol=0, atol=1e-15)
    # a coincident output point is the input point's row, whatever its other neighbours say
    out, _ = R.blend(np.array([[1, 2]]), np.array([[0.0, 0.25]]), attr, plan)
    assert np.array_equal(out, attr[1:2])
    # neighbour 0 has no direction and the others cancel exactly: neighbour 0's vector
    attr0 = np.array([[0, 0, 0.0], [0.5, 0.25, 1], [-0.5, -0.25, -1]])
    out, _ = R.blend(np.array([[0, 1, 2]]), np.array([[0.5, 1.0, 1.0]]), attr0, [(R.UNIT, 3)])
    assert np.array_equal(out, [[0, 0, 0.0]])


def test_pca_restatement_on_constructed_cases():
    rng = np.random.default_rng(3)
    q = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    flat = np.concatenate([rng.standard_normal((32, 2)), np.zeros((32, 1))], axis=1) @ q.T + 5.0      # a plane with normal q[:, 2]
    n, var, gap = R.pca(flat, np.tile(np.arange(32), (32, 1)))
    assert R.angle(n, np.tile(q[:, 2], (32, 1))).max() < 1e-7 and var.max() < 1e-14 and gap.min() > 0.1
    n, var, gap = R.pca(np.ones((64, 3)), np.tile(np.arange(64), (64, 1)))
    assert np.array_equal(n, np.tile([0, 0, 1.0], (64, 1))) and not var.any() and not gap.any()
    p = np.array([[0, 0, 2.0], [0, 0, -2.0]])
    assert np.array_equal(R.orient(np.array([[0, 0, -1.0], [0, 0, -1.0]]), p), [[0, 0, 1.0], [0, 0, -1.0]])
    assert np.array_equal(R.orient(np.array([[0, 0, -1.0], [0, 0, -1.0]]), p, viewpoint=(0, 0, 5)), [[0, 0, 1.0], [0, 0, 1.0]])


@pytest.mark.parametrize("name,sigma,k", R.PCA_CASES)
def test_pca_cases_keep_their_eigenvalue_gap_and_meet_the_sagitta_bar(name, sigma, k):
    """What the GPU comparison relies on, with the restatement alone: at most 1 % of a case's neighbourhoods have a relative
    eigenvalue gap below 1e-2 (measured: none), and without noise at k = 16 the restated normals are within the chord-sagitta bar
    of the analytic ones (measured mean angle / bar: sphere 0.020 / 0.085 rad, torus 0.058 / 0.267 rad; smallest gap of any case 0.015)."""
    pts, analytic = R.surface(name, sigma)
    idx = R.knn_brute(pts, k)
    n, var, gap = R.pca(pts, idx)
    share = float((gap < R.GAP_MIN).mean())
    print(f"{name} sigma {sigma} k {k}: rows below the gap {share:.4%}, smallest gap {gap.min():.3e}")
    assert share <= R.GAP_SHARE
    assert (var >= 0).all() and (var <= 1 / 3 + 1e-15).all()
    if sigma == 0.0 and k == 16:
        mean, bar = float(R.angle(n, analytic).mean()), R.sagitta_bar(pts, idx, R.SURFACES[name][1])
        print(f"  mean angle to the analytic normal {mean:.4e} rad, chord-sagitta bar {bar:.4e} rad")
        assert mean < bar
