"""The evaluation metrics' restatements (tests/eval_ref.py) against the reference's scoring step (tests/golden/eval_*.npz,
tools/make_golden_eval.py), the OFF reader, and argument validation of the new entry points - no GPU needed."""
import os

import numpy as np
import pytest

import eval_ref as R


@pytest.fixture(scope="module")
def built_lib():
    from puflow_amd import build
    return build.build(verbose=False)


def test_approx_match_restatement_matches_reference_cpu_op(golden_dir):
    g = np.load(os.path.join(golden_dir, "eval_emd.npz"))
    for k in g["cases"]:
        ref = float(g[f"{k}_cost8"])
        got = R.approx_match_cost(g[f"{k}_a"], g[f"{k}_b"], top=8)
        assert abs(got - ref) <= 1e-6 * abs(ref), (k, got, ref)


def test_jsd_restatement_matches_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "eval_jsd.npz"))
    for i in range(int(g["npairs"])):
        ca = R.occupancy(R.normalize(g[f"j{i}_a"]) * 0.5)
        cb = R.occupancy(R.normalize(g[f"j{i}_b"]) * 0.5)
        np.testing.assert_array_equal(ca, g[f"j{i}_count_a"])
        np.testing.assert_array_equal(cb, g[f"j{i}_count_b"])
        assert abs(R.jsd_counts(ca, cb) - float(g[f"j{i}_jsd"])) <= 1e-9


def test_point_mesh_restatement_matches_cgal(golden_dir):
    g = np.load(os.path.join(golden_dir, "eval_p2f.npz"))
    for c in range(int(g["ncases"])):
        ref = g[f"c{c}_cgal_dist"]
        got = R.point_mesh_dist(g[f"c{c}_pred"], g[f"c{c}_verts"], g[f"c{c}_faces"])
        # the binary prints 6 significant digits: half a unit of the 6th digit, plus the rounding of a value near zero
        assert np.all(np.abs(got - ref) <= 5e-6 * np.abs(ref) + 1e-12), c


def test_metrics_grid_is_the_restated_grid():
    from puflow_amd import metrics
    g = metrics.sphere_grid(28)
    np.testing.assert_array_equal(g, R.sphere_grid(28))
    assert g.dtype == np.float32 and g.shape[1] == 3


def test_jsd_from_counts_matches_restatement(golden_dir):
    from puflow_amd import metrics
    g = np.load(os.path.join(golden_dir, "eval_jsd.npz"))
    for i in range(int(g["npairs"])):
        got = metrics.jsd_from_counts(g[f"j{i}_count_a"], g[f"j{i}_count_b"])
        assert abs(got - float(g[f"j{i}_jsd"])) <= 1e-12


def test_read_off_header_variants_and_polygons(tmp_path):
    from puflow_amd.metrics import read_off
    body = "0 0 0\n1 0 0\n1 1 0\n0 1 0\n0.5 0.5 1  # apex\n4 0 1 2 3\n3 0 1 4 255 0 0\n"
    (tmp_path / "a.off").write_text("OFF\n# a comment line\n5 2 0\n" + body)
    (tmp_path / "b.off").write_text("OFF 5 2 0\n" + body)
    (tmp_path / "c.off").write_text("# leading comment\nOFF\n\n5 2 0\n" + body.replace("\n", "\n\n"))
    for name in ("a.off", "b.off", "c.off"):
        v, f = read_off(str(tmp_path / name))
        assert v.dtype == np.float32 and v.shape == (5, 3)
        np.testing.assert_array_equal(v[4], [0.5, 0.5, 1.0])
        np.testing.assert_array_equal(f, [[0, 1, 2], [0, 2, 3], [0, 1, 4]])      # the quad as a fan, colours ignored
    (tmp_path / "bad.off").write_text("PLY\n")
    with pytest.raises(ValueError):
        read_off(str(tmp_path / "bad.off"))


def test_cli_p2m_format_is_the_binary_format(golden_dir):
    """format_p2m of the fixture points' double values and the binary's own distances gives the binary's file."""
    from puflow_amd.evaluate import format_p2m
    g = np.load(os.path.join(golden_dir, "eval_p2f.npz"))
    for c in range(int(g["ncases"])):
        text = bytes(g[f"c{c}_cgal_text"]).decode()
        ref = [ln.split() for ln in text.splitlines()]
        mine = format_p2m(g[f"c{c}_pred"].astype(np.float64), np.array([float(r[3]) for r in ref])).splitlines()
        assert [ln.split()[:3] for ln in mine] == [r[:3] for r in ref], c


def test_eval_entry_points_validate_arguments_without_gpu(built_lib):
    from puflow_amd import _lib
    lib = _lib.load()
    assert lib.pf_approxmatch_emd(None, None, 1, 16, 16, 7, None, None, 0, None) == -1
    assert lib.pf_approxmatch_emd(8, 8, 0, 16, 16, 7, 8, 8, 1 << 20, None) == -2           # B = 0
    assert lib.pf_approxmatch_emd(8, 8, 1, 16, 0, 7, 8, 8, 1 << 20, None) == -2            # m = 0
    assert lib.pf_approxmatch_emd(8, 8, 1, 16, 16, 16, 8, 8, 1 << 20, None) == -2          # top out of range
    assert lib.pf_approxmatch_emd(8, 8, 1, 16, 16, 7, 8, 8, 10, None) == -5                # workspace too small
    assert lib.pf_approxmatch_ws_floats(1, 16, 16, 7) > 0 and lib.pf_approxmatch_ws_floats(1, -1, 16, 7) == -2
    assert lib.pf_point_mesh_dist(None, 4, None, 4, None, 0, None, None, None, 0, None) == -1
    assert lib.pf_point_mesh_dist(8, 0, 8, 4, None, 0, 8, None, 8, 1 << 20, None) == -2    # P = 0
    assert lib.pf_point_mesh_dist(8, 4, 8, -1, None, 0, 8, None, 8, 1 << 20, None) == -2   # F < 0
    assert lib.pf_point_mesh_dist(8, 4, 8, 4, None, 0, 8, None, 8, 3, None) == -5          # workspace too small
    # F * P beyond int: the workspace query stays exact (64-bit)
    assert lib.pf_point_mesh_ws_floats(20000, 1000000) > 0


def test_metrics_refuse_cpu_tensors():
    import torch
    from puflow_amd import _lib, metrics
    with pytest.raises(_lib.PuflowHipError):
        metrics.approx_match_emd(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3))
    with pytest.raises(_lib.PuflowHipError):
        metrics.point_to_mesh_distance(torch.zeros(4, 3), torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.long))
