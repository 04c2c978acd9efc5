"""Per-point attributes on the GPU (csrc/attr.hip, puflow_amd/attributes.py): the blend and the PCA normals against the float64
restatements of tests/attr_ref.py on the neighbourhoods the device search returned, the ragged forms against the dense ones on
every cloud alone (torch.equal), and the CLI's three options end to end."""
import filecmp

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attr_ref as R
from puflow_amd.weights import synth_state_dict

DEV = "cuda:0"
EPS = 2.0 ** -24
PLANS = {1: "lin1", 7: "normal,lin3,near1", 16: "lin2,near1,normal,lin6,near4"}


def _ref_plan(plan):
    return [(s.kind, s.cols) for s in plan]


def _attr(rng, n, plan):
    """random rows for a plan: unit columns hold unit vectors of both signs, near columns integer labels, lin columns N(0, 3)"""
    cols = []
    for kind, c in _ref_plan(plan):
        if kind == R.UNIT:
            v = rng.standard_normal((n, 3))
            cols.append(v / np.linalg.norm(v, axis=1, keepdims=True))
        elif kind == R.NEAR:
            cols.append(rng.integers(0, 9, size=(n, c)).astype(np.float64))
        else:
            cols.append(3.0 * rng.standard_normal((n, c)))
    return np.concatenate(cols, axis=1).astype(np.float32)


@pytest.fixture(scope="module")
def blend_inputs():
    """N = 300 references, M = 1000 queries of which the first 300 ARE the references; one search per K"""
    from puflow_amd import ops
    rng = np.random.default_rng(5)
    ref = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    query = np.concatenate([ref, rng.uniform(-1.1, 1.1, (700, 3)).astype(np.float32)])
    ref_d, query_d = torch.from_numpy(ref).to(DEV)[None], torch.from_numpy(query).to(DEV)[None]
    return {k: ops.knn_large(ref_d, query_d, k) for k in (1, 3, 8)}


@pytest.mark.parametrize("C", [1, 7, 16])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_blend_against_the_float64_restatement(blend_inputs, K, C):
    """lin within (2K + 8) 2^-24 max|column| (K products, K - 1 sums, the normalisation and the divisions, one rounding each, of a
    convex combination; the kernel divides exactly); near columns and coincident rows bit for bit; unit columns of length 1 within
    2^-22 and within the lin tolerance / |blend| of the restated direction."""
    from puflow_amd import attributes as A, ops
    plan = A.parse_plan(PLANS[C])
    attr = _attr(np.random.default_rng(100 + C), 300, plan)
    idx, d2 = blend_inputs[K]
    out = ops.attr_blend(idx, d2, torch.from_numpy(attr).to(DEV)[None], A._segments(plan))[0]
    torch.cuda.synchronize()
    idx_h, d2_h, got = idx[0].cpu().numpy(), d2[0].cpu().numpy(), out.cpu().numpy()
    want, unit_len = R.blend(idx_h, d2_h, attr, _ref_plan(plan))
    exact = d2_h[:, 0] == 0
    assert exact[:300].all() and exact.sum() == 300 and np.array_equal(idx_h[:300, 0], np.arange(300))
    assert np.array_equal(got[exact], attr[idx_h[exact, 0]])                       # the references get their own rows back
    assert np.isfinite(got).all()
    c = 0
    for kind, n in _ref_plan(plan):
        g, w = got[:, c:c + n].astype(np.float64), want[:, c:c + n]
        tol = (2 * K + 8) * EPS * np.abs(attr[:, c:c + n]).max()
        if kind == R.NEAR:
            assert np.array_equal(got[:, c:c + n], attr[idx_h[:, 0], c:c + n])
        elif kind == R.LIN:
            err = np.abs(g - w).max()
            print(f"K {K} C {C} lin columns {c}..{c + n - 1}: max error {err:.3e}, tolerance {tol:.3e}")
            assert err <= tol
        else:
            free = ~exact
            length = np.abs(np.linalg.norm(g[free], axis=1) - 1.0).max()
            err = (np.abs(g[free] - w[free]) * unit_len[free, None]).max()
            print(f"K {K} C {C} unit columns: | |n| - 1 | {length:.3e} (2^-22 = {2.0 ** -22:.3e}), error x |blend| {err:.3e}, "
                  f"tolerance {tol:.3e}, shortest blend {unit_len[free].min():.3f}")
            assert length <= 2.0 ** -22 and err <= tol
        c += n


def test_blend_constructed_cases():
    """opposite normals at equal distances do not cancel; a blend that is exactly zero writes neighbour 0's vector; a coincident
    point copies its row although its plan blends"""
    from puflow_amd import _lib, ops
    attr = torch.tensor([[[0, 0, 1.0], [0, 0, -1.0], [0.6, 0, 0.8], [0, 0, 0.0], [0.5, 0.25, 1.0], [-0.5, -0.25, -1.0]]], device=DEV)
    unit = [(_lib.PF_ATTR_UNIT, 3)]
    idx = torch.tensor([[[0, 1], [1, 0]]], dtype=torch.int32, device=DEV)
    d2 = torch.tensor([[[0.5, 0.5], [0.25, 0.25]]], device=DEV)
    out = ops.attr_blend(idx, d2, attr, unit)[0].cpu()
    assert torch.equal(out, torch.tensor([[0, 0, 1.0], [0, 0, -1.0]]))             # neighbour 0's side, full length
    # neighbour 0 (row 3) has no direction and rows 4, 5 cancel exactly; an output point ON row 2 copies it
    idx = torch.tensor([[[3, 4, 5], [2, 1, 0]]], dtype=torch.int32, device=DEV)
    d2 = torch.tensor([[[0.5, 1.0, 1.0], [0.0, 1.0, 1.0]]], device=DEV)
    out = ops.attr_blend(idx, d2, attr, unit)[0].cpu()
    assert torch.equal(out, torch.tensor([[0, 0, 0.0], [0.6, 0, 0.8]]))
    want, _ = R.blend(idx[0].cpu().numpy(), d2[0].cpu().numpy(), attr[0].cpu().numpy(), [(R.UNIT, 3)])
    assert np.array_equal(out.numpy(), want.astype(np.float32))


SIZES, OUT_SIZES = [300, 512, 1029], [700, 333, 1500]


def _ragged_clouds():
    rng = np.random.default_rng(8)
    clouds = [torch.from_numpy((rng.uniform(-1, 1, (n, 3)) * (1 + i) + i).astype(np.float32)).to(DEV) for i, n in enumerate(SIZES)]
    # a third of every cloud's output points ARE input points, the others lie anywhere in its box
    preds = [torch.cat([c[: m // 3], torch.from_numpy((rng.uniform(-1, 1, (m - m // 3, 3)) * (1 + i) + i).astype(np.float32)).to(DEV)])
             for i, (c, m) in enumerate(zip(clouds, OUT_SIZES))]
    return rng, clouds, preds


def test_ragged_blend_equals_the_dense_call_on_each_cloud_alone():
    from puflow_amd import attributes as A
    rng, clouds, preds = _ragged_clouds()
    plan = A.parse_plan(PLANS[7])
    attrs = [torch.from_numpy(_attr(rng, n, plan)).to(DEV) for n in SIZES]
    for k in (1, 8):
        together = A.transfer_ragged(preds, clouds, attrs, plan, k=k)
        for p, c, a, t in zip(preds, clouds, attrs, together):
            alone = A.transfer(p, c, a, plan, k=k)
            assert t.shape == (p.shape[0], 7) and torch.equal(t, alone)
        batch = A.transfer(torch.stack([preds[0], preds[0].flip(0)]), torch.stack([clouds[0], clouds[0]]),
                           torch.stack([attrs[0], attrs[0] * 2]), plan, k=k)      # a dense batch: every cloud its own rows
        assert torch.equal(batch[0], together[0])
        assert torch.equal(batch[1], A.transfer(preds[0].flip(0), clouds[0], attrs[0] * 2, plan, k=k))


@pytest.mark.parametrize("viewpoint", [None, (0.5, -2.0, 7.0)])
def test_ragged_normals_equal_the_dense_call_on_each_cloud_alone(viewpoint):
    from puflow_amd import attributes as A
    clouds = [torch.from_numpy(R.surface(name, 0.002, n)[0] * s + s).to(DEV) for name, n, s in
              (("sphere", 300, 1.0), ("torus", 512, 2.0), ("sphere", 1029, 0.5))]
    normals, var = A.estimate_normals_ragged(clouds, 16, viewpoint)
    for c, n, v in zip(clouds, normals, var):
        n1, v1 = A.estimate_normals(c, 16, viewpoint)
        assert n.shape == c.shape and torch.equal(n, n1) and torch.equal(v, v1)
    n2, v2 = A.estimate_normals(torch.stack([clouds[0], clouds[0].flip(0)]), 16, viewpoint)
    assert torch.equal(n2[0], normals[0]) and torch.equal(v2[0], var[0])


@pytest.fixture(scope="module")
def pca_runs():
    """every case's device neighbourhoods, normals (centroid rule) and variation, computed once"""
    from puflow_amd import ops
    runs = {}
    for name, sigma, k in R.PCA_CASES:
        pts, analytic = R.surface(name, sigma)
        p = torch.from_numpy(pts).to(DEV)[None]
        idx, _ = ops.knn_large(p, p, k)
        normal, var = ops.normals_pca(p, idx)
        runs[name, sigma, k] = (pts, analytic, idx[0].cpu().numpy(), normal[0].cpu().numpy(), var[0].cpu().numpy())
    return runs


@pytest.mark.parametrize("name,sigma,k", R.PCA_CASES)
def test_pca_normals_against_eigh(pca_runs, name, sigma, k):
    """angle to numpy.linalg.eigh's eigenvector (float64, same neighbourhoods) <= 1e-5 rad wherever the relative eigenvalue gap
    is at least 1e-2; at most 1 % of the rows may be below it; unit length; variation as restated and inside [0, 1/3]"""
    pts, analytic, idx, normal, var = pca_runs[name, sigma, k]
    want, want_var, gap = R.pca(pts, idx)
    keep = gap >= R.GAP_MIN
    assert (~keep).mean() <= R.GAP_SHARE
    ang = R.angle(normal, want)
    print(f"{name} sigma {sigma} k {k}: max angle to eigh {ang[keep].max():.3e} rad over {keep.sum()} rows, "
          f"variation error {np.abs(var - want_var).max():.3e}")
    assert np.isfinite(normal).all() and np.abs(np.linalg.norm(normal.astype(np.float64), axis=1) - 1).max() <= 2.0 ** -22
    assert ang[keep].max() <= 1e-5
    assert np.abs(var - want_var).max() <= 2 * EPS
    assert var.min() >= 0 and var.max() <= np.float32(1 / 3)
    assert np.array_equal(normal, R.orient(normal.astype(np.float64), pts).astype(np.float32))    # the centroid rule holds
    if sigma == 0.0 and k == 16:
        mean, bar = float(R.angle(normal, analytic).mean()), R.sagitta_bar(pts, idx, R.SURFACES[name][1])
        print(f"  mean angle to the analytic normal {mean:.4e} rad, chord-sagitta bar {bar:.4e} rad")
        assert mean < bar


def test_normal_orientation_and_degenerate_input(pca_runs):
    from puflow_amd import attributes as A
    pts, _, _, normal, _ = pca_runs["sphere", 0.0, 16]
    assert ((normal.astype(np.float64) * pts).sum(axis=1) > 0).all()               # centroid rule: outwards on the sphere
    view = np.array([0.0, 0.0, 5.0])
    seen, _ = A.estimate_normals(torch.from_numpy(pts).to(DEV), 16, viewpoint=view)
    seen = seen.cpu().numpy().astype(np.float64)
    assert ((seen * (view - pts)).sum(axis=1) >= 0).all()
    flipped = (seen * normal).sum(axis=1) < 0
    assert flipped.any() and np.array_equal(np.where(flipped[:, None], -seen, seen).astype(np.float32), normal)
    n, v = A.estimate_normals(torch.full((64, 3), 0.37, device=DEV), 64)
    assert torch.equal(n.cpu(), torch.tensor([0, 0, 1.0]).expand(64, 3)) and not v.cpu().any()
    n, v = A.estimate_normals(torch.full((64, 3), 0.37, device=DEV), 8, viewpoint=(1, 2, 3))
    assert torch.equal(n.cpu(), torch.tensor([0, 0, 1.0]).expand(64, 3)) and not v.cpu().any()


# ---- the CLI ---------------------------------------------------------------------------------------------------------------
FILES = {"a.xyz": 600, "b.xyz": 600, "c.xyz": 777, "d.xyz": 1500}
PLAN = "normal,lin2,near1"


def _sphere_rows(n, seed):
    """xyz on the unit sphere | normal = p | lin = (x, x + y) | label = the octant"""
    p = R.sphere(n, seed)[0].astype(np.float64)
    octant = (p[:, 0] > 0) * 1 + (p[:, 1] > 0) * 2 + (p[:, 2] > 0) * 4
    return np.concatenate([p, p, p[:, :1], p[:, :1] + p[:, 1:2], octant[:, None].astype(np.float64)], axis=1)


@pytest.fixture(scope="module")
def scans(tmp_path_factory):
    """the four 9-column files, their 3-column versions, the checkpoint, and the one-file-at-a-time runs of both directories"""
    from puflow_amd import upsample as U
    root = tmp_path_factory.mktemp("attributes")
    for d in ("in9", "in3", "one9", "one3"):
        (root / d).mkdir()
    for k, (name, n) in enumerate(FILES.items()):
        rows = _sphere_rows(n, 70 + k)
        np.savetxt(root / "in9" / name, rows, fmt="%.6f")
        np.savetxt(root / "in3" / name, rows[:, :3], fmt="%.6f")
    sd = synth_state_dict(9)
    torch.save(sd, root / "ckpt.pt")
    U.main(["--source", str(root / "in9"), "--target", str(root / "one9"), "--checkpoint", str(root / "ckpt.pt"),
            "--cloud_batch", "1", "--attributes", PLAN])
    U.main(["--source", str(root / "in3"), "--target", str(root / "one3"), "--checkpoint", str(root / "ckpt.pt"),
            "--cloud_batch", "1"])
    return root, sd


def _run(root, sd, tag, src="in9", names=FILES, **kw):
    from puflow_amd import upsample as U
    (root / tag).mkdir()
    U.upsampling([str(root / src / name) for name in names], str(root / tag), None, up_ratio=4, num_outlier=24, num_patch=256,
                 seed=2021, state_dict=sd, **kw)
    return root / tag


def _same(a, b, names):
    match, mismatch, errors = filecmp.cmpfiles(a, b, list(names), shallow=False)
    return sorted(match) == sorted(names) and not mismatch and not errors


def _xyz_bytes(path):
    with open(path, "rb") as f:
        return [b" ".join(line.split(b" ")[:3]) for line in f.read().splitlines()]


def _check_columns(out_path, in_path, n):
    """(a) is the caller's; (d) labels are input labels; (e) carried normals within 0.1 rad of p"""
    out, inp = np.loadtxt(out_path), np.loadtxt(in_path)
    assert out.shape == (4 * n, 9) and np.isfinite(out).all()
    assert set(np.unique(out[:, 8])) <= set(np.unique(inp[:, 8]))
    ang = np.arccos(np.clip((out[:, 3:6] * out[:, :3]).sum(axis=1) / (np.linalg.norm(out[:, 3:6], axis=1) * np.linalg.norm(out[:, :3], axis=1)), -1, 1))
    print(f"{out_path.name}: largest angle between a carried normal and p {ang.max():.4f} rad")
    assert ang.max() <= 0.1
    assert np.abs(np.linalg.norm(out[:, 3:6], axis=1) - 1).max() < 2e-6              # six decimals of a unit vector


def test_cli_one_file_at_a_time(scans):
    """(a) the xyz columns are the bytes of the run without --attributes on the 3-column files; (d), (e) on every file"""
    root, _ = scans
    for name, n in FILES.items():
        assert _xyz_bytes(root / "one9" / name) == _xyz_bytes(root / "one3" / name), name
        _check_columns(root / "one9" / name, root / "in9" / name, n)


class _Capture:
    """records every blend the CLI makes (dense and ragged) and checks (c) on it: an output point that coincides with an input
    point (d2_0 == 0 in the search's float32) carries that point's row exactly"""

    def __init__(self, monkeypatch):
        from puflow_amd import ops
        self.coincident = self.rows = 0
        dense, ragged = ops.attr_blend, ops.attr_blend_ragged

        def blend(idx, d2, attr, segments):
            out = dense(idx, d2, attr, segments)
            for b in range(idx.shape[0]):
                self.check(idx[b], d2[b], attr[b], out[b])
            return out

        def blend_ragged(idx, d2, attr, lengths, out_lengths, segments):
            out = ragged(idx, d2, attr, lengths, out_lengths, segments)
            for i, d, a, o in zip(torch.split(idx, out_lengths), torch.split(d2, out_lengths), torch.split(attr, lengths),
                                  torch.split(out, out_lengths)):
                self.check(i, d, a, o)
            return out

        monkeypatch.setattr(ops, "attr_blend", blend)
        monkeypatch.setattr(ops, "attr_blend_ragged", blend_ragged)

    def check(self, idx, d2, attr, out):
        hit = d2[:, 0] == 0
        assert torch.equal(out[hit], attr[idx[hit, 0].long()])
        self.coincident += int(hit.sum())
        self.rows += int(hit.numel())


def test_cli_batching_changes_no_file(scans, monkeypatch):
    """(b) --cloud_batch 4 (one ragged pass of four files) and --cloud_batch 2 (the dense pair 600 / 600, then the ragged pair
    777 / 1500) write the bytes of the one-file-at-a-time run; (c) on every blend these runs make"""
    root, sd = scans
    cap = _Capture(monkeypatch)
    four = _run(root, sd, "four", cloud_batch=4, attributes=PLAN)
    two = _run(root, sd, "two", cloud_batch=2, attributes=PLAN)
    assert _same(root / "one9", four, FILES) and _same(root / "one9", two, FILES)
    print(f"{cap.coincident} of {cap.rows} output points coincide with an input point")
    assert cap.rows == 2 * 4 * sum(FILES.values()) and cap.coincident > 0


def test_cli_sharding_changes_no_file(scans, monkeypatch):
    """(b) WORLD_SIZE = 2: ranks 0 and 1 together write the bytes of one process"""
    root, sd = scans
    monkeypatch.setenv("WORLD_SIZE", "2")
    (root / "ranks").mkdir()
    from puflow_amd import upsample as U
    for rank in ("0", "1"):
        monkeypatch.setenv("RANK", rank)
        U.upsampling([str(root / "in9" / name) for name in FILES], str(root / "ranks"), None, up_ratio=4, num_outlier=24,
                     num_patch=256, seed=2021, state_dict=sd, attributes=PLAN)
    assert _same(root / "one9", root / "ranks", FILES)


def test_cli_tiled_file(scans, monkeypatch):
    """--tile_points 512 on the 1500-point file: (a), (c), (d), (e) against the whole input cloud"""
    root, sd = scans
    cap = _Capture(monkeypatch)
    t9 = _run(root, sd, "tiled9", names=["d.xyz"], tile_points=512, attributes=PLAN)
    t3 = _run(root, sd, "tiled3", src="in3", names=["d.xyz"], tile_points=512)
    assert _xyz_bytes(t9 / "d.xyz") == _xyz_bytes(t3 / "d.xyz")
    assert not filecmp.cmp(t3 / "d.xyz", root / "one3" / "d.xyz", shallow=False)     # it did go through the tiles
    _check_columns(t9 / "d.xyz", root / "in9" / "d.xyz", 1500)
    assert cap.rows == 4 * 1500


def test_cli_estimate_normals(scans):
    """--estimate_normals 16 appends three columns of unit length (outwards on the sphere: the centroid rule), alone and after
    carried columns; with a plan that holds `normal` it exits with a message; so does a 9-column file without a plan"""
    from puflow_amd import upsample as U
    root, sd = scans
    out = _run(root, sd, "normals", src="in3", estimate_normals=16)                 # all four: the shuffles are drawn in file order
    for name in FILES:
        rows = np.loadtxt(out / name)
        assert rows.shape == (4 * FILES[name], 6) and _xyz_bytes(out / name) == _xyz_bytes(root / "one3" / name)
        assert np.abs(np.linalg.norm(rows[:, 3:], axis=1) - 1).max() < 2e-6
        assert ((rows[:, 3:] * rows[:, :3]).sum(axis=1) > 0).mean() > 0.99
    both = _run(root, sd, "both", names=["a.xyz"], attributes="lin3,lin2,near1", estimate_normals=16, normals_viewpoint="0,0,5")
    rows = np.loadtxt(both / "a.xyz")
    assert rows.shape == (2400, 12) and np.abs(np.linalg.norm(rows[:, 9:], axis=1) - 1).max() < 2e-6
    assert ((rows[:, 9:] * (np.array([0, 0, 5.0]) - rows[:, :3])).sum(axis=1) >= -1e-5).all()
    argv = ["--source", str(root / "in9"), "--target", str(root / "refused"), "--checkpoint", str(root / "ckpt.pt")]
    with pytest.raises(SystemExit, match="estimate_normals"):
        U.main(argv + ["--attributes", PLAN, "--estimate_normals", "16"])
    with pytest.raises(SystemExit, match="--attributes"):
        U.main(argv)
    with pytest.raises(SystemExit, match="--attributes"):
        U.main(argv + ["--attributes", "normal,lin2"])                               # the plan does not cover the file


def test_cli_continuous_model_takes_the_same_flags(tmp_path):
    """upsample_cnf.main with --attributes and --attr_k on one 600-point file, on a uniform step schedule (a short run)"""
    from puflow_amd import cnf, upsample_cnf
    from puflow_amd.weights import synth_cnf_state_dict
    (tmp_path / "in").mkdir()
    np.savetxt(tmp_path / "in" / "a.xyz", _sphere_rows(600, 70), fmt="%.6f")
    torch.save(synth_cnf_state_dict(7), tmp_path / "cnf.pt")
    cnf.save_schedule(cnf.uniform_schedule(3), tmp_path / "sched.json")
    upsample_cnf.main(["--source", str(tmp_path / "in"), "--target", str(tmp_path / "out"), "--checkpoint", str(tmp_path / "cnf.pt"),
                       "--num_patch", "128", "--schedule", str(tmp_path / "sched.json"), "--attributes", PLAN, "--attr_k", "4"])
    rows, inp = np.loadtxt(tmp_path / "out" / "a.xyz"), np.loadtxt(tmp_path / "in" / "a.xyz")
    assert rows.shape == (2400, 9) and np.isfinite(rows).all()
    assert set(np.unique(rows[:, 8])) <= set(np.unique(inp[:, 8]))
    assert np.abs(np.linalg.norm(rows[:, 3:6], axis=1) - 1).max() < 2e-6
