"""The restatement of the surface-connected neighbourhoods (tests/surface_ref.py) against what the definition implies, on the
CPU - and the margins the GPU tests (tests/test_gpu_surface.py) rely on, for the same meshes, seeds' generator and radii."""
import os

import numpy as np
import pytest

import surface_ref as SR
import uniform_ref as U


def _sources(v, f, seed, S):
    s, face = U.seeds_from_uniforms(v, f, U.uniforms(seed, S))
    return s.astype(np.float32), face


def test_flat_grid_is_euclidean():
    v, f = SR.grid(8, 8)
    pts, pf = _sources(v, f, 1, 300)
    for s, f0 in zip(*_sources(v, f, 0, 5)):
        b2 = SR.field(s, int(f0), v, f)
        d2 = SR.tri_d2(s, v[f])
        np.testing.assert_array_equal(b2, d2)                     # every face along the straight segment is nearer
        e = SR.euclid2(pts, s)
        D = SR.surface_d2(pts, pf, s, int(f0), v, f)
        assert np.all(D >= e) and np.all(D <= e * (1 + 1e-6) + 1e-12)      # the face's own d2 is no farther than its point
        assert (D == e).mean() > 0.95


def test_u_strip_goes_round_the_bend():
    L, g = 2.0, 0.1
    v, f = SR.u_strip(L, g)
    f0 = 0                                                        # lower arm, at x = 0
    s = v[f[f0]].astype(np.float64).mean(0).astype(np.float32)
    b2 = SR.field(s, f0, v, f)
    upper_near = 64 + np.flatnonzero(v[f[64:128]][:, :, 0].max(1) <= 0.25)     # upper arm, opposite the source
    assert len(upper_near) >= 4
    wall = (L - s[0]) ** 2
    assert np.all(np.abs(b2[upper_near] - wall) <= 0.15 * wall), (b2[upper_near], wall)   # one quad (L / 16) of slack
    assert np.all(b2[upper_near] > 100 * g * g)
    assert np.all(SR.tri_d2(s, v[f])[upper_near] < 2 * (g * g + 0.25 ** 2 * 2))


def test_sandwich_other_sheet_is_unreachable():
    v, f = SR.sandwich(SR.GAP)
    for s, f0 in zip(*_sources(v, f, 2, 6)):
        b2 = SR.field(s, int(f0), v, f)
        mine = SR.sheet_of("sandwich", f0)
        assert np.all(np.isfinite(b2[SR.sheet_of("sandwich", np.arange(256)) == mine]))
        assert np.all(np.isinf(b2[SR.sheet_of("sandwich", np.arange(256)) != mine]))


def test_values_below_the_smaller_stop_do_not_depend_on_the_stop(golden_dir):
    fx = np.load(os.path.join(golden_dir, "eval_uniform.npz"))
    for v, f in (SR.u_strip(), (fx["c2_verts"], fx["c2_faces"].astype(np.int64)), (fx["c0_verts"], fx["c0_faces"].astype(np.int64))):
        diag = float(np.linalg.norm(np.ptp(v, axis=0)))
        for s, f0 in zip(*_sources(v, f, 3, 4)):
            full = SR.field(s, int(f0), v, f)
            for r in (0.2 * diag, 0.4 * diag):
                rf, rd2, rb2 = SR.bottleneck(s, int(f0), v, f, r)
                ok = np.isfinite(rb2)
                np.testing.assert_array_equal(rb2[ok], full[rf][ok])            # finite values are exact
                assert np.all(full[rf][~ok] > np.float32(r * r))                # the others lie beyond the stop
                assert np.all(np.delete(full, rf) > np.float32(r * r))


def test_unwelded_copy_has_the_same_field():
    for v, f in (SR.u_strip(), SR.grid(8, 8)):
        uv, uf = SR.unwelded(v, f)
        for s, f0 in zip(*_sources(v, f, 4, 3)):
            np.testing.assert_array_equal(SR.field(s, int(f0), v, f), SR.field(s, int(f0), uv, uf))


def test_wrong_source_face_has_no_row():
    v, f = SR.grid(8, 8)
    s = v[f[0]].mean(0)
    assert len(SR.bottleneck(s, 127, v, f, 0.2)[0]) == 0 and len(SR.bottleneck(s, 500, v, f, 0.2)[0]) == 0


# ---- the margins of the GPU tests -------------------------------------------------------------------------------------------
def _disk_case(v, f, seed):
    mapped, mf = _sources(v, f, seed + 50, SR.DISK_POINTS)
    seeds, sf = _sources(v, f, seed, SR.DISK_SEEDS)
    return mapped, mf, seeds, sf, U.area_radii(v, f)[0]


@pytest.mark.parametrize("mesh", ["grid", "sandwich"])
def test_margins_of_the_disk_cases(mesh):
    v, f = SR.grid(8, 8) if mesh == "grid" else SR.sandwich(SR.GAP)
    mapped, mf, seeds, sf, radii = _disk_case(v, f, SR.DISK_KEY)
    D = SR.disks(mapped, mf, seeds, sf, v, f, radii)[4]
    assert SR.radius_margin(D, radii) > 1e-5
    assert SR.radius_margin(U.seed_distances(mapped, seeds), radii) > 1e-5      # the balls they are compared with
    if mesh == "sandwich":
        assert SR.GAP < radii[0]


def test_margins_of_the_folded_sheet(golden_dir):
    fx = np.load(os.path.join(golden_dir, "eval_uniform.npz"))
    v, f = fx["c2_verts"], fx["c2_faces"].astype(np.int64)
    S = SR.SHEET_SEEDS
    seeds = fx["c2_seeds"][:S]
    sf = U.seeds_from_uniforms(v, f, fx["uniforms"])[1][:S]
    mf = U.closest_points(fx["c2_cloud"], v, f)[1]
    counts, _, _, _, D = SR.disks(fx["c2_mapped"], mf, seeds, sf, v, f, fx["c2_radii"])
    assert SR.radius_margin(D, fx["c2_radii"]) > 1e-5                        # a face at the stop itself holds no member
    ball = fx["c2_counts"][:S].astype(np.int64)
    assert np.all(counts <= ball) and counts[:, -1].sum() < ball[:, -1].sum()
    print("surface / ball members:", counts.sum(0) / ball.sum(0))


@pytest.mark.parametrize("mesh", ["sandwich", "u_strip"])
def test_margins_of_the_patch_pools(mesh):
    """Stand-ins for the patch seeds (the real ones come out of the elimination on the GPU, where the margin is asserted
    again): the pools' last places are not contested within 1e-6."""
    v, f = SR.sandwich() if mesh == "sandwich" else SR.u_strip()
    P = SR.PATCH
    seeds, sf = _sources(v, f, 9, P["n_patches"])
    for n_out, n_set, sd in ((P["num_point"], P["ratio"] * P["cloud_points"], 2),
                             (P["num_point"] * P["up_ratio"], P["ratio"] * P["cloud_points"] * P["up_ratio"], 1)):
        samples, face = _sources(v, f, sd, n_set)
        for s, f0 in zip(seeds, sf):
            idx, d, fd2 = SR.patch_pool(samples, face, s, int(f0), v, f, P["ratio"] * n_out)
            assert np.all(np.isfinite(d[idx])) and SR.pool_margin(d, P["ratio"] * n_out, fd2) > 1e-6
            if mesh == "sandwich":
                assert np.all(SR.sheet_of(mesh, face[idx]) == SR.sheet_of(mesh, f0))


def test_margins_of_the_field_cases(golden_dir):
    """No face of a field case lies within 1e-5 of its source's stop: the candidate lists are compared exactly."""
    for name, (v, f, r_stop) in SR.field_cases(golden_dir).items():
        for s in SR.field_sources(name, v, f, 65)[0]:
            assert SR.stop_margin(s, v, f, r_stop) > 1e-5, name


@pytest.mark.parametrize("mesh", ["sandwich", "u_strip"])
def test_pools_whose_last_place_lies_beyond_the_first_stop(mesh):
    """The premise of the GPU test of sampling.surface_pool: for some seeds the k-th smallest D2 is above the first r_stop^2,
    and taking the first k values that show finite inside that stop would pick other samples than the whole mesh's k
    smallest - r_stop has to grow until the k-th value is at or below it."""
    v, f, q, qf, seeds, sf = SR.pool_case(mesh)
    k, beyond, wrong = SR.POOL_K, 0, 0
    for s, f0 in zip(seeds, sf):
        idx, d, fd2 = SR.patch_pool(q, qf, s, int(f0), v, f, k)
        assert SR.pool_margin(d, k, fd2) > 1e-6 and SR.order_defects(idx, d) == 0
        r = SR.first_stop(q, s, k)
        shown = SR.shown_d2(q, qf, s, int(f0), v, f, r)
        small = shown <= np.float32(r * r)
        np.testing.assert_array_equal(shown[small], d[small])                   # at or below the stop: exact
        assert np.all(d[~small] > np.float32(r * r))                            # above it: itself or +inf, never smaller
        beyond += int(np.sort(d)[k - 1] > np.float32(r * r))
        if np.isfinite(shown).sum() >= k:
            wrong += int(set(np.lexsort((np.arange(len(shown)), shown))[:k]) != set(idx))
        grown = SR.shown_d2(q, qf, s, int(f0), v, f, r * 1.5 ** 8)
        assert np.sort(grown)[k - 1] <= np.float32((r * 1.5 ** 8) ** 2)
        np.testing.assert_array_equal(np.lexsort((np.arange(len(grown)), grown))[:k], idx)
    print(mesh, "beyond the first stop:", beyond, "wrong by the finite rule:", wrong)
    assert beyond >= 2 and wrong >= 2
