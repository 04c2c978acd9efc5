"""Ragged passes on the GPU: clouds of different sizes stored back to back go through normalise -> seed FPS -> kNN-256 patches
-> network -> FPS merge -> de-normalise -> outlier removal together.  The criterion everywhere is torch.equal with the dense
operator run on each cloud ALONE (B = 1) - which the existing tests pin to the reference - plus one direct comparison with the
CPU oracle."""
import filecmp

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import patch_ref as P
from kernel_trace import launched, ran
from puflow_amd.weights import synth_patches, synth_state_dict

DEV = "cuda:0"
SIZE_SETS = {
    "typical": [5000, 4100, 5903, 2048, 5000],
    "odd": [2048, 300, 777, 2051],            # no multiples of 64; the 300-point cloud merges 4 x 1280 = 5120 candidates (below the
                                              # cooperative kernel's 8192), its companions more: both FPS kernels in one pass
    "single": [5000],
    "equal": [2048, 2048, 2048],
}


def make_clouds(sizes, seed):
    """clouds of the given sizes, each with its own position and scale (the global normalisation has something to do)"""
    return [(synth_patches(1, n, seed=seed + 13 * i, surface=True)[0] * (1.0 + 0.5 * i) + 0.3 * i).to(DEV) for i, n in enumerate(sizes)]


def n_patch(n):
    return int(n / 256 * 4)


@pytest.fixture(scope="module")
def net():
    from puflow_amd.interpflow import PointInterpFlow
    net = PointInterpFlow(3)
    net.load_state_dict(synth_state_dict(31))
    net.set_to_initialized_state()
    return net.to(DEV).eval()


@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_ragged_ops_equal_the_dense_ops_on_each_cloud_alone(name):
    from puflow_amd import ops
    sizes = SIZE_SETS[name]
    clouds = make_clouds(sizes, seed=100)
    packed = torch.cat(clouds)
    # normalise: all three outputs
    out, cen, fd = ops.normalize_pc_ragged(packed, sizes)
    for i, (o, c) in enumerate(zip(torch.split(out, sizes), clouds)):
        do, dc, dfd = ops.normalize_pc(c[None])
        assert torch.equal(o, do[0]) and torch.equal(cen[i:i + 1], dc) and torch.equal(fd[i:i + 1], dfd), (name, i)
    # seed FPS (no hint), then the kNN-256 patches of those seeds: indices and distances
    seeds_n = [n_patch(n) for n in sizes]
    idx = ops.furthest_point_sample_ragged(out, sizes, seeds_n)
    dense_idx = [ops.furthest_point_sample(o[None], m)[0] for o, m in zip(torch.split(out, sizes), seeds_n)]
    assert idx.dtype == torch.int32 and torch.equal(idx, torch.cat(dense_idx)), name
    first = np.cumsum([0] + sizes[:-1])
    queries = torch.cat([o[i.long()] for o, i in zip(torch.split(out, sizes), dense_idx)])
    dist, kidx = ops.knn_ragged(out, sizes, queries, seeds_n, 256)
    assert kidx.dtype == torch.int64 and tuple(kidx.shape) == (sum(seeds_n), 256)
    knn = ops.KNN(k=256, transpose_mode=True)
    for i, (o, q, d, k) in enumerate(zip(torch.split(out, sizes), torch.split(queries, seeds_n), torch.split(dist, seeds_n),
                                         torch.split(kidx, seeds_n))):
        dd, di = knn(o[None], q[None])
        assert torch.equal(k, di[0]) and torch.equal(d, dd[0]), (name, i, int(first[i]))
    # nearest distance, 4 n + 24 points against the cloud (2048 references: pf_nn1's MFMA-filter kernel; the others its scan)
    xs = [(synth_patches(1, 4 * n + 24, seed=300 + i, surface=True)[0] * (1.0 + 0.5 * i) + 0.3 * i).to(DEV) for i, n in enumerate(sizes)]
    nd = ops.nearest_distance_ragged(torch.cat(xs), [x.shape[0] for x in xs], packed, sizes)
    for i, (x, c, d) in enumerate(zip(xs, clouds, torch.split(nd, [x.shape[0] for x in xs]))):
        assert torch.equal(d, ops.nearest_distance(x[None], c[None])[0]), (name, i)


@pytest.mark.parametrize("name", ["typical", "odd", "equal"])
def test_ragged_fps_with_the_merge_hint(name):
    """The FPS merge's shape: n_patch x 1280 candidates per cloud with group = 1280, 4 n + 24 samples.  'odd' has 5120
    candidates for its 300-point cloud: the single-workgroup kernel and the cooperative one in the same pass."""
    from puflow_amd import ops
    sizes = SIZE_SETS[name]
    cand_n = [n_patch(n) * 1280 for n in sizes]
    samples = [4 * n + 24 for n in sizes]
    cand = [synth_patches(1, m, seed=500 + i, surface=True)[0].to(DEV) for i, m in enumerate(cand_n)]
    got, names = launched(lambda: ops.furthest_point_sample_ragged(torch.cat(cand), cand_n, samples, group=1280))
    assert ran(names, "fps_coopm_ragged_kernel"), sorted(names)
    if name == "odd":
        assert ran(names, "fps_ragged_kernel"), sorted(names)
    plain = ops.furthest_point_sample_ragged(torch.cat(cand), cand_n, samples)
    assert torch.equal(got, plain)                                               # the hint changes no index
    for i, (c, g, m) in enumerate(zip(cand, torch.split(got, samples), samples)):
        assert torch.equal(g, ops.furthest_point_sample(c[None], m, group=1280)[0]), (name, i)
        assert int(g[0]) == 0


def test_ragged_fps_cooperative_on_the_seed_side_and_against_the_oracle():
    """[10240, 9000]: both clouds above the cooperative threshold with different numbers of workgroups; against the dense
    operator AND the CPU oracle's FPS."""
    from puflow_amd import ops
    sizes, samples = [10240, 9000], [160, 140]
    clouds = [synth_patches(1, n, seed=700 + i, surface=True)[0] for i, n in enumerate(sizes)]
    clouds[1][5] = clouds[1][9]                                                  # a duplicate: ties go to the first maximum
    lay = ops.fps_ragged_layout(sizes)
    assert all(w >= 2 for w in lay["workgroups"]) and lay["workgroups"][0] != lay["workgroups"][1]
    got, names = launched(lambda: ops.furthest_point_sample_ragged(torch.cat(clouds).to(DEV), sizes, samples))
    assert ran(names, "fps_coopm_ragged_kernel") and not ran(names, "fps_ragged_kernel"), sorted(names)
    for c, g, m in zip(clouds, torch.split(got, samples), samples):
        assert torch.equal(g, ops.furthest_point_sample(c[None].to(DEV), m)[0])
        assert torch.equal(g.cpu().long(), P.fps(c[None], m)[0])
    many = [2500, 2200]                                                          # many rounds of the exchange
    got = ops.furthest_point_sample_ragged(torch.cat(clouds).to(DEV), sizes, many)
    for c, g, m in zip(clouds, torch.split(got, many), many):
        assert torch.equal(g, ops.furthest_point_sample(c[None].to(DEV), m)[0])


def test_ragged_patches_against_the_cpu_oracle():
    """oracle.patch_ref directly (not through the dense operators): FPS seeds and kNN-256 patches of two clouds of different
    size."""
    from puflow_amd import ops
    sizes = [3000, 2051]
    clouds = [synth_patches(1, n, seed=900 + i, surface=True)[0] for i, n in enumerate(sizes)]
    packed = torch.cat(clouds).to(DEV)
    seeds_n = [n_patch(n) for n in sizes]
    idx = ops.furthest_point_sample_ragged(packed, sizes, seeds_n)
    for c, g, m in zip(clouds, torch.split(idx, seeds_n), seeds_n):
        assert torch.equal(g.cpu().long(), P.fps(c[None], m)[0])
    queries = torch.cat([c.to(DEV)[g.long()] for c, g in zip(clouds, torch.split(idx, seeds_n))])
    _, kidx = ops.knn_ragged(packed, sizes, queries, seeds_n, 256)
    for c, k, m in zip(clouds, torch.split(kidx, seeds_n), seeds_n):
        ref = P.extract_knn_patch(c[None], 256, 4)                               # [1, n_patch, 256, 3]
        assert torch.equal(c[k.cpu()], ref[0])


def run_dense(ph, net, cloud, npoint):
    from puflow_amd.patch import PatchHelper
    up = ph.upsample(net, cloud[None], npoint=npoint, upratio=4)
    return up[0], PatchHelper.remove_outliers(up, cloud[None], 24)[0]


@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_upsample_ragged_equals_upsample_per_cloud(net, name):
    from puflow_amd.patch import PatchHelper
    sizes = SIZE_SETS[name]
    clouds = make_clouds(sizes, seed=1000)
    npoints = [4 * n + 24 for n in sizes]
    ph = PatchHelper(256, 4)
    with torch.no_grad():
        ups = ph.upsample_ragged(net, clouds, npoints, upratio=4)
        outs = PatchHelper.remove_outliers_ragged(ups, clouds, 24)
        assert [tuple(u.shape) for u in ups] == [(m, 3) for m in npoints]
        assert [tuple(o.shape) for o in outs] == [(4 * n, 3) for n in sizes]
        for i, (c, m) in enumerate(zip(clouds, npoints)):
            up, out = run_dense(ph, net, c, m)
            assert torch.equal(ups[i], up), (name, i)
            assert torch.equal(outs[i], out), (name, i)


def test_a_cloud_does_not_depend_on_its_companions(net):
    """The same cloud in two different size sets, at two positions: one result."""
    from puflow_amd.patch import PatchHelper
    ph = PatchHelper(256, 4)
    x = make_clouds([4100], seed=1234)[0]
    a = make_clouds([5000, 777], seed=1300)
    b = make_clouds([300, 2048, 5903], seed=1400)
    with torch.no_grad():
        ra = ph.upsample_ragged(net, [a[0], x, a[1]], [20024, 16424, 3132], upratio=4)
        rb = ph.upsample_ragged(net, [x] + b, [16424, 1224, 8216, 23636], upratio=4)
        oa = PatchHelper.remove_outliers_ragged(ra, [a[0], x, a[1]], 24)
        ob = PatchHelper.remove_outliers_ragged(rb, [x] + b, 24)
    assert torch.equal(ra[1], rb[0]) and torch.equal(oa[1], ob[0])


def test_upsample_ragged_refuses_a_cloud_smaller_than_a_patch(net):
    from puflow_amd._lib import PuflowHipError
    from puflow_amd.patch import PatchHelper
    clouds = make_clouds([2048, 200], seed=5)
    with pytest.raises(PuflowHipError, match="tiny.xyz"):
        PatchHelper(256, 4).upsample_ragged(net, clouds, [8216, 824], upratio=4, names=["big.xyz", "tiny.xyz"])
    with pytest.raises(PuflowHipError):                                          # the dense path's exception type
        PatchHelper(256, 4).upsample(net, clouds[1][None], npoint=824, upratio=4)


def test_cli_mixed_sizes_share_passes_without_changing_any_file(tmp_path, monkeypatch):
    """A directory where no two neighbours have the same size: the default cloud_batch takes it in ONE pass, --cloud_batch 1 file
    by file (the dense path), a --pass_points limit in three passes - every output file byte for byte the same."""
    from puflow_amd import upsample as U
    from puflow_amd.patch import PatchHelper
    src = tmp_path / "in"
    src.mkdir()
    sizes = {"a.xyz": 1024, "b.xyz": 768, "c.xyz": 1300, "d.xyz": 1024, "e.xyz": 600}
    for k, (name, n) in enumerate(sizes.items()):
        np.savetxt(src / name, (synth_patches(1, n, seed=40 + k)[0] * 2.0 - 0.5).numpy(), fmt="%.6f")
    sd = synth_state_dict(9)
    paths = [str(src / name) for name in sizes]
    calls = {"ragged": 0, "dense": 0}
    ragged, dense = PatchHelper.upsample_ragged, PatchHelper.upsample

    def count_ragged(self, *a, **k):
        calls["ragged"] += 1
        return ragged(self, *a, **k)

    def count_dense(self, *a, **k):
        calls["dense"] += 1
        return dense(self, *a, **k)

    monkeypatch.setattr(PatchHelper, "upsample_ragged", count_ragged)
    monkeypatch.setattr(PatchHelper, "upsample", count_dense)
    passes = {}
    for tag, kw in (("default", {}), ("one", {"cloud_batch": 1}), ("split", {"pass_points": 2500})):
        dst = tmp_path / tag
        dst.mkdir()
        calls["ragged"] = calls["dense"] = 0
        U.upsampling(paths, str(dst), None, up_ratio=4, num_outlier=24, num_patch=256, seed=2021, state_dict=sd, **kw)
        passes[tag] = dict(calls)
    assert passes["default"] == {"ragged": 1, "dense": 0}                        # one pass for five files
    assert passes["one"] == {"ragged": 0, "dense": 5}
    assert passes["split"] == {"ragged": 2, "dense": 1}                          # [1024, 768], [1300, 1024], [600]
    for tag in ("default", "split"):
        match, mismatch, errors = filecmp.cmpfiles(tmp_path / "one", tmp_path / tag, list(sizes), shallow=False)
        assert sorted(match) == sorted(sizes) and not mismatch and not errors, (tag, mismatch, errors)
    assert np.loadtxt(tmp_path / "default" / "c.xyz").shape == (1300 * 4, 3)


def test_ragged_fps_status_words():
    """Every cloud of a ragged pass has a status word - 0 after a normal run, whichever kernel sampled it; a word set by hand
    (1 = gave up waiting, 2 = never finished) makes the wrapper's check raise.  No kernel is made to fail."""
    from puflow_amd import _lib, ops
    lib = _lib.load()
    sizes, samples = [10240, 300, 9000], [64, 16, 64]
    lay = ops.fps_ragged_layout(sizes)
    pts = torch.cat([synth_patches(1, n, seed=77 + i)[0] for i, n in enumerate(sizes)]).to(DEV)
    scratch = torch.empty((lay["total_floats"],), dtype=torch.float32, device=DEV)
    idx = torch.zeros((sum(samples),), dtype=torch.int32, device=DEV)
    _lib.check(lib.pf_fps_ragged(pts.data_ptr(), _lib.counts(sizes), _lib.counts(samples), 3, 0, scratch.data_ptr(), idx.data_ptr(),
                                 None), "pf_fps_ragged")
    torch.cuda.synchronize()
    words = scratch.view(torch.int64)
    assert [int(words[w]) for w in lay["status_words"]] == [0, 0, 0]
    ops._check_fps_abort_ragged(scratch, lay["status_words"])                    # clean: no exception
    for cloud in (0, 1, 2):
        for status in (1, 2):
            words[lay["status_words"][cloud]] = status
            with pytest.raises(_lib.PuflowHipError, match=rf"\[{cloud}\]"):
                ops._check_fps_abort_ragged(scratch, lay["status_words"])
            words[lay["status_words"][cloud]] = 0
