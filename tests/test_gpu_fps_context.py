"""pf_fps_ragged_ctx on the GPU: FPS whose min-distances start at the distance to a fixed context.  The criterion is
torch.equal with the numpy restatement (tests/tiles_ref.py: oracle/patch_ref.py's arithmetic, first maximum) for the indices and
bit equality for the radius, in both kernel families and in one launch that mixes them."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tiles_ref as R
from kernel_trace import launched, ran
from puflow_amd.weights import synth_patches

DEV = "cuda:0"


def run(clouds, samples, ctxs, group=0):
    """one ragged launch over numpy clouds / contexts (None or [C,3]) -> (list of index arrays, r2 array, kernel names)"""
    from puflow_amd import ops
    xyz = torch.from_numpy(np.concatenate(clouds)).to(DEV)
    cl = [0 if c is None else len(c) for c in ctxs]
    ctx = torch.from_numpy(np.concatenate([c for c in ctxs if c is not None and len(c)])).to(DEV) if sum(cl) else None
    (idx, r2), names = launched(lambda: ops.furthest_point_sample_ragged(xyz, [len(c) for c in clouds], samples, group=group,
                                                                         context=ctx, context_lengths=cl, return_radius=True))
    assert idx.dtype == torch.int32 and r2.dtype == torch.float32
    return [i.cpu().numpy() for i in torch.split(idx, samples)], r2.cpu().numpy(), names


def check(clouds, samples, ctxs, got_idx, got_r2):
    for i, (p, m, c) in enumerate(zip(clouds, samples, ctxs)):
        idx, d = R.fps_ctx(p, m, c)
        assert np.array_equal(got_idx[i], idx), (i, np.nonzero(got_idx[i] != idx)[0][:5])
        assert got_r2[i].tobytes() == d[-1].tobytes(), (i, got_r2[i], d[-1])
        assert np.all(d[1:] <= d[:-1])                                   # min-distances never grow


def lattice(n, seed):
    """n points of a 0.125 lattice in random order: many exactly equal distances"""
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    return (g[rng.permutation(len(g))[:n]] * 0.125).astype(np.float32)


SMALL = {
    "lattice": lambda: (lattice(300, 1), (lattice(400, 2)[-5:] + np.float32(0.0625)).astype(np.float32)),
    "coincident": lambda: (lambda p: (p, p[[3, 50, 51, 200, 299]].copy()))(synth_patches(1, 300, seed=11)[0].numpy()),
    "few_distinct": lambda: (np.tile(synth_patches(1, 20, seed=12)[0].numpy(), (15, 1)),
                             synth_patches(1, 5, seed=13, surface=False)[0].numpy()),
}


@pytest.mark.parametrize("name", list(SMALL))
def test_single_workgroup_kernel(name):
    """300 candidates, 5 context points, 40 samples: ties on a lattice, context points that ARE candidates (distance 0 from
    the start), more samples than distinct points (the tail is all zero distances: index order decides)."""
    p, c = SMALL[name]()
    assert p.shape == (300, 3) and c.shape == (5, 3)
    idx, r2, names = run([p], [40], [c])
    assert ran(names, "fps_ragged_ctx_kernel") and not ran(names, "fps_coopm"), sorted(names)
    check([p], [40], [c], idx, r2)
    if name == "coincident":
        assert not set(idx[0][:35].tolist()) & {3, 50, 51, 200, 299}     # taken points are not taken again while others are left
    if name == "few_distinct":
        assert r2[0] == 0.0


def test_cooperative_kernel_context_sizes():
    """N = 8192 + 37 (no multiple of anything), 600 samples, contexts of 0, 1 and 700 points - three clouds of one launch"""
    p = synth_patches(1, 8192 + 37, seed=21)[0].numpy()
    big = synth_patches(1, 700, seed=22)[0].numpy()
    ctxs = [None, big[:1].copy(), big]
    idx, r2, names = run([p, p, p], [600] * 3, ctxs)
    assert ran(names, "fps_coopm_ragged_ctx_kernel") and not ran(names, "fps_ragged_ctx_kernel"), sorted(names)
    check([p, p, p], [600] * 3, ctxs, idx, r2)
    assert idx[0][0] == 0 and not np.array_equal(idx[0], idx[2])


def test_cooperative_kernel_group_hint_changes_no_index():
    p = synth_patches(1, 10240, seed=31)[0].numpy()
    c = synth_patches(1, 300, seed=32)[0].numpy()
    plain, r2a, _ = run([p], [600], [c], group=0)
    hinted, r2b, names = run([p], [600], [c], group=1280)
    assert ran(names, "fps_coopm_ragged_ctx_kernel"), sorted(names)
    assert np.array_equal(plain[0], hinted[0]) and r2a.tobytes() == r2b.tobytes()
    check([p], [600], [c], hinted, r2b)


def test_one_launch_mixes_kernels_and_a_cloud_without_context():
    """a cooperative cloud with a context, a small cloud with a context, a cloud with none: the third gets the samples of
    furthest_point_sample_ragged without a context, bit for bit"""
    from puflow_amd import ops
    clouds = [synth_patches(1, 8192 + 37, seed=41)[0].numpy(), lattice(300, 42), synth_patches(1, 9000, seed=43)[0].numpy()]
    ctxs = [synth_patches(1, 700, seed=44)[0].numpy(), lattice(400, 45)[-5:], None]
    samples = [200, 40, 150]
    idx, r2, names = run(clouds, samples, ctxs)
    assert ran(names, "fps_coopm_ragged_ctx_kernel") and ran(names, "fps_ragged_ctx_kernel"), sorted(names)
    check(clouds, samples, ctxs, idx, r2)
    alone = ops.furthest_point_sample_ragged(torch.from_numpy(clouds[2]).to(DEV), [9000], [150])
    assert torch.equal(torch.from_numpy(idx[2]).to(DEV), alone)
    # and the defaults still give today's call: no context kernel runs
    _, names = launched(lambda: ops.furthest_point_sample_ragged(torch.from_numpy(clouds[2]).to(DEV), [9000], [150]))
    assert not ran(names, "ctx_kernel"), sorted(names)


def test_status_words_and_radius_limit():
    """the entry point keeps pf_fps_ragged's status words: 0 after a normal run for every cloud, one word set by hand makes
    the wrapper's check raise; a radius above the limit raises too and names the cloud.  No kernel is made to fail."""
    from puflow_amd import _lib, ops
    lib = _lib.load()
    sizes, samples, cl = [10240, 300, 9000], [64, 16, 64], [50, 5, 0]
    lay = ops.fps_ragged_layout(sizes)
    pts = torch.cat([synth_patches(1, n, seed=77 + i)[0] for i, n in enumerate(sizes)]).to(DEV)
    ctx = synth_patches(1, 55, seed=99)[0].to(DEV)
    scratch = torch.empty((lay["total_floats"],), dtype=torch.float32, device=DEV)
    idx = torch.zeros((sum(samples),), dtype=torch.int32, device=DEV)
    r2 = torch.zeros((3,), dtype=torch.float32, device=DEV)
    _lib.check(lib.pf_fps_ragged_ctx(pts.data_ptr(), _lib.counts(sizes), _lib.counts(samples), ctx.data_ptr(), _lib.counts(cl), 3, 0,
                                     scratch.data_ptr(), idx.data_ptr(), r2.data_ptr(), None), "pf_fps_ragged_ctx")
    torch.cuda.synchronize()
    words = scratch.view(torch.int64)
    assert [int(words[w]) for w in lay["status_words"]] == [0, 0, 0]
    ops._check_fps_abort_ragged(scratch, lay["status_words"], (r2, float(r2.max())))
    for cloud in (0, 1, 2):
        words[lay["status_words"][cloud]] = 1
        with pytest.raises(_lib.PuflowHipError, match=rf"\[{cloud}\]"):
            ops._check_fps_abort_ragged(scratch, lay["status_words"], (r2, float(r2.max())))
        words[lay["status_words"][cloud]] = 0
    worst = int(r2.argmax())
    with pytest.raises(ops.FpsRadiusError, match=rf"\[{worst}\]") as e:
        ops.furthest_point_sample_ragged(pts, sizes, samples, context=ctx, context_lengths=cl,
                                         radius_limit=float(np.nextafter(np.float32(r2.max().item()), np.float32(0))))
    assert e.value.clouds == [worst]
