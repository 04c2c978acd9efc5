"""Device-resident training data without a GPU: the Philox restatement the GPU tests compare against, pf_patch_batch's argument
validation, DevicePatchData's refusal of a CPU device, and the distribution of the parallel subsample selection."""
import numpy as np
import pytest

import philox_ref as P

# twice the largest two-sample KS statistic between ten PatchData._nonuniform runs (seeds 100..109, 2048 patches of 256 out of
# 1024 each, all 45 pairs): measured 0.02063 on the CPU (mean over the pairs 0.0067) -> 0.0413.  The 256 indices of a patch share
# one `loc`, so the pooled sample is far from 524 288 independent draws: that is why the bar is measured and not the textbook one.
KS_BAR = 0.0413
N_IN, N, PATCHES = 1024, 256, 2048


@pytest.fixture(scope="module")
def lib():
    from puflow_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_philox_restatement_known_answers():
    """Random123's known-answer vectors for Philox-4x32-10 (kat_vectors): all-zero and all-ones counter and key."""
    got = P.philox4x32(np.zeros(4, np.uint32), np.zeros(2, np.uint32))
    assert [int(v) for v in got] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    got = P.philox4x32(np.full(4, 0xffffffff, np.uint32), np.full(2, 0xffffffff, np.uint32))
    assert [int(v) for v in got] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    # vectorised over leading dimensions, and the uniform mapping stays inside (0, 1)
    many = P.philox4x32(np.zeros((3, 5, 4), np.uint32), np.zeros((3, 5, 2), np.uint32))
    assert many.shape == (3, 5, 4) and (many == np.array([0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8], np.uint32)).all()
    edge = np.array([0, 0xff, 0x100, 0xffffffff], np.uint32)
    for dt in (np.float64, np.float32):
        u = P.u01(edge, dt)
        assert (u > 0).all() and (u < 1).all() and u[0] == u[1] == dt(2.0 ** -25)


def _call(lib, **kw):
    a = dict(inp=8, gt=8, radius=8, order=8, M=64, n_in=256, n_out=1024, pos=0, b=32, n=256, slot0=0, seed=1, flags=0, sigma=0.01,
             clip=0.03, lo=0.8, hi=1.2, shift=0.0, out_inp=8, out_gt=8, out_radius=8, params=8, idx=None, cand=None, T=0, status=8)
    a.update(kw)
    return lib.pf_patch_batch(a["inp"], a["gt"], a["radius"], a["order"], a["M"], a["n_in"], a["n_out"], a["pos"], a["b"], a["n"],
                              a["slot0"], a["seed"], a["flags"], a["sigma"], a["clip"], a["lo"], a["hi"], a["shift"], a["out_inp"],
                              a["out_gt"], a["out_radius"], a["params"], a["idx"], a["cand"], a["T"], a["status"], None)


def test_patch_batch_argument_validation_without_gpu(lib):
    """pf_patch_batch rejects bad arguments before touching the device: -1 null pointers, -2 shapes, -3 unsupported sizes."""
    for name in ("inp", "gt", "radius", "order", "out_inp", "out_gt", "out_radius", "params", "status"):
        assert _call(lib, **{name: None}) == -1, name
    assert _call(lib, M=0) == -2 and _call(lib, b=0) == -2 and _call(lib, n=0) == -2 and _call(lib, pos=-1) == -2
    assert _call(lib, n=512) == -2                                   # more points asked for than a patch has
    assert _call(lib, n_in=1024) == -2                               # n_in > n and no subsample stage to choose n of them
    assert _call(lib, cand=8, T=0) == -2
    assert _call(lib, sigma=-1.0) == -2 and _call(lib, lo=1.2, hi=0.8) == -2 and _call(lib, shift=-0.1) == -2
    assert _call(lib, flags=64) == -3                                # not a stage
    assert _call(lib, n_in=8193, flags=1) == -3                      # PF_PATCH_MAX_NIN: the LDS first-occurrence table
    assert _call(lib, n_in=8192, n=4097, flags=1) == -3              # PF_PATCH_MAX_N
    assert lib.pf_error_string(-3) != lib.pf_error_string(-2)


def test_device_patch_data_has_no_cpu_fallback():
    from puflow_amd import _lib
    from puflow_amd.data import DevicePatchData, SyntheticDevicePatchData
    z = np.zeros((4, 256, 3), np.float32)
    with pytest.raises(_lib.PuflowHipError):
        DevicePatchData(z, np.zeros((4, 1024, 3), np.float32), device="cpu")
    with pytest.raises(_lib.PuflowHipError):
        SyntheticDevicePatchData(num_patches=4, batch_size=2, device="cpu")


def test_synthetic_data_default_is_unchanged_and_random_input_gets_the_4x_cloud():
    """SyntheticPatchData shares its arrays with the device twin: the default is what it always was (a subset of the dense
    cloud, normalised by the sparse one), use_random_input makes the sparse cloud 4n points."""
    from puflow_amd.data import SyntheticPatchData
    from puflow_amd.weights import synth_patches
    d = SyntheticPatchData(num_patches=3, num_point_patch=64, up_ratio=4, seed=5, batch_size=3)
    dense = synth_patches(3, 256, seed=5).numpy()
    rng = np.random.default_rng(6)
    sparse = np.stack([x[rng.permutation(256)[:64]] for x in dense])
    c = sparse.mean(axis=1, keepdims=True)
    far = np.sqrt(((sparse - c) ** 2).sum(-1)).max(axis=1, keepdims=True)[..., None]
    assert np.array_equal(d.inp, ((sparse - c) / far).astype(np.float32)) and np.array_equal(d.gt, ((dense - c) / far).astype(np.float32))
    r = SyntheticPatchData(num_patches=3, num_point_patch=64, up_ratio=4, seed=5, batch_size=3, use_random_input=True, is_augment=False)
    assert r.inp.shape == (3, 256, 3) and next(iter(r))["input_sparse_xyz_pl"].shape == (3, 64, 3)


def test_selection_restatement_is_the_sequential_rejection_loop():
    """`select` (first occurrences ranked by stream position) yields what the reference's one-at-a-time loop yields."""
    rng = np.random.default_rng(0)
    for n_in, n in ((64, 16), (1024, 256), (40, 40)):
        cand = rng.integers(-n_in // 2, n_in + n_in // 2, size=4096)
        chosen = {}
        for a in cand:
            if 0 <= a < n_in and len(chosen) < n:
                chosen.setdefault(int(a))
        idx, rounds, short = P.select(cand, n_in, n)
        assert not short and idx.tolist() == list(chosen) and 1 <= rounds <= 4
    idx, rounds, short = P.select(np.array([3, 3, -1, 5, 99]), 8, 4)
    assert short and idx.tolist() == [3, 5, 5, 5]


def test_float32_candidates_stay_within_the_share_the_gpu_test_relies_on():
    """The GPU test lets the kernel's fp32 candidates differ from the float64 restatement by one index on at most 1 % of the
    entries: the restatement in float32 against itself in float64 must stay well inside that (measured: 0.007 % differ)."""
    diff = total = 0
    for slot in range(64):
        c64, c32 = P.candidates(7, slot, 1536, 2048), P.candidates(7, slot, 1536, 2048, np.float32)
        assert np.abs(c64 - c32).max() <= 1
        diff += int((c64 != c32).sum()); total += c64.size
    assert diff <= 0.01 * total


def test_parallel_selection_has_the_distribution_of_nonuniform_sampling():
    """The first n distinct valid candidates of the restated Philox stream against PatchData._nonuniform: pooled indices of 2048
    patches each, two-sample KS statistic at most KS_BAR (measured here: 0.0016 .. 0.0155 against the ten calibration runs)."""
    from puflow_amd.data import PatchData
    pd = PatchData(np.zeros((1, N_IN, 3), np.float32), np.zeros((1, N, 3), np.float32), seed=100)
    ref = np.concatenate([pd._nonuniform(N_IN, N) for _ in range(PATCHES)])
    mine = []
    for slot in range(PATCHES):
        idx, rounds, short = P.select(P.candidates(2021, slot, N_IN, 2048), N_IN, N)
        assert not short and len(set(idx.tolist())) == N and idx.min() >= 0 and idx.max() < N_IN
        mine.append(idx)
    ks = P.ks_statistic(np.concatenate(mine), ref, N_IN)
    print(f"KS(restated selection, _nonuniform) = {ks:.4f}  bar {KS_BAR}")
    assert ks <= KS_BAR
