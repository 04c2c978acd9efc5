"""Ragged passes without a GPU: how the CLI groups files of different sizes (upsample.plan_passes) and the scratch tables
pf_fps_ragged works from (pf_fps_ragged_layout: a host function of the library)."""
import random

import pytest


def _check_plan(sizes, cloud_batch, pass_points):
    from puflow_amd.upsample import plan_passes
    passes = plan_passes(sizes, cloud_batch, pass_points)
    assert [i for a, b in passes for i in range(a, b)] == list(range(len(sizes)))         # every file once, in file order
    for k, (a, b) in enumerate(passes):
        assert 1 <= b - a <= max(cloud_batch, 1)
        if pass_points is not None:
            assert sum(sizes[a:b]) <= pass_points or b - a == 1                            # a larger file: a pass of its own
        if k + 1 < len(passes):                                                            # greedy: the next file did not fit
            assert b - a == max(cloud_batch, 1) or (pass_points is not None and sum(sizes[a:b + 1]) > pass_points)
    return passes


def test_plan_passes_rules():
    from puflow_amd.upsample import plan_passes
    assert plan_passes([], 16) == []
    assert _check_plan([5000, 4100, 5903, 2048, 5000], 16, None) == [(0, 5)]               # sizes no longer split a pass
    assert _check_plan([5000, 4100, 5903, 2048, 5000], 2, None) == [(0, 2), (2, 4), (4, 5)]
    assert _check_plan([5000, 4100, 5903, 2048, 5000], 1, None) == [(i, i + 1) for i in range(5)]
    assert _check_plan([5000, 4100, 5903, 2048, 5000], 0, None) == [(i, i + 1) for i in range(5)]
    assert _check_plan([5000, 4100, 5903, 2048, 5000], 16, 10000) == [(0, 2), (2, 4), (4, 5)]
    assert _check_plan([300, 50000, 300, 300], 16, 1000) == [(0, 1), (1, 2), (2, 4)]       # one file above the limit
    assert _check_plan([1000, 1000], 16, 2000) == [(0, 2)]                                 # the limit itself is allowed
    rng = random.Random(7)
    for _ in range(200):
        sizes = [rng.choice([256, 300, 2048, 5000, 5903, 40000]) for _ in range(rng.randint(1, 40))]
        _check_plan(sizes, rng.choice([1, 2, 3, 16, 64]), rng.choice([None, 256, 6000, 20000, 10 ** 6]))


@pytest.mark.parametrize("count,cloud_batch", [(1, 16), (16, 16), (17, 16), (40, 16), (7, 3), (5, 1)])
def test_plan_passes_equal_sizes_group_as_before(count, cloud_batch):
    """All files of one size and no point limit: runs of `cloud_batch` files, the grouping the CLI had before ragged passes."""
    from puflow_amd.upsample import plan_passes
    before = [(a, min(a + cloud_batch, count)) for a in range(0, count, cloud_batch)]
    assert plan_passes([5000] * count, cloud_batch, None) == before


def test_cli_loop_and_plan_share_one_rule():
    """The CLI decides file by file (it draws every file's shuffle in file order while loading): replaying its loop with
    pass_is_full gives plan_passes' ranges."""
    from puflow_amd.upsample import pass_is_full, plan_passes
    rng = random.Random(11)
    for _ in range(100):
        sizes = [rng.randint(256, 9000) for _ in range(rng.randint(1, 30))]
        cb, pp = rng.choice([1, 4, 16]), rng.choice([None, 9000, 30000])
        passes, pending = [], []
        for i, n in enumerate(sizes):
            if pass_is_full(len(pending), sum(sizes[j] for j in pending), n, cb, pp):
                passes.append((pending[0], pending[-1] + 1))
                pending = []
            pending.append(i)
        passes.append((pending[0], pending[-1] + 1))
        assert passes == plan_passes(sizes, cb, pp)


@pytest.fixture(scope="module")
def built_lib():
    from puflow_amd import build
    return build.build(verbose=False)


@pytest.mark.parametrize("sizes,group", [([5000, 4100, 5903, 2048, 5000], 0), ([99840, 79360, 119040, 40960, 5120], 1280),
                                         ([10240, 9000], 0), ([8191, 8192, 8193, 300, 262144, 262145], 0), ([777], 0),
                                         ([40960, 5120, 15361, 40961], 1280)])
def test_fps_ragged_layout_is_what_the_kernels_expect(built_lib, sizes, group):
    """Scratch rows: in cloud order, disjoint, each at least its cloud's points long (the single-workgroup kernel's running
    distances) and starting on a 64-bit boundary (the cooperative kernel reads its ring there as 64-bit words; the ring and the
    dense kernel's status slot, 2050 words, fit the smallest cooperative row).  Workgroups: 0 below 8192 points, else
    ceil(n / (256 ppt)) <= 32 with one ppt for the pass.  Status words: one per cloud, behind every row."""
    from puflow_amd import ops
    lay = ops.fps_ragged_layout(sizes, group)
    off, wgs, ppt = lay["scratch_off"], lay["workgroups"], lay["ppt"]
    assert off[0] == 0 and all(o % 2 == 0 for o in off)
    for i, n in enumerate(sizes):
        end = off[i + 1] if i + 1 < len(sizes) else 2 * lay["status_words"][0]
        assert end - off[i] >= n and end - off[i] <= n + 1
        coop = 8192 <= n <= 32 * 8192
        if coop:
            assert ppt in (1, 4, 8, 12, 16, 20, 24, 32)
            assert wgs[i] == -(-n // (256 * ppt)) and 1 <= wgs[i] <= 32
            assert end - off[i] >= 2 * (4 * 4 * 128 + 2)
        else:
            assert wgs[i] == 0
    assert (ppt == 0) == all(w == 0 for w in wgs)
    st = lay["status_words"]
    assert len(st) == len(sizes) and st[0] * 2 >= off[-1] + sizes[-1]
    assert all(b - a == 2 for a, b in zip(st, st[1:]))                                     # status, then the round count
    assert lay["total_floats"] == 2 * (st[-1] + 2)
    if group == 1280 and max(sizes) >= 10240:
        assert ppt == 20                                                                  # one patch per wave (64 x 20 points)


def test_ragged_entry_points_validate_before_any_launch(built_lib):
    from puflow_amd import _lib
    lib = _lib.load()
    c = _lib.counts
    assert lib.pf_normalize_pc_ragged(None, c([4]), 1, None, None, None, None) == -1
    assert lib.pf_normalize_pc_ragged(8, c([4, 0]), 2, 8, 8, 8, None) == -2
    assert lib.pf_fps_ragged(8, c([300]), c([301]), 1, 0, 8, 8, None) == -2               # more samples than points
    assert lib.pf_fps_ragged(8, c([300]), c([4]), 1, 0, 12, 8, None) == -2                # scratch not 8-byte aligned
    assert lib.pf_fps_ragged_layout(c([300, -1]), 2, 0, None, None, None, None, None) == -2
    assert lib.pf_knn_large_ragged(8, 8, c([300, 200]), c([4, 4]), 2, 256, 8, None, None) == -2     # K > a cloud's points
    assert lib.pf_knn_large_ragged(8, 8, c([30000]), c([4]), 1, 9000, 8, None, None) == -3
    assert lib.pf_nn1_ragged(8, 8, c([4]), c([0]), 1, 8, None, None) == -2
    assert lib.pf_nn1_ragged(None, 8, c([4]), c([4]), 1, 8, None, None) == -1
