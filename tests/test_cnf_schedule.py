"""Frozen CNF step schedules without a GPU (puflow_amd/cnf.py: uniform_schedule, refine_schedule, save_schedule / load_schedule,
validate_schedule, schedule_from_steps, schedule_step_lists) and the C ABI of the one-launch replay (csrc/cnf_replay.hip:
pf_cnf_replay): exported, declared, and bad arguments rejected before the device is touched."""
import os

import pytest
import torch

from puflow_amd import cnf
from puflow_amd.weights import CNF_PU1K_END_TIMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _add32(a, b):
    return float(torch.tensor(a, dtype=torch.float32) + torch.tensor(b, dtype=torch.float32))


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def test_schedule_keys_are_the_running_order():
    keys = cnf.schedule_keys()
    assert keys == [(i, False) for i in range(6)] + [(i, True) for i in (5, 4, 3, 2, 1, 0)]
    assert [cnf._log_row(i, r) for i, r in keys] == list(range(12))


def test_uniform_schedule():
    s = cnf.uniform_schedule(4)
    assert sorted(s) == sorted(cnf.schedule_keys())
    assert all(g == (0.0, 0.25, 0.5, 0.75, 1.0) for g in s.values())
    assert cnf.uniform_schedule(1)[(3, True)] == (0.0, 1.0)
    assert cnf.uniform_schedule(3)[(0, False)][-1] == 1.0                 # the end is 1.0 itself, not 3 x (1 / 3)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError):
            cnf.uniform_schedule(bad)


def test_refine_schedule_halves_every_step_and_keeps_the_old_boundaries():
    s = cnf.uniform_schedule(2)
    s[(5, False)] = (0.0, 0.02, 0.1, 0.3, 0.6, 1.0)
    r = cnf.refine_schedule(s, 2)
    assert r[(0, True)] == (0.0, 0.25, 0.5, 0.75, 1.0)
    g = r[(5, False)]
    assert len(g) == 11 and g[::2] == s[(5, False)]
    assert all(abs(m - (a + b) / 2) < 1e-15 for a, m, b in zip(g[0::2], g[1::2], g[2::2]))
    assert cnf.refine_schedule(s, 1) == cnf.validate_schedule(s)
    assert len(cnf.refine_schedule(s, 3)[(5, False)]) == 16
    with pytest.raises(ValueError):
        cnf.refine_schedule(s, 0)


def test_json_round_trip_is_exact(tmp_path):
    s = cnf.uniform_schedule(3)
    s[(4, True)] = (0.0, 1e-7, 0.1 + 0.2, 2 / 3, 1.0)                     # float64 values with no short decimal form
    path = tmp_path / "sched.json"
    cnf.save_schedule(s, path)
    back = cnf.load_schedule(path)
    assert back == cnf.validate_schedule(s)
    assert all(isinstance(k, tuple) and isinstance(g, tuple) for k, g in back.items())
    (tmp_path / "other.json").write_text('{"format": "something else"}')
    with pytest.raises(ValueError, match="not a step-schedule file"):
        cnf.load_schedule(tmp_path / "other.json")
    (tmp_path / "broken.json").write_text("{")
    with pytest.raises(ValueError, match="not a step-schedule file"):
        cnf.load_schedule(tmp_path / "broken.json")


@pytest.mark.parametrize("edit,match", [
    (lambda s: s.pop((2, True)), "no grid"),
    (lambda s: s.__setitem__((6, False), (0.0, 1.0)), "unknown integration"),
    (lambda s: s.__setitem__((1, False), (0.0, 0.5, 0.5, 1.0)), "strictly increasing"),
    (lambda s: s.__setitem__((1, False), (0.0, 0.7, 0.3, 1.0)), "strictly increasing"),
    (lambda s: s.__setitem__((1, False), (0.1, 0.5, 1.0)), "starts at 0.0"),
    (lambda s: s.__setitem__((1, False), (0.0, 0.5, 0.99)), "ends at 1.0"),
    (lambda s: s.__setitem__((1, False), (1.0,)), "at least"),
    (lambda s: s.__setitem__((1, False), (0.0, float("nan"), 1.0)), "non-finite"),
    (lambda s: s.__setitem__((1, False), "ab"), "sequence of numbers"),
])
def test_validation_errors_say_what_is_wrong(edit, match):
    s = dict(cnf.uniform_schedule(2))
    edit(s)
    with pytest.raises(ValueError, match=match):
        cnf.validate_schedule(s)
    with pytest.raises(ValueError):
        cnf.validate_schedule([0.0, 1.0])


def test_the_net_validates_on_assignment():
    net = cnf.PointInterpFlow(3)
    assert net.step_schedule is None
    net.step_schedule = cnf.uniform_schedule(2)
    assert net.step_schedule[(5, True)] == (0.0, 0.5, 1.0)
    with pytest.raises(ValueError):
        net.step_schedule = {(0, False): (0.0, 1.0)}
    net.step_schedule = None
    assert net.step_schedule is None
    with pytest.raises(ValueError):
        net.schedule_error_ratios()


# ---- the fp32 step-list rule --------------------------------------------------------------------------------------------------------
def _lists(schedule, T_ends):
    sdev = cnf._ScheduleDev(cnf.validate_schedule(schedule), torch.device("cpu"))
    steps = sdev.lists(torch.tensor(T_ends, dtype=torch.float64))
    assert steps.dtype == torch.float32 and steps.shape == (12, max(sdev.n), 2)
    return sdev, [[(float(s), float(h)) for s, h in steps[k, :n].tolist()] for k, n in enumerate(sdev.n)]


def test_step_lists_are_contiguous_in_fp32_and_land_on_the_end_time():
    s = cnf.uniform_schedule(7)
    s[(5, False)] = (0.0, 1e-4, 0.02, 0.1, 0.3, 0.6, 1.0)
    s[(4, True)] = (0.0, 0.5, 1.0)
    sdev, lists = _lists(s, CNF_PU1K_END_TIMES)
    for (i, reverse), steps, grid in zip(sdev.keys, lists, (s[k] for k in sdev.keys)):
        T = CNF_PU1K_END_TIMES[i]
        t0, t1 = (-T, 0.0) if reverse else (0.0, T)
        assert len(steps) == len(grid) - 1
        assert steps[0][0] == _f32(t0)
        for (a, h), (b, _) in zip(steps, steps[1:]):
            assert h > 0 and b == _add32(a, h), (i, reverse, a, h, b)          # s' = s + h in fp32, bit for bit
        for (a, h), g0, g1 in list(zip(steps, grid, grid[1:]))[:-1]:
            assert h == _f32(T * (g1 - g0)), (i, reverse)                     # h_k = fl(T d_k)
        a, h = steps[-1]
        assert h == _f32(t1 - a)                                              # the last step is cut to end on t1 ...
        assert abs((a + h) - t1) <= 2.0 ** -23 * T                            # ... within half an fp32 ulp of the interval
        assert abs(h - T * (grid[-1] - grid[-2])) <= 12 * 2.0 ** -23 * T       # and is the grid's last step but for the drift of s


def test_a_recorded_list_comes_back_bit_for_bit():
    """schedule_from_steps then schedule_step_lists: the (s, h) a taped controller would record - fp32 values, s' = s + h in
    fp32, a tiny first step, the covering step cut - reproduce exactly, for the long block too."""
    g = torch.Generator().manual_seed(5)
    recorded = []
    for i, reverse in cnf.schedule_keys():
        T = CNF_PU1K_END_TIMES[i]
        t0, t1 = (-T, 0.0) if reverse else (0.0, T)
        s, steps = _f32(t0), []
        h = _f32(T * 3e-5)
        while s + h < t1:
            steps.append((s, h))
            s = _add32(s, h)
            h = _f32(h * float(1.2 + 2.5 * torch.rand(1, generator=g)))
        steps.append((s, _f32(t1 - s)))
        recorded.append(steps)
    assert max(len(r) for r in recorded) >= 8
    sched = cnf.schedule_from_steps(recorded, CNF_PU1K_END_TIMES)
    _, lists = _lists(sched, CNF_PU1K_END_TIMES)
    assert lists == recorded
    # refined by two: twice the steps, still contiguous, still on t1
    _, fine = _lists(cnf.refine_schedule(sched, 2), CNF_PU1K_END_TIMES)
    assert [len(f) for f in fine] == [2 * len(r) for r in recorded]
    for (i, reverse), f, r in zip(cnf.schedule_keys(), fine, recorded):
        t1 = 0.0 if reverse else CNF_PU1K_END_TIMES[i]
        assert f[0][0] == r[0][0] and f[-1][1] == _f32(t1 - f[-1][0])
        assert all(b == _add32(a, h) for (a, h), (b, _) in zip(f, f[1:]))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from puflow_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_replay_entry_points_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "puflow_hip.h")).read()
    for name in ("pf_cnf_replay", "pf_cnf_replay_workspace_bytes"):
        assert hasattr(lib, name), name
        assert f" {name}(" in header, name
    from puflow_amd import build
    assert "cnf_replay.hip" in build.SOURCES and build.EXTRA_FLAGS["cnf_replay.hip"] == build.EXTRA_FLAGS["cnf.hip"]


def test_replay_validates_arguments(lib):
    p = 64                                                              # any non-null value: nothing is dereferenced
    #     x x_stride steps n_steps reverse ctx e rec states y_out f_start f_end errsq rtol atol rows R ws stream
    ok = [p, 3, p, 5, 0, p, p, p, p, p, p, p, p, 1e-5, 1e-5, 40, 4, p, None]
    for j in (0, 2, 5, 6, 7, 9):                                        # every required pointer
        bad = list(ok); bad[j] = None
        assert lib.pf_cnf_replay(*bad) == -1, j
    bad = list(ok); bad[17] = None                                      # errsq without its workspace
    assert lib.pf_cnf_replay(*bad) == -1
    for j, v in ((3, 0), (3, -1), (1, 2), (1, 5), (16, 0), (16, -1), (16, 3), (15, 0), (15, -8)):
        bad = list(ok); bad[j] = v                                      # n_steps < 1, x_stride, R < 1, rows % R, rows <= 0
        assert lib.pf_cnf_replay(*bad) == -2, (j, v)


def test_replay_workspace_bytes(lib):
    assert lib.pf_cnf_replay_workspace_bytes(40, 3) == 1 * 4 * 3 * 8                # one workgroup of four waves, three steps
    assert lib.pf_cnf_replay_workspace_bytes(65, 1) == 2 * 4 * 1 * 8
    assert lib.pf_cnf_replay_workspace_bytes(1 << 20, 10) == 1024 * 4 * 10 * 8      # at most 1024 workgroups
    for rows, n in ((0, 3), (-1, 3), (40, 0), (40, -2)):
        assert lib.pf_cnf_replay_workspace_bytes(rows, n) < 0
