"""The CNF modules' host-side pieces without a GPU: the digest of the deferred controller's tables
(puflow_amd/cnf_train.py: digest_train_tables, what `PointInterpFlow.check_train_logs` makes of its one read) on synthetic host
tables, and the one table of the integration order (puflow_amd/cnf_schedule.py)."""
import os
import subprocess
import sys

import pytest
import torch

from puflow_amd import cnf, cnf_schedule
from puflow_amd._lib import PuflowHipError
from puflow_amd.cnf_schedule import MAX_NUM_STEPS, PACK_ROW
from puflow_amd.cnf_train import digest_train_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tables():
    """-> (logs [12, 16], sticky [13, 4], seen): nothing has run."""
    return torch.zeros((12, 16), dtype=torch.float64), torch.zeros((13, 4), dtype=torch.int32), torch.zeros((13, 4), dtype=torch.int32)


def _enter(sticky, k, status, not_clean=1, last=0):
    """Row k of the sticky table after `not_clean` runs that ended with `status` (runs, not clean, status, max attempts / block)."""
    sticky[k] = torch.tensor([not_clean, not_clean, status, last], dtype=torch.int32)


# ---- the table digest ---------------------------------------------------------------------------------------------------------------
def test_attempts_that_ran_out_double_that_rows_attempts():
    logs, sticky, seen = _tables()
    k = cnf._log_row(2, True)
    _enter(sticky, k, 4)
    budget = {(2, True): (5, 8), (0, False): (3, 4)}
    assert digest_train_tables(logs, sticky, seen, budget) == (1, 1)
    assert budget == {(2, True): (10, 8), (0, False): (3, 4)}
    budget = {(2, True): (0, 8)}                                          # the floor
    assert digest_train_tables(logs, sticky, seen, budget)[0] == 1 and budget[(2, True)] == (2, 8)
    budget = {(2, True): (MAX_NUM_STEPS - 1, 8)}                          # the ceiling
    assert digest_train_tables(logs, sticky, seen, budget)[0] == 1 and budget[(2, True)] == (MAX_NUM_STEPS, 8)


def test_a_full_tape_doubles_the_cap_and_lifts_the_attempts_to_it():
    logs, sticky, seen = _tables()
    _enter(sticky, cnf._log_row(4, False), 3)
    budget = {(4, False): (4, 8)}
    assert digest_train_tables(logs, sticky, seen, budget) == (1, 1)
    assert budget == {(4, False): (16, 16)}
    budget = {(4, False): (40, 8)}                                        # attempts above the new cap stay
    digest_train_tables(logs, sticky, seen, budget)
    assert budget == {(4, False): (40, 16)}
    budget = {(4, False): (4, MAX_NUM_STEPS)}
    digest_train_tables(logs, sticky, seen, budget)
    assert budget == {(4, False): (MAX_NUM_STEPS, MAX_NUM_STEPS)}


def test_a_row_without_a_learnt_budget_is_counted_but_not_entered():
    logs, sticky, seen = _tables()
    _enter(sticky, cnf._log_row(1, False), 4)
    _enter(sticky, cnf._log_row(1, True), 3)
    budget = {(0, False): (3, 4)}
    assert digest_train_tables(logs, sticky, seen, budget) == (2, 1)
    assert budget == {(0, False): (3, 4)}


def test_an_error_state_behind_a_short_row_is_its_consequence_alone_it_raises():
    logs, sticky, seen = _tables()
    k = cnf._log_row(3, True)                                             # row 8: behind every f integration
    _enter(sticky, k, 1)
    logs[k, 0], logs[k, 1] = -1.25, 0.5
    _enter(sticky, cnf._log_row(5, False), 4)                             # row 5 fell short first: row 8 choked on its NaN
    budget = {(5, False): (5, 8)}
    assert digest_train_tables(logs, sticky, seen, budget) == (1, 1)
    assert budget == {(5, False): (10, 8)}
    sticky[cnf._log_row(5, False)] = 0                                    # the same row 8 with no short row before it
    with pytest.raises(PuflowHipError, match=r"non-finite error norm in block 3 at t = -1\.25"):
        digest_train_tables(logs, sticky, seen, budget)
    _enter(sticky, k, 2)
    with pytest.raises(PuflowHipError, match=r"underflow in dt \(0\.5\) at t = -1\.25, block 3"):
        digest_train_tables(logs, sticky, seen, budget)
    assert budget == {(5, False): (10, 8)}
    _enter(sticky, cnf._log_row(0, True), 4)                              # a short row BEHIND the error does not excuse it
    with pytest.raises(PuflowHipError):
        digest_train_tables(logs, sticky, seen, budget)


@pytest.mark.parametrize("bit,path", [(1, "f16x2"), (2, "f16n")])
def test_a_pack_status_raises_the_packers_error_for_the_recorded_block(bit, path):
    logs, sticky, seen = _tables()
    _enter(sticky, PACK_ROW, bit, last=4)                                 # word 3 of the pack's row: the block
    _enter(sticky, 0, 4)                                                  # (the NaN weights made the integrations fall short too)
    budget = {(0, False): (5, 8)}
    with pytest.raises(ValueError, match=f"block 4: .*{path} path"):
        digest_train_tables(logs, sticky, seen, budget)
    assert budget == {(0, False): (5, 8)}


def test_unchanged_counts_give_zero_and_touch_nothing():
    logs, sticky, seen = _tables()
    for k, st in ((0, 4), (7, 3), (9, 1), (PACK_ROW, 1)):                 # old news: `seen` holds the same counts
        _enter(sticky, k, st, not_clean=2)
    budget = {(0, False): (5, 8), (4, True): (4, 8)}
    before = (logs.clone(), sticky.clone(), dict(budget))
    assert digest_train_tables(logs, sticky, sticky.clone(), budget) == (0, 0)
    assert torch.equal(logs, before[0]) and torch.equal(sticky, before[1]) and budget == before[2]
    assert cnf.PointInterpFlow(3).check_train_logs() == 0                 # no tables yet: nothing to read


def test_skipped_steps_are_the_most_new_counts_of_any_integration():
    logs, sticky, seen = _tables()
    _enter(sticky, 2, 4, not_clean=5)
    _enter(sticky, 11, 3, not_clean=7)
    _enter(seen, 11, 3, not_clean=4)                                      # four of the seven are old
    _enter(seen, PACK_ROW, 1, not_clean=9)                                # the pack's row does not count (and is not new here)
    _enter(sticky, PACK_ROW, 1, not_clean=9)
    assert digest_train_tables(logs, sticky, seen, {}) == (2, 5)


# ---- the integration order ----------------------------------------------------------------------------------------------------------
def test_the_order_has_one_table():
    keys = cnf.schedule_keys()
    assert len(keys) == 12 == PACK_ROW == cnf.PACK_ROW
    for k, (i, reverse) in enumerate(keys):
        assert cnf._log_row(i, reverse) == k and cnf._row_key(k) == (i, reverse)
    assert [i for i, r in keys if not r] == list(range(6)) and [i for i, r in keys if r] == list(reversed(range(6)))
    assert cnf._ScheduleDev(cnf.uniform_schedule(1), torch.device("cpu")).keys == keys
    for name in ("schedule_keys", "_log_row", "_row_key", "_ScheduleDev", "PACK_ROW"):
        assert getattr(cnf, name) is getattr(cnf_schedule, name), name


def test_the_schedule_module_loads_without_the_library():
    code = ("import sys; from puflow_amd import cnf_schedule as s; assert s.uniform_schedule(2)[(0, False)] == (0.0, 0.5, 1.0); "
            "bad = [m for m in sys.modules if m.startswith('puflow_amd.') and m.split('.')[1] in "
            "('_lib', '_abi', 'cnf', 'cnf_engine', 'cnf_train', 'interpflow')]; assert not bad, bad")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
