"""The C ABI of the taped CNF integration and its one-launch reverse sweep (csrc/cnf.hip: pf_cnf_steps_taped, csrc/cnf_bwd.hip:
pf_cnf_tape_vjp) without a GPU: the entry points are exported and reject bad arguments before the device is touched."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from puflow_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_tape_entry_points_are_exported(lib):
    for name in ("pf_cnf_tape_vjp", "pf_cnf_tape_vjp_workspace_bytes", "pf_cnf_steps_taped"):
        assert hasattr(lib, name), name


def test_tape_vjp_validates_arguments(lib):
    p = 64                                                              # any non-null value: nothing is dereferenced
    #     states steps n_steps sgn ctx e rec ybar ctxbar grad rows R ws stream
    ok = [p, p, 3, 1.0, p, p, p, p, p, p, 40, 4, p, None]
    for j in (0, 1, 4, 5, 6, 7, 8, 9, 12):                              # every pointer
        bad = list(ok); bad[j] = None
        assert lib.pf_cnf_tape_vjp(*bad) == -1, j
    for rows, R in ((0, 4), (-8, 4), (40, 0), (40, -1), (40, 20), (40, 3)):     # rows <= 0, R <= 0, R > 16, rows % R != 0
        bad = list(ok); bad[10], bad[11] = rows, R
        assert lib.pf_cnf_tape_vjp(*bad) == -2, (rows, R)
    for n in (0, -1):
        bad = list(ok); bad[2] = n
        assert lib.pf_cnf_tape_vjp(*bad) == -2, n


def test_tape_vjp_workspace_is_the_per_evaluation_kernels(lib):
    for rows, R in ((40, 4), (201, 3), (32768, 1)):
        assert lib.pf_cnf_tape_vjp_workspace_bytes(rows, R) == lib.pf_cnf_rhs_vjp_workspace_bytes(rows, R) > 0
    assert lib.pf_cnf_tape_vjp_workspace_bytes(201, 3) == 4 * 4900 * 4
    for rows, R in ((0, 1), (40, 0), (40, 3), (40, 20)):
        assert lib.pf_cnf_tape_vjp_workspace_bytes(rows, R) == lib.pf_cnf_rhs_vjp_workspace_bytes(rows, R) < 0


def test_steps_taped_validates_arguments(lib):
    p = 64
    #     ctl states steps cap fa fb ctx e rec rtol atol rows R n_attempts ws stream
    ok = [p, p, p, 8, p, p, p, p, p, 1e-5, 1e-5, 40, 4, 2, p, None]
    for j in (0, 1, 2, 4, 5, 6, 7, 8, 14):
        bad = list(ok); bad[j] = None
        assert lib.pf_cnf_steps_taped(*bad) == -1, j
    for j, v in ((3, 0), (3, -2), (11, 0), (12, 0), (13, 0)):           # cap, rows, R, n_attempts
        bad = list(ok); bad[j] = v
        assert lib.pf_cnf_steps_taped(*bad) == -2, (j, v)
