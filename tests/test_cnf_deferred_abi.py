"""The C ABI of the deferred taped integration (csrc/cnf.hip: pf_cnf_tape_close, pf_cnf_init_dev; csrc/cnf_bwd.hip:
pf_cnf_tape_vjp_dev; csrc/pointwise.hip: pf_cnf_context_dev; csrc/cnf_pack.hip: pf_cnf_pack_status) without a GPU: the entry points
are declared in the header, pass the export map, are bound from the header's types, and reject bad arguments before the device is
touched."""
import ctypes
import os
import re

import pytest

NEW = ("pf_cnf_tape_close", "pf_cnf_tape_vjp_dev", "pf_cnf_init_dev", "pf_cnf_context_dev", "pf_cnf_pack_status")


@pytest.fixture(scope="module")
def lib():
    from puflow_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    from puflow_amd import _abi, build
    _, _, sigs = _abi.header()
    with open(build.EXPORTS) as f:
        glob = re.search(r"global:\s*([\w*]+)\s*;", f.read()).group(1)
    assert glob.endswith("*")
    for name in NEW:
        assert name in sigs, name                                       # include/puflow_hip.h
        assert name.startswith(glob[:-1]), name                         # csrc/exports.map
        fn = getattr(lib, name)                                         # the dynamic symbol table
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == sigs[name][1], name
    # the derived binding: the step count's place is taken by (const double* ctl, int cap)
    host, dev = sigs["pf_cnf_tape_vjp"][1], sigs["pf_cnf_tape_vjp_dev"][1]
    assert len(dev) == len(host) + 1 and dev[:2] == host[:2] and dev[4:] == host[3:]
    assert dev[2].elem is ctypes.c_double and dev[3] is ctypes.c_int
    close = sigs["pf_cnf_tape_close"][1]
    assert [getattr(t, "elem", t) for t in close] == [ctypes.c_double, ctypes.c_float, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                                      ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    assert os.path.exists(build.LIB)


def test_tape_close_validates_arguments(lib):
    p = 64                                                              # any non-null value: nothing is dereferenced
    #     ctl states cap fa fb rows y_out f_end sticky stream
    ok = [p, p, 8, p, p, 40, p, p, p, None]
    for j in (0, 1, 3, 4, 6, 7, 8):
        bad = list(ok); bad[j] = None
        assert lib.pf_cnf_tape_close(*bad) == -1, j
    for j, v in ((2, 0), (2, -3), (5, 0), (5, -1)):                     # cap, rows
        bad = list(ok); bad[j] = v
        assert lib.pf_cnf_tape_close(*bad) == -2, (j, v)


def test_tape_vjp_dev_validates_arguments(lib):
    p = 64
    #     states steps ctl cap sgn ctx e rec ybar ctxbar grad rows R ws stream
    ok = [p, p, p, 3, 1.0, p, p, p, p, p, p, 40, 4, p, None]
    for j in (0, 1, 2, 5, 6, 7, 8, 9, 10, 13):
        bad = list(ok); bad[j] = None
        assert lib.pf_cnf_tape_vjp_dev(*bad) == -1, j
    for rows, R in ((0, 4), (-8, 4), (40, 0), (40, -1), (40, 20), (40, 3)):     # as pf_cnf_tape_vjp
        bad = list(ok); bad[11], bad[12] = rows, R
        assert lib.pf_cnf_tape_vjp_dev(*bad) == -2, (rows, R)
    for cap in (0, -1):
        bad = list(ok); bad[3] = cap
        assert lib.pf_cnf_tape_vjp_dev(*bad) == -2, cap


def test_device_side_pack_consumers_validate_arguments(lib):
    p = 64
    #     ctl x x_stride y f0 ctx e rec t_end n_tot extra_d0 extra_scale reverse rtol atol rows R ws stream
    ok = [p, p, 3, p, p, p, p, p, p, 160.0, None, 1.0, 0, 1e-5, 1e-5, 40, 1, p, None]
    for j in (0, 1, 3, 4, 5, 6, 7, 8, 17):
        bad = list(ok); bad[j] = None
        assert lib.pf_cnf_init_dev(*bad) == -1, j
    for j, v in ((2, 5), (9, 0.0), (15, 0), (16, 0)):                   # x_stride, n_tot, rows, R
        bad = list(ok); bad[j] = v
        assert lib.pf_cnf_init_dev(*bad) == -2, (j, v)
    #     c cd hc_image hb scales ctx T stream
    ok = [p, 64, p, p, p, p, 40, None]
    for j in (0, 2, 3, 4, 5):
        bad = list(ok); bad[j] = None
        assert lib.pf_cnf_context_dev(*bad) == -1, j
    bad = list(ok); bad[6] = 0
    assert lib.pf_cnf_context_dev(*bad) == -2
    bad = list(ok); bad[1] = 48
    assert lib.pf_cnf_context_dev(*bad) == -3                           # PF_ERR_UNSUPPORTED, as pf_cnf_context
    #     meta nb rec scales sticky stream
    ok = [p, 6, p, p, p, None]
    for j in (0, 2, 3, 4):
        bad = list(ok); bad[j] = None
        assert lib.pf_cnf_pack_status(*bad) == -1, j
    for nb in (0, 7):
        bad = list(ok); bad[1] = nb
        assert lib.pf_cnf_pack_status(*bad) == -2, nb


def test_switch_is_off_by_default_and_the_error_names_it():
    from puflow_amd import cnf, trainer
    assert trainer.default_cfg(model="continuous").cnf_deferred is False
    assert "cannot be captured" in trainer.GRAPH_ERROR and "cnf_deferred" in trainer.GRAPH_ERROR
    net = cnf.PointInterpFlow(3)
    assert net.train_deferred is False and net.tape_budget == {} and net.check_train_logs() == 0
    assert net.last_train_steps is None
    net.last_train_steps = [[(0.0, 0.1)]]
    assert net.last_train_steps == [[(0.0, 0.1)]]
    assert trainer.TrainerModule(trainer.default_cfg(model="continuous", cnf_deferred=True)).network.train_deferred is True
    assert [cnf._row_key(cnf._log_row(i, r)) for i in range(6) for r in (False, True)] == [(i, r) for i in range(6) for r in (False, True)]
