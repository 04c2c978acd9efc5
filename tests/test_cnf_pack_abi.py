"""The C ABI of the device-side CNF weight packer (csrc/cnf_pack.hip: pf_cnf_pack_blocks) without a GPU: the entry point is
declared in the header, bound from it, exported, and rejects bad arguments before the device is touched."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from puflow_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _args(nb=2, cds=(32, 128), null_param=None, null_out=None):
    from puflow_amd import _lib
    p = 64                                                              # any non-null value: nothing is dereferenced
    params = (ctypes.c_void_p * (16 * nb))(*[None if j == null_param else p for j in range(16 * nb)])
    outs = [(ctypes.c_void_p * nb)(*[None if (null_out == (k, j)) else p for j in range(nb)]) for k in range(3)]
    #       params cd nb rec hb hc hplain image meta stream
    return [params, _lib.counts(cds), nb, p, p, outs[0], outs[1], outs[2], p, None]


def test_pack_entry_point_is_declared_bound_and_exported(lib):
    from puflow_amd import _lib
    assert hasattr(lib, "pf_cnf_pack_blocks")
    res, args = _lib.SIGNATURES["pf_cnf_pack_blocks"]
    assert res is ctypes.c_int and len(args) == 10
    assert args[0].elem is ctypes.c_void_p and args[1].elem is ctypes.c_int and args[8].elem is ctypes.c_double
    assert args[3].elem is ctypes.c_float and args[9] is ctypes.c_void_p


def test_pack_validates_arguments(lib):
    for j in (0, 1, 3, 4, 5, 6, 7, 8):                                  # every pointer argument
        bad = _args(); bad[j] = None
        assert lib.pf_cnf_pack_blocks(*bad) == -1, j
    assert lib.pf_cnf_pack_blocks(*_args(null_param=17)) == -1           # one parameter pointer of block 1
    for k in range(3):
        assert lib.pf_cnf_pack_blocks(*_args(null_out=(k, 1))) == -1, k  # one per-block output pointer
    for nb in (0, -1, 7):                                                # 1 <= nb <= 6
        bad = _args(); bad[2] = nb
        assert lib.pf_cnf_pack_blocks(*bad) == -2, nb
    for cds in ((32, 48), (0, 32), (256, 128)):                          # context width: 32, 64 or 128
        assert lib.pf_cnf_pack_blocks(*_args(cds=cds)) == -3, cds


def test_pack_rejects_host_arrays_of_another_type(lib):
    """The binding made from the header checks the element type of host arrays: a float array for the int widths never reaches C."""
    bad = _args()
    bad[1] = (ctypes.c_float * 2)(32.0, 128.0)
    with pytest.raises(ctypes.ArgumentError):
        lib.pf_cnf_pack_blocks(*bad)
