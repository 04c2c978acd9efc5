"""The CNF layouts have one home, csrc/pf_cnf.h: its named offsets equal packing.py's, each of the three layouts tiles its
record without gap or overlap, and the kernel sources no longer define the record sizes themselves.  Layout constants only;
the literal offsets stay pinned independently by test_oracle_cnf.py, test_cnf_grad_abi.py and test_gpu_cnf_grad.py."""
import os
import re

import pytest

from puflow_amd import packing

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "puflow_amd", "csrc")
INT_DEFS = re.compile(r"^\s*constexpr\s+int\s+([^;]*);", re.M)      # one statement may define several: NAME = value, NAME = value;


def int_constants(text):
    return {name: int(value) for stmt in INT_DEFS.findall(text) for name, value in re.findall(r"(\w+)\s*=\s*(\d+)\s*(?:,|$)", stmt.strip())}


# (name, floats) in record order; the last name of each is the record's size
RECORD = (("CNF_W2", 4096), ("CNF_W2T", 4096), ("CNF_W3", 1024), ("CNF_W1B", 256), ("CNF_W3T", 256), ("CNF_B1", 64),
          ("CNF_B2", 64), ("CNF_B3", 16), ("CNF_TV", 288), ("CNF_REC", 0))
CONTEXT = (("CNF_CTX_G1", 64), ("CNF_CTX_B1", 64), ("CNF_CTX_G2", 64), ("CNF_CTX_B2", 64), ("CNF_CTX_G3", 16),
           ("CNF_CTX_B3", 16), ("CNF_CTX", 0))
GRADIENT = (("CNF_GRAD_W2", 64 * 64), ("CNF_GRAD_W1", 64 * 3), ("CNF_GRAD_B1", 64), ("CNF_GRAD_B2", 64), ("CNF_GRAD_W3", 3 * 64),
            ("CNF_GRAD_B3", 3), ("CNF_GRAD_UNUSED", 1), ("CNF_GRAD_TV", 288), ("CNF_GRAD", 0))


@pytest.fixture(scope="module")
def header():
    return int_constants(open(os.path.join(CSRC, "pf_cnf.h")).read())


@pytest.mark.parametrize("layout", [RECORD, CONTEXT, GRADIENT], ids=["record", "context", "gradient"])
def test_header_and_packing_agree_and_tile(header, layout):
    at = 0
    for name, size in layout:
        assert header[name] == getattr(packing, name) == at, name
        at += size


def test_the_one_unused_gradient_word(header):
    assert header["CNF_GRAD_UNUSED"] == 4611 and header["CNF_GRAD_TV"] - header["CNF_GRAD_UNUSED"] == 1


def test_derived_tables_follow_the_names(header):
    assert header["CNF_TV"] + header["CNF_CTX"] == header["CNF_REC"]           # the time coefficients are one context row
    assert header["CNF_GRAD_TV"] + header["CNF_CTX"] == header["CNF_GRAD"]
    assert packing.CNF_CTX_SLOTS == tuple((header[n], rows) for n, rows in (
        ("CNF_CTX_G1", 64), ("CNF_CTX_B1", 64), ("CNF_CTX_G2", 64), ("CNF_CTX_B2", 64), ("CNF_CTX_G3", 3), ("CNF_CTX_B3", 3)))


@pytest.mark.parametrize("source", ["cnf.hip", "cnf_bwd.hip"])
def test_kernel_sources_take_the_sizes_from_the_header(source):
    text = open(os.path.join(CSRC, source)).read()
    assert '#include "pf_cnf.h"' in text
    assert not set(int_constants(text)) & {"CNF_REC", "CNF_CTX", "CNF_GRAD"}
