"""The C ABI of the CNF right-hand side's vector-Jacobian product (csrc/cnf_bwd.hip) without a GPU: the entry points are
exported and reject bad arguments before the device is touched; the host-side unpacking of its gradient record."""
import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def built_lib():
    from puflow_amd import build
    return build.build(verbose=False)


def test_vjp_entry_points_are_exported_and_validate_arguments(built_lib):
    from puflow_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "pf_cnf_rhs_vjp") and hasattr(lib, "pf_cnf_rhs_vjp_workspace_bytes")
    p = 64                                                              # any non-null value: nothing is dereferenced
    ok = [p, p, 0.1, 1.0, p, p, p, p, p, p, 40, 4, p, None]
    assert lib.pf_cnf_rhs_vjp(*(ok[:10] + [0, 4, p, None])) == -2       # rows <= 0
    assert lib.pf_cnf_rhs_vjp(*(ok[:10] + [-8, 4, p, None])) == -2
    assert lib.pf_cnf_rhs_vjp(*(ok[:10] + [40, 0, p, None])) == -2      # R <= 0
    assert lib.pf_cnf_rhs_vjp(*(ok[:10] + [40, -1, p, None])) == -2
    assert lib.pf_cnf_rhs_vjp(*(ok[:10] + [40, 3, p, None])) == -2      # rows not a multiple of R
    assert lib.pf_cnf_rhs_vjp(*(ok[:10] + [40, 20, p, None])) == -2     # R > 16: a point would straddle MFMA tiles
    for j in (0, 1, 4, 5, 6, 7, 8, 9, 12):                              # every pointer
        bad = list(ok); bad[j] = None
        assert lib.pf_cnf_rhs_vjp(*bad) == -1, j
    assert lib.pf_cnf_rhs_vjp_workspace_bytes(0, 1) < 0 and lib.pf_cnf_rhs_vjp_workspace_bytes(40, 0) < 0
    # one 4900-float slab per workgroup, one workgroup per 64-row tile (4 waves x floor(16 / R) R rows), at most 256
    assert lib.pf_cnf_rhs_vjp_workspace_bytes(40, 4) == 4900 * 4
    assert lib.pf_cnf_rhs_vjp_workspace_bytes(201, 3) == 4 * 4900 * 4   # 60 rows per workgroup
    assert lib.pf_cnf_rhs_vjp_workspace_bytes(32768, 1) == 256 * 4900 * 4


def test_unpack_cnf_grads_is_keyed_and_shaped_like_the_state_dict():
    from puflow_amd.packing import CNF_CTX, CNF_GRAD, cnf_hyper_matrix, unpack_cnf_grads
    from puflow_amd.weights import synth_cnf_state_dict
    sd = synth_cnf_state_dict(7)
    i = 5
    p = f"flow_blocks.{i}.cnf.odefunc.diffeq.layers"
    cd = sd[f"{p}.0._hyper_gate.weight"].shape[1] - 1
    grad = torch.arange(CNF_GRAD, dtype=torch.float32)
    dH = torch.arange(CNF_CTX * cd, dtype=torch.float32).reshape(CNF_CTX, cd) + 10000
    dhb = torch.arange(CNF_CTX, dtype=torch.float32) + 50000
    out = unpack_cnf_grads(i, grad, dH, dhb)
    assert sorted(out) == sorted(k for k in sd if k.startswith(p + "."))
    for k, v in out.items():
        assert v.shape == sd[k].shape, k
    assert out[f"{p}.1._layer.weight"][2, 5] == 2 * 64 + 5 and out[f"{p}.0._layer.weight"][7, 2] == 4096 + 7 * 3 + 2
    assert out[f"{p}.2._layer.weight"][1, 9] == 4416 + 64 + 9 and out[f"{p}.2._layer.bias"][2] == 4610
    assert out[f"{p}.1._hyper_gate.weight"][3, 0] == 4612 + 128 + 3                     # the t-column is column 0
    assert out[f"{p}.1._hyper_gate.weight"][3, 2] == 10000 + (128 + 3) * cd + 1
    assert out[f"{p}.2._hyper_bias.weight"][1, 0] == 4612 + 272 + 1 and out[f"{p}.2._hyper_gate.bias"][2] == 50000 + 258
    # the un-folded hyper matrix against the state dict (layer 3 in each of its four slots)
    H = cnf_hyper_matrix(sd, i)
    assert H.shape == (CNF_CTX, cd + 1)
    assert np.array_equal(H[192:256], sd[f"{p}.1._hyper_bias.weight"].numpy())
    for qq in range(4):
        assert np.array_equal(H[256 + 4 * qq:259 + 4 * qq], sd[f"{p}.2._hyper_gate.weight"].numpy())
        assert np.all(H[259 + 4 * qq] == 0)
