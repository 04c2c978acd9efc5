"""pf_cnf_pack_blocks (csrc/cnf_pack.hip) against the numpy packers it replaces in the training step, bit for bit: the weight
record, the folded and the plain hyper matrices, the context GEMM's bias and fragment image, the meta row - for all six blocks of
synth_cnf_state_dict(7) in one launch, with the special values the host packers treat specially (an all-zero hyper matrix,
a magnitude outside fp16's range); and `flow_block(pack="device")` against `pack="host"`, outputs and gradients, bit for bit."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from puflow_amd.packing import cnf_hyper_matrix, pack_cnf_block, pack_cnf_context
from puflow_amd.weights import synth_cnf_state_dict

DEV = "cuda:0"
NB = 6


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(got, ref_np, what):
    ref = torch.from_numpy(np.ascontiguousarray(ref_np, dtype=np.float32))
    got = got.detach().cpu().reshape(ref.shape)
    assert torch.equal(got, ref), (what, "values")
    assert torch.equal(_bits(got), _bits(ref)), (what, "bits (signed zeros, fp16 pairs read as floats)")


def _blocks(sd):
    from puflow_amd.cnf import _pack_keys
    return [[sd[k].to(DEV) for k in _pack_keys(i)] for i in range(NB)]


@functools.lru_cache(maxsize=None)
def _sd():
    """synth_cnf_state_dict(7) with block 2's hyper networks blind to the context (c-columns all zero -> image scale 1) and a
    subnormal and a large-but-legal weight in block 4."""
    sd = {k: v.clone() for k, v in synth_cnf_state_dict(7).items()}
    p = "flow_blocks.2.cnf.odefunc.diffeq.layers"
    for l in range(3):
        for n in ("_hyper_gate.weight", "_hyper_bias.weight"):
            sd[f"{p}.{l}.{n}"][:, 1:] = 0.0
    p4 = "flow_blocks.4.cnf.odefunc.diffeq.layers"
    sd[f"{p4}.1._layer.weight"][3, 5] = 1e-41
    sd[f"{p4}.1._layer.weight"][7, 9] = 2.0e4            # x 2 log2e = 57 708 < 65 504
    sd[f"{p4}.0._hyper_bias.weight"][11, 4] = -3.0e-40
    return sd


def test_all_blocks_in_one_launch_match_the_numpy_packers():
    from puflow_amd.cnf import _DevicePack
    sd = _sd()
    pk = _DevicePack(_blocks(sd), torch.device(DEV))
    assert pk.rec.shape == (NB, 10160) and pk.hb.shape == (NB, 288) and pk.meta.shape == (NB, 4)
    for i in range(NB):
        rec, Hc, hb, T_end = pack_cnf_block(sd, i)
        img, inv = pack_cnf_context(Hc)
        _same_bits(pk.rec[i], rec, (i, "rec"))
        _same_bits(pk.Hc[i], Hc, (i, "Hc"))
        _same_bits(pk.hb[i], hb, (i, "hb"))
        _same_bits(pk.Hplain[i], cnf_hyper_matrix(sd, i)[:, 1:], (i, "Hplain"))
        _same_bits(pk.image[i], img, (i, "image"))
        meta = pk.meta[i].cpu()
        assert torch.equal(meta[:2].float(), torch.tensor([T_end, float(inv)], dtype=torch.float32)), (i, meta)
        assert pk.T_end[i] == T_end and pk.inv_scale[i] == float(inv)          # the doubles the host path hands to the kernels
        assert float(meta[2]) == 0.0 and float(meta[3]) == 0.0
    assert pk.inv_scale[2] == 1.0 and float(pk.Hc[2].abs().max()) == 0.0      # the all-zero matrix: scale 1


def test_fewer_blocks_and_any_order():
    """nb = 1 and nb = 3 with the blocks in another order (widths 128, 32, 64): entry j is the j-th block given."""
    from puflow_amd.cnf import _DevicePack
    sd = _sd()
    blocks = _blocks(sd)
    for order in ((1,), (5, 0, 1)):
        pk = _DevicePack([blocks[i] for i in order], torch.device(DEV))
        for j, i in enumerate(order):
            rec, Hc, hb, _ = pack_cnf_block(sd, i)
            _same_bits(pk.rec[j], rec, (order, j, "rec"))
            _same_bits(pk.image[j], pack_cnf_context(Hc)[0], (order, j, "image"))
            _same_bits(pk.hb[j], hb, (order, j, "hb"))


@pytest.mark.parametrize("key,where", [("1._layer.weight", "f16x2"), ("2._layer.weight", "f16x2"), ("0._hyper_gate.weight", None)])
def test_out_of_range_weight_sets_status_and_raises_like_the_host(key, where):
    """A weight of 7e4 in block 3: the numpy packer raises ValueError for the record's f16x2 images; the device sets the block's
    status word and the host raises the same error.  In a hyper matrix the power-of-two scale absorbs it: both pack."""
    from puflow_amd.cnf import _DevicePack
    sd = {k: v.clone() for k, v in _sd().items()}
    sd[f"flow_blocks.3.cnf.odefunc.diffeq.layers.{key}"][1, 2] = 7e4
    if where is None:
        rec, Hc, hb, _ = pack_cnf_block(sd, 3)
        pk = _DevicePack(_blocks(sd), torch.device(DEV))
        _same_bits(pk.image[3], pack_cnf_context(Hc)[0], "image")
        _same_bits(pk.rec[3], rec, "rec")
        return
    with pytest.raises(ValueError, match=where):
        pack_cnf_block(sd, 3)
    with pytest.raises(ValueError, match=where):
        _DevicePack(_blocks(sd), torch.device(DEV))
    # the status word itself: bit 0 for block 3 alone
    from puflow_amd import _lib
    import ctypes
    blocks = _blocks(sd)
    cds = [int(b[2].shape[1]) - 1 for b in blocks]
    f32 = dict(dtype=torch.float32, device=DEV)
    rec, hb = torch.empty((NB, 10160), **f32), torch.empty((NB, 288), **f32)
    outs = [[torch.empty(288 * cd, **f32) for cd in cds] for _ in range(3)]
    meta = torch.empty((NB, 4), dtype=torch.float64, device=DEV)
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    _lib.check(_lib.load().pf_cnf_pack_blocks(ptrs([t for b in blocks for t in b]), _lib.counts(cds), NB, rec.data_ptr(), hb.data_ptr(),
                                              ptrs(outs[0]), ptrs(outs[1]), ptrs(outs[2]), meta.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "pf_cnf_pack_blocks")
    assert meta[:, 2].cpu().tolist() == [0.0, 0.0, 0.0, 1.0, 0.0, 0.0]


CASES = {"b0_fwd_R1": (0, 200, 1, False, True), "b5_rev_R4": (5, 100, 4, True, False)}      # DESIGN 9a's cases


@pytest.mark.parametrize("name", list(CASES))
def test_flow_block_device_pack_gives_the_bits_of_the_host_pack(name):
    from puflow_amd.cnf import PointInterpFlow
    block, T, R, reverse, use_logp = CASES[name]
    sd = synth_cnf_state_dict(7)
    g = torch.Generator().manual_seed(40 + block)                         # tests/test_gpu_cnf_grad.py's inputs
    cd = sd[f"flow_blocks.{block}.cnf.odefunc.diffeq.layers.0._hyper_gate.weight"].shape[1] - 1
    c = torch.randn(T, cd, generator=g) * 0.7
    e = torch.randn(T, 3, generator=g)
    x = torch.randn(T * R, 3, generator=g) * 0.8
    gx = torch.randn(T * R, 3, generator=g).to(DEV)
    gl = (torch.randn(T * R, generator=g) if use_logp else torch.zeros(T * R)).to(DEV)
    res = {}
    for pack in ("device", "host"):
        net = PointInterpFlow(3)
        net.load_state_dict(sd, strict=True)
        net = net.to(DEV).train()
        xd, cdv = x.to(DEV).requires_grad_(True), c.to(DEV).requires_grad_(True)
        ox, ol = net.flow_block(block, xd, cdv, e.to(DEV), R, reverse, pack=pack)
        ((ox * gx).sum() + (ol * gl).sum()).backward()
        res[pack] = dict(out_x=ox.detach(), out_l=ol.detach(), x=xd.grad, c=cdv.grad, steps=list(net.last_block_steps),
                         **{n: p.grad for n, p in net.flow_blocks[block].named_parameters()})
    assert res["device"]["steps"] == res["host"]["steps"] and len(res["host"]["steps"]) >= 2
    assert len(res["host"]) == 5 + 16
    for k, v in res["host"].items():
        if k != "steps":
            assert v is not None and torch.equal(res["device"][k], v), k
