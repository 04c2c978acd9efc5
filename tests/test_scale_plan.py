"""The scale plan of interp_kernel's chains (puflow_amd/packing.py, "scale plan of interp_kernel's chains"):
  * the stored matrices are the folded plan's matrices times exact powers of two, and their fragment images hold them;
  * every activation the CPU oracle produces at synth_patches(2, 256), times the 2^a it is stored with, stays a factor
    HEADROOM under fp16's 65504 - for the synthetic weights and for the pretrained PU1K checkpoint.
CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
from puflow_amd import packing as P
from puflow_amd.weights import synth_patches, synth_state_dict

FP16_MAX = 65504.0
HEADROOM = 16.0           # documented next to packing.ec4_scales: the wanted exponents leave at least this factor at these inputs


@pytest.fixture(scope="module", params=["synth", "pretrained"])
def case(request, golden_dir):
    if request.param == "synth":
        sd = synth_state_dict(2021)
    else:
        g = np.load(golden_dir + "/pretrained_pu1k.npz")
        sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}
    plan = P.fold_state_dict(sd)
    xyz = synth_patches(2, 256, seed=2021)
    with torch.no_grad():
        st = O.forward(sd, xyz, 4, stages=True)
    return sd, plan, P.pack_plan(plan), xyz, st


def _undo(W, rows, cols=0):
    e = np.asarray(cols, np.int64).reshape(1, -1) - np.asarray(rows, np.int64).reshape(-1, 1)
    return np.ldexp(W, np.broadcast_to(e, W.shape).astype(np.int32))


def _image_holds(img, W, tag):
    """hi + lo of the f16n image against the fp32 matrix it was made from: 2^-21 relative, 2^-25 absolute floor (stored units)."""
    got = P.frag_unpack_f16n(img, *W.shape)
    assert np.all(np.abs(got - W) <= np.abs(W) * 2.0 ** -21 + 2.0 ** -25), tag


def test_interp_matrices_are_the_parents_times_powers_of_two(case):
    _, plan, pk, _, _ = case
    ip = plan["interp"]
    x, m = P.interp_scaled(ip)
    assert x == pk["exps"]["interp"]
    g = x["g"]
    assert g[0] >= 0 and all(b >= a for a, b in zip(g, g[1:])) and max(g) <= 7
    assert 0 <= x["d1"] <= x["d2"] <= x["w1"] and max(g) <= x["w1"] <= x["w2"] <= x["w3"]
    gr = np.repeat(g, 16)
    ec, ft = ip["ec"], ip["f_tab"]
    # the edge tables multiply (x_i, 2^ETAB_VSHIFT (x_i - x_j), |x_i - x_j|, 1): PA x_i + QB x_j = (PA + QB) x_i - QB (x_i - x_j)
    rel = lambda PA, QB: ((PA.astype(np.float64) + QB).astype(np.float32), np.ldexp(-QB.astype(np.float64), -P.ETAB_VSHIFT).astype(np.float32))
    assert P.ETAB_VSHIFT == 4                                     # csrc/interp.hip multiplies the difference by 16
    np.testing.assert_array_equal(_undo(m["dtab"], x["d1"]), P._etab_dense(*rel(ip["d_PA"], ip["d_QB"]), ip["d_wn"], ip["d_b0"]))
    np.testing.assert_array_equal(_undo(m["ectab"], gr), P._etab_dense(*rel(ec["PA"][:128], ec["QB"][:128]), None, ec["pb"][:128]))
    np.testing.assert_array_equal(_undo(m["w1tab"], x["w1"]), P._etab_dense(*rel(ft[:, 0:3], ft[:, 3:6]), None, ft[:, 6] + ip["f_b0"]))
    for t in range(1, 8):
        np.testing.assert_array_equal(_undo(m[f"G{t}"], g[t], gr[:16 * t]), ec[f"G{t}"])
    np.testing.assert_array_equal(_undo(m["d_W3"], x["d2"], x["d1"]), ip["d_W3"])
    np.testing.assert_array_equal(_undo(m["f_dW"], x["w1"], x["d2"]), ip["f_dW"])
    np.testing.assert_array_equal(_undo(m["f_eW"], x["w1"], gr), ip["f_eW"])
    np.testing.assert_array_equal(_undo(m["w_W3"], x["w2"], x["w1"]), ip["w_W3"])
    np.testing.assert_array_equal(_undo(m["w_W6full"], x["w3"], x["w2"]), ip["w_W6"])
    np.testing.assert_array_equal(_undo(m["w_W6"], x["w3"], x["w2"])[4:8], ip["w_W6"][:4])
    for k, b, a in (("d_b3", ip["d_b3"], x["d2"]), ("w_b3", ip["w_b3"], x["w2"]), ("w_b6full", ip["w_b6"], x["w3"])):
        np.testing.assert_array_equal(np.ldexp(m[k], -a), b)
    # the blob: images of exactly these matrices, biases verbatim, and the `scales` slot = what the kernel still applies
    blob, off = pk["blob"], dict(zip(P.INTERP_SLOTS, pk["interp"]))
    _image_holds(blob[off["d_W3"]:off["d_W3"] + 8 * 512], m["d_W3"], "d_W3")
    _image_holds(blob[off["d_W6"]:off["d_W6"] + 16 * 512], m["f_dW"], "f_dW")
    _image_holds(blob[off["w_W0"]:off["w_W0"] + 32 * 512], m["f_eW"], "f_eW")
    _image_holds(blob[off["w_W3"]:off["w_W3"] + 16 * 512], m["w_W3"], "w_W3")
    _image_holds(blob[off["w_W6full"]:off["w_W6full"] + 4 * 512], m["w_W6full"], "w_W6")
    f0 = 0
    for t in range(1, 8):
        n = (t + 1) // 2
        _image_holds(blob[off["ec_w"] + f0 * 512:off["ec_w"] + (f0 + n) * 512], m[f"G{t}"], f"G{t}")
        f0 += n
    for tab, slot, rows in (("dtab", "dtab", 64), ("ectab", "ectab", 128), ("w1tab", "w_b0", 128)):
        h0, h1, lo, z = P.etab_unpack_frag1(blob[off[slot]:off[slot] + (rows // 16) * 256], rows)
        T = m[tab][:, P._ETAB_COLS].astype(np.float64)
        assert np.array_equal(h0, h1) and not z.any()
        assert np.all(np.abs(h0 + lo - T) <= np.abs(T) * 2.0 ** -21 + 2.0 ** -25), tab
    np.testing.assert_array_equal(blob[off["d_b3"]:off["d_b3"] + 64], m["d_b3"])
    np.testing.assert_array_equal(blob[off["w_b3"]:off["w_b3"] + 64], m["w_b3"])
    np.testing.assert_array_equal(blob[off["scales"]:off["scales"] + 6], np.array([1, 1, 1, 1, 1, 2.0 ** -x["w3"]], np.float32))
    # the logits' matrix sits where f16n_scale puts every matrix whose rescale stays
    assert 2.0 ** 13 <= np.abs(m["w_W6full"]).max() < 2.0 ** 14


def _below(name, act, a):
    peak = float(act.abs().max()) * 2.0 ** a
    print(f"{name}: max |x| {float(act.abs().max()):.3f}  stored x 2^{a} = {peak:.1f}  (limit {FP16_MAX / HEADROOM:.0f})")
    assert peak * HEADROOM < FP16_MAX, name


def test_interp_activations_keep_their_headroom(case):
    sd, _, pk, xyz, st = case
    x = pk["exps"]["interp"]
    idx8 = st["idx8"]
    with torch.no_grad():
        nb = O.knn_gather(xyz, idx8)
        xi = xyz.unsqueeze(2).expand_as(nb)
        vec = xi - nb
        fd = torch.cat([xi, nb, vec, torch.sqrt(torch.sum(vec ** 2, dim=-1, keepdim=True))], dim=-1).permute(0, 3, 1, 2)
        p = "interp.knn_context.distance_encoder.mlp"
        d1 = O._conv_bn_lrelu01(sd, p, 0, fd)
        d2 = O._conv_bn_lrelu01(sd, p, 3, d1)
        _below("d1", d1, x["d1"]); _below("d2", d2, x["d2"])
        d = F.conv2d(d2, sd[p + ".6.weight"], sd[p + ".6.bias"])
        f = torch.cat([xi, nb, nb - xi], dim=-1).permute(0, 3, 1, 2)             # the EdgeConv's growth chain (ref_cpu.edgeconv_unit)
        for t in range(8):
            g = O._conv_bn_lrelu(sd, f"interp.knn_context.feat_conv.convs.{t}", f, 0.05)
            _below(f"growth {t}", g, x["g"][t])
            f = torch.cat([f, g], dim=1)
        feat = F.conv2d(f, sd["interp.knn_context.feat_conv.conv_out.weight"], sd["interp.knn_context.feat_conv.conv_out.bias"])
        p = "interp.weight_unit.mlp"
        w1 = O._conv_bn_lrelu01(sd, p, 0, torch.cat([d, feat], dim=1))
        w2 = O._conv_bn_lrelu01(sd, p, 3, w1)
        _below("w1", w1, x["w1"]); _below("w2", w2, x["w2"])
        # the chain above is the oracle's: its softmax weights are the stage the forward returned
        w = F.conv2d(w2, sd[p + ".6.weight"], sd[p + ".6.bias"]).permute(0, 2, 1, 3)
        assert torch.allclose(F.softmax(w[:, :, :4], dim=-1), st["w"], atol=1e-6)
