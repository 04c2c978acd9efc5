"""tests/extract_train_ref.py (the float64 restatement that tests/test_gpu_extract_train.py holds the training kernels of the
feature extractor and the interpolation-weight branch to) against the pinned oracle, the evidence that its bar notices a
subtly wrong kernel - every deliberate error, applied to the restatement itself, breaks the bar on at least one quantity of
every case it applies to - and every condition the case tables of the GPU test state (small cases: no decision within
MIN_PREACT; large cases: the masked shares and the size of the flip widening).  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import extract_train_ref as R
from oracle import ref_cpu as O

_REFS = {}


def _refs(key, make, need_clear=True):
    """(problem, r64, r32, rec) of a case: computed once, shared by the tests of this file, never written."""
    if key not in _REFS:
        prob = make()
        _REFS[key] = (prob,) + R.references(prob, need_clear)
    return _REFS[key]


def _ulp_close(a, b, r64, what, layers):
    """Two float32 evaluations of the same expressions in another operation order (conv2d on [B, C, N, K] and F.batch_norm there,
    F.linear on rows and the written-out BatchNorm here): NOT equal to the last bit, but within a few ulp - four float32 ulps
    (4 x 2^-23) of the tensor's largest value for every conv / BatchNorm layer the value has passed: a layer is an inner product
    of at most 512 terms summed in another order (a few ulp of its result) followed by a normalisation to unit variance, which
    carries the relative error on and adds its own."""
    err = float((a.double() - b.double()).abs().max())
    bound = 4.0 * layers * 2.0 ** -23 * float(r64.abs().max())
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e} ({err / (2.0 ** -23 * float(r64.abs().max())):.1f} ulp of the maximum)"


# ------------------------------------------------------------------------------------------------ the pinned oracle
def _oracle_sd(P, state, pfx, dtype):
    sd = {pfx + k: v.to(dtype) for k, v in P.items()}
    sd.update({pfx + k: (v.to(dtype) if v.is_floating_point() else v) for k, v in state.items()})
    return sd


@pytest.mark.parametrize("unit,pooling,K", [("u3", True, 16), ("u64", True, 16), ("u128", False, 16), ("k8", False, 8)])
def test_unit_equals_the_oracle(unit, pooling, K):
    """edgeconv_unit against oracle.ref_cpu.edgeconv_unit_train (+ _bn_train's running updates): to 1e-12 of the largest value
    in float64 - the same function - and to float32 rounding in float32 (another operation order: see _ulp_close)."""
    case = dict(unit=unit, K=K, pooling=pooling, B=2, N=19)
    prob = R.unit_problem(case, seed=1)
    x, idx = prob["inputs"]["x"], prob["idx"]
    P = {k: v for k, v in prob["inputs"].items() if k != "x"}
    outs = {}
    for dtype in (torch.float64, torch.float32):
        ts = O.TrainState()
        sd = _oracle_sd(P, prob["state"], "u.", dtype)
        y = O.edgeconv_unit_train(sd, "u", x.to(dtype), idx, ts, pooling=pooling)
        mine = prob["ref"]({k: v.to(dtype) for k, v in prob["inputs"].items()})
        if not pooling:
            y = y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])
        outs[dtype] = (y, mine, ts)
    y64, m64, ts64 = outs[torch.float64]
    assert float((y64 - m64["out"]).abs().max()) <= 1e-12 * float(y64.abs().max())
    for k, v in ts64.bn_updates.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 101
        else:
            assert float((v - m64[k[2:]]).abs().max()) <= 1e-12 * float(v.abs().max()), k
    y32, m32, ts32 = outs[torch.float32]
    layers = R.n_convs(P, "") + 1
    _ulp_close(m32["out"], y32, m64["out"], "out", layers)
    for k, v in ts32.bn_updates.items():
        if not k.endswith("num_batches_tracked"):
            _ulp_close(m32[k[2:]], v, m64[k[2:]], k, layers)


def test_merge_equals_the_oracle_to_the_last_bit():
    """merge against oracle.ref_cpu.feat_merge: the same two F.linear calls on the same rows - bit-identical in float32."""
    prob = R.merge_problem(dict(ccs=[(64, 64)], T=37), seed=1)
    lv = {k: v.float() for k, v in prob["inputs"].items()}
    sd = {"merge_convs.0." + k[3:]: v for k, v in lv.items() if k.startswith("m0.")}
    assert torch.equal(prob["ref"](lv)["c0"], O.feat_merge(sd, 0, lv["h0"]))
    # ReLU through the recorded sign equals F.relu wherever the input is not exactly zero
    z = F.linear(lv["h0"], lv["m0.conv1.weight"], lv["m0.conv1.bias"])
    assert torch.equal(R.Decisions().act(z, 0.0), F.relu(z))


def test_features_and_interp_logits_equal_the_oracle_forward_train():
    """The composed restatements on the model's synthetic state dict against oracle.ref_cpu.forward_train itself: the BatchNorm
    running updates of all six feature units and of the interpolation branch (its two MLPs and the K = 8 unit) that the
    oracle's train step records are functions of exactly the tensors `features` / `interp_logits` compute - 1e-12 in float64,
    float32 rounding in float32 (another operation order: see _ulp_close).  The interpolation logits, which forward_train does
    not return, are compared with the oracle's own layers (_bn_train, edgeconv_unit_train) composed as its lines do."""
    from puflow_amd.weights import synth_patches, synth_state_dict
    sd0 = synth_state_dict(7)
    xyz = synth_patches(2, 40, seed=5)
    res = {}
    for dtype in (torch.float64, torch.float32):
        sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd0.items()}
        x = xyz.to(dtype)
        if dtype == torch.float64:
            _, idx16 = O.knn_canonical(xyz, xyz, 16)
            idx8 = idx16[..., :8].contiguous()
            assert torch.equal(idx16, R.knn(xyz.double(), 16))
        cs, fs = R.features(sd, x, idx16, state=sd)
        w, ws = R.interp_logits(sd, x, idx8, state=sd)
        wf, wfs = R.interp_logits(sd, x, idx8, state=sd, folded=True)
        # the oracle: forward_train for the updates (it works in float32; the float64 run calls its layers)
        ts = O.TrainState()
        h, ocs = x, []
        for i in range(6):
            h = O.edgeconv_unit_train(sd, f"feat_convs.{i}", h, idx16, ts)
            ocs.append(O.feat_merge(sd, i, h))
        nb = O.knn_gather(x, idx8)
        xi = x.unsqueeze(2).expand_as(nb)
        vec = xi - nb
        d = torch.cat([xi, nb, vec, torch.sqrt(torch.sum(vec ** 2, dim=-1, keepdim=True))], dim=-1).permute(0, 3, 1, 2)
        for a in (0, 3):
            d = F.conv2d(d, sd[f"{R.P_DE}{a}.weight"], sd[f"{R.P_DE}{a}.bias"])
            d = F.leaky_relu(O._bn_train(sd, f"{R.P_DE}{a + 1}", d, ts), 0.01)
        d = F.conv2d(d, sd[R.P_DE + "6.weight"], sd[R.P_DE + "6.bias"])
        feat = O.edgeconv_unit_train(sd, R.P_FC[:-1], x, idx8, ts, pooling=False)
        ow = torch.cat([d, feat], dim=1)
        for a in (0, 3):
            ow = F.conv2d(ow, sd[f"{R.P_WU}{a}.weight"], sd[f"{R.P_WU}{a}.bias"])
            ow = F.leaky_relu(O._bn_train(sd, f"{R.P_WU}{a + 1}", ow, ts), 0.01)
        ow = F.conv2d(ow, sd[R.P_WU + "6.weight"], sd[R.P_WU + "6.bias"]).permute(0, 2, 3, 1).reshape(-1, 32)
        res[dtype] = (cs, {**fs, **ws}, w, wf, wfs, ocs, ow, ts)
    cs64, st64, w64, wf64, wfs64, ocs64, ow64, ts64 = res[torch.float64]
    for c, oc in zip(cs64, ocs64):
        assert float((c - oc).abs().max()) <= 1e-12 * float(oc.abs().max())
    assert float((w64 - ow64).abs().max()) <= 1e-12 * float(ow64.abs().max())
    assert float((wf64 - w64).abs().max()) <= 1e-12 * float(w64.abs().max())
    assert len(ts64.bn_updates) == 3 * (4 * 1 + 4 * 5 + 8 + 4)
    for k, v in ts64.bn_updates.items():
        if not k.endswith("num_batches_tracked"):
            assert float((v - st64[k]).abs().max()) <= 1e-12 * float(v.abs().max()), k
            if k in wfs64:
                assert float((v - wfs64[k]).abs().max()) <= 1e-12 * float(v.abs().max()), k
    cs32, st32, w32, _, _, ocs32, ow32, ts32 = res[torch.float32]
    for i, (c, oc) in enumerate(zip(cs32, ocs32)):
        _ulp_close(c, oc, cs64[i], f"c{i}", 5 * (i + 1) + 2)          # i + 1 units of 4 + 1 convs, the merge unit's two
    _ulp_close(w32, ow32, w64, "w", 9 + 3)                            # the 8 + 1 convs of the K = 8 unit, the weight unit's three
    # forward_train itself (float32): the updates it records are the ones the layer-by-layer composition above recorded
    _, _, tsf = O.forward_train(sd0, xyz, 4)
    assert set(tsf.bn_updates) >= set(ts32.bn_updates)
    for k, v in ts32.bn_updates.items():
        assert torch.equal(tsf.bn_updates[k], v), k
        if not k.endswith("num_batches_tracked"):
            _ulp_close(st32[k], v, st64[k], k, 30 if k.startswith("feat_convs.") else 12)


def test_folded_and_plain_interp_logits_agree_in_float64():
    """The FoldWuFn algebra written out (interp_logits(folded=True)) against the plain form: logits, every parameter gradient
    and the running statistics to 1e-12 of the tensor's largest value."""
    prob = R.composed_problem(dict(part="interp", B=2, N=21), seed=3)
    rec = R.Decisions()
    plain = R.run(prob, lambda lv: prob["ref"](lv, rec))
    fold = R.run(prob, lambda lv: prob["ref"](lv, R.Decisions(replay=rec), folded=True))
    assert set(plain) == set(fold)
    gmax = max(float(v.abs().max()) for k, v in plain.items() if k.startswith("d"))
    for k, v in plain.items():
        if R.is_residue(k, "composed"):                    # true value zero: both forms leave ~1e-17
            assert float(fold[k].abs().max()) <= 1e-12 * gmax and float(v.abs().max()) <= 1e-12 * gmax, k
            continue
        assert float((fold[k] - v).abs().max()) <= 1e-12 * float(v.abs().max()), k


def test_replayed_decisions_are_the_float64_ones():
    """A float32 run that replays takes the float64 side of every kink and the float64 argmax of every pool and stays within
    rounding of float64; a flipped replay takes the other side in the DERIVATIVE only: same outputs, other gradients."""
    prob = R.unit_problem(dict(unit="u32", K=16, pooling=True, B=1, N=17), seed=1)
    r64, r32, rec = R.references(prob)
    assert rec.k == 5 and [it[0] for it in rec.items] == ["act"] * 4 + ["pool"]
    assert float((r32["out"].double() - r64["out"]).abs().max()) <= 1e-5 * float(r64["out"].abs().max())
    for it in rec.items:                                          # force every decision to "near": flip then takes them all the other way
        it[-1].fill_(True)
    flipped = R.run(prob, lambda lv: prob["ref"](lv, R.Decisions(replay=rec, flip=True)))
    assert float((flipped["out"] - r64["out"]).abs().max()) <= 1e-12 * float(r64["out"].abs().max())
    assert float((flipped["dx"] - r64["dx"]).abs().max()) > 1e-2 * float(r64["dx"].abs().max())


# ------------------------------------------------------------------------------------------------ deliberate errors
UNIT_BASES = {}
for _c in R.unit_cases():
    UNIT_BASES.setdefault((_c["base"], _c["tap"]), _c)
UNIT_BASES = list(UNIT_BASES.values())
BNMLP, MERGE, COMPOSED = R.bnmlp_cases(), R.merge_cases(), R.composed_cases()


def _bugs_break(prob, r64, r32, what, fmt=None):
    """Every deliberate error that applies breaks the bar.  fmt: the format widening of a problem that also runs through the
    fused unit - the errors must break the WIDENED bar as well, but for the dropped eps: 1e-5 beside a variance of O(1) moves
    the gradients by 5e-6 of themselves, the size of the split-bf16 format's own error (the per-op tier and the BatchNorm
    MLPs, held to the unwidened bar, are where a dropped eps shows)."""
    assert not R.failures(R.hold(r64, r64, r32, prob["kind"])[0])
    # float32 against float64 stays at rounding level: the bar is far tighter than the suite's tier-against-tier bars
    for k, v in r64.items():
        if not R.is_residue(k, prob["kind"]):
            assert R.bar_of(v, r32[k]) <= 2e-4 * float(v.abs().max()) + 1e-30, (k, R.bar_of(v, r32[k]), float(v.abs().max()))
    n = 0
    for bug in R.BUGS:
        if not R.bug_applies(bug, prob):
            continue
        wrong = R.run(prob, lambda lv: prob["ref"](lv, R.Decisions(bug=(bug,)), (bug,)))
        assert R.failures(R.hold(wrong, r64, r32, prob["kind"])[0]), f"{bug} stays inside the bar on every quantity of {what}"
        if fmt and bug != "no_eps":
            assert R.failures(R.hold(wrong, r64, r32, prob["kind"], fmt=fmt)[0]), f"{bug} stays inside the widened bar of {what}"
        n += 1
    return n


@pytest.mark.parametrize("case", UNIT_BASES, ids=[c["base"] + ("-tap" if c["tap"] else "") for c in UNIT_BASES])
def test_the_bar_catches_every_deliberate_error_in_a_unit(case):
    prob, r64, r32, rec = _refs(("unit", case["base"], case["tap"]), lambda: R.unit_problem(case))
    assert rec.clear()                                              # the seed keeps every decision MIN_PREACT clear
    fmt = R.format_widening(prob, r64, rec)
    for k, w in fmt.items():                                        # one draw of the format stays under the 2e-4 cap with the bar
        assert R.is_residue(k, "unit") or R.bar_of(r64[k], r32[k]) + w / R.FORMAT_DRAWS <= R.GRAD_CAP * float(r64[k].abs().max()), (k, w)
    assert max(fmt.values()) > 0 and fmt["dconv_out.bias"] <= 1e-12 * float(r64["dconv_out.bias"].abs().max())   # a plain sum: no product
    assert _bugs_break(prob, r64, r32, case["id"], fmt) == (9 if case["pooling"] else 8)


@pytest.mark.parametrize("case", BNMLP, ids=[c["id"] for c in BNMLP])
def test_the_bar_catches_every_deliberate_error_in_a_batchnorm_mlp(case):
    prob, r64, r32, rec = _refs(case["id"], lambda: R.bnmlp_problem(case))
    assert rec.clear()
    assert _bugs_break(prob, r64, r32, case["id"]) == 5


@pytest.mark.parametrize("case", MERGE, ids=[c["id"] for c in MERGE])
def test_the_bar_catches_a_leaky_merge_unit(case):
    prob, r64, r32, rec = _refs(case["id"], lambda: R.merge_problem(case))
    assert rec.clear()
    assert _bugs_break(prob, r64, r32, case["id"]) == 1


def test_the_bar_catches_the_fold_and_distance_errors():
    for o, k6, ko in ((128, 64, 137), (16, 5, 7)):
        prob = R.fold_problem(o, k6, ko)
        r64, r32, _ = R.references(prob)
        assert _bugs_break(prob, r64, r32, prob["case"]["id"]) == 1
    for B, N in ((1, 16), (1, 17), (1, 257)):
        prob = R.dist_problem(B, N)
        r64, r32, _ = R.references(prob)
        assert _bugs_break(prob, r64, r32, prob["case"]["id"]) == 1


@pytest.mark.parametrize("case", COMPOSED, ids=[c["id"] for c in COMPOSED])
def test_the_bar_catches_every_deliberate_error_in_the_composed_parts(case):
    prob, r64, r32, rec = _refs(case["id"], lambda: R.composed_problem(case))
    assert rec.clear()
    assert _bugs_break(prob, r64, r32, case["id"], R.format_widening(prob, r64, rec)) == (10 if case["part"] == "features" else 9)


def test_every_deliberate_error_applies_somewhere():
    probs = [dict(kind="unit", case=c) for c in UNIT_BASES] + [dict(kind="bnmlp", case=c) for c in BNMLP] + \
            [dict(kind="merge", case=c) for c in MERGE] + [dict(kind="composed", case=c) for c in COMPOSED] + \
            [dict(kind="fold", case={}), dict(kind="dist", case={})]
    for bug in R.BUGS:
        assert sum(R.bug_applies(bug, p) for p in probs) >= 1, bug


# ------------------------------------------------------------------------------------------------ the case tables
def test_per_op_node_cases_meet_their_input_conditions():
    """The inputs of the per-op node cases of the GPU test: small BatchNorm nodes keep every LeakyReLU input MIN_PREACT clear,
    large ones mask at most 1e-4 of their elements; no activation input and no pool gap lies within MIN_PREACT; every family
    has a size past its kernels' sweep - for the max-pool one past the backward's (T K C) and one past the forward's (T C)."""
    for rows, C in R.BN_NODE_SIZES:
        prob = R.bn_node_problem(rows, C)
        assert prob["near_share"] <= R.MAX_KINK_SHARE if prob["large"] else prob["clear"], (rows, C)
    assert any(r * c > R.SWEEP for r, c in R.BN_NODE_SIZES) and any(r > 1024 * 1024 for r, c in R.BN_NODE_SIZES)
    for n in R.ACT_NODE_SIZES:
        assert R.act_node_problem(0.05, n)["clear"], n
    assert max(R.ACT_NODE_SIZES) > R.SWEEP
    for T, C, K in R.MAXPOOL_NODE_SIZES:
        assert R.maxpool_node_problem(T, C, K)["clear"], (T, C, K)
    assert any(T * K * C > R.SWEEP for T, C, K in R.MAXPOOL_NODE_SIZES) and any(T * C > R.SWEEP for T, C, K in R.MAXPOOL_NODE_SIZES)


def test_case_tables_hold_what_the_gpu_test_needs():
    """Every unit shape at every small size, every variant on a narrow and a wide unit at (1, 33) and (3, 17), the K = 8 unit at
    an edge count that is no multiple of 16, every BatchNorm-MLP form at every row count."""
    cs = R.unit_cases()
    for u in ("u3", "u32", "u64", "u128"):
        assert {(c["B"], c["N"]) for c in cs if c["unit"] == u and c["pooling"] and c["variant"] == "csr"} == set(R.SMALL_BN)
        assert len([c for c in cs if c["unit"] == u and not c["pooling"]]) == 2
    assert {(c["B"], c["N"]) for c in cs if c["unit"] == "k8"} == set(R.K8_BN)
    assert any(c["unit"] == "k8" and (c["B"] * c["N"] * 8) % 16 for c in cs)
    for u in ("u3", "u128"):
        for bn in ((1, 33), (3, 17)):
            assert {c["variant"] for c in cs if c["unit"] == u and (c["B"], c["N"]) == bn and c["pooling"]} == set(R.VARIANTS)
    assert {(c["form"], c["rows"]) for c in BNMLP} == {(f, r) for f in ("distance", "weight", "sum", "last") for r in R.BNMLP_ROWS}
    assert 272 % 128 == 16 and 528 % 128 == 528 % 256 == 528 % 512 == 16       # (1, 17) / (1, 33): whole chunks plus one tile
    for c in R.large_unit_cases():
        assert c["B"] * c["N"] * c["K"] // 16 == 2313 > 2048 and 2313 % 4 == 1  # past one grid sweep, the last round partial


LARGE = R.large_unit_cases() + [dict(id=f"bnmlp-{f}-large", form=f, rows=R.BNMLP_LARGE_ROWS, large=True) for f in ("weight", "sum")]


@pytest.mark.parametrize("case", LARGE, ids=[c["id"] for c in LARGE])
def test_large_cases_meet_their_input_conditions(case):
    """Large cases mask instead of keeping clear.  The inputs must keep the masked pools <= 2e-3 and the near-kink hidden
    elements <= 1e-4 of all, and the flip widening no larger than the UNWIDENED bar for the per-row input gradients (whose spoilt
    rows are left out) and no larger than the suite's existing tier-against-tier bar for the row-reduced ones
    (extract_train_ref.large_ceiling; the module docstring says why not the unwidened bar there).  Forward values and running
    statistics do not depend on a decision's side: their widening is zero."""
    prob, r64, r32, rec, extra = R.large_references(case)
    pools, kinks = rec.shares()
    assert pools <= R.MAX_POOL_SHARE and kinks <= R.MAX_KINK_SHARE, (pools, kinks)
    assert prob["masked"] > 0 or rec.clear()
    gmax = max(float(v.abs().max()) for k, v in r64.items() if k.startswith("d"))
    for k, v in r64.items():
        if R.is_residue(k, prob["kind"]):
            continue
        if not k.startswith("d"):
            assert extra[k] == 0.0, k
        if k in ("dx", "dxa", "dxb"):          # per-row gradients, the spoilt rows left out: the issue's own condition holds
            cap = R.bar_of(R.skip_rows(prob, r64)[k], R.skip_rows(prob, r32)[k])
        else:
            cap = R.large_ceiling(k, v, gmax)
        assert extra[k] <= cap, f"{case['id']} {k}: flip widening {extra[k]:.3e} > ceiling {cap:.3e}"
