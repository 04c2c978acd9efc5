"""tests/infer_ref.py (the float64 anchor that tests/test_gpu_infer_anchor.py holds the inference kernels to) against the pinned
oracle; the conditioning figures of the trained checkpoint, pinned; and the evidence that the committed bars notice a subtly
wrong kernel: the fp32 oracle with one unit's weights kept to 11 or 14 significant bits, two swapped output channels or one
wrong LeakyReLU slope misses that unit's bar.  No GPU."""
import numpy as np
import pytest
import torch

import infer_ref as R
from oracle import ref_cpu as O

TEETH_CASES = ("s4_3x24", "s0_2x256")


# ---------------------------------------------------------------------------------------------- the anchor is the oracle
# the fp32 oracle's measured distance from float64 (z, x, worst cs, ldj relative), each times 2
@pytest.mark.parametrize("case,z,x", [("s0_2x256", 1.2e-6, 1.4e-6), ("s4_5x61", 5.6e-7, 9.6e-7)])
def test_anchor_rounded_to_fp32_is_the_pinned_oracle(case, z, x):
    C = R.case(case)
    A, E = C["A"], C["E"]
    ref = O.forward(C["sd"], C["xyz"], 4, stages=True)
    assert torch.equal(A["idx16"], ref["idx16"]) and torch.equal(A["idx8"], ref["idx8"])
    e = E["e32"]
    print(case, {q: f"{v:.2e}" for q, v in e.items()})
    assert e["z"] <= 2 * z and e["x"] <= 2 * x
    assert e["fz"] <= 2 * z                                     # a convex combination of latents
    assert max(e[f"cs{i}"] for i in range(6)) <= 2 * 7.4e-7
    assert e["ldj"] <= 2 * 1.7e-7 and e["logp"] <= 2 * 1.7e-7
    # and the rounded anchor itself, not only the table: the same statement on the tensors
    assert float((A["z"].float() - ref["z"]).abs().max()) <= 2 * z + 2.0 ** -24 * float(ref["z"].abs().max())
    assert float((A["x"].float() - ref["x"]).abs().max()) <= 2 * x + 2.0 ** -24
    assert float((A["w"].float() - ref["w"]).abs().max()) <= 1e-6 and tuple(A["w"].shape) == tuple(ref["w"].shape)
    for i in range(6):
        assert float((A["hs"][i].float() - ref["hs"][i]).abs().max()) <= 4e-6 * float(ref["hs"][i].abs().max())


def test_stage_inputs_are_the_rounded_anchor_and_float64_is_float64():
    C = R.case("s4_3x24")
    A, S = C["A"], C["S"]
    assert all(t.dtype == torch.float64 for t in A["hs"] + A["cs"] + [A["z"], A["ldj"], A["logp"], A["w"], A["fz"], A["x"]])
    assert torch.equal(S["unit3"]["inp"]["h_in"], A["hs"][2].float()) and torch.equal(S["unit0"]["inp"]["h_in"], C["xyz"])
    assert torch.equal(S["cg"]["inp"]["fz"], A["fz"].float()) and torch.equal(S["interp"]["inp"]["z"], A["z"].float())
    for s in R.STAGES:
        for q, v in S[s]["out64"].items():
            assert v.dtype == torch.float64 and S[s]["out32"][q].dtype == torch.float32, (s, q)
            assert 0 < S[s]["e32"][q] < 1e-5, (s, q)             # the two evaluations differ, and by fp32 rounding only
    # a stage's float64 output on the rounded input is the anchor's own value up to that rounding
    assert float((S["unit5"]["out64"]["h"] - A["hs"][5]).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------------- the conditioning figures
@pytest.mark.parametrize("case", ["a", "b"])
def test_trained_checkpoint_conditioning_figures(case):
    """What the trained checkpoint does to an fp32 evaluation, measured instead of told: the fp32 oracle's latent z is a few
    1e-4 from float64 while x, which g computes back with the same cs, is within 1e-5; cs5 within 2e-6 of its scale; and the flow
    f alone, fed the float64 cs rounded to fp32, carries a large share of the latent's error - the flow's own arithmetic, not
    only the features.  The committed golden z (the reference's own run) is as far from float64 as the oracle's."""
    wkey, sd, xyz = R.case_inputs(f"ckpt_{case}")
    A = R.anchor(sd, xyz, 4)
    E = R.e2e(sd, xyz, 4, A)
    F = R.stages(sd, xyz, 4, A, which=("f",))["f"]
    e = E["e32"]
    scale5 = float(A["cs"][5].abs().max())
    print(f"case {case}: z {e['z']:.2e} fz {e['fz']:.2e} x {e['x']:.2e} cs5 {e['cs5']:.2e} of {scale5:.0f}; flow f alone z {F['e32']['z']:.2e}")
    assert 1e-4 <= e["z"] <= 1e-3
    assert e["x"] <= 1e-5
    assert e["cs5"] <= 2e-6 * scale5
    assert 5e-5 <= F["e32"]["z"] <= 1e-3
    g = R.pretrained()
    eg = R.err(torch.from_numpy(g[f"{case}/z"]), A["z"])
    print(f"case {case}: golden z {eg:.2e} from the anchor")
    assert e["z"] / 2 <= eg <= e["z"] * 2
    assert np.array_equal(g[f"{case}/idx16"].astype(np.int64), A["idx16"].numpy())


# ---------------------------------------------------------------------------------------------- the bars have teeth
def _unit_out(C, u, sd=None):
    S = C["S"][f"unit{u}"]
    return S, R.run_stage(f"unit{u}", C["sd"] if sd is None else sd, S["inp"], C["A"]["idx16"])


@pytest.mark.parametrize("case", TEETH_CASES)
@pytest.mark.parametrize("u", range(6))
def test_unit_bar_rejects_a_short_weight_image(case, u):
    """ONE unit's conv weights kept to 11 significant bits (a dropped low fp16 half) and to 14: the fp32 oracle misses that
    unit's committed bar.  The untouched oracle passes it, so the bar is not simply unattainable."""
    C = R.case(case)
    stage = f"unit{u}"
    S, clean = _unit_out(C, u)
    assert not R.rejected(stage, S, clean)
    for bits in (11, 14):
        S, out = _unit_out(C, u, R.degraded(C["sd"], stage, bits))
        e = R.err(out["h"], S["out64"]["h"])
        print(f"{case} unit {u}: {bits} bits -> {e:.2e} = {e / S['e32']['h']:.0f} x e32, bar {R.bar(stage, 'h', S):.2e}")
        assert R.rejected(stage, S, out), (case, u, bits)


@pytest.mark.parametrize("case", TEETH_CASES)
@pytest.mark.parametrize("u", range(6))
def test_unit_bar_rejects_swapped_channels_and_a_wrong_slope(case, u, monkeypatch):
    C = R.case(case)
    stage, pfx = f"unit{u}", f"feat_convs.{u}"
    sd = dict(C["sd"])
    for k in (pfx + ".conv_out.weight", pfx + ".conv_out.bias"):          # output channels 0 and 1 swapped
        t = sd[k].clone()
        t[[0, 1]] = t[[1, 0]]
        sd[k] = t
    S, out = _unit_out(C, u, sd)
    assert R.rejected(stage, S, out), "swapped channels"
    orig = O._conv_bn_lrelu

    def wrong_slope(sd_, p, f, slope, training=False):                    # LeakyReLU 0.01 in place of 0.05 in the first growth layer
        return orig(sd_, p, f, 0.01 if p == pfx + ".convs.0" else slope, training)
    monkeypatch.setattr(O, "_conv_bn_lrelu", wrong_slope)
    S, out = _unit_out(C, u)
    assert R.rejected(stage, S, out), "slope"


def test_finest_weight_image_every_stage_bar_rejects():
    """Per GPU stage: the largest number of kept weight bits the committed bar still rejects (printed; the table for both
    shapes is in profiles/infer_anchor/accuracy.txt).  Units must notice 14 bits; every stage must notice a dropped fp16 low
    half (11 bits)."""
    C = R.case("s4_3x24")
    for s in R.STAGES:
        if s in ("f", "g"):
            continue
        n = R.finest_rejected_bits(s, C["sd"], C["S"][s], C["A"]["idx16"], C["R"])
        print(f"{s}: rejects every weight image of {n} bits or fewer")
        assert n >= (14 if s.startswith("unit") else 11), s


# ---------------------------------------------------------------------------------------------- no bar admits more than the old
def _old(q, E, kind):
    """The bar tests/test_gpu_parity.py sets for quantity q on a case of its kind, in the units of infer_ref.err."""
    scale = float(E["ref64"][q].abs().max())
    if q in R.RELATIVE:
        return 1e-5
    if kind == "ckpt":
        return {"x": 1e-5, "z": 2e-3, "fz": 2e-3, "cs0": 2e-6 * scale, "cs5": 2e-6 * scale}.get(q)
    if kind == "tr":
        return None if q == "fz" else (1e-5 if q == "x" else 1e-5 * max(1.0, scale))
    return 1e-5


@pytest.mark.parametrize("case", ["s0_2x256", "s4_5x61", "tr3_2x256", "ckpt_a"])
def test_no_new_bar_admits_more_than_the_old_one(case):
    """On the cases the parity tests run, RATIO_E2E * e32 + floor never exceeds the old bar plus the fp32 oracle's own distance
    from float64; nor do the stage bars of unit 0 and of the interpolation exceed the 1e-5 their stage-isolated parity tests
    (tests/test_gpu_epilogue.py) hold on synthetic weights."""
    C = R.case(case)
    E = C["E"]
    kind = "ckpt" if case.startswith("ckpt") else "tr" if case.startswith("tr") else "synth"
    for q in R.E2E_QUANTITIES:
        old = _old(q, E, kind)
        if old is None:
            continue
        new = R.bar_e2e(q, E)
        print(f"{case} {q}: new bar {new:.3e}  old bar + oracle's error {old + E['e32'][q]:.3e}")
        assert new <= old + E["e32"][q], (case, q)
    if kind == "synth":
        for s, q in (("unit0", "h"), ("interp", "fz")):
            S = C["S"][s]
            assert R.bar(s, q, S) <= 1e-5 + S["e32"][q], (s, q)
