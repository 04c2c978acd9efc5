"""The float64 anchor of the INFERENCE path.  TEST INFRASTRUCTURE ONLY; imports nothing from the GPU side.

The oracle's stage functions (oracle/ref_cpu.py) are dtype-agnostic: given a state dict whose floating tensors are float64 and
float64 inputs they evaluate the same network in float64.  `anchor` composes them into the whole forward; `stages` cuts that
forward into the pieces the HIP library exposes and evaluates every piece twice ON THE SAME fp32 INPUT (the anchor's value of the
piece's input, rounded to fp32): in float64 (`out64`) and with the fp32 oracle (`out32`).  `e32 = max |out32 - out64|` is the
reference's own rounding error on that input - the yardstick of every bar in tests/test_gpu_infer_anchor.py:

    max |gpu - out64|  <=  RATIO[quantity] * e32  +  2^-24 * max |out64|

The neighbour lists are always the canonical ones of the fp32 cloud, so every evaluation gathers the same rows.

Stages (the input is what the HIP entry points take, the output what they return):
  unit0 .. unit5   h[u-1] (xyz for unit 0)  ->  h[u]                       pf_pq_gemm + pf_edgeconv, pf_edgeconv_pq
  cond             h[0..5]                  ->  cs[0..5]                   pf_cond_all
  f                xyz, cs                  ->  z, ldj, logp               (the arithmetic of flow f alone: CPU figures only)
  cf               xyz, h[0..5]             ->  z, ldj, logp               pf_cond_all + pf_flow_fwd_logp
  interp           xyz, z                   ->  w, fz                      pf_interp, pf_interp_weights
  g                fz, cs                   ->  x                          (flow g alone: CPU figures only)
  cg               fz, h[0..5]              ->  x                          pf_cond_all + pf_flow_inv
  icg              w, z, h[0..5]            ->  x                          pf_cond_all + pf_flow_inv_interp (the weighted latent sum
                                                                           formed inside the flow kernel, R <= 4)
The library hands the conditioner's result to the flow kernels in internal layouts (cp, st), so on the GPU the flows are reached
from h, not from cs: `cf` and `cg` are the stages the GPU tests hold; `f` and `g` isolate the flows' own arithmetic on the CPU.

The constants RATIO / RATIO_E2E cannot be derived (the kernels sum in another order and split their operands): they are twice the
worst ratio measured on an MI355X over the cases of tests/test_gpu_infer_anchor.py and both EdgeConv arithmetic modes, rounded up
to the next power of two (twice: the maximum of rounding noise over a few thousand elements moves by about a factor of 2 between
seeds).  The ratio measured is the one the bar needs, (e_gpu - floor) / e32: it is e_gpu / e32 wherever e32 is well above the
floor, and stays meaningful for a single number such as logp, whose fp32 value can by chance lie within a hundredth of an ulp
of the float64 one.  The measurements, and what the bars can notice, are in ACCURACY_FILE (written by
tools/infer_anchor_report.py)."""
from __future__ import annotations

import functools
import math
import os
from typing import Dict

import numpy as np
import torch

from oracle import ref_cpu as O
from puflow_amd.weights import synth_patches, synth_state_dict

ACCURACY_FILE = os.path.join("profiles", "infer_anchor", "accuracy.txt")     # relative to the repository root

# stage-isolated bars: quantity -> ratio (units: one per EdgeConv unit), synthetic and trained-style weights
RATIO = {
    "unit": (4.0, 4.0, 4.0, 2.0, 4.0, 2.0),
    "cs": 2.0,
    "z": 4.0, "ldj": 2.0, "logp": 8.0,
    "w": 2.0, "fz": 2.0,
    "x": 4.0,
}
# the same for the trained checkpoint's weights, scoped on their own so that what they need does not loosen the other cases:
# flow g needs 4.3 there (log-scales up to 5.3 through the one-multiply exp of csrc/pf_mfma.h, 1 x e32 by itself, and operand
# images of conditioning features up to 481 at 2^-21 relative, 1 to 2 x e32), 1.1 everywhere else
RATIO_CKPT = {
    "unit": (2.0, 2.0, 2.0, 2.0, 2.0, 2.0),
    "cs": 4.0,
    "z": 4.0, "ldj": 2.0, "logp": 2.0,
    "w": 4.0, "fz": 2.0,
    "x": 16.0,
}
# end-to-end bars: quantity -> ratio on the fp32 oracle's end-to-end distance from the anchor.  cs and x are capped below the
# rule's 4 by the parity tests' bars on the trained checkpoint (cs5 within 2e-6 of its scale, x within 1e-5): no bar here admits
# more than the old bar plus the oracle's own error (tests/test_infer_ref.py); the worst measured ratios are 1.56 and 1.35
RATIO_E2E = {"cs": 3.0, "z": 4.0, "ldj": 2.0, "logp": 4.0, "fz": 4.0, "x": 3.5}

FLOOR = 2.0 ** -24                      # half an ulp at the quantity's scale: only matters where e32 happens to be near zero
RELATIVE = ("ldj", "logp")              # quantities compared as relative errors


# ------------------------------------------------------------------------------------------------ cases
# name -> (weights, data seed, B, N, surface).  Weights: "s<seed>" synth_state_dict(seed); "tr<seed>" trained-style weights
# calibrated by the oracle (tests/test_gpu_parity.py test_trained_style_dynamic_range); "ckpt" the trained checkpoint fixture.
CASES = {
    "s0_1x16": ("s0", 16, 1, 16, True),          # smallest legal N for K = 16
    "s4_3x24": ("s4", 27, 3, 24, False),         # T = 72: no multiple of 16, items straddle a tile, most workgroups have no tile
    "s4_5x61": ("s4", 2, 5, 61, False),          # N % 16 != 0: the two-launch log-likelihood path (a case of the parity tests)
    "s0_1x272": ("s0", 273, 1, 272, True),       # 17 tiles
    "s0_2x256": ("s0", 0, 2, 256, True),         # ordinary small shape (a case of the parity tests)
    "tr3_2x256": ("tr3", 2, 2, 256, True),       # trained-style dynamic range
    "ckpt_a": ("ckpt", None, 2, 256, True),      # the trained checkpoint fixture, its case a
}
GPU_CASES = tuple(CASES)
EXTRA_R = {"s4_3x24": 3, "s0_1x272": 8}          # other up ratios, for the interpolation and flow g stages


def golden_dir() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def pretrained():
    """tests/golden/pretrained_pu1k.npz with the outputs as captured under the MKL branch the suite pins (tests/conftest.py)."""
    g = np.load(os.path.join(golden_dir(), "pretrained_pu1k.npz"))
    d = np.load(os.path.join(golden_dir(), "pretrained_pu1k_compat.npz"))
    out = {k: g[k] for k in g.files}
    for k in d.files:
        out[k] = out[k] + d[k]
    return out


@functools.lru_cache(maxsize=None)
def weights(key: str):
    if key == "ckpt":
        g = pretrained()
        return {k[3:]: torch.from_numpy(g[k]) for k in g if k.startswith("sd/")}
    if key.startswith("tr"):
        return O.calibrate(synth_state_dict(int(key[2:]), style="trained"), synth_patches(4, 256, seed=1))
    return synth_state_dict(int(key[1:]))


def case_inputs(name: str):
    """-> (weights key, state dict, xyz fp32 [B,N,3])"""
    if name == "ckpt_b":
        wkey, seed, B, N, surface = "ckpt", None, 1, 2048, True
    else:
        wkey, seed, B, N, surface = CASES[name]
    if wkey == "ckpt":
        B, N, seed = (int(v) for v in pretrained()[f"{name[-1]}/meta"])
    return wkey, weights(wkey), synth_patches(B, N, seed=seed, surface=surface)


# ------------------------------------------------------------------------------------------------ dtype plumbing
def to64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def r32(t):
    """float64 value -> the fp32 the kernels are fed (lists element-wise)"""
    if isinstance(t, (list, tuple)):
        return [r32(v) for v in t]
    return t.float()


def r64(t):
    if isinstance(t, (list, tuple)):
        return [r64(v) for v in t]
    return t.double()


# ------------------------------------------------------------------------------------------------ stage functions
# each: (state dict, inputs in the state dict's dtype, neighbour lists, R) -> dict of named outputs
def st_unit(u):
    def fn(sd, inp, idx16, R):
        return {"h": O.edgeconv_unit(sd, f"feat_convs.{u}", inp["h_in"], idx16)}
    return fn


def st_cond(sd, inp, idx16, R):
    return {f"cs{i}": O.feat_merge(sd, i, inp["hs"][i]) for i in range(O.NUM_BLOCKS)}


def _logp(sd, xyz, cs):
    z, logp, ldj = O.log_prob(sd, xyz, cs)
    return {"z": z, "ldj": ldj, "logp": logp.reshape(1)}


def st_f(sd, inp, idx16, R):
    return _logp(sd, inp["xyz"], inp["cs"])


def st_cf(sd, inp, idx16, R):
    return _logp(sd, inp["xyz"], [O.feat_merge(sd, i, inp["hs"][i]) for i in range(O.NUM_BLOCKS)])


def st_interp(sd, inp, idx16, R):
    fz, w = O.interp(sd, inp["z"], inp["xyz"], idx16[..., :O.K_INTERP].contiguous(), R)
    return {"w": w, "fz": fz}


def st_g(sd, inp, idx16, R):
    return {"x": O.flow_g(sd, inp["fz"], inp["cs"], R)}


def st_cg(sd, inp, idx16, R):
    return {"x": O.flow_g(sd, inp["fz"], [O.feat_merge(sd, i, inp["hs"][i]) for i in range(O.NUM_BLOCKS)], R)}


def st_icg(sd, inp, idx16, R):
    nz = O.knn_gather(inp["z"], idx16[..., :O.K_INTERP].contiguous()).permute(0, 1, 3, 2)
    fz = torch.einsum("bnck,bnrk->bncr", nz, inp["w"])
    return {"x": O.flow_g(sd, fz, [O.feat_merge(sd, i, inp["hs"][i]) for i in range(O.NUM_BLOCKS)], R)}


STAGE_FN = {**{f"unit{u}": st_unit(u) for u in range(O.NUM_BLOCKS)},
            "cond": st_cond, "f": st_f, "cf": st_cf, "interp": st_interp, "g": st_g, "cg": st_cg, "icg": st_icg}
STAGES = tuple(STAGE_FN)


def ratio_of(stage: str, q: str, wkey: str = "") -> float:
    """The committed constant that bounds output `q` of `stage` on weights `wkey`."""
    tab = RATIO_CKPT if wkey == "ckpt" else RATIO
    if stage.startswith("unit"):
        return tab["unit"][int(stage[4:])]
    return tab["cs"] if q.startswith("cs") else tab[q]


# ------------------------------------------------------------------------------------------------ the anchor
@torch.no_grad()
def anchor(sd, xyz, R: int = 4) -> dict:
    """The whole forward in float64 on the fp32 cloud's canonical neighbour lists."""
    xyz = xyz.float()
    _, idx16 = O.knn_canonical(xyz, xyz, O.K_FEAT)
    idx8 = idx16[..., :O.K_INTERP].contiguous()
    sd64, x64 = to64(sd), xyz.double()
    cs, hs = O.feat_extract(sd64, x64, idx16)
    z, logp, ldj = O.log_prob(sd64, x64, cs)
    fz, w = O.interp(sd64, z, x64, idx8, R)
    x = O.flow_g(sd64, fz, cs, R)
    return dict(idx16=idx16, idx8=idx8, hs=hs, cs=cs, z=z, ldj=ldj, logp=logp, w=w, fz=fz, x=x)


def stage_inputs(A: dict, xyz) -> Dict[str, dict]:
    """Per stage: its input, the anchor's value rounded to fp32."""
    xyz = xyz.float()
    hs, cs = r32(A["hs"]), r32(A["cs"])
    out = {f"unit{u}": {"h_in": xyz if u == 0 else hs[u - 1]} for u in range(O.NUM_BLOCKS)}
    out["cond"] = {"hs": hs}
    out["f"] = {"xyz": xyz, "cs": cs}
    out["cf"] = {"xyz": xyz, "hs": hs}
    out["interp"] = {"xyz": xyz, "z": r32(A["z"])}
    out["g"] = {"fz": r32(A["fz"]), "cs": cs}
    out["cg"] = {"fz": r32(A["fz"]), "hs": hs}
    out["icg"] = {"w": r32(A["w"]), "z": r32(A["z"]), "hs": hs}
    return out


def err(got, ref64, relative: bool = False) -> float:
    """max |got - ref64| (relative: max of |got - ref64| / |ref64|), in float64; NaN where `got` holds one."""
    d = (got.double().reshape(ref64.shape) - ref64).abs()
    if relative:
        d = d / ref64.abs()
    return float("nan") if bool(torch.isnan(d).any()) else float(d.max())


def floor_of(ref64, relative: bool = False) -> float:
    return FLOOR if relative else FLOOR * float(ref64.abs().max())


@torch.no_grad()
def run_stage(stage: str, sd, inp32: dict, idx16, R: int = 4) -> dict:
    """The fp32 oracle's `stage` with weights `sd` on the fp32 input."""
    return STAGE_FN[stage](sd, inp32, idx16, R)


@torch.no_grad()
def stages(sd, xyz, R: int = 4, A: dict = None, which=STAGES, wkey: str = "") -> Dict[str, dict]:
    """Per stage: inp (fp32), out64, out32, e32 and floor per output quantity."""
    A = anchor(sd, xyz, R) if A is None else A
    sd64 = to64(sd)
    inputs = stage_inputs(A, xyz)
    res = {}
    for s in which:
        inp = inputs[s]
        out64 = STAGE_FN[s](sd64, {k: r64(v) for k, v in inp.items()}, A["idx16"], R)
        out32 = STAGE_FN[s](sd, inp, A["idx16"], R)
        rel = {q: q in RELATIVE for q in out64}
        res[s] = dict(inp=inp, out64=out64, out32=out32, wkey=wkey,
                      e32={q: err(out32[q], out64[q], rel[q]) for q in out64},
                      floor={q: floor_of(out64[q], rel[q]) for q in out64})
    return res


def bar(stage: str, q: str, S: dict) -> float:
    """ratio * e32 + floor for output q of a `stages` entry"""
    return ratio_of(stage, q, S.get("wkey", "")) * S["e32"][q] + S["floor"][q]


# ------------------------------------------------------------------------------------------------ end to end
E2E_QUANTITIES = ("cs0", "cs1", "cs2", "cs3", "cs4", "cs5", "z", "ldj", "logp", "fz", "x")


def e2e_view(st: dict) -> dict:
    """A stages=True dict of the oracle, the anchor, or the GPU's forward_stages -> quantity -> tensor"""
    out = {f"cs{i}": st["cs"][i] for i in range(O.NUM_BLOCKS)}
    out.update(z=st["z"], ldj=st["ldj"], logp=st["logp"].reshape(1), fz=st["fz"], x=st["x"])
    return out


@torch.no_grad()
def e2e(sd, xyz, R: int = 4, A: dict = None) -> dict:
    """ref64 (the anchor), e32 (the fp32 oracle's end-to-end distance from it) and floor per quantity."""
    A = anchor(sd, xyz, R) if A is None else A
    ref64 = e2e_view(A)
    o32 = e2e_view(O.forward(sd, xyz, R, stages=True))
    rel = {q: q in RELATIVE for q in ref64}
    return dict(ref64=ref64, out32=o32, e32={q: err(o32[q], ref64[q], rel[q]) for q in ref64},
                floor={q: floor_of(ref64[q], rel[q]) for q in ref64})


def bar_e2e(q: str, E: dict) -> float:
    return RATIO_E2E["cs" if q.startswith("cs") else q] * E["e32"][q] + E["floor"][q]


# ------------------------------------------------------------------------------------------------ cached per case
@functools.lru_cache(maxsize=None)
def case(name: str, R: int = 4) -> dict:
    """Everything the tests of a case share, computed once and never written again: sd, xyz, the anchor, the stage table, the
    end-to-end table."""
    wkey, sd, xyz = case_inputs(name)
    A = anchor(sd, xyz, R)
    return dict(name=name, wkey=wkey, sd=sd, xyz=xyz, R=R, A=A, S=stages(sd, xyz, R, A, wkey=wkey), E=e2e(sd, xyz, R, A))


# ------------------------------------------------------------------------------------------------ deliberate faults
def round_bits(w, bits: int):
    """w rounded to `bits` significant bits (round to nearest, exponent kept): a weight image that lost its low part"""
    m, e = torch.frexp(w.double())
    return torch.ldexp(torch.round(m * 2.0 ** bits) / 2.0 ** bits, e).to(w.dtype)


STAGE_WEIGHTS = {**{f"unit{u}": (f"feat_convs.{u}.",) for u in range(O.NUM_BLOCKS)},
                 "cond": ("merge_convs.",), "f": ("flow_blocks.",), "cf": ("merge_convs.", "flow_blocks."),
                 "interp": ("interp.",), "g": ("flow_blocks.",), "cg": ("merge_convs.", "flow_blocks."),
                 "icg": ("merge_convs.", "flow_blocks.")}


def degraded(sd, stage: str, bits: int):
    """sd with the matrix weights (conv / linear `.weight` of 2 or more dimensions) of `stage` kept to `bits` bits."""
    out = dict(sd)
    for k, v in sd.items():
        if k.startswith(STAGE_WEIGHTS[stage]) and k.endswith(".weight") and v.dim() >= 2:
            out[k] = round_bits(v, bits)
    return out


def rejected(stage: str, S: dict, out: dict) -> bool:
    """Does any output of a (faulty) evaluation of `stage` miss the committed bar?"""
    for q, ref64 in S["out64"].items():
        e = err(out[q], ref64, q in RELATIVE)
        if not e <= bar(stage, q, S):
            return True
    return False


def finest_rejected_bits(stage: str, sd, S: dict, idx16, R: int = 4) -> int:
    """The largest number of kept weight bits (of the fp32 oracle's weights for `stage`) whose result the stage's bar still
    rejects; every coarser image is rejected too when the scan finds no gap.  0: even an 8-bit image passes."""
    best, gap = 0, False
    for bits in range(8, 24):
        rej = rejected(stage, S, run_stage(stage, degraded(sd, stage, bits), S["inp"], idx16, R))
        if rej and not gap:
            best = bits
        else:
            gap = True
    return best


def pow2_ceil(v: float) -> float:
    return 2.0 ** math.ceil(math.log2(v)) if v > 0 else 1.0


def constant_from(worst_ratio: float) -> float:
    """The rule of the constants: twice the worst measured ratio, rounded up to the next power of two; never below 2."""
    return max(2.0, pow2_ceil(2.0 * worst_ratio))
