"""The inference kernels against the float64 anchor (tests/infer_ref.py), stage by stage and end to end.  The parity tests
(tests/test_gpu_parity.py) pin the fp32 oracle's bits with flat bars of 5 to 30 times that oracle's own rounding error; these
pin the truth with bars made of that error:

    max |gpu - stage64|  <=  RATIO[stage] * e32  +  2^-24 * max |stage64|

where stage64 / e32 are the float64 value of the stage on the fp32 input the kernel gets and the fp32 oracle's distance from it
on that same input (computed on the CPU, never from the kernels), and RATIO is twice the worst ratio measured on an MI355X,
rounded up to a power of two (profiles/infer_anchor/accuracy.txt; tests/test_infer_ref.py shows what the bars reject).  Every
output buffer is NaN-prefilled, so a row left unwritten fails.

Shapes (the smallest that reach the corners of the tile walks; tests/test_gpu_pq_tail.py, tests/test_gpu_epilogue.py):
  (1, 16)    smallest legal N for K = 16
  (3, 24)    T = 72 is no multiple of 16, batch items straddle a tile, most workgroups have no tile; R = 3 as well
  (5, 61)    N % 16 != 0: the two-launch log-likelihood path; a volume cloud
  (1, 272)   17 tiles; R = 8 as well (all 32 rows of the weight unit's last conv)
  (2, 256)   ordinary small shape: synthetic weights, trained-style weights, the trained checkpoint fixture (its case a)
Needs a real MI355X:  python -m pytest tests -m gpu"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import infer_ref as R

CASES = R.GPU_CASES
MODES = ("f16n", "f32")
EXTRA = [(c, r) for c, r in R.EXTRA_R.items()]


def _hold(rows):
    bad = []
    for r in rows:
        ratio = r["e_gpu"] / r["e32"] if r["e32"] > 0 else float("inf")
        print(f"{r['case']} {r['mode']} R={r['R']} {r['stage']:6s} {r['q']:4s} {r['form']}: e32 {r['e32']:.3e} e_gpu {r['e_gpu']:.3e} "
              f"ratio {ratio:.2f} bar {r['bar']:.3e}")
        if not r["e_gpu"] <= r["bar"]:           # a NaN (an unwritten row) fails too
            bad.append((r["stage"], r["form"], r["q"], r["e_gpu"], r["bar"]))
    assert not bad, bad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_edgeconv_units(case, mode):
    """(a) unit u: the fp32-rounded anchor h[u-1] (xyz for unit 0) through pf_pq_gemm and pf_edgeconv; in the product arithmetic
    also through pf_edgeconv_pq fuse 0, 1 and 2, whose h and next-unit P|Q tables must be bit-identical."""
    import infer_anchor_gpu as G
    for u in range(6):
        rows, _ = G.measure(case, mode, f"unit{u}")
        _hold(rows)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_conditioner_stage(case, mode):
    """(b) all six fp32-rounded anchor h through pf_cond_all: the conditioning features cs[0..5]."""
    import infer_anchor_gpu as G
    rows, _ = G.measure(case, mode, "cond")
    _hold(rows)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_flow_f_with_log_likelihood(case, mode):
    """(b) + (c): pf_cond_all's internal layouts (cp, st) through pf_flow_fwd_logp: z, per-item log-det and logp (the last two as
    relative errors)."""
    import infer_anchor_gpu as G
    rows, _ = G.measure(case, mode, "cf")
    _hold(rows)


@pytest.mark.parametrize("case,Rr,mode", [(c, 4, m) for c in CASES for m in MODES] + [(c, r, "f16n") for c, r in EXTRA])
def test_interpolation(case, Rr, mode):
    """(d) pf_interp (fz) and, for R <= 4, pf_interp_weights (w) on the fp32-rounded anchor z; the softmax weights sum to one."""
    import infer_anchor_gpu as G
    rows, forms = G.measure(case, mode, "interp", Rr)
    _hold(rows)
    if Rr <= 4:
        w = forms["pf_interp_weights"]["w"]
        assert float((w.double().sum(-1) - 1.0).abs().max()) <= 2.0 ** -22


@pytest.mark.parametrize("case,Rr,mode", [(c, 4, m) for c in CASES for m in MODES] + [(c, r, "f16n") for c, r in EXTRA])
def test_flow_g(case, Rr, mode):
    """(b) + (e): pf_flow_inv on the fp32-rounded anchor fz; for R <= 4 pf_flow_inv_interp on the fp32-rounded anchor weights and
    latents, and the split order's bits against the fused order's."""
    import infer_anchor_gpu as G
    rows, _ = G.measure(case, mode, "cg", Rr)
    _hold(rows)


@pytest.mark.parametrize("case,Rr,mode", [(c, 4, m) for c in CASES for m in MODES] + [(c, r, "f16n") for c, r in EXTRA])
def test_forward_end_to_end(case, Rr, mode):
    """forward_stages against the anchor: every quantity within RATIO_E2E times the fp32 oracle's own end-to-end distance from the
    anchor on that case.  On the trained checkpoint this is the bar of the latent: z and fz within a small multiple of the
    2.5e-4 the reference itself is away, where the parity test allows 2e-3."""
    import infer_anchor_gpu as G
    _hold(G.measure_e2e(case, mode, Rr))
