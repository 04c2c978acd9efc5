"""The HIP entry points of the inference path, one stage of tests/infer_ref.py at a time, fed the fp32-rounded anchor input and
writing into NaN-prefilled buffers.  Shared by tests/test_gpu_infer_anchor.py (which asserts the bars) and
tools/infer_anchor_report.py (which measures the ratios the bars are made of).  Needs a real MI355X."""
import functools

import torch

import infer_ref as R
from oracle import ref_cpu as O

DEV = "cuda:0"
MODES = ("f16n", "f32")
NB = O.NUM_BLOCKS


@functools.lru_cache(maxsize=None)
def net(wkey: str, mode: str):
    """One module per (weights, EdgeConv arithmetic): the packed plan depends on both."""
    from puflow_amd import _lib
    from puflow_amd.interpflow import PointInterpFlow
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _lib.load()                                  # raises if the HIP library is missing: no silent fallback
    n = PointInterpFlow(3)
    n.load_state_dict(R.weights(wkey))
    n.set_to_initialized_state()
    n = n.to(DEV).eval()
    n.ec_mode = mode
    assert n._engine(4).ec_mode == mode
    return n


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _dev(t):
    return t.float().contiguous().to(DEV)


def _idx(C):
    return C["A"]["idx16"].to(torch.int32).contiguous().to(DEV)


def _check(rc, what):
    assert rc == 0, (what, rc)


# ------------------------------------------------------------------------------------------------ stage runners
# each -> {form name: {quantity: tensor on the CPU, shaped like the stage's out64}}, and a list of (name a, name b) forms whose
# outputs must be bit-identical
def run_unit(e, C, u):
    from puflow_amd.packing import FEAT_CHANNELS
    B, N, _ = C["xyz"].shape
    T, s, idx = B * N, e._stream(), _idx(C)
    h_in = _dev(C["S"][f"unit{u}"]["inp"]["h_in"]).view(T, -1)
    if u == 0:
        src = h_in
    else:                                        # the unit reads the per-point P|Q vectors of its input
        src = _nan(T, 512)                       # unit 1 reads it densely packed as [T, 256]
        _check(e.lib.pf_pq_gemm(u - 1, h_in.data_ptr(), e.base, e.post[u - 1], src.data_ptr(), T, s), f"pf_pq_gemm[{u - 1}]")
    odim = FEAT_CHANNELS[u + 1]
    h = _nan(T, odim)
    e._edgeconv(u, src.data_ptr(), idx, h, B, N, s)
    forms, same, tables = {"pf_edgeconv": h}, [], {}
    if e.ec_mode == "f16n" and u < NB - 1:       # the product arithmetic has the forms that write the next unit's P|Q table too
        w = e.ec1n_w[u] if u < 2 else e.ec4_w[u]
        for fuse in (0, 1, 2):
            out, nxt = _nan(T, odim), _nan(T, 256 if u == 0 else 512)
            _check(e.lib.pf_edgeconv_pq(u, src.data_ptr(), idx.data_ptr(), e._p(w), out.data_ptr(), e.base, e.post[u],
                                        nxt.data_ptr(), B, N, fuse, s), f"pf_edgeconv_pq[{u}] fuse {fuse}")
            forms[f"pf_edgeconv_pq fuse {fuse}"], tables[fuse] = out, nxt
            same.append(("pf_edgeconv", f"pf_edgeconv_pq fuse {fuse}"))
    torch.cuda.synchronize()
    for fuse in (1, 2):
        if fuse in tables:                       # the next unit's table: every row written, the two-launch bits
            assert not torch.isnan(tables[0]).any(), (u, "pq_next of the two-launch form")
            assert torch.equal(tables[0], tables[fuse]), (u, fuse, "pq_next")
    return {k: {"h": v.cpu().view(B, N, odim)} for k, v in forms.items()}, same


def _cond(e, C, stage, want_cs):
    B, N, _ = C["xyz"].shape
    T, s = B * N, e._stream()
    from puflow_amd.packing import COND_CHANNELS
    hs = [_dev(h).view(T, -1) for h in C["S"][stage]["inp"]["hs"]]
    cs = [_nan(B, N, COND_CHANNELS[i]) for i in range(NB)] if want_cs else None
    st, cp = _nan(NB, T, 8), _nan(NB, T, 64)
    e._cond_all(hs, cs, st, cp, T, s)
    return cs, st, cp


def run_cond(e, C):
    cs, st, cp = _cond(e, C, "cond", True)
    torch.cuda.synchronize()
    return {"pf_cond_all": {f"cs{i}": cs[i].cpu() for i in range(NB)}}, []


def run_cf(e, C):
    B, N, _ = C["xyz"].shape
    T, s = B * N, e._stream()
    _, st, cp = _cond(e, C, "cf", False)
    xyz = _dev(C["xyz"])
    z, ld_pt, ldj, lps, logp = _nan(B, N, 3), _nan(T), _nan(B), _nan(B), _nan(1)
    ws = e.logp_ws(B, N, DEV)
    _check(e.lib.pf_flow_fwd_logp(xyz.data_ptr(), cp.data_ptr(), st.data_ptr(), e._p(e.flow), z.data_ptr(), ld_pt.data_ptr(),
                                  e.ld_const, B, N, ldj.data_ptr(), lps.data_ptr(), logp.data_ptr(), ws.data_ptr(), s),
           "pf_flow_fwd_logp")
    torch.cuda.synchronize()
    assert not torch.isnan(ld_pt).any() and not torch.isnan(lps).any()
    return {"pf_cond_all + pf_flow_fwd_logp": {"z": z.cpu(), "ldj": ldj.cpu(), "logp": logp.cpu()}}, []


def run_interp(e, C):
    B, N, _ = C["xyz"].shape
    Rr, s, idx = C["R"], e._stream(), _idx(C)
    inp = C["S"]["interp"]["inp"]
    xyz, z = _dev(inp["xyz"]), _dev(inp["z"])
    u = _nan(B, N * Rr, 3)
    _check(e.lib.pf_interp(xyz.data_ptr(), z.data_ptr(), idx.data_ptr(), e.base, e.interp_off, u.data_ptr(), B, N, Rr, s), "pf_interp")
    out = {"pf_interp": {"fz": u.view(B, N, Rr, 3).transpose(2, 3).cpu()}}
    if Rr <= 4:
        aw = _nan(B * N, 8, 4)
        _check(e.lib.pf_interp_weights(xyz.data_ptr(), idx.data_ptr(), e.base, e.interp_off, aw.data_ptr(), B, N, s), "pf_interp_weights")
        out["pf_interp_weights"] = {"w": aw.view(B, N, 8, 4)[..., :Rr].permute(0, 1, 3, 2).cpu()}
    torch.cuda.synchronize()
    return out, []


def run_cg(e, C):
    """x from the fp32-rounded fz (pf_flow_inv); for R <= 4 also from the fp32-rounded weights and latents, the weighted sum
    formed inside the flow kernel (pf_flow_inv_interp; stage `icg`), and the identity of the split and the fused order on the
    GPU's own interpolation weights."""
    B, N, _ = C["xyz"].shape
    Rr, s, idx = C["R"], e._stream(), _idx(C)
    T = B * N
    _, st, cp = _cond(e, C, "cg", False)
    fz = C["S"]["cg"]["inp"]["fz"]                                              # [B, N, 3, R]
    u = _dev(torch.flatten(fz.transpose(2, 3), 1, 2))                          # [B, N R, 3], row n R + r
    x = _nan(B, N * Rr, 3)
    _check(e.lib.pf_flow_inv(u.data_ptr(), cp.data_ptr(), st.data_ptr(), e._p(e.flow), x.data_ptr(), T, Rr, s), "pf_flow_inv")
    out, same = {"pf_cond_all + pf_flow_inv": {"x": x.cpu()}}, []
    if Rr <= 4:
        inp = C["S"]["icg"]["inp"]
        z, xyz = _dev(inp["z"]), _dev(C["xyz"])
        aw = torch.zeros(B, N, 8, 4)
        aw[..., :Rr] = inp["w"].permute(0, 1, 3, 2)
        aw = _dev(aw).view(T, 8, 4)
        x2 = _nan(B, N * Rr, 3)
        _check(e.lib.pf_flow_inv_interp(aw.data_ptr(), z.data_ptr(), idx.data_ptr(), cp.data_ptr(), st.data_ptr(), e._p(e.flow),
                                        x2.data_ptr(), B, N, Rr, s), "pf_flow_inv_interp")
        out["icg: pf_cond_all + pf_flow_inv_interp"] = {"x": x2.cpu()}
        # split order == fused order, bit for bit, on what the GPU's own interpolation module returns
        ua, awg, xa, xb = _nan(B, N * Rr, 3), _nan(T, 8, 4), _nan(B, N * Rr, 3), _nan(B, N * Rr, 3)
        _check(e.lib.pf_interp(xyz.data_ptr(), z.data_ptr(), idx.data_ptr(), e.base, e.interp_off, ua.data_ptr(), B, N, Rr, s), "pf_interp")
        _check(e.lib.pf_flow_inv(ua.data_ptr(), cp.data_ptr(), st.data_ptr(), e._p(e.flow), xa.data_ptr(), T, Rr, s), "pf_flow_inv")
        _check(e.lib.pf_interp_weights(xyz.data_ptr(), idx.data_ptr(), e.base, e.interp_off, awg.data_ptr(), B, N, s), "pf_interp_weights")
        _check(e.lib.pf_flow_inv_interp(awg.data_ptr(), z.data_ptr(), idx.data_ptr(), cp.data_ptr(), st.data_ptr(), e._p(e.flow),
                                        xb.data_ptr(), B, N, Rr, s), "pf_flow_inv_interp")
        torch.cuda.synchronize()
        assert not torch.isnan(xa).any() and torch.equal(xa, xb), "pf_interp + pf_flow_inv != pf_interp_weights + pf_flow_inv_interp"
    torch.cuda.synchronize()
    return out, same


RUNNERS = {**{f"unit{u}": functools.partial(run_unit, u=u) for u in range(NB)},
           "cond": run_cond, "cf": run_cf, "interp": run_interp, "cg": run_cg}
GPU_STAGES = tuple(RUNNERS)


def measure(case: str, mode: str, stage: str, Rr: int = 4):
    """Run `stage` of `case` on the GPU in `mode` -> rows (stage, form, quantity, e32, floor, e_gpu, bar); the bit-identities of
    the forms are asserted here."""
    C = R.case(case, Rr)
    e = net(C["wkey"], mode)._engine(4)
    forms, same = RUNNERS[stage](e, C)
    for a, b in same:
        for q in forms[a]:
            assert torch.equal(forms[a][q], forms[b][q]), (stage, a, b, q)
    rows = []
    for form, outs in forms.items():
        sname = "icg" if form.startswith("icg") else stage
        S = C["S"][sname]
        for q, got in outs.items():
            rows.append(dict(case=case, mode=mode, R=Rr, stage=sname, form=form, q=q, e32=S["e32"][q], floor=S["floor"][q],
                             e_gpu=R.err(got, S["out64"][q], q in R.RELATIVE), bar=R.bar(sname, q, S)))
    return rows, forms


def measure_e2e(case: str, mode: str, Rr: int = 4):
    """forward_stages of `case` in `mode` against the anchor -> rows as `measure`, stage "e2e"."""
    C = R.case(case, Rr)
    n = net(C["wkey"], mode)
    st = n.forward_stages(C["xyz"].to(DEV), Rr)
    torch.cuda.synchronize()
    assert torch.equal(st["idx16"].cpu().long(), C["A"]["idx16"])
    got = R.e2e_view({k: ([c.cpu() for c in v] if k == "cs" else v.cpu()) for k, v in st.items() if k in ("cs", "z", "ldj", "logp", "fz", "x")})
    E = C["E"]
    return [dict(case=case, mode=mode, R=Rr, stage="e2e", form="forward_stages", q=q, e32=E["e32"][q], floor=E["floor"][q],
                 e_gpu=R.err(got[q], E["ref64"][q], q in R.RELATIVE), bar=R.bar_e2e(q, E)) for q in R.E2E_QUANTITIES]
