"""The training kernels of the flow blocks, all three tiers, against the float64 restatement of tests/flow_train_ref.py:
the per-op nodes (train_perop, csrc/train_ops.hip), the per-block fused nodes (train_fusedfn, csrc/train_flow.hip and
csrc/train_mlp.hip) and FlowChainFn (csrc/train_flowchain.hip).  Every node output and EVERY gradient - inputs, dcflat, dst, all
eight parameters of every block - is held to

    |gpu - ref64| <= 16 max|ref32 - ref64| + 2^-21 max|ref64|        per tensor,

ref32 being the same restatement in float32 on the CPU: the bar never sees a kernel (tests/test_flow_train_ref.py shows on the
CPU that it catches a dropped log|det W|, a wrong sign, a swapped split, ... in every chain case).  Cases with hidden LeakyReLU
layers use seeds chosen on the CPU that keep the float64 pre-activations >= 2e-5 away from the kink; each test asserts that
first.  `pytest -s` prints err / bar per case and quantity (profiles/flow_train/accuracy.txt)."""
import ctypes

import pytest
import torch

import flow_train_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

# Row-reduced quantities (parameter gradients, ssum, ld, logp) whose honest float32 summation needs more than the bar: case id ->
# {name: the terms it sums, from the case's inputs and upstream weights}.  Their bar grows by R.sum_envelope(terms), the rounding
# of a float32 tree sum over those terms (never beyond R.ceiling_of, the suite's tier-against-tier bar).  Both are sums whose terms
# cancel - sum(s) over 197 379 values of either sign, db4 = the column sums of 68 random output weights - so that the kernel's
# rounding is a few ulp of the partial sums but more than the float32 CPU run happened to lose in its own order; measured
# err / bar before widening: 1.42 and 1.22 (profiles/flow_train/accuracy.txt).  Per-row quantities are never listed.
WIDENED = {
    "couple_inject2-td2-rows65793-dssum0": {"ssum": lambda inputs, upstream: inputs["s"].reshape(-1, 1)},
    "couple_inject2-td2-rows65793-dssum1": {"ssum": lambda inputs, upstream: inputs["s"].reshape(-1, 1)},
    "mlp-td2-cdiv4-cc128-T17": {"db4": lambda inputs, upstream: upstream["out"]},
}


def _hold(case, ref, gpu, inputs, upstream, kinks=False):
    """One case: the restatement in float64 and float32 on the CPU, the node on the GPU, every tensor against the bar."""
    if kinks:
        assert R.min_preactivation(lambda: ref(inputs)) >= R.MIN_PREACT, "the case's seed no longer keeps off the LeakyReLU kinks"
    r64 = R.grads(ref, inputs, upstream)
    r32 = R.grads(ref, inputs, upstream, dtype=torch.float32)
    got = R.grads(gpu, inputs, upstream, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    assert set(got) == set(r64), set(got) ^ set(r64)
    widened = {k: terms(inputs, upstream) for k, terms in WIDENED.get(case, {}).items()}
    cmp = R.compare(got, r64, r32, widened)
    print("\n" + R.report(case, cmp, widened), end="")
    assert not R.failures(cmp), (case, R.failures(cmp))
    return got


def _rng(*key):
    """A generator per (test, parameters): the seed is the key's digits in base 100 003."""
    import numpy as np
    seed = 0
    for k in key:
        seed = seed * 100003 + int(k) + 1
    return np.random.Generator(np.random.PCG64(seed))


def _affine_params(seed, negative=False):
    sd = R.make_blocks(2, [32, 32], [1, 1], seed)
    p = "flow_blocks.1." if negative else "flow_blocks.0."
    return sd[p + "actnorm.logs"], sd[p + "actnorm.bias"], sd[p + "permutate1.permutater.W"]


ROWS = (1, 255, 257)


# ------------------------------------------------------------------------------------------------ a. per-op nodes
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("inv", [0, 1])
def test_actnorm_node(inv, rows):
    from puflow_amd.train_perop import ActNormFn
    rng = _rng(1, inv, rows)
    logs, bias, _ = _affine_params(3)
    inputs = {"x": R.randn(rng, (1, rows, 3)), "logs": logs, "bias": bias}
    _hold(f"actnorm-inv{inv}-rows{rows}", lambda lv: {"y": R.actnorm(lv["x"], lv["logs"], lv["bias"], inv)},
          lambda lv: {"y": ActNormFn.apply(lv["x"], lv["logs"], lv["bias"], inv)}, inputs, {"y": R.randn(rng, (1, rows, 3))})


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("td", [1, 2])
def test_couple_inject_node(td, rows):
    from puflow_amd.train_perop import CoupleInjectFn
    rng = _rng(2, td, rows)
    inputs = {"y": R.randn(rng, (rows, 3)), "o": R.randn(rng, (rows, 3 - td)), "s": R.randn(rng, (rows, 3), scale=0.3),
              "t": R.randn(rng, (rows, 3), scale=0.5)}
    _hold(f"couple_inject-td{td}-rows{rows}", lambda lv: {"out": R.couple_inject(lv["y"], lv["o"], lv["s"], lv["t"], td)},
          lambda lv: {"out": CoupleInjectFn.apply(lv["y"], lv["o"], lv["s"], lv["t"], td)}, inputs, {"out": R.randn(rng, (rows, 3))})


@pytest.mark.parametrize("rows", ROWS)
def test_inject_inv_node(rows):
    from puflow_amd.train_perop import InjectInvFn
    rng = _rng(3, rows)
    inputs = {"u": R.randn(rng, (rows, 3)), "s": R.randn(rng, (rows, 3), scale=0.3), "t": R.randn(rng, (rows, 3), scale=0.5)}
    _hold(f"inject_inv-rows{rows}", lambda lv: {"v": R.inject_inv(lv["u"], lv["s"], lv["t"])},
          lambda lv: {"v": InjectInvFn.apply(lv["u"], lv["s"], lv["t"])}, inputs, {"v": R.randn(rng, (rows, 3))})


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("td", [1, 2])
def test_couple_add_node(td, rows):
    from puflow_amd.train_perop import CoupleAddFn
    rng = _rng(4, td, rows)
    inputs = {"v": R.randn(rng, (rows, 3)), "o": R.randn(rng, (rows, 3 - td))}
    _hold(f"couple_add-td{td}-rows{rows}", lambda lv: {"out": R.couple_add(lv["v"], lv["o"], td)},
          lambda lv: {"out": CoupleAddFn.apply(lv["v"], lv["o"], td)}, inputs, {"out": R.randn(rng, (rows, 3))})


@pytest.mark.parametrize("M", [3, 771, 3 * 4099])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("mode", [0, 1])
def test_batch_sum_node(mode, B, M):
    from puflow_amd.train_perop import BatchSumFn
    rng = _rng(5, mode, B, M)
    inputs = {"x": R.randn(rng, (B, M // 3, 3))}
    _hold(f"batch_sum-mode{mode}-B{B}-M{M}", lambda lv: {"sum": R.batch_sum(lv["x"], mode)},
          lambda lv: {"sum": BatchSumFn.apply(lv["x"], mode)}, inputs, {"sum": R.randn(rng, (B,))})


# ------------------------------------------------------------------------------------------------ b. per-block fused nodes
@pytest.mark.parametrize("into", ["Winv", "ld", "both"])
@pytest.mark.parametrize("n", [1, 256])
@pytest.mark.parametrize("negative", [False, True])
def test_flow_params_node(negative, n, into):
    from puflow_amd.train_fusedfn import FlowParamsFn
    rng = _rng(6, negative, n)
    logs, _, W = _affine_params(5, negative)
    assert (float(torch.det(W)) < 0) == negative
    upstream = {k: w for k, w in (("Winv", R.randn(rng, (3, 3))), ("ld", R.randn(rng, (1,)))) if into in (k, "both")}

    def ref(lv):
        Winv, ld = R.flow_params(lv["W"], lv["logs"], float(n))
        return {"Winv": Winv, "ld": ld}

    def gpu(lv):
        Winv, ld = FlowParamsFn.apply(lv["W"], lv["logs"], float(n))
        return {"Winv": Winv, "ld": ld}

    _hold(f"flow_params-det{'-' if negative else '+'}-n{n}-into-{into}", ref, gpu, {"W": W, "logs": logs}, upstream)


BIG_ROWS = (1, 257, 65793)                     # 65 793 rows: past flow_grid's 256 workgroups, grid-stride loops + all 256 partials


@pytest.mark.parametrize("rows", BIG_ROWS)
@pytest.mark.parametrize("inv,td", [(0, 0), (1, 1), (1, 2)])
def test_flow_affine_node(inv, td, rows):
    """inv = 0 without o, inv = 1 with the coupling shift; the 15 parameter sums (dlogs, dbias, dM) are reduced in the kernel."""
    from puflow_amd.train_fusedfn import FlowAffineFn
    rng = _rng(7, inv, td, rows)
    logs, bias, W = _affine_params(7, negative=bool(td == 2))
    inputs = {"x": R.randn(rng, (rows, 3)), "logs": logs, "bias": bias, "M": torch.inverse(W).float().double() if inv else W}
    if inv:
        inputs["o"] = R.randn(rng, (rows, 3 - td))
    ref = lambda lv: {"y": R.flow_affine(lv["x"], lv.get("o"), td, lv["logs"].reshape(3), lv["bias"].reshape(3), lv["M"], inv)}
    gpu = lambda lv: {"y": FlowAffineFn.apply(lv["x"], lv.get("o"), td, lv["logs"], lv["bias"], lv["M"], inv)}
    _hold(f"flow_affine-inv{inv}-td{td}-rows{rows}", ref, gpu, inputs, {"y": R.randn(rng, (rows, 3))})


@pytest.mark.parametrize("with_dssum", [False, True])
@pytest.mark.parametrize("rows", BIG_ROWS)
@pytest.mark.parametrize("td", [1, 2])
def test_couple_inject2_node(td, rows, with_dssum):
    from puflow_amd.train_fusedfn import CoupleInject2Fn
    rng = _rng(8, td, rows)
    inputs = {"y": R.randn(rng, (rows, 3)), "o": R.randn(rng, (rows, 3 - td)), "s": R.randn(rng, (rows, 3), scale=0.3),
              "t": R.randn(rng, (rows, 3), scale=0.5)}
    upstream = {"out": R.randn(rng, (rows, 3))}
    if with_dssum:
        upstream["ssum"] = R.randn(rng, (1,))

    def gpu(lv):
        out, ssum = CoupleInject2Fn.apply(lv["y"], lv["o"], lv["s"], lv["t"], td)
        return {"out": out, "ssum": ssum}

    _hold(f"couple_inject2-td{td}-rows{rows}-dssum{int(with_dssum)}",
          lambda lv: {"out": R.couple_inject(lv["y"], lv["o"], lv["s"], lv["t"], td), "ssum": lv["s"].sum().reshape(1)}, gpu, inputs, upstream)


@pytest.mark.parametrize("Rr,T", [(Rr, T) for Rr in (1, 2, 3, 4, 16) for T in (1, 65)] + [(16, 4097)])      # 16 x 4097 > 65 536 rows
def test_inject_inv2_node(Rr, T):
    from puflow_amd.train_fusedfn import InjectInv2Fn
    rng = _rng(9, Rr, T)
    inputs = {"u": R.randn(rng, (T * Rr, 3)), "s": R.randn(rng, (T, 3), scale=0.3), "t": R.randn(rng, (T, 3), scale=0.5)}
    _hold(f"inject_inv2-R{Rr}-T{T}", lambda lv: {"v": R.inject_inv(lv["u"], lv["s"], lv["t"], Rr)},
          lambda lv: {"v": InjectInv2Fn.apply(lv["u"], lv["s"], lv["t"], Rr)}, inputs, {"v": R.randn(rng, (T * Rr, 3))})


MLP_CASES = R.mlp_cases()


@pytest.mark.parametrize("case", MLP_CASES, ids=[c["id"] for c in MLP_CASES])
def test_conditioner_mlp_node(case):
    """`mlp_fused` in its "cond" form (LinearA1D on cat[y[:, :td], c[row // cdiv]], csrc/train_mlp.hip) through cond_net_fused,
    which materialises the repeat for a replica count that is no power of two: against float64 lin_a1d."""
    from puflow_amd import train_ops as T
    from puflow_amd.train_fusedfn import _Lin
    assert {c["td"] for c in MLP_CASES} == {0, 1, 2} and {c["cdiv"] for c in MLP_CASES} == {1, 2, 3, 4, 8, 16}
    assert {c["cc"] for c in MLP_CASES} == {32, 64, 128} and {c["T"] for c in MLP_CASES} == {1, 17, 130}
    assert len({(c["td"], c["cdiv"]) for c in MLP_CASES}) == 18
    inputs, upstream, ref = R.mlp_problem(case)
    td, cdiv = case["td"], case["cdiv"]

    def gpu(lv):
        layers = [_Lin(lv["w0"]), _Lin(lv["w2"], lv["b2"]), _Lin(lv["w4"], lv["b4"])]
        c = lv["c"].view(1, case["T"], case["cc"])
        return {"out": T.cond_net_fused(layers, lv["y"] if td else None, c, td, cdiv).reshape(case["T"] * cdiv, -1)}

    _hold(case["id"], ref, gpu, inputs, upstream, kinks=True)


# ------------------------------------------------------------------------------------------------ c. the chain node
CHAIN_CASES = R.chain_cases()


def _chain_gpu(case):
    from puflow_amd.train_fusedfn import FlowChainFn

    def gpu(lv):
        prm = [lv[f"b{i}.{n}"] for i in range(case["nb"]) for n in R.PARAMS]
        res = FlowChainFn.apply(case["inv"], case["R"], float(case["N"]), tuple(case["ccs"]), lv["x"], lv["cflat"], lv["st"],
                                case["Bsz"], *prm)
        if case["inv"]:
            return {"out": res}
        return {"z": res[0], "logp": res[1]} if case["Bsz"] else {"z": res[0], "ssum": res[1], "ld": res[2]}
    return gpu


@pytest.mark.parametrize("case", CHAIN_CASES, ids=[c["id"] for c in CHAIN_CASES])
def test_flow_chain_node(case):
    """FlowChainFn.apply on synthetic parameter leaves, a cflat leaf and an st leaf - no network: outputs, dx, dcflat, dst and
    the eight parameter gradients of every block."""
    from puflow_amd._prof import profile_calls
    inputs, upstream, ref = R.chain_problem(case)
    with profile_calls() as prof:
        got = _hold(case["id"], ref, _chain_gpu(case), inputs, upstream, kinks=True)
    assert len(prof.events.get("pf_flowchain_fwd", [])) == 1 and len(prof.events.get("pf_flowchain_bwd", [])) == 1
    assert {"dx", "dcflat", "dst"} <= set(got) and sum(k.startswith("db") for k in got) == 8 * case["nb"]


def test_flow_chain_g_takes_the_image_f_packed():
    """f and then g on the same parameter tensors inside one begin_forward scope: the g chain finds the packed weight image of
    the f chain (PfFlowChain.img_ready, no second pack launch).  Outputs and every gradient equal the separate calls bit for bit."""
    from puflow_amd import train_state as S
    from puflow_amd.train_fusedfn import FlowChainFn
    B, N, Rr, nb = 3, 25, 4, 6
    f_case = dict(id="img-f", inv=0, nb=nb, ccs=list(R.MODEL_CCS), tds=list(R.MODEL_TDS), R=1, B=B, N=N, Bsz=B, seed=1)
    inputs, up_f, _ = R.chain_problem(f_case)
    rng = _rng(10)
    u0, wo = R.randn(rng, (B, N * Rr, 3)), R.randn(rng, (B, N * Rr, 3))

    def run(shared):
        lv = {k: v.to(device=DEV, dtype=torch.float32).requires_grad_(True) for k, v in inputs.items()}
        u = u0.to(device=DEV, dtype=torch.float32).requires_grad_(True)
        prm = [lv[f"b{i}.{n}"] for i in range(nb) for n in R.PARAMS]
        if shared:
            S.begin_forward(False, False)
        try:
            z, logp = FlowChainFn.apply(0, 1, float(N), R.MODEL_CCS, lv["x"], lv["cflat"], lv["st"], B, *prm)
            img = S._FC_IMG[torch.device(DEV, torch.cuda.current_device())][1] if shared else None
            out = FlowChainFn.apply(1, Rr, float(N), R.MODEL_CCS, u, lv["cflat"], lv["st"], 0, *prm)
            if shared:                                                      # the g call kept the f call's image
                assert S._FC_IMG[torch.device(DEV, torch.cuda.current_device())][1] is img
        finally:
            if shared:
                S.end_forward()
        loss = (z * up_f["z"].to(z)).sum() + 0.37 * logp.sum() + (out * wo.to(out)).sum()
        gs = torch.autograd.grad(loss, list(lv.values()) + [u])
        torch.cuda.synchronize()
        return [z.detach(), logp.detach(), out.detach()] + [g.detach() for g in gs]

    a, b = run(False), run(True)
    assert len(a) == len(b) == 3 + len(inputs) + 1
    for k, (ta, tb) in enumerate(zip(a, b)):
        assert torch.equal(ta, tb), k


def test_flow_chain_entry_point_declines_what_it_does_not_take():
    """pf_flowchain_fwd on the ABI: R = 3 and cc = 48 are not built (PF_ERR_UNSUPPORTED), rows that are no multiple of R are a shape
    error - all before any launch."""
    from puflow_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device=DEV)
    d = _lib.PfFlowChain()
    d.nb, d.rows, d.R, d.inv = 1, 48, 1, 1
    d.td[0], d.cc[0] = 1, 64
    for name in ("x", "pin", "mid", "o", "h1", "h2", "out", "ssum", "ld", "part", "img"):
        setattr(d, name, buf.data_ptr())
    d.counter = torch.zeros(1, dtype=torch.int32, device=DEV).data_ptr()
    d.R = 3
    assert lib.pf_flowchain_fwd(ctypes.byref(d), None) == _lib.PF_ERR_UNSUPPORTED
    d.R, d.rows = 2, 47
    assert lib.pf_flowchain_fwd(ctypes.byref(d), None) == _lib.PF_ERR_SHAPE
    d.R, d.rows, d.cc[0] = 1, 48, 48
    assert lib.pf_flowchain_fwd(ctypes.byref(d), None) == _lib.PF_ERR_UNSUPPORTED
    d.cc[0] = 64
    assert lib.pf_flowchain_fwd(ctypes.byref(d), None) == _lib.PF_ERR_NULL         # a complete shape: the parameters are missing
    torch.cuda.synchronize()
