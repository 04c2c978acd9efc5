"""The training kernels of the feature extractor and the interpolation-weight branch - the six EdgeConv units, the merge MLPs,
pf_dist_feature, the two BatchNorm MLPs, the K = 8 unit and FoldWuFn - in every tier and variant, against the float64
restatement of tests/extract_train_ref.py.  Every output, EVERY input gradient, every parameter gradient and the running
statistics are held, per tensor, to

    |gpu - ref64| <= 16 max|ref32 - ref64| + 2^-21 max|ref64|,

ref32 being the same restatement in float32 on the CPU with the float64 run's decisions (LeakyReLU / ReLU sides, pool argmax)
replayed: the bar never sees a kernel and measures rounding only (tests/test_extract_train_ref.py shows on the CPU that it
catches a swapped edge feature, a wrong slope, a missing BatchNorm mean term, ... in every case).  num_batches_tracked is
compared exactly.  Conv biases in front of a BatchNorm have a true gradient of zero; the kernels return rounding residue there,
held by the suite's residue rule (extract_train_ref.residue_ok).  `pytest -s` prints err / bar per case and quantity
(profiles/extract_train/accuracy.txt).

The fused EdgeConv unit forms the two products of its backward over the growth channels - dA = dy W (ec_bwdg16_kernel,
ec_bwdp_kernel) and dW = dy^T act (ec_dw3_kernel) - from split-bf16 operands: x = hi + mid, hi = bf16(x), mid = bf16(x - hi), the
mid mid product dropped; a product is off by up to 3 x 2^-16 of itself, where a float32 rounding is 2^-24.  The bars of its
gradients are therefore widened by extract_train_ref.format_widening - per tensor, the float64 restatement with exactly those two
products formed from split operands against the plain one, times two (the emulation is one draw of the rounded-off bits, a
kernel's another; the derivation stands next to the function): a term of the number format alone, never beyond the suite's
fused-against-un-fused bar of 2e-4 of the tensor's largest value.  Cases so widened print "[bf16]".  Outputs, running statistics
and every f32-product tier meet the unwidened bar at <= 0.25.  (These tests found the split TRUNCATING both parts: gradients 5 - 21
bars off for one unit, all towards zero, and past the 2e-4 ceiling for the first of the six chained units; both parts are now
rounded to nearest.)

Small cases carry the edges: their seeds (constants, chosen on the CPU) keep every float64 decision MIN_PREACT = 2e-5 clear,
which each test asserts first; nothing is masked.

Structural sizes, read from the launch functions:
  per-edge kernels (ec_fwd*, ec_bwdg*; pf_ec_dims)   tiles of 16 edges, one per wave, 4 per workgroup, at most EC_GRID = 512
                                                     workgroups: one sweep = 2048 tiles; a unit needs E % 16 == 0
  persistent kernels (ec_fwdp / ec_bwdp; pf_ecp_grid) 8 waves per workgroup, up to 4 tiles per wave, workgroups spread over the CUs
  weight-gradient chunks (ec_dw3_kernel)             128 / 256 / 512 edges for GT = 32 / 64 / 128, one workgroup per chunk
  dPQ (ec_pq_bwd*_kernel)                            grid-stride, at most 8192 workgroups of 256 threads
  BatchNorm MLPs (bnl_*; pf_bnmlp_train_*)           rows >= 16, tiles of 16 rows (the last partial), 4 per workgroup, at most
                                                     512 workgroups: one sweep = 32 768 rows; BNL_CHUNK = 256 rows per
                                                     weight-gradient chunk, staged in blocks of 32 rows
  statistics                                         per-workgroup partial sums into STAT_COPIES accumulators, the last one finalises
  per-op nodes (train_ops.hip)                       grid-stride, at most 8192 workgroups x 256 threads = 2 097 152 elements per
                                                     sweep; column statistics in at most 1024 chunks of >= 1024 rows
Small sizes: (1, 17) = 17 tiles (a workgroup with one tile; 272 edges = whole chunks + 16 for the 128- and 256-edge chunks),
(1, 33) = 33 tiles (528 edges = whole chunks + 16 for every chunk size), (3, 17) = three clouds.  Large cases are only for what
small ones cannot reach: (9, 257) = 2313 tiles (K = 8: (18, 257)), a BatchNorm MLP of 32 793 rows, one of each per-op node
past its sweep.  They cannot keep every decision clear: outputs whose float64 route passes a near decision get no upstream
gradient, and the bar of each tensor grows by max|ref64 - ref64 with every near decision taken the other way| (a first-order
estimate).  The rows of a per-row input gradient whose own route passes a near decision are left out like the outputs - a
BatchNorm MLP's masked rows, the points at either end of a unit's spoilt edges - and the CPU test keeps what is left of their
estimate under the unwidened bar; for row-reduced gradients it keeps the estimate under the suite's tier-against-tier bar
(extract_train_ref.large_ceiling; that file's docstring says why)."""
import pytest
import torch

import extract_train_ref as R
from kernel_trace import launched, ran

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = dict(dtype=torch.float32, device=DEV)

# Row-reduced quantities (weight / bias / gamma / beta gradients, running statistics) whose honest float32 summation needs more
# than the bar: case id -> {name: the terms it sums}.  Their bar grows by R.sum_envelope(terms), never beyond R.ceiling_of.
WIDENED = {}

_CACHE = {}


def _refs(key, make, need_clear=True):
    """(problem, r64, r32, rec): computed once per process, shared by the variants of a case, never written."""
    if key not in _CACHE:
        prob = make()
        _CACHE[key] = (prob,) + R.references(prob, need_clear)
    return _CACHE[key]


class _H:
    """Attribute holder with the names of an nn.Module (weight, bias, running_mean, ...) around leaves and buffers."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _bn(lv, state, name, bns):
    bn = _H(weight=lv[name + ".weight"], bias=lv[name + ".bias"], eps=R.EPS, momentum=R.MOMENTUM, name=name,
            running_mean=state[name + ".running_mean"].to(**F32).clone(), running_var=state[name + ".running_var"].to(**F32).clone(),
            num_batches_tracked=state[name + ".num_batches_tracked"].to(DEV).clone())
    bns.append(bn)
    return bn


def _unit(lv, state, bns, pfx=""):
    convs, t = [], 0
    while f"{pfx}convs.{t}.0.weight" in lv:
        q = f"{pfx}convs.{t}"
        convs.append([_H(weight=lv[q + ".0.weight"], bias=lv[q + ".0.bias"]), _bn(lv, state, q + ".1", bns)])
        t += 1
    return _H(convs=convs, conv_out=_H(weight=lv[pfx + "conv_out.weight"], bias=lv[pfx + "conv_out.bias"]))


def _stats(out, bns):
    for bn in bns:
        out[bn.name + ".running_mean"], out[bn.name + ".running_var"] = bn.running_mean.clone(), bn.running_var.clone()
    return out


def _fmt(key, prob, r64, rec, **form):
    """extract_train_ref.format_widening of a problem whose gradients pass the fused unit's split-bf16 products: once per problem."""
    key = ("fmt", key, tuple(sorted(form.items())))
    if key not in _CACHE:
        _CACHE[key] = R.format_widening(prob, r64, rec, **form)
    return _CACHE[key]


def _hold(cid, prob, refs, gpu, extra=None, det=False, fmt=None):
    """One case: the node on the GPU through flow_train_ref.grads, every tensor against the bar, the residues by their rule."""
    from puflow_amd import train_ops
    r64, r32 = refs
    bns = []
    old = train_ops.deterministic()
    train_ops.set_deterministic(det)
    try:
        fn = lambda lv: gpu(lv, bns)
        if prob["upstream"]:
            got = R.grads(fn, prob["inputs"], prob["upstream"], dtype=torch.float32, device=DEV)
        else:
            with torch.no_grad():
                got = fn({k: v.to(**F32) for k, v in prob["inputs"].items()})
        torch.cuda.synchronize()
    finally:
        train_ops.set_deterministic(old)
    assert set(got) == set(r64), set(got) ^ set(r64)
    for bn in bns:                                                      # exactly one more batch
        assert int(bn.num_batches_tracked) == int(prob["state"][bn.name + ".num_batches_tracked"]) + 1, bn.name
    widened = {k: terms(prob) for k, terms in WIDENED.get(cid, {}).items()}
    cmp, residues = R.hold(got, r64, r32, prob["kind"], widened, extra, prob, fmt)
    print("\n" + R.report(cid + ("[bf16]" if fmt else ""), cmp, widened), end="")
    for k in residues:
        assert R.residue_ok(got[k], prob["upstream"]), (cid, k, float(got[k].abs().max()))
    assert not R.failures(cmp), (cid, R.failures(cmp))
    return got


# ------------------------------------------------------------------------------------------------ a. EdgeConv units
def _unit_gpu(prob, variant):
    """The unit of a problem on the GPU in one of its variants -> fn(lv, bns) for _hold."""
    from puflow_amd import train_ops as T
    case = prob["case"]
    idx = prob["idx"].to(device=DEV, dtype=torch.int32).contiguous()
    pooling = case["pooling"]

    def gpu(lv, bns):
        p = _unit(lv, prob["state"], bns)
        x = lv["x"]
        res = None
        if variant == "perop":
            out = T.edgeconv_perop(p, x, idx, pooling)
        elif variant == "auto":                                         # edgeconv_train's own choice (the K = 8 unit)
            out = T.edgeconv_train(p, x, idx, pooling=pooling, csr=T.knn_csr(idx))
        elif variant == "atomics":
            out = T.edgeconv_train_fused(p, x, idx, pooling, None)
        elif variant in ("csr", "det"):
            out = T.edgeconv_train_fused(p, x, idx, pooling, T.knn_csr(idx))
        elif variant == "persistent":
            out = T.edgeconv_train_fused(p, x, idx, pooling, T.knn_csr(idx), True)
        elif variant == "prefold":
            pre = T.ec_prefold([p], x, case["K"])
            assert pre is not None and len(pre) == 1
            out = T.edgeconv_train_fused(p, x, idx, pooling, T.knn_csr(idx), prefold=pre[0])
        elif variant == "tap":
            res = T.edgeconv_train_fused(p, x, idx, pooling, T.knn_csr(idx), tap=True)
            assert isinstance(res, tuple) and res[1].data_ptr() == x.data_ptr()
            out = res[0]
        elif variant == "out":
            out = T.edgeconv_train_fused(p, x, idx, pooling, T.knn_csr(idx), out=(p.conv_out.weight, p.conv_out.bias))
        else:
            raise KeyError(variant)
        o = {"out": out}
        if case.get("tap"):
            o["tap"] = res[1] if res is not None else x * 1.0
        return _stats(o, bns)
    return gpu


def _unit_problem_of(case, need_clear=True):
    return _refs(("unit", case["base"], case["tap"]), lambda: R.unit_problem(case), need_clear)


UNIT_CASES = R.unit_cases()


@pytest.mark.parametrize("case", UNIT_CASES, ids=[c["id"] for c in UNIT_CASES])
def test_edgeconv_unit(case):
    """Every unit shape of the network at the small sizes, pooled and un-pooled, and every variant of the fused unit on a narrow
    and a wide shape: per-op tier, float atomics (csr=None), transposed lists, persistent, prefold=, tap=True with a second
    consumer's gradient, out=(W, b), the deterministic switch.  The variants of a case share its references."""
    from puflow_amd import train_ops as T
    prob, r64, r32, rec = _unit_problem_of(case)
    assert rec.clear()
    v = case["variant"]
    E = case["B"] * case["N"] * case["K"]
    fmt = _fmt(("unit", case["base"], case["tap"]), prob, r64, rec)          # every fused variant: gradients through split-bf16 products
    if case["unit"] == "k8":
        # edgeconv_train decides: the fused unit where E % 16 == 0, else the per-op path - held as well
        fused = E % 16 == 0
        p = _unit({k: val.to(**F32) for k, val in prob["inputs"].items()}, prob["state"], [])
        assert T._ec_fused_supported(p, prob["inputs"]["x"], prob["idx"], False) == fused
        got, names = launched(lambda: _hold(case["id"], prob, (r64, r32), _unit_gpu(prob, "auto"), fmt=fmt if fused else None))
        assert (ran(names, "ec_fwd") and ran(names, "ec_dw")) == fused, sorted(names)
        assert ran(names, "bn_apply_kernel") != fused, sorted(names)     # the per-op BatchNorm ran exactly when the unit declined
        return
    if v == "persistent":
        assert T._PERSIST
        got, names = launched(lambda: _hold(case["id"], prob, (r64, r32), _unit_gpu(prob, v), fmt=fmt))
        # a residency check that wrongly says "does not fit" would fall back to the per-layer kernels
        assert ran(names, "ec_fwdp_kernel") and ran(names, "ec_bwdp_kernel"), sorted(names)
        assert T._sync_words(torch.device(DEV, torch.cuda.current_device())).tolist() == [0, 0, 0, 0]
        T.check_persist_status()
        return
    if v == "prefold":
        got, names = launched(lambda: _hold(case["id"], prob, (r64, r32), _unit_gpu(prob, v), fmt=fmt))
        assert ran(names, "ec_fold_batch_kernel") and not ran(names, "ec_fold_kernel"), sorted(names)
        return
    got, names = launched(lambda: _hold(case["id"], prob, (r64, r32), _unit_gpu(prob, v), det=(v == "det"),
                                        fmt=None if v == "perop" else fmt))
    if v == "perop":
        assert not ran(names, "ec_fwd") and ran(names, "bn_apply_kernel"), sorted(names)
    else:
        assert ran(names, "ec_fwd") and not ran(names, "ec_fwdp_kernel") and not ran(names, "bn_apply_kernel"), sorted(names)
        assert ran(names, "ec_pq_bwd_csr_kernel") == (v != "atomics"), sorted(names)
        assert ran(names, "csr_sort_kernel") == (v == "det"), sorted(names)


LARGE_UNITS = R.large_unit_cases()


@pytest.mark.parametrize("case", LARGE_UNITS, ids=[c["id"] for c in LARGE_UNITS])
def test_edgeconv_unit_past_one_grid_sweep(case):
    """2313 tiles: more than the 2048 of one sweep of the per-edge kernels, the last round partial; 73 - 290 weight-gradient
    chunks, the last partial.  Masked upstream, flip-widened bar (see the file's docstring)."""
    prob, r64, r32, rec, extra = R.large_references(case)
    pools, kinks = rec.shares()
    assert pools <= R.MAX_POOL_SHARE and kinks <= R.MAX_KINK_SHARE, (pools, kinks)
    print(f"\n{case['id']}: masked outputs {prob['masked']} (no upstream gradient), points left out of dx {prob['skipped']} of "
          f"{case['B'] * case['N']}, near pools {pools:.2e}, near kinks {kinks:.2e}", end="")
    _hold(case["id"], prob, (r64, r32), _unit_gpu(prob, "csr"), extra=extra, fmt=_fmt(case["id"], prob, r64, rec))


# ------------------------------------------------------------------------------------------------ b. BatchNorm MLPs
def _mlp(lv, state, bns, widths, form):
    def conv(a, co, ci):
        if f"{a}.weight" in lv:
            return _H(weight=lv[f"{a}.weight"], bias=lv[f"{a}.bias"])
        return _H(weight=torch.zeros((co, ci, 1, 1), **F32), bias=torch.zeros((co,), **F32))      # shapes only (sum / last)
    return [conv(0, widths[1], widths[0]), _bn(lv, state, "1", bns), None, conv(3, widths[2], widths[1]), _bn(lv, state, "4", bns),
            None, conv(6, widths[3], widths[2])]


def _bnmlp_gpu(prob, tier):
    from puflow_amd import train_ops as T
    form = prob["case"]["form"]
    widths = (10, 64, 64, 128) if form in ("distance", "last") else (256, 128, 64, 32)

    def gpu(lv, bns):
        mlp = _mlp(lv, prob["state"], bns, widths, form)
        if tier == "perop":
            out = T._mlp_bn(mlp, torch.cat([lv["xa"], lv["xb"]], dim=1) if form == "weight" else lv["xa"])
        elif form == "distance":
            out = T.bnmlp_fused(mlp, lv["xa"])
        elif form == "weight":
            out = T.bnmlp_fused(mlp, lv["xa"], lv["xb"])
        elif form == "sum":
            out = T.bnmlp_fused(mlp, lv["xa"], lv["xb"], sum_inputs=True)
        else:
            out = T.bnmlp_fused(mlp, lv["xa"], last=(lv["lastW"], lv["lastb"]))
        return _stats({"out": out}, bns)
    return gpu


BNMLP_CASES = R.bnmlp_cases()


@pytest.mark.parametrize("case", BNMLP_CASES, ids=[c["id"] for c in BNMLP_CASES])
def test_batchnorm_mlp(case):
    """bnmlp_fused in its four forms - distance (10 -> 64 -> 64 -> 128), weight on two inputs, sum_inputs=True, last=(W, b) - at
    16, 17, 40, 255, 257 and 264 rows (partial tiles, partial 32-row blocks, a partial second chunk), and _mlp_bn, the per-op
    tier, in the two forms it has.  Running means near the batch means: they are the pivots of the fused statistics."""
    prob, r64, r32, rec = _refs(case["id"], lambda: R.bnmlp_problem(case))
    assert rec.clear()
    got, names = launched(lambda: _hold(case["id"], prob, (r64, r32), _bnmlp_gpu(prob, "fused")))
    assert ran(names, "bnl_fwd_kernel") and ran(names, "bnl_dw_kernel") and not ran(names, "bn_apply_kernel"), sorted(names)
    assert ran(names, "bnl_sum_kernel") == (case["form"] == "sum"), sorted(names)
    if case["form"] in ("distance", "weight"):
        _hold(case["id"] + "-perop", prob, (r64, r32), _bnmlp_gpu(prob, "perop"))


@pytest.mark.parametrize("form", ["weight", "sum"])
def test_batchnorm_mlp_past_one_grid_sweep(form):
    """32 793 rows: 2050 tiles, past 512 workgroups x 4 tiles, the last tile with 9 rows; 129 weight-gradient chunks."""
    case = dict(id=f"bnmlp-{form}-large", form=form, rows=R.BNMLP_LARGE_ROWS, large=True)
    prob, r64, r32, rec, extra = R.large_references(case)
    _, kinks = rec.shares()
    assert kinks <= R.MAX_KINK_SHARE, kinks
    print(f"\n{case['id']}: masked rows {prob['masked']} (no upstream gradient; left out of dxa / dxb too), near kinks {kinks:.2e}", end="")
    _hold(case["id"], prob, (r64, r32), _bnmlp_gpu(prob, "fused"), extra=extra)


@pytest.mark.parametrize("o,k6,ko", [(128, 64, 137), (16, 5, 7)])
def test_fold_wu_node(o, k6, ko):
    """FoldWuFn alone against the float64 products and their chain rule: the model's shape and a small odd one."""
    from puflow_amd.train_fusedfn import FoldWuFn
    prob = R.fold_problem(o, k6, ko)
    r64, r32, _ = R.references(prob)

    def gpu(lv, bns):
        return dict(zip(("W6f", "b6f", "Wof", "bof"), FoldWuFn.apply(lv["W0"], lv["b0"], lv["W6"], lv["b6"], lv["Wout"], lv["bout"])))

    _hold(prob["case"]["id"], prob, (r64, r32), gpu)


# ------------------------------------------------------------------------------------------------ c. merge MLPs, distance feature
MERGE_CASES = R.merge_cases()


@pytest.mark.parametrize("case", MERGE_CASES, ids=[c["id"] for c in MERGE_CASES])
def test_merge_mlp(case):
    """mlp_fused in its merge form (Linear, ReLU, Linear without bias) and the per-op composition for cc in {32, 64, 128} and T in
    {1, 17, 130}; MergeBatchFn with the model's six widths at T in {17, 130}."""
    from puflow_amd import train_ops as T
    from puflow_amd.train_fusedfn import MergeBatchFn, _Lin, mlp_fused
    prob, r64, r32, rec = _refs(case["id"], lambda: R.merge_problem(case))
    assert rec.clear()
    n = len(case["ccs"])

    def fused(lv, bns):
        if n == 1:
            return {"c0": mlp_fused(None, lv["h0"], 0, 1, (0.0,), [_Lin(lv["m0.conv1.weight"], lv["m0.conv1.bias"]), _Lin(lv["m0.conv2.weight"])])}
        mp = []
        for i in range(n):
            mp += [lv[f"m{i}.conv1.weight"], lv[f"m{i}.conv1.bias"], lv[f"m{i}.conv2.weight"]]
        flat = MergeBatchFn.apply(n, *[lv[f"h{i}"] for i in range(n)], *mp)
        out, off = {}, 0
        for i, (_, co) in enumerate(case["ccs"]):
            out[f"c{i}"] = flat[off:off + case["T"] * co].view(case["T"], co)
            off += case["T"] * co
        assert off == flat.numel()
        return out

    def perop(lv, bns):
        return {f"c{i}": T.linear(T.ActFn.apply(T.linear(lv[f"h{i}"], lv[f"m{i}.conv1.weight"], lv[f"m{i}.conv1.bias"]), 0.0),
                                  lv[f"m{i}.conv2.weight"]) for i in range(n)}

    got, names = launched(lambda: _hold(case["id"], prob, (r64, r32), fused))
    assert ran(names, "mlp_fwd_kernel") and ran(names, "mlp_dw_kernel"), sorted(names)
    if n == 1:
        _hold(case["id"] + "-perop", prob, (r64, r32), perop)


@pytest.mark.parametrize("B,N", [(1, 16), (1, 17), (1, 257)])
def test_dist_feature(B, N):
    """pf_dist_feature: [x_i, x_j, x_i - x_j, |x_i - x_j|] per edge of the 8-neighbour lists (no gradient: inputs only)."""
    from puflow_amd import _lib
    from puflow_amd.train_state import _stream
    prob = R.dist_problem(B, N)
    r64, r32, _ = R.references(prob)
    idx8 = prob["idx"].to(device=DEV, dtype=torch.int32).contiguous()

    def gpu(lv, bns):
        xyz = lv["xyz"].contiguous()
        fd = torch.full((B * N * 8, 10), float("nan"), **F32)
        _lib.check(_lib.load().pf_dist_feature(xyz.data_ptr(), idx8.data_ptr(), B, N, 8, fd.data_ptr(), _stream()), "pf_dist_feature")
        return {"fd": fd}

    _hold(prob["case"]["id"], prob, (r64, r32), gpu)


# ------------------------------------------------------------------------------------------------ d. per-op nodes on their own
def _node(cid, inputs, upstream, ref, gpu):
    prob = dict(kind="node", case=dict(id=cid), inputs=inputs, upstream=upstream, state={}, ref=lambda lv, dec=None, bug=(): ref(lv, dec))
    r64, r32, _ = R.references(prob)
    return _hold(cid, prob, (r64, r32), lambda lv, bns: gpu(lv))


SWEEP = R.SWEEP                                 # elements one sweep of a grid-stride per-op kernel covers
ROWS = (1, 255, 257)


@pytest.mark.parametrize("rows", ROWS + (1024 * 1024 + 1025,))
def test_linear_node(rows):
    """LinearFn: y = x W^T + b, dx, dW, db.  The last size: the bias gradient's column sums past their 1024 chunks of 1024 rows."""
    from puflow_amd.train_perop import LinearFn
    big = rows > 1000
    cin, cout = (4, 4) if big else (45, 33)
    rng = R._rng(41, rows)
    inputs = {"x": R.randn(rng, (rows, cin)), "W": R.randn(rng, (cout, cin), scale=cin ** -0.5), "b": R.randn(rng, (cout,), scale=0.1)}
    upstream = {"y": R.randn(rng, (rows, cout))}
    _node(f"linear-rows{rows}", inputs, upstream, lambda lv, dec: {"y": torch.nn.functional.linear(lv["x"], lv["W"], lv["b"])},
          lambda lv: {"y": LinearFn.apply(lv["x"], lv["W"], lv["b"])})


@pytest.mark.parametrize("rows,C", R.BN_NODE_SIZES)
def test_bn_lrelu_node(rows, C):
    """BnLreluFn (rows >= 2): two-pass statistics, the running update, dx, dgamma, dbeta.  32 793 x 64 > one sweep of the apply
    kernels; 1 049 601 rows > 1024 statistics chunks of 1024 rows.  Large sizes: elements within MIN_PREACT of the kink get no
    upstream gradient; their share stays <= 1e-4 (tests/test_extract_train_ref.py asserts the input conditions on the CPU too)."""
    from puflow_amd.train_perop import BnLreluFn
    prob = R.bn_node_problem(rows, C)
    assert prob["near_share"] <= R.MAX_KINK_SHARE if prob["large"] else prob["clear"]
    r64, r32, rec = R.references(prob)
    extra = R.flip_widening(prob, r64, rec) if prob["large"] else None
    state = prob["state"]

    def gpu(lv, bns):
        bn = _bn({"bn.weight": lv["bn.weight"], "bn.bias": lv["bn.bias"]}, state, "bn", [])
        y = BnLreluFn.apply(lv["x"], bn.weight, bn.bias, bn.running_mean, bn.running_var, 0.05, R.EPS, R.MOMENTUM)
        return {"y": y, "bn.running_mean": bn.running_mean.clone(), "bn.running_var": bn.running_var.clone()}

    _hold(prob["case"]["id"], prob, (r64, r32), gpu, extra=extra)


@pytest.mark.parametrize("n", R.ACT_NODE_SIZES)
@pytest.mark.parametrize("slope", [0.0, 0.05])
def test_act_node(slope, n):
    from puflow_amd.train_perop import ActFn
    prob = R.act_node_problem(slope, n)
    assert prob["clear"]
    r64, r32, _ = R.references(prob)
    _hold(prob["case"]["id"], prob, (r64, r32), lambda lv, bns: {"y": ActFn.apply(lv["x"], slope)})


def _cloud(rng, B, N, C, K):
    xyz = R.patches(rng, B, N)
    return R.knn(xyz, K), R.randn(rng, (B, N, C))


@pytest.mark.parametrize("B,N,C", [(1, 1, 5), (1, 255, 5), (1, 257, 5), (3, 17, 64), (1, 2049, 64)])
def test_edge_feature_node(B, N, C):
    """EdgeFeatureFn: cat[x_i, x_j, x_j - x_i] and its scatter-add backward (float atomics: reduced in another order every run).
    2049 x 16 edges x 64 channels: past one sweep."""
    from puflow_amd.train_perop import EdgeFeatureFn
    K = min(16, N)
    rng = R._rng(53, B, N, C)
    idx, x = _cloud(rng, B, N, C, K)
    idx32 = idx.to(device=DEV, dtype=torch.int32).contiguous()
    assert B * N * K * C > SWEEP or N < 2049
    _node(f"edge_feature-{B}x{N}x{C}", {"x": x}, {"f": R.randn(rng, (B * N * K, 3 * C))},
          lambda lv, dec: {"f": R.edge_feature(lv["x"], idx)}, lambda lv: {"f": EdgeFeatureFn.apply(lv["x"], idx32)})


@pytest.mark.parametrize("T,C,K", R.MAXPOOL_NODE_SIZES)
def test_maxpool_node(T, C, K):
    """MaxPoolKFn through the float64 argmax (inputs: every pool gap MIN_PREACT clear by construction).  (2049, 64, 16): T K C past
    one sweep of maxpool_bwd_kernel; (16385, 128, 2): T C past one sweep of maxpool_fwd_kernel, which also writes the argmax."""
    from puflow_amd.train_perop import MaxPoolKFn
    prob = R.maxpool_node_problem(T, C, K)
    assert prob["clear"]
    assert T < 2049 or T * K * C > SWEEP
    assert T < 16385 or T * C > SWEEP
    r64, r32, _ = R.references(prob)
    _hold(prob["case"]["id"], prob, (r64, r32), lambda lv, bns: {"o": MaxPoolKFn.apply(lv["y"], K)})


@pytest.mark.parametrize("B,N,C", [(1, 1, 3), (1, 255, 3), (1, 257, 20), (1, 2049, 128)])
def test_gather_rows_node(B, N, C):
    from puflow_amd.train_perop import GatherRowsFn
    K = min(8, N)
    rng = R._rng(61, B, N, C)
    idx, z = _cloud(rng, B, N, C, K)
    idx32 = idx.to(device=DEV, dtype=torch.int32).contiguous()
    assert B * N * K * C > SWEEP or N < 2049
    _node(f"gather_rows-{B}x{N}x{C}", {"z": z}, {"g": R.randn(rng, (B * N * K, C))},
          lambda lv, dec: {"g": lv["z"][torch.arange(B).view(B, 1, 1), idx].reshape(B * N * K, C)},
          lambda lv: {"g": GatherRowsFn.apply(lv["z"], idx32)})


@pytest.mark.parametrize("N,C,Rr", [(1, 3, 4), (255, 3, 4), (257, 64, 3), (8201, 256, 2)])
def test_repeat_rows_node(N, C, Rr):
    from puflow_amd.train_perop import RepeatRowsFn
    rng = R._rng(67, N, C, Rr)
    assert N * C > SWEEP or N < 8201
    _node(f"repeat_rows-N{N}-C{C}-R{Rr}", {"c": R.randn(rng, (1, N, C))}, {"r": R.randn(rng, (1, N * Rr, C))},
          lambda lv, dec: {"r": torch.repeat_interleave(lv["c"], Rr, dim=1)}, lambda lv: {"r": RepeatRowsFn.apply(lv["c"], Rr)})


# ------------------------------------------------------------------------------------------------ e. composed
COMPOSED = R.composed_cases()


# _features never reads _FOLD_WU: it runs once, under the default; the interpolation branch runs with the fold on and off
COMPOSED_RUNS = [(c, f) for c in COMPOSED for f in ((True,) if c["part"] == "features" else (True, False))]


@pytest.mark.parametrize("case,fold", COMPOSED_RUNS, ids=[f"{c['id']}-{'foldwu' if f else 'nofold'}" for c, f in COMPOSED_RUNS])
def test_features_and_interp_weights_on_the_model(case, fold):
    """train_ops._features (once: the fold does not reach it) and train_ops._interp_weights with _FOLD_WU on and off, on a
    PointInterpFlow with the problem's parameters, against `features` / `interp_logits` (the plain form: the truth for the folded
    path too) in float64."""
    from puflow_amd import train_ops as T
    from puflow_amd.interpflow import PointInterpFlow
    prob, r64, r32, rec = _refs(case["id"], lambda: R.composed_problem(case))
    assert rec.clear()
    B, N = case["B"], case["N"]
    net = PointInterpFlow(3)
    sd = {k: v.float() for k, v in prob["inputs"].items()}
    sd.update({k: (v.float() if v.is_floating_point() else v) for k, v in prob["state"].items()})
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected
    net = net.to(DEV).train()
    xyz = prob["xyz"].to(**F32).contiguous()
    idx16 = prob["idx16"].to(device=DEV, dtype=torch.int32).contiguous()
    old = T._FOLD_WU
    T._FOLD_WU = fold
    try:
        idx8, csr16, csr8 = T._neighbour_lists(idx16)
        pre = T.ec_prefold(list(net.feat_convs), xyz, 16)
        assert pre is not None
        f_features = lambda: T._features(net, xyz, idx16, csr16, pre)
        f_interp = lambda: T._interp_weights(net, xyz, idx8, csr8)

        def step():
            if case["part"] == "features":
                cs, _ = f_features()
                outs = {f"c{i}": c for i, c in enumerate(cs)}
            else:
                outs = {"w": f_interp()}
            loss = sum((outs[k] * prob["upstream"][k].to(**F32).view_as(outs[k])).sum() for k in outs)
            loss.backward()
            return outs
        outs, names = launched(step)
    finally:
        T._FOLD_WU = old
    params = dict(net.named_parameters())
    got = {k: v.detach() for k, v in outs.items()}
    for k in prob["inputs"]:
        got["d" + k] = params[k].grad if params[k].grad is not None else torch.zeros_like(params[k])
    bufs = dict(net.named_buffers())
    for k, v in prob["state"].items():
        if k.endswith("num_batches_tracked"):
            assert int(bufs[k]) == int(v) + 1, k
        else:
            got[k] = bufs[k].detach().clone()
    assert set(got) == set(r64), set(got) ^ set(r64)
    cid = case["id"] if case["part"] == "features" else f"{case['id']}-{'foldwu' if fold else 'nofold'}"
    fused_unit = case["part"] == "features" or (B * N * 8) % 16 == 0       # else the K = 8 unit took the per-op path: f32 products
    # (the folded path forms dW0 from the fused unit's conv_out gradient: its format term is that of the folded restatement)
    form = dict(folded=True) if (fold and case["part"] == "interp") else {}
    fmt = _fmt(case["id"], prob, r64, rec, **form) if fused_unit else None
    cmp, residues = R.hold(got, r64, r32, "composed", fmt=fmt)
    print("\n" + R.report(cid + ("[bf16]" if fmt else ""), cmp), end="")
    for k in residues:
        assert R.residue_ok(got[k], prob["upstream"]), (cid, k, float(got[k].abs().max()))
    assert not R.failures(cmp), (cid, R.failures(cmp))
    if case["part"] == "features":
        assert ran(names, "ec_fwd") and ran(names, "mlp_fwd_kernel") and ran(names, "ec_pq_bwd_csr_kernel"), sorted(names)
    else:
        folded = fold and (B * N * 8) % 16 == 0                     # the fused K = 8 unit (and with it the fold) needs whole tiles
        assert ran(names, "fold_wu_fwd_kernel") == folded and ran(names, "fold_wu_bwd_kernel") == folded, sorted(names)
        assert ran(names, "bnl_sum_kernel") == folded and ran(names, "dist_feature_kernel"), sorted(names)
