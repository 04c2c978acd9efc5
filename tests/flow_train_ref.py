"""Float64 restatement of the discrete model's flow blocks in train mode.  TEST INFRASTRUCTURE ONLY: torch on the CPU, no
import of the library.

The mathematics is that of `oracle/ref_cpu.py::flow_block_forward`, `flow_block_inverse` and `lin_a1d` (pinned to the
reference's goldens by tests/test_oracle_golden.py; tests/test_flow_train_ref.py ties this file to them), restated so that
  - the coupling's split `td` is read from the first layer's shape (the chain kernel does the same) instead of the block's parity,
  - the injector scale and shift may be given as a leaf `st` [2 nb, T, 3] (what FlowChainFn takes), and
  - one deliberate error (`bug`) can be switched on: tests/test_flow_train_ref.py shows that the bar below notices each of them.
Everything runs in the dtype of its inputs: float64 for the reference, float32 for the bar
    |gpu - ref64| <= 16 max|ref32 - ref64| + 2^-21 max|ref64|          per compared tensor,
i.e. sixteen times the float32 rounding of the same expressions (another summation order over up to 65 793 rows, f32-MFMA
accumulation order, hardware exp against libm) with a floor of a quarter of a float32 ulp of the tensor's largest value for
tensors that float32 happens to reproduce exactly."""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

Tensor = torch.Tensor
LOG2PI = float(math.log(2 * math.pi))
HDIM = 64
MODEL_CCS = (32, 64, 128, 128, 128, 128)         # the model's conditioning channels and splits per block
MODEL_TDS = (1, 2, 1, 2, 1, 2)
PARAMS = ("logs", "bias", "W", "w0", "w2", "b2", "w4", "b4")          # FlowChainFn's order per block
_KEY = {"logs": "actnorm.logs", "bias": "actnorm.bias", "W": "permutate1.permutater.W",
        "w0": "coupling1.bias_net.layers.0.weight", "w2": "coupling1.bias_net.layers.2.weight",
        "b2": "coupling1.bias_net.layers.2.bias", "w4": "coupling1.bias_net.layers.4.weight",
        "b4": "coupling1.bias_net.layers.4.bias"}
BUGS = ("no_logdet", "ssum_sign", "td_swapped", "no_reverse", "exp_sign", "cond_row", "ds_rm1", "dw_no_inv", "slope0")
MIN_PREACT = 2e-5                                # smallest |hidden pre-activation| a case's seed must leave (float64 run)

_REC: Optional[List[float]] = None               # min_preactivation's recorder


def _f32(v, dtype) -> Tensor:
    """Values rounded to float32 first: the float64 and the float32 runs, and the GPU, then start from the same numbers."""
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dtype)


def randn(rng, shape, dtype=torch.float64, scale: float = 1.0) -> Tensor:
    return _f32(rng.standard_normal(shape) * scale, dtype)


def _lin_a1d_init(sd, rng, pfx: str, cin: int, cout: int, dtype) -> None:
    """Fan-in scaled, as weights.synth_state_dict("unit")."""
    sd[pfx + ".layers.0.weight"] = _f32(rng.standard_normal((HDIM, cin)) / np.sqrt(cin), dtype)
    sd[pfx + ".layers.2.weight"] = _f32(rng.standard_normal((HDIM, HDIM)) / np.sqrt(HDIM), dtype)
    sd[pfx + ".layers.2.bias"] = _f32(rng.standard_normal((HDIM,)) * 0.1, dtype)
    sd[pfx + ".layers.4.weight"] = _f32(rng.standard_normal((cout, HDIM)) * (0.4 / np.sqrt(HDIM)), dtype)
    sd[pfx + ".layers.4.bias"] = _f32(rng.standard_normal((cout,)) * 0.05, dtype)


def make_blocks(nb: int, ccs: Sequence[int], tds: Sequence[int], seed: int, dtype=torch.float64) -> Dict[str, Tensor]:
    """State-dict fragment of nb flow blocks (keys of oracle/ref_cpu.py).  logs ~ 0.3 N, bias ~ 0.2 N, W = orthogonal x column
    scales in [0.7, 1.4] with det W > 0 in the even blocks and, its first row negated, det W < 0 in the odd ones."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd: Dict[str, Tensor] = {}
    for i in range(nb):
        p = f"flow_blocks.{i}"
        cc, td = int(ccs[i]), int(tds[i])
        sd[p + ".actnorm.logs"] = _f32(rng.standard_normal((1, 1, 3)) * 0.3, dtype)
        sd[p + ".actnorm.bias"] = _f32(rng.standard_normal((1, 1, 3)) * 0.2, dtype)
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        W = q * rng.uniform(0.7, 1.4, (1, 3))
        if np.linalg.det(W) < 0:
            W[0] = -W[0]
        if i % 2 == 1:
            W[0] = -W[0]
        sd[p + ".permutate1.permutater.W"] = _f32(W, dtype)
        sd[p + ".permutate2.permutater.direct_idx"] = torch.tensor([2, 1, 0], dtype=torch.int64)
        sd[p + ".permutate2.permutater.inverse_idx"] = torch.tensor([2, 1, 0], dtype=torch.int64)
        _lin_a1d_init(sd, rng, p + ".coupling1.bias_net", td + cc, 3 - td, dtype)
        _lin_a1d_init(sd, rng, p + ".coupling2.bias_net", cc, 3, dtype)
        _lin_a1d_init(sd, rng, p + ".coupling2.scale_net", cc, 3, dtype)
    return sd


def block_params(sd, i: int) -> List[Tensor]:
    """Block i's eight parameters in FlowChainFn's order."""
    return [sd[f"flow_blocks.{i}.{_KEY[n]}"] for n in PARAMS]


# ---------------------------------------------------------------------------------------------------- the blocks
def lin_a1d(sd, pfx: str, h: Tensor, slope: float = 0.01) -> Tensor:
    """LinearA1D (ref_cpu.lin_a1d): Linear(no bias) -> LReLU(.01) -> Linear -> LReLU -> Linear."""
    z = F.linear(h, sd[pfx + ".layers.0.weight"])
    _note(z)
    z = F.linear(F.leaky_relu(z, slope), sd[pfx + ".layers.2.weight"], sd[pfx + ".layers.2.bias"])
    _note(z)
    return F.linear(F.leaky_relu(z, slope), sd[pfx + ".layers.4.weight"], sd[pfx + ".layers.4.bias"])


def _note(z: Tensor) -> None:
    if _REC is not None and z.numel():
        _REC.append(float(z.detach().abs().min()))


def _td(sd, i: int, c: Tensor) -> int:
    return int(sd[f"flow_blocks.{i}.coupling1.bias_net.layers.0.weight"].shape[1]) - int(c.shape[-1])


def _couple(sd, i: int, p: Tensor, c: Tensor, sign: float, bug) -> Tensor:
    """cat[h1, h2 + sign net(cat[h1, c])] with h1 = p[..., :td]  (coupling.py:55-58, 82-85, 114-118)."""
    td = _td(sd, i, c)
    slope = 0.0 if "slope0" in bug else 0.01
    net = f"flow_blocks.{i}.coupling1.bias_net"
    if "td_swapped" in bug:                       # the untouched coordinates taken from the other end
        h2, h1 = p[..., :3 - td], p[..., 3 - td:]
        return torch.cat([h2 + sign * lin_a1d(sd, net, torch.cat([h1, c], dim=-1), slope), h1], dim=-1)
    h1, h2 = p[..., :td], p[..., td:]
    return torch.cat([h1, h2 + sign * lin_a1d(sd, net, torch.cat([h1, c], dim=-1), slope)], dim=-1)


def _st(sd, i: int, c: Tensor, st, bug):
    """Injector scale and shift [B, N, 3] of block i: the leaf's rows, or the two nets on c."""
    if st is not None:
        return st[2 * i].reshape(c.shape[0], c.shape[1], 3), st[2 * i + 1].reshape(c.shape[0], c.shape[1], 3)
    slope = 0.0 if "slope0" in bug else 0.01
    pf = f"flow_blocks.{i}"
    return lin_a1d(sd, pf + ".coupling2.scale_net", c, slope), lin_a1d(sd, pf + ".coupling2.bias_net", c, slope)


def block_f(sd, i: int, p: Tensor, c: Tensor, st=None, bug=()):
    """ref_cpu.flow_block_forward -> (p', ld = (sum(logs) + log|det W|) N, sum(s))."""
    pf = f"flow_blocks.{i}"
    N = p.shape[1]
    logs, bias, W = sd[pf + ".actnorm.logs"], sd[pf + ".actnorm.bias"], sd[pf + ".permutate1.permutater.W"]
    p = p * torch.exp(logs) + bias                                   # normalize.py:34
    ld = torch.sum(logs) * N
    p = torch.einsum("ij,bnj->bni", W, p)                            # permutate.py:118
    if "no_logdet" not in bug:
        ld = ld + torch.slogdet(W)[1] * N
    p = _couple(sd, i, p, c, -1.0, bug)
    if "no_reverse" not in bug:
        p = p[:, :, sd[pf + ".permutate2.permutater.direct_idx"]]    # permutate.py:77
    s, t = _st(sd, i, c, st, bug)
    p = (p - t) * torch.exp(s if "exp_sign" in bug else -s)          # coupling.py:136
    return p, ld, torch.sum(s)


def block_g(sd, i: int, z: Tensor, c: Tensor, s: Tensor, t: Tensor, bug=()) -> Tensor:
    """ref_cpu.flow_block_inverse with s, t and c already one row per row of z."""
    pf = f"flow_blocks.{i}"
    z = z * torch.exp(-s if "exp_sign" in bug else s) + t            # coupling.py:149
    if "no_reverse" not in bug:
        z = z[:, :, sd[pf + ".permutate2.permutater.inverse_idx"]]
    z = _couple(sd, i, z, c, 1.0, bug)
    W = sd[pf + ".permutate1.permutater.W"]
    Winv = torch.inverse(W.detach() if "dw_no_inv" in bug else W)
    z = torch.einsum("ij,bnj->bni", Winv, z)                         # permutate.py:123-124
    logs, bias = sd[pf + ".actnorm.logs"], sd[pf + ".actnorm.bias"]
    return (z - bias) * torch.exp(-logs)                             # normalize.py:41


def _nblocks(sd) -> int:
    nb = 0
    while f"flow_blocks.{nb}.actnorm.logs" in sd:
        nb += 1
    return nb


def chain_f(sd, x: Tensor, cs: List[Tensor], st=None, bug=()):
    """PointInterpFlow.f + log_prob (ref_cpu.flow_f / log_prob) over the blocks of sd.  x [B, N, 3], cs[i] [B, N, cc_i]
    -> (z, ssum [nb] = sum(s_i), ld [nb], logp = -(sum log N(z) / B + sum_i ld_i - sum_i ssum_i / B))."""
    B = x.shape[0]
    p, lds, ssums = x, [], []
    for i in range(_nblocks(sd)):
        p, ld, ss = block_f(sd, i, p, cs[i], st, bug)
        lds.append(ld)
        ssums.append(ss)
    ssum, ld = torch.stack(ssums), torch.stack(lds)
    gauss = torch.sum(-0.5 * (p ** 2 + LOG2PI))
    sgn = 1.0 if "ssum_sign" in bug else -1.0
    logp = -(gauss / B + ld.sum() + sgn * ssum.sum() / B)
    return p, ssum, ld, logp


def _replicate(v: Tensor, R: int, bug, grad_bug: bool = False) -> Tensor:
    """[B, N, C] -> [B, N R, C]: row r of the output reads point r // R (ref_cpu.flow_g's repeat_interleave)."""
    B, N, C = v.shape
    if "cond_row" in bug:                         # ... replaced by r % T over the flattened rows
        flat = v.reshape(B * N, C)
        return flat[torch.arange(B * N * R) % (B * N)].reshape(B, N * R, C)
    out = torch.repeat_interleave(v, R, dim=1)
    if grad_bug and "ds_rm1" in bug:              # the last replica's contribution to ds / dt is lost
        last = (torch.arange(N * R) % R == R - 1).view(1, N * R, 1)
        out = torch.where(last, out.detach(), out)
    return out


def chain_g(sd, u: Tensor, cs: List[Tensor], R: int, st=None, bug=()) -> Tensor:
    """PointInterpFlow.g (ref_cpu.flow_g) on u [B, N R, 3]: the R replicas of a point share its conditioning row."""
    z = u
    for i in reversed(range(_nblocks(sd))):
        s, t = _st(sd, i, cs[i], st, bug)
        z = block_g(sd, i, z, _replicate(cs[i], R, bug), _replicate(s, R, bug, True), _replicate(t, R, bug, True), bug)
    return z


# ---------------------------------------------------------------------------------------------------- single nodes
def actnorm(x, logs, bias, inv: int):
    """ActNormFn: y = x exp(logs) + bias (inv = 0) or (x - bias) exp(-logs) (inv = 1)."""
    return (x - bias) * torch.exp(-logs) if inv else x * torch.exp(logs) + bias


def couple_inject(y, o, s, t, td: int):
    """CoupleInjectFn: out = (reverse(cat[y[:td], y[td:] - o]) - t) exp(-s)."""
    return (torch.cat([y[..., :td], y[..., td:] - o], dim=-1).flip(-1) - t) * torch.exp(-s)


def inject_inv(u, s, t, Rr: int = 1):
    """InjectInvFn / InjectInv2Fn: v = reverse(u exp(s) + t), s and t [T, 3] of the original points, u [T Rr, 3]."""
    return (u * torch.exp(s.repeat_interleave(Rr, dim=0)) + t.repeat_interleave(Rr, dim=0)).flip(-1)


def couple_add(v, o, td: int):
    """CoupleAddFn: out = cat[v[:td], v[td:] + o]."""
    return torch.cat([v[..., :td], v[..., td:] + o], dim=-1)


def batch_sum(x, mode: int):
    """BatchSumFn: x [B, ...] -> [B], mode 0 = sum, mode 1 = sum of -0.5 (x^2 + log 2 pi)."""
    return (x if mode == 0 else -0.5 * (x ** 2 + LOG2PI)).reshape(x.shape[0], -1).sum(dim=1)


def flow_params(W, logs, n: float):
    """FlowParamsFn: W -> (W^-1, (sum(logs) + log|det W|) n)."""
    return torch.inverse(W), ((logs.sum() + torch.slogdet(W)[1]) * n).reshape(1)


def flow_affine(x, o, td: int, logs, bias, M, inv: int):
    """FlowAffineFn: inv = 0: y = M (x e^logs + bias); inv = 1: y = (M [x_head, x_tail + o] - bias) e^-logs."""
    if not inv:
        return (x * torch.exp(logs) + bias) @ M.t()
    return ((couple_add(x, o, td) if o is not None else x) @ M.t() - bias) * torch.exp(-logs)


# ---------------------------------------------------------------------------------------------------- autograd pass, bar
def grads(fn: Callable[[Dict[str, Tensor]], Dict[str, Tensor]], inputs: Dict[str, Tensor], upstream: Dict[str, Tensor],
          dtype=torch.float64, device="cpu") -> Dict[str, Tensor]:
    """One autograd pass of fn over leaves made from `inputs` (cast to dtype on device): every output under its name and the
    gradient of sum_k <outputs[k], upstream[k]> with respect to input `name` under "d" + name."""
    leaves = {k: v.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for k, v in inputs.items()}
    outs = fn(leaves)
    loss = None
    for k, w in upstream.items():
        term = (outs[k] * w.to(device=device, dtype=dtype).reshape(outs[k].shape)).sum()
        loss = term if loss is None else loss + term
    gs = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    res = {k: v.detach() for k, v in outs.items()}
    for (k, leaf), g in zip(leaves.items(), gs):
        res["d" + k] = torch.zeros_like(leaf) if g is None else g.detach()
    return res


def min_preactivation(fn: Callable[[], object]) -> float:
    """Smallest |pre-activation| over all hidden LeakyReLU layers that `fn()` evaluates through lin_a1d."""
    global _REC
    _REC = []
    try:
        fn()
        return min(_REC) if _REC else float("inf")
    finally:
        _REC = None


def bar_of(r64: Tensor, r32: Tensor) -> float:
    r64 = r64.detach().double().cpu()
    e32 = float((r32.detach().double().cpu() - r64).abs().max()) if r64.numel() else 0.0
    return 16.0 * e32 + 2.0 ** -21 * (float(r64.abs().max()) if r64.numel() else 0.0)


def ceiling_of(r64: Tensor, gmax: float) -> float:
    """The widest bar a row-reduced quantity may be given: the suite's tier-against-tier bar (tests/test_gpu_train.py)."""
    return 2e-4 * float(r64.detach().abs().max()) + 1e-5 * gmax


def sum_envelope(terms: Tensor) -> float:
    """Four standard deviations of the rounding of a float32 tree sum over terms [n, ...] (dim 0), from the number format alone:
    an addition whose result has magnitude m rounds by up to 2^-24 m; over a tree of ceil(log2 n) levels the squared partial sums
    of one level add up to about sum x_i^2, so the rounding errors - independent, zero mean - have variance about
    2^-48 ceil(log2 n) sum x_i^2 / 3 <= (2^-24)^2 ceil(log2 n) sum x_i^2.  It exceeds the ulp of the result when the terms cancel;
    a single float32 run on the CPU (one more order) does not show that."""
    t = terms.detach().double().reshape(terms.shape[0], -1)
    levels = max(1, math.ceil(math.log2(max(t.shape[0], 2))))
    return float(4.0 * 2.0 ** -24 * torch.sqrt(levels * (t ** 2).sum(dim=0)).max())


def compare(got: Dict[str, Tensor], r64: Dict[str, Tensor], r32: Dict[str, Tensor], widened=None) -> Dict[str, tuple]:
    """name -> (error, bar) for every tensor of `got`.  widened: name -> the terms [n, ...] that a row-reduced quantity sums; its
    bar grows by sum_envelope(terms), never beyond the suite's tier-against-tier bar (ceiling_of)."""
    widened = widened or {}
    gmax = max([float(v.abs().max()) for k, v in r64.items() if k.startswith("d") and v.numel()] or [0.0])
    out = {}
    for k, g in got.items():
        ref = r64[k].detach().double().cpu()
        g = g.detach().double().cpu().reshape(ref.shape)
        err = float((g - ref).abs().max()) if ref.numel() else 0.0
        if not math.isfinite(err):
            err = float("inf")
        bar = bar_of(ref, r32[k])
        if k in widened:
            bar = min(bar + sum_envelope(widened[k]), max(bar, ceiling_of(ref, gmax)))
        out[k] = (err, bar)
    return out


def report(case: str, cmp: Dict[str, tuple], widened=()) -> str:
    """One line per case: the worst err / bar and every quantity's ratio (what profiles/flow_train/accuracy.txt holds)."""
    worst = max(cmp, key=lambda k: cmp[k][0] / cmp[k][1] if cmp[k][1] > 0 else (0.0 if cmp[k][0] == 0 else float("inf")))
    parts = [f"{k}{'[widened]' if k in widened else ''} {e:.2e}/{b:.2e}={e / b if b > 0 else 0.0:.2f}" for k, (e, b) in cmp.items()]
    return f"{case}: worst {worst} | " + " ".join(parts)


def failures(cmp: Dict[str, tuple]) -> List[str]:
    return [f"{k}: err {e:.3e} > bar {b:.3e}" for k, (e, b) in cmp.items() if not e <= b]


# ---------------------------------------------------------------------------------------------------- the chain cases
def _cyc(seq, n):
    return [seq[i % len(seq)] for i in range(n)]


def _case(name, inv, ccs, tds, R, B, N, Bsz, seed):
    return dict(id=name, inv=inv, nb=len(ccs), ccs=list(ccs), tds=list(tds), R=R, B=B, N=N, Bsz=Bsz, seed=seed)


# Seeds: constants, chosen on the CPU (`python tests/flow_train_ref.py` prints the search: the first seed >= 1 that qualifies) so
# that the float64 run keeps every hidden pre-activation at least MIN_PREACT away from the LeakyReLU kink - inner products here
# are at most 132 long over O(1) operands, a float32 pre-activation is off by a few 1e-6, so no tier lands on the other slope.
# Cases that are not listed take seed 1.
_SEEDS: Dict[str, int] = {
    "f-nb7-B1x35": 2, "f-nb7-B3x35": 2, "f-model-3x100": 173, "g-nb1-R2-T5": 2, "g-nb1-R16-T33": 2, "g-model-R4-3x25": 62,
    "mlp-td1-cdiv1-cc64-T130": 2, "mlp-td1-cdiv4-cc64-T130": 2, "mlp-td2-cdiv2-cc32-T130": 4, "mlp-td2-cdiv8-cc32-T130": 23,
}


def chain_cases() -> List[dict]:
    cs = []
    for T in (1, 16, 17, 528):                                       # 528 rows: 33 tiles, the strided sum loops twice
        cs.append(_case(f"f-nb1-T{T}", 0, [32], [1], 1, 1, T, 0, 0))
    cs.append(_case("f-nb8-T48", 0, _cyc([32, 64, 128], 8), _cyc([1, 2], 8), 1, 1, 48, 0, 0))
    for B in (1, 3):                                                 # 7 blocks: the most that still takes the logp epilogue
        cs.append(_case(f"f-nb7-B{B}x35", 0, _cyc([128, 64, 32], 7), _cyc([2, 1], 7), 1, B, 35, B, 0))
    cs.append(_case("f-model-3x100", 0, MODEL_CCS, MODEL_TDS, 1, 3, 100, 3, 0))
    for R in (1, 2, 4, 8, 16):
        for T in (1, 5, 33):
            cs.append(_case(f"g-nb1-R{R}-T{T}", 1, [64], [2], R, 1, T, 0, 0))
    cs.append(_case("g-nb2-R16-T17", 1, [32, 128], [1, 2], 16, 1, 17, 0, 0))      # 272 rows: five workgroups, the last partial
    cs.append(_case("g-nb8-R8-T6", 1, _cyc([64, 128, 32], 8), _cyc([2, 2, 1], 8), 8, 1, 6, 0, 0))
    cs.append(_case("g-model-R4-3x25", 1, MODEL_CCS, MODEL_TDS, 4, 3, 25, 0, 0))
    for c in cs:
        c["seed"] = _SEEDS.get(c["id"], 1)
    return cs


def chain_problem(case: dict, seed: Optional[int] = None):
    """-> (inputs, upstream, ref) of a chain case: `inputs` name -> float64 tensor (x, cflat, st, b<i>.<param>), `upstream` the
    random output weights, `ref(leaves, bug=())` the restatement on such a dict -> dict of outputs."""
    seed = case["seed"] if seed is None else seed
    nb, ccs, R, B, N = case["nb"], case["ccs"], case["R"], case["B"], case["N"]
    T = B * N
    sd = make_blocks(nb, ccs, case["tds"], 7919 * seed + 11, torch.float64)
    rng = np.random.Generator(np.random.PCG64(104729 * seed + 5))
    inputs = {"x": randn(rng, (B, N * R, 3)),
              "cflat": torch.cat([randn(rng, (T * cc,)) for cc in ccs]),
              "st": torch.stack([randn(rng, (T, 3), scale=0.3 if k % 2 == 0 else 0.5) for k in range(2 * nb)])}
    for i in range(nb):
        for n, p in zip(PARAMS, block_params(sd, i)):
            inputs[f"b{i}.{n}"] = p
    upstream = {"out" if case["inv"] else "z": randn(rng, (B, N * R, 3))}
    if not case["inv"]:
        if case["Bsz"]:
            upstream["logp"] = torch.tensor([0.37], dtype=torch.float64)
        else:
            upstream["ssum"], upstream["ld"] = randn(rng, (nb,)), randn(rng, (nb,))
    idx = {k: v for k, v in sd.items() if v.dtype == torch.int64}

    def ref(lv, bug=()):
        s = dict(idx)
        for i in range(nb):
            for n in PARAMS:
                s[f"flow_blocks.{i}.{_KEY[n]}"] = lv[f"b{i}.{n}"]
        cs, off = [], 0
        for cc in ccs:
            cs.append(lv["cflat"][off:off + T * cc].view(B, N, cc))
            off += T * cc
        if case["inv"]:
            return {"out": chain_g(s, lv["x"], cs, R, lv["st"], bug)}
        z, ssum, ld, logp = chain_f(s, lv["x"], cs, lv["st"], bug)
        return {"z": z, "logp": logp.reshape(1)} if case["Bsz"] else {"z": z, "ssum": ssum, "ld": ld}

    return inputs, upstream, ref


def bug_applies(bug: str, case: dict) -> bool:
    """Whether a deliberate error changes the function of a case at all."""
    if bug == "no_logdet":
        return not case["inv"]
    if bug == "ssum_sign":
        return not case["inv"] and case["Bsz"] > 0
    if bug == "cond_row":
        return bool(case["inv"]) and case["R"] > 1 and case["B"] * case["N"] > 1
    if bug == "ds_rm1":
        return bool(case["inv"]) and case["R"] > 1
    if bug == "dw_no_inv":
        return bool(case["inv"])
    return True


def mlp_cases() -> List[dict]:
    """`mlp_fused` in its "cond" form: every (td, cdiv) pair, every cc in {32, 64, 128} and every T in {1, 17, 130}."""
    cs = []
    for ti, td in enumerate((0, 1, 2)):
        for ci, cdiv in enumerate((1, 2, 3, 4, 8, 16)):
            cc, T = (32, 64, 128)[(ti + ci) % 3], (1, 17, 130)[(2 * ti + ci) % 3]
            name = f"mlp-td{td}-cdiv{cdiv}-cc{cc}-T{T}"
            cs.append(dict(id=name, td=td, cdiv=cdiv, cc=cc, T=T, seed=_SEEDS.get(name, 1)))
    return cs


def mlp_problem(case: dict, seed: Optional[int] = None):
    """-> (inputs, upstream, ref) of a conditioner case: LinearA1D on cat[y[:, :td], c[row // cdiv]], against lin_a1d."""
    seed = case["seed"] if seed is None else seed
    td, cdiv, cc, T = case["td"], case["cdiv"], case["cc"], case["T"]
    rows, dout = T * cdiv, (3 - td if td else 3)
    rng = np.random.Generator(np.random.PCG64(15485863 * seed + 3))
    sd: Dict[str, Tensor] = {}
    _lin_a1d_init(sd, rng, "n", td + cc, dout, torch.float64)
    inputs = {"c": randn(rng, (T, cc)), "w0": sd["n.layers.0.weight"], "w2": sd["n.layers.2.weight"], "b2": sd["n.layers.2.bias"],
              "w4": sd["n.layers.4.weight"], "b4": sd["n.layers.4.bias"]}
    if td:
        inputs["y"] = randn(rng, (rows, 3))
    upstream = {"out": randn(rng, (rows, dout))}

    def ref(lv, bug=()):
        s = {"n.layers.0.weight": lv["w0"], "n.layers.2.weight": lv["w2"], "n.layers.2.bias": lv["b2"],
             "n.layers.4.weight": lv["w4"], "n.layers.4.bias": lv["b4"]}
        h = lv["c"].repeat_interleave(cdiv, dim=0)
        if td:
            h = torch.cat([lv["y"][:, :td], h], dim=1)
        return {"out": lin_a1d(s, "n", h)}

    return inputs, upstream, ref


def _clear_of_kinks(problem) -> bool:
    inputs, _, ref = problem
    return min_preactivation(lambda: ref(inputs)) >= MIN_PREACT


def find_seed(problem: Callable[[int], object], tries: int = 1000, clear: Callable[[object], bool] = _clear_of_kinks) -> int:
    """The first seed >= 1 whose float64 run stays MIN_PREACT away from every kink.  clear(problem(seed)): the test of one
    seed (tests/extract_train_ref.py has pool decisions besides the kinks, and its own)."""
    for seed in range(1, tries + 1):
        if clear(problem(seed)):
            return seed
    raise RuntimeError("no seed found")


if __name__ == "__main__":
    for c in chain_cases():
        print(f'    "{c["id"]}": {find_seed(lambda s: chain_problem(c, s))},', flush=True)
    for c in mlp_cases():
        print(f'    "{c["id"]}": {find_seed(lambda s: mlp_problem(c, s))},', flush=True)
