"""pf_patch_batch / DevicePatchData on the GPU: one launch gathers, subsamples and augments a training batch from a
device-resident dataset.  The references are the indexing itself (bit for bit), the numpy restatement of the kernel's Philox
streams in float64 (tests/philox_ref.py) and float64 recomputations from the kernel's own `params`.  Every test also asserts
that the sticky status word stayed 0.  B = 32, n = 256, n_out = 1024 throughout."""
import numpy as np
import pytest
import torch

import philox_ref as P
from test_data_device import KS_BAR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N, N_OUT, M = 32, 256, 1024, 80
SUB, JIT, ROT, ZROT, SCA, SHI = 1, 2, 4, 8, 16, 32


class _Set:
    """A random dataset on the device + the epoch's permutation + a status word."""

    def __init__(self, n_in, seed=0, m=M):
        rng = np.random.default_rng(seed)
        self.inp_h = (rng.random((m, n_in, 3), dtype=np.float32) * 2 - 1) * np.float32(1.5)      # |x| <= 1.5
        self.gt_h = (rng.random((m, N_OUT, 3), dtype=np.float32) * 2 - 1) * np.float32(1.5)
        self.rad_h = rng.uniform(0.5, 2.0, m).astype(np.float32)
        self.order_h = rng.permutation(m).astype(np.int32)
        self.inp, self.gt, self.rad, self.order = (torch.from_numpy(a).to(DEV) for a in (self.inp_h, self.gt_h, self.rad_h, self.order_h))
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.m = m

    def sel(self, pos, b=B):
        return self.order_h[(pos + np.arange(b)) % self.m]

    def run(self, flags, pos=0, b=B, slot0=0, seed=2021, **kw):
        from puflow_amd.data import patch_batch
        out = patch_batch(self.inp, self.gt, self.rad, self.order, pos, b, N, slot0, seed, flags, self.status, **kw)
        torch.cuda.synchronize()
        assert int(self.status.item()) == 0, "status word"
        return [None if t is None else t.cpu().numpy() for t in out]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_gather_only_is_the_indexing_bit_for_bit():
    """The validation setting: no stage.  Rows wrap around the end of `order` like PatchData's batches."""
    ds = _Set(N)
    for pos in (0, 64, 79):                                             # 64 + 32 > 80, 79 + 32 > 80: both wrap
        inp, gt, rad, prm, idx, cand = ds.run(0, pos=pos, want_idx=True)
        sel = ds.sel(pos)
        assert np.array_equal(_bits(inp), _bits(ds.inp_h[sel])) and np.array_equal(_bits(gt), _bits(ds.gt_h[sel]))
        assert np.array_equal(_bits(rad), _bits(ds.rad_h[sel]))
        assert np.array_equal(idx, np.broadcast_to(np.arange(N), (B, N))) and cand is None
        want = np.zeros((B, 16), np.float32); want[:, [0, 4, 8, 9]] = 1.0                 # identity, scale 1, no shift, no loc
        assert np.array_equal(prm, want)


def test_subsample_structure():
    """The selection replayed on the host from the kernel's OWN candidates reproduces idx, order included; every row holds n
    distinct indices; the points are inp[sel][idx] bit for bit; what was not consumed of `cand` is untouched."""
    ds = _Set(1024)
    T = 3000                                                            # not a multiple of the round length
    inp, gt, rad, prm, idx, cand = ds.run(SUB, pos=70, want_idx=True, cand_len=T)
    sel = ds.sel(70)
    rounds = prm[:, 14].astype(np.int64)
    assert (rounds >= 1).all() and (rounds <= 64).all() and (prm[:, 13] > 0.1 - 1e-6).all() and (prm[:, 13] < 0.9 + 1e-6).all()
    for r in range(B):
        used = min(T, rounds[r] * 1024)
        want, want_rounds, short = P.select(cand[r, :used], 1024, N)
        assert not short and want_rounds == rounds[r] and np.array_equal(idx[r], want), r
        assert (cand[r, used:] == -2 ** 31).all()
        assert len(set(idx[r].tolist())) == N and idx[r].min() >= 0 and idx[r].max() < 1024
        assert np.array_equal(_bits(inp[r]), _bits(ds.inp_h[sel[r]][idx[r]])), r
    assert np.array_equal(_bits(gt), _bits(ds.gt_h[sel])) and np.array_equal(_bits(rad), _bits(ds.rad_h[sel]))


def test_subsample_randomness():
    """The candidates are the float64 restatement on the restated Philox bits up to fp32 truncation flips (within 1 everywhere,
    equal on >= 99 %: a condition - tests/test_data_device.py checks float32 against float64 on the CPU), and the kept indices
    have the pooled distribution of PatchData._nonuniform (KS bar of the CPU file, 2048 patches)."""
    from puflow_amd.data import PatchData
    ds = _Set(1536)
    seed, slot0 = 99, (5 << 32) + 7                                     # a slot beyond 32 bits: both counter words in use
    inp, gt, rad, prm, idx, cand = ds.run(SUB, slot0=slot0, seed=seed, want_idx=True, cand_len=1024)
    diff = 0
    for r in range(B):
        want = P.candidates(seed, slot0 + r, 1536, 1024)
        d = np.abs(cand[r].astype(np.int64) - want)
        assert d.max() <= 1, (r, d.max())
        diff += int((d != 0).sum())
    print(f"candidates differing from float64 by one: {diff} of {B * 1024}")
    assert diff <= 0.01 * B * 1024
    ds = _Set(1024)
    patches = 2048
    idx = ds.run(SUB, b=patches, want_idx=True)[4]                      # 2048 rows in one launch (the patches repeat mod M)
    assert all(len(set(row.tolist())) == N for row in idx)
    pd = PatchData(np.zeros((1, 1024, 3), np.float32), np.zeros((1, N, 3), np.float32), seed=100)
    ref = np.concatenate([pd._nonuniform(1024, N) for _ in range(patches)])
    ks = P.ks_statistic(idx, ref, 1024)
    print(f"KS(kernel idx, _nonuniform) = {ks:.4f}  bar {KS_BAR}")
    assert ks <= KS_BAR


@pytest.mark.parametrize("z_rotated", [False, True])
def test_parameters(z_rotated):
    """loc, scale, shifts against the float64 restatement (1e-6 relative).  `params` carries R, not the angles: R is held against
    Rz Ry Rx recomputed in float64 from the angles as the kernel forms them (fp32 2 pi u of the restated bits; 1e-6 absolute),
    which pins the kernel's angles through R; R orthonormal with det 1 (1e-6)."""
    ds = _Set(1024)
    seed, slot0 = 4242, 1000
    kw = dict(scale_low=0.8, scale_high=1.2, shift_range=0.1)
    prm = ds.run(SUB | ROT | SCA | SHI | (ZROT if z_rotated else 0), slot0=slot0, seed=seed, **kw)[3]
    for r in range(B):
        p64, p32 = P.patch_params(seed, slot0 + r, **kw), P.patch_params(seed, slot0 + r, dtype=np.float32, **kw)
        assert abs(prm[r, 13] - p64["loc"]) <= 1e-6 * abs(p64["loc"]) and abs(prm[r, 9] - p64["scale"]) <= 1e-6 * abs(p64["scale"])
        assert (np.abs(prm[r, 10:13] - p64["shift"]) <= 1e-6 * np.abs(p64["shift"])).all(), (prm[r, 10:13], p64["shift"])
        R = prm[r, :9].astype(np.float64).reshape(3, 3)
        assert np.abs(R - P.rotation(p32["angles"], z_rotated)).max() <= 1e-6, r
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(R) - 1.0) <= 1e-6
        if z_rotated:
            assert R[2, 2] == 1.0 and R[0, 2] == 0.0 and R[2, 0] == 0.0


def test_jitter_alone():
    """out - in is the restated clipped noise (1e-3 sigma absolute: fp32 logf near u -> 1 leaves ~2e-4 on the radius), never beyond
    the clip (+ the rounding of the sum), and the ground truth and radius are untouched."""
    ds = _Set(N)
    sigma, clip, seed, slot0 = 0.01, 0.02, 11, 320                      # clip at 2 sigma: ~4.6 % of the values are clipped
    inp, gt, rad, prm, _, _ = ds.run(JIT, pos=3, slot0=slot0, seed=seed, jitter_sigma=sigma, jitter_max=clip)
    sel = ds.sel(3)
    d = inp.astype(np.float64) - ds.inp_h[sel].astype(np.float64)
    clipped = 0
    for r in range(B):
        want = P.jitter_noise(seed, slot0 + r, N, sigma, clip)
        assert np.abs(d[r] - want).max() <= 1e-3 * sigma, (r, np.abs(d[r] - want).max())
        clipped += int((np.abs(want) == clip).sum())
    assert clipped > 0 and (np.abs(d) <= clip + 2.0 ** -23 * np.abs(ds.inp_h[sel])).all()
    assert np.array_equal(_bits(gt), _bits(ds.gt_h[sel])) and np.array_equal(_bits(rad), _bits(ds.rad_h[sel]))


@pytest.mark.parametrize("n_in", [N, 1024])
def test_full_augmentation(n_in):
    """Input and ground truth are ((x [+ noise]) @ R) s + t in float64 from the kernel's own params (2e-6 absolute: ~12 fp32
    operations on |x| <= 1.5); the radius is radius * s.  x + noise is the jitter-only launch of the same slots (bit-exact fp32),
    x the points the subsample picked."""
    ds = _Set(n_in)
    sub = SUB if n_in > N else 0
    kw = dict(pos=17, slot0=96, seed=5, shift_range=0.05)
    xj, _, _, _, idx_j, _ = ds.run(sub | JIT, want_idx=True, **kw)
    inp, gt, rad, prm, idx, _ = ds.run(sub | JIT | ROT | SCA | SHI, want_idx=True, **kw)
    sel = ds.sel(17)
    assert np.array_equal(idx, idx_j)                                   # a stage's stream does not depend on the other switches
    assert (np.abs(prm[:, 10:13]) <= 0.05).all() and (np.abs(prm[:, 10:13]) > 0).all() and (prm[:, 9] >= 0.8).all() and (prm[:, 9] <= 1.2).all()
    for r in range(B):
        R, s, t = prm[r, :9].astype(np.float64).reshape(3, 3), float(prm[r, 9]), prm[r, 10:13].astype(np.float64)
        assert np.abs(inp[r] - ((xj[r].astype(np.float64) @ R) * s + t)).max() <= 2e-6, r
        assert np.abs(gt[r] - ((ds.gt_h[sel[r]].astype(np.float64) @ R) * s + t)).max() <= 2e-6, r
    assert np.array_equal(_bits(rad), _bits(ds.rad_h[sel] * prm[:, 9]))


def test_invariance_is_bit_exact():
    """A batch is a pure function of (dataset, order, seed, slots): the same call twice, and the rows a world = 4 rank produces
    against the slice of the world = 1 batch, give the same bits; another seed or step changes every patch's params."""
    from puflow_amd.dist import shard_bounds
    ds = _Set(1024)
    flags, step = SUB | JIT | ROT | SCA | SHI, 12
    kw = dict(seed=2021, shift_range=0.05, want_idx=True)
    a = ds.run(flags, pos=60, slot0=step * B, **kw)
    b = ds.run(flags, pos=60, slot0=step * B, **kw)
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for rank in range(4):
        lo, hi = shard_bounds(B, rank, 4)
        part = ds.run(flags, pos=60 + lo, b=hi - lo, slot0=step * B + lo, **kw)
        for x, y in zip(a[:5], part[:5]):
            assert np.array_equal(x[lo:hi].view(np.uint32), y.view(np.uint32)), rank
    other_seed = ds.run(flags, pos=60, slot0=step * B, **{**kw, "seed": 2022})[3]
    other_step = ds.run(flags, pos=60, slot0=(step + 1) * B, **kw)[3]
    for o in (other_seed, other_step):
        assert ((o[:, :9] != a[3][:, :9]).any(axis=1) & (o[:, 9] != a[3][:, 9]) & (o[:, 10] != a[3][:, 10]) & (o[:, 13] != a[3][:, 13])).all()


def _ids(data):
    return np.concatenate([b["up_ratio_pl"].cpu().numpy() for b in data]).astype(np.int64)


def test_epoch_behaviour():
    """DevicePatchData: without augmentation one pass over a 10-batch set yields every patch exactly once, in the order of the
    uploaded permutation; epochs use different permutations; two objects with one seed yield identical streams; a rank of four
    yields its rows of the whole batch."""
    from puflow_amd.data import DevicePatchData
    m = 10 * B
    rng = np.random.default_rng(1)
    inp, gt = rng.random((m, N, 3), dtype=np.float32), rng.random((m, N_OUT, 3), dtype=np.float32)
    ident = np.arange(m, dtype=np.float32)                              # the radius names the patch
    d = DevicePatchData(inp, gt, ident, batch_size=B, num_point_patch=N, is_augment=False, device=DEV, seed=3)
    assert len(d) == 10
    e0 = _ids(d)
    assert np.array_equal(e0, d.order.cpu().numpy()) and np.array_equal(np.sort(e0), np.arange(m))
    first = next(iter(DevicePatchData(inp, gt, ident, batch_size=B, num_point_patch=N, is_augment=False, device=DEV, seed=3)))
    assert np.array_equal(_bits(first["input_sparse_xyz_pl"].cpu().numpy()), _bits(inp[e0[:B]]))
    e1 = _ids(d)
    assert np.array_equal(np.sort(e1), np.arange(m)) and not np.array_equal(e0, e1)
    assert d.status() == 0 and d.step == 20
    aug = dict(batch_size=B, num_point_patch=N, use_random_input=True, is_augment=True, device=DEV, seed=8, shift_range=0.02)
    inp4 = rng.random((m, 4 * N, 3), dtype=np.float32)
    a, b = DevicePatchData(inp4, gt, ident, **aug), DevicePatchData(inp4, gt, ident, **aug)
    ranks = [DevicePatchData(inp4, gt, ident, rank=r, world=4, **aug) for r in range(4)]
    for _epoch in range(2):
        its = [iter(r) for r in ranks]
        for k, (x, y) in enumerate(zip(a, b)):
            assert x["input_sparse_xyz_pl"].data_ptr() != y["input_sparse_xyz_pl"].data_ptr()
            parts = [next(it) for it in its]
            for key in x:
                assert torch.equal(x[key], y[key]), (k, key)
                assert torch.equal(x[key], torch.cat([p[key] for p in parts])), (k, key)
            if k >= 2:
                break
        for it in its:
            it.close()
    assert a.status() == 0 and b.status() == 0 and all(r.status() == 0 for r in ranks)


def test_bound_batches_feed_the_captured_step(monkeypatch):
    """fit(graph=True) binds the data object to the captured step's inputs: 12 batches (two epochs of six) written straight into
    `graph.static` give, bit for bit (deterministic mode), the per-batch losses and final parameters of the same 12 batches
    materialised first and fed through GraphedTrainStep.__call__ from an identical module; once bound, the yielded tensors ARE
    the captured inputs."""
    from puflow_amd import train_ops
    from puflow_amd.data import KEYS, SyntheticDevicePatchData
    from puflow_amd.train import fit
    from puflow_amd.train_graph import GraphedTrainStep
    from puflow_amd.trainer import TrainerModule, default_cfg
    from puflow_amd.weights import synth_state_dict

    def make():
        torch.manual_seed(0)
        tm = TrainerModule(default_cfg(learning_rate=1e-3, deterministic=True), loss_mix="pu1k")
        tm.network.load_state_dict(synth_state_dict(21))
        return tm.to(DEV)

    def data():
        return SyntheticDevicePatchData(num_patches=2 * B, num_point_patch=N, up_ratio=4, seed=13, batch_size=B, num_batches=6,
                                        use_random_input=True, is_augment=True, device=DEV)

    try:
        # reference: the batches first, then one captured step fed through its copy-in
        src = data()
        batches = [{k: v.clone() for k, v in b.items()} for _ in range(2) for b in src]
        assert len(batches) == 12 and src.status() == 0
        tr = make()
        step = tr.graphed_train_step(batches[0], tr.configure_optimizers()["optimizer"], 1e-2, warmup=1)
        want = [step.warmup_loss.clone()] + [step(b).clone() for b in batches[1:]]
        torch.cuda.synchronize()

        got, steps = [], []
        tm = make()
        inner = tm.graphed_train_step

        def capture(batch, optimizer, clip=1e-2, warmup=2):
            s = inner(batch, optimizer, clip, warmup=warmup)
            got.append(s.warmup_loss.clone()); steps.append(s)
            return s

        replay = GraphedTrainStep.__call__

        def call(self, batch):
            if self is steps[0]:
                assert all(batch[k].data_ptr() == self.static[k].data_ptr() for k in KEYS), "batch not in place"
            loss = replay(self, batch)
            got.append(loss.clone())
            return loss

        monkeypatch.setattr(tm, "graphed_train_step", capture)
        monkeypatch.setattr(GraphedTrainStep, "__call__", call)
        bound = data()
        hist = fit(tm, bound, None, max_epochs=2, log=None, graph=True)
        torch.cuda.synchronize()
        assert hist["epochs"] == 2 and len(steps) == 1 and len(got) == 12 and bound.status() == 0 and bound.step == 12
        assert all(torch.equal(g, w) for g, w in zip(got, want)), ([float(g) for g in got], [float(w) for w in want])
        sa, sb = tm.state_dict(), tr.state_dict()
        bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
        assert not bad, bad[:5]
        nxt = next(iter(bound))                                         # fit() unbinds on its way out: fresh tensors again
        assert all(nxt[k].data_ptr() != steps[0].static[k].data_ptr() for k in KEYS)
        bound.bind(steps[0].static)
        nxt = next(iter(bound))
        assert all(nxt[k] is steps[0].static[k] for k in KEYS)
    finally:
        train_ops.set_deterministic(False)
