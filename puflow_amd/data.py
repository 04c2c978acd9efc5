"""Patch datasets for the training entry points.

Mirrors what the reference's PU1K data path feeds `TrainerModule` (`dataset/pu1k/fetcher.py:11-48` loader and normalisation,
`:69-101` batch assembly and augmentation, `dataset/pu1k/dataset.py:24-52` dict batches) without TensorFlow / Lightning /
a background thread: a plain iterator of batches that are already torch tensors on the training device.

File formats: the reference's HDF5 container (datasets `poisson_<n>`; needs `h5py`, which this image does not ship: the
reader raises with that message instead of failing at import) and an `.npz` with the same array names (tests, synthetic data).
`SyntheticPatchData` makes surface patches in memory (the build / bench machines have no datasets).
"""
from __future__ import annotations

from typing import Dict, Iterator, Optional, Tuple

import numpy as np
import torch

from . import _lib


def load_patch_arrays(path: str, num_point: int = 256, up_ratio: int = 4, use_random_input: bool = False,
                      skip_rate: int = 1) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (input [M, n_in, 3], gt [M, num_point * up_ratio, 3], radius [M]) fp32, normalised like the reference
    (`fetcher.py:32-40`): both clouds are centred on the INPUT's centroid and divided by the input's furthest distance."""
    n_in = num_point * 4 if use_random_input else num_point
    n_out = num_point * up_ratio
    if path.endswith(".npz"):
        with np.load(path) as f:
            inp, gt = f[f"poisson_{n_in}"].astype(np.float32), f[f"poisson_{n_out}"].astype(np.float32)
    else:
        try:
            import h5py
        except ImportError as e:               # pragma: no cover - h5py is not installed in the build image
            raise ImportError("reading the reference's .h5 patch files needs h5py (not installed); convert the two arrays "
                              f"'poisson_{n_in}' / 'poisson_{n_out}' to an .npz with the same names") from e
        with h5py.File(path, "r") as f:       # pragma: no cover
            inp, gt = f[f"poisson_{n_in}"][:].astype(np.float32), f[f"poisson_{n_out}"][:].astype(np.float32)
    if len(inp) != len(gt):
        raise ValueError("input / ground-truth patch counts differ")
    inp, gt = inp[..., :3].copy(), gt[..., :3].copy()
    centroid = inp.mean(axis=1, keepdims=True)
    inp -= centroid
    far = np.sqrt((inp ** 2).sum(-1)).max(axis=1, keepdims=True)[..., None]
    inp /= far
    gt = (gt - centroid) / far
    radius = np.ones(len(inp), np.float32)
    return inp[::skip_rate], gt[::skip_rate], radius[::skip_rate]


# ---- augmentation (the reference applies jitter -> rotation -> scale, fetcher.py:96-100) --------------------------------
def jitter(rng: np.random.Generator, x: np.ndarray, sigma: float, clip: float) -> np.ndarray:
    return x + np.clip(sigma * rng.standard_normal(x.shape), -clip, clip).astype(np.float32)


def random_rotations(rng: np.random.Generator, n: int) -> np.ndarray:
    """[n, 3, 3] rotations Rz Ry Rx with independent uniform angles (applied as row-vector x @ R)."""
    a = rng.uniform(0.0, 2.0 * np.pi, size=(n, 3))
    c, s = np.cos(a), np.sin(a)
    R = np.zeros((n, 3, 3, 3))
    R[:, 0] = np.eye(3); R[:, 1] = np.eye(3); R[:, 2] = np.eye(3)
    R[:, 0, 1, 1], R[:, 0, 1, 2], R[:, 0, 2, 1], R[:, 0, 2, 2] = c[:, 0], -s[:, 0], s[:, 0], c[:, 0]        # about x
    R[:, 1, 0, 0], R[:, 1, 0, 2], R[:, 1, 2, 0], R[:, 1, 2, 2] = c[:, 1], s[:, 1], -s[:, 1], c[:, 1]        # about y
    R[:, 2, 0, 0], R[:, 2, 0, 1], R[:, 2, 1, 0], R[:, 2, 1, 1] = c[:, 2], -s[:, 2], s[:, 2], c[:, 2]        # about z
    return (R[:, 2] @ R[:, 1] @ R[:, 0]).astype(np.float32)


def augment(rng: np.random.Generator, inp: np.ndarray, gt: np.ndarray, radius: np.ndarray, jitter_sigma: float,
            jitter_max: float, scale_low: float = 0.8, scale_high: float = 1.2):
    inp = jitter(rng, inp, jitter_sigma, jitter_max)
    R = random_rotations(rng, len(inp))
    inp, gt = np.einsum("bnk,bkl->bnl", inp, R), np.einsum("bnk,bkl->bnl", gt, R)
    sc = rng.uniform(scale_low, scale_high, size=len(inp)).astype(np.float32)
    return inp * sc[:, None, None], gt * sc[:, None, None], radius * sc


class PatchData:
    """Iterable of dict batches with the reference's keys (`dataset.py:45-52`): 'input_sparse_xyz_pl' [B, n, 3],
    'gt_dense_xyz_pl' [B, n * up_ratio, 3], 'up_ratio_pl' [B] (the patch radius).  One pass = `num_batches` batches of
    a fresh shuffle; under torch.distributed every rank draws the same shuffle and keeps its contiguous shard."""

    def __init__(self, inp: np.ndarray, gt: np.ndarray, radius: Optional[np.ndarray] = None, batch_size: int = 32,
                 num_point_patch: int = 256, use_random_input: bool = False, is_augment: bool = True,
                 jitter_sigma: float = 0.01, jitter_max: float = 0.03, num_batches: Optional[int] = None,
                 device: str = "cpu", seed: int = 2021, rank: int = 0, world: int = 1):
        self.inp, self.gt = inp, gt
        self.radius = radius if radius is not None else np.ones(len(inp), np.float32)
        self.batch_size, self.npoint, self.random_input = batch_size, num_point_patch, use_random_input
        self.is_augment, self.jitter_sigma, self.jitter_max = is_augment, jitter_sigma, jitter_max
        self.num_batches = num_batches if num_batches is not None else len(inp) // batch_size
        self.device, self.rank, self.world = device, rank, world
        self.rng = np.random.default_rng(seed)                      # the same stream on every rank

    def __len__(self) -> int:
        return self.num_batches

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        from .dist import shard_bounds
        order = self.rng.permutation(len(self.inp))
        for b in range(self.num_batches):
            sel = order[(b * self.batch_size) % len(order):][:self.batch_size]
            if len(sel) < self.batch_size:                           # wrap (num_batches may exceed one pass)
                sel = np.concatenate([sel, order[:self.batch_size - len(sel)]])
            inp, gt, rad = self.inp[sel].copy(), self.gt[sel].copy(), self.radius[sel].copy()
            if self.random_input:                                    # non-uniform subsample of the 4x input (fetcher.py:88-95)
                new = np.zeros((len(sel), self.npoint, 3), np.float32)
                for i in range(len(sel)):
                    new[i] = inp[i][self._nonuniform(inp.shape[1], self.npoint)]
                inp = new
            if self.is_augment:
                inp, gt, rad = augment(self.rng, inp, gt, rad, self.jitter_sigma, self.jitter_max)
            lo, hi = shard_bounds(len(sel), self.rank, self.world)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a[lo:hi], dtype=np.float32)).to(self.device)
            yield {"input_sparse_xyz_pl": t(inp), "gt_dense_xyz_pl": t(gt), "up_ratio_pl": t(rad)}

    def _nonuniform(self, num: int, sample_num: int) -> np.ndarray:
        """Indices clustered around a random location (Gaussian in index space), without repetition."""
        loc = self.rng.uniform(0.1, 0.9)
        chosen: Dict[int, None] = {}
        while len(chosen) < sample_num:
            for a in (self.rng.normal(loc, 0.3, size=2 * sample_num) * num).astype(np.int64):
                if 0 <= a < num and len(chosen) < sample_num:
                    chosen.setdefault(int(a))
        return np.fromiter(chosen, dtype=np.int64)


def patch_data_from_file(path: str, on_device: bool = False, **kw):
    """-> PatchData, or DevicePatchData with on_device=True (the whole file is uploaded once)."""
    npoint, up = kw.get("num_point_patch", 256), kw.pop("up_ratio", 4)
    inp, gt, rad = load_patch_arrays(path, npoint, up, kw.get("use_random_input", False))
    return (DevicePatchData if on_device else PatchData)(inp, gt, rad, **kw)


def _synth_arrays(num_patches: int, num_point_patch: int, up_ratio: int, seed: int, n_in: int):
    """Surface patches made in memory (`weights.synth_patches`): dense = n*up points on a random smooth surface, sparse =
    n_in of them, both normalised by the SPARSE cloud like `load_patch_arrays`."""
    from .weights import synth_patches
    dense = synth_patches(num_patches, num_point_patch * up_ratio, seed=seed).numpy()
    rng = np.random.default_rng(seed + 1)
    sparse = np.stack([d[rng.permutation(d.shape[0])[:n_in]] for d in dense])
    c = sparse.mean(axis=1, keepdims=True)
    far = np.sqrt(((sparse - c) ** 2).sum(-1)).max(axis=1, keepdims=True)[..., None]
    return ((sparse - c) / far).astype(np.float32), ((dense - c) / far).astype(np.float32)


class SyntheticPatchData(PatchData):
    """`_synth_arrays` as a PatchData; with use_random_input the sparse cloud has 4n points (all of the dense one at up_ratio 4)."""

    def __init__(self, num_patches: int = 256, num_point_patch: int = 256, up_ratio: int = 4, seed: int = 2021, **kw):
        n_in = min(num_point_patch * 4, num_point_patch * up_ratio) if kw.get("use_random_input") else num_point_patch
        inp, gt = _synth_arrays(num_patches, num_point_patch, up_ratio, seed, n_in)
        super().__init__(inp, gt, num_point_patch=num_point_patch, seed=seed, **kw)


# ---- batches assembled on the device (csrc/data_aug.hip: pf_patch_batch) ----------------------------------------------------
PATCH_SUBSAMPLE, PATCH_JITTER, PATCH_ROTATE, PATCH_Z_ROTATED, PATCH_SCALE, PATCH_SHIFT = (
    _lib.PF_PATCH_SUBSAMPLE, _lib.PF_PATCH_JITTER, _lib.PF_PATCH_ROTATE, _lib.PF_PATCH_Z_ROTATED, _lib.PF_PATCH_SCALE, _lib.PF_PATCH_SHIFT)
KEYS = ("input_sparse_xyz_pl", "gt_dense_xyz_pl", "up_ratio_pl")


def patch_batch(inp: torch.Tensor, gt: torch.Tensor, radius: torch.Tensor, order: torch.Tensor, pos: int, b: int, n: int,
                slot0: int, seed: int, flags: int, status: torch.Tensor, jitter_sigma: float = 0.01, jitter_max: float = 0.03,
                scale_low: float = 0.8, scale_high: float = 1.2, shift_range: float = 0.0, out=None,
                params: Optional[torch.Tensor] = None, want_idx: bool = False, cand_len: int = 0):
    """One `pf_patch_batch` launch on the current stream (include/puflow_hip.h has the contract): rows [0, b) taking patches
    order[(pos + r) % M] with the random numbers of global patch slots slot0 + r.  out: (out_inp, out_gt, out_radius) to write
    into, else fresh tensors.  -> (out_inp [b,n,3], out_gt [b,n_out,3], out_radius [b], params [b,16], idx [b,n] int32 or
    None, cand [b,cand_len] int32 or None).  No host synchronisation."""
    from .ops import _stream
    lib = _lib.load()
    for t, dt in ((inp, torch.float32), (gt, torch.float32), (radius, torch.float32), (order, torch.int32), (status, torch.int32)):
        if not t.is_cuda:
            raise _lib.PuflowHipError("patch_batch needs GPU tensors (no CPU fallback)")
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError("patch_batch: dataset tensors must be contiguous fp32 (order, status: int32)")
    M, n_in, n_out, dev = inp.shape[0], inp.shape[1], gt.shape[1], inp.device
    if gt.shape[0] != M or radius.numel() != M or order.numel() != M:
        raise ValueError("patch_batch: inp, gt, radius and order disagree on the number of patches")
    if out is None:
        out = (torch.empty((b, n, 3), dtype=torch.float32, device=dev), torch.empty((b, n_out, 3), dtype=torch.float32, device=dev),
               torch.empty((b,), dtype=torch.float32, device=dev))
    o_inp, o_gt, o_rad = out
    for t, shape in ((o_inp, (b, n, 3)), (o_gt, (b, n_out, 3)), (o_rad, (b,))):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"patch_batch: output tensor {tuple(t.shape)} is not a contiguous fp32 {shape} on {dev}")
    if params is None:
        params = torch.empty((b, 16), dtype=torch.float32, device=dev)
    elif tuple(params.shape) != (b, 16) or params.dtype != torch.float32 or not params.is_contiguous() or params.device != dev:
        raise ValueError("patch_batch: params must be a contiguous fp32 [b, 16] tensor on the dataset's device")
    idx = torch.empty((b, n), dtype=torch.int32, device=dev) if want_idx else None
    cand = torch.full((b, cand_len), -2 ** 31, dtype=torch.int32, device=dev) if cand_len > 0 else None
    _lib.check(lib.pf_patch_batch(inp.data_ptr(), gt.data_ptr(), radius.data_ptr(), order.data_ptr(), M, n_in, n_out, int(pos), b, n,
                                  int(slot0) & (2 ** 64 - 1), int(seed) & (2 ** 64 - 1), int(flags), jitter_sigma, jitter_max,
                                  scale_low, scale_high, shift_range, o_inp.data_ptr(), o_gt.data_ptr(), o_rad.data_ptr(),
                                  params.data_ptr(), idx.data_ptr() if want_idx else None,
                                  cand.data_ptr() if cand is not None else None, cand_len, status.data_ptr(), _stream()),
               "pf_patch_batch")
    return o_inp, o_gt, o_rad, params, idx, cand


class DevicePatchData:
    """PatchData's batches without host work: the dataset lives on the device (uploaded once; every rank keeps all of it), the
    host draws one permutation per epoch and uploads it, and every batch is ONE `pf_patch_batch` launch on the current stream
    (gather, non-uniform subsample, jitter, rotation, scale, shift - csrc/data_aug.hip).  A batch is a pure function of (dataset,
    seed, step): under world > 1 a rank generates rows `shard_bounds` of it with their global patch slots.  The random numbers
    are the kernel's own counter-based stream, not numpy's: the distribution of PatchData's batches, not their values.

    bind(static_batch): later batches are written straight into these tensors (a captured step's inputs) and the same dict is
    yielded every time; unbound, every batch gets fresh tensors.  status(): the kernel's sticky word (a synchronisation)."""

    def __init__(self, inp: np.ndarray, gt: np.ndarray, radius: Optional[np.ndarray] = None, batch_size: int = 32,
                 num_point_patch: int = 256, use_random_input: bool = False, is_augment: bool = True,
                 jitter_sigma: float = 0.01, jitter_max: float = 0.03, num_batches: Optional[int] = None,
                 device: str = "cuda", seed: int = 2021, rank: int = 0, world: int = 1, scale_low: float = 0.8,
                 scale_high: float = 1.2, z_rotated: bool = False, shift_range: float = 0.0):
        from . import _lib
        from .dist import shard_bounds
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PuflowHipError("DevicePatchData assembles its batches in a HIP kernel: it needs a GPU device (no CPU fallback; "
                                      "PatchData is the host path)")
        _lib.load()
        inp, gt = np.asarray(inp, dtype=np.float32), np.asarray(gt, dtype=np.float32)
        if inp.ndim != 3 or gt.ndim != 3 or inp.shape[2] != 3 or gt.shape[2] != 3 or len(inp) != len(gt):
            raise ValueError("DevicePatchData: inp [M, n_in, 3] and gt [M, n_out, 3] expected")
        if (inp.shape[1] != num_point_patch and not use_random_input) or inp.shape[1] < num_point_patch:
            raise ValueError(f"DevicePatchData: {inp.shape[1]} input points per patch for num_point_patch={num_point_patch}"
                             f" (use_random_input={use_random_input})")
        radius = np.ones(len(inp), np.float32) if radius is None else np.asarray(radius, dtype=np.float32)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.inp, self.gt, self.radius = up(inp), up(gt), up(radius)
        self.batch_size, self.npoint, self.random_input = batch_size, num_point_patch, use_random_input
        self.is_augment, self.jitter_sigma, self.jitter_max = is_augment, jitter_sigma, jitter_max
        self.scale_low, self.scale_high, self.z_rotated, self.shift_range = scale_low, scale_high, z_rotated, shift_range
        self.num_batches = num_batches if num_batches is not None else len(inp) // batch_size
        self.rank, self.world, self.seed = rank, world, int(seed)
        self.lo, self.hi = shard_bounds(batch_size, rank, world)
        self.rng = np.random.default_rng(seed)                      # the same shuffles on every rank
        self.order = torch.zeros(len(inp), dtype=torch.int32, device=self.device)
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.params = torch.zeros((self.hi - self.lo, 16), dtype=torch.float32, device=self.device)    # of the latest batch
        self.step = 0                                               # batches produced so far, over all epochs
        self._bound = None

    def __len__(self) -> int:
        return self.num_batches

    @property
    def flags(self) -> int:
        f = PATCH_SUBSAMPLE if self.inp.shape[1] > self.npoint else 0
        if self.is_augment:
            f |= PATCH_JITTER | PATCH_ROTATE | PATCH_SCALE | (PATCH_Z_ROTATED if self.z_rotated else 0)
            f |= PATCH_SHIFT if self.shift_range > 0 else 0
        return f

    def bind(self, static_batch) -> None:
        """Write the batches that follow into static_batch's tensors (dict with the three keys, or None to unbind)."""
        if static_batch is not None:
            b, n_out = self.hi - self.lo, self.gt.shape[1]
            for k, shape in zip(KEYS, ((b, self.npoint, 3), (b, n_out, 3), (b,))):
                t = static_batch[k]
                if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.inp.device:
                    raise ValueError(f"DevicePatchData.bind: '{k}' is not a contiguous fp32 {shape} tensor on {self.inp.device}")
        self._bound = static_batch

    def status(self) -> int:
        """The sticky status word (PF_PATCH_ST_*: 1 = a patch ran out of distinct candidates, 2 = corrupt permutation), read
        and cleared.  Synchronises: call it where the host waits anyway (end of an epoch)."""
        st = int(self._status.item())
        if st:
            self._status.zero_()
        return st

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        M, bs = self.inp.shape[0], self.batch_size
        with torch.cuda.device(self.device):
            self.order.copy_(torch.from_numpy(self.rng.permutation(M).astype(np.int32)))       # once per epoch, stream-ordered
        for b in range(self.num_batches):
            bound = self._bound
            with torch.cuda.device(self.device):
                out = patch_batch(self.inp, self.gt, self.radius, self.order, (b * bs) % M + self.lo, self.hi - self.lo, self.npoint,
                                  self.step * bs + self.lo, self.seed, self.flags, self._status, self.jitter_sigma, self.jitter_max,
                                  self.scale_low, self.scale_high, self.shift_range,
                                  out=None if bound is None else tuple(bound[k] for k in KEYS), params=self.params)
            self.step += 1
            yield bound if bound is not None else dict(zip(KEYS, out[:3]))


class SyntheticDevicePatchData(DevicePatchData):
    """SyntheticPatchData's patches as a DevicePatchData."""

    def __init__(self, num_patches: int = 256, num_point_patch: int = 256, up_ratio: int = 4, seed: int = 2021, **kw):
        n_in = min(num_point_patch * 4, num_point_patch * up_ratio) if kw.get("use_random_input") else num_point_patch
        inp, gt = _synth_arrays(num_patches, num_point_patch, up_ratio, seed, n_in)
        super().__init__(inp, gt, num_point_patch=num_point_patch, seed=seed, **kw)
