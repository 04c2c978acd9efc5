"""numpy restatement of the random streams of `pf_patch_batch` (include/puflow_hip.h states the layout): Philox-4x32-10, the
word-to-uniform mapping, the patch parameters, the subsample candidates and their selection, the jitter noise.  Everything
takes a dtype: float64 is the reference the GPU tests compare against, float32 repeats the kernel's own roundings (libm's
log / sin / cos in place of the device's, so values agree to a few ulp, not bit for bit)."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
STREAM_PARAMS, STREAM_CAND, STREAM_JITTER = 0, 1, 2
MASK = np.uint64(0xFFFFFFFF)


def philox4x32(ctr, key):
    """ctr [..., 4], key [..., 2] (anything that casts to uint32) -> [..., 4] uint32, ten rounds."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) & MASK for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) & MASK for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def draw(seed, slot, stream, elems):
    """The four words of counters (elem, stream, slot lo, slot hi) under key (seed lo, seed hi); elems: int array -> [..., 4]."""
    e = np.asarray(elems, dtype=np.uint64)
    ctr = np.stack([e, np.full_like(e, stream), np.full_like(e, slot & 0xFFFFFFFF), np.full_like(e, (slot >> 32) & 0xFFFFFFFF)], -1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64), e.shape + (2,))
    return philox4x32(ctr, key)


def u01(x, dtype=np.float64):
    """(x >> 8) 2^-24 + 2^-25; in float32 with the kernel's rounding and its cap just below 1."""
    k = (np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(dtype)
    u = k * dtype(2.0 ** -24) + dtype(2.0 ** -25)
    return np.minimum(u, dtype(1 - 2.0 ** -24)) if dtype == np.float32 else u


def normal(x, y, which, dtype=np.float64):
    """Box-Muller on the words (x, y): which 0 -> r cos(2 pi u1), 1 -> r sin(2 pi u1)."""
    r = np.sqrt(dtype(-2.0) * np.log(u01(x, dtype)))
    th = dtype(2.0 * np.pi) * u01(y, dtype)
    return (r * np.where(np.asarray(which) == 1, np.sin(th), np.cos(th))).astype(dtype)


def patch_params(seed, slot, scale_low=0.8, scale_high=1.2, shift_range=0.0, dtype=np.float64):
    """-> dict(loc, angles [3] about x, y, z, scale, shift [3]) of one global patch slot."""
    q = draw(seed, slot, STREAM_PARAMS, np.arange(2))
    u0, u1 = u01(q[0], dtype), u01(q[1], dtype)
    sym = ((q[1] >> np.uint32(8)).astype(np.int64) * 2 + 1 - 2 ** 24).astype(dtype) * dtype(2.0 ** -24)      # 2u - 1, exact
    return dict(loc=dtype(0.1) + dtype(0.8) * u0[0], angles=dtype(2.0 * np.pi) * u0[1:4],
                scale=dtype(scale_low) + (dtype(scale_high) - dtype(scale_low)) * u1[0], shift=dtype(shift_range) * sym[1:4])


def rotation(angles, z_rotated=False):
    """Rz Ry Rx in float64 (applied as row vector times R)."""
    ax, ay, az = (float(a) for a in angles)
    if z_rotated:
        ax = ay = 0.0
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def candidates(seed, slot, n_in, count, dtype=np.float64):
    """The first `count` candidates of a slot's stream: int((loc + 0.3 z_p) n_in), truncated, out-of-range values included."""
    p = np.arange(count)
    q = draw(seed, slot, STREAM_CAND, p >> 2)
    hi = (p & 2) != 0
    z = normal(np.where(hi, q[:, 2], q[:, 0]), np.where(hi, q[:, 3], q[:, 1]), p & 1, dtype)
    loc = patch_params(seed, slot, dtype=dtype)["loc"]
    return np.trunc((loc + dtype(0.3) * z) * dtype(n_in)).astype(np.int64)


def select(cand, n_in, n, round_len=1024):
    """The parallel selection restated: the first n distinct values of `cand` inside [0, n_in), in stream order.
    -> (idx [n] - padded with its last value when the stream is too short, rounds of `round_len` consumed, short?)."""
    cand = np.asarray(cand, dtype=np.int64)
    pos = np.flatnonzero((cand >= 0) & (cand < n_in))
    vals, first = np.unique(cand[pos], return_index=True)              # first occurrence of every valid value
    keep = np.sort(pos[first])                                         # stream positions of the first occurrences, in order
    idx = cand[keep][:n]
    if len(idx) < n:
        pad = idx[-1] if len(idx) else 0
        return np.concatenate([idx, np.full(n - len(idx), pad, np.int64)]), -(-len(cand) // round_len), True
    return idx, keep[n - 1] // round_len + 1, False


def jitter_noise(seed, slot, n, sigma, clip, dtype=np.float64):
    """[n, 3]: clip(sigma z, -clip, clip) of output points 0..n-1."""
    q = draw(seed, slot, STREAM_JITTER, np.arange(n))
    z = np.stack([normal(q[:, 0], q[:, 1], 0, dtype), normal(q[:, 0], q[:, 1], 1, dtype), normal(q[:, 2], q[:, 3], 0, dtype)], -1)
    return np.clip(dtype(sigma) * z, -dtype(clip), dtype(clip))


def ks_statistic(a, b, bins):
    """Two-sample Kolmogorov-Smirnov statistic of integer samples in [0, bins)."""
    ca = np.cumsum(np.bincount(np.asarray(a).ravel(), minlength=bins)) / np.asarray(a).size
    cb = np.cumsum(np.bincount(np.asarray(b).ravel(), minlength=bins)) / np.asarray(b).size
    return float(np.abs(ca - cb).max())
