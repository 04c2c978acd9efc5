"""CPU restatement of the weighted sample elimination (csrc/poisson.hip, puflow_amd/sampling.py) in numpy float32 and integers:
the neighbour graph with its integer edge weights, the sequential greedy process that DEFINES the result, and the phase / round
form the kernels run.  Indices are inside the pool; every function takes one pool."""
import heapq
import math

import numpy as np


def elimination_params(area, s, m):
    """(r_max, r_min) in float64."""
    t = float(m) / float(s)
    r_max = math.sqrt(float(area) / (2.0 * math.sqrt(3.0) * float(m)))
    return r_max, r_max * (1.0 - t * math.sqrt(t)) * 0.65


def constants(area, s, m):
    """(R2, inv, lo) as float32."""
    r_max, r_min = elimination_params(area, s, m)
    return np.float32((2.0 * r_max) * (2.0 * r_max)), np.float32(1.0 / (2.0 * r_max)), np.float32(2.0 * r_min)


def neighbour_graph(points, area, m, chunk=1024):
    """(offsets [s+1] int64, nbr [nnz] int32 ascending per row, q [nnz] int64) of one pool, points [s,3] float32."""
    p = np.ascontiguousarray(points, dtype=np.float32)
    s = len(p)
    R2, inv, lo = constants(area, s, m)
    one, zero = np.float32(1.0), np.float32(0.0)
    rows, cols, qs = [], [], []
    for a in range(0, s, chunk):
        d = p[None, :, :] - p[a:a + chunk, None, :]                       # float32
        d2 = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])
        near = d2 < R2
        near[np.arange(len(near)), np.arange(a, a + len(near))] = False
        r, c = np.nonzero(near)                                           # row-major: ascending column inside a row
        dist = np.sqrt(d2[r, c])
        x = np.maximum(one - np.maximum(dist, lo) * inv, zero)
        x2 = x * x
        x4 = x2 * x2
        x8 = x4 * x4
        assert x8.dtype == np.float32
        rows.append(r + a)
        cols.append(c)
        qs.append(np.rint(x8 * np.float32(65536.0)).astype(np.int64))
    rows, cols, qs = np.concatenate(rows), np.concatenate(cols), np.concatenate(qs)
    offsets = np.zeros(s + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=s), out=offsets[1:])
    return offsets, cols.astype(np.int32), qs


def weights(offsets, q):
    return np.add.reduceat(np.concatenate([q, [0]]), offsets[:-1]) * (np.diff(offsets) > 0)


def eliminate_sequential(offsets, nbr, q, m):
    """The definition: while more than m are alive, remove the alive i with the largest (w_i, smaller index first) and take
    q_ij off every alive neighbour.  -> the alive indices, ascending."""
    s = len(offsets) - 1
    w = weights(offsets, q).astype(np.int64).tolist()
    alive = [True] * s
    heap = [(-w[i], i) for i in range(s)]
    heapq.heapify(heap)
    nbr_l, q_l, off = nbr.tolist(), q.tolist(), offsets.tolist()
    left = s - m
    while left > 0:
        nw, i = heapq.heappop(heap)
        if not alive[i] or -nw != w[i]:
            continue                                                      # a stale entry
        alive[i] = False
        left -= 1
        for e in range(off[i], off[i + 1]):
            j = nbr_l[e]
            if alive[j]:
                w[j] -= q_l[e]
                heapq.heappush(heap, (-w[j], j))
    return np.nonzero(alive)[0]


def eliminate_phases(offsets, nbr, q, m):
    """What the kernels run.  -> (alive indices ascending, phases, rounds)."""
    s = len(offsets) - 1
    w = weights(offsets, q).astype(np.int64)
    idx = np.arange(s, dtype=np.int64)
    alive = np.ones(s, dtype=bool)
    row = np.repeat(idx, np.diff(offsets))
    col = nbr.astype(np.int64)
    phases = rounds = 0
    while alive.sum() > m:
        k = int(alive.sum()) - m
        key = (w << 32) | (0xFFFFFFFF - idx)
        tau = np.sort(key[alive])[::-1][k]
        phases += 1
        while True:
            key = (w << 32) | (0xFFFFFFFF - idx)
            cand = alive & (key > tau)
            if not cand.any():
                break
            rounds += 1
            beaten = np.zeros(s, dtype=bool)
            e = alive[row] & alive[col] & (key[col] > key[row])
            beaten[row[e]] = True
            pick = cand & ~beaten
            assert pick.any()
            e = pick[row] & alive[col]
            assert not pick[col[e]].any()                                 # no two neighbours in one round
            np.subtract.at(w, col[e], q[e])
            alive &= ~pick
    return np.nonzero(alive)[0], phases, rounds


def nn_distance_cv(p):
    """std / mean of the nearest-neighbour distance inside the set p [n,3] (float64)."""
    p = np.asarray(p, dtype=np.float64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    d = np.sqrt(d2.min(1))
    return float(d.std() / d.mean())


def square_pool(s, seed, triple=False):
    """s uniform points of the unit square (z = 0), float32; triple: points 1 and 2 are copies of point 0."""
    p = np.zeros((s, 3), dtype=np.float32)
    p[:, :2] = np.random.default_rng(seed).random((s, 2), dtype=np.float32)
    if triple:
        p[1] = p[0]
        p[2] = p[0]
    return p
