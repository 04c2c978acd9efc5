"""Band growth at the exits (include/puflow_hip.h, "closing holes": pf_recon_grow and the host loop around it) restated in numpy
on top of recon_ref, which it leaves as it is: the shifted grid, the exit rule, one round, the loop, and the clouds with holes the
tests share.  Everything but the IMLS value is exact: the device's `added` bytes, its flags after every round, the vertices
(bitwise), the faces and their order and the exits per round must equal this."""
import numpy as np

import attr_ref as A
import recon_ref as M

F = np.float32
MAX_ROUNDS = 64


# ---- grid -----------------------------------------------------------------------------------------------------------------
def grid(lo, hi, h, rounds=0):
    """recon_ref.grid with `rounds` more corners of padding per side: D_a = ceil((hi_a - lo_a) / h) + 7 + 2 rounds and
    g_a[i] = float32(o_a + (i - rounds) h) with the unchanged o = lo - 3 h"""
    lo, hi, h, r = np.asarray(lo, F).astype(np.float64), np.asarray(hi, F).astype(np.float64), float(h), int(rounds)
    o = lo - M.PAD * h
    dims = [int(np.ceil((hi[a] - lo[a]) / h)) + 2 * M.PAD + 1 + 2 * r for a in range(3)]
    return tuple(dims), [(o[a] + (np.arange(dims[a], dtype=np.float64) - r) * h).astype(F) for a in range(3)]


def grid_of(pts, h, rounds=0):
    p = np.asarray(pts, F)
    return grid(p.min(axis=0), p.max(axis=0), h, rounds)


# ---- one round --------------------------------------------------------------------------------------------------------------
def _shift(a, axis, by):
    """a moved by `by` (+1 / -1) along axis, zeros coming in: out[i] = a[i - by]"""
    out = np.zeros_like(a)
    src, dst = [slice(None)] * 3, [slice(None)] * 3
    src[axis], dst[axis] = (slice(None, -1), slice(1, None)) if by > 0 else (slice(1, None), slice(None, -1))
    out[tuple(dst)] = a[tuple(src)]
    return out


def grow(flags, f):
    """flags uint8 / f float32 [D_z, D_y, D_x] -> (exits bool, added uint8), both [D_z, D_y, D_x].  An exit is an inactive cell
    (by lower corner, not on the last index of an axis) with a face neighbour inside the grid that is ACTIVE and whose shared
    face has four corners that do not all agree in f < 0; every exit puts 1 at its own 8 corners of `added`."""
    act = M.active_cells(flags)
    cell = np.zeros(flags.shape, bool)
    cell[:-1, :-1, :-1] = True
    inside = (np.asarray(f, F) < 0).astype(np.int8)                      # -0.0, +0.0 and nan: not inside
    exits = np.zeros(flags.shape, bool)
    for axis in range(3):
        b, c = [a for a in range(3) if a != axis]
        # the face with lower corner p across `axis`: corners p, p + e_b, p + e_c, p + e_b + e_c
        n = inside + _shift(inside, b, -1) + _shift(inside, c, -1) + _shift(_shift(inside, b, -1), c, -1)
        cross = (n != 0) & (n != 4)
        exits |= _shift(act, axis, 1) & cross                            # the neighbour below shares the face at the cell's corner
        exits |= _shift(act, axis, -1) & _shift(cross, axis, -1)         # the neighbour above the face one further
    exits &= cell & ~act
    added = np.zeros(flags.shape, np.uint8)
    k, j, i = np.nonzero(exits)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                added[k + dz, j + dy, i + dx] = 1
    return exits, added


def close(flags, f, rounds, value):
    """up to `rounds` rounds on copies of flags and f.  value(corner indices, ascending) -> the implicit values there.
    -> (flags, f, grown_cells: exits per round that added something, history: the flags after each of those rounds)"""
    flags, f = flags.copy(), np.asarray(f, F).copy()
    grown, history = [], []
    for _ in range(int(rounds)):
        exits, added = grow(flags, f)
        new = np.flatnonzero((added != 0) & (flags == 0)).astype(np.int64)
        if len(new) == 0:
            assert not exits.any()                                       # an exit is inactive: one of its corners is new
            break
        f.reshape(-1)[new] = np.asarray(value(new), F)
        flags |= added
        grown.append(int(exits.sum()))
        history.append(flags.copy())
    return flags, f, grown, history


# ---- the whole call ---------------------------------------------------------------------------------------------------------
def nearest(query, pts, k):
    """the k nearest points of every query by (fp32 squared distance, index), as recon_ref.mesh_from_cloud's stable sort gives
    them, from a partition: rows with a tie at the k-th distance go through the sort"""
    idx = np.empty((len(query), k), np.int64)
    for s in range(0, len(query), 4096):
        d = M.sqd(query[s:s + 4096, None], pts[None])
        part = np.argpartition(d, k - 1, axis=1)[:, :k]
        kth = np.take_along_axis(d, part, axis=1).max(axis=1)
        order = np.lexsort((part, np.take_along_axis(d, part, axis=1)), axis=1)
        idx[s:s + 4096] = np.take_along_axis(part, order, axis=1)
        for r in np.flatnonzero((d <= kth[:, None]).sum(axis=1) > k):
            idx[s + r] = np.argsort(d[r], kind="stable")[:k]
    return idx


def mesh_from_cloud(pts, normals, h, k=8, sigma=1.0, close_holes=0):
    """recon_ref.mesh_from_cloud on the grid padded for close_holes rounds, then the rounds, then ONE extraction"""
    pts = np.asarray(pts, F)
    dims, tables = grid_of(pts, h, close_holes)
    value = lambda x: M.imls(x, pts, normals, nearest(x, pts, k), sigma * h).astype(F)
    flags = M.mark(pts, tables)
    c, x = M.corners(flags, tables)
    f = np.zeros(flags.shape, F)
    f.reshape(-1)[c] = value(x)
    Dx, Dy = dims[0], dims[1]
    at = lambda c: np.stack([tables[0][c % Dx], tables[1][(c // Dx) % Dy], tables[2][c // (Dx * Dy)]], axis=1)
    flags, f, grown, history = close(flags, f, close_holes, lambda c: value(at(c)))
    verts, faces, _ = M.extract(f, flags, tables)
    return verts, faces, {"h": h, "dims": dims, "flags": flags, "f": f, "tables": tables, "grown_cells": grown,
                          "grow_rounds": len(grown), "history": history}


# ---- the clouds with holes ----------------------------------------------------------------------------------------------------
def sphere_with_hole(n, angle):
    """attr_ref's noiseless unit sphere of n points without the cap arccos(n_x) < angle: (points, normals) float32"""
    pts, nrm = A.surface("sphere", 0.0, n)
    keep = np.arccos(np.clip(nrm[:, 0], -1.0, 1.0)) >= angle
    return pts[keep], nrm[keep].astype(F)


def torus_with_hole(n=2048):
    """attr_ref's noiseless torus without the patch |atan2(y, x)| < 0.35, |atan2(z, hypot(x, y) - 1)| < 1"""
    pts, nrm = A.surface("torus", 0.0, n)
    p = pts.astype(np.float64)
    cut = (np.abs(np.arctan2(p[:, 1], p[:, 0])) < 0.35) & (np.abs(np.arctan2(p[:, 2], np.hypot(p[:, 0], p[:, 1]) - 1.0)) < 1.0)
    return pts[~cut], nrm[~cut].astype(F)


def cloud(name):
    """"sphere-512-0.7" (points, hole angle), "torus", "disc", "noisy" -> (points, normals) float32"""
    if name == "torus":
        return torus_with_hole()
    if name == "disc":
        pts, nrm = M.disc(512, 0)                                        # seed 0: the disc of the recorded figures (160 open edges)
        return pts, nrm.astype(F)
    if name == "noisy":
        pts, nrm = A.surface("sphere", 0.002, 512)
        return pts, nrm.astype(F)
    _, n, angle = name.split("-")
    return sphere_with_hole(int(n), float(angle))


def random_field(seed, shape=(9, 10, 19), density=0.85):
    """random values, a fifth of them exactly +0.0 / -0.0, random flags, and whole bricks of flags at both ends, so that active
    cells sit on the grid's first and last cells"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(shape).astype(F)
    z = rng.uniform(0, 1, shape)
    f[z < 0.1] = 0.0
    f[(z >= 0.1) & (z < 0.2)] = -0.0
    flags = (rng.uniform(0, 1, shape) < density).astype(np.uint8)
    flags[:3, :3, :3] = 1
    flags[-3:, -3:, -3:] = 1
    return f, flags


def exits_left(flags, f):
    return int(grow(flags, f)[0].sum())
