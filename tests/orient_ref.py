"""The contract of pf_normals_orient (include/puflow_hip.h) restated on the CPU in numpy: the symmetrised edge set of the
neighbour lists, fp32 dots in the stated order, Kruskal with union-find over the strict key (w, min, max), a walk of the forest
from every component's seed for the parities, the seed rule and the smallest-index labels.  Everything is exact: the device's
output must equal this bit for bit.  The test surfaces come from attr_ref."""
import numpy as np

F = np.float32


def edge_dots(normals, a, b):
    """d_ab = ((nx_a*nx_b) + (ny_a*ny_b)) + (nz_a*nz_b), every operation rounded to float32"""
    n = np.asarray(normals, F)
    return (n[a, 0] * n[b, 0] + n[a, 1] * n[b, 1]) + n[a, 2] * n[b, 2]


def edges(idx):
    """the undirected edges {i, j}, i != j, with j in i's list or i in j's list: (a, b) with a < b, each once; entries outside
    the cloud are ignored"""
    idx = np.asarray(idx, np.int64)
    M, K = idx.shape
    i, j = np.repeat(np.arange(M), K), idx.reshape(-1)
    keep = (i != j) & (j >= 0) & (j < M)
    i, j = i[keep], j[keep]
    pair = np.unique(np.minimum(i, j) * M + np.maximum(i, j))
    return pair // M, pair % M


def forest(normals, idx):
    """-> (a, b, d of the minimum spanning forest's edges, root [M] of the union-find)"""
    M = len(normals)
    a, b = edges(idx)
    d = edge_dots(normals, a, b)
    w = np.maximum(F(0), F(1) - np.abs(d)).astype(F)
    parent = np.arange(M)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    taken = []
    for e in np.lexsort((b, a, w)):                                     # by w, then min, then max
        ra, rb = find(a[e]), find(b[e])
        if ra != rb:
            parent[ra] = rb
            taken.append(e)
    taken = np.asarray(taken, np.int64)
    return a[taken], b[taken], d[taken], np.array([find(x) for x in range(M)])


def orient(pts, normals, idx, viewpoint=None):
    """pts, normals [M,3], idx [M,K] -> (normals with consistent signs [M,3] float32, comp [M] int32)"""
    pts, normals = np.asarray(pts, F), np.asarray(normals, F)
    M = len(pts)
    ta, tb, td, root = forest(normals, idx)
    adj = [[] for _ in range(M)]
    for a, b, d in zip(ta, tb, td):
        adj[a].append((b, d < 0))
        adj[b].append((a, d < 0))
    if viewpoint is None:
        order = -(pts[:, 2] + F(0))                                     # the largest z first; -0 and +0 are one value
    else:
        v = np.asarray(viewpoint, F)
        dx, dy, dz = pts[:, 0] - v[0], pts[:, 1] - v[1], pts[:, 2] - v[2]
        order = (dx * dx + dy * dy) + dz * dz
    flip, comp = np.zeros(M, bool), np.empty(M, np.int32)
    for r in np.unique(root):
        members = np.flatnonzero(root == r)
        seed = members[np.lexsort((members, order[members]))[0]]        # the lowest index among equals
        n = normals[seed]
        if viewpoint is None:
            t = n[2]
        else:
            t = (n[0] * (v[0] - pts[seed, 0]) + n[1] * (v[1] - pts[seed, 1])) + n[2] * (v[2] - pts[seed, 2])
        flip[seed] = t < 0                                              # an exact 0: the seed keeps its input sign
        stack, seen = [seed], {seed}
        while stack:
            x = stack.pop()
            for y, neg in adj[x]:
                if y not in seen:
                    seen.add(y)
                    flip[y] = flip[x] ^ bool(neg)
                    stack.append(y)
        assert len(seen) == len(members)
        comp[members] = members.min()
    bits = normals.view(np.uint32) ^ (flip.astype(np.uint32) << np.uint32(31))[:, None]
    return bits.view(F), comp


def scramble(normals, seed):
    """the rows negated at random"""
    s = np.random.default_rng(seed).integers(0, 2, len(normals)).astype(F) * 2 - 1
    return (np.asarray(normals) * s[:, None]).astype(F)


def opposed(normals, analytic):
    """how many rows point against the analytic normal"""
    return int(((np.asarray(normals, np.float64) * analytic).sum(axis=1) < 0).sum())


def two_spheres(nested):
    """600 points of sphere(., 11) and 424 of sphere(., 13), the second beside the first (scaled by 0.5, moved to (3, 0, 0.2)) or
    nested in it (scaled by 0.4, concentric), and the analytic outward normals: two components, labels 0 and 600"""
    import attr_ref as R
    p0, n0 = R.sphere(600, 11)
    p1, n1 = R.sphere(424, 13)
    p1 = p1 * F(0.4) if nested else p1 * F(0.5) + np.array([3, 0, 0.2], F)
    return np.concatenate([p0, p1]).astype(F), np.concatenate([n0, n1])
