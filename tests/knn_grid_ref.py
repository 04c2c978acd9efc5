"""numpy restatement of the uniform-grid search (puflow_amd/csrc/knn_grid.hip) in the kernel's own float32 operations, the
float32 brute force it must equal, and the adversarial inputs both the CPU and the GPU tests run on.

Every arithmetic step is one np.float32 operation (numpy does not fuse), in the kernel's order: the choice of the cell edge h
and the cell counts G, cell_a, the ring search, and the stopping bound with its checked edges.  `STATS` counts what the search
did, among it how often a face's edge failed its own check (kg_face_bound: the face then gives 0) - the rounding argument says
never."""
import numpy as np

F = np.float32
GMAX = 256
CELLS_PER_POINT = 2
MAX_K = 64
STATS = {"unverified": 0, "faces": 0, "rings": 0, "candidates": 0, "queries": 0}


def axis_cells(n):
    g = 1
    while g < GMAX and g ** 3 < CELLS_PER_POINT * int(n):
        g += 1
    return g


def cell(x, lo, inv_h, G):
    """clamp((int)floorf((x - lo) * inv_h), 0, G - 1), x a float32 scalar or array"""
    with np.errstate(over="ignore"):
        t = np.floor((np.asarray(x, F) - F(lo)) * F(inv_h))
    return np.clip(t, F(0), F(G - 1)).astype(np.int64)


class Grid:
    def __init__(self, ref):
        ref = np.ascontiguousarray(ref, F)
        self.ref, self.n = ref, ref.shape[0]
        g = axis_cells(self.n)
        lo, hi = ref.min(axis=0), ref.max(axis=0)
        e = (hi - lo).max()
        ma = max(np.abs(lo).max(), np.abs(hi).max())
        h = F(e) / F(g)
        h = max(h, F(ma) * F(2.0 ** -19))
        h = max(h, F(2.0 ** -100))
        self.lo, self.h, self.inv_h = lo, F(h), F(1) / F(h)
        self.G = [int(cell(hi[a], lo[a], self.inv_h, g)) + 1 for a in range(3)]
        c = [cell(ref[:, a], lo[a], self.inv_h, self.G[a]) for a in range(3)]
        cid = (c[2] * self.G[1] + c[1]) * self.G[0] + c[0]
        self.order = np.argsort(cid, kind="stable")
        self.cstart = np.searchsorted(cid[self.order], np.arange(self.G[0] * self.G[1] * self.G[2] + 1))

    def cells_of(self, q):
        return [int(cell(q[a], self.lo[a], self.inv_h, self.G[a])) for a in range(3)]

    def face_bound(self, q, a, c, r):
        """(lower bound of the computed d2 beyond the block's faces of axis a, whether a face is interior)"""
        lo, h, G = self.lo[a], self.h, self.G[a]
        b, face = F(np.inf), False
        lc, hc = c - r, c + r
        if lc > 0:
            face = True
            E = lo + F(lc) * h
            E = E + max(abs(lo), abs(E)) * F(2.0 ** -20)
            gap = F(q) - E
            ok = int(cell(E, lo, self.inv_h, G)) >= lc
            STATS["faces"] += 1
            STATS["unverified"] += not ok
            b = min(b, gap * gap if ok and gap > 0 else F(0))
        if hc < G - 1:
            face = True
            E = lo + F(hc + 1) * h
            E = E - max(abs(lo), abs(E)) * F(2.0 ** -20)
            gap = E - F(q)
            ok = int(cell(E, lo, self.inv_h, G)) <= hc
            STATS["faces"] += 1
            STATS["unverified"] += not ok
            b = min(b, gap * gap if ok and gap > 0 else F(0))
        return F(b), face


def d2_f32(q, p):
    """((dx*dx)+(dy*dy))+(dz*dz), dx = q - p, every operation rounded to float32"""
    d = np.asarray(q, F)[None, :] - np.asarray(p, F)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def keys_of(d2, idx):
    return (d2.astype(F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)


def search(grid, q, K):
    """the K smallest keys of query q, as the kernel finds them -> (idx [K], d2 [K])"""
    q = np.asarray(q, F)
    G, cs = grid.G, grid.cstart
    cx, cy, cz = grid.cells_of(q)
    best = np.empty((0,), np.uint64)
    STATS["queries"] += 1
    r = 0
    while True:
        x0, x1 = max(cx - r, 0), min(cx + r, G[0] - 1)
        runs = []
        for z in range(max(cz - r, 0), min(cz + r, G[2] - 1) + 1):
            for y in range(max(cy - r, 0), min(cy + r, G[1] - 1) + 1):
                base = (z * G[1] + y) * G[0]
                if abs(z - cz) == r or abs(y - cy) == r:
                    runs.append((cs[base + x0], cs[base + x1 + 1]))
                else:
                    if cx - r >= 0:
                        runs.append((cs[base + cx - r], cs[base + cx - r + 1]))
                    if cx + r < G[0]:
                        runs.append((cs[base + cx + r], cs[base + cx + r + 1]))
        pos = [np.arange(s, e) for s, e in runs if e > s]
        if pos:
            idx = grid.order[np.concatenate(pos)]
            STATS["candidates"] += idx.size
            best = np.sort(np.concatenate([best, keys_of(d2_f32(q, grid.ref[idx]), idx)]))[:MAX_K]
        STATS["rings"] += 1
        bound, face = F(np.inf), False
        for a, c in enumerate((cx, cy, cz)):
            b, f = grid.face_bound(q[a], a, c, r)
            bound, face = min(bound, b), face or f
        if not face:
            break
        kth_hi = int(best[K - 1] >> np.uint64(32)) if best.size >= K else 0xFFFFFFFF
        if kth_hi < int(F(bound).view(np.uint32)):
            break
        r += 1
    best = best[:K]
    return (best & np.uint64(0xFFFFFFFF)).astype(np.int32), (best >> np.uint64(32)).astype(np.uint32).view(F)


def knn_grid(ref, query, K):
    grid = Grid(ref)
    out = [search(grid, q, K) for q in np.asarray(query, F)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def brute(ref, query, K):
    """float32 brute force ordered by (d2, index): np.lexsort((idx, d2))"""
    ref = np.ascontiguousarray(ref, F)
    idx_all = np.arange(ref.shape[0])
    I, D = [], []
    for q in np.asarray(query, F):
        d2 = d2_f32(q, ref)
        o = np.lexsort((idx_all, d2))[:K]
        I.append(o.astype(np.int32))
        D.append(d2[o])
    return np.stack(I), np.stack(D)


# ---- the inputs --------------------------------------------------------------------------------------------------------------
def sphere(n, seed):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def cases():
    """name -> (ref [N,3], query [M,3], the Ks), float32"""
    rng = np.random.default_rng(5)
    out = {}
    cube = rng.uniform(-1, 1, (300, 3)).astype(F)
    cube_q = np.concatenate([cube, rng.uniform(-1.1, 1.1, (700, 3)).astype(F)])
    out["cube"] = (cube, cube_q, (1, 3, 8, 16, 64))
    # 8 x 8 x 8 lattice, spacing 0.125: exact coordinates on cell edges; queries on lattice points, edge midpoints, cell centres
    i = np.arange(8)
    lat = (np.stack(np.meshgrid(i, i, i, indexing="ij"), axis=-1).reshape(-1, 3) * 0.125).astype(F)
    mid = lat[(lat[:, 0] < 0.8)] + np.array([0.0625, 0, 0], F)
    cen = lat[(lat < 0.8).all(axis=1)] + F(0.0625)
    out["lattice"] = (lat, np.concatenate([lat, mid, cen]).astype(F), (8, 16, 27))
    eight = rng.uniform(-1, 1, (8, 3)).astype(F)
    dup = np.tile(eight, (64, 1))
    out["duplicates"] = (dup, np.concatenate([eight, rng.uniform(-1, 1, (56, 3)).astype(F)]), (1, 16, 64))
    same = np.full((100, 3), 0.37, F)
    out["identical"] = (same, np.concatenate([same[:4], rng.uniform(-1, 1, (28, 3)).astype(F)]), (16,))
    plane = rng.uniform(-1, 1, (400, 3)).astype(F)
    plane[:, 2] = F(0.25)
    out["plane"] = (plane, np.concatenate([plane, rng.uniform(-1, 1, (200, 3)).astype(F)]), (8, 16))
    line = np.zeros((300, 3), F)
    line[:, 0] = rng.uniform(-1, 1, 300).astype(F)
    line[:, 1], line[:, 2] = F(0.5), F(-0.25)
    out["line"] = (line, np.concatenate([line, rng.uniform(-1, 1, (100, 3)).astype(F)]), (8,))
    # two tight clusters 100 extents apart; K = 64 from inside the 40-point one has to cross the empty gap
    small = rng.uniform(0, 0.01, (40, 3)).astype(F)
    large = (rng.uniform(0, 0.01, (1960, 3)) + np.array([1.0, 0, 0])).astype(F)
    out["clusters"] = (np.concatenate([small, large]), np.concatenate([small, large[:24]]), (8, 64))
    sph = sphere(5000, 11)
    out["sphere_self"] = (sph, sph, (16,))
    out["sphere_far"] = (sph, (sph * F(3)).astype(F), (8,))
    out["offset_4096"] = ((cube + F(4096)).astype(F), (cube_q + F(4096)).astype(F), (8,))
    far = (rng.uniform(0, 4, (300, 3)) + 2.0 ** 20).astype(F)                  # quantised to 0.125: duplicates, ties, h at its floor
    far_q = np.concatenate([far, (rng.uniform(-1, 5, (200, 3)) + 2.0 ** 20).astype(F)])
    out["offset_2p20"] = (far, far_q, (8, 16))
    out["above_chunk"] = (rng.uniform(-1, 1, (20000, 3)).astype(F), rng.uniform(-1, 1, (4096, 3)).astype(F), (16,))
    return out


def edge_cloud(offset=0.0, scale=1.0):
    """600 references of which 30 sit at -1, 0, +1 ulp around every interior cell edge of the x axis (the box is pinned by its
    two corners, the cell count by N), and queries at the same places -> (ref, query)"""
    rng = np.random.default_rng(17)
    n, extra = 600, 30
    base = (rng.uniform(0, 1, (n - extra, 3)) * scale + offset).astype(F)
    base[0], base[1] = F(offset), F(offset) + F(scale)
    g = axis_cells(n)
    assert g == 11 and extra == 3 * (g - 1)
    lo = base[:, 0].min()
    h = (base[:, 0].max() - lo) / F(g)
    pts = (rng.uniform(0, 1, (extra, 3)) * scale + offset).astype(F)
    for j in range(1, g):
        E = F(lo + F(j) * h)
        pts[3 * (j - 1):3 * j, 0] = [np.nextafter(E, F(-np.inf)), E, np.nextafter(E, F(np.inf))]
    ref = np.concatenate([base, pts]).astype(F)
    query = pts.copy()
    query[:, 1:] = (rng.uniform(0, 1, (extra, 2)) * scale + offset).astype(F)
    return ref, np.concatenate([query, pts])
