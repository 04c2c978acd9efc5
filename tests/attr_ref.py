"""numpy restatements, in float64, of the attribute blend (pf_attr_blend) and of the PCA normal (pf_normals_pca), with the test
surfaces the CPU and the GPU tests share.  The GPU tests feed `blend` the idx / d2 the device search returned and `pca` the
neighbourhoods it returned: the restatements pin the new kernels, not the search."""
import numpy as np

LIN, UNIT, NEAR = "lin", "unit", "near"


def blend(idx, d2, attr, plan):
    """idx, d2 [M,K] (ordered by distance), attr [N,C], plan [(kind, columns), ...] -> (out [M,C] float64, unit_len [M] float64:
    the length of the last unit segment's blend before it was normalised, 1 where there is none).
    w_k = (1 / d2_k) / sum_j (1 / d2_j); lin = sum_k w_k a_k; unit = sign-aligned to neighbour 0, blended, normalised (length 0 or
    not finite: neighbour 0's vector); near = neighbour 0's values; a row with d2_0 == 0 is neighbour 0's row."""
    idx, d2, attr = np.asarray(idx), np.asarray(d2, np.float64), np.asarray(attr, np.float64)
    M, K = idx.shape
    rows = attr[idx]                                                    # [M,K,C]
    exact = ~(d2[:, 0] > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = 1.0 / d2
        w = w / w.sum(axis=1, keepdims=True)
    w[exact] = 0.0
    out = np.empty((M, attr.shape[1]), np.float64)
    unit_len = np.ones(M, np.float64)
    c = 0
    for kind, n in plan:
        seg = rows[:, :, c:c + n]
        if kind == NEAR:
            out[:, c:c + n] = seg[:, 0]
        elif kind == LIN:
            out[:, c:c + n] = (w[:, :, None] * seg).sum(axis=1)
        else:
            assert kind == UNIT and n == 3
            sign = np.where((seg * seg[:, :1]).sum(axis=2) < 0, -1.0, 1.0)
            b = ((w * sign)[:, :, None] * seg).sum(axis=1)
            ln = np.sqrt((b * b).sum(axis=1))
            ok = (ln > 0) & np.isfinite(ln)
            with np.errstate(divide="ignore", invalid="ignore"):
                out[:, c:c + n] = np.where(ok[:, None], b / ln[:, None], seg[:, 0])
            unit_len = np.where(ok, ln, 1.0)
        c += n
    assert c == attr.shape[1]
    out[exact] = rows[exact, 0]
    return out, unit_len


def pca(pts, idx):
    """pts [M,3], idx [M,K] -> (normal [M,3] of arbitrary sign, variation [M] = l0 / (l0 + l1 + l2), gap [M] = (l1 - l0) / l2):
    numpy.linalg.eigh of the neighbourhood's covariance about its own centroid.  All moments 0: (0, 0, 1), variation 0, gap 0."""
    nb = np.asarray(pts, np.float64)[np.asarray(idx)]                   # [M,K,3]
    d = nb - nb.mean(axis=1, keepdims=True)
    cov = np.einsum("mki,mkj->mij", d, d) / idx.shape[1]
    lam, vec = np.linalg.eigh(cov)                                      # ascending
    flat = ~(lam.sum(axis=1) > 0)
    normal = np.where(flat[:, None], np.array([0.0, 0.0, 1.0]), vec[:, :, 0])
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.where(flat, 0.0, lam[:, 0] / lam.sum(axis=1))
        gap = np.where(flat, 0.0, (lam[:, 1] - lam[:, 0]) / lam[:, 2])
    return normal, var, gap


def orient(normal, pts, viewpoint=None):
    """the sign rule: dot(n, viewpoint - p) >= 0, or dot(n, p - centroid) >= 0 without a viewpoint"""
    pts = np.asarray(pts, np.float64)
    to = (np.asarray(viewpoint, np.float64) - pts) if viewpoint is not None else (pts - pts.mean(axis=0))
    return np.where(((normal * to).sum(axis=1) < 0)[:, None], -normal, normal)


def angle(a, b):
    """angle between the LINES along a and b [M,3] (sign-blind), from the cross product's norm, in float64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return np.arcsin(np.clip(s, 0.0, 1.0))


def knn_brute(pts, k):
    """the k nearest points of every point (itself included), by (distance, index): the CPU stand-in for the device search"""
    p = np.asarray(pts, np.float64)
    d = ((p[:, None] - p[None]) ** 2).sum(axis=2)
    return np.argsort(d, axis=1, kind="stable")[:, :k]


def sphere(n, seed, sigma=0.0):
    """n points on the unit sphere (float32) with Gaussian noise sigma, and their analytic normals (float64)"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v + sigma * rng.standard_normal((n, 3))).astype(np.float32), v


def torus(n, seed, sigma=0.0, R=1.0, r=0.35):
    """n points on the torus of radii R, r about the z axis, uniform by area (rejection on 1 + (r / R) cos v), with noise sigma"""
    rng = np.random.default_rng(seed)
    u, v = np.empty(0), np.empty(0)
    while v.size < n:
        cu, cv, t = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 1, n)
        keep = t * (R + r) <= R + r * np.cos(cv)
        u, v = np.concatenate([u, cu[keep]]), np.concatenate([v, cv[keep]])
    u, v = u[:n], v[:n]
    p = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=1)
    nrm = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], axis=1)
    return (p + sigma * rng.standard_normal((n, 3))).astype(np.float32), nrm


SURFACES = {"sphere": (sphere, 1.0), "torus": (torus, 0.35)}             # generator, smallest radius of curvature
PCA_CASES = [(name, sigma, k) for name in SURFACES for sigma in (0.0, 0.002) for k in (8, 16, 64)]
GAP_MIN = 1e-2                # rows whose relative eigenvalue gap is below this are not compared ...
GAP_SHARE = 0.01              # ... and at most this share of a case's rows may be


def surface(name, sigma, n=2048):
    gen, _ = SURFACES[name]
    return gen(n, seed=11 if name == "sphere" else 12, sigma=sigma)


def sagitta_bar(pts, idx, radius):
    """The chord-sagitta bound on the tilt of a plane fitted to a neighbourhood of a surface whose radius of curvature is at least
    `radius`: within a chord of half-length rho (the neighbourhood's farthest point) the surface leaves its tangent plane by at
    most the sagitta s = radius - sqrt(radius^2 - rho^2), so the plane tilts by at most atan(s / rho).  Mean over the points."""
    p = np.asarray(pts, np.float64)
    rho = np.sqrt(((p[idx] - p[:, None]) ** 2).sum(axis=2).max(axis=1))
    rho = np.minimum(rho, radius)
    return float(np.arctan((radius - np.sqrt(radius ** 2 - rho ** 2)) / rho).mean())
