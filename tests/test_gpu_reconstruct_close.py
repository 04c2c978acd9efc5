"""Band growth at the exits on the device against its numpy restatement (recon_grow_ref).  pf_recon_grow's `added` bytes, the
flags after every round, the vertices (bitwise), the faces, their order and the exits per round are exact: equal to the
restatement, which is fed the DEVICE's own implicit values so that a last-bit difference in f cannot change a sign between the
two sides.  The values at the grown corners are held to the float64 restatement by pf_imls's bound.  Then: the default path is
the call without the argument, a cloud without holes gives the unpadded mesh bit for bit, the clouds with holes come out closed,
the bound on the rounds holds, a rim stays a rim, and what cannot be done is refused by name."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import recon_grow_ref as G
import recon_ref as M

DEV = "cuda:0"
F = np.float32
ROUNDS = 8
CLOSED = {"sphere-512-0.7": (2, 2), "sphere-2048-0.5": (5, 2), "torus": (5, 0)}        # rounds that grow, V - E + F once closed


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _cloud(name):
    pts, nrm = G.cloud(name)
    return pts, nrm, _dev(pts), _dev(nrm)


@functools.lru_cache(maxsize=None)
def _call(name, rounds):
    """mesh_from_cloud(close_holes=rounds) on a cloud, on the host; rounds None: the call without the argument"""
    from puflow_amd import reconstruct as P
    _, _, p, n = _cloud(name)
    v, fa, info = P.mesh_from_cloud(p, n) if rounds is None else P.mesh_from_cloud(p, n, close_holes=rounds)
    return v.cpu(), fa.cpu(), info


@functools.lru_cache(maxsize=None)
def _device_rounds(name, rounds=ROUNDS):
    """mesh_from_cloud's loop by hand, stage by stage, with everything kept: the band and the device's f before the first round,
    then per round (f and flags as the kernel saw them, its `added`, the new corners, their queries, neighbours and values)"""
    from puflow_amd import ops, reconstruct as P
    pts, nrm, p, n = _cloud(name)
    h = P.cell_size(p)
    assert h == M.cell_size(pts)
    dims, tables = P.corner_tables(pts.min(axis=0).astype(np.float64), pts.max(axis=0).astype(np.float64), h, rounds=rounds)
    wdims, wtables = G.grid_of(pts, h, rounds)
    assert dims == wdims and all(a.tobytes() == b.tobytes() for a, b in zip(tables, wtables))
    dtables = [_dev(t) for t in tables]

    def value(corner):
        query = np.stack([tables[0][corner % dims[0]], tables[1][(corner // dims[0]) % dims[1]], tables[2][corner // (dims[0] * dims[1])]],
                         axis=1)
        idx, _ = ops.knn_grid(p[None], _dev(query)[None], 8)
        return query, idx[0].cpu().numpy(), ops.imls(_dev(query), p, n, idx[0], 1.0 * h)
    flags = ops.recon_mark(p, dtables)
    assert torch.equal(flags.cpu(), torch.from_numpy(M.mark(pts, tables)))
    corner = np.flatnonzero(flags.cpu().numpy().reshape(-1))
    f = torch.zeros(flags.shape, dtype=torch.float32, device=DEV)
    f.reshape(-1)[_dev(corner)] = value(corner)[2]
    start = (flags.cpu().numpy().copy(), f.cpu().numpy().copy())
    steps = []
    for _ in range(rounds):
        added = ops.recon_grow(f, flags)
        assert added.dtype == torch.uint8 and added.shape == flags.shape
        new = np.flatnonzero((added.cpu().numpy() != 0).reshape(-1) & (flags.cpu().numpy() == 0).reshape(-1))
        if len(new) == 0:
            break
        query, idx, val = value(new)
        steps.append(dict(f=f.cpu().numpy().copy(), flags=flags.cpu().numpy().copy(), added=added.cpu().numpy(), new=new, query=query,
                          idx=idx, value=val.cpu().numpy()))
        f.reshape(-1)[_dev(new)] = val
        flags |= added
    return dict(h=h, dims=dims, tables=tables, start=start, steps=steps, flags=flags.cpu().numpy(), f=f.cpu().numpy())


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,density", [(1, 0.85), (2, 0.6), (3, 0.95)])
def test_kernel_equals_the_restatement_on_a_random_field(seed, density):
    """19 x 10 x 9: no multiple of anything, more than one block of 256 lanes, exits on every side of active cells and next to the
    grid's last cells; nan where nothing is flagged changes no byte: f is read at the corners of active cells only"""
    from puflow_amd import ops
    f, flags = G.random_field(seed, density=density)
    act = M.active_cells(flags)
    assert ((f == 0) & np.signbit(f)).sum() > 100 and ((f == 0) & ~np.signbit(f)).sum() > 100
    assert act[-2, -2, -2] and act[0, 0, 0] and act[-2].sum() >= 4 and act[:, -2].sum() >= 4 and act[:, :, -2].sum() >= 4
    exits, want = G.grow(flags, f)
    assert exits.sum() > 50 and exits[-2].any() and exits[:, -2].any() and exits[:, :, -2].any()
    got = ops.recon_grow(_dev(f), _dev(flags))
    assert got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == want.tobytes()
    poisoned = f.copy()
    poisoned[flags == 0] = np.nan
    assert ops.recon_grow(_dev(poisoned), _dev(flags)).cpu().numpy().tobytes() == want.tobytes()
    assert not ops.recon_grow(_dev(f), _dev(np.ones_like(flags))).any()                     # every cell active: no exit
    assert not ops.recon_grow(_dev(f), _dev(np.zeros_like(flags))).any()                    # no cell active: no exit either


@pytest.mark.parametrize("name", ["sphere-512-0.7", "torus"])
def test_kernel_equals_the_restatement_at_every_round(name):
    run = _device_rounds(name)
    assert len(run["steps"]) == CLOSED[name][0]
    for step in run["steps"]:
        exits, want = G.grow(step["flags"], step["f"])
        assert exits.sum() > 0 and step["added"].tobytes() == want.tobytes()
    from puflow_amd import ops
    exits, want = G.grow(run["flags"], run["f"])                                             # and after the last: nothing
    assert exits.sum() == 0 and not ops.recon_grow(_dev(run["f"]), _dev(run["flags"])).any()


# ---- 2. the whole call --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CLOSED))
def test_whole_call_equals_the_restatement(name):
    run = _device_rounds(name)
    final = run["f"].reshape(-1)
    flags, f, grown, history = G.close(*run["start"], ROUNDS, lambda c: final[c])            # the device's own values
    assert len(history) == len(run["steps"]) == CLOSED[name][0]
    for r, step in enumerate(run["steps"]):                                                  # flags after each round
        assert np.array_equal(history[r], step["flags"] | step["added"])
    assert np.array_equal(flags, run["flags"]) and f.tobytes() == run["f"].tobytes()
    wverts, wfaces, _ = M.extract(f, flags, run["tables"])
    verts, faces, info = _call(name, ROUNDS)
    print(f"close {name}: h {info['h']:.5f} dims {info['dims']} exits {info['grown_cells']} V {len(verts)} F {len(faces)} open "
          f"{info['open_edges']} euler {M.euler(verts.numpy(), faces.numpy())} volume {M.volume(verts.numpy(), faces.numpy()):.4f}")
    assert faces.dtype == torch.int32 and torch.equal(faces, torch.from_numpy(wfaces))
    assert torch.equal(_bits(verts), torch.from_numpy(wverts.view(np.int32)))
    assert info["grown_cells"] == grown and info["grow_rounds"] == len(grown) and all(type(g) is int for g in info["grown_cells"])
    assert info["h"] == run["h"] and info["dims"] == run["dims"] and info["layout"] == "dense"
    # and that mesh is what the rounds are for: closed, of the right genus, pointing outwards; before, it was not
    faces = faces.numpy()
    assert info["open_edges"] == M.open_edges(faces) == 0 and M.is_oriented_manifold(faces)
    assert M.euler(verts.numpy(), faces) == CLOSED[name][1] and M.volume(verts.numpy(), faces) > 0
    assert _call(name, None)[2]["open_edges"] > 0 and G.exits_left(flags, f) == 0


@pytest.mark.parametrize("name", ["sphere-512-0.7", "torus"])
def test_implicit_value_at_the_grown_corners(name):
    """pf_imls's bar, |f - f_ref| <= 2^-23 |f_ref| + 2^-40 h, at corners up to three cells further from the points than the band's"""
    pts, nrm, _, _ = _cloud(name)
    run = _device_rounds(name)
    worst = 0.0
    for step in run["steps"]:
        want = M.imls(step["query"], pts, nrm, step["idx"], 1.0 * run["h"])
        err = np.abs(step["value"].astype(np.float64) - want)
        bound = 2.0 ** -23 * np.abs(want) + 2.0 ** -40 * run["h"]
        worst = max(worst, float(np.max(err / bound)))
        assert step["value"].dtype == F and (err <= bound).all()
        assert np.array_equal(run["f"].reshape(-1)[step["new"]], step["value"])               # they are what the mesh is cut from
    print(f"imls at grown corners {name}: {sum(len(s['new']) for s in run['steps'])} corners, max err / bound {worst:.3f}")


# ---- 3. what does not change ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere-512-0.7", "noisy", "disc"])
def test_zero_rounds_are_the_call_without_the_argument(name):
    (v, fa, info), (v0, f0, i0) = _call(name, None), _call(name, 0)
    assert torch.equal(_bits(v), _bits(v0)) and torch.equal(fa, f0) and info == i0
    assert info["grow_rounds"] == 0 and info["grown_cells"] == []
    from puflow_amd import reconstruct as P
    _, _, p, n = _cloud(name)
    vs, fs, _ = P.mesh_from_cloud(p, n, layout="sparse", close_holes=0)                     # no growth: any layout
    assert torch.equal(_bits(vs.cpu()), _bits(v)) and torch.equal(fs.cpu(), fa)


def test_nothing_to_grow_is_the_unpadded_mesh_bit_for_bit():
    (v0, f0, i0), (v4, f4, i4) = _call("noisy", None), _call("noisy", 4)
    assert i0["open_edges"] == 0 and len(f0) > 100
    assert torch.equal(_bits(v4), _bits(v0)) and torch.equal(f4, f0)
    assert i4["grow_rounds"] == 0 and i4["grown_cells"] == [] and i4["dims"] == tuple(d + 8 for d in i0["dims"])


def test_two_calls_give_the_same_bits():
    from puflow_amd import reconstruct as P
    _, _, p, n = _cloud("torus")
    v, fa, info = _call("torus", ROUNDS)
    for _ in range(2):
        v2, f2, i2 = P.mesh_from_cloud(p, n, close_holes=ROUNDS)
        assert torch.equal(_bits(v2.cpu()), _bits(v)) and torch.equal(f2.cpu(), fa) and i2 == info


# ---- 4. the bound and the rim ---------------------------------------------------------------------------------------------------
def test_eight_rounds_do_not_close_a_wide_hole():
    verts, faces, info = _call("sphere-2048-0.9", 8)
    print(f"sphere-2048-0.9: exits {info['grown_cells']} open {info['open_edges']} (without: {_call('sphere-2048-0.9', None)[2]['open_edges']})")
    assert info["grow_rounds"] == 8 and len(info["grown_cells"]) == 8 and min(info["grown_cells"]) > 0
    assert info["open_edges"] == M.open_edges(faces.numpy()) > 0


def test_a_rim_stays_a_rim():
    verts, faces, info = _call("disc", 3)
    before = _call("disc", None)[2]["open_edges"]
    print(f"disc: exits {info['grown_cells']} open {info['open_edges']} (without: {before})")
    assert info["grow_rounds"] == 3 and info["open_edges"] == M.open_edges(faces.numpy()) > 0 and before > 0
    assert M.euler(verts.numpy(), faces.numpy()) == 1
    # the band reaches two cells past a point, every round at most one more per axis (and one to spare for the roundings)
    assert np.abs(verts.numpy()[:, :2]).max() <= 1.0 + (2 + 3 + 1) * info["h"]


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    from puflow_amd import _lib, ops, reconstruct as P
    _, _, p, n = _cloud("sphere-512-0.7")
    with pytest.raises(_lib.PuflowHipError, match="close_holes = 2: growth needs the dense layout"):
        P.mesh_from_cloud(p, n, layout="sparse", close_holes=2)
    for bad in (-1, 65, 2.5, "3", None, True):
        with pytest.raises(_lib.PuflowHipError, match="close_holes"):
            P.mesh_from_cloud(p, n, close_holes=bad)
    # 16 points whose box is 406^3 corners at cell 1: under the dense cap as it is, over it with one round of padding
    rng = np.random.default_rng(3)
    far = rng.uniform(0, 399, (16, 3)).astype(F)
    far[0], far[1] = 0.0, 399.0
    q = _dev(far)
    for layout in ("dense", "auto"):
        with pytest.raises(_lib.PuflowHipError, match=r"close_holes = 1: growth needs the dense layout.*408 x 408 x 408"):
            P.mesh_from_cloud(q, q, cell=1.0, layout=layout, close_holes=1)
    assert P.mesh_from_cloud(p, n, layout="auto", close_holes=2)[2]["layout"] == "dense"    # auto under the cap: dense, and grown
    with pytest.raises(_lib.PuflowHipError, match="flags"):
        ops.recon_grow(torch.zeros(4, 4, 4, device=DEV), torch.zeros(4, 4, device=DEV, dtype=torch.uint8))
    with pytest.raises(_lib.PuflowHipError, match="recon_grow"):
        ops.recon_grow(torch.zeros(4, 4, 5, device=DEV), torch.zeros(4, 4, 4, device=DEV, dtype=torch.uint8))


# ---- 6. the CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_closes_the_file_and_stays_the_same_without_the_flag(tmp_path, capsys):
    from puflow_amd import metrics, reconstruct as P
    from puflow_amd.upsample import load_xyz
    pts, nrm, _, _ = _cloud("sphere-512-0.7")
    (tmp_path / "in").mkdir()
    np.savetxt(tmp_path / "in" / "sphere.xyz", np.concatenate([pts, nrm], axis=1).astype(np.float64), fmt="%.6f")
    base = ["--source", str(tmp_path / "in"), "--target"]
    P.main(base + [str(tmp_path / "closed"), "--close_holes", "2"])
    assert "open edges" not in capsys.readouterr().out
    verts, faces = metrics.read_off(tmp_path / "closed" / "sphere.off")
    assert M.open_edges(faces) == 0 and M.is_oriented_manifold(faces) and M.euler(verts, faces) == 2 and M.volume(verts, faces) > 0
    P.main(base + [str(tmp_path / "again"), "--close_holes", "2"])
    assert (tmp_path / "again" / "sphere.off").read_bytes() == (tmp_path / "closed" / "sphere.off").read_bytes()
    # without the flag: the open mesh, the line that says so, and the bytes of the library call without the argument
    P.main(base + [str(tmp_path / "open")])
    said = capsys.readouterr().out
    assert "sphere.off" in said and "open edges" in said
    rows = np.atleast_2d(load_xyz(str(tmp_path / "in" / "sphere.xyz")))
    xyz, n = _dev(rows[:, :3]), _dev(rows[:, 3:6])
    n = n / n.norm(dim=1, keepdim=True).clamp_min(1e-30)
    v, fa, info = P.mesh_from_cloud(xyz, n)
    assert info["open_edges"] > 0
    P.write_off(tmp_path / "want.off", v, fa)
    assert (tmp_path / "open" / "sphere.off").read_bytes() == (tmp_path / "want.off").read_bytes()
    P.main(base + [str(tmp_path / "zero"), "--close_holes", "0"])
    assert (tmp_path / "zero" / "sphere.off").read_bytes() == (tmp_path / "want.off").read_bytes()
    with pytest.raises(_lib_error(), match="growth needs the dense layout"):
        P.main(base + [str(tmp_path / "sparse"), "--close_holes", "2", "--layout", "sparse"])


def _lib_error():
    from puflow_amd import _lib
    return _lib.PuflowHipError
