"""Tiled passes on the GPU: the box query and the cell assignment against numpy, the device tiling against its restatement,
PatchHelper.upsample_tiled (one tile = `upsample` bit for bit; several tiles: counts, ownership and the spacing invariant
min pairwise distance^2 >= min_t r2[t]) and the CLI's --tile_points."""
import filecmp

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tiles_ref as R
from puflow_amd.weights import synth_patches, synth_state_dict

DEV = "cuda:0"


@pytest.fixture(scope="module")
def net():
    from puflow_amd.interpflow import PointInterpFlow
    net = PointInterpFlow(3)
    net.load_state_dict(synth_state_dict(31))
    net.set_to_initialized_state()
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def helper():
    from puflow_amd.patch import PatchHelper
    return PatchHelper(256, 4)


def surface(n, seed):
    return (synth_patches(1, n, seed=seed, surface=True)[0] * 1.5 + 0.25).to(DEV)


def min_pair_sqd(p: torch.Tensor) -> float:
    """smallest squared distance between two different rows, float64 differences, in row blocks on the device"""
    p = p.double()
    n, best = p.shape[0], float("inf")
    step = max(1, (1 << 24) // n)
    for i0 in range(0, n, step):
        a = p[i0:i0 + step]
        d = ((a[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        d[torch.arange(a.shape[0], device=p.device), torch.arange(i0, i0 + a.shape[0], device=p.device)] = float("inf")
        best = min(best, float(d.min()))
    return best


def chamfer(a: torch.Tensor, b: torch.Tensor) -> float:
    from puflow_amd import ops
    return float(ops.nearest_distance(a[None], b[None]).mean() + ops.nearest_distance(b[None], a[None]).mean())


def test_box_query_equals_numpy():
    """1000 points, 7 boxes: infinite faces, an empty box, an inverted box, faces that pass exactly through points"""
    from puflow_amd import ops
    pts = synth_patches(1, 1000, seed=3, surface=False)[0]
    p = pts.numpy()
    inf = np.inf
    boxes = np.array([
        [-inf, -inf, -inf, inf, inf, inf],                               # everything
        [-inf, 0.0, -inf, 0.25, inf, inf],                               # half-open slabs
        [p[7, 0], p[7, 1], p[7, 2], p[7, 0], p[7, 1], p[7, 2]],          # one point: all six faces pass through it
        [p[11, 0], -inf, -inf, p[500, 0], inf, inf],                     # two faces on points (possibly inverted: then empty)
        [5.0, 5.0, 5.0, 6.0, 6.0, 6.0],                                  # empty: away from the cloud
        [0.5, 0.5, 0.5, -0.5, -0.5, -0.5],                               # empty: lo > hi
        [-0.3, -0.3, -0.3, 0.3, 0.3, 0.3],
    ], np.float32)
    counts, offsets, member = ops.box_query(pts.to(DEV), torch.from_numpy(boxes).to(DEV))
    want = R.box_members(p, boxes)
    assert counts.tolist() == [len(w) for w in want] and counts[0] == 1000 and counts[2] == 1 and counts[4] == 0 and counts[5] == 0
    assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    for t, w in enumerate(want):
        assert member.dtype == torch.int32 and np.array_equal(member[offsets[t]:offsets[t + 1]].cpu().numpy(), w), t


@pytest.mark.parametrize("n,tile_points,kind", [(2048, 512, "surface"), (1000, 128, "surface"), (1000, 128, "equal_coordinates"),
                                                (300, 512, "surface")])
def test_device_tiling_and_cell_assignment_equal_the_restatement(n, tile_points, kind):
    """kd_tiles on the device: order, offsets, tree and boxes; pf_kd_assign: the numpy descent for the cloud's own points (every
    split value is a point's coordinate: points exactly on a split) and for points off the cloud"""
    from puflow_amd import ops, tiles
    pc = synth_patches(1, n, seed=17)[0]
    if kind == "equal_coordinates":
        pc = torch.round(pc * 2) / 2 + 0
    order, offsets, (axis, split, L), boxes = tiles.kd_tiles(pc.to(DEV), tile_points)
    r_order, r_offsets, (r_axis, r_split), r_boxes = R.kd_tiles(pc.numpy(), tile_points)
    assert L == R.kd_depth(n, tile_points) and offsets == r_offsets.tolist()
    assert np.array_equal(order.cpu().numpy(), r_order)
    assert np.array_equal(axis.cpu().numpy(), r_axis) and np.array_equal(split.cpu().numpy(), r_split)
    assert np.array_equal(boxes.cpu().numpy(), r_boxes)
    other = synth_patches(1, 777, seed=18, surface=False)[0]
    for q in (pc, other):
        leaf = ops.kd_assign(q.to(DEV), axis, split, L)
        assert leaf.dtype == torch.int32 and np.array_equal(leaf.cpu().numpy(), R.kd_descend(q.numpy(), r_axis, r_split, L))
    if L:
        on_split = (pc.numpy()[:, None, :] == r_split[None, :, None]).any()
        assert on_split


def test_a_single_tile_is_upsample_bit_for_bit(net, helper):
    pc = surface(2048, 5)
    with torch.no_grad():
        want = helper.upsample(net, pc[None], npoint=8216, upratio=4)[0]
        for tp in (2048, 4096):
            assert torch.equal(helper.upsample_tiled(net, pc, 8216, upratio=4, tile_points=tp), want)
        got, stats = helper.upsample_tiled(net, pc, 8216, upratio=4, tile_points=2048, return_stats=True)
    assert torch.equal(got, want) and stats["tiles"] == 1 and stats["quota"] == [8216]


@pytest.fixture(scope="module")
def four_tiles(net, helper):
    pc = surface(2048, 7)
    with torch.no_grad():
        out, stats = helper.upsample_tiled(net, pc, 8216, upratio=4, tile_points=512, return_stats=True)
    return pc, out, stats


def check_tiled(out, stats, npoint):
    assert tuple(out.shape) == (npoint, 3) and bool(torch.isfinite(out).all())
    assert sum(stats["quota"]) == npoint and len(stats["quota"]) == stats["tiles"]
    r2 = stats["r2"].numpy()
    assert np.all(r2 <= np.float32(stats["h"]) * np.float32(stats["h"]))
    got = min_pair_sqd(stats["normalised"])
    print(f"tiles {stats['tiles']} colours {stats['colours']} h {stats['h']:.5f} min r2 {r2.min():.6e} min pair d2 {got:.6e} "
          f"working {stats['working']} candidates {stats['candidates']} quota {stats['quota']} context {stats['context']}")
    assert got >= float(r2.min()) * (1 - 1e-6), (got, float(r2.min()))


def test_four_tiles(four_tiles):
    """2048 points, tile_points = 512: exactly npoint finite rows, every row one of its tile's kept candidates and inside its
    tile's cell, quotas that sum to npoint, r2[t] <= h^2, and the invariant (the slack covers only the float64 re-computation of
    float32 distances)"""
    pc, out, stats = four_tiles
    assert stats["tiles"] == 4 and stats["core"] == [512] * 4 and stats["quota"] == [2054] * 4
    check_tiled(out, stats, 8216)
    boxes, kept, first = stats["boxes"], stats["kept"], stats["kept_first"]
    for t, rows in enumerate(torch.split(stats["normalised"], stats["quota"])):
        mine = kept[first[t]:first[t + 1]]
        assert bool((rows[:, None, :] == mine[None, :, :]).all(-1).any(1).all()), t
        assert bool(((rows >= boxes[t, :3]) & (rows <= boxes[t, 3:])).all()), t
    assert all(c > 0 for t, c in enumerate(stats["context"]) if stats["colour"][t] > 0)
    assert all(w >= c for w, c in zip(stats["working"], stats["core"]))


def test_tiles_per_pass_changes_nothing(net, helper, four_tiles):
    pc, out, _ = four_tiles
    with torch.no_grad():
        assert torch.equal(helper.upsample_tiled(net, pc, 8216, upratio=4, tile_points=512, tiles_per_pass=1), out)
        assert torch.equal(helper.upsample_tiled(net, pc, 8216, upratio=4, tile_points=512, tiles_per_pass=64), out)


def test_quality_next_to_the_untiled_pipeline_recorded(net, helper, four_tiles):
    """Recorded, not asserted (no derivation: the untiled pipeline on the same cloud is the yardstick; the figures are kept in
    profiles/tiled/quality.txt): min_t r2 against the untiled output's smallest pairwise distance^2, and the Chamfer distance
    tiled <-> untiled next to the one between two untiled runs on differently shuffled input."""
    pc, out, stats = four_tiles
    with torch.no_grad():
        plain = helper.upsample(net, pc[None], npoint=8216, upratio=4)[0]
        perm = torch.randperm(2048, generator=torch.Generator().manual_seed(1)).to(DEV)
        shuffled = helper.upsample(net, pc[perm][None], npoint=8216, upratio=4)[0]
    g = pc.mean(0)
    scale = float((pc - g).norm(dim=1).max())
    print(f"quality 2048 -> 8216, tile_points 512: min_t r2 {float(stats['r2'].min()):.6e} (normalised), untiled min pair d2 "
          f"{min_pair_sqd((plain - g) / scale):.6e}; Chamfer tiled-untiled {chamfer(out, plain):.6e}, untiled-untiled(shuffled input) "
          f"{chamfer(plain, shuffled):.6e}")
    assert tuple(plain.shape) == tuple(out.shape)


def test_above_the_cliff(net, helper):
    """16 384 points with tile_points = 4096 (the untiled merge of this cloud would leave the cooperative FPS kernel): it
    finishes; count, finiteness and the invariant"""
    pc = surface(16384, 9)
    with torch.no_grad():
        out, stats = helper.upsample_tiled(net, pc, 4 * 16384 + 24, upratio=4, tile_points=4096, return_stats=True)
    assert stats["tiles"] == 4 and max(stats["candidates"]) <= 262144
    check_tiled(out, stats, 4 * 16384 + 24)


def test_errors_name_the_tile(net, helper):
    from puflow_amd._lib import PuflowHipError
    pc = surface(2048, 7)
    with torch.no_grad(), pytest.raises(PuflowHipError, match=r"tile \d+: \d+ candidates in its cell, fewer than its share"):
        helper.upsample_tiled(net, pc, 200000, upratio=4, tile_points=512)


def test_cli_tile_points(tmp_path):
    """--tile_points unset: a directory's outputs are byte-identical to a run with the keyword absent; --tile_points 1024: the
    3000-point file is written with 3000 x 4 rows and the 900-point file beside it gets the bytes it gets without the option"""
    from puflow_amd import upsample as U
    src = tmp_path / "in"
    src.mkdir()
    sizes = {"a.xyz": 3000, "b.xyz": 900}
    for k, (name, n) in enumerate(sizes.items()):
        np.savetxt(src / name, (synth_patches(1, n, seed=60 + k)[0] * 2.0 - 0.5).numpy(), fmt="%.6f")
    sd = synth_state_dict(9)
    torch.save(sd, tmp_path / "ckpt.pt")
    for tag in ("absent", "unset", "tiled"):
        (tmp_path / tag).mkdir()
    U.upsampling([str(src / name) for name in sizes], str(tmp_path / "absent"), None, up_ratio=4, num_outlier=24, num_patch=256,
                 seed=2021, state_dict=sd)
    argv = ["--source", str(src), "--target", "", "--checkpoint", str(tmp_path / "ckpt.pt")]
    argv[3] = str(tmp_path / "unset")
    U.main(argv)
    argv[3] = str(tmp_path / "tiled")
    U.main(argv + ["--tile_points", "1024"])
    match, mismatch, errors = filecmp.cmpfiles(tmp_path / "absent", tmp_path / "unset", list(sizes), shallow=False)
    assert sorted(match) == sorted(sizes) and not mismatch and not errors
    assert filecmp.cmp(tmp_path / "absent" / "b.xyz", tmp_path / "tiled" / "b.xyz", shallow=False)
    tiled = np.loadtxt(tmp_path / "tiled" / "a.xyz")
    assert tiled.shape == (3000 * 4, 3) and np.isfinite(tiled).all()
    assert not filecmp.cmp(tmp_path / "absent" / "a.xyz", tmp_path / "tiled" / "a.xyz", shallow=False)
