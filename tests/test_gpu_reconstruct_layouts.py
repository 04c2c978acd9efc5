"""mesh_from_cloud's stage hook and the one extraction body under both layouts.  The hook must not change the call - the same
verts, faces and info, bit for bit - and must see exactly the documented stages of the layout in the order they run; extract /
extract_sparse on the call's own f and flags (rebuilt from what the hook saw: the compactions' indices and the IMLS stages'
values) must give the call's mesh again.  What the mesh itself has to be is the business of test_gpu_reconstruct*.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attr_ref as R

CASES = [("sphere-512-0.0", "dense", 0), ("sphere-512-0.0", "sparse", 0), ("torus-2048-0.002", "dense", 2)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _cloud(name):
    """the clouds of test_gpu_reconstruct.py by their names there: (points float32, unit normals float32)"""
    kind, n, sigma = name.split("-")
    pts, nrm = R.surface(kind, float(sigma), int(n))
    return pts, nrm.astype(np.float32)


def _documented(layout, rounds, info, faces):
    """the stages of mesh_from_cloud's docstring for a call that ended with this info and these faces"""
    names = ["cell-size search"] + (["block list"] if layout == "sparse" else []) + ["mark", "compaction", "K search", "IMLS"]
    names += ["grow", "compaction", "K search", "IMLS"] * info["grow_rounds"]
    if info["grow_rounds"] < rounds:                                        # the round that adds nothing ends the growth
        names += ["grow", "compaction"]
    return names + ["count"] + (["emit", "unique", "vertices"] if len(faces) else [])


@pytest.mark.parametrize("name,layout,rounds", CASES)
def test_the_hook_sees_the_documented_stages_and_changes_nothing(name, layout, rounds):
    from puflow_amd import reconstruct as P
    pts, nrm = _cloud(name)
    points, normals = _dev(pts), _dev(nrm)
    kw = dict(layout=layout, **({"close_holes": rounds} if rounds else {}))
    seen = []

    def stage(stage_name, thunk):
        out = thunk()
        seen.append((stage_name, out))
        return out
    verts, faces, info = P.mesh_from_cloud(points, normals, _stage=stage, **kw)
    plain = P.mesh_from_cloud(points, normals, **kw)
    assert torch.equal(verts.view(torch.int32), plain[0].view(torch.int32)) and torch.equal(faces, plain[1]) and info == plain[2]
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and len(faces) > 0
    assert [s for s, _ in seen] == _documented(layout, rounds, info, faces)
    assert info["layout"] == layout and (info["blocks"] > 0) == (layout == "sparse")

    # the call's own field: flags as the mark stage returned them (growth ors into that array), f from the values of every
    # IMLS stage at the indices of the compaction before it
    of = lambda which: [out for s, out in seen if s == which]
    flags = of("mark")[0]
    index = [i for i in of("compaction") if i.shape[0]]
    assert len(index) == len(of("IMLS")) == 1 + info["grow_rounds"]
    f = torch.zeros(flags.shape, dtype=torch.float32, device=flags.device)
    for i, value in zip(index, of("IMLS")):
        f.reshape(-1)[i] = value
    assert int(flags.sum()) == sum(int(i.shape[0]) for i in index)          # every flagged corner got its value, once
    dims, tables = P.corner_tables(pts.min(axis=0).astype(np.float64), pts.max(axis=0).astype(np.float64), info["h"], layout, rounds)
    assert dims == info["dims"]
    tables = [_dev(t) for t in tables]
    if layout == "sparse":
        blocks, links = of("block list")[0]
        assert blocks.shape[0] == info["blocks"]
        v, t = P.extract_sparse(f, flags, blocks, links, tables)
    else:
        v, t = P.extract(f, flags, tables)
    assert t.dtype == torch.int64
    assert torch.equal(v.view(torch.int32), verts.view(torch.int32)) and torch.equal(t.to(torch.int32), faces)
