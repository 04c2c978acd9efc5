"""PatchHelper: the patch pipeline around the network - normalise, FPS seeds, K=256 kNN patches, network,
concatenate, FPS merge, de-normalise, outlier removal.  Mirrors the reference's surface and step order
(`modules/utils/patch.py:18-214`); FPS / kNN / Chamfer run in the HIP library, the rest is tensor re-layout
and O(points x 3) normalisation arithmetic in torch, as in the reference.
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import ops


class PatchHelper(object):

    def __init__(self, npoint_patch: int, patch_expand_ratio: float, extract: str = "knn"):
        if extract != "knn":
            raise NotImplementedError("only kNN patch extraction exists (as in the reference)")
        self._npoint_patch = npoint_patch
        self._patch_expand_ratio = patch_expand_ratio
        self.knn = ops.KNN(k=npoint_patch, transpose_mode=False)

    # ---- patch.py:35-80
    def upsample(self, upsampler, pc: Tensor, npoint: int, upratio=None, jitter: bool = False, **kwargs) -> Tensor:
        B, N, C = pc.shape
        pc, g_centroid, g_furthest_distance = PatchHelper.normalize_pc(pc)
        if jitter:
            pc = PatchHelper.jitter_perturbation_point_cloud(pc)
        patches = PatchHelper.extract_knn_patch(pc, self.knn, self._npoint_patch, self._patch_expand_ratio)
        patches = patches.reshape(B, -1, self._npoint_patch, C)
        predict_patches = PatchHelper.upsampling_patches(upsampler, patches, upratio, **kwargs)
        predict_pc = PatchHelper.merge_patches(predict_patches, npoint)            # [B,3,npoint]
        predict_pc = predict_pc * g_furthest_distance + g_centroid.transpose(1, 2)
        return predict_pc.transpose(1, 2).contiguous()

    # ---- patch.py:82-93
    @staticmethod
    def upsampling_patches(upsampler, patches: Tensor, upratio=None, **kwargs) -> Tensor:
        B, n_patch, k1, C = patches.shape
        patches = patches.reshape(B * n_patch, k1, C)
        patches, centroids, furthest_distance = PatchHelper.normalize_pc(patches)
        predict = upsampler.sample(patches.contiguous(), upratio=(upratio or 4), **kwargs)
        predict = torch.cat([predict, patches], dim=1)
        predict = predict * furthest_distance + centroids
        return predict.reshape(B, n_patch, -1, C)

    # ---- patch.py:95-125
    @staticmethod
    def extract_idx_patches(pc: Tensor, knn_searcher, npoint_patch: int, expand_ratio: float, seed_centroids_idx=None):
        _, N, _ = pc.shape
        pc_T = pc.transpose(1, 2).contiguous()
        if seed_centroids_idx is None:
            n_patch = int(N / npoint_patch * expand_ratio)
            patch_centroids_idx = ops.furthest_point_sample(pc, n_patch)
        else:
            n_patch = seed_centroids_idx.shape[1]
            patch_centroids_idx = seed_centroids_idx
        patch_centroids = ops.gather_operation(pc_T, patch_centroids_idx)          # [B,C,n_patch]
        _, idx_patches = knn_searcher(pc_T, patch_centroids)                       # [B,k,n_patch]
        return idx_patches, n_patch

    @staticmethod
    def extract_knn_patch(pc: Tensor, knn_searcher, npoint_patch: int, expand_ratio: float, seed_centroids_idx=None) -> Tensor:
        B, _, C = pc.shape
        idx_b = torch.arange(B, device=pc.device).view(-1, 1)
        idx_patches, n_patch = PatchHelper.extract_idx_patches(pc, knn_searcher, npoint_patch, expand_ratio, seed_centroids_idx)
        idx_patches = idx_patches.transpose(1, 2).flatten(start_dim=1)
        patches = pc[idx_b, idx_patches]
        return patches.reshape(B, n_patch, npoint_patch, C)

    @staticmethod
    def fps(pc: Tensor, n_point: int, transpose: bool = True) -> Tensor:
        idx = ops.furthest_point_sample(pc, n_point)
        cent = ops.gather_operation(pc.transpose(1, 2).contiguous(), idx)
        return cent.transpose(1, 2).contiguous() if transpose else cent

    # ---- patch.py:142-158
    @staticmethod
    def merge_patches(patches: Tensor, npoint: int, origins: Tensor = None) -> Tensor:
        B, _, per_patch, C = patches.shape
        patches = patches.reshape(B, -1, C)
        if origins is not None:
            patches = torch.cat([patches, origins], dim=1)
        patches = patches.contiguous()
        # layout hint (same indices, bit for bit): the candidates arrive patch after patch, `per_patch` consecutive points each
        idx = ops.furthest_point_sample(patches, npoint, group=per_patch if origins is None else 0)
        return ops.gather_operation(patches.transpose(1, 2).contiguous(), idx)     # [B,3,npoint]

    # ---- patch.py:168-178
    # ---- patch.py:162-165 (the reference uses its in-tree torch FPS here; same algorithm, see tests/golden/fps_ref.npz)
    @staticmethod
    def merge_pc(pc1: Tensor, pc2: Tensor, npoint: int) -> Tensor:
        tmp = torch.cat([pc1, pc2], dim=1).contiguous()
        idx = ops.furthest_point_sample(tmp, npoint).long()
        return tmp[torch.arange(tmp.shape[0], device=tmp.device).view(-1, 1), idx]

    @staticmethod
    def normalize_pc(pc: Tensor):
        if pc.is_cuda and pc.dim() == 3 and pc.shape[-1] == 3:
            return ops.normalize_pc(pc)          # fixed summation order: a cloud's result does not depend on the batch
        centroid = torch.mean(pc, dim=1, keepdim=True)
        pc = pc - centroid
        dist = torch.sum(pc ** 2, dim=-1, keepdim=True).sqrt()
        furthest_distance, _ = torch.max(dist, dim=1, keepdim=True)
        return pc / furthest_distance, centroid, furthest_distance

    @staticmethod
    def jitter_perturbation_point_cloud(pc: Tensor, sigma: float = 0.010, clip: float = 0.020) -> Tensor:
        if sigma <= 0:
            return pc
        B, N, C = pc.shape
        jit = torch.clamp(sigma * torch.randn(B, N, C, device=pc.device), -clip, clip)
        jit[:, :, 3:] = 0
        return jit + pc

    # ---- patch.py:198-214
    @staticmethod
    def remove_outliers(sr: Tensor, lr: Tensor, num_outliers: int) -> Tensor:
        (B, N, _), device = sr.shape, sr.device
        dist1 = ops.nearest_distance(sr, lr)       # = chamfer_3DDist()(sr, lr)[0] (patch.py:203 uses only dist1): half the work
        idx_outliers = torch.argsort(dist1, dim=-1, descending=True, stable=True)[:, :num_outliers]
        idxb = torch.arange(B, device=device).view(-1, 1)
        keep = torch.ones((B, N), dtype=torch.int32, device=device)
        keep[idxb, idx_outliers] = 0
        idx_inverse = torch.nonzero(keep, as_tuple=False)[:, 1].view(B, N - num_outliers)
        return sr[idxb, idx_inverse]

    # ---- ragged pass: clouds of different sizes through the pipeline together (no reference counterpart) ----
    @staticmethod
    def _rows(lengths, device):
        """For a packed tensor of these lengths: (first row of every cloud [B], cloud of every row [sum], row inside the cloud
        [sum]), built from the host lengths without a device -> host read."""
        cnt = torch.tensor(lengths, dtype=torch.int64)
        first = torch.cumsum(cnt, 0) - cnt
        total = int(cnt.sum())
        cnt, first = cnt.to(device), first.to(device)
        cloud = torch.repeat_interleave(torch.arange(len(lengths), device=device), cnt, output_size=total)
        return first, cloud, torch.arange(total, device=device) - first[cloud]

    def upsample_ragged(self, upsampler, clouds, npoints, upratio=None, names=None, **kwargs):
        """`upsample` for clouds of different sizes in ONE pass: clouds = list of [N_i, 3] GPU tensors, npoints = output size
        per cloud (a list, or one int for all) -> list of [npoint_i, 3].  Every cloud gets, bit for bit, what
        `upsample(upsampler, cloud[None], npoint_i, upratio)` gives it alone: the patches of all clouds go through the network
        as one batch, FPS / kNN / normalisation run as ragged launches (ops.*_ragged).  names: what to call the clouds in an
        error message (the CLI passes its file names)."""
        B, k = len(clouds), self._npoint_patch
        lengths = [int(c.shape[0]) for c in clouds]
        npoints = [int(npoints)] * B if isinstance(npoints, int) else [int(v) for v in npoints]
        for i, n in enumerate(lengths):
            if n < k:       # the dense path fails in its kNN (K > N): the same exception, before anything is launched
                raise ops._lib.PuflowHipError(f"{names[i] if names else 'cloud %d' % i}: {n} points, fewer than one patch ({k})")
        dev = clouds[0].device
        # every index helper depends on the sizes alone: built (and uploaded) before the first kernel of the pass is queued
        index = self._ragged_index(lengths, upratio, dev)
        cand_lengths, per_patch = index[3], index[4]
        m_first, _, _ = PatchHelper._rows(cand_lengths, dev)
        _, o_cloud, _ = PatchHelper._rows(npoints, dev)
        pc = torch.cat([c.reshape(-1, 3) for c in clouds], dim=0)
        pc, g_centroid, g_furthest_distance = ops.normalize_pc_ragged(pc, lengths)
        cand = self._ragged_candidates(upsampler, pc, lengths, upratio, index, **kwargs)
        idx = PatchHelper._ragged_merge(cand, cand_lengths, npoints, per_patch, m_first[o_cloud])
        out = cand[idx] * g_furthest_distance.view(B, 1)[o_cloud] + g_centroid.view(B, 3)[o_cloud]
        return list(torch.split(out, npoints))

    # The two halves of a ragged pass (upsample_ragged runs them back to back; upsample_tiled, tiles.py, puts the tiles'
    # ownership between them and merges with a context)
    def _ragged_index(self, lengths, upratio, dev):
        """What the candidate half needs of the sizes alone: (first row of every cloud, cloud of every patch, patches per cloud,
        candidates per cloud, candidates per patch)."""
        k = self._npoint_patch
        n_patch = [int(n / k * self._patch_expand_ratio) for n in lengths]
        c_first, _, _ = PatchHelper._rows(lengths, dev)
        _, p_cloud, _ = PatchHelper._rows(n_patch, dev)
        per_patch = k * ((upratio or 4) + 1)                                                   # sampled points + the patch itself
        return c_first, p_cloud, n_patch, [p * per_patch for p in n_patch], per_patch

    def _ragged_candidates(self, upsampler, pc: Tensor, lengths, upratio, index=None, **kwargs) -> Tensor:
        """Candidates of the clouds of a packed, already normalised tensor pc [sum lengths, 3]: FPS seeds, K-nearest patches,
        per-patch normalisation, network, concatenation with the patch -> [sum n_patch x per_patch, 3], cloud after cloud,
        patch after patch."""
        k = self._npoint_patch
        c_first, p_cloud, n_patch, _, per_patch = index if index is not None else self._ragged_index(lengths, upratio, pc.device)
        seeds = ops.furthest_point_sample_ragged(pc, lengths, n_patch).long() + c_first[p_cloud]
        _, idx_patches = ops.knn_ragged(pc, lengths, pc[seeds], n_patch, k)                    # [sum n_patch, k] inside the cloud
        patches = pc[idx_patches + c_first[p_cloud].view(-1, 1)]                               # [sum n_patch, k, 3]
        patches, centroids, furthest_distance = PatchHelper.normalize_pc(patches)
        predict = upsampler.sample(patches.contiguous(), upratio=(upratio or 4), **kwargs)
        predict = torch.cat([predict, patches], dim=1)
        predict = predict * furthest_distance + centroids                                      # [sum n_patch, per_patch, 3]
        if predict.shape[1] != per_patch:
            raise ValueError(f"the upsampler returned {predict.shape[1] - k} points per patch, expected {per_patch - k}")
        return predict.reshape(-1, 3).contiguous()

    @staticmethod
    def _ragged_merge(cand: Tensor, cand_lengths, npoints, group: int, first: Tensor) -> Tensor:
        """FPS merge of every cloud's candidates -> rows of cand, int64 [sum npoints] (first: the first candidate row of every
        output row's cloud)."""
        return ops.furthest_point_sample_ragged(cand, cand_lengths, npoints, group=group).long() + first

    def upsample_tiled(self, upsampler, pc: Tensor, npoint: int, upratio=None, tile_points: int = 4096, halo: float = 1.0,
                       tiles_per_pass: int = 64, return_stats: bool = False, **kwargs):
        """`upsample` for ONE large cloud pc [N, 3] -> [npoint, 3] in k-d tiles merged by FPS with a fixed context (tiles.py; no
        reference counterpart).  tile_points >= N: one tile, `upsample`'s tensor bit for bit."""
        from . import tiles
        return tiles.upsample_tiled(self, upsampler, pc, npoint, upratio=upratio, tile_points=tile_points, halo=halo,
                                    tiles_per_pass=tiles_per_pass, return_stats=return_stats, **kwargs)

    @staticmethod
    def remove_outliers_ragged(srs, lrs, num_outliers: int):
        """`remove_outliers` for lists of clouds of different sizes: srs[i] [n_i, 3] against lrs[i] [m_i, 3] -> list of
        [n_i - num_outliers, 3]; the same stable descending order per cloud, one nearest-neighbour pass for all."""
        B, dev = len(srs), srs[0].device
        ns, ms = [int(s.shape[0]) for s in srs], [int(l.shape[0]) for l in lrs]
        if min(ns) < num_outliers:
            raise ValueError(f"cannot remove {num_outliers} outliers from a cloud of {min(ns)} points")
        sr = torch.cat([s.reshape(-1, 3) for s in srs], dim=0)
        _, row_cloud, row_col = PatchHelper._rows(ns, dev)
        dist1 = ops.nearest_distance_ragged(sr, ns, torch.cat([l.reshape(-1, 3) for l in lrs], dim=0), ms)
        padded = torch.full((B, max(ns)), float("-inf"), dtype=torch.float32, device=dev)     # padding sorts behind every distance
        padded[row_cloud, row_col] = dist1
        idx_outliers = torch.argsort(padded, dim=-1, descending=True, stable=True)[:, :num_outliers]
        keep = torch.ones((B, max(ns)), dtype=torch.bool, device=dev)
        keep[torch.arange(B, device=dev).view(-1, 1), idx_outliers] = False
        return list(torch.split(sr[keep[row_cloud, row_col]], [n - num_outliers for n in ns]))
