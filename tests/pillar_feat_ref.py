"""Restatements of the pillar encoders' point decoration for the tests of `point_voxel_stats` and `pillar_decorate`:

  * numpy, fp32, one rounded operation at a time (`stats_ref`, `decorate_ref`): the fixed sequence of include/gd3d.h written as array
    statements — the voxel's points added one rank at a time in ascending point index, one division — which the device and the `_cpu`
    twin must equal bit for bit;
  * torch (`stats_statements`, `decorate_statements`): the reference's statements (models/voxel_encoders/utils.py:48-89,
    pillar_encoder.py:105-153) written out over this package's `Scatter` / plain tensors, for the comparisons on the device.
"""
import numpy as np
import torch

FLAG_NAMES = ('with_cluster_center', 'with_cluster_center_offset', 'with_covariance', 'with_voxel_center', 'with_voxel_point_count',
              'with_voxel_center_offset')
ALL = {k: True for k in FLAG_NAMES}
F32 = np.float32


def same_bits(a, b):
    """equal shapes, dtypes and bits; for floats NaN must sit at the same places (payloads may differ)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != 'f':
        return bool((a == b).all())
    na, nb = np.isnan(a), np.isnan(b)
    bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool((na == nb).all() and (a.view(bits)[~na] == b.view(bits)[~nb]).all())


def offsets(voxel_size, point_cloud_range):
    """voxel_size / 2 + range_min in double, rounded once"""
    return np.array([float(v) / 2 + float(lo) for v, lo in zip(voxel_size, point_cloud_range[:3])], dtype=F32)


def group(coors):
    """sorted unique non-negative rows -> (map (N,) with -1 for dropped points, counts (V,), per-voxel lists of ascending point ids)"""
    coors = np.asarray(coors).astype(np.int64)
    keep = (coors >= 0).all(1) if len(coors) else np.zeros(0, bool)
    pmap = np.full(len(coors), -1, np.int64)
    if keep.any():
        rows, inv = np.unique(coors[keep], axis=0, return_inverse=True)
        pmap[keep] = inv.reshape(-1)
        V = len(rows)
    else:
        V = 0
    members = [np.flatnonzero(pmap == v) for v in range(V)]
    return pmap, np.array([len(m) for m in members], np.int64), members


def _sequential_mean(rows, members):
    """per voxel: its rows in ascending point id added in sequence to +0 in fp32, then one division"""
    out = np.zeros((len(members), rows.shape[1]), F32)
    for v, ids in enumerate(members):
        acc = np.zeros(rows.shape[1], F32)
        for i in ids:
            acc = acc + rows[i]
        out[v] = acc / F32(len(ids))
    return out


def stats_ref(points, coors, voxel_size, point_cloud_range, append_features=False, **flags):
    """numpy restatement of gd3d_point_voxel_stats -> (N, width) fp32"""
    f = dict(ALL)
    f.update(flags)
    points = np.asarray(points, F32)
    coors = np.asarray(coors)
    xyz = points[:, :3]
    N = len(xyz)
    pmap, counts, members = group(coors)
    dropped = pmap < 0
    cols = [xyz]
    with np.errstate(all='ignore'):
        if f['with_cluster_center'] or f['with_cluster_center_offset'] or f['with_covariance']:
            mean = _sequential_mean(xyz, members)
            c = np.zeros((N, 3), F32)
            c[~dropped] = mean[pmap[~dropped]]
            d = xyz - c
            if f['with_cluster_center']:
                cols.append(c)
            if f['with_cluster_center_offset']:
                cols.append(d)
            if f['with_covariance']:
                prod = (d[:, :, None] * d[:, None, :]).reshape(N, 9)
                cov_v = _sequential_mean(prod, members)
                cov = np.zeros((N, 9), F32)
                cov[~dropped] = cov_v[pmap[~dropped]]
                cols.append(cov)
        if f['with_voxel_center'] or f['with_voxel_center_offset']:
            vs, off = np.array(voxel_size, F32), offsets(voxel_size, point_cloud_range)
            ctr = np.stack([coors[:, -1 - k].astype(F32) * vs[k] + off[k] for k in range(3)], 1) if N else np.zeros((0, 3), F32)
            if f['with_voxel_center']:
                cols.append(ctr)
            if f['with_voxel_center_offset']:
                cols.append(xyz - ctr)
        if f['with_voxel_point_count']:
            cnt = np.zeros((N, 1), F32)
            cnt[~dropped, 0] = counts[pmap[~dropped]].astype(F32)
            cols.append(cnt)
    if append_features:
        cols.append(points[:, 3:])
    return np.concatenate(cols, 1).astype(F32)


def decorate_ref(features, num_points, coors, voxel_size, point_cloud_range, with_cluster_center=True, with_voxel_center=True, with_distance=False):
    """numpy restatement of gd3d_pillar_decorate -> (V, P, width) fp32; padded slots +0, never read"""
    features = np.asarray(features, F32)
    V, P, C = features.shape
    n = np.clip(np.asarray(num_points).astype(np.int64), 0, P)
    valid = np.arange(P)[None, :] < n[:, None]                                     # (V, P)
    f = np.where(valid[:, :, None], features, F32(0))                               # padded input is not read
    xyz = f[:, :, :3]
    cols = [f]
    with np.errstate(all='ignore'):
        if with_cluster_center:
            acc = np.zeros((V, 3), F32)
            for s in range(P):
                acc = np.where((s < n)[:, None], acc + xyz[:, s], acc)
            mean = np.where((n > 0)[:, None], acc / np.maximum(n, 1).astype(F32)[:, None], F32(0))
            cols.append(xyz - mean[:, None, :])
        if with_voxel_center:
            vs, off = np.array(voxel_size, F32), offsets(voxel_size, point_cloud_range)
            ctr = np.stack([np.asarray(coors)[:, 3 - k].astype(F32) * vs[k] + off[k] for k in range(3)], 1) if V else np.zeros((0, 3), F32)
            cols.append(xyz - ctr[:, None, :])
        if with_distance:
            cols.append(np.sqrt((xyz[..., 0] * xyz[..., 0] + xyz[..., 1] * xyz[..., 1]) + xyz[..., 2] * xyz[..., 2])[..., None])
    out = np.concatenate(cols, 2).astype(F32)
    return np.where(valid[:, :, None], out, F32(0))


# ---- the reference's statements over this package's ops (torch, any device) ---------------------------------------------------------

def stats_statements(pts_xyz, scatter, voxel_size, point_cloud_range, **flags):
    """PointVoxelStatsCalculator.forward written out over `Scatter.reduce_mapback` / `mapback`"""
    f = dict(ALL)
    f.update(flags)
    coors = scatter.pts_coors
    parts = [pts_xyz]
    if f['with_cluster_center'] or f['with_cluster_center_offset'] or f['with_covariance']:
        centre = scatter.reduce_mapback(pts_xyz, 'mean')
        diff = pts_xyz - centre
        if f['with_cluster_center']:
            parts.append(centre)
        if f['with_cluster_center_offset']:
            parts.append(diff)
        if f['with_covariance']:
            outer = (diff.unsqueeze(1) * diff.unsqueeze(2)).reshape(-1, 9)
            parts.append(scatter.reduce_mapback(outer, 'mean'))
    if f['with_voxel_center'] or f['with_voxel_center_offset']:
        half = [float(v) / 2 + float(lo) for v, lo in zip(voxel_size, point_cloud_range[:3])]
        cell = torch.stack([coors[:, -1 - k] * float(voxel_size[k]) + half[k] for k in range(3)], dim=-1)
        if f['with_voxel_center']:
            parts.append(cell)
        if f['with_voxel_center_offset']:
            parts.append(pts_xyz - cell)
    if f['with_voxel_point_count']:
        parts.append(scatter.mapback(scatter.voxel_pts_counts.unsqueeze(-1)))
    return torch.cat(parts, dim=-1)


def decorate_statements(features, num_points, coors, voxel_size, point_cloud_range, with_cluster_center=True, with_voxel_center=True,
                        with_distance=False):
    """the decoration of PillarFeatureNet.forward (legacy=False) written out: torch's own sum, the 0 / 1 mask at the end"""
    parts = [features]
    xyz = features[:, :, :3]
    if with_cluster_center:
        mean = xyz.sum(dim=1, keepdim=True) / num_points.to(features.dtype).view(-1, 1, 1)
        parts.append(xyz - mean)
    if with_voxel_center:
        half = [float(v) / 2 + float(lo) for v, lo in zip(voxel_size, point_cloud_range[:3])]
        centre = torch.stack([coors[:, 3 - k].to(features.dtype) * float(voxel_size[k]) + half[k] for k in range(3)], dim=-1)
        parts.append(xyz - centre.unsqueeze(1))
    if with_distance:
        parts.append(torch.norm(xyz, 2, 2, keepdim=True))
    full = torch.cat(parts, dim=-1)
    mask = num_points.view(-1, 1) > torch.arange(features.size(1), device=features.device).view(1, -1)
    return full * mask.unsqueeze(-1).to(full.dtype)
