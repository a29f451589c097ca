"""The pillar encoders' point decoration: what the pillar detectors run between voxelization and their first `nn.Linear` —
`PointVoxelStatsCalculator.forward` (the reference's mmdet3d_gaussian/models/voxel_encoders/utils.py:48-89; `DynamicPillarFeatureNet`
and, once per view, `PillarMVFFeatureNet`) and the decoration of `PillarFeatureNet.forward` (pillar_encoder.py:105-153).

The reference runs either as a chain of small torch ops (two `reduce_mapback`s, an outer product, a `stack`, `cat`s; sums, masks and a
`cat` over the padded voxel tensor).  Here `point_voxel_stats` is two launches — a voxel-ordered table of means and covariances, then
a point-ordered pass over the flat output — and `pillar_decorate` one (csrc/pillar_feat.hip).  Every output element
is one fixed fp32 operation sequence (include/gd3d.h): CUDA tensors go to the kernels on the current stream, CPU tensors to the
library's `_cpu` twins (csrc/pillar_feat_cpu.cpp), and the two agree bit for bit.  No gradient: the inputs are raw points.
"""
import ctypes

import torch
from torch import nn

from . import _host, scatter as _scatter
from .voxelize import _floats

CLUSTER_CENTER, CLUSTER_OFFSET, COVARIANCE, VOXEL_CENTER, VOXEL_OFFSET, POINT_COUNT, APPEND = 1, 2, 4, 8, 16, 32, 64   # GD3D_PVS_*
PD_CLUSTER_CENTER, PD_VOXEL_CENTER, PD_DISTANCE = 1, 2, 4                                                                  # GD3D_PD_*


@_host.memo
def _geometry(voxel_size, range_min):
    """(voxel_size, offset) as host float arrays; offset = voxel_size / 2 + range_min in double, rounded once (the modules' Python
    statement `self.vx / 2 + point_cloud_range[0]`, which torch then rounds to the tensor's fp32)"""
    return (ctypes.c_float * 3)(*voxel_size), (ctypes.c_float * 3)(*(v / 2 + lo for v, lo in zip(voxel_size, range_min)))


def _geom(voxel_size, point_cloud_range):
    vs = _floats(voxel_size, 3, 'voxel_size')
    rng = tuple(float(x) for x in point_cloud_range)
    if len(rng) < 3:
        raise RuntimeError(f'point_cloud_range must hold at least the 3 lower bounds, got {len(rng)} values')
    return _geometry(vs, rng[:3])


def stats_flags(with_cluster_center=True, with_cluster_center_offset=True, with_covariance=True, with_voxel_center=True,
                with_voxel_point_count=True, with_voxel_center_offset=True, append_features=False):
    return (CLUSTER_CENTER * bool(with_cluster_center) | CLUSTER_OFFSET * bool(with_cluster_center_offset) | COVARIANCE * bool(with_covariance)
            | VOXEL_CENTER * bool(with_voxel_center) | VOXEL_OFFSET * bool(with_voxel_center_offset) | POINT_COUNT * bool(with_voxel_point_count)
            | APPEND * bool(append_features))


def stats_width(flags, C=3):
    """columns of the output for these flags (C: the points' columns, counted with APPEND only)"""
    return (3 + 3 * bool(flags & CLUSTER_CENTER) + 3 * bool(flags & CLUSTER_OFFSET) + 9 * bool(flags & COVARIANCE) + 3 * bool(flags & VOXEL_CENTER)
            + 3 * bool(flags & VOXEL_OFFSET) + bool(flags & POINT_COUNT) + (C - 3) * bool(flags & APPEND))


def _index(scatter_or_coors, dev):
    """-> (coors, map, counts, order, seg) from a `Scatter` (the CUDA form) or from point rows (CPU tensors: the grouping comes from
    scatter._index_and_grouping_torch, whose torch ops run on the CPU; CUDA rows: a `Scatter` is built)"""
    s = scatter_or_coors
    if isinstance(s, torch.Tensor):
        if s.dim() != 2 or s.dtype.is_floating_point or s.dtype == torch.bool:
            raise RuntimeError(f'shape mismatch: coors must be an integer (N, ndim) tensor, got {s.dtype} {tuple(s.shape)}')
        if s.device != dev:
            raise RuntimeError(f'coors are on {s.device}, the points on {dev}')
        if s.is_cuda:
            s = _scatter.Scatter(s)
        else:
            if s.size(0) == 0:
                return s, None, None, None, None
            _, pmap, counts, (order, seg) = _scatter._index_and_grouping_torch(s.contiguous())
            return s, pmap, counts, order, seg
    elif not isinstance(s, _scatter.Scatter):
        raise RuntimeError(f'point_voxel_stats: expected a Scatter or the points\' coors, got {type(s).__name__}')
    if s.pts_coors.device != dev:
        raise RuntimeError(f'the Scatter is on {s.pts_coors.device}, the points on {dev}')
    if s._grouping is None:
        return s.pts_coors, None, None, None, None
    return (s.pts_coors, s.pts_voxel_maps, s.voxel_pts_counts) + tuple(s._grouping)


def point_voxel_stats(points, scatter_or_coors, voxel_size, point_cloud_range, with_cluster_center=True, with_cluster_center_offset=True,
                      with_covariance=True, with_voxel_center=True, with_voxel_point_count=True, with_voxel_center_offset=True,
                      append_features=False, out=None):
    """`PointVoxelStatsCalculator.forward` in at most two launches -> (N, width) fp32, the reference's channel order:

        xyz | c (with_cluster_center) | xyz - c (with_cluster_center_offset) | covariance, 9 (with_covariance) |
        voxel centre (with_voxel_center) | xyz - centre (with_voxel_center_offset) | count (with_voxel_point_count) |
        points[:, 3:] (append_features: the `torch.cat` of DynamicPillarFeatureNet.forward in the same launch)

    points : (N, C >= 3) floating point; columns 0..2 are x, y, z and are read through the row stride, so the reference's
             `features[:, :3]` view costs no copy.  Without append_features the other columns are ignored.
    scatter_or_coors : the `Scatter` of the points' rows (CUDA), or the rows themselves, (N, ndim) int32 / int64 with the last three
             columns z, y, x (required for CPU tensors, where `Scatter` has no path; accepted on CUDA, where a `Scatter` is built).
    c is the mean over the voxel's points in ascending point index, added in sequence in fp32 and divided once — the bits of
    `Scatter.reduce_mapback(xyz, 'mean')`; the covariance is the same mean of d_a * d_b with d from the rounded c; the centre is
    (float)coor * voxel_size + (voxel_size / 2 + range_min).  A dropped point (a negative entry in its row) gets c = 0, d = xyz,
    zero covariance, count 0, and the centre of its own row's values.  NaN and inf propagate as in the torch statements.
    out=(tensor, col) : write into columns [col, col + width) of a preallocated fp32 (N, total) tensor (unit column stride) and return
             that view: two views and trailing features land in one tensor without a `cat`.
    No gradient."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.size(1) < 3 or not points.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: points must be floating-point rows of at least 3 columns (x, y, z), got '
                           f'{getattr(points, "dtype", None)} {tuple(getattr(points, "shape", ()))}')
    flags = stats_flags(with_cluster_center, with_cluster_center_offset, with_covariance, with_voxel_center, with_voxel_point_count,
                        with_voxel_center_offset, append_features)
    N, dev = points.size(0), points.device
    C = points.size(1) if append_features else 3
    if C > 256:
        raise RuntimeError(f'points rows of {C} columns: at most 256 are supported')
    size, off = _geom(voxel_size, point_cloud_range)
    coors, pmap, counts, order, seg = _index(scatter_or_coors, dev)
    if coors.dim() != 2 or coors.size(0) != N or not 3 <= coors.size(1) <= 8:
        raise RuntimeError(f'shape mismatch: the points\' coors must be ({N}, 3..8), got {tuple(coors.shape)}')
    pts = points.detach()
    if pts.dtype != torch.float32:
        pts = pts.float()
    if N > 0 and (pts.stride(1) != 1 or pts.stride(0) < C):
        pts = pts.contiguous()
    if coors.dtype not in (torch.int32, torch.int64):
        coors = coors.long()
    coors = coors.contiguous()
    W = stats_width(flags, C)
    if out is None:
        res = torch.empty((N, W), dtype=torch.float32, device=dev)
    else:
        buf, col = out
        col = int(col)
        if not isinstance(buf, torch.Tensor) or buf.dim() != 2 or buf.size(0) != N or buf.dtype != torch.float32 or buf.device != dev or \
                col < 0 or col + W > buf.size(1) or (N > 0 and (buf.stride(1) != 1 or buf.stride(0) < buf.size(1))):
            raise RuntimeError(f'shape mismatch: out must be (an fp32 ({N}, >= {col + W}) tensor of unit column stride on {dev}, column), got '
                               f'{getattr(buf, "dtype", None)} {tuple(getattr(buf, "shape", ()))} at column {col}')
        res = buf[:, col:col + W]
    if N == 0:
        return res
    V = counts.numel()
    table = None
    if flags & (CLUSTER_CENTER | CLUSTER_OFFSET | COVARIANCE) and V > 0:
        table = torch.empty((V, 12 if flags & COVARIANCE else 3), dtype=torch.float32, device=dev)
    ptr = _host.ptr_or_null
    _host.call('gd3d_point_voxel_stats', dev,
               (pts.data_ptr(), N, pts.stride(0), C, coors.data_ptr(), int(coors.dtype == torch.int64), coors.size(1), ptr(pmap), ptr(counts),
                ptr(order), ptr(seg), V, size, off, flags, ptr(table), res.data_ptr(), res.stride(0)))
    return res


class PointVoxelStatsCalculator(nn.Module):
    """The reference's `PointVoxelStatsCalculator` (utils.py:7-89): same constructor, `out_channels` and
    forward(pts_xyz (N, 3), scatter) -> (N, out_channels), through `point_voxel_stats`."""

    def __init__(self, voxel_size, point_cloud_range, with_cluster_center=True, with_cluster_center_offset=True, with_covariance=True,
                 with_voxel_center=True, with_voxel_point_count=True, with_voxel_center_offset=True):
        super().__init__()
        self.voxel_size = list(_floats(voxel_size, 3, 'voxel_size'))
        self.point_cloud_range = [float(x) for x in point_cloud_range]
        _geom(self.voxel_size, self.point_cloud_range)            # a bad geometry raises here, not at the first forward
        self.flags = dict(with_cluster_center=bool(with_cluster_center), with_cluster_center_offset=bool(with_cluster_center_offset),
                          with_covariance=bool(with_covariance), with_voxel_center=bool(with_voxel_center),
                          with_voxel_point_count=bool(with_voxel_point_count), with_voxel_center_offset=bool(with_voxel_center_offset))

    @property
    def out_channels(self):
        return stats_width(stats_flags(**self.flags))

    def forward(self, pts_xyz, scatter, out=None):
        if pts_xyz.dim() != 2 or pts_xyz.size(1) != 3:
            raise RuntimeError(f'shape mismatch: pts_xyz must be (N, 3) — pass `features[:, :3]` — got {tuple(pts_xyz.shape)}')
        return point_voxel_stats(pts_xyz, scatter, self.voxel_size, self.point_cloud_range, out=out, **self.flags)

    def extra_repr(self):
        return f'voxel_size={self.voxel_size}, point_cloud_range={self.point_cloud_range}, ' + ', '.join(k for k, v in self.flags.items() if v)


def pillar_decorate(features, num_points, coors, voxel_size, point_cloud_range, with_cluster_center=True, with_voxel_center=True,
                    with_distance=False):
    """The decoration of `PillarFeatureNet.forward` (legacy=False) in one launch: features (V, P, C >= 3), num_points (V,), coors
    (V, 4) [b, z, y, x] -> (V, P, C + 3 * with_cluster_center + 3 * with_voxel_center + with_distance) fp32.

    For the slots p < min(num_points, P) of a voxel: the C input columns, then xyz - mean (the mean being `voxel_mean`'s fixed
    sequence: slots 0, 1, 2, .. added in order, one division), then xyz - ((float)coor * voxel_size + (voxel_size / 2 + range_min)),
    then sqrt((x*x + y*y) + z*z).  Every other slot is written as +0 and its input is not read: garbage there, NaN included, cannot
    leak, and a voxel with num_points == 0 (the tail rows of hard_voxelize(static=True)) gives zero rows where the reference's 0 / 0
    gives NaN.  No gradient."""
    if not isinstance(features, torch.Tensor) or features.dim() != 3 or features.size(2) < 3 or not features.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: features must be a floating-point (V, P, C >= 3) tensor, got {tuple(getattr(features, "shape", ()))}')
    V, P, C = features.shape
    if P < 1 or C > 256:
        raise RuntimeError(f'pillar_decorate: needs P >= 1 and C <= 256, got P={P}, C={C}')
    dev = features.device
    if not isinstance(num_points, torch.Tensor) or num_points.shape != (V,) or num_points.dtype.is_floating_point or num_points.dtype == torch.bool:
        raise RuntimeError(f'shape mismatch: num_points must be an integer ({V},) tensor, got {tuple(getattr(num_points, "shape", ()))}')
    if not isinstance(coors, torch.Tensor) or coors.shape != (V, 4) or coors.dtype.is_floating_point or coors.dtype == torch.bool:
        raise RuntimeError(f'shape mismatch: coors must be an integer ({V}, 4) tensor [b, z, y, x], got {tuple(getattr(coors, "shape", ()))}')
    if num_points.device != dev or coors.device != dev:
        raise RuntimeError(f'num_points is on {num_points.device}, coors on {coors.device}, features on {dev}')
    size, off = _geom(voxel_size, point_cloud_range)
    flags = PD_CLUSTER_CENTER * bool(with_cluster_center) | PD_VOXEL_CENTER * bool(with_voxel_center) | PD_DISTANCE * bool(with_distance)
    feats = _host.f32c(features.detach())
    cnt = num_points.to(torch.int32).contiguous()
    c32 = coors.to(torch.int32).contiguous()
    W = C + 3 * bool(with_cluster_center) + 3 * bool(with_voxel_center) + bool(with_distance)
    out = torch.empty((V, P, W), dtype=torch.float32, device=dev)
    ptr = _host.ptr_or_null
    _host.call('gd3d_pillar_decorate', dev, (ptr(feats), ptr(cnt), ptr(c32), V, P, C, size, off, flags, ptr(out)))
    return out


class PillarFeatureDecorator(nn.Module):
    """`PillarFeatureNet`'s decoration with its geometry arguments: forward(features (V, P, C), num_points, coors (V, 4)) -> the
    (V, P, C + ..) tensor its PFN layers take.  `legacy=True` (the in-place variant that overwrites the input's xyz) is not provided."""

    def __init__(self, with_distance=False, with_cluster_center=True, with_voxel_center=True, voxel_size=(0.2, 0.2, 4),
                 point_cloud_range=(0, -40, -3, 70.4, 40, 1), legacy=False):
        super().__init__()
        if legacy:
            raise RuntimeError('PillarFeatureDecorator: legacy=True is not provided (every shipped config uses legacy=False)')
        self.with_distance, self.with_cluster_center, self.with_voxel_center = bool(with_distance), bool(with_cluster_center), bool(with_voxel_center)
        self.voxel_size = list(_floats(voxel_size, 3, 'voxel_size'))
        self.point_cloud_range = [float(x) for x in point_cloud_range]

    def out_channels(self, in_channels):
        return in_channels + 3 * self.with_cluster_center + 3 * self.with_voxel_center + self.with_distance

    def forward(self, features, num_points, coors):
        return pillar_decorate(features, num_points, coors, self.voxel_size, self.point_cloud_range, self.with_cluster_center,
                               self.with_voxel_center, self.with_distance)
