"""Hard voxelization, dynamic voxelization and the mean voxel encoder: the first stage the data meets — `PVRCNN.voxelize` plus the
`HardSimpleVFE` call of `extract_feat` (the reference's mmdet3d_gaussian/models/detectors/pv_rcnn.py:43-49, 66-86), and the front of
every `hv_*` config (PointPillars, CenterPoint, PV-RCNN share mmdet3d's `Voxelization` op).

The reference loops over the samples in Python around mmdet3d's CUDA op, concatenates, pads the batch index in with one `F.pad` per
sample and reads `coors[-1, 0].item()` to learn the batch size.  Here the whole stacked batch is ONE stream-ordered call
(csrc/hard_voxel.hip): key, stable radix sort, two scans, one scatter, one mean.  mmdet3d is not pinned by the
reference; its published `hard_voxelize` is restated (include/gd3d.h) in its DETERMINISTIC order — voxels numbered by first appearance
in point order, the first `max_num_points` points of a voxel, the first `max_voxels` voxels of a sample — which is what mmdet3d's CPU
op and its `deterministic=True` GPU path return; runs replay bit for bit.  CUDA tensors go to the kernels on the current stream, CPU
tensors to the library's `_cpu` twins (csrc/hard_voxel_cpu.cpp: the sequential walk over a hash map).  No gradient: the reference
voxelizes under `no_grad`, and the encoder's input is raw points.
"""
import ctypes

import torch
from torch import nn

from . import _host, _lib


@_host.memo
def _geometry(voxel_size, point_cloud_range):
    """(voxel_size (3 floats), range_min (3 floats), grid_size (3 int32)) as host arrays; the grid is mmdet3d's module statement
    `torch.round((range[3:] - range[:3]) / voxel_size)` on fp32 host tensors"""
    vs = torch.tensor(voxel_size, dtype=torch.float32)
    rng = torch.tensor(point_cloud_range, dtype=torch.float32)
    grid = torch.round((rng[3:] - rng[:3]) / vs).long().tolist()
    if not all(float(v) > 0 for v in voxel_size) or not all(1 <= g <= (1 << 24) for g in grid):
        raise RuntimeError(f'voxel_size {voxel_size} over point_cloud_range {point_cloud_range} gives the grid {grid}: every '
                           'voxel size must be positive and every axis must hold 1 .. 2^24 cells')
    return (ctypes.c_float * 3)(*voxel_size), (ctypes.c_float * 3)(*point_cloud_range[:3]), (ctypes.c_int32 * 3)(*grid)


def _floats(v, n, name):
    v = tuple(float(x) for x in v)
    if len(v) != n:
        raise RuntimeError(f'{name} must hold {n} values, got {len(v)}')
    return v


def grid_size(voxel_size, point_cloud_range):
    """(Gx, Gy, Gz) = round((range[3:] - range[:3]) / voxel_size) in fp32, as mmdet3d's `Voxelization` module computes it"""
    return tuple(_geometry(_floats(voxel_size, 3, 'voxel_size'), _floats(point_cloud_range, 6, 'point_cloud_range'))[2])


def _stacked(points, points_batch_cnt, who):
    """the two input forms -> (rows (N, C) fp32 with unit column stride, counts (B,) int32 on the rows' device)"""
    if isinstance(points, (list, tuple)):
        if points_batch_cnt is not None:
            raise RuntimeError(f'{who}: points_batch_cnt belongs to the stacked form, not to a list of samples')
        if len(points) == 0:
            raise RuntimeError(f'{who}: points must be a non-empty list of (n, C) tensors')
        for p in points:
            if not isinstance(p, torch.Tensor) or p.dim() != 2 or p.size(1) != points[0].size(1) or p.device != points[0].device:
                raise RuntimeError(f'shape mismatch: every entry of points must be an (n, C) tensor of one width on one device, got '
                                   f'{tuple(getattr(p, "shape", ()))}')
        cnt = torch.tensor([p.size(0) for p in points], dtype=torch.int32)       # sizes the host knows: a copy TO the device
        points = points[0] if len(points) == 1 else torch.cat(list(points), dim=0)
        cnt = cnt.to(points.device, non_blocking=True)
    else:
        if not isinstance(points, torch.Tensor) or points.dim() != 2:
            raise RuntimeError(f'shape mismatch: points must be an (N, C) tensor or a list of them, got {tuple(getattr(points, "shape", ()))}')
        if points_batch_cnt is None:
            cnt = torch.tensor([points.size(0)], dtype=torch.int32).to(points.device, non_blocking=True)
        else:
            cnt = _host.counts_i32(points_batch_cnt, points, 'points_batch_cnt')
    if points.size(1) < 3 or not points.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: points must be floating-point rows of at least 3 columns (x, y, z), got '
                           f'{points.dtype} {tuple(points.shape)}')
    if points.size(1) > 256:
        raise RuntimeError(f'points rows of {points.size(1)} columns: at most 256 are supported')
    if cnt.numel() > 1024:
        raise RuntimeError(f'{cnt.numel()} samples in one call: at most 1024 are supported')
    points = points.detach()
    if points.dtype != torch.float32:
        points = points.float()
    if points.size(0) > 0 and (points.stride(1) != 1 or points.stride(0) < points.size(1)):
        points = points.contiguous()                                               # a row-strided view is read where it lies
    return points, cnt


_workspace_bytes = _host.memo(lambda n, b, mv: _lib.load().gd3d_hard_voxelize_workspace_bytes(n, b, mv))


def _launch(points, cnt, voxel_size, point_cloud_range, max_num_points, max_voxels, num_features, with_voxels, with_mean):
    """the one call -> dict of the upper-bound tensors (R = min(N, B * max_voxels) rows) and `num` (2,) int64 = (V, dropped points)"""
    size, lo, grid = _geometry(_floats(voxel_size, 3, 'voxel_size'), _floats(point_cloud_range, 6, 'point_cloud_range'))
    max_num_points, max_voxels = int(max_num_points), int(max_voxels)
    if max_num_points < 1 or max_voxels < 1:
        raise RuntimeError(f'hard_voxelize: max_num_points and max_voxels must be at least 1, got {max_num_points} and {max_voxels}')
    N, C, B, dev = points.size(0), points.size(1), cnt.numel(), points.device
    F = C if num_features is None else int(num_features)
    if with_mean and not 1 <= F <= C:
        raise RuntimeError(f'hard_voxelize: num_features must lie in [1, {C}], got {F}')
    if not with_voxels and not with_mean:
        raise RuntimeError('hard_voxelize: with_voxels=False needs with_mean=True (the mean is then the only feature output)')
    R = min(N, B * max_voxels)
    out = dict(voxels=torch.empty((R, max_num_points, C), dtype=torch.float32, device=dev) if with_voxels else None,
               mean=torch.empty((R, F), dtype=torch.float32, device=dev) if with_mean else None,
               coors=torch.empty((R, 4), dtype=torch.int32, device=dev), num_points=torch.empty((R,), dtype=torch.int32, device=dev),
               voxel_batch_cnt=torch.empty((B,), dtype=torch.int32, device=dev), num=torch.empty((2,), dtype=torch.int64, device=dev))
    work = torch.empty((_workspace_bytes(N, B, max_voxels),), dtype=torch.uint8, device=dev) if dev.type == 'cuda' else None
    ptr = _host.ptr_or_null
    _host.call('gd3d_hard_voxelize', dev,
               (ptr(points), N, points.stride(0) if N > 0 else C, C, ptr(cnt), B, size, lo, grid, max_num_points, max_voxels, F, ptr(work),
                ptr(out['voxels']), ptr(out['mean']), ptr(out['coors']), ptr(out['num_points']), ptr(out['voxel_batch_cnt']),
                out['num'].data_ptr()))
    return out


def hard_voxelize(points, voxel_size, point_cloud_range, max_num_points, max_voxels, points_batch_cnt=None, num_features=None,
                  with_voxels=True, with_mean=False, static=False):
    """mmdet3d's hard `Voxelization` for a whole batch in one call -> (voxels (V, P, C) fp32, coors (V, 4) int32 [b, z, y, x],
    num_points (V,) int32, voxel_batch_cnt (B,) int32), plus mean (V, num_features) fp32 when `with_mean`.

    points : a per-sample list of (n_b, C) tensors (the detectors' form), or stacked rows (N, C) grouped by sample with
             points_batch_cnt (B,) (None: one sample).  Columns 0, 1, 2 are x, y, z; all C columns are copied.  A row-strided view
             (`big[:, :4]`) is read where it lies.
    Semantics (restated, include/gd3d.h): grid = round((range[3:] - range[:3]) / voxel_size) in fp32 on the host; per axis
    c = floor((p - lo) / vs) in fp32 — one subtraction, one correctly rounded division, one floor — and a point is dropped unless
    0 <= c < grid on every axis, compared in floating point BEFORE any conversion (NaN, +-inf, 1e30 are dropped).  The kept points of a
    sample are walked in index order: a new cell becomes the sample's next voxel while fewer than `max_voxels` are numbered, otherwise
    the point is skipped — a `continue`, not a `break`: later points of numbered voxels still join them; a point takes slot
    num_points[v] while that is < `max_num_points` = P, otherwise it is skipped.  Unused slots are zero.  The samples' voxels follow
    one another as `torch.cat` lays them, the batch index is column 0 of `coors`.
    mean   : `HardSimpleVFE(num_features)` — voxels[:, :, :num_features].sum(1) / num_points with the sum FIXED as slots 0, 1, 2, ..
             added in sequence to +0 in fp32, then one division: the device, the CPU twin and a numpy fp32 loop agree bit for bit.
    with_voxels=False, with_mean=True skips the (V, P, C) tensor altogether (`voxels` is returned as None): PV-RCNN's only consumer of
             it is the mean.
    static=True returns the upper-bound tensors — R = min(N, B * max_voxels) rows, the rows at and past V holding coors -1, num_points
             0, zero features and mean — and reads nothing back: capturable in a hipGraph (record the stacked form with its counts
             resident on the device; the list form copies the sizes the host knows TO the device).  static=False slices to V with ONE read-back
             (the reference's `.item()` at pv_rcnn.py:49 disappears: B is known from the call).
    No gradient.  Empty samples, and a batch in which every point is dropped, are fine (V = 0)."""
    pts, cnt = _stacked(points, points_batch_cnt, 'hard_voxelize')
    out = _launch(pts, cnt, voxel_size, point_cloud_range, max_num_points, max_voxels, num_features, with_voxels, with_mean)
    names = ('voxels', 'coors', 'num_points')
    if not static:
        V = int(out['num'][0])                                                      # the one read-back
        for k in names + ('mean',):
            if out[k] is not None:
                out[k] = out[k][:V]
    res = tuple(out[k] for k in names) + (out['voxel_batch_cnt'],)
    return res + (out['mean'],) if with_mean else res


def dynamic_voxelize(points, voxel_size, point_cloud_range, points_batch_cnt=None):
    """mmdet3d's dynamic voxelization for a whole batch in one launch -> coors (N, 4) int32 [b, z, y, x] per point, all -1 for a
    dropped point (outside the grid, non-finite, or a row of no sample): the `coors` operand of `Scatter` / `scatter_index`, which the
    dynamic configs build from the op plus one `F.pad` per sample.  Same inputs and the same cell arithmetic as `hard_voxelize`."""
    pts, cnt = _stacked(points, points_batch_cnt, 'dynamic_voxelize')
    size, lo, grid = _geometry(_floats(voxel_size, 3, 'voxel_size'), _floats(point_cloud_range, 6, 'point_cloud_range'))
    N = pts.size(0)
    coors = torch.empty((N, 4), dtype=torch.int32, device=pts.device)
    ptr = _host.ptr_or_null
    _host.call('gd3d_dynamic_voxelize', pts.device, (ptr(pts), N, pts.stride(0) if N > 0 else 3, ptr(cnt), cnt.numel(), size, lo, grid, ptr(coors)))
    return coors


def voxel_mean(features, num_points, num_features=None):
    """`HardSimpleVFE.forward` on caller-held voxels: features (V, P, C), num_points (V,) -> (V, num_features) fp32, the first
    num_points slots added in sequence (see `hard_voxelize`); a voxel without points gives zeros"""
    if not isinstance(features, torch.Tensor) or features.dim() != 3 or not features.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: features must be a floating-point (V, P, C) tensor, got {tuple(getattr(features, "shape", ()))}')
    V, P, C = features.shape
    F = C if num_features is None else int(num_features)
    if P < 1 or not 1 <= F <= C or C > 256:
        raise RuntimeError(f'voxel_mean: needs P >= 1 and 1 <= num_features <= C <= 256, got P={P}, C={C}, num_features={F}')
    if not isinstance(num_points, torch.Tensor) or num_points.shape != (V,) or num_points.dtype.is_floating_point or \
            num_points.dtype == torch.bool:
        raise RuntimeError(f'shape mismatch: num_points must be an integer ({V},) tensor, got {tuple(getattr(num_points, "shape", ()))}')
    if num_points.device != features.device:
        raise RuntimeError(f'num_points is on {num_points.device}, features on {features.device}')
    feats = _host.f32c(features.detach())
    cnt = num_points.to(torch.int32).contiguous()
    mean = torch.empty((V, F), dtype=torch.float32, device=feats.device)
    ptr = _host.ptr_or_null
    _host.call('gd3d_voxel_mean', feats.device, (ptr(feats), ptr(cnt), V, P, C, F, ptr(mean)))
    return mean


class Voxelization(nn.Module):
    """mmdet3d's `Voxelization` layer: forward(points (n, C)) of ONE sample -> (voxels (V, P, C), coors (V, 3) int32 [z, y, x],
    num_points (V,) int32); with max_num_points == -1 or max_voxels == -1 the dynamic (n, 3) coors, -1 rows for dropped points.
    `max_voxels` may be a (train, test) pair, selected by `self.training`.  `deterministic` is accepted and ignored: the result is
    always the deterministic one (module docstring)."""

    def __init__(self, voxel_size, point_cloud_range, max_num_points, max_voxels=20000, deterministic=True):
        super().__init__()
        self.voxel_size = list(_floats(voxel_size, 3, 'voxel_size'))
        self.point_cloud_range = list(_floats(point_cloud_range, 6, 'point_cloud_range'))
        self.max_num_points = int(max_num_points)
        self.max_voxels = tuple(int(v) for v in max_voxels) if isinstance(max_voxels, (tuple, list)) else (int(max_voxels),) * 2
        if len(self.max_voxels) != 2:
            raise RuntimeError(f'max_voxels must be a number or a (train, test) pair, got {max_voxels!r}')
        self.deterministic = deterministic
        gx, gy, gz = grid_size(self.voxel_size, self.point_cloud_range)
        self.grid_size = torch.tensor([gx, gy, gz])
        self.pcd_shape = [gx, gy, 1]

    def forward(self, input):
        max_voxels = self.max_voxels[0] if self.training else self.max_voxels[1]
        if self.max_num_points == -1 or max_voxels == -1:
            return dynamic_voxelize(input, self.voxel_size, self.point_cloud_range)[:, 1:]
        voxels, coors, num_points, _ = hard_voxelize(input, self.voxel_size, self.point_cloud_range, self.max_num_points, max_voxels)
        return voxels, coors[:, 1:], num_points

    def extra_repr(self):
        return (f'voxel_size={self.voxel_size}, point_cloud_range={self.point_cloud_range}, max_num_points={self.max_num_points}, '
                f'max_voxels={self.max_voxels}, deterministic={self.deterministic}')


class HardSimpleVFE(nn.Module):
    """mmdet3d's `HardSimpleVFE`: forward(features (V, P, C), num_points (V,), coors) -> (V, num_features), the mean of the points of
    each voxel in the fixed summation order of `hard_voxelize`.  `coors` is accepted and not used, as in mmdet3d."""

    def __init__(self, num_features=4):
        super().__init__()
        self.num_features = int(num_features)

    def forward(self, features, num_points, coors=None):
        return voxel_mean(features, num_points, self.num_features)


def pvrcnn_voxelize(points, voxel_layer_cfg, training, with_mean=True):
    """`PVRCNN.voxelize` plus the voxel encoder for the whole batch in one call (pv_rcnn.py:43-49, 66-86) -> the reference's
    `voxel_dict` — voxels (V, P, C), num_points (V,), coors (V, 4) [b, z, y, x] — plus `voxel_features` (V, C) = HardSimpleVFE(C)
    (with_mean) and `batch_size` = len(points), which the reference reads back from coors[-1, 0] (and gets wrong when the last sample
    has no voxel).  voxel_layer_cfg: the config's `voxel_layer` dict (voxel_size, point_cloud_range, max_num_points, max_voxels as a
    number or a (train, test) pair); `training` selects the limit as `Voxelization` does."""
    if not isinstance(points, (list, tuple)) or len(points) == 0:
        raise RuntimeError('pvrcnn_voxelize: points must be the detector\'s non-empty list of (n, C) tensors')
    get = _host.cfg_get
    max_voxels = get(voxel_layer_cfg, 'max_voxels', 20000)
    if isinstance(max_voxels, (tuple, list)):
        max_voxels = max_voxels[0] if training else max_voxels[1]
    res = hard_voxelize(points, get(voxel_layer_cfg, 'voxel_size'), get(voxel_layer_cfg, 'point_cloud_range'),
                        get(voxel_layer_cfg, 'max_num_points'), max_voxels, with_mean=with_mean)
    out = dict(voxels=res[0], num_points=res[2], coors=res[1], batch_size=len(points))
    if with_mean:
        out['voxel_features'] = res[4]
    return out
