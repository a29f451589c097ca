"""Voxel query and `VoxelQueryAndGroup` — the pooling op of Voxel R-CNN and PV-RCNN++ (the published `VoxelQuery` /
`VoxelQueryAndGroup`) on top of the HIP kernels of csrc/voxel_query.hip (include/gd3d.h, gd3d_vsa_voxel_*).  The
reference ships the kernel (ops/vsa/src/voxel_query_gpu.cu:10-89) without a Python caller.

A query looks only at the cells of a window around its own cell: `xyz` (N, 3) holds one point per row of `coors` (N, 4)
[b, z, y, x] — the voxel centres of a sparse tensor and its `indices`, say — and the cells are looked up either in a
`VoxelQueryIndex` (sorted 64-bit keys, `voxel_query_index`) or in the reference's dense (B, Z, Y, X) table (`voxel_point_indices`).
`idx` holds GLOBAL rows of `xyz`; membership is inclusive (d2 <= radius2); a NaN distance is no member.

CUDA tensors go to the kernels on the current stream, CPU tensors to the library's `_cpu` twins (bit-identical outputs).  No wrapper
reads a value back, so every op can be captured in a hipGraph; the kernels skip whatever they cannot use (a query whose sample is
outside [0, B), a looked-up row outside [0, N), a row of `coors` outside the grid).
"""
import ctypes
import math
from typing import NamedTuple, Tuple

import torch

from . import _host, _lib
from ._host import ptr_or_null as _ptr, rows_f32 as _rows
from .vsa import _check_nsample

MAX_RANGE = 16


class VoxelQueryIndex(NamedTuple):
    """The sorted voxel index of `voxel_query_index`: skey (N,) int64 ascending, srow (N,) int32 the rows of `coors` in that order."""
    skey: torch.Tensor
    srow: torch.Tensor
    spatial_shape: Tuple[int, int, int]
    batch_size: int


def _grid(spatial_shape, batch_size):
    shape = tuple(int(s) for s in spatial_shape)
    if len(shape) != 3 or min(shape) < 1:
        raise RuntimeError(f'spatial_shape must be three positive extents (Z, Y, X), got {tuple(spatial_shape)}')
    b = int(batch_size)
    if b < 0:
        raise RuntimeError(f'batch_size must not be negative, got {batch_size}')
    return shape, b


def _coors(coors):
    if coors.dim() != 2 or coors.size(1) != 4 or coors.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f'shape mismatch: coors must be an int32 or int64 (N, 4) tensor [b, z, y, x], got {coors.dtype} {tuple(coors.shape)}')
    return coors.detach().contiguous()


_index_workspace_bytes = _host.memo(lambda n: _lib.load().gd3d_vsa_voxel_index_workspace_bytes(n))


def voxel_query_index(coors, spatial_shape, batch_size):
    """coors (N, 4) int32 / int64 [b, z, y, x] -> VoxelQueryIndex: the keys ((b * Z + z) * Y + y) * X + x sorted ascending (stable:
    of several rows in one cell the lowest comes first) with their rows.  A row with any coordinate outside the grid gets the key
    B * Z * Y * X, sorts last and is never found.  One stream-ordered call, no read-back."""
    c = _coors(coors)
    (z, y, x), b = _grid(spatial_shape, batch_size)
    n, dev = c.size(0), c.device
    skey = torch.empty((n,), dtype=torch.int64, device=dev)
    srow = torch.empty((n,), dtype=torch.int32, device=dev)
    if n > 0:
        work = torch.empty((_index_workspace_bytes(n),), dtype=torch.uint8, device=dev) if dev.type == 'cuda' else None
        _host.call('gd3d_vsa_voxel_index', dev,
                   (_ptr(c), int(c.dtype == torch.int64), n, b, z, y, x, _ptr(work), _ptr(skey), _ptr(srow)))
    return VoxelQueryIndex(skey, srow, (z, y, x), b)


def voxel_point_indices(coors, spatial_shape, batch_size):
    """coors (N, 4) -> the reference's dense table (B, Z, Y, X) int32: the row of each cell or -1; of several rows in one cell the
    lowest.  A fill and one launch; B * Z * Y * X * 4 bytes — at PV-RCNN's first level 369 MB per sample: prefer `voxel_query_index`."""
    c = _coors(coors)
    (z, y, x), b = _grid(spatial_shape, batch_size)
    table = torch.empty((b, z, y, x), dtype=torch.int32, device=c.device)
    if table.numel() > 0:
        _host.call('gd3d_vsa_voxel_table', c.device, (_ptr(c), int(c.dtype == torch.int64), c.size(0), b, z, y, x, _ptr(table)))
    return table


def voxel_query_coords(new_xyz, new_xyz_batch_cnt, voxel_size, point_cloud_range, scale_factor=1):
    """new_xyz (M, 3) stacked with new_xyz_batch_cnt (B,) -> new_coords (M, 4) int32 [b, z, y, x]: the cell of every query on the grid
    of cells `voxel_size * scale_factor` (x, y, z; rounded once to fp32) from `point_cloud_range[:3]`.  Per axis
    c = floor((p - lo) / cell) in fp32 (hard_voxelize's sequence).  b comes from the counts (no `repeat_interleave`, no sync); a row
    past the counts' sum, or with a coordinate for which -2^30 <= c < 2^30 does not hold (NaN, inf), gets b = -1.  Cells outside the
    grid are not clamped: their window may still reach in."""
    q = _rows(new_xyz, 3, 'new_xyz')
    qc = _host.counts_i32(new_xyz_batch_cnt, q, 'new_xyz_batch_cnt')
    vs = [float(v) * float(scale_factor) for v in voxel_size]
    lo = [float(v) for v in point_cloud_range[:3]]
    if len(vs) != 3 or len(lo) != 3 or not all(v > 0 and math.isfinite(v) for v in vs) or not all(math.isfinite(v) for v in lo):
        raise RuntimeError(f'voxel_query_coords: voxel_size * scale_factor must be three positive values and point_cloud_range finite, '
                           f'got {vs} and {list(point_cloud_range)}')
    m = q.size(0)
    out = torch.empty((m, 4), dtype=torch.int32, device=q.device)
    if m > 0:
        f3 = ctypes.c_float * 3
        _host.call('gd3d_vsa_voxel_coords', q.device, (_ptr(q), _ptr(qc), qc.numel(), m, f3(*vs), f3(*lo), _ptr(out)))
    return out


def _check_range(max_range):
    r = tuple(int(v) for v in max_range)
    if len(r) != 3 or not all(0 <= v <= MAX_RANGE for v in r):
        raise RuntimeError(f'max_range must be three values (rz, ry, rx) in [0, {MAX_RANGE}], got {tuple(max_range)}')
    return r


def _check_query(xyz, new_xyz, new_coords, index):
    """-> (xyz, new_xyz, new_coords, skey | None, srow | None, table | None, (B, Z, Y, X)) normalised; every mismatch raises."""
    x = _rows(xyz, 3, 'xyz')
    q = _rows(new_xyz, 3, 'new_xyz')
    dev = x.device
    if q.device != dev:
        raise RuntimeError(f'xyz is on {dev}, new_xyz on {q.device}')
    if new_coords.dim() != 2 or new_coords.size(1) != 4 or new_coords.size(0) != q.size(0) or new_coords.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f'shape mismatch: new_coords must be an integer ({q.size(0)}, 4) tensor [b, z, y, x], got {new_coords.dtype} '
                           f'{tuple(new_coords.shape)}')
    if new_coords.device != dev:
        raise RuntimeError(f'new_coords is on {new_coords.device}, xyz on {dev}')
    nc = new_coords.detach().to(torch.int32).contiguous()
    if isinstance(index, VoxelQueryIndex):
        skey, srow = index.skey, index.srow
        if skey.dtype != torch.int64 or srow.dtype != torch.int32 or skey.dim() != 1 or skey.shape != srow.shape or skey.size(0) != x.size(0):
            raise RuntimeError(f'shape mismatch: the index must hold skey int64 and srow int32 of ({x.size(0)},), one entry per row of xyz, got '
                               f'{skey.dtype} {tuple(skey.shape)} and {srow.dtype} {tuple(srow.shape)}')
        if skey.device != dev or srow.device != dev:
            raise RuntimeError(f'the index is on {skey.device}, xyz on {dev}')
        (z, y, xx), b = _grid(index.spatial_shape, index.batch_size)
        return x, q, nc, skey.contiguous(), srow.contiguous(), None, (b, z, y, xx)
    if isinstance(index, torch.Tensor):
        if index.dim() != 4 or index.dtype != torch.int32 or min(index.shape[1:]) < 1:
            raise RuntimeError(f'shape mismatch: a dense table must be an int32 (B, Z, Y, X) tensor, got {index.dtype} {tuple(index.shape)}')
        if index.device != dev:
            raise RuntimeError(f'the table is on {index.device}, xyz on {dev}')
        return x, q, nc, None, None, index.detach().contiguous(), tuple(index.shape)
    raise RuntimeError(f'index must be a VoxelQueryIndex or a dense int32 (B, Z, Y, X) table, got {type(index).__name__}')


def _launch(x, q, nc, skey, srow, table, grid, features, max_range, radius, nsample, use_xyz, group):
    """The one forward launch: (out | None, idx, cnt, mask)."""
    dev = q.device
    n, m = x.size(0), q.size(0)
    c = features.size(1) if features is not None else 0
    idx = torch.empty((m, nsample), dtype=torch.int32, device=dev)
    cnt = torch.empty((m,), dtype=torch.int32, device=dev)
    mask = torch.empty((m,), dtype=torch.bool, device=dev)
    out = torch.empty((m, (3 if use_xyz else 0) + c, nsample), dtype=torch.float32, device=dev) if group else None
    if m > 0:
        b, z, y, xx = grid
        r3 = (ctypes.c_int32 * 3)(*max_range)
        head = (_ptr(x), _ptr(q), _ptr(nc), _ptr(skey), _ptr(srow), _ptr(table))
        if group:
            _host.call('gd3d_vsa_voxel_query_and_group', dev,
                       head + (_ptr(features), b, z, y, xx, n, m, c, r3, float(radius), nsample, 1 if use_xyz else 0, _ptr(out), _ptr(idx),
                               _ptr(cnt), _ptr(mask)), (0,))
        else:
            _host.call('gd3d_vsa_voxel_query', dev,
                       head + (b, z, y, xx, n, m, r3, float(radius), nsample, _ptr(idx), _ptr(cnt), _ptr(mask)), (0,))
    return out, idx, cnt, mask


def voxel_query(max_range, radius, nsample, xyz, new_xyz, new_coords, index, return_cnt=False):
    """-> (idx (M, nsample) int32 GLOBAL rows of xyz, empty_mask (M,) bool); with `return_cnt` also cnt (M,) int32, the member count
    clipped to nsample.  The argument order of the published `VoxelQuery`.

    radius2 = radius * radius in fp32; the window of `max_range` = (rz, ry, rx) cells around new_coords[m] is walked with dz slowest
    and dx fastest, each ascending; a cell outside the grid or without a row is skipped; the cell's row is a member iff
    d2 = (nx-x)*(nx-x) + (ny-y)*(ny-y) + (nz-z)*(nz-z) <= radius2 (fp32, left to right, no fma; inclusive, NaN is no member); the
    first `nsample` members fill idx[m, :], the slots beyond repeat the first member; an empty query gives idx[m, :] = 0 and
    empty_mask[m] = True.  `index`: a `VoxelQueryIndex` or a dense int32 (B, Z, Y, X) table.  Not differentiable."""
    nsample = _check_nsample(nsample)
    max_range = _check_range(max_range)
    x, q, nc, skey, srow, table, grid = _check_query(xyz, new_xyz, new_coords, index)
    _, idx, cnt, mask = _launch(x, q, nc, skey, srow, table, grid, None, max_range, radius, nsample, False, False)
    return (idx, mask, cnt) if return_cnt else (idx, mask)


class _VoxelQueryAndGroup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, x, q, nc, skey, srow, table, grid, max_range, radius, nsample, use_xyz):
        f32 = features.detach().to(torch.float32).contiguous() if features is not None else None
        out, idx, cnt, _ = _launch(x, q, nc, skey, srow, table, grid, f32, max_range, radius, nsample, use_xyz, True)
        ctx.mark_non_differentiable(idx)
        if features is not None:
            ctx.save_for_backward(idx, cnt)
            ctx.shape = tuple(f32.shape)
            ctx.c_off = 3 if use_xyz else 0
            ctx.dtype = features.dtype
        return out, idx

    @staticmethod
    def backward(ctx, grad_out, _grad_idx):
        idx, cnt = ctx.saved_tensors
        n, c = ctx.shape
        m, nsample = idx.shape
        g = grad_out.detach().to(torch.float32).contiguous()
        grad = torch.empty((n, c), dtype=torch.float32, device=g.device)
        if n > 0 and c > 0:
            # a batch of ONE sample: global rows are local rows.  The two counts are device fills, not host copies: the call captures
            xyz_cnt = torch.full((1,), n, dtype=torch.int32, device=g.device)
            new_cnt = torch.full((1,), m, dtype=torch.int32, device=g.device)
            _host.call('gd3d_vsa_query_and_group_backward', g.device,
                       (_ptr(g), _ptr(idx), _ptr(cnt), _ptr(new_cnt), _ptr(xyz_cnt), 1, n, m, c, nsample, ctx.c_off, _ptr(grad)))
        return (grad.to(ctx.dtype),) + (None,) * 11


class VoxelQueryAndGroup(torch.nn.Module):
    """The published `VoxelQueryAndGroup(max_range, radius, nsample)` as ONE kernel launch: the voxel query, both groupings, the centre
    subtraction, the padded tail and the empty-query zeroing, with `QueryAndGroup`'s conventions.

    forward(xyz, new_xyz, new_coords, index, features=None) -> (new_features, idx)
      new_features (M, 3 + C, nsample): the grouped xyz minus the query centre, then the grouped features (one row per row of xyz);
      every channel of an empty query is zero; `use_xyz=False` drops the three xyz channels; `features=None` needs `use_xyz=True`.
      idx (M, nsample) int32 as `voxel_query` returns it.
    Differentiable with respect to `features` ONLY, through `QueryAndGroup`'s backward kernel called as a batch of one sample (float
    atomics: the last bits depend on the order of arrival); rows of empty queries pass no gradient."""

    def __init__(self, max_range, radius, nsample, use_xyz=True):
        super().__init__()
        self.max_range, self.radius, self.nsample, self.use_xyz = _check_range(max_range), float(radius), _check_nsample(nsample), bool(use_xyz)

    def forward(self, xyz, new_xyz, new_coords, index, features=None):
        if features is None and not self.use_xyz:
            raise RuntimeError('Cannot have not features and not use xyz as a feature!')
        x, q, nc, skey, srow, table, grid = _check_query(xyz, new_xyz, new_coords, index)
        dtype = new_xyz.dtype
        if features is not None:
            if features.dim() != 2 or not features.dtype.is_floating_point or features.size(0) != x.size(0):
                raise RuntimeError(f'shape mismatch: features must be a floating-point ({x.size(0)}, C) tensor (one row per row of xyz), '
                                   f'got {features.dtype} {tuple(features.shape)}')
            if features.size(1) == 0:
                raise RuntimeError('shape mismatch: features has no channels')
            if features.device != x.device:
                raise RuntimeError(f'features is on {features.device}, xyz on {x.device}')
            dtype = features.dtype
        out, idx = _VoxelQueryAndGroup.apply(features, x, q, nc, skey, srow, table, grid, self.max_range, self.radius, self.nsample,
                                             self.use_xyz)
        return out.to(dtype), idx
