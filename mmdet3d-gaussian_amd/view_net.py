"""The multi-view pillar encoder's view ops: what `PillarODCenterPoint` / `PillarODVoxelNet` and `SingleViewNet` run outside their
networks (the reference's mmdet3d_gaussian/models/detectors/pillar_od.py:24-70 and models/voxel_encoders/pillar_mvf_encoder.py:80-107):
`multi_view_voxelize` = `voxelize` / `voxelize_view` with the `to_cylindrical` / `to_spherical` transforms, `pillar_scatter` /
`PointPillarsScatter` = mmdet3d's dense pillar canvas (`SingleViewNet.pillar_scatter` and `pts_middle_encoder`), `view_sample` = the
per-sample `grid_sample(align_corners=False)` loop (:88-105).

The reference transforms, voxelizes and pads per view and per sample (about ten small ops each), scatters per sample with a mask, two
index ops, a transpose and an indexed assign, and samples per sample behind a `torch.where(... == i)` — a host sync that keeps the loop
out of a hipGraph.  Here: one launch for all views of the whole batch, a fill and one launch for the canvas and one gather for its
backward, one launch for the sampling and a fill plus one launch of float atomics for its backward (csrc/view_net.hip; DESIGN.md
§3.16).  No wrapper reads a value back.  CUDA tensors go to the kernels on the current stream, CPU tensors to the library's `_cpu`
twins (csrc/view_net_cpu.cpp).
"""
import ctypes

import torch
from torch import nn

from . import _host
from ._host import f32c
from .voxelize import _floats, _geometry, _stacked

VIEWS = {'cartesian': 0, 'cylindrical': 1, 'spherical': 2}       # GD3D_VIEW_*
MAX_VIEWS = 4
# The NCHW gradient of `view_sample`: True sums in a channels-last workspace and transposes once (three launches), False adds straight
# into the NCHW gradient, one lane per 4-byte segment (two launches).  profiles/r18_view_net_time.txt holds both.
NCHW_BACKWARD_VIA_WORKSPACE = True


def _view_kinds(views, voxel_sizes, point_cloud_ranges, who):
    if isinstance(views, str) or not 1 <= len(views) <= MAX_VIEWS:
        raise RuntimeError(f'{who}: views must be a sequence of 1 to {MAX_VIEWS} names, got {views!r}')
    for v in views:
        if v not in VIEWS:
            raise RuntimeError(f"{who}: a view must be 'cartesian', 'cylindrical' or 'spherical', got {v!r}")
    if voxel_sizes is not None and (len(voxel_sizes) != len(views) or len(point_cloud_ranges) != len(views)):
        raise RuntimeError(f'{who}: {len(views)} views need one voxel size and one range each, got {len(voxel_sizes)} and '
                           f'{len(point_cloud_ranges)}')
    return [VIEWS[v] for v in views]


def _launch_views(pts, cnt, kinds, geometry, with_coors):
    """the one launch -> (list of per-view points, list of per-view coors or None)"""
    N, C, dev, n = pts.size(0), pts.size(1), pts.device, len(kinds)
    out_pts = [pts if k == 0 else torch.empty((N, C), dtype=torch.float32, device=dev) for k in kinds]
    out_coors = [torch.empty((N, 4), dtype=torch.int32, device=dev) for _ in kinds] if with_coors else None
    if N == 0:
        return out_pts, out_coors
    ptr = _host.ptr_or_null
    kinds_arr = (ctypes.c_int32 * n)(*kinds)
    pts_arr = (ctypes.c_void_p * n)(*[None if k == 0 else ptr(t) for k, t in zip(kinds, out_pts)])
    coors_arr = (ctypes.c_void_p * n)(*[ptr(t) for t in out_coors]) if with_coors else (ctypes.c_void_p * n)()
    if with_coors:
        sizes = (ctypes.c_float * (3 * n))(*[v for g in geometry for v in g[0]])
        mins = (ctypes.c_float * (3 * n))(*[v for g in geometry for v in g[1]])
        grids = (ctypes.c_int32 * (3 * n))(*[v for g in geometry for v in g[2]])
    else:
        sizes = mins = grids = None
    _host.call('gd3d_multi_view_voxelize', dev,
               (ptr(pts), N, pts.stride(0), C, ptr(cnt), cnt.numel() if cnt is not None else 0, n, kinds_arr, sizes, mins, grids, pts_arr,
                coors_arr))
    return out_pts, out_coors


def multi_view_voxelize(points, views, voxel_sizes, point_cloud_ranges, points_batch_cnt=None):
    """`PillarODCenterPoint.voxelize` / `PillarODVoxelNet.voxelize` (pillar_od.py:47-70) for every view of the whole batch in ONE launch
    -> (multi_points, multi_coors): per view the stacked (N, C) fp32 points in that view's coordinates and (N, 4) int32 coors [b, z, y, x].

    points : the reference's per-sample list of (n_b, C >= 3) tensors, or stacked rows (N, C) grouped by sample with points_batch_cnt
             (B,) (None: one sample), as `dynamic_voxelize` takes them.  Every point is read once.
    views  : 1 to 4 names from 'cartesian' | 'cylindrical' | 'spherical', with one voxel size (3) and one range (6) per view, in the
             view's own coordinates; the grid is mmdet3d's round((range[3:] - range[:3]) / voxel_size) in fp32.
    The fixed fp32 sequence per point (include/gd3d.h), each step one correctly rounded operation:
      cylindrical: s = x*x + y*y, rho = sqrt(s), phi = fx_atan2f(y, x)                                       -> (phi, z, rho, rest..)
      spherical  : s2 = x*x + y*y, r2 = sqrt(s2), rho = sqrt(s2 + z*z), yaw = fx_atan2f(y, x), pitch = fx_atan2f(z, r2)
                                                                                                              -> (yaw, pitch, rho, rest..)
      'cartesian' returns the stacked input itself, not a copy.  fx_atan2f is the library's own polynomial (within 2.7e-7 rad of fp64;
      DESIGN.md §3.16); the reference's pitch asin(z / rho) is the same angle and NaN at the origin, where this form gives 0: restated.
    The cell of the transformed point is `dynamic_voxelize`'s (one subtraction, one division, one floor, compared as floats).  Column 0
    is the REFERENCE's layout, not `dynamic_voxelize`'s: `F.pad(coor, (1, 0), value=i)` writes the sample id into every row of a
    sample, so a dropped point (outside the grid, or a non-finite transformed coordinate) is [b, -1, -1, -1]; only a row past the
    counts' sum is all -1.  `Scatter` drops any row with a negative entry; `view_sample` reads the id from this column, as the
    reference's loop does.  For a row with a non-finite input coordinate the three transformed values are unspecified.
    Nothing is read back, no gradient (the reference runs this under `no_grad`)."""
    kinds = _view_kinds(views, voxel_sizes, point_cloud_ranges, 'multi_view_voxelize')
    geometry = [_geometry(_floats(vs, 3, 'voxel_size'), _floats(rng, 6, 'point_cloud_range')) for vs, rng in zip(voxel_sizes, point_cloud_ranges)]
    pts, cnt = _stacked(points, points_batch_cnt, 'multi_view_voxelize')
    return _launch_views(pts, cnt, kinds, geometry, True)


def _transform(points, kind, who):
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.size(1) < 3 or not points.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: {who} takes a floating-point (n, C >= 3) tensor, got '
                           f'{getattr(points, "dtype", type(points))} {tuple(getattr(points, "shape", ()))}')
    if points.size(1) > 256:
        raise RuntimeError(f'points rows of {points.size(1)} columns: at most 256 are supported')
    pts = f32c(points.detach())
    return _launch_views(pts, None, [kind], None, False)[0][0]


def to_cylindrical(points):
    """`to_cylindrical` (pillar_od.py:29-36) of one (n, C) tensor -> (n, C) fp32 rows (phi, z, rho, rest..), through the kernel of
    `multi_view_voxelize`: its fixed sequence, its bits."""
    return _transform(points, VIEWS['cylindrical'], 'to_cylindrical')


def to_spherical(points):
    """`to_spherical` (pillar_od.py:38-45) of one (n, C) tensor -> (n, C) fp32 rows (yaw, pitch, rho, rest..), through the kernel of
    `multi_view_voxelize`; the pitch is atan2(z, sqrt(x*x + y*y)): 0 at the origin, where the reference's asin(z / rho) is NaN."""
    return _transform(points, VIEWS['spherical'], 'to_spherical')


# ---- the pillar canvas -------------------------------------------------------------------------------------------------------------

def _launch_scatter(feats, coors, B, ny, nx, layout):
    V, C = feats.shape
    canvas = torch.empty((B, C, ny, nx), dtype=torch.float32, device=feats.device,
                         memory_format=torch.channels_last if layout else torch.contiguous_format)
    ptr = _host.ptr_or_null
    _host.call('gd3d_pillar_scatter', feats.device,
               (ptr(feats), ptr(coors), int(coors.dtype == torch.int64), coors.size(1), layout, V, C, B, ny, nx, ptr(canvas)))
    return canvas


def _launch_scatter_backward(g, coors, V, layout):
    """g (B, C, ny, nx) fp32 dense in `layout` -> grad_features (V, C): one gather"""
    B, C, ny, nx = g.shape
    grad = torch.empty((V, C), dtype=torch.float32, device=g.device)
    ptr = _host.ptr_or_null
    _host.call('gd3d_pillar_scatter_backward', g.device,
               (ptr(g), ptr(coors), int(coors.dtype == torch.int64), coors.size(1), layout, V, C, B, ny, nx, ptr(grad)))
    return grad


def _in_layout(t, layout):
    """t (B, C, H, W) as dense fp32 in `layout` (0 contiguous NCHW, 1 channels last); t itself when it already is"""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous(memory_format=torch.channels_last) if layout else t.contiguous()


class _PillarScatter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, voxel_features, coors, B, ny, nx, layout, track):
        canvas = _launch_scatter(f32c(voxel_features), coors, B, ny, nx, layout)
        if track and ctx.needs_input_grad[0]:
            ctx.save_for_backward(coors)
            ctx.state = (layout, voxel_features.size(0), voxel_features.dtype)
        return canvas if voxel_features.dtype == torch.float32 else canvas.to(voxel_features.dtype)

    @staticmethod
    @_host.guard_double_backward
    def backward(ctx, grad_canvas):
        (coors,) = ctx.saved_tensors
        layout, V, dtype = ctx.state
        grad = _launch_scatter_backward(_in_layout(grad_canvas, layout), coors, V, layout)
        return (grad if dtype == torch.float32 else grad.to(dtype)), None, None, None, None, None, None


def pillar_scatter(voxel_features, coors, batch_size, output_shape, channels_last=False):
    """mmdet3d's `PointPillarsScatter` for the whole batch -> canvas (B, C, ny, nx) of voxel_features' dtype: zeros, with
    canvas[b, :, y, x] = voxel_features[v].  A fill and one launch; the backward with respect to voxel_features is ONE gather launch,
    no atomics: deterministic.

    voxel_features : (V, C) floating point.       output_shape : (ny, nx).
    coors          : (V, 4) [b, z, y, x], or (V, 3) [z, y, x] with batch_size 1 (mmdet3d's `forward_single`); int32 or int64.  The
                     index is y * nx + x; the z column is ignored.  A row whose b, y or x lies outside the canvas is skipped and gets
                     a zero gradient (the reference would index out of range).  Rows must be unique per (b, y, x), as a `Scatter`'s
                     are: the value at a duplicated cell is one of its rows and otherwise unspecified.
    channels_last  : True returns the canvas in `torch.channels_last` memory — one row is C contiguous floats, written with 16-byte
                     stores when C % 4 == 0.  False (contiguous NCHW) stages 64 voxels x 64 channels through LDS, so the stores to a
                     channel plane come from consecutive lanes (a `Scatter`'s voxels arrive sorted by (b, y, x)).  The same values.
    mmdet3d is not pinned by the reference: its published module is restated.  Non-fp32 features are scattered in fp32 and cast back.
    Under `torch.no_grad()`, or when voxel_features needs no gradient, nothing is saved.  batch_size == 0 returns an empty canvas."""
    if not isinstance(voxel_features, torch.Tensor) or voxel_features.dim() != 2 or not voxel_features.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: voxel_features must be a floating-point (V, C) tensor, got '
                           f'{getattr(voxel_features, "dtype", type(voxel_features))} {tuple(getattr(voxel_features, "shape", ()))}')
    V, C = voxel_features.shape
    if not isinstance(coors, torch.Tensor) or coors.dim() != 2 or coors.size(0) != V or coors.size(1) not in (3, 4):
        raise RuntimeError(f'shape mismatch: coors must be ({V}, 4) [b, z, y, x] or ({V}, 3) [z, y, x], got {tuple(getattr(coors, "shape", ()))}')
    if coors.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f'coors must be an int32 or int64 tensor, got {coors.dtype}')
    if coors.device != voxel_features.device:
        raise RuntimeError(f'coors is on {coors.device}, voxel_features on {voxel_features.device}')
    batch_size = int(batch_size)
    if batch_size < 0 or (coors.size(1) == 3 and batch_size != 1):
        raise RuntimeError(f'batch_size must not be negative, and must be 1 for (V, 3) coors, got {batch_size}')
    if len(output_shape) != 2:
        raise RuntimeError(f'output_shape must be (ny, nx), got {tuple(output_shape)}')
    ny, nx = int(output_shape[0]), int(output_shape[1])
    if C < 1 or not 1 <= ny <= (1 << 24) or not 1 <= nx <= (1 << 24):
        raise RuntimeError(f'pillar_scatter: needs C >= 1 and 1 <= ny, nx <= 2^24, got C={C}, ny={ny}, nx={nx}')
    c = coors if coors.is_contiguous() else coors.contiguous()
    return _PillarScatter.apply(voxel_features, c, batch_size, ny, nx, int(bool(channels_last)), torch.is_grad_enabled())


class PointPillarsScatter(nn.Module):
    """mmdet3d's `PointPillarsScatter(in_channels, output_shape)`: forward(voxel_features, coors, batch_size=None) -> (B, in_channels,
    ny, nx); batch_size None is its `forward_single` ((V, 3) or (V, 4) coors of ONE sample, the batch column ignored).  Serves both
    `SingleViewNet.pillar_scatter` and the detectors' `pts_middle_encoder`.  `channels_last=True` returns the canvas in channels-last
    memory (see `pillar_scatter`)."""

    def __init__(self, in_channels, output_shape, channels_last=False):
        super().__init__()
        self.output_shape = output_shape
        self.ny = output_shape[0]
        self.nx = output_shape[1]
        self.in_channels = in_channels
        self.channels_last = bool(channels_last)
        self.fp16_enabled = False

    def forward(self, voxel_features, coors, batch_size=None):
        if voxel_features.dim() != 2 or voxel_features.size(1) != self.in_channels:
            raise RuntimeError(f'shape mismatch: voxel_features must be (V, {self.in_channels}), got {tuple(voxel_features.shape)}')
        if batch_size is None:
            return pillar_scatter(voxel_features, coors[:, -3:], 1, (self.ny, self.nx), self.channels_last)
        return pillar_scatter(voxel_features, coors, batch_size, (self.ny, self.nx), self.channels_last)

    def extra_repr(self):
        return f'in_channels={self.in_channels}, output_shape=({self.ny}, {self.nx}), channels_last={self.channels_last}'


# ---- the view-map sampling ---------------------------------------------------------------------------------------------------------

@_host.memo
def _axes(rng):
    """(lo_x, half_x, lo_y, half_y): lo as the reference's Python float, the divisor (hi - lo) / 2 made in double, each rounded once
    to fp32 by the call"""
    return float(rng[0]), (rng[3] - rng[0]) / 2.0, float(rng[1]), (rng[4] - rng[1]) / 2.0


def _dense(m):
    """the map as fp32 in a layout the kernels read where it lies -> (tensor, layout); any other striding takes one copy"""
    m = m if m.dtype == torch.float32 else m.float()
    if m.is_contiguous():
        return m, 0
    if m.is_contiguous(memory_format=torch.channels_last):
        return m, 1
    return m.contiguous(), 0


def _launch_sample(xyz, ids, m, layout, axes):
    B, C, H, W = m.shape
    N = xyz.size(0)
    out = torch.empty((N, C), dtype=torch.float32, device=m.device)
    _host.call('gd3d_view_sample', m.device,
               (xyz.data_ptr(), xyz.stride(0), ids.data_ptr(), int(ids.dtype == torch.int64), ids.stride(0), _host.ptr_or_null(m), layout, N, B,
                C, H, W, *axes, out.data_ptr()))
    return out


def _launch_sample_backward(g, xyz, ids, layout, shape, axes, via_workspace):
    """g (N, C) contiguous fp32 -> grad_map (B, C, H, W) dense in `layout`, every element written"""
    B, C, H, W = shape
    grad = torch.empty(shape, dtype=torch.float32, device=g.device,
                       memory_format=torch.channels_last if layout else torch.contiguous_format)
    work = torch.empty((B * C * H * W,), dtype=torch.float32, device=g.device) if via_workspace and layout == 0 and g.is_cuda else None
    _host.call('gd3d_view_sample_backward', g.device,
               (g.data_ptr(), xyz.data_ptr(), xyz.stride(0), ids.data_ptr(), int(ids.dtype == torch.int64), ids.stride(0), layout, xyz.size(0),
                B, C, H, W, *axes, _host.ptr_or_null(work), _host.ptr_or_null(grad)))
    return grad


class _ViewSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, view_map, xyz, ids, axes, track):
        m, layout = _dense(view_map)
        out = _launch_sample(xyz, ids, m, layout, axes)
        if track and ctx.needs_input_grad[0]:      # the points, the ids and the geometry: the map itself is not needed again
            ctx.save_for_backward(xyz, ids)
            ctx.state = (layout, tuple(m.shape), axes, view_map.dtype)
        return out if view_map.dtype == torch.float32 else out.to(view_map.dtype)

    @staticmethod
    @_host.guard_double_backward
    def backward(ctx, grad_out):
        xyz, ids = ctx.saved_tensors
        layout, shape, axes, dtype = ctx.state
        grad = _launch_sample_backward(f32c(grad_out), xyz, ids, layout, shape, axes, NCHW_BACKWARD_VIA_WORKSPACE)
        return (grad if dtype == torch.float32 else grad.to(dtype)), None, None, None, None


def view_sample(view_map, pts_xyz, pts_coors, point_cloud_range):
    """Lines :88-105 of `SingleViewNet.forward` — the grid normalisation and the per-sample `F.grid_sample(mode='bilinear',
    padding_mode='zeros', align_corners=False)` loop — for the whole batch in ONE launch -> (N, C), contiguous, of view_map's dtype.

    view_map  : (B, C, H, W) floating point, H, W >= 1.  Contiguous NCHW and `torch.channels_last` are consumed where they lie; any
                other striding takes ONE `.contiguous()` copy.  The forward result is the same bits for both layouts.
    pts_xyz   : (N, >= 2) floating point; only columns 0 and 1 are read, through the row stride — a `features[:, :3]` view is taken
                as it lies.
    pts_coors : the (N, 4) coors of `multi_view_voxelize` (column 0 is read through its stride) or an (N,) id vector, int32 or int64.
                B comes from the map.
    point_cloud_range (6): the view's range; only x and y (entries 0, 1, 3, 4) are used.
    In fp32, in the reference's order (include/gd3d.h spells the sequence out), per axis with n = W | H cells:
      g = (v - lo) / ((hi - lo) / 2) - 1 (the divisor made in double on the host, rounded once);  pix = ((g + 1) * n - 1) / 2;
      x0 = floor(ix), x1 = x0 + 1; weights (x1 - ix) * (y1 - iy), ..; value = ((nw*w_nw + ne*w_ne) + sw*w_sw) + se*w_se, a neighbour
      outside the map contributing 0.  With half-pixel alignment every point in the outer half cell of the range has one.
    A point whose pixel coordinate is not inside (-1, W) x (-1, H), whose coordinate is non-finite, or whose sample id is outside
    [0, B) gives a zero row and passes no gradient (for the id the reference leaves `new_empty` garbage: restated, not matched).  No
    index leaves the map for any input.
    Differentiable with respect to view_map ONLY: the points are raw inputs.  The backward writes every element of the gradient in
    view_map's layout: a fill and one launch of float atomics, lanes along C — in channels last one wave instruction covers 256
    contiguous bytes at C = 64, which is the layout to prefer; for contiguous NCHW the sums are made in a channels-last workspace and
    transposed once (NCHW_BACKWARD_VIA_WORKSPACE; profiles/r18_view_net_time.txt).  Where several points share a cell the last bits may
    depend on the order of arrival; on the CPU the backward is sequential and deterministic.  Non-fp32 maps are evaluated in fp32 and
    cast back.  Under `torch.no_grad()`, or when view_map needs no gradient, nothing is saved.  N == 0 or B == 0 returns an empty /
    zero tensor without a launch."""
    rng = _floats(point_cloud_range, 6, 'point_cloud_range')
    if not isinstance(view_map, torch.Tensor) or view_map.dim() != 4 or not view_map.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: view_map must be a floating-point (B, C, H, W) tensor, got '
                           f'{getattr(view_map, "dtype", type(view_map))} {tuple(getattr(view_map, "shape", ()))}')
    if not isinstance(pts_xyz, torch.Tensor) or pts_xyz.dim() != 2 or pts_xyz.size(1) < 2 or not pts_xyz.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: pts_xyz must be a floating-point (N, >= 2) tensor, got '
                           f'{getattr(pts_xyz, "dtype", type(pts_xyz))} {tuple(getattr(pts_xyz, "shape", ()))}')
    N = pts_xyz.size(0)
    if not isinstance(pts_coors, torch.Tensor) or pts_coors.size(0) != N or not (pts_coors.dim() == 1 or (pts_coors.dim() == 2 and pts_coors.size(1) >= 1)):
        raise RuntimeError(f'shape mismatch: pts_coors must be ({N}, 4) coors or an ({N},) id vector, got {tuple(getattr(pts_coors, "shape", ()))}')
    if pts_coors.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f'pts_coors must be an int32 or int64 tensor, got {pts_coors.dtype}')
    if pts_xyz.device != view_map.device or pts_coors.device != view_map.device:
        raise RuntimeError(f'pts_xyz is on {pts_xyz.device}, pts_coors on {pts_coors.device}, view_map on {view_map.device}')
    B, C, H, W = view_map.shape
    if C < 1 or not 1 <= H <= (1 << 24) or not 1 <= W <= (1 << 24):
        raise RuntimeError(f'view_sample: needs C >= 1 and 1 <= H, W <= 2^24, got C={C}, H={H}, W={W}')
    axes = _axes(rng)
    half = torch.tensor([axes[1], axes[3]], dtype=torch.float64).float()
    if not bool((half > 0).all() & torch.isfinite(half).all()):
        raise RuntimeError(f'view_sample: the range must have a positive finite extent in x and y, got {point_cloud_range}')
    if N == 0 or B == 0:
        return view_map.new_zeros((N, C))
    xyz = pts_xyz.detach()
    if xyz.dtype != torch.float32:
        xyz = xyz.float()
    if xyz.stride(1) != 1:
        xyz = xyz.contiguous()
    ids = pts_coors[:, 0] if pts_coors.dim() == 2 else pts_coors
    return _ViewSample.apply(view_map, xyz, ids, axes, torch.is_grad_enabled())     # grad mode is off inside Function.forward: read here
