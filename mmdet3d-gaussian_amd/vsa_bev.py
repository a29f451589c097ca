"""The statements of PV-RCNN's `VoxelSetAbstraction.forward` outside its MLPs that feed the grouping ops (the reference's
mmdet3d_gaussian/models/middle_encoders/voxel_set_abstraction.py): `bev_interpolate` = `interpolate_from_bev_features` (:153-177),
`voxel_centers` = `get_voxel_centers` (:179-193) plus the per-sample count loop of forward (:303-305), `sample_keypoints` = the
keypoint gather of `get_sampled_points` (:195-244).

The reference builds the normalised grid with about ten small tensor ops, calls `F.grid_sample`, and permutes the result; per
sparse-conv level it runs six elementwise ops and B compare / sum / assign triples; it picks the keypoints in a Python loop.  Here:
one launch for the interpolation (csrc/vsa_bev.hip), a fill and one launch for its backward, a fill and one launch
for the centres with their counts, and `furthest_point_sample_stacked` plus one gather for the keypoints.  No wrapper reads a value
back, so the stage can be captured in a hipGraph.  CUDA tensors go to the kernels on the current stream, CPU tensors to the
library's `_cpu` twins (csrc/vsa_bev_cpu.cpp).
"""
import ctypes

import torch

from . import _host
from ._host import f32c
from .vsa import furthest_point_sample_stacked

ALIGNMENTS = ('half', 'halfmin')


def _triple(v, n, name):
    v = tuple(float(x) for x in v)
    if len(v) != n:
        raise RuntimeError(f'{name} must hold {n} values, got {len(v)}')
    return v


def _check_geometry(voxel_size, point_cloud_range, scale_factor, voxel_center_align, who):
    vs, rng = _triple(voxel_size, 3, 'voxel_size'), _triple(point_cloud_range, 6, 'point_cloud_range')
    if voxel_center_align not in ALIGNMENTS:
        raise RuntimeError(f"{who}: voxel_center_align must be 'half' or 'halfmin', got {voxel_center_align!r} "
                           '(the reference silently uses the raw range there)')
    if isinstance(scale_factor, bool) or not isinstance(scale_factor, (int, float)) or not scale_factor > 0:
        raise RuntimeError(f'{who}: scale_factor must be a positive number, got {scale_factor!r}')
    return vs, rng


@_host.memo
def _corners(vs_xy, lo_xy, hi_xy, scale, align):
    """(tl_x, tl_y, br_x, br_y) in fp32, the reference's statements :157-166 in their order on host tensors"""
    vs = torch.tensor(vs_xy, dtype=torch.float32)
    tl, br = torch.tensor(lo_xy, dtype=torch.float32), torch.tensor(hi_xy, dtype=torch.float32)
    if align == 'half':
        tl.add_(0.5 * vs * scale)
        br.sub_(0.5 * vs * scale)
    else:
        tl.add_(0.5 * vs)
        br.sub_(vs * (scale - 0.5))
    return tuple(float(v) for v in tl) + tuple(float(v) for v in br)


@_host.memo
def _centre_terms(vs, lo, scale, align):
    """(voxel_size, range_min, add) as three-float host arrays: `add` is the in-place term of :187-190 in the reference's order"""
    v = torch.tensor(vs, dtype=torch.float32)
    add = 0.5 * v * scale if align == 'half' else 0.5 * v
    arr = ctypes.c_float * 3
    return arr(*vs), arr(*lo), arr(*(float(x) for x in add))


def _launch_interp(kp, bev, layout, corners):
    """kp (B, M, >= 2) fp32 with unit last stride, bev (B, C, H, W) fp32 dense in `layout` -> (B, M, C): the one launch"""
    B, C, H, W = bev.shape
    M = kp.size(1)
    out = torch.empty((B, M, C), dtype=torch.float32, device=bev.device)
    _host.call('gd3d_vsa_bev_interp', bev.device,
               (kp.data_ptr(), kp.stride(0), kp.stride(1), bev.data_ptr(), layout, B, M, C, H, W, *corners, out.data_ptr()))
    return out


def _launch_interp_backward(g, kp, layout, shape, corners):
    """g (B, M, C) contiguous fp32 -> grad_bev (B, C, H, W) dense in `layout`, every element written: a fill and one launch"""
    B, C, H, W = shape
    grad = torch.empty(shape, dtype=torch.float32, device=g.device,
                       memory_format=torch.channels_last if layout else torch.contiguous_format)
    _host.call('gd3d_vsa_bev_interp_backward', g.device,
               (g.data_ptr(), kp.data_ptr(), kp.stride(0), kp.stride(1), layout, B, kp.size(1), C, H, W, *corners, grad.data_ptr()))
    return grad


def _dense(bev):
    """bev as fp32 in a layout the kernels read where it lies -> (tensor, layout): 0 contiguous NCHW, 1 channels last; any other
    striding takes one `.contiguous()` copy"""
    b = bev if bev.dtype == torch.float32 else bev.float()     # preserves a dense layout
    if b.is_contiguous():
        return b, 0
    if b.is_contiguous(memory_format=torch.channels_last):
        return b, 1
    return b.contiguous(), 0


class _BevInterp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bev_features, kp, corners, track):
        bev, layout = _dense(bev_features)
        out = _launch_interp(kp, bev, layout, corners)
        if track and ctx.needs_input_grad[0]:       # the keypoints and the geometry: the map itself is not needed again
            ctx.save_for_backward(kp)
            ctx.state = (layout, tuple(bev.shape), corners, bev_features.dtype)
        return out if bev_features.dtype == torch.float32 else out.to(bev_features.dtype)

    @staticmethod
    @_host.guard_double_backward
    def backward(ctx, grad_out):
        (kp,) = ctx.saved_tensors
        layout, shape, corners, dtype = ctx.state
        grad = _launch_interp_backward(f32c(grad_out), kp, layout, shape, corners)
        return (grad if dtype == torch.float32 else grad.to(dtype)), None, None, None


def bev_interpolate(keypoints, bev_features, voxel_size, point_cloud_range, scale_factor, voxel_center_align='half'):
    """`VoxelSetAbstraction.interpolate_from_bev_features` in one launch -> (B, M, C), contiguous, of bev_features' dtype.

    keypoints     : (B, M, >= 2) floating point; only columns 0 (x) and 1 (y) are read, through the row strides — a `[..., :3]`
                    view is taken as it lies (a last dimension that is not unit-strided takes one copy).
    bev_features  : (B, C, H, W) floating point, H, W >= 2, C >= 1.  Contiguous NCHW and `torch.channels_last` are consumed where
                    they lie, through element strides; any other striding takes ONE `.contiguous()` copy.  The forward result is
                    the same bits for both layouts.
    voxel_size (3), point_cloud_range (6), scale_factor > 0 (the map's stride, `bev_sa_config.scale_factor`), voxel_center_align:
      'half'    : tl = range[:2] + 0.5*vs*scale,  br = range[3:5] - 0.5*vs*scale
      'halfmin' : tl = range[:2] + 0.5*vs,        br = range[3:5] - vs*(scale - 0.5)
      anything else raises (the reference silently uses the raw range).  tl / br are the centres of the first / last cell, computed
      on the host in fp32 in the reference's operation order; br > tl is required (the reference divides by zero otherwise).
    The value is `F.grid_sample(bev, grid, align_corners=True)` on the reference's grid, bilinear, zero padding: the pixel coordinate
    is ((xy - tl) * (size - 1)) / (br - tl) in fp32, the four neighbours are summed in one fixed order (include/gd3d.h spells the
    sequence out), neighbours outside the map contribute zero.  A keypoint a cell or more outside the map, or with a NON-FINITE
    coordinate, gives a zero row and passes no gradient — the reference's result for a non-finite coordinate is unspecified:
    restated, not matched.  No index leaves the map for any input.
    Differentiable with respect to bev_features ONLY: the keypoints are furthest-point picks of input points and no caller uses
    their gradient — the reference's `grid_sample` would return a gradient for its grid, this op does not.  The backward writes every
    element of the gradient, in bev_features' layout, and sums with float atomics on the GPU: where several keypoints share a cell
    the last bits may depend on the order of arrival (as with `grouping`'s backward); on the CPU it is sequential and deterministic.
    Non-fp32 inputs are evaluated in fp32 and cast back.  Under `torch.no_grad()`, or when bev_features needs no gradient, nothing
    is saved.  B == 0 or M == 0 returns an empty tensor without a launch."""
    vs, rng = _check_geometry(voxel_size, point_cloud_range, scale_factor, voxel_center_align, 'bev_interpolate')
    if not isinstance(keypoints, torch.Tensor) or keypoints.dim() != 3 or keypoints.size(2) < 2 or not keypoints.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: keypoints must be a floating-point (B, M, >= 2) tensor, got '
                           f'{getattr(keypoints, "dtype", type(keypoints))} {tuple(getattr(keypoints, "shape", ()))}')
    if not isinstance(bev_features, torch.Tensor) or bev_features.dim() != 4 or not bev_features.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: bev_features must be a floating-point (B, C, H, W) tensor, got '
                           f'{getattr(bev_features, "dtype", type(bev_features))} {tuple(getattr(bev_features, "shape", ()))}')
    B, C, H, W = bev_features.shape
    if keypoints.size(0) != B:
        raise RuntimeError(f'shape mismatch: keypoints has {keypoints.size(0)} samples, bev_features {B}')
    if keypoints.device != bev_features.device:
        raise RuntimeError(f'keypoints is on {keypoints.device}, bev_features on {bev_features.device}')
    if C < 1 or H < 2 or W < 2:
        raise RuntimeError(f'bev_interpolate: needs C >= 1 and H, W >= 2, got C={C}, H={H}, W={W}')
    corners = _corners(vs[:2], rng[:2], rng[3:5], scale_factor, voxel_center_align)
    if not (corners[2] > corners[0] and corners[3] > corners[1]):
        raise RuntimeError(f'bev_interpolate: the last cell centre {corners[2:]} must lie beyond the first {corners[:2]} on both axes')
    M = keypoints.size(1)
    if B == 0 or M == 0:
        return bev_features.new_zeros((B, M, C))
    kp = keypoints.detach()
    if kp.dtype != torch.float32:
        kp = kp.float()
    if kp.stride(2) != 1:
        kp = kp.contiguous()
    return _BevInterp.apply(bev_features, kp, corners, torch.is_grad_enabled())     # grad mode is off inside Function.forward: read here


def voxel_centers(coors, voxel_size, point_cloud_range, scale_factor, voxel_center_align, batch_size):
    """`get_voxel_centers` plus forward's per-sample count loop in one call -> (xyz (N, 3) fp32, xyz_batch_cnt (batch_size,) int32).

    coors : (N, 4) int32 or int64, columns [b, z, y, x] (a sparse-conv level's `indices`).
    xyz   = ((c * voxel_size) * scale_factor + point_cloud_range[:3]) + add in fp32, left to right, c = coors[:, [3, 2, 1]] as fp32,
            add = (0.5*voxel_size)*scale_factor for 'half', 0.5*voxel_size for 'halfmin' (anything else raises, as the reference
            does): the fp32 torch statements' bits.
    xyz_batch_cnt[b] = the rows whose batch id is b: integer adds, exact.  A row whose id is outside [0, batch_size) is counted for
            no sample; its centre is still written.  `batch_size` is an argument: nothing is read back from `coors`.
    N == 0 gives an empty xyz and zero counts.  Not differentiable (integer input)."""
    vs, rng = _check_geometry(voxel_size, point_cloud_range, scale_factor, voxel_center_align, 'voxel_centers')
    if not isinstance(coors, torch.Tensor) or coors.dim() != 2 or coors.size(1) != 4:
        raise RuntimeError(f'shape mismatch: coors must be an (N, 4) tensor [b, z, y, x], got {tuple(getattr(coors, "shape", ()))}')
    if coors.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f'coors must be an int32 or int64 tensor, got {coors.dtype}')
    batch_size = int(batch_size)
    if batch_size < 0:
        raise RuntimeError(f'batch_size must not be negative, got {batch_size}')
    c = coors if coors.is_contiguous() else coors.contiguous()
    N = c.size(0)
    xyz = torch.empty((N, 3), dtype=torch.float32, device=c.device)
    cnt = torch.empty((batch_size,), dtype=torch.int32, device=c.device)
    size, lo, add = _centre_terms(vs, rng[:3], scale_factor, voxel_center_align)
    _host.call('gd3d_vsa_voxel_centers', c.device,
               (_host.ptr_or_null(c), int(c.dtype == torch.int64), N, size, float(scale_factor), lo, add, batch_size, _host.ptr_or_null(xyz),
                _host.ptr_or_null(cnt)))
    return xyz, cnt


def sample_keypoints(*args):
    """The keypoint gather of `get_sampled_points` -> (B, num_keypoints, 3), of the points' dtype.

    sample_keypoints(points, num_keypoints)             : points = the reference's per-sample list of (n_b, >= 3) tensors
    sample_keypoints(xyz, xyz_batch_cnt, num_keypoints) : stacked rows (N, 3) grouped by sample, with their counts (B,)
    It is `furthest_point_sample_stacked` — all samples in one launch, the reference's wrap-around for n < num_keypoints included
    (out[j] = out[j % n]) — plus ONE gather whose row offsets come from a device cumsum of the counts: nothing is read back.  A
    sample without points takes row indices clamped into the array (the reference fails there).  Not differentiable: the keypoints
    are picks of input points.
    The `voxel_center_as_source` branch is `sample_keypoints(*voxel_centers(coors, ..., scale_factor=1, ..., batch_size), K)`:
    valid for `coors` grouped by sample, which the reference's stacked ops assume of every level's indices."""
    if len(args) == 2:
        points, num_keypoints = args
        if not isinstance(points, (list, tuple)) or len(points) == 0:
            raise RuntimeError('sample_keypoints: points must be a non-empty list of (n, >= 3) tensors')
        for p in points:
            if not isinstance(p, torch.Tensor) or p.dim() != 2 or p.size(1) < 3 or not p.dtype.is_floating_point:
                raise RuntimeError(f'shape mismatch: every entry of points must be a floating-point (n, >= 3) tensor, got '
                                   f'{getattr(p, "dtype", type(p))} {tuple(getattr(p, "shape", ()))}')
        xyz = torch.cat([p[:, :3] for p in points], dim=0)
        cnt = torch.tensor([p.size(0) for p in points], dtype=torch.int32).to(xyz.device, non_blocking=True)   # sizes the host knows: a copy TO the device
    elif len(args) == 3:
        xyz, cnt, num_keypoints = args
        if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2 or xyz.size(1) != 3 or not xyz.dtype.is_floating_point:
            raise RuntimeError(f'shape mismatch: xyz must be a floating-point (N, 3) tensor, got '
                               f'{getattr(xyz, "dtype", type(xyz))} {tuple(getattr(xyz, "shape", ()))}')
    else:
        raise RuntimeError('sample_keypoints takes (points, num_keypoints) or (xyz, xyz_batch_cnt, num_keypoints)')
    num_keypoints = int(num_keypoints)
    if num_keypoints < 0:
        raise RuntimeError(f'num_keypoints must not be negative, got {num_keypoints}')
    xyz = xyz.detach()
    cnt = _host.counts_i32(cnt, xyz, 'xyz_batch_cnt')
    if xyz.size(0) == 0:
        raise RuntimeError('sample_keypoints: there are no points to pick from')
    local = furthest_point_sample_stacked(xyz, cnt, num_keypoints)              # (B, K) int64, local to each sample
    ends = torch.cumsum(cnt, dim=0, dtype=torch.int64)
    rows = (local + (ends - cnt).unsqueeze(1)).clamp_(max=xyz.size(0) - 1)      # an empty last sample must not index past the array
    return xyz[rows.reshape(-1)].reshape(cnt.numel(), num_keypoints, 3)
