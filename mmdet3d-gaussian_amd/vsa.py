"""PV-RCNN's voxel-set-abstraction ops — the call surface of /root/reference/mmdet3d_gaussian/ops/vsa/group_points.py
(`ball_query` :7-39, `grouping` :42-94, `QueryAndGroup` :97-183) and ops/vsa/sample_points.py (`furthest_point_sample` :7-33)
on top of the HIP kernels of csrc/vsa.hip (include/gd3d.h, gd3d_vsa_*).

All data is stacked: `xyz` (N1+N2+..., 3) with `xyz_batch_cnt` (B,), `new_xyz` (M1+M2+..., 3) with `new_xyz_batch_cnt` (B,).  A query
sees the points of its own sample only; indices are local to the sample.

CUDA tensors go to the kernels on the current stream, CPU tensors to the library's `_cpu` twins (bit-identical idx, cnt, mask and
FPS picks).  No wrapper reads a value back to validate the counts — the reference's `assert xyz.shape[0] == xyz_batch_cnt.sum()`
is a host sync on every call — so every op can be captured in a hipGraph.  Instead the kernels clamp every sample's segment to
the arrays' row counts and every gathered index to its segment: inconsistent counts or indices cannot read or write outside the
buffers (rows of `new_xyz` that the counts do not cover are empty balls).

Inputs are fp32 with int32 counts and int32 `idx`; other float dtypes are evaluated in fp32 and cast back (as GDLoss does), int64
counts are converted.
"""
import torch

from . import _host, _lib
from ._host import counts_i32 as _cnt32, ptr_or_null as _ptr, rows_f32 as _rows

MAX_NSAMPLE = 1024


def _check_nsample(nsample):
    nsample = int(nsample)
    if not 1 <= nsample <= MAX_NSAMPLE:
        raise RuntimeError(f'nsample must be in [1, {MAX_NSAMPLE}], got {nsample}')
    return nsample


def _query_and_group(xyz, xyz_cnt, new_xyz, new_cnt, features, radius, nsample, use_xyz, group):
    """The one forward launch: (out | None, idx, cnt, mask); every argument already fp32 / int32 / contiguous."""
    dev = new_xyz.device
    n, m, b = xyz.size(0), new_xyz.size(0), xyz_cnt.numel()
    c = features.size(1) if features is not None else 0
    idx = torch.empty((m, nsample), dtype=torch.int32, device=dev)
    cnt = torch.empty((m,), dtype=torch.int32, device=dev)
    mask = torch.empty((m,), dtype=torch.bool, device=dev)
    out = torch.empty((m, (3 if use_xyz else 0) + c, nsample), dtype=torch.float32, device=dev) if group else None
    if m == 0:
        return out, idx, cnt, mask
    _host.call('gd3d_vsa_query_and_group', dev,
               (_ptr(xyz), _ptr(xyz_cnt), _ptr(new_xyz), _ptr(new_cnt), _ptr(features), b, n, m, c, float(radius), nsample,
                1 if use_xyz else 0, _ptr(out), _ptr(idx), _ptr(cnt), _ptr(mask)), (0,))
    return out, idx, cnt, mask


def _check_stacked(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt):
    x = _rows(xyz, 3, 'xyz')
    q = _rows(new_xyz, 3, 'new_xyz')
    if x.device != q.device:
        raise RuntimeError(f'xyz is on {x.device}, new_xyz on {q.device}')
    xc = _cnt32(xyz_batch_cnt, x, 'xyz_batch_cnt')
    qc = _cnt32(new_xyz_batch_cnt, x, 'new_xyz_batch_cnt')
    if xc.numel() != qc.numel():
        raise RuntimeError(f'shape mismatch: xyz_batch_cnt has {xc.numel()} samples, new_xyz_batch_cnt {qc.numel()}')
    return x, xc, q, qc


def ball_query(radius, nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, return_cnt=False):
    """-> (idx (M, nsample) int32, empty_ball_mask (M,) bool) — what the reference's `BallQuery.forward` returns after its fix-up
    (group_points.py:26-32); with `return_cnt` also cnt (M,) int32, the member count clipped to nsample.

    radius2 = radius * radius in fp32; in ascending point index d2 = (nx-x)*(nx-x) + (ny-y)*(ny-y) + (nz-z)*(nz-z) (fp32, left to
    right, no fma); the first `nsample` points with d2 < radius2 (strict) fill idx[m, :], the slots beyond repeat the first member;
    an empty ball gives idx[m, :] = 0 and empty_ball_mask[m] = True.  Not differentiable (neither is the reference's)."""
    nsample = _check_nsample(nsample)
    x, xc, q, qc = _check_stacked(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
    _, idx, cnt, mask = _query_and_group(x, xc, q, qc, None, radius, nsample, False, False)
    return (idx, mask, cnt) if return_cnt else (idx, mask)


class _Grouping(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, features_batch_cnt, idx, idx_batch_cnt):
        f32 = features.detach().to(torch.float32).contiguous()
        n, c = f32.shape
        m, nsample = idx.shape
        b = features_batch_cnt.numel()
        out = torch.empty((m, c, nsample), dtype=torch.float32, device=f32.device)
        if m > 0:
            _host.call('gd3d_vsa_group', f32.device,
                       (_ptr(f32), _ptr(features_batch_cnt), _ptr(idx), _ptr(idx_batch_cnt), b, n, m, c, nsample, _ptr(out)), (0,))
        ctx.save_for_backward(idx, features_batch_cnt, idx_batch_cnt)
        ctx.shape = (n, c)
        ctx.dtype = features.dtype
        return out.to(features.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        idx, features_batch_cnt, idx_batch_cnt = ctx.saved_tensors
        n, c = ctx.shape
        m, nsample = idx.shape
        g = grad_out.detach().to(torch.float32).contiguous()
        grad = torch.empty((n, c), dtype=torch.float32, device=g.device)
        if n > 0:
            _host.call('gd3d_vsa_group_backward', g.device,
                       (_ptr(g), _ptr(idx), _ptr(idx_batch_cnt), _ptr(features_batch_cnt), features_batch_cnt.numel(), n, m, c,
                        nsample, _ptr(grad)))
        return grad.to(ctx.dtype), None, None, None


def grouping(features, features_batch_cnt, idx, idx_batch_cnt):
    """features (N1+N2+..., C), idx (M1+M2+..., nsample) int32 local indices -> (M, C, nsample) with
    out[m, c, s] = features[start_b + idx[m, s], c] (reference `GroupingOperation`, group_points.py:42-94).  Differentiable wrt
    `features`: grad_features[start_b + idx[m, s], c] += grad_out[m, c, s], summed with float atomics on the GPU (the last bits
    depend on the order of arrival, as with the reference's atomicAdd)."""
    if features.dim() != 2 or not features.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: features must be a floating-point (rows, C) tensor, got {features.dtype} {tuple(features.shape)}')
    if features.size(1) == 0:
        raise RuntimeError('shape mismatch: features has no channels')
    if idx.dim() != 2 or idx.dtype.is_floating_point or idx.dtype == torch.bool:
        raise RuntimeError(f'shape mismatch: idx must be an integer (M, nsample) tensor, got {idx.dtype} {tuple(idx.shape)}')
    if idx.device != features.device:
        raise RuntimeError(f'idx is on {idx.device}, features on {features.device}')
    _check_nsample(idx.size(1))
    fc = _cnt32(features_batch_cnt, features, 'features_batch_cnt')
    ic = _cnt32(idx_batch_cnt, features, 'idx_batch_cnt')
    if fc.numel() != ic.numel():
        raise RuntimeError(f'shape mismatch: features_batch_cnt has {fc.numel()} samples, idx_batch_cnt {ic.numel()}')
    return _Grouping.apply(features, fc, idx.to(torch.int32).contiguous(), ic)


class _QueryAndGroup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, xyz, xyz_cnt, new_xyz, new_cnt, radius, nsample, use_xyz):
        f32 = features.detach().to(torch.float32).contiguous() if features is not None else None
        out, idx, cnt, _ = _query_and_group(xyz, xyz_cnt, new_xyz, new_cnt, f32, radius, nsample, use_xyz, True)
        ctx.mark_non_differentiable(idx)
        if features is not None:
            ctx.save_for_backward(idx, cnt, xyz_cnt, new_cnt)
            ctx.shape = tuple(f32.shape)
            ctx.c_off = 3 if use_xyz else 0
            ctx.dtype = features.dtype
        return out, idx

    @staticmethod
    def backward(ctx, grad_out, _grad_idx):
        idx, cnt, xyz_cnt, new_cnt = ctx.saved_tensors
        n, c = ctx.shape
        m, nsample = idx.shape
        g = grad_out.detach().to(torch.float32).contiguous()
        grad = torch.empty((n, c), dtype=torch.float32, device=g.device)
        if n > 0 and c > 0:
            _host.call('gd3d_vsa_query_and_group_backward', g.device,
                       (_ptr(g), _ptr(idx), _ptr(cnt), _ptr(new_cnt), _ptr(xyz_cnt), xyz_cnt.numel(), n, m, c, nsample, ctx.c_off,
                        _ptr(grad)))
        return (grad.to(ctx.dtype),) + (None,) * 7


class QueryAndGroup(torch.nn.Module):
    """The reference's `QueryAndGroup(radius, nsample, use_xyz=True)` (group_points.py:97-183) as ONE kernel launch: the ball
    query, both groupings, the centre subtraction, the padded tail and the empty-ball zeroing — the reference makes about seven
    passes over the grouped tensor.  Its `debug` argument (an open3d viewer) is not taken.

    forward(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None) -> (new_features, idx)
      new_features (M, 3 + C, nsample): the grouped xyz minus the query centre, then the grouped features; every channel of an
      empty ball is zero; `use_xyz=False` drops the three xyz channels; `features=None` needs `use_xyz=True`.
      idx (M, nsample) int32 as `ball_query` returns it.
    Differentiable with respect to `features` ONLY: the grouped xyz carries no gradient a caller uses in the reference (the
    keypoints and raw points are inputs, not activations), so no gradient flows to `xyz` or `new_xyz`; rows of empty balls pass
    no gradient.  The backward adds with float atomics (last bits depend on the order of arrival, as the reference's atomicAdd);
    the padded slots of a ball all name its first member and are summed before one add."""

    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = float(radius), _check_nsample(nsample), bool(use_xyz)

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None):
        if features is None and not self.use_xyz:
            raise RuntimeError('Cannot have not features and not use xyz as a feature!')
        x, xc, q, qc = _check_stacked(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
        dtype = new_xyz.dtype
        if features is not None:
            if features.dim() != 2 or not features.dtype.is_floating_point or features.size(0) != x.size(0):
                raise RuntimeError(f'shape mismatch: features must be a floating-point ({x.size(0)}, C) tensor (one row per point of xyz), '
                                   f'got {features.dtype} {tuple(features.shape)}')
            if features.size(1) == 0:
                raise RuntimeError('shape mismatch: features has no channels')
            if features.device != x.device:
                raise RuntimeError(f'features is on {features.device}, xyz on {x.device}')
            dtype = features.dtype
        out, idx = _QueryAndGroup.apply(features, x, xc, q, qc, self.radius, self.nsample, self.use_xyz)
        return out.to(dtype), idx


def _fps_workspace(lib, n_rows, dev):
    return torch.empty(lib.gd3d_vsa_fps_workspace_bytes(n_rows), dtype=torch.uint8, device=dev)


def furthest_point_sample(xyz, npoint):
    """xyz (B, N, 3) -> (B, npoint) int32 (reference `furthest_point_sample`, sample_points.py:7-33).  The first pick is index 0;
    each later pick is the arg max over the sample of the running min of the squared distances (fp32, the ball query's expression
    order, no fma) to all earlier picks.  On exactly equal distances the LOWEST index wins (the reference's choice there depends on
    its block size).  N < npoint returns the N picks cyclically, N == 0 zeros.  Not differentiable."""
    if xyz.dim() != 3 or xyz.size(2) != 3 or not xyz.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: xyz must be a floating-point (B, N, 3) tensor, got {xyz.dtype} {tuple(xyz.shape)}')
    npoint = int(npoint)
    if npoint < 0:
        raise RuntimeError(f'npoint must not be negative, got {npoint}')
    lib = _lib.load()
    x = xyz.detach().to(torch.float32).contiguous()
    b, n = x.size(0), x.size(1)
    out = torch.empty((b, npoint), dtype=torch.int32, device=x.device)
    if b == 0 or npoint == 0:
        return out
    if x.is_cuda:
        ws = _fps_workspace(lib, b * n, x.device)
        with _host.on_device(x.device) as stream:
            rc = lib.gd3d_vsa_fps(_ptr(x), b, n, npoint, _ptr(out), ws.data_ptr(), stream)
    else:
        rc = lib.gd3d_vsa_fps_cpu(_ptr(x), b, n, npoint, _ptr(out), 0)
    _lib.check(rc, 'gd3d_vsa_fps')
    return out


def furthest_point_sample_stacked(xyz, xyz_batch_cnt, npoint):
    """xyz (N1+N2+..., 3), xyz_batch_cnt (B,) -> (B, npoint) int64 indices LOCAL to each sample, all samples in one launch: the
    per-sample loop of the reference's `VoxelSetAbstraction.get_sampled_points` (voxel_set_abstraction.py:205-217) including its
    wrap-around — a sample with n < npoint points returns its n picks cyclically, out[j] = out[j % n].  A sample with n == 0
    returns zeros (the reference would fail there).  Pick rule as `furthest_point_sample`."""
    x = _rows(xyz, 3, 'xyz')
    xc = _cnt32(xyz_batch_cnt, x, 'xyz_batch_cnt')
    npoint = int(npoint)
    if npoint < 0:
        raise RuntimeError(f'npoint must not be negative, got {npoint}')
    lib = _lib.load()
    b, n = xc.numel(), x.size(0)
    out = torch.empty((b, npoint), dtype=torch.int64, device=x.device)
    if b == 0 or npoint == 0:
        return out
    if x.is_cuda:
        ws = _fps_workspace(lib, n, x.device)
        with _host.on_device(x.device) as stream:
            rc = lib.gd3d_vsa_fps_stacked(_ptr(x), _ptr(xc), b, n, npoint, _ptr(out), ws.data_ptr(), stream)
    else:
        rc = lib.gd3d_vsa_fps_stacked_cpu(_ptr(x), _ptr(xc), b, n, npoint, _ptr(out), 0)
    _lib.check(rc, 'gd3d_vsa_fps_stacked')
    return out
