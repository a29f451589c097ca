"""oracle/ref_kernels.py — TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Driver of the REFERENCE's own device kernels, compiled from where they lie into oracle/_ref/ (Makefile targets `ref_vsa`, `ref_vox`):
  ref_vsa.so  ball query, point grouping (+ gradient), furthest point sampling, voxel query   (ctypes; ref_vsa_bind.hip)
  ref_vox.so  dynamic scatter: index, reduce, backward                                         (a torch extension; build_ref_vox.py)

THIS MODULE IS THE SAFETY BOUNDARY.  The reference kernels check no bounds and their host wrappers call exit(-1) on a launch error
(an empty grid is one), so every function here asserts ON THE HOST, from CPU copies of its arguments, that nothing the kernel will
index can leave its buffer — before it launches.  An argument that fails raises AssertionError and nothing runs.  Tests give these
functions well-formed inputs only; hostile inputs belong to the product's own suites.

Every call is bracketed by torch.cuda.synchronize(): the voxel query and the scatter launch on the null stream.  Outputs are
allocated as the reference's Python (ops/vsa/group_points.py, sample_points.py) and C++ (scatter_points_cuda.cu) allocate them.
Only tests/ import this module; nothing under mmdet3d-gaussian_amd/ may.
"""
import ctypes
import importlib.util

import numpy as np
import torch

from . import ref_vsa_path, ref_vox_path

VSA_ENTRIES = ('ref_vsa_ball_query', 'ref_vsa_group_points', 'ref_vsa_group_points_grad', 'ref_vsa_furthest_point_sampling',
               'ref_vsa_fps_block', 'ref_vsa_voxel_query')
VOX_ENTRIES = ('dynamic_point_to_voxel_scatter_index', 'dynamic_point_to_voxel_scatter_reduce', 'dynamic_point_to_voxel_backward')
INT_MAX = 2 ** 31 - 1

_vsa = None
_vox = None


def load_vsa():
    """ctypes handle of oracle/_ref/ref_vsa.so with every entry typed; None if the file is absent or does not load."""
    global _vsa
    if _vsa is None:
        path = ref_vsa_path()
        if not path:
            return None
        try:
            L = ctypes.CDLL(path)
            i, f, vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
            L.ref_vsa_ball_query.argtypes = [f, i, i, i, vp, vp, vp, vp, vp, vp]
            L.ref_vsa_group_points.argtypes = [vp, vp, vp, vp, i, i, i, i, i, vp, vp]
            L.ref_vsa_group_points_grad.argtypes = [vp, vp, vp, vp, i, i, i, i, i, vp, vp]
            L.ref_vsa_furthest_point_sampling.argtypes = [vp, vp, vp, i, i, i, vp]
            L.ref_vsa_fps_block.argtypes = [i]
            L.ref_vsa_voxel_query.argtypes = [i, i, i, i, i, f, i, i, i, vp, vp, vp, vp, vp]
            for name in VSA_ENTRIES:
                getattr(L, name).restype = i
        except (OSError, AttributeError):
            return None
        _vsa = L
    return _vsa


def load_vox():
    """oracle/_ref/ref_vox*.so imported as a module; None if it is absent or does not load against this torch."""
    global _vox
    if _vox is None:
        path = ref_vox_path()
        if not path:
            return None
        try:
            spec = importlib.util.spec_from_file_location('ref_vox', path)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            for name in VOX_ENTRIES:
                getattr(mod, name)
        except (ImportError, OSError, AttributeError, RuntimeError):
            return None
        _vox = mod
    return _vox


# ---------------------------------------------------------------- host-side validation

def _host(t):
    return t.detach().cpu().numpy()


def _dev(t, dtype, shape, what):
    """t is a contiguous device tensor of `dtype` and `shape` (None entries: any extent); floats are finite.  -> its CPU copy."""
    assert isinstance(t, torch.Tensor) and t.is_cuda, f'{what}: not a device tensor'
    assert t.dtype == dtype, f'{what}: {t.dtype}, expected {dtype}'
    assert t.is_contiguous(), f'{what}: not contiguous'
    assert t.dim() == len(shape) and all(s is None or s == e for s, e in zip(shape, t.shape)), f'{what}: shape {tuple(t.shape)}, expected {shape}'
    h = _host(t)
    if dtype == torch.float32:
        assert np.isfinite(h).all(), f'{what}: holds a value that is not finite'
    return h


def _counts(cnt, rows, b, what):
    """(b,) int32 on the device, non-negative, summing to `rows`.  -> CPU copy (int64)"""
    h = _dev(cnt, torch.int32, (b,), what).astype(np.int64)
    assert b >= 1, f'{what}: no sample'
    assert (h >= 0).all(), f'{what}: a negative count'
    assert int(h.sum()) == rows, f'{what}: sums to {int(h.sum())}, the array has {rows} rows'
    return h


def _idx_in_samples(idx_h, idx_cnt_h, feat_cnt_h, what):
    """every idx[m, s] names a row of ITS sample: 0 <= idx < n_b"""
    n_of_row = np.repeat(feat_cnt_h, idx_cnt_h)[:, None]
    assert ((idx_h >= 0) & (idx_h < n_of_row)).all(), f'{what}: an index outside its sample'


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bracket(fn):
    torch.cuda.synchronize()
    try:
        return fn()
    finally:
        torch.cuda.synchronize()


# ---------------------------------------------------------------- ref_vsa

def ball_query(radius, nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt):
    """-> idx (M, nsample) int32 as the KERNEL leaves it on the zeros that `BallQuery.forward` allocates: an empty ball has -1 in
    slot 0 and zeros behind it.  `ball_query_fixup` is the rest of that forward."""
    L = load_vsa()
    n, m, b = xyz.size(0), new_xyz.size(0), xyz_batch_cnt.numel()
    _dev(xyz, torch.float32, (n, 3), 'xyz')
    _dev(new_xyz, torch.float32, (m, 3), 'new_xyz')
    _counts(xyz_batch_cnt, n, b, 'xyz_batch_cnt')
    _counts(new_xyz_batch_cnt, m, b, 'new_xyz_batch_cnt')
    assert m >= 1 and 1 <= nsample and m * nsample <= INT_MAX and 3 * max(n, m) <= INT_MAX
    assert np.isfinite(np.float32(radius))
    idx = new_xyz.new_zeros((m, nsample), dtype=torch.int32)
    _bracket(lambda: L.ref_vsa_ball_query(float(radius), nsample, b, m, new_xyz.data_ptr(), new_xyz_batch_cnt.data_ptr(), xyz.data_ptr(),
                                          xyz_batch_cnt.data_ptr(), idx.data_ptr(), _stream()))
    return idx


def ball_query_fixup(idx):
    """group_points.py:30-32: empty_ball_mask = idx[:, 0] == -1; idx[empty_ball_mask] = 0  -> (idx, mask), on a copy"""
    idx = idx.clone()
    mask = idx[:, 0] == -1
    idx[mask] = 0
    return idx, mask


def group_points(features, features_batch_cnt, idx, idx_batch_cnt):
    """-> (M, C, nsample) fp32.  Every idx must lie inside its own sample: a row of a sample WITHOUT points cannot be given."""
    L = load_vsa()
    n, c = features.shape
    m, nsample = idx.shape
    b = features_batch_cnt.numel()
    _dev(features, torch.float32, (n, c), 'features')
    idx_h = _dev(idx, torch.int32, (m, nsample), 'idx')
    fc = _counts(features_batch_cnt, n, b, 'features_batch_cnt')
    ic = _counts(idx_batch_cnt, m, b, 'idx_batch_cnt')
    assert m >= 1 and c >= 1 and nsample >= 1 and m * c * nsample <= INT_MAX and n * c <= INT_MAX
    _idx_in_samples(idx_h, ic, fc, 'idx')
    out = features.new_empty((m, c, nsample))
    _bracket(lambda: L.ref_vsa_group_points(features.data_ptr(), features_batch_cnt.data_ptr(), idx.data_ptr(), idx_batch_cnt.data_ptr(),
                                            b, n, c, m, nsample, out.data_ptr(), _stream()))
    return out


def group_points_grad(grad_out, idx, idx_batch_cnt, features_batch_cnt, n):
    """-> grad_features (n, C) fp32, atomically summed into zeros"""
    L = load_vsa()
    m, c, nsample = grad_out.shape
    b = features_batch_cnt.numel()
    _dev(grad_out, torch.float32, (m, c, nsample), 'grad_out')
    idx_h = _dev(idx, torch.int32, (m, nsample), 'idx')
    fc = _counts(features_batch_cnt, n, b, 'features_batch_cnt')
    ic = _counts(idx_batch_cnt, m, b, 'idx_batch_cnt')
    assert m >= 1 and c >= 1 and nsample >= 1 and m * c * nsample <= INT_MAX and n * c <= INT_MAX
    _idx_in_samples(idx_h, ic, fc, 'idx')
    grad = grad_out.new_zeros((n, c))
    _bracket(lambda: L.ref_vsa_group_points_grad(grad_out.data_ptr(), idx.data_ptr(), idx_batch_cnt.data_ptr(),
                                                 features_batch_cnt.data_ptr(), b, n, c, m, nsample, grad.data_ptr(), _stream()))
    return grad


def fps_block(n):
    """the block size the reference launches for n points: 2^floor(log2 n), at most 1024 (its own opt_n_threads)"""
    return load_vsa().ref_vsa_fps_block(int(n))


def furthest_point_sampling(xyz, npoint):
    """xyz (B, n, 3) -> (B, npoint) int32; 1 <= npoint <= n only: the reference has no rule past n"""
    L = load_vsa()
    b, n = xyz.size(0), xyz.size(1)
    _dev(xyz, torch.float32, (b, n, 3), 'xyz')
    assert b >= 1 and n >= 1 and 1 <= npoint <= n and b * n * 3 <= INT_MAX
    block = fps_block(n)
    assert 1 <= block <= min(n, 1024) and block & (block - 1) == 0, f'block size {block} for n = {n}'
    out = xyz.new_empty((b, npoint), dtype=torch.int32)
    temp = xyz.new_full((b, n), 1e10)
    _bracket(lambda: L.ref_vsa_furthest_point_sampling(xyz.data_ptr(), temp.data_ptr(), out.data_ptr(), b, n, npoint, _stream()))
    return out


def voxel_query(max_range, radius, nsample, xyz, new_xyz, new_coords, table):
    """-> idx (M, nsample) int32 GLOBAL rows, as the kernel leaves it on zeros (an empty query: -1 in slot 0).
    table (B, Z, Y, X) int32 with entries in [-1, N); new_coords (M, 4) int32 [b, z, y, x] with b in [0, B)."""
    L = load_vsa()
    n, m = xyz.size(0), new_xyz.size(0)
    _dev(xyz, torch.float32, (n, 3), 'xyz')
    _dev(new_xyz, torch.float32, (m, 3), 'new_xyz')
    nc = _dev(new_coords, torch.int32, (m, 4), 'new_coords').astype(np.int64)
    tb = _dev(table, torch.int32, (None,) * 4, 'table')
    bsz, z, y, x = table.shape
    rz, ry, rx = (int(r) for r in max_range)
    assert m >= 1 and nsample >= 1 and m * nsample <= INT_MAX and 3 * max(n, m) <= INT_MAX
    assert bsz >= 1 and min(z, y, x) >= 1 and bsz * z * y * x <= INT_MAX
    assert min(rz, ry, rx) >= 0 and max(rz, ry, rx) <= 64
    assert ((tb >= -1) & (tb < n)).all(), 'table: an entry outside [-1, N)'
    assert ((nc[:, 0] >= 0) & (nc[:, 0] < bsz)).all(), 'new_coords: a batch index outside [0, B)'
    assert (np.abs(nc[:, 1:]) < 2 ** 20).all(), 'new_coords: a cell far outside any grid'
    assert np.isfinite(np.float32(radius))
    idx = new_xyz.new_zeros((m, nsample), dtype=torch.int32)
    _bracket(lambda: L.ref_vsa_voxel_query(m, z, y, x, nsample, float(radius), rz, ry, rx, new_xyz.data_ptr(), xyz.data_ptr(),
                                           new_coords.data_ptr(), table.data_ptr(), idx.data_ptr()))
    return idx


# ---------------------------------------------------------------- ref_vox

def scatter_index(coors):
    """coors (N, ndim) int32 on the device -> (voxel_coors, point2voxel_map int32, voxel_points_count int32)"""
    mod = load_vox()
    _dev(coors, torch.int32, (None, None), 'coors')
    assert coors.size(0) >= 1 and coors.size(1) >= 1
    return _bracket(lambda: tuple(mod.dynamic_point_to_voxel_scatter_index(coors)))


def _check_map(point2voxel_map, voxel_points_count, n):
    pm = _dev(point2voxel_map, torch.int32, (n,), 'point2voxel_map').astype(np.int64)
    v = voxel_points_count.numel()
    cnt = _dev(voxel_points_count, torch.int32, (v,), 'voxel_points_count').astype(np.int64)
    assert v >= 1 and ((pm >= -1) & (pm < v)).all(), 'point2voxel_map: an entry outside [-1, V)'
    assert (np.bincount(pm[pm >= 0], minlength=v) == cnt).all() and (cnt >= 1).all(), 'voxel_points_count: not the counts of the map'
    return pm, cnt, v


def scatter_reduce(feats, point2voxel_map, voxel_points_count, reduce_type):
    """-> (V, C) fp32, filled and reduced as scatter_points_cuda.cu:181-217 does"""
    mod = load_vox()
    n, c = feats.shape
    _dev(feats, torch.float32, (n, c), 'feats')
    assert n >= 1 and c >= 1 and n * c <= INT_MAX and reduce_type in ('sum', 'mean', 'max')
    _check_map(point2voxel_map, voxel_points_count, n)
    return _bracket(lambda: mod.dynamic_point_to_voxel_scatter_reduce(feats, point2voxel_map, voxel_points_count, reduce_type))


def scatter_backward(grad_voxel_feats, feats, voxel_feats, point2voxel_map, voxel_points_count, reduce_type):
    """-> grad_feats (N, C) fp32 (zeros_like(feats) handed to the C++, as `_scatter_reduce.backward` does).  For 'max' the kernel
    writes through an index that stays N unless some point EQUALS the reduced value, so `voxel_feats` must be exactly the maxima."""
    mod = load_vox()
    n, c = feats.shape
    f = _dev(feats, torch.float32, (n, c), 'feats')
    assert n >= 1 and c >= 1 and n * c <= INT_MAX and reduce_type in ('sum', 'mean', 'max')
    pm, _, v = _check_map(point2voxel_map, voxel_points_count, n)
    _dev(grad_voxel_feats, torch.float32, (v, c), 'grad_voxel_feats')
    red = _dev(voxel_feats, torch.float32, (v, c), 'voxel_feats')
    if reduce_type == 'max':
        top = np.full((v, c), -np.inf, np.float32)
        np.maximum.at(top, pm[pm >= 0], f[pm >= 0])
        assert (top == red).all(), 'voxel_feats: not the maxima of feats (the trace-back would write out of bounds)'
    grad = torch.zeros_like(feats)
    _bracket(lambda: mod.dynamic_point_to_voxel_backward(grad, grad_voxel_feats, feats, voxel_feats, point2voxel_map, voxel_points_count,
                                                         reduce_type))
    return grad
