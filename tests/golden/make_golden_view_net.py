#!/usr/bin/env python3
"""Recorded results of the reference's own multi-view voxelization and view-map sampling, FROM THE REAL REFERENCE (build container only):
    python3 -B tests/golden/make_golden_view_net.py

Executes mmdet3d_gaussian/models/detectors/pillar_od.py (`to_cylindrical`, `to_spherical`, `voxelize_view`) and
mmdet3d_gaussian/models/voxel_encoders/pillar_mvf_encoder.py (`SingleViewNet.forward`) from where they lie and writes
tests/golden/view_net.npz (data only: inputs, settings, outputs).  Absent third-party symbols are stubbed:
  * mmdet / mmdet3d / mmcv imports (registries, `force_fp32`, `auto_fp16`, `multi_apply`, `BasicBlock`, builders) and `.detectors_rev`:
    no-ops / empty base classes;
  * `mmdet3d.ops.voxel.voxelize.Voxelization`: the numpy dynamic voxelizer — floor((p - lo) / vs) in the points' dtype, [z, y, x], a
    row of -1 for a point outside the grid;
  * `...ops.Scatter`: a CPU stand-in — voxels are the sorted unique non-negative rows, reduce('max') is a differentiable amax;
  * `mmdet3d.models.middle_encoders.PointPillarsScatter`: its published text restated;
  * `SingleViewNet.pointnet` and `forward_view`: identity (the scatter, the grid and the sampling loop are what is recorded).
Every case is run in fp32 and again in fp64 (inputs converted from the same fp32 values).  The points keep at least MARGIN from every
cell face of their view, asserted in fp64, so the recorded cells do not depend on the last bits of a transform.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_loader import REF_ROOT  # noqa: E402

MARGIN = 1e-5


class Voxelization(torch.nn.Module):
    """numpy dynamic voxelizer (see the module docstring)"""

    def __init__(self, voxel_size, point_cloud_range, max_num_points=-1, max_voxels=-1):
        super().__init__()
        self.vs, self.rng = np.array(voxel_size, np.float64), np.array(point_cloud_range, np.float64)
        self.grid = np.round((self.rng[3:] - self.rng[:3]) / self.vs).astype(np.int64)

    def forward(self, points):
        p = points[:, :3].numpy()
        cell = np.floor((p - self.rng[:3].astype(p.dtype)) / self.vs.astype(p.dtype))
        inside = ((cell >= 0) & (cell < self.grid)).all(1)
        zyx = cell[:, ::-1].astype(np.int64)
        zyx[~inside] = -1
        return torch.from_numpy(zyx.astype(np.int32))


class Scatter:
    """CPU stand-in of the reference's ops.Scatter (see the module docstring)"""

    def __init__(self, coors):
        self.pts_coors = coors
        keep = (coors >= 0).all(-1)
        rows, inv = torch.unique(coors[keep], dim=0, return_inverse=True)
        self.voxel_coors, self.keep, self.inv = rows, keep, inv
        self.batch_size = int(coors[:, 0].max()) + 1

    def reduce(self, pts_feats, reduce_op):
        assert reduce_op == 'max'
        out = pts_feats.new_zeros((self.voxel_coors.size(0), pts_feats.size(1)))
        idx = self.inv.unsqueeze(-1).expand(-1, pts_feats.size(1))
        return out.scatter_reduce(0, idx, pts_feats[self.keep], 'amax', include_self=False), self.voxel_coors


class PointPillarsScatter(torch.nn.Module):
    """mmdet3d's module, `forward_batch` restated from its published text"""

    def __init__(self, in_channels, output_shape):
        super().__init__()
        self.ny, self.nx, self.in_channels = output_shape[0], output_shape[1], in_channels

    def forward(self, voxel_features, coors, batch_size):
        batch_canvas = []
        for batch_itt in range(batch_size):
            canvas = torch.zeros(self.in_channels, self.nx * self.ny, dtype=voxel_features.dtype, device=voxel_features.device)
            batch_mask = coors[:, 0] == batch_itt
            this_coors = coors[batch_mask, :]
            indices = this_coors[:, 2] * self.nx + this_coors[:, 3]
            indices = indices.type(torch.long)
            voxels = voxel_features[batch_mask, :]
            voxels = voxels.t()
            canvas[:, indices] = voxels
            batch_canvas.append(canvas)
        batch_canvas = torch.stack(batch_canvas, 0)
        return batch_canvas.view(batch_size, self.in_channels, self.ny, self.nx)


def load_reference():
    sys.dont_write_bytecode = True
    for name in ('mmdet', 'mmdet.models', 'mmdet.core', 'mmdet.models.backbones', 'mmdet.models.backbones.resnet', 'mmdet3d', 'mmdet3d.ops',
                 'mmdet3d.ops.voxel', 'mmdet3d.ops.voxel.voxelize', 'mmdet3d.models', 'mmdet3d.models.builder', 'mmdet3d.models.middle_encoders',
                 'mmdet3d.models.voxel_encoders', 'mmdet3d.models.voxel_encoders.utils', 'mmcv', 'mmcv.cnn', 'mmcv.runner'):
        sys.modules.setdefault(name, types.ModuleType(name))

    class _Reg:
        def register_module(self, *a, **k):
            return lambda c: c
    passthrough = lambda *a, **k: (lambda fn: fn)
    sys.modules['mmdet.models'].DETECTORS = _Reg()
    sys.modules['mmdet.core'].multi_apply = lambda fn, *args, **kw: tuple(map(list, zip(*[fn(*a, **kw) for a in zip(*args)])))
    sys.modules['mmdet.models.backbones.resnet'].BasicBlock = torch.nn.Identity
    sys.modules['mmdet3d.ops.voxel.voxelize'].Voxelization = Voxelization
    sys.modules['mmdet3d.models.builder'].VOXEL_ENCODERS = _Reg()
    sys.modules['mmdet3d.models.middle_encoders'].PointPillarsScatter = PointPillarsScatter
    sys.modules['mmdet3d.models.voxel_encoders.utils'].__all__ = []
    sys.modules['mmcv.cnn'].build_norm_layer = lambda cfg, n: ('bn', torch.nn.Identity())
    sys.modules['mmcv.cnn'].build_upsample_layer = lambda *a, **k: torch.nn.Identity()
    sys.modules['mmcv.runner'].force_fp32 = passthrough
    sys.modules['mmcv.runner'].auto_fp16 = passthrough
    base = os.path.join(REF_ROOT, 'mmdet3d_gaussian')
    for name, path in (('_refvn', base), ('_refvn.models', os.path.join(base, 'models')),
                       ('_refvn.models.detectors', os.path.join(base, 'models', 'detectors')),
                       ('_refvn.models.voxel_encoders', os.path.join(base, 'models', 'voxel_encoders'))):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    ops = types.ModuleType('_refvn.ops')
    ops.Scatter = Scatter
    sys.modules['_refvn.ops'] = ops
    rev = types.ModuleType('_refvn.models.detectors.detectors_rev')
    rev.CenterPointRev = type('CenterPointRev', (), {})
    rev.VoxelNetRev = type('VoxelNetRev', (), {})
    sys.modules[rev.__name__] = rev
    mods = {}
    for sub, leaf in (('detectors', 'pillar_od'), ('voxel_encoders', 'utils'), ('voxel_encoders', 'pillar_mvf_encoder')):
        name = f'_refvn.models.{sub}.{leaf}'
        spec = importlib.util.spec_from_file_location(name, os.path.join(base, 'models', sub, leaf + '.py'))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mods[leaf] = mod
    return mods['pillar_od'], mods['pillar_mvf_encoder']


def view_coords64(view, xyz):
    x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
    if view == 'cartesian':
        return np.stack([x, y, z], 1)
    if view == 'cylindrical':
        return np.stack([np.arctan2(y, x), z, np.hypot(x, y)], 1)
    rho = np.sqrt(x * x + y * y + z * z)
    return np.stack([np.arctan2(y, x), np.arcsin(z / rho), rho], 1)


def clear_of_faces(views, voxel_sizes, ranges, xyz):
    """rows whose coordinates keep MARGIN from every cell face of every view, in fp64"""
    ok = np.ones(len(xyz), bool)
    for view, vs, rng in zip(views, voxel_sizes, ranges):
        u = (view_coords64(view, xyz) - np.array(rng[:3])) / np.array(vs)
        ok &= (np.abs(u - np.round(u)) * np.array(vs) >= MARGIN).all(1)
    return ok


def run_case(od, mvf, name, c, rng, out):
    views, sizes, ranges = c['views'], c['voxel_sizes'], c['ranges']
    samples = []
    for n in c['counts']:
        xyz = np.empty((0, 3), np.float32)
        while len(xyz) < n:
            cand = (np.array(c['lo'], np.float32) + rng.random((4 * n + 8, 3), dtype=np.float32) * np.array(c['span'], np.float32)).astype(np.float32)
            xyz = np.concatenate([xyz, cand[clear_of_faces(views, sizes, ranges, cand)]])[:n]
        samples.append(np.concatenate([xyz, rng.random((n, c['C'] - 3), dtype=np.float32)], 1))
    stacked = np.concatenate(samples)
    assert clear_of_faces(views, sizes, ranges, stacked[:, :3]).all()
    out[f'{name}.points'], out[f'{name}.counts'] = stacked, np.array(c['counts'], np.int32)
    out[f'{name}.views'] = np.array(views)
    out[f'{name}.voxel_sizes'], out[f'{name}.ranges'] = np.array(sizes, np.float64), np.array(ranges, np.float64)
    feats = rng.integers(-8, 9, (len(stacked), c['feat'])).astype(np.float32) / 4       # small multiples of 1/4: the max is exact
    grad_out = rng.standard_normal((len(stacked), c['feat'])).astype(np.float32)
    out[f'{name}.features'], out[f'{name}.grad_out'] = feats, grad_out
    k = c['sample_view']
    for dtype, tag in ((torch.float32, '32'), (torch.float64, '64')):
        torch.set_default_dtype(dtype)
        det = od.PillarODCenterPoint.__new__(od.PillarODCenterPoint)
        pts = [torch.from_numpy(s).to(dtype) for s in samples]
        for i, (view, vs, r) in enumerate(zip(views, sizes, ranges)):
            vpts, vcoors = det.voxelize_view(view, Voxelization(vs, r), pts)
            out[f'{name}.view{i}.points{tag}'], out[f'{name}.view{i}.coors{tag}'] = vpts.numpy(), vcoors.numpy()
            if i == k:
                net = mvf.SingleViewNet.__new__(mvf.SingleViewNet)
                torch.nn.Module.__init__(net)
                net.pointnet = torch.nn.Identity()
                net.pcrange, net.vs, net.feat_channels, net.reduce_op = list(r), list(vs), c['feat'], 'max'
                H, W = c['map']
                net.pillar_scatter = PointPillarsScatter(c['feat'], (H, W))
                seen = {}

                def forward_view(x):
                    x.retain_grad()
                    seen['x'] = x
                    return x
                net.forward_view = forward_view
                f = torch.from_numpy(feats).to(dtype).requires_grad_(True)
                res = net(vpts[:, :3], f, Scatter(vcoors.long()))
                res.backward(torch.from_numpy(grad_out).to(dtype))
                out[f'{name}.sample.map{tag}'], out[f'{name}.sample.out{tag}'] = seen['x'].detach().numpy(), res.detach().numpy()
                out[f'{name}.sample.grad_map{tag}'] = seen['x'].grad.numpy()
                out[f'{name}.sample.view'], out[f'{name}.sample.shape'] = np.int64(i), np.array([H, W], np.int64)
    torch.set_default_dtype(torch.float32)
    assert (out[f'{name}.sample.map32'].astype(np.float64) == out.pop(f'{name}.sample.map64')).all()      # the max is exact: one copy is kept
    for i in range(len(views)):
        assert (out[f'{name}.view{i}.coors32'] == out[f'{name}.view{i}.coors64']).all(), 'the margin keeps fp32 and fp64 in one cell'
        kept = int((out[f'{name}.view{i}.coors32'] >= 0).all(1).sum())
        print(name, views[i], 'kept', kept, 'of', len(stacked))
        assert 0 < kept < len(stacked)


def main():
    torch.set_num_threads(1)
    od, mvf = load_reference()
    rng = np.random.default_rng(20261019)
    out = {}
    cases = {
        # the shipped cylindrical geometry (voxel 0.0025 rad x 0.04 m x 100 m) on a cropped range: a 30 x 40 map
        'cyl': dict(views=['cartesian', 'cylindrical', 'spherical'], counts=[150, 0, 110], C=4, feat=3, sample_view=1, map=(30, 40),
                    voxel_sizes=[(0.16, 0.16, 4.0), (0.0025, 0.04, 100.0), (0.0025, 0.005, 100.0)],
                    ranges=[(0.0, -1.28, -3.0, 40.96, 1.28, 1.0), (-0.05, -1.0, 0.0, 0.05, 0.2, 100.0), (-0.05, -0.06, 0.0, 0.05, 0.02, 100.0)],
                    lo=(2.0, -1.5, -1.2), span=(38.0, 3.0, 1.6)),
        # a cartesian geometry of exactly representable cell sizes: a 16 x 32 map
        'cart': dict(views=['cartesian'], counts=[120, 90], C=5, feat=3, sample_view=0, map=(16, 32), voxel_sizes=[(0.25, 0.5, 4.0)],
                     ranges=[(0.0, -4.0, -3.0, 8.0, 4.0, 1.0)], lo=(-0.5, -4.5, -3.5), span=(9.0, 9.0, 5.0)),
    }
    for name, c in cases.items():
        run_case(od, mvf, name, c, rng, out)
    path = os.path.join(HERE, 'view_net.npz')
    np.savez_compressed(path, **out)
    print('view_net.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
