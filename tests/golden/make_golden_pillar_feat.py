#!/usr/bin/env python3
"""Recorded results of the reference's own pillar decoration, FROM THE REAL REFERENCE (build container only):
    python3 -B tests/golden/make_golden_pillar_feat.py

Executes mmdet3d_gaussian/models/voxel_encoders/{utils,pillar_encoder}.py from where they lie — `PointVoxelStatsCalculator.forward`
and `PillarFeatureNet.forward` — and writes tests/golden/pillar_feat.npz (data only: inputs, settings, outputs).  Absent third-party
symbols are stubbed:
  * mmdet3d / mmcv imports (registries, `build_norm_layer`, `force_fp32`, `auto_fp16`): no-ops;
  * `...ops.Scatter`: a CPU stand-in — voxels are the sorted unique non-negative rows, a reduce adds the voxel's points in ascending
    point index in sequence in the run's dtype and divides once, `mapback` gathers with a default for dropped points;
  * `PFNLayer`: identity (the decoration is what is recorded);
  * `get_paddings_indicator`: restated (num_points > arange(P)).
Every case is run in fp32 and again with the default dtype set to float64 (inputs converted from the same fp32 values).
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


class Scatter:
    """CPU stand-in of the reference's ops.Scatter (see the module docstring)"""

    def __init__(self, coors):
        self._coors = coors
        keep = (coors >= 0).all(-1)
        rows, inv = torch.unique(coors[keep], dim=0, return_inverse=True)         # sorted unique rows
        self.voxel_coors = rows
        self.pts_voxel_maps = torch.full((coors.size(0),), -1, dtype=torch.int32)
        self.pts_voxel_maps[keep] = inv.to(torch.int32)
        self.voxel_pts_counts = torch.bincount(inv, minlength=rows.size(0)).to(torch.int32)

    @property
    def pts_coors(self):
        return self._coors

    def reduce(self, pts_feats, reduce_op):
        assert reduce_op == 'mean'
        out = torch.zeros((self.voxel_coors.size(0), pts_feats.size(1)), dtype=pts_feats.dtype)
        for i, m in enumerate(self.pts_voxel_maps.tolist()):                        # ascending point index, in sequence
            if m >= 0:
                out[m] = out[m] + pts_feats[i]
        return out / self.voxel_pts_counts.to(pts_feats.dtype).unsqueeze(-1), self.voxel_coors

    def mapback(self, voxel_feats, default_feat=0):
        idx = self.pts_voxel_maps.long()
        rows = voxel_feats[idx.clamp(min=0)]
        return torch.where((idx >= 0).unsqueeze(-1), rows, rows.new_full((), default_feat))

    def reduce_mapback(self, pts_feats, reduce_op, default_feat=0):
        return self.mapback(self.reduce(pts_feats, reduce_op)[0], default_feat)


def _paddings_indicator(actual_num, max_num, axis=0):
    actual_num = torch.unsqueeze(actual_num, axis + 1)
    shape = [1] * actual_num.dim()
    shape[axis + 1] = -1
    return actual_num.int() > torch.arange(max_num, dtype=torch.int).view(shape)


class _PFNLayer(torch.nn.Module):
    def __init__(self, *a, **k):
        super().__init__()

    def forward(self, features, num_points=None):
        return features


def load_reference():
    sys.dont_write_bytecode = True
    for name in ('mmdet3d', 'mmdet3d.models', 'mmdet3d.models.voxel_encoders', 'mmdet3d.models.voxel_encoders.utils', 'mmdet3d.models.builder',
                 'mmcv', 'mmcv.cnn', 'mmcv.runner'):
        sys.modules.setdefault(name, types.ModuleType(name))

    class _Reg:
        def register_module(self, *a, **k):
            return lambda c: c
    passthrough = lambda *a, **k: (lambda fn: fn)
    sys.modules['mmdet3d.models.builder'].VOXEL_ENCODERS = _Reg()
    sys.modules['mmcv.cnn'].build_norm_layer = lambda cfg, n: ('bn', torch.nn.Identity())
    sys.modules['mmcv.runner'].force_fp32 = passthrough
    sys.modules['mmcv.runner'].auto_fp16 = passthrough
    stub = sys.modules['mmdet3d.models.voxel_encoders.utils']
    stub.PFNLayer, stub.get_paddings_indicator = _PFNLayer, _paddings_indicator
    stub.__all__ = ['PFNLayer', 'get_paddings_indicator']
    base = os.path.join(REF_ROOT, 'mmdet3d_gaussian')
    for name, path in (('_refpf', base), ('_refpf.models', os.path.join(base, 'models')),
                       ('_refpf.models.voxel_encoders', os.path.join(base, 'models', 'voxel_encoders'))):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    ops = types.ModuleType('_refpf.ops')
    ops.Scatter = Scatter
    sys.modules['_refpf.ops'] = ops
    mods = {}
    for leaf in ('utils', 'pillar_encoder'):
        name = '_refpf.models.voxel_encoders.' + leaf
        spec = importlib.util.spec_from_file_location(name, os.path.join(base, 'models', 'voxel_encoders', leaf + '.py'))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mods[leaf] = mod
    return mods['utils'], mods['pillar_encoder']


def stats_inputs(rng, n, ndim, voxel_size, pcr, span, outside):
    """points bunched in a corner of the range (a few points per voxel), `outside` of them beyond it; coors by our own floor"""
    lo, vs = np.array(pcr[:3], np.float32), np.array(voxel_size, np.float32)
    xyz = (lo + rng.random((n, 3), dtype=np.float32) * np.array(span, np.float32)).astype(np.float32)
    out = rng.choice(n, outside, replace=False)
    xyz[out[: outside // 2], rng.integers(0, 3)] -= np.float32(50.0)
    xyz[out[outside // 2:]] += np.float32(500.0)
    cell = np.floor((xyz - lo) / vs).astype(np.int64)
    grid = np.round((np.array(pcr[3:], np.float32) - lo) / vs).astype(np.int64)
    inside = ((cell >= 0) & (cell < grid)).all(1)
    zyx = cell[:, ::-1].copy()
    zyx[~inside] = -1
    if ndim == 4:
        coors = np.concatenate([(np.arange(n) % 3)[:, None], zyx], 1)
        coors[~inside] = -1
        part = np.flatnonzero(inside)[:3]
        coors[part, 2] = -1                                       # partly negative rows: dropped, the centre from the row's own values
        inside[part] = False
    else:
        coors = zyx
    return xyz, coors.astype(np.int64), int((~inside).sum())


def main():
    torch.set_num_threads(1)
    utils, pillar = load_reference()
    rng = np.random.default_rng(20261019)
    out = {}
    stats = {'stats_a': dict(n=300, ndim=4, voxel_size=(0.2, 0.2, 4.0), pcr=(0.0, -40.0, -3.0, 70.4, 40.0, 1.0), span=(0.9, 0.7, 3.9), outside=21),
             'stats_b': dict(n=250, ndim=3, voxel_size=(0.16, 0.16, 0.5), pcr=(-51.2, -51.2, -5.0, 51.2, 51.2, 3.0), span=(0.5, 0.5, 0.9), outside=120)}
    for name, c in stats.items():
        xyz, coors, dropped = stats_inputs(rng, c['n'], c['ndim'], c['voxel_size'], c['pcr'], c['span'], c['outside'])
        out[f'{name}.xyz'], out[f'{name}.coors'] = xyz, coors
        out[f'{name}.voxel_size'], out[f'{name}.point_cloud_range'] = np.array(c['voxel_size'], np.float64), np.array(c['pcr'], np.float64)
        for dtype, tag in ((torch.float32, '32'), (torch.float64, '64')):
            torch.set_default_dtype(dtype)
            calc = utils.PointVoxelStatsCalculator(list(c['voxel_size']), list(c['pcr']))
            sc = Scatter(torch.from_numpy(coors))
            out[f'{name}.out{tag}'] = calc(torch.from_numpy(xyz).to(dtype), sc).numpy()
        torch.set_default_dtype(torch.float32)
        print(name, 'dropped', dropped, 'voxels', sc.voxel_coors.size(0), 'largest', int(sc.voxel_pts_counts.max()), out[f'{name}.out32'].shape)
    deco = {'deco_a': dict(V=50, P=9, C=5, voxel_size=(0.2, 0.2, 8.0), pcr=(-51.2, -51.2, -5.0, 51.2, 51.2, 3.0))}
    for name, c in deco.items():
        V, P, C = c['V'], c['P'], c['C']
        coors = np.stack([rng.integers(0, 4, V), np.zeros(V, np.int64), rng.integers(0, 512, V), rng.integers(0, 512, V)], 1).astype(np.int32)
        num = rng.integers(1, P + 1, V).astype(np.int32)
        num[:3] = (1, P, P)
        feats = np.zeros((V, P, C), np.float32)
        centre = np.array(c['pcr'][:3], np.float32) + (coors[:, :0:-1].astype(np.float32) + 0.5) * np.array(c['voxel_size'], np.float32)
        for v in range(V):
            feats[v, :num[v], :3] = centre[v] + (rng.random((num[v], 3), dtype=np.float32) - 0.5) * np.array(c['voxel_size'], np.float32)
            feats[v, :num[v], 3:] = rng.random((num[v], C - 3), dtype=np.float32)
        out[f'{name}.features'], out[f'{name}.num_points'], out[f'{name}.coors'] = feats, num, coors
        out[f'{name}.voxel_size'], out[f'{name}.point_cloud_range'] = np.array(c['voxel_size'], np.float64), np.array(c['pcr'], np.float64)
        for dtype, tag in ((torch.float32, '32'), (torch.float64, '64')):
            torch.set_default_dtype(dtype)
            net = pillar.PillarFeatureNet(in_channels=C, feat_channels=(64,), with_distance=True, with_cluster_center=True, with_voxel_center=True,
                                          voxel_size=c['voxel_size'], point_cloud_range=c['pcr'], legacy=False)
            out[f'{name}.out{tag}'] = net(torch.from_numpy(feats).to(dtype), torch.from_numpy(num), torch.from_numpy(coors)).numpy()
        torch.set_default_dtype(torch.float32)
        print(name, out[f'{name}.out32'].shape)
    path = os.path.join(HERE, 'pillar_feat.npz')
    np.savez_compressed(path, **out)
    print('pillar_feat.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
